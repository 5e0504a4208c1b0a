"""The two pieces of host plumbing the receiver banks share (spandsp_amd/csrc/bank_host.hip): the per-channel lengths of an
_rx_var call and the read-back of a call's result rows, through engine.py.  Two banks of this library are compared, bit for
bit: one takes a line in ragged ticks, or in calls that make its result blocks grow, its twin takes the same line in whole
calls.  The values themselves are pinned to the reference by the family suites.

Lines: fsk, mct, sigtone and the V.29 receivers hear lines made here on the host (the oracle's receivers report on every
one of them: checked on the CPU when the lines were chosen); the text telephones and the caller-ID receivers hear their own
family's senders, which carry a whole character or message inside the samples a test feeds."""
import functools
import os

import numpy as np
import pytest

from test_bank_core_gpu import N, WATCH

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OK, BAD_ARG, STATE = 0, -2, -5
# a ragged tick's lengths: nobody, one sample, an odd length, the full tick and four in between; all different, so that
# channels with different rotations hold different lengths in every tick
M = (0, 1, 37, 2000, 1500, 999, 903, 560)
T = sum(M)                          # 6000: past the 550 ms of tone before ANS is declared, a caller-ID message, four Baudot characters
FULL = max(M)
CALLS = (160, 1600, 160, 37)        # both blocks grow, are reused by a smaller call, take an odd length
QUIET = 160
START = {"v18": 2680}               # where CALLS begin in a line: the first Baudot character ends more than 3957 samples into its line
FAMILIES = ("fsk", "mct", "sigtone", "v18", "adsi", "v29")
PREFIX = {"fsk": "fsk", "mct": "mct", "mct6": "mct", "sigtone": "sigtone", "v18": "v18", "adsi": "adsi", "v29": "modem", "qam": "modem"}
ALWAYS_LAUNCH = ("v18", "adsi")     # the other families make no launch on an all-zero tick


def rot(c):
    return (c + c//64) % len(M)


def _bits_to_fsk(bits, spb, f_zero, f_one, n, phase):
    t = np.arange(n)
    f = np.where(bits[np.minimum((t/spb).astype(int), len(bits) - 1)] == 1, f_one, f_zero)
    return 6000.0*np.sin(2*np.pi*np.cumsum(f)/8000.0 + phase)


@functools.lru_cache(maxsize=None)
def line(name):
    """[N, T] int16, read-only: what channel c hears from sample 0 on."""
    from spandsp_amd import engine
    rng = np.random.default_rng(29)
    out = np.zeros((N, T), np.float64)
    if name == "fsk":                   # V.21 channel 2, random bits from the first sample
        for c in range(N):
            out[c] = _bits_to_fsk(rng.integers(0, 2, T//26 + 2), 8000.0/300.0, 1850.0, 1650.0, T, rng.uniform(0, 6.28))
    elif name == "mct":                 # ANS: 50 ms of silence, then 2100 Hz for the rest (a plain ANS is declared after 550 ms)
        for c in range(N):
            out[c, 400:] = 6000.0*np.sin(2*np.pi*2100.0*np.arange(T - 400)/8000.0 + rng.uniform(0, 6.28))
    elif name == "mct6":                # V.21 channel 2 carrying HDLC flags: the preamble is declared after 40 bits.  (The detector
                                        # of the preamble alone: the reference's CED-or-preamble detector runs its two halves one
                                        # after the other over a call, so what it reports depends on where the calls are cut.)
        flags = np.array([0, 1, 1, 1, 1, 1, 1, 0]*(T//200))
        for c in range(N):
            out[c] = _bits_to_fsk(flags, 8000.0/300.0, 1850.0, 1650.0, T, rng.uniform(0, 6.28))
    elif name == "sigtone":             # 2280 Hz, 600 samples on and 400 off, the first burst at 100 + c
        for c in range(N):
            tone = 6000.0*np.sin(2*np.pi*2280.0*np.arange(T)/8000.0 + rng.uniform(0, 6.28))
            out[c] = np.where(((np.arange(T) - 100 - c) % 1000 < 600) & (np.arange(T) >= 100 + c), tone, 0.0)
    elif name in ("v29", "qam"):        # the V.29 9600 line of the parity suite, a little later in every channel
        amp = np.load(os.path.join(GOLDEN, "v29_9600.npz"))["amp"].astype(np.float64)
        for c in range(N):
            out[c, c % 32:] = amp[:T - c % 32]
    elif name == "v18":
        tx = engine.V18Bank(engine.V18_MODE_WEITBRECHT_5BIT_4545, N)
        assert (tx.put([b"RY%d OK" % c for c in range(N)]) >= 0).all()
        out = tx.tx_host(T)[0]
        tx.close()
    else:                               # caller-ID: marks for a preamble, so that the message ends inside the first 1957 samples
        standards = (engine.ADSI_CLASS, engine.ADSI_CLIP, engine.ADSI_ACLIP, engine.ADSI_JCLIP)
        tx = engine.AdsiTxBank(standards, N)
        msgs = []
        for c in range(N):
            tx.set_preamble(c, 0, 40, 5, -1)
            s = standards[c % 4]
            m = engine.adsi_add_field(s, b"", 0x40 if s == engine.ADSI_JCLIP else 0x80)
            msgs.append(engine.adsi_add_field(s, m, 0x02, b"55%02d" % c))
        assert np.array_equal(tx.put_message(msgs), [len(m) for m in msgs])
        out = tx.tx_host(T)[0]
        tx.close()
    out = np.clip(np.rint(out), -32768, 32767).astype(np.int16)
    out.setflags(write=False)
    return out


def make(name, n=N):
    from spandsp_amd import engine
    if name == "fsk":
        return engine.FskBank(engine.FSK_V21CH2, n, engine.FSK_FRAME_MODE_ASYNC)
    if name in ("mct", "mct6"):
        return engine.MctBank(engine.MCT_ANS if name == "mct" else engine.MCT_FAX_PREAMBLE, n)
    if name == "sigtone":
        b = engine.SigToneRxBank(engine.SIG_TONE_2280HZ, n)
        b.set_mode(engine.SIG_TONE_RX_PASSTHROUGH)
        return b
    if name == "v18":
        return engine.V18Bank(engine.V18_MODE_WEITBRECHT_5BIT_4545, n)
    if name == "adsi":
        return engine.AdsiRxBank((engine.ADSI_CLASS, engine.ADSI_CLIP, engine.ADSI_ACLIP, engine.ADSI_JCLIP), n)
    b = engine.V29Bank(n)
    if name == "qam":
        b.qam_tap()
    return b


class Heard:
    """What a bank reported, per channel, call after call, in terms that do not depend on where the calls were cut: a
    signalling tone report carries its sample of the call, a qam report the events of the call before it."""

    def __init__(self, name, n=N):
        self.name = name
        self.all = [[] for _ in range(n)]
        self.samples = np.zeros(n, np.int64)
        self.events = np.zeros(n, np.int64)

    def call(self, bank, lens):
        """the last call's results, added to the record; lens: what each channel took"""
        name = self.name
        if name == "v18":
            last = [list(t) for t in bank.text()]
        elif name == "adsi":
            last = bank.messages()
        elif name == "sigtone":
            last = [[(int(s) + int(self.samples[c]), int(st), int(d)) for s, st, d in e] for c, e in enumerate(bank.events())]
        elif name == "qam":
            ev = bank.events()
            last = [[(int(r[0]) + int(self.events[c]),) + tuple(int(x) for x in r[1:]) for r in q] for c, q in enumerate(bank.qam_reports())]
            self.events += [len(e) for e in ev]
        else:
            last = [np.asarray(e).tolist() for e in bank.events()]
        for c, e in enumerate(last):
            self.all[c] += e
        self.samples += lens
        return last


def state(bank, c):
    s = bank.get_state(c)
    return np.concatenate([np.asarray(x).view(np.uint32) for x in s]) if isinstance(s, tuple) else np.asarray(s)


def states(bank):
    return [state(bank, c) for c in WATCH]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def rx_var(bank, rows, lens, width):
    """rows[c, :lens[c]] in a frame `width` wide; past a channel's length the frame holds what no receiver may read"""
    frames = np.full((N, width), 0x2B2B, np.int16)
    for c in range(N):
        frames[c, :lens[c]] = rows[c][:lens[c]]
    bank.rx_host_var(frames, lens)


def raw_rx_var(name, bank, frames, lens, max_samples):
    from spandsp_amd import engine
    fn = getattr(engine.lib(), "spangpu_%s_rx_var" % PREFIX[name])
    lens = np.ascontiguousarray(lens, np.int32)
    return fn(bank.h, frames.ctypes.data, engine.MEM_HOST, lens.ctypes.data, max_samples, frames.shape[1])


@pytest.mark.parametrize("name", FAMILIES)
def test_ragged_ticks_equal_whole_ticks(built, name):
    x = line(name)
    a, b = make(name), make(name)
    got, want = Heard(name), Heard(name)
    for k in range(len(M)):
        lens = np.array([M[(rot(c) + k) % len(M)] for c in range(N)], np.int32)
        assert len({int(lens[c]) for c in WATCH}) == len(WATCH)
        rx_var(a, [x[c, got.samples[c]:] for c in range(N)], lens, FULL)
        last = got.call(a, lens)
        assert all(last[c] == [] for c in np.nonzero(lens == 0)[0]), (name, k)
    assert (got.samples == T).all()
    for at, m in ((0, T//2), (T//2, T - T//2)):
        b.rx_host(x[:, at:at + m])
        want.call(b, m)
    reported = sum(1 for w in want.all if w)
    print(name, "channels with a report:", reported, "of", N, "; reports:", sum(len(w) for w in want.all))
    assert 2*reported >= N, (name, reported)
    for c in range(N):
        assert got.all[c] == want.all[c], (name, c, got.all[c][:6], want.all[c][:6])
    assert same(states(a), states(b)), name
    a.close()
    b.close()


@pytest.mark.parametrize("name", FAMILIES)
def test_edges_of_the_lengths_path(built, name):
    from spandsp_amd import engine
    x = np.array(line(name))            # (a copy: the signalling tone receivers write their frames)
    a, b = make(name), make(name)
    with pytest.raises(engine.SpanGpuError) as e:
        Heard(name).call(a, 0)
    assert e.value.code == STATE
    rc = raw_rx_var(name, a, x, np.zeros(N, np.int32), 0)
    assert rc == (OK if name == "v29" else BAD_ARG), rc
    # equal lengths are the plain call
    a.rx_host_var(x, np.full(N, T, np.int32))
    b.rx_host(x)
    first = Heard(name).call(a, T)
    assert first == Heard(name).call(b, T) and same(states(a), states(b))
    assert 2*sum(1 for f in first if f) >= N
    # a length out of range: refused, and nobody moved
    before = states(a)
    for bad in (-1, T + 1):
        for where in (0, 64, N - 1):
            lens = np.full(N, T, np.int32)
            lens[where] = bad
            assert raw_rx_var(name, a, x, lens, T) == BAD_ARG, (name, bad, where)
            assert same(before, states(a)), (name, bad, where)
    # nobody brings a sample: no launch and the read-back of the call before, or a launch that leaves empty records (and,
    # in the text telephones' words, the status of a call in which nothing happened)
    assert raw_rx_var(name, a, x, np.zeros(N, np.int32), T) == OK
    after = Heard(name).call(a, 0)
    if name in ALWAYS_LAUNCH:
        assert after == [[] for _ in range(N)], name
    else:
        assert after == first and same(before, states(a)), name
    a.close()
    b.close()


@pytest.mark.parametrize("name", ("fsk", "mct6", "sigtone", "v18", "adsi", "v29", "qam"))
def test_read_back_across_regrowth(built, name):
    x = line(name)[:, START.get(name, 0):]
    a, b = make(name), make(name)
    got, want = Heard(name), Heard(name)
    quiet = np.zeros((N, QUIET), np.int16)
    at = 0
    for m in CALLS:
        a.rx_host(x[:, at:at + m])
        got.call(a, m)
        at += m
    b.rx_host(x[:, :at])
    want.call(b, at)
    print(name, "channels with a report:", sum(1 for w in want.all if w), "of", N, "; reports:", sum(len(w) for w in want.all))
    for c in range(N):
        assert got.all[c] == want.all[c], (name, c, got.all[c][:6], want.all[c][:6])
    a.rx_host(quiet)
    b.rx_host(quiet)
    hush = got.call(a, QUIET)
    assert hush == want.call(b, QUIET), name
    if name in ("v18", "adsi"):
        assert hush == [[] for _ in range(N)], name
    assert same(states(a), states(b)), name
    a.close()
    b.close()


@pytest.mark.parametrize("name", ("fsk", "v18"))
def test_one_speaker_in_the_tail_wave(built, name):
    x = line(name)
    a, solo = make(name), make(name, 1)
    lens = np.zeros(N, np.int32)
    lens[N - 1] = T
    rx_var(a, x, lens, T)
    got = Heard(name).call(a, lens)
    solo.rx_host(x[N - 1:, :])
    want = Heard(name, 1).call(solo, T)
    assert got[N - 1] == want[0] and want[0], (name, got[N - 1][:6], want[0][:6])
    assert got[:N - 1] == [[] for _ in range(N - 1)], name
    assert np.array_equal(state(a, N - 1), state(solo, 0)), name
    a.close()
    solo.close()
