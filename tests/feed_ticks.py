"""Shared by test_feed_ticks.py (no GPU: what the oracle makes of the lines) and test_feed_ticks_gpu.py (the pipelined feeds of
csrc/feed_api.hip against it): the tick schedules, the collect patterns, the slot poisoning, the lines with their oracle results
(computed once per process), and one driver for the three feed families.

A tick schedule is a list of tick lengths, cycled.  A collect pattern says how many of the outstanding ticks are collected after
each commit.  Before a tick's samples are written, the acquired slot is filled over its whole stride with a full-scale pattern
the oracle never sees: a kernel or a conversion that reads past the tick's samples gives a mismatch."""
import functools
import os

import numpy as np

import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- schedules -------------------------------------------------------------------------------------------------------------
XFEED_MAX = 400
# echo and modem ticks: 400 at index i and a 1- or 2-sample tick at index i + d for d = 1, 2, 3, 5 and 8 (the tick that takes the
# slot of tick i in a ring of d slots): 7 -> 8, 6 -> 8, 5 -> 8, 3 -> 8 and 0 -> 8 (and 15, 14, 13, 11 -> 16)
XFEED_SCHEDULE = [400, 7, 333, 400, 160, 400, 400, 400, 1, 159, 400, 161, 400, 8, 400, 400, 2, 64, 5, 400]
XFEED_TICKS = 60
DEPTHS = (1, 2, 3, 5, 8)

TONE_MAX = 1024
TONE_BLOCK = {"dtmf": 102, "bell": 120, "r2": 133}
TONE_TICKS = 50
TONE_CHANNELS = 200
N_CH = 70                                       # echo and modem banks: two workgroups, the second ragged


def tone_schedule(kind):
    """block - 1 samples and then one: the block end falls inside the 1-sample tick, every cycle (the pad makes a cycle a whole
    number of blocks, and every channel of a bank is at the same block phase)."""
    block = TONE_BLOCK[kind]
    s = [block - 1, 1, 1024, 1024, 1, 7, 64, 160, 333]
    pad = -sum(s) % block
    return s + ([pad] if pad else [])


def cuts_of(schedule, ticks):
    return [schedule[t % len(schedule)] for t in range(ticks)]


def starts_of(cuts):
    return np.concatenate([[0], np.cumsum(cuts)]).astype(np.int64)


def slot_reuse(cuts, depth):
    """ticks t of 1 or 2 samples whose slot held a 400-sample tick the time before"""
    return [t for t in range(depth, len(cuts)) if cuts[t] <= 2 and cuts[t - depth] == XFEED_MAX]


def collect_plan(depth, ticks, seed=0):
    """How many ticks to collect after each commit (what is left is collected after the last one).  Depth 1: each at once;
    depths 2 .. 5: `depth` - 1 ticks behind; depth 8: anything from none to all that are outstanding, seeded, but never none
    while every slot is taken."""
    if depth < 8:
        return [1 if t >= depth - 1 else 0 for t in range(ticks)]
    rng = np.random.default_rng(1000*depth + seed)
    plan = []
    out = 0
    for t in range(ticks):
        out += 1
        k = int(rng.integers(1 if out == depth else 0, out + 1))
        if rng.random() < 0.5:
            k = min(k, 1 if out == depth else 0)                # mostly let them pile up: a full ring is the interesting state
        plan.append(k)
        out -= k
    return plan


# ---- poison ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g711_tables(law):
    name = "alaw" if law == 1 else "ulaw"
    dec = np.load(os.path.join(GOLDEN, "g711_decode.npz"))[name].astype(np.int16)
    enc = np.load(os.path.join(GOLDEN, "g711_encode.npz"))[name]
    return dec, enc


def encode(law, pcm):
    return g711_tables(law)[1][pcm.astype(np.int32) + 32768]


def decode(law, codes):
    return g711_tables(law)[0][codes]


def poison(buf, law):
    """Full scale over the whole slot: 32767, -32768, ... or the two G.711 codes of the largest magnitude in turn."""
    if law:
        dec = g711_tables(law)[0].astype(np.int32)
        hi, lo = int(np.argmax(dec)), int(np.argmin(dec))
    else:
        hi, lo = 32767, -32768
    buf[:, 0::2] = hi
    buf[:, 1::2] = lo


# ---- tone lines and what the oracle makes of them --------------------------------------------------------------------------------
def _tone_pairs(kind):
    if kind == "dtmf":
        return [(synth.DTMF_ROW[i >> 2], synth.DTMF_COL[i & 3]) for i in range(16)]
    fr = synth.BELL_FREQS if kind == "bell" else synth.R2_FWD
    return [(fr[i], fr[j]) for i in range(6) for j in range(i + 1, 6)]


# on / off samples: a period below 1024, so that a 1024-sample tick can hold two digits of one channel
_TONE_CADENCE = {"dtmf": dict(on=400, off=440), "bell": dict(on=500, off=340, level_db=(-20.0, -5.0), twist_db=(-4.0, 4.0), noise_db=(-55.0, -35.0)),
                 "r2": dict(on=520, off=320, level_db=(-25.0, -5.0), twist_db=(-5.0, 5.0), noise_db=(-55.0, -35.0))}


class ToneCase:
    """kind 'dtmf' / 'bell' / 'r2' (forward), law 0 / 1 / 2: the cuts, what goes into the slots (`wire`: int16, or G.711 bytes),
    what the detectors see (`pcm`), and per tick and channel the digits the oracle detector accepted in it."""

    def __init__(self, kind, law):
        from oracle import restated as orc
        self.kind, self.law = kind, law
        self.block = TONE_BLOCK[kind]
        self.cuts = cuts_of(tone_schedule(kind), TONE_TICKS)
        self.starts = starts_of(self.cuts)
        sig, _ = synth.tone_pair_channels(TONE_CHANNELS, int(self.starts[-1]), _tone_pairs(kind), seed=7100 + self.block, **_TONE_CADENCE[kind])
        if law:
            self.wire = encode(law, sig)
            self.pcm = decode(law, self.wire)
        else:
            self.wire = self.pcm = sig
        make = {"dtmf": lambda: orc.Dtmf(0), "bell": lambda: orc.BellMf(0), "r2": lambda: orc.R2Mf(True, True)}[kind]
        dets = [make() for _ in range(TONE_CHANNELS)]
        self.digits = []                        # [tick][channel] -> str
        for t, n in enumerate(self.cuts):
            a = int(self.starts[t])
            row = []
            for c, d in enumerate(dets):
                if kind == "r2":
                    d.sink.clear()
                    d.rx(self.pcm[c, a:a + n], want_blocks=False)
                    row.append("".join(chr(int(e["a"])) for e in d.sink.events() if int(e["a"])))
                else:
                    d.rx(self.pcm[c, a:a + n], want_blocks=False)
                    row.append(d.get())
            self.digits.append(row)

    def block_end_ticks(self):
        """the 1-sample ticks that hold a block end"""
        return [t for t, n in enumerate(self.cuts) if n == 1 and int(self.starts[t] + 1) % self.block == 0]


@functools.lru_cache(maxsize=None)
def tone_case(kind, law=0):
    return ToneCase(kind, law)


# ---- echo lines ------------------------------------------------------------------------------------------------------------
class EchoCase:
    """70 lines of echo_lines.make_channels over the echo / modem schedule: `wire_tx` / `wire_rx` go into the slots, the oracle
    cancellers see `tx` / `rx` (the decoded codes with a G.711 law) in the same cuts; clean[tick] = what collect() must hand out
    (encoded with a law), dets = the oracle objects after the last tick."""

    def __init__(self, taps, mode, use_hpf_tx, law):
        from oracle import restated as orc
        import echo_lines
        self.taps, self.mode, self.use_hpf_tx, self.law = taps, mode, use_hpf_tx, law
        self.cuts = cuts_of(XFEED_SCHEDULE, XFEED_TICKS)
        self.starts = starts_of(self.cuts)
        tx, rx = echo_lines.make_channels(N_CH, int(self.starts[-1]), taps, seed=5150 + taps)
        if law:
            self.wire_tx, self.wire_rx = encode(law, tx), encode(law, rx)
            tx, rx = decode(law, self.wire_tx), decode(law, self.wire_rx)
        else:
            self.wire_tx, self.wire_rx = tx, rx
        self.tx, self.rx = tx, rx
        self.dets = [orc.EchoCan(taps, mode) for _ in range(N_CH)]
        self.clean_pcm = []
        for t, n in enumerate(self.cuts):
            a = int(self.starts[t])
            self.clean_pcm.append(np.stack([d.run(tx[c, a:a + n], rx[c, a:a + n], use_hpf_tx) for c, d in enumerate(self.dets)]))
        self.clean = [encode(law, x) for x in self.clean_pcm] if law else self.clean_pcm


@functools.lru_cache(maxsize=None)
def echo_case(taps, mode, use_hpf_tx, law):
    return EchoCase(taps, mode, use_hpf_tx, law)


# ---- modem lines -----------------------------------------------------------------------------------------------------------
MODEMS = [("v29", 9600), ("v29", 4800), ("v27ter", 4800), ("v27ter", 2400), ("v17", 14400), ("v17", 7200)]
SECOND_CALL = 1000                              # samples of the second call: it is given up just after its receiver begins to train


def modem_line(name, rate):
    """The first call (the channel_signals() of the receiver's own test, cut where the run would end too early for what
    follows), 480 samples of silence, and the start of the same call again: a caller that hangs up during training, which
    brings a receiver's reports closer together than a whole call does.  (In a whole V.29 call no two reports of a channel are
    less than 440 samples apart -- carrier up to training in progress, by the oracle on a dozen seeds of these lines -- and no
    400-sample tick could hold two; with the call cut here, training in progress and carrier down fall into one.)"""
    mod = __import__("test_%s_gpu" % name)
    first = mod.channel_signals(rate, N_CH, seed=rate + 77)
    total = sum(cuts_of(XFEED_SCHEDULE, XFEED_TICKS))
    first = first[:, :total - 480 - SECOND_CALL]
    sig = np.zeros((N_CH, total), np.int16)
    sig[:, :first.shape[1]] = first
    at = first.shape[1] + 480
    sig[:, at:at + SECOND_CALL] = first[:, :SECOND_CALL]
    return sig


class ModemCase:
    """events[tick][channel] = the oracle receiver's put_bit / status calls of the tick (int8: bits 0 / 1, negative SIG_STATUS
    codes), state[channel] = (float words as bits, int words) after the last tick."""

    def __init__(self, name, rate):
        from oracle import restated as orc
        from test_oracle_pin import bits, use_golden_modem_tables
        use_golden_modem_tables()
        self.name, self.rate = name, rate
        self.cuts = cuts_of(XFEED_SCHEDULE, XFEED_TICKS)
        self.starts = starts_of(self.cuts)
        self.sig = modem_line(name, rate)
        make = {"v29": orc.V29, "v27ter": orc.V27ter, "v17": orc.V17}[name]
        self.events = [[None]*N_CH for _ in self.cuts]
        self.state = []
        for c in range(N_CH):
            o = make(rate)
            for t, n in enumerate(self.cuts):
                a = int(self.starts[t])
                o.sink.clear()
                o.rx(self.sig[c, a:a + n])
                self.events[t][c] = o.sink.events()["a"].astype(np.int8)
            f, w = o.snapshot()
            self.state.append((bits(f).copy(), w))


@functools.lru_cache(maxsize=None)
def modem_case(name, rate):
    return ModemCase(name, rate)


SHORT_SCHEDULE = [8, 1, 7, 2, 5, 8, 3, 8, 4, 6]
SHORT_TICKS = 60


class ShortModemCase:
    """A feed made for ticks of at most `max_samples` (8 or fewer) samples -- its packed rows hold a header word and a few bits a
    channel -- takes a bank over in mid call: the first `lead` ticks of modem_case() (until channel 0 has trained) go through a
    400-sample feed, then SHORT_TICKS ticks of the short schedule (cut to max_samples) through the small one.  events[tick][channel]
    and state as in ModemCase, for the short ticks, from oracle receivers fed all of it in these cuts."""

    def __init__(self, name, rate, max_samples):
        from oracle import restated as orc
        from test_oracle_pin import bits
        base = modem_case(name, rate)
        self.base, self.max_samples = base, max_samples
        self.lead = 1 + min(t for t in range(len(base.cuts)) if np.any(base.events[t][0] == -4))    # SIG_STATUS_TRAINING_SUCCEEDED
        self.origin = int(base.starts[self.lead])
        self.cuts = [min(n, max_samples) for n in cuts_of(SHORT_SCHEDULE, SHORT_TICKS)]
        self.starts = starts_of(self.cuts) + self.origin
        make = {"v29": orc.V29, "v27ter": orc.V27ter, "v17": orc.V17}[name]
        self.events = [[None]*N_CH for _ in self.cuts]
        self.state = []
        for c in range(N_CH):
            o = make(rate)
            for t in range(self.lead):
                a = int(base.starts[t])
                o.rx(base.sig[c, a:a + base.cuts[t]])
            for t, n in enumerate(self.cuts):
                a = int(self.starts[t])
                o.sink.clear()
                o.rx(base.sig[c, a:a + n])
                self.events[t][c] = o.sink.events()["a"].astype(np.int8)
            f, w = o.snapshot()
            self.state.append((bits(f).copy(), w))


@functools.lru_cache(maxsize=None)
def short_modem_case(name, rate, max_samples):
    return ShortModemCase(name, rate, max_samples)


SHORT_MODEMS = [("v29", 9600, 8), ("v27ter", 4800, 1)]


def modem_bank(engine, name, rate, n_ch=N_CH):
    return {"v29": engine.V29Bank, "v27ter": engine.V27terBank, "v17": engine.V17Bank}[name](n_ch, rate)


class closing_in_order:
    """with closing_in_order(bank) as own: feed = own(Feed(...)) ... -- whatever the body raises, the feed is destroyed before
    its bank (a feed uses its bank until then; left to the garbage collector after a failed assertion, the order is anyone's)."""

    def __init__(self, *objs):
        self.objs = list(objs)

    def __enter__(self):
        return self

    def __call__(self, obj):
        self.objs.append(obj)
        return obj

    def __exit__(self, *exc):
        for o in reversed(self.objs):
            o.close()
        return False


# ---- the three families behind one face ----------------------------------------------------------------------------------------
class ToneOps:
    """A tick comes back as the sorted (channel, digit, block) entries."""
    views = False

    def __init__(self, engine, feed, wire):
        self.engine, self.feed, self.wire, self.law = engine, feed, wire, feed.law

    def acquire(self):
        return [self.feed.slot()]

    def write(self, bufs, a, n):
        bufs[0][:, :n] = self.wire[:, a:a + n]

    def commit(self, n):
        self.feed.commit(n)

    def outstanding(self):
        return self.feed.outstanding()

    def collect(self):
        r = self.feed.collect()
        if r is None:
            return None
        return sorted(zip(r[0].tolist(), r[1].tolist(), r[2].tolist())), None, []


class EchoOps:
    """A tick comes back as a copy of its clean rows [n_ch, samples]; the view handed out is kept for the hold check."""
    views = True

    def __init__(self, engine, feed, wire_tx, wire_rx):
        self.engine, self.feed, self.wire_tx, self.wire_rx, self.law = engine, feed, wire_tx, wire_rx, feed.law

    def acquire(self):
        return list(self.feed.slots())

    def write(self, bufs, a, n):
        bufs[0][:, :n] = self.wire_tx[:, a:a + n]
        bufs[1][:, :n] = self.wire_rx[:, a:a + n]

    def commit(self, n):
        self.feed.commit(n)

    def outstanding(self):
        return self.feed.outstanding()

    def collect(self):
        r = self.feed.collect()
        if r is None:
            return None
        clean, n = r
        return clean[:, :n].copy(), n, [clean]


class ModemOps:
    """A tick comes back unpacked: a list of per-channel int8 arrays.  collect() goes to the C call itself, for the samples per
    channel it returns (engine.ModemFeed.collect() drops them)."""
    views = True
    law = 0

    def __init__(self, engine, feed, sig):
        self.engine, self.feed, self.sig = engine, feed, sig

    def acquire(self):
        return [self.feed.slot()]

    def write(self, bufs, a, n):
        bufs[0][:, :n] = self.sig[:, a:a + n]

    def commit(self, n):
        self.feed.commit(n)

    def outstanding(self):
        return self.feed.outstanding()

    def collect(self):
        import ctypes as C
        f, e = self.feed, self.engine
        if f.outstanding() <= 0:
            return None
        pk, st = C.c_void_p(), C.c_void_p()
        n = e.lib().spangpu_modem_feed_collect(f.h, C.byref(pk), C.byref(st))
        assert n > 0, (n, e.lib().spangpu_last_error())
        packed = np.frombuffer((C.c_uint32*(f.n_ch*f.wpc)).from_address(pk.value), np.uint32).reshape(f.n_ch, f.wpc)
        status = np.frombuffer((C.c_uint32*(1 + 2*f.status_cap)).from_address(st.value), np.uint32)
        assert int(status[0]) <= f.status_cap, "status list overflow"
        used = status[:1 + 2*int(status[0])]
        return e.unpack_modem_events(packed, status, f.status_cap, f.max_samples*4 + 64), n, [packed, used]


def drive(ops, cuts, plan, depth, max_samples, hold=False, edges=False, origin=0):
    """The tick loop: acquire, poison, write, commit, collect as the plan says; the rest after the last commit.  The first tick
    begins at sample `origin` of the lines.
    -> per tick (in commit order) what ops.collect() made of it, and the samples per channel collect() reported (None: the family
    does not say).
    hold: the arrays handed out for tick t are kept as they are (no copy) and must be unchanged just before the tick that takes
    tick t's slot is committed -- after depth - 1 later ticks have gone through the other slots.
    edges: every refusal of the contract on the way -- commit(0), commit(max_samples + 1), acquire and commit while every slot is
    taken, collect with nothing outstanding; none may consume a slot or disturb a tick."""
    import pytest
    err = ops.engine.SpanGpuError
    starts = starts_of(cuts) + origin
    got, said = [], []
    held = {}

    def take():
        t = len(got)
        res, n, views = ops.collect()
        got.append(res)
        said.append(n)
        if hold:
            held[t] = (views, [v.copy() for v in views])

    def check_held(t):
        if t in held:
            views, copies = held.pop(t)
            for v, c in zip(views, copies):
                assert np.array_equal(v, c), ("a collected tick changed before its slot was committed again", t)

    if edges:
        assert ops.collect() is None
    for t, n in enumerate(cuts):
        bufs = ops.acquire()
        for b in bufs:
            poison(b, ops.law)
        ops.write(bufs, int(starts[t]), n)
        if edges:
            before = ops.outstanding()
            for bad in (0, max_samples + 1, -1):
                with pytest.raises(err):
                    ops.commit(bad)
            assert ops.outstanding() == before                  # the slot is still the caller's
        check_held(t - depth)
        ops.commit(n)
        if edges and ops.outstanding() == depth:
            with pytest.raises(err):
                ops.acquire()
            with pytest.raises(err):
                ops.commit(n)
            assert ops.outstanding() == depth
        for _ in range(plan[t]):
            take()
    while len(got) < len(cuts):
        take()
    for t in sorted(held):
        check_held(t)
    assert ops.collect() is None and ops.outstanding() == 0
    return got, said
