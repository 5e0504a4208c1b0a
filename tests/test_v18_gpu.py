"""V.18 text banks on the device against live v18 objects of the real reference (tests/v18_ref.py): integer arithmetic end to
end, so every comparison is for equality -- every sample, every returned length, every printed character in the call it was
printed in, and the text layer's state words."""
import ctypes as C

import numpy as np
import pytest

import fsktx_ref
import v18_ref
from spandsp_amd import engine

pytestmark = pytest.mark.gpu

N = 70          # one full wave and a partial one
MODE_IDS = ["4545", "476", "50"]


def check_state(bank, refs, channels, where):
    for c in channels:
        w = bank.get_state(c)
        r = refs[c]
        got = (w[engine.V18_W_TX_SIGNAL_ON], w[engine.V18_W_TX_DRAINING], w[engine.V18_W_BAUDOT_TX_SHIFT], w[engine.V18_W_RX_SUPPRESSION])
        want = (r.field("tx_signal_on"), r.field("tx_draining"), r.field("baudot_tx_shift"), r.field("rx_suppression_timer"))
        assert tuple(int(x) for x in got) == want, (where, c, got, want)


def sender_plan(mode):
    rng = np.random.default_rng(1800 + mode)
    puts = {}           # tick -> [(channel, text)]
    for c in range(N):
        puts.setdefault(int(rng.integers(0, 100)), []).append((c, v18_ref.seeded_text(rng, int(rng.integers(1, 26)))))
    for k, t in enumerate((0, 100, 200, 300, 400)):     # channel 3: its ring wraps, and one message does not fit
        puts.setdefault(t, []).append((3, v18_ref.seeded_text(rng, 50)))
    puts.setdefault(5, []).append((9, b"\x00\x01\x7f"))   # nothing that has a code: the sender idles out unstarted
    return puts


@pytest.mark.parametrize("schedule", [[160], [1, 37, 160, 401]], ids=["ticks", "ragged"])
@pytest.mark.parametrize("mode", v18_ref.MODES, ids=MODE_IDS)
def test_sender_parity(built, mode, schedule):
    puts = sender_plan(mode)
    refs = [v18_ref.RefV18(mode) for _ in range(N)]
    bank = engine.V18Bank(mode, N)
    done = 0
    call = 0
    while done < 450*160:
        tick = done//160
        for t in [t for t in list(puts) if t <= tick]:
            for c, text in puts.pop(t):
                want = refs[c].put(text)
                got = bank.put([text], first=c)
                assert int(got[0]) == want, (call, c, got, want)
        n = schedule[call % len(schedule)]
        pcm, lens = bank.tx_host(n)
        for c in range(N):
            row, got = refs[c].tx(n)
            assert int(lens[c]) == got, (call, c, lens[c], got)
            full = np.zeros(n, np.int16)
            full[:got] = row[:got]
            assert np.array_equal(pcm[c], full), (call, c)
        if call % 64 == 0:
            check_state(bank, refs, range(N), call)
        done += n
        call += 1
    check_state(bank, refs, range(N), "end")
    assert not puts and sum(r.field("tx_signal_on") == 0 for r in refs) >= N//2     # shutdowns, partial calls included, were met
    bank.close()


@pytest.mark.parametrize("mode", v18_ref.MODES, ids=MODE_IDS)
def test_quirks(built, mode):
    """A put after the sender shut down is accepted and never sent; spangpu_v18_restart() lets the line speak again; a
    message that does not fit is refused whole."""
    bank = engine.V18Bank(mode, 3)
    refs = [v18_ref.RefV18(mode) for _ in range(3)]

    def both_put(text, channels=range(3)):
        for c in channels:
            want = refs[c].put(text)
            assert int(bank.put([text], first=c)[0]) == want
        return want

    def run(ticks, want_signal):
        heard = False
        for k in range(ticks):
            pcm, lens = bank.tx_host(160)
            for c in range(3):
                row, got = refs[c].tx(160)
                full = np.zeros(160, np.int16)
                full[:got] = row[:got]
                assert int(lens[c]) == got and np.array_equal(pcm[c], full), (k, c)
                heard = heard or got > 0
        assert heard == want_signal
        check_state(bank, refs, range(3), "run")

    assert both_put(b"Hi 5") == 4
    run(140, True)
    assert all(r.field("tx_signal_on") == 0 for r in refs)
    assert both_put(b"LOST") == 4           # accepted ...
    run(40, False)                          # ... and never sent
    # too long for what is left of the ring: refused whole, nothing changes
    before = [bank.get_state(c) for c in range(3)]
    assert both_put(bytes(range(32, 32 + 125))) == -1
    assert all(np.array_equal(bank.get_state(c), before[c]) for c in range(3))
    # restart: the reference's equivalent is a fresh object, which has an empty ring -- the device keeps LOST in its ring,
    # as v18_set_modem() would, so the fresh object is given both messages
    for c in range(3):
        bank.restart(c, mode)
    refs = [v18_ref.RefV18(mode) for _ in range(3)]
    for r in refs:
        assert r.put(b"LOST") == 4
    assert both_put(b"Back 2") == 6
    pcm_seen = False
    for k in range(220):
        pcm, lens = bank.tx_host(160)
        for c in range(3):
            row, got = refs[c].tx(160)
            full = np.zeros(160, np.int16)
            full[:got] = row[:got]
            assert int(lens[c]) == got and np.array_equal(pcm[c], full), (k, c)
            pcm_seen = pcm_seen or got > 0
    assert pcm_seen and all(r.field("tx_signal_on") == 0 for r in refs)
    bank.close()


# ---- receiver ---------------------------------------------------------------------------------------------------------

# fsk_rx_set_signal_cutoff(min_level = -30): the carrier detector comes on at -32.8 dBm0 -- of the signal behind its one-tap
# differencer and halving, which takes 20*log10(sin(pi*1600/8000)) = -4.6 dB off these tones.  A line below about -28.2 dBm0
# is silence to the reference (and must be to the device); the levels -31.4, -35.7 and -40 of the sweep are such lines.
CARRIER_ON_DBM0 = -30.0 + 2.5 - 5.3 + 4.6
SNRS = [None, 30.0, 15.0, 9.0, 6.0, 3.0]
_lines = {}


def impaired_lines(mode):
    """[N][samples] line signals, what was sent on each, and each channel's level in dBm0 (None: silent)"""
    if mode in _lines:
        return _lines[mode]
    from oracle import ref
    rng = np.random.default_rng(4545 + mode)
    total = 160*150
    lines = np.zeros((N, total), np.int16)
    sent = []
    levels = []
    alphabet = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ 0123456789,.?!$'"
    for c in range(N):
        text = bytes(alphabet[i] for i in rng.integers(0, len(alphabet), 10))
        clean, _ = v18_ref.send_all(mode, text)
        level = -10.0 - 30.0*(c % 8)/7.0                # -10 ... -40 dBm0; the sender makes -14
        if c == 5 or c == 6:
            level = -14.0 - 6.0*(c - 5)
        x = clean.astype(np.float64)*10.0**((level + 14.0)/20.0)
        if c == 5:
            x[9000:11000] = 0.0                         # the carrier drops in mid-character and returns
        if c == 6:
            x = x[3000:]                                # starts in mid-signal
        start = int(rng.integers(0, 160))
        y = np.zeros(total)
        m = min(len(x), total - start)
        y[start:start + m] = x[:m]
        snr = SNRS[c % len(SNRS)]
        if snr is not None:
            y += ref.awgn(1000 + c, level - snr, total).astype(np.float64)
        if c == 7:
            y[:] = 0.0
            level = None
        lines[c] = np.clip(np.rint(y), -32768, 32767).astype(np.int16)
        sent.append(text)
        levels.append(level)
    _lines[mode] = (lines, sent, levels)
    return _lines[mode]


def reference_prints(mode, lines, plan):
    """plan(tick, channel) -> ('rx', n) | ('fillin', n) | ('skip', 0); per channel the list of per-call prints"""
    out = []
    for c in range(N):
        r = v18_ref.RefV18(mode)
        pos = 0
        calls = []
        for t in range(lines.shape[1]//160):
            what, n = plan(t, c)
            n = min(n, lines.shape[1] - pos)
            if what == "rx":
                calls.append(r.rx(lines[c, pos:pos + n]) if n > 0 else b"")
                pos += n
            elif what == "fillin":
                r.fillin(n)
                pos += n
                calls.append(b"")
            else:
                calls.append(b"")
        out.append(calls)
    return out


def assert_fixture_says_something(want, sent, levels):
    heard = [c for c in range(N) if levels[c] is not None and levels[c] > CARRIER_ON_DBM0]
    assert len(heard) >= N//2
    for c in heard:
        assert b"".join(want[c]) != b"", c                   # the reference prints text on every channel it can hear
    assert any(b"".join(want[c]) != sent[c] for c in heard)    # and on at least one, not what was sent


@pytest.mark.parametrize("mode", v18_ref.MODES, ids=MODE_IDS)
def test_receiver_parity(built, mode):
    lines, sent, levels = impaired_lines(mode)
    want = reference_prints(mode, lines, lambda t, c: ("rx", 160))
    assert_fixture_says_something(want, sent, levels)
    bank = engine.V18Bank(mode, N)
    assert bank.text_capacity(160) == 160*v18_ref.BAUD_X100[mode]//(800000*7) + 2
    for t in range(lines.shape[1]//160):
        bank.rx_host(lines[:, t*160:(t + 1)*160])
        got = bank.text()
        for c in range(N):
            assert got[c] == want[c][t], (t, c, got[c], want[c][t])
    status = [int(bank.get_state(c)[engine.V18_W_RX_STATUS]) for c in (0, 7)]
    assert status[1] == 0
    bank.close()


@pytest.mark.parametrize("mode", v18_ref.MODES, ids=MODE_IDS)
def test_receiver_var_and_fillin(built, mode):
    lines, sent, levels = impaired_lines(mode)

    def plan(t, c):
        if c % 9 == 4 and t % 11 == 5:
            return ("fillin", 160)
        if c % 5 == 1 and t % 7 == 3:
            return ("skip", 0)
        if c % 5 == 2 and t % 3 == 1:
            return ("rx", 77)
        return ("rx", 160)

    want = reference_prints(mode, lines, plan)
    assert any(b"".join(w) for w in want)
    bank = engine.V18Bank(mode, N)
    pos = np.zeros(N, np.int64)
    total = lines.shape[1]
    for t in range(total//160):
        block = np.zeros((N, 160), np.int16)
        lens = np.zeros(N, np.int32)
        for c in range(N):
            what, n = plan(t, c)
            n = int(min(n, total - pos[c]))
            if what == "rx":
                block[c, :n] = lines[c, pos[c]:pos[c] + n]
                lens[c] = n
            elif what == "fillin":
                bank.fillin(c, n)
            pos[c] += n
        bank.rx_host_var(block, lens)
        if lens.max() == 0:
            continue
        got = bank.text()
        for c in range(N):
            assert got[c] == want[c][t], (t, c, got[c], want[c][t])
    bank.close()


# ---- half duplex ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["tx_rx", "rx_tx"])
@pytest.mark.parametrize("mode", v18_ref.MODES, ids=MODE_IDS)
def test_half_duplex(built, mode, order):
    """A line hears its own sender mixed with a far end: nothing is printed until 300 ms after its last pulled byte, then
    the far end's text, in the same calls as the reference."""
    far_sig, _ = v18_ref.send_all(mode, b"THE QUICK BROWN FOX 123")
    ticks = len(far_sig)//160
    n = 4
    bank = engine.V18Bank(mode, n)
    near = v18_ref.RefV18(mode)
    assert near.put(b"Hi 2") == 4 and list(bank.put([b"Hi 2"]*n)) == [4]*n
    own_ref = np.zeros(160, np.int16)
    own_dev = np.zeros((n, 160), np.int16)
    printed = []
    silent_until = None
    for t in range(ticks):
        far = far_sig[t*160:(t + 1)*160].astype(np.int32)//2
        if order == "tx_rx":
            row, got = near.tx(160)
            own_ref = np.zeros(160, np.int16)
            own_ref[:got] = row[:got]
            own_dev, lens = bank.tx_host(160)
            assert all(int(x) == got for x in lens)
        mixed_ref = np.clip(own_ref.astype(np.int32)//2 + far, -32768, 32767).astype(np.int16)
        mixed_dev = np.clip(own_dev.astype(np.int32)//2 + far[None, :], -32768, 32767).astype(np.int16)
        want = near.rx(mixed_ref)
        bank.rx_host(mixed_dev)
        got_text = bank.text()
        assert all(g == want for g in got_text), (t, got_text, want)
        if near.field("rx_suppression_timer") > 0:
            assert want == b""
            silent_until = t
        printed.append(want)
        if order == "rx_tx":
            row, got = near.tx(160)
            own_ref = np.zeros(160, np.int16)
            own_ref[:got] = row[:got]
            own_dev, lens = bank.tx_host(160)
            assert all(int(x) == got for x in lens)
        w = bank.get_state(0)
        assert int(w[engine.V18_W_RX_SUPPRESSION]) == near.field("rx_suppression_timer"), t
    assert silent_until is not None and silent_until > 20
    assert b"".join(printed[:silent_until + 1]) == b"" and len(b"".join(printed[silent_until + 1:])) >= 3
    bank.close()


# ---- sender bank -> HBM -> receiver bank ---------------------------------------------------------------------------------

def test_device_resident_loop(built):
    mode = v18_ref.MODES[0]
    n, own, ticks = 4096, 64, 100           # 2 s of signal
    rng = np.random.default_rng(18)
    alphabet = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ 0123456789,.?!"
    texts = [bytes(alphabet[i] for i in rng.integers(0, len(alphabet), int(rng.integers(1, 7)))) for _ in range(own)]
    want = []
    for c in range(own):
        s, r = v18_ref.RefV18(mode), v18_ref.RefV18(mode)
        assert s.put(texts[c]) == len(texts[c])
        calls = []
        for t in range(ticks):
            row, got = s.tx(160)
            full = np.zeros(160, np.int16)
            full[:got] = row[:got]
            calls.append(r.rx(full))
        want.append(calls)
    assert all(b"".join(w) for w in want)
    sender = engine.V18Bank(mode, n)
    receiver = engine.V18Bank(mode, n)
    res = sender.put([texts[c % own] for c in range(n)])
    assert all(int(res[c]) == len(texts[c % own]) for c in range(n))
    rows = fsktx_ref.DeviceRows(n, 160)
    rows.fill(0x55)
    for t in range(ticks):
        sender.tx_device(rows.ptr, 160, 160, rows.lens)
        sender.sync()
        receiver.rx_device(rows.ptr, 160, 160)
        got = receiver.text()
        for c in range(own):
            assert got[c] == want[c][t], (t, c, got[c], want[c][t])
        for c in range(own, n):
            assert got[c] == got[c % own], (t, c)
    rows.free()
    sender.close()
    receiver.close()


# ---- the committed fixture ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", v18_ref.MODES, ids=MODE_IDS)
def test_golden_fixture(built, mode):
    """The same answers from tests/golden/v18_weitbrecht.npz, where the live reference is not needed."""
    g = v18_ref.golden()
    m = "%04x" % mode
    text = g["text_" + m].tobytes()
    near, far = engine.V18Bank(mode, 1), engine.V18Bank(mode, 1)
    assert int(near.put([text])[0]) == len(text)
    far_text = []
    for t in range(len(g["len_" + m])):
        pcm, lens = near.tx_host(160)
        assert int(lens[0]) == int(g["len_" + m][t]) and np.array_equal(pcm[0], g["tx_" + m][t]), t
        near.rx_host(pcm)
        assert near.text()[0] == b""            # its own receiver is suppressed
        far.rx_host(pcm)
        far_text += [(t, ch) for ch in far.text()[0]]
    assert [t for t, _ in far_text] == list(g["far_at_" + m]) and bytes(ch for _, ch in far_text) == g["far_" + m].tobytes()
    near.close()
    far.close()
