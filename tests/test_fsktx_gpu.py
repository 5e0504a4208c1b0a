"""The FSK and connect tone transmitter banks on the GPU against the real reference's fsk_tx(), modem_connect_tones_tx()
and async_tx_get_bit(): every int16 sample and every returned length equal, no tolerance."""
import functools

import numpy as np
import pytest

import fsktx_ref as fr

pytestmark = pytest.mark.gpu

N = 70                      # one full wave of channels and a ragged one
FRAMES = fr.SCHEDULE*2
POISON = 0x5555


def seeds_of(n):
    s = np.array([(c*37 + 5) & 0x7FFF for c in range(n)], np.uint32)
    s[3] = 0                # the stuck register: every bit a space
    return s


@functools.lru_cache(maxsize=None)
def lfsr_reference(which):
    """Per frame, the rows of 70 reference senders: own seeds, every ninth its own power, every 17th restarted onto the
    next preset after frame 7."""
    seeds = seeds_of(N)
    refs = [fr.RefFskTx(which, seed=int(seeds[c])) for c in range(N)]
    for c in range(0, N, 9):
        refs[c].power(-20.0 - 0.25*c)
    out = []
    for k, m in enumerate(FRAMES):
        rows = np.zeros((N, m), np.int16)
        for c, r in enumerate(refs):
            rows[c], got = r.tx(m)
            assert got == m
        rows.setflags(write=False)
        out.append(rows)
        if k == 7:
            for c in range(0, N, 17):
                refs[c].restart((which + 1) % 11)
    return out


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("which", [1, 2, 3, 7])
def test_fsk_bank_lfsr_source(built, which, mem):
    """V.21 ch 2, V.23 ch 1 (baud_frac reaches 800000 exactly), V.23 ch 2 (frames without a bit boundary), Weitbrecht 45.45
    (irregular spacing).  Device rows have an odd stride (element stores), host rows go through the 16-byte path."""
    from spandsp_amd import engine
    want = lfsr_reference(which)
    bank = engine.FskTxBank(which, N, engine.FSKTX_LFSR, seeds_of(N))
    for c in range(0, N, 9):
        bank.power(c, -20.0 - 0.25*c)
    dev = fr.DeviceRows(N, 1027) if mem == "device" else None
    for k, m in enumerate(FRAMES):
        if dev:
            dev.fill(0x55)
            bank.tx_device(dev.ptr, dev.stride, m, dev.lens)
            bank.sync()
            rows = dev.rows()
            lens = dev.lengths()
            assert (rows[:, m:] == POISON).all(), k
            rows = rows[:, :m]
        else:
            rows, lens = bank.tx_host(m)
        assert (lens == m).all(), k
        bad = [c for c in range(N) if not np.array_equal(rows[c], want[k][c])]
        assert not bad, (which, k, m, bad[:5])
        if k == 7:
            for c in range(0, N, 17):
                bank.restart(c, (which + 1) % 11)
    assert len(bank.events()) == 0
    if dev:
        dev.free()
    bank.close()


@pytest.mark.parametrize("which", [1, 2])
def test_fsk_bank_queue_source_and_end_of_data(built, which):
    from spandsp_amd import engine
    qbits = 64
    rng = np.random.default_rng(77 + which)
    bank = engine.FskTxBank(which, N, engine.FSKTX_QUEUE, queue_bits=qbits)
    counts = [[0, 1, 3, 40, 100][c % 5] for c in range(N)]
    bits = [rng.integers(0, 2, k).astype(np.uint8) for k in counts]
    acc = bank.put_bits(bits)
    assert list(acc) == [min(k, qbits) for k in counts]
    feeds = [fr.BitFeed() for _ in range(N)]
    refs = [fr.RefFskTx(which, get_bit=feeds[c]) for c in range(N)]
    for c in range(N):
        feeds[c].bits = [int(b) for b in bits[c][:acc[c]]]
        assert bank.queued(c) == acc[c]
        if c % 2:
            feeds[c].end_of_data = True
            bank.end_of_data(c)
    down = set()

    def step(m):
        rows, lens = bank.tx_host(m)
        newly = []
        for c in range(N):
            seen = len(refs[c].status)
            want, got = refs[c].tx(m)
            assert lens[c] == got, (c, m, lens[c], got)
            assert np.array_equal(rows[c], want), (c, m)        # want is zero past `got`: so is the bank's row
            if len(refs[c].status) > seen:
                assert refs[c].status[seen:] == [fr.END_OF_DATA, fr.SHUTDOWN_COMPLETE]
                newly.append(c)
            if c in down:
                assert got == 0
        assert list(bank.events()) == newly, (m, newly)
        down.update(newly)

    for m in [160, 333, 77, 1024, 160, 8, 1024, 160]:
        step(m)
    assert down == set(range(1, N, 2))
    assert all(bank.queued(c) == 0 for c in range(N))
    # a restart revives a channel; its end-of-data mark is the caller's to clear
    for c in (1, 41):
        bank.restart(c, which)
        bank.end_of_data(c, False)
        refs[c].restart(which)
        feeds[c].end_of_data = False
        down.discard(c)
    more = [rng.integers(0, 2, 20).astype(np.uint8) for _ in range(N)]
    assert (bank.put_bits(more) == 20).all()
    for c in range(N):
        feeds[c].bits = [int(b) for b in more[c]]
    for m in [160, 160, 333]:
        step(m)
    bank.close()


@pytest.mark.parametrize("which,data_bits,parity,stop_bits", [(1, 8, 0, 1), (7, 5, 0, 2)])
def test_framed_senders(built, which, data_bits, parity, stop_bits):
    """put_bytes() in front of the modulator against the reference's fsk_tx() fed by its own async_tx_get_bit(); bytes
    arrive between calls, so idle marks fall between characters."""
    from spandsp_amd import engine
    n = 10
    rng = np.random.default_rng(5 + which)
    bank = engine.FskTxBank(which, n, engine.FSKTX_QUEUE)
    bank.set_framing(data_bits, parity, stop_bits)
    asyncs = [fr.RefAsyncTx(data_bits, parity, stop_bits) for _ in range(n)]
    refs = [fr.RefFskTx(which, get_bit=asyncs[c].get_bit) for c in range(n)]
    first = True
    for m, k in [(160, 2), (1024, 0), (333, 3), (2000, 1), (160, 0), (4000, 2), (5000, 0)]:
        if k:
            texts = [bytes(rng.integers(0, 256, k + (c % 2)).astype(np.uint8)) for c in range(n)]
            pre = 4 if first else 0
            acc = bank.put_bytes(texts, presend_bits=pre)
            assert list(acc) == [len(t) for t in texts]
            for c in range(n):
                if pre:
                    asyncs[c].presend(pre)
                asyncs[c].put(texts[c])
            first = False
        rows, lens = bank.tx_host(m)
        for c in range(n):
            want, got = refs[c].tx(m)
            assert lens[c] == got == m
            assert np.array_equal(rows[c], want), (c, m)
    bank.close()


def test_framed_loop_on_device(built):
    """FskTxBank -> HBM -> FskBank in framed mode, 130 channels, each its own text: the received characters are those sent."""
    from spandsp_amd import engine
    n, m = 130, 160
    rng = np.random.default_rng(9)
    texts = [bytes(rng.integers(0, 256, 6 + c % 5).astype(np.uint8)) for c in range(n)]
    tx = engine.FskTxBank(engine.FSK_V21CH2, n, engine.FSKTX_QUEUE)
    rx = engine.FskBank(engine.FSK_V21CH2, n, engine.FSK_FRAME_MODE_FRAMED)
    assert list(tx.put_bytes(texts, presend_bits=40)) == [len(t) for t in texts]
    dev = fr.DeviceRows(n, m)
    got = [[] for _ in range(n)]
    for _ in range(40 + 12*27*10//m + 10):
        tx.tx_device(dev.ptr, m, m)
        tx.sync()
        rx.rx_device(dev.ptr.value, m, m)
        for c, e in enumerate(rx.events()):
            got[c] += [int(v) for v in e if v >= 0]
    dev.free()
    assert [bytes(g) for g in got] == texts


def test_v21_preamble_loop_on_device(built):
    """HDLC flags at -15 dBm0 from the bank into the FAX preamble detector bank: the reports are those ref.MctRx makes of
    ref.fsk_tx() with the same bits."""
    from oracle import ref
    from spandsp_amd import engine
    n, m, frames = 66, 160, 80
    rng = np.random.default_rng(21)
    bits = [[0, 1, 1, 1, 1, 1, 1, 0]*(30 + c % 7) + [int(b) for b in rng.integers(0, 2, 100)] for c in range(n)]
    tx = engine.FskTxBank(engine.FSK_V21CH2, n, engine.FSKTX_QUEUE)
    rx = engine.MctBank(engine.MCT_FAX_PREAMBLE, n)
    for c in range(n):
        tx.power(c, -15.0)
    assert list(tx.put_bits(bits)) == [len(b) for b in bits]
    dev = fr.DeviceRows(n, m)
    got = [[] for _ in range(n)]
    for _ in range(frames):
        tx.tx_device(dev.ptr, m, m)
        tx.sync()
        rx.rx_device(dev.ptr.value, m, m)
        for c, e in enumerate(rx.events()):
            got[c] += [(int(t), int(lv)) for t, lv in e]
    dev.free()
    for c in range(n):
        o = ref.MctRx(engine.MCT_FAX_PREAMBLE)
        o.rx(ref.fsk_tx(1, m*frames, bits=bits[c], level_dbm0=-15.0))
        want = [(int(e["a"]), int(e["b"])) for e in o.sink.events() if e["kind"] == 1]
        assert got[c] == want and want, (c, got[c], want)


# ---- modem connect tones ----------------------------------------------------------------------------------------------
FINITE = {2: 22400, 3: 28000, 4: 41600, 5: 41600, 8: 22400}      # samples until the tone has ended
RESTARTED = [5, 28, 64, 69]


def mct_schedules(tone_type):
    if tone_type in FINITE:
        return {"frames": [160]*(FINITE[tone_type]//160 + 2),
                "ragged": FRAMES + [9000, 7001, 9000, 9000, 9000, 160, 160]}
    # 28000 = 175 x 160 (and 20800 = 130 x 160): in 160-sample frames the cadence wraps on a call's end and nothing is
    # skipped; one long call skips a sample at every wrap; the last schedule wraps inside its second and third calls
    return {"frames": [160]*190, "ragged": FRAMES + [9000, 7001, 9000, 9000], "one_call": [60000],
            "mid_call": [27000, 2000, 30000, 1001, 160, 25000, 7, 21000]}


@pytest.mark.parametrize("tone_type", [1, 2, 3, 4, 5, 8, 9])
def test_connect_tone_bank(built, tone_type):
    from spandsp_amd import engine
    for name, sched in mct_schedules(tone_type).items():
        bank = engine.MctTxBank(tone_type, N)
        plain, again = fr.RefMctTx(tone_type), fr.RefMctTx(tone_type)    # the two histories among the 70 channels
        zero_calls = 0
        for k, m in enumerate(sched):
            rows, lens = bank.tx_host(m)
            w0, g0 = plain.tx(m)
            w1, g1 = again.tx(m)
            for c in range(N):
                want, got = (w1, g1) if c in RESTARTED else (w0, g0)
                assert lens[c] == got, (name, k, c, lens[c], got)
                assert np.array_equal(rows[c], want), (name, k, c)
            zero_calls += (g0 == 0)
            if k == 3:
                for c in RESTARTED:
                    bank.restart(c)
                again.restart()
        if tone_type in FINITE:
            assert zero_calls >= 1, name            # a call after the end returned 0
        if name == "one_call":
            # the call stepped over one sample at each wrap: from there on the tone is that of a sender called in
            # 160-sample frames (which wraps on a call's end and skips nothing), one sample and then two samples late.
            # (The burst's own first sample may be 0: FAX CNG's 4000 samples of 1100 Hz are 550 whole cycles.)
            framed = fr.RefMctTx(tone_type)
            flat = np.concatenate([framed.tx(160)[0] for _ in range(60000//160)])
            period = 28000 if tone_type == 1 else 20800
            assert flat[period:period + 400].any()
            for late, i in enumerate((period, 2*period + 1), 1):
                assert w0[i] == 0 and not w0[i - 8:i].any()
                assert np.array_equal(w0[i + 1:i + 401], flat[i + 1 - late:i + 401 - late])
                assert not np.array_equal(w0[i:i + 400], flat[i:i + 400])
        bank.close()


@pytest.mark.parametrize("tone_type", [1, 3])
def test_connect_tone_loop_on_device(built, tone_type):
    """MctTxBank -> HBM -> MctBank of the same type: the reports are those ref.MctRx makes of the reference's modem_connect_tones_tx()."""
    from oracle import ref
    from spandsp_amd import engine
    n, m, frames = 66, 160, 200
    tx = engine.MctTxBank(tone_type, n)
    rx = engine.MctBank(tone_type, n)
    dev = fr.DeviceRows(n, m)
    got = [[] for _ in range(n)]
    for _ in range(frames):
        dev.fill(0)
        tx.tx_device(dev.ptr, m, m)
        tx.sync()
        rx.rx_device(dev.ptr.value, m, m)
        for c, e in enumerate(rx.events()):
            got[c] += [(int(t), int(lv)) for t, lv in e]
    dev.free()
    gen = fr.RefMctTx(tone_type)             # called with the same lengths: the cadence's wrap depends on them
    sig = np.concatenate([gen.tx(m)[0] for _ in range(frames)])
    o = ref.MctRx(tone_type)
    o.rx(sig)
    want = [(int(e["a"]), int(e["b"])) for e in o.sink.events() if e["kind"] == 1]
    assert want and all(g == want for g in got), (got[0], want)
