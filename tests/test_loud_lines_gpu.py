"""The int16 receiver banks on lines at and beyond full scale (tests/loud_lines.py) against the oracle, which
tests/test_loud_lines.py holds to the reference on exactly these lines: where a float is narrowed to int16, where a sum
saturates, where an adaption step overflows -- the places a GPU and the reference's host most naturally part ways.

Everything is equality, floats as bit patterns.  Banks of 70 channels (a full wave and a ragged one; the echo canceller
37): channel c carries line c mod L rotated by 977 c samples; calls of uneven lengths, every other one with per-channel
lengths for the channels c mod 3 == 0 where the bank has such a call, so those channels fall behind the others.
"""
import ctypes

import numpy as np
import pytest

import loud_lines as ll

pytestmark = pytest.mark.gpu

N_CH = 70
SIZES = (160, 1, 7, 333, 64, 160)
MODES = (0x00, 0x40, 0xC0)


@pytest.fixture(scope="module", autouse=True)
def the_fixtures_lines(built):
    """a sample that rounds the other way on this platform shows as that, not as a kernel mismatch"""
    assert np.array_equal(ll.line_crcs(), ll.load()["line_crcs"]), "the lines generated here are not the fixture's"


def ticks(n, var):
    """(tick, frame length, per-channel lengths or None for a plain call), until the channels that take every sample whole
    have had their line"""
    pos = 0
    k = 0
    while pos < ll.N:
        m = min(SIZES[k % len(SIZES)], ll.N - pos)
        lens = None
        if var and k % 2 == 1:
            lens = np.full(n, m, np.int32)
            held = np.arange(0, n, 3)
            lens[held] = 0 if k % 8 == 7 else (7*k + 13*held) % (m + 1)
        yield k, m, lens
        pos += m
        k += 1


class Feed:
    """the rows of a bank, each channel at its own place in its line"""

    def __init__(self, *rows):
        self.rows = rows
        self.n = rows[0].shape[0]
        self.pos = np.zeros(self.n, np.int64)

    def frames(self, m, lens):
        """per set of rows: [n, m] frames (12345 past a channel's length) and the channels' own samples"""
        full = np.full(self.n, m, np.int32) if lens is None else lens
        out = []
        for r in self.rows:
            fr = np.full((self.n, m), 12345, np.int16)
            segs = []
            for c in range(self.n):
                seg = r[c, self.pos[c]:self.pos[c] + full[c]]
                assert len(seg) == full[c]
                fr[c, :full[c]] = seg
                segs.append(seg)
            out.append((fr, segs))
        self.pos += full
        return full, out


def bank_rows(family, n=N_CH):
    return ll.rows([x for _, x in ll.family_lines(family)], n)


# ---- in-band signalling tones ----------------------------------------------------------------------------------------------
def sig_oracle_call(o, seg):
    """the receiver's rewritten samples and its reports as (sample of the call, state, duration): where a call reports, it
    is run again a sample at a time from the state it started in, which says at which sample each report came"""
    saved = o.buf.copy()
    o.sink.clear()
    want = o.rx(seg)
    ev = o.sink.events()
    if not len(ev):
        return want, []
    after = o.buf.copy()
    o.buf[:] = saved
    o.sink.clear()
    at = []
    again = []
    for i in range(len(seg)):
        again.append(o.rx(seg[i:i + 1]))
        k = len(o.sink.events())
        at.extend([i]*(k - len(at)))
    assert np.array_equal(np.concatenate(again), want) and np.array_equal(o.buf, after)
    return want, [(i, int(e["a"]), int(e["c"])) for i, e in zip(at, ev)]


@pytest.mark.parametrize("tone_type", [1, 2, 3])
def test_sigtone_rx_on_loud_lines(built, tone_type):
    from oracle import restated as orc
    from spandsp_amd import engine
    feed = Feed(bank_rows("sigrx"))
    bank = engine.SigToneRxBank(tone_type, N_CH)
    orcs = []
    for c in range(N_CH):
        bank.set_mode(MODES[(c//17 + c % 17) % 3], c)                 # every line under every mode
        orcs.append(orc.SigToneRx(tone_type, MODES[(c//17 + c % 17) % 3]))
    reports = 0
    railed = 0
    for k, m, lens in ticks(N_CH, True):
        full, [(frame, segs)] = feed.frames(m, lens)
        out = bank.rx_host(frame) if lens is None else bank.rx_host_var(frame, lens)
        ev = bank.events() if full.max() > 0 else [np.zeros((0, 3), np.int32)]*N_CH
        for c, o in enumerate(orcs):
            want, want_ev = sig_oracle_call(o, segs[c])
            assert np.array_equal(out[c, :full[c]], want), (c, k, np.nonzero(out[c, :full[c]] != want)[0][:5])
            assert np.array_equal(out[c, full[c]:], frame[c, full[c]:]), (c, k)
            assert [tuple(int(v) for v in e) for e in ev[c]] == want_ev, (c, k)
            reports += len(want_ev)
            railed += ll.on_rail(want, segs[c])
        if k % 9 == 0:
            for c in range(N_CH):
                assert np.array_equal(bank.get_state(c), orcs[c].snapshot()), (c, k)
    for c in range(N_CH):
        assert np.array_equal(bank.get_state(c), orcs[c].snapshot()), c
    assert reports >= 40 and railed >= 1000, (reports, railed)


@pytest.mark.parametrize("stride", [168, 163], ids=["vector-rows", "scalar-rows"])
def test_sigtone_rx_device_rows_on_loud_lines(built, stride):
    """frames resident on the device: rows a multiple of eight samples apart (the vector row path) and not (the scalar one)"""
    from oracle import restated as orc
    from spandsp_amd import engine
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    samples = 160
    rows = bank_rows("sigrx")
    bank = engine.SigToneRxBank(3, N_CH)
    orcs = []
    for c in range(N_CH):
        bank.set_mode(MODES[(c//17 + c % 17 + 1) % 3], c)
        orcs.append(orc.SigToneRx(3, MODES[(c//17 + c % 17 + 1) % 3]))
    buf = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(buf), N_CH*stride*2) == 0
    try:
        for f in range(ll.N//samples):
            frame = np.full((N_CH, stride), 12345, np.int16)
            frame[:, :samples] = rows[:, f*samples:(f + 1)*samples]
            assert hip.hipMemcpy(buf, frame.ctypes.data, frame.nbytes, 1) == 0
            bank.rx_device(buf, samples, stride)
            bank.sync()
            out = np.zeros_like(frame)
            assert hip.hipMemcpy(out.ctypes.data, buf, out.nbytes, 2) == 0
            ev = bank.events()
            for c, o in enumerate(orcs):
                o.sink.clear()
                assert np.array_equal(out[c, :samples], o.rx(frame[c, :samples])), (c, f)
                assert [(int(s), int(d)) for _, s, d in ev[c]] == [(int(e["a"]), int(e["c"])) for e in o.sink.events()], (c, f)
            assert (out[:, samples:] == 12345).all()
    finally:
        hip.hipFree(buf)
    for c in range(N_CH):
        assert np.array_equal(bank.get_state(c), orcs[c].snapshot()), c


@pytest.mark.parametrize("tone_type", [1, 2, 3])
def test_sigtone_tx_on_loud_lines(built, tone_type):
    """full-scale media under the tones: the sum saturates; every update request answered from the channel's script"""
    from oracle import restated as orc
    from spandsp_amd import engine
    feed = Feed(bank_rows("sigtx"))
    scripts = [ll.sigtx_script(tone_type, c) for c in range(N_CH)]
    at = [0]*N_CH
    bank = engine.SigToneTxBank(tone_type, N_CH)
    orcs = [orc.SigToneTx(tone_type, scripts[c]) for c in range(N_CH)]
    first = 0x15 if tone_type == 3 else 0x11
    bank.set_modes(np.full(N_CH, first, np.int32), np.full(N_CH, 120, np.int32))
    for o in orcs:
        o.set_mode(first, 120)
    asked = [0]

    def on_request(who):
        asked[0] += len(who)
        modes, durs = [], []
        for c in who:
            mode, dur = scripts[c][at[c]] if at[c] < len(scripts[c]) else (-1, 0)
            at[c] += 1
            modes.append(mode)
            durs.append(dur)
        return np.array(modes, np.int32), np.array(durs, np.int32)

    railed = 0
    for k, m, _ in ticks(N_CH, False):
        full, [(frame, segs)] = feed.frames(m, None)
        out = bank.tx_host(frame, on_request)
        for c, o in enumerate(orcs):
            want = o.tx(segs[c])
            assert np.array_equal(out[c], want), (c, k, np.nonzero(out[c] != want)[0][:5])
            railed += ll.on_rail(want, segs[c])
        if k % 9 == 0:
            for c in range(N_CH):
                assert np.array_equal(bank.get_state(c), orcs[c].snapshot()[:5]), (c, k)
    for c in range(N_CH):
        assert np.array_equal(bank.get_state(c), orcs[c].snapshot()[:5]), c
    assert asked[0] == sum(o.requests() for o in orcs) and asked[0] > 10*N_CH
    assert railed >= 1000, railed


# ---- modem connect tones ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_callback", [True, False], ids=["callback", "latch"])
@pytest.mark.parametrize("tone_type", [1, 2, 3, 4, 7, 8, 9])
def test_connect_tones_on_loud_lines(built, tone_type, use_callback):
    from oracle import restated as orc
    from spandsp_amd import engine
    feed = Feed(bank_rows("mct"))
    bank = engine.MctBank(tone_type, N_CH, use_callback=use_callback)
    orcs = [orc.Mct(tone_type, use_callback=use_callback) for _ in range(N_CH)]
    told = 0
    latched = 0
    for k, m, lens in ticks(N_CH, True):
        full, [(frame, segs)] = feed.frames(m, lens)
        if lens is None:
            bank.rx_host(frame)
        else:
            bank.rx_host_var(frame, lens)
        ev = bank.events() if full.max() > 0 else [np.zeros((0, 2), np.int32)]*N_CH
        for c, o in enumerate(orcs):
            o.sink.clear()
            if full[c]:
                o.rx(segs[c])
            if use_callback:                          # (the latch form has no callback to compare with: `hit`, below)
                want = [(int(e["a"]), int(e["b"])) for e in o.sink.events() if e["kind"] == 1]
                assert [(int(t), int(lv)) for t, lv in ev[c]] == want, (c, k)
                told += len(want)
        if k % 9 == 0:
            for c in range(N_CH):
                assert np.array_equal(bank.get_state(c), orcs[c].snapshot()), (c, k)         # type 7: the V.21 words too
                if not use_callback:
                    hit = bank.get(c)
                    assert hit == orcs[c].get(), (c, k)
                    latched += int(hit != 0)
    for c in range(N_CH):
        assert np.array_equal(bank.get_state(c), orcs[c].snapshot()), c
    if tone_type not in (8, 9):
        assert (told if use_callback else latched) > 0


# ---- FSK -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [1, 2], ids=["one-wave", "two-waves"])
@pytest.mark.parametrize("which,mode", [(1, 1), (6, 0), (3, 0), (1, 2)])
def test_fsk_on_loud_lines(built, which, mode, waves):
    """the whole receiver in one lane and the receiver cut over two wavefronts, sync / async / framed"""
    from oracle import restated as orc
    from spandsp_amd import engine
    feed = Feed(bank_rows("fsk"))
    orcs = [orc.Fsk(which, mode) for _ in range(N_CH)]
    total = 0
    engine.tune_fsk_waves(waves)
    try:
        bank = engine.FskBank(which, N_CH, mode)
        for k, m, lens in ticks(N_CH, True):
            full, [(frame, segs)] = feed.frames(m, lens)
            if lens is None:
                bank.rx_host(frame)
            else:
                bank.rx_host_var(frame, lens)
            ev = bank.events() if full.max() > 0 else [np.zeros(0, np.int16)]*N_CH
            for c, o in enumerate(orcs):
                o.sink.clear()
                if full[c]:
                    o.rx(segs[c])
                want = np.array([e["a"] for e in o.sink.events() if e["kind"] == 3], np.int64)
                assert np.array_equal(ev[c].astype(np.int64), want), (c, k, len(ev[c]), len(want))
                total += len(want)
            if k % 9 == 0:
                for c in range(N_CH):
                    assert np.array_equal(bank.get_state(c), orcs[c].snapshot()), (c, k)
        for c in range(N_CH):
            assert np.array_equal(bank.get_state(c), orcs[c].snapshot()), c
    finally:
        engine.tune_fsk_waves(0)
    assert total > (N_CH if mode == 2 else 20*N_CH), total


# ---- echo canceller --------------------------------------------------------------------------------------------------------
ECHO_N = 37
MIXED = (0x00, 0x01, 0x06, 0x67)


@pytest.mark.parametrize("taps,mode,lanes", [(128, m, lanes) for m in (0x01, 0x67) for lanes in (0, 2, 4, 8, 16)]
                         + [(32, 0x67, 0), (512, 0x67, 0), (128, None, 0), (128, None, 4), (32, None, 2)],
                         ids=lambda v: "mixed" if v is None else str(v))
def test_echo_on_loud_lines(built, taps, mode, lanes):
    """mode None: channels hold 0x00 / 0x01 / 0x06 / 0x67 by c mod 4, which puts the bank on the kernel that reads each
    channel's mode word (no adaption; NLP + CNG without adaption among them)"""
    from oracle import restated as orc
    from spandsp_amd import engine
    from test_echo_gpu import compare_state
    pairs = ll.echo_pairs()
    feed = Feed(ll.rows([t for _, t, _ in pairs], ECHO_N), ll.rows([r for _, _, r in pairs], ECHO_N))
    modes = [MIXED[c % 4] if mode is None else mode for c in range(ECHO_N)]
    assert engine.lib().spangpu_tune_echo_lanes_per_channel(lanes) == 0
    try:
        bank = engine.EchoBank(ECHO_N, taps, modes[0])
    finally:
        engine.lib().spangpu_tune_echo_lanes_per_channel(0)
    if mode is None:
        for c in range(ECHO_N):
            bank.adaption_mode(modes[c], channel=c)
    dets = [orc.EchoCan(taps, modes[c]) for c in range(ECHO_N)]
    hpf = taps != 32
    railed = 0
    for k, m, lens in ticks(ECHO_N, True):
        full, [(tx, tx_segs), (rx, rx_segs)] = feed.frames(m, lens)
        if lens is None:
            got = bank.update_host(tx, rx, use_hpf_tx=hpf)
        else:
            got, _ = bank.update_var_host(tx, rx, lens, use_hpf_tx=np.full(ECHO_N, int(hpf), np.uint8))
        for c, d in enumerate(dets):
            if full[c]:
                want = d.run(tx_segs[c], rx_segs[c], hpf)
                assert np.array_equal(got[c, :full[c]], want), (k, c, hex(modes[c]), np.nonzero(got[c, :full[c]] != want)[0][:5])
                railed += ll.on_rail(want, rx_segs[c])
        if k % 16 == 0:
            compare_state(bank, dets, (taps, mode, lanes, k))
    compare_state(bank, dets, "final")
    snaps = [d.snapshot() for d in dets]
    # (the reach conditions proper are asserted on the reference's results in tests/test_loud_lines.py)
    big = max(int(np.abs(s["taps32"].astype(np.int64)).max()) for s in snaps)
    assert big > 50000000, big
    for c, s in enumerate(snaps):
        if modes[c] in (0x00, 0x06):
            assert not s["taps32"].any(), c
    if mode == 0x67:
        assert railed >= 50, railed
    bank.close()


# ---- tone banks ------------------------------------------------------------------------------------------------------------
_KERNELS = [(1, 1), (2, 1), (1, 2), (1, 3), (2, 3)]          # the lane mappings and kernel families tests/test_tone_gpu.py cycles
_FAMILY = {1: "general", 2: "loader", 3: "stream"}


@pytest.fixture(params=_KERNELS, ids=lambda p: "lpc%d-%s" % (p[0], _FAMILY[p[1]]))
def tone_kernel(request, built):
    from spandsp_amd import engine
    lpc, variant = request.param
    engine.tune_lanes_per_channel(lpc)
    engine.tune_tone_kernel(variant)
    yield request.param
    engine.tune_lanes_per_channel(0)
    engine.tune_tone_kernel(0)


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("kind", ["dtmf", "bell", "r2f", "r2b", "st"])
def test_tone_banks_on_loud_lines(built, tone_kernel, kind):
    """block records, and every Goertzel energy as a uint32 word; the DTMF bank with the dial-tone filter on every other
    channel"""
    from oracle import restated as orc
    from spandsp_amd import engine
    feed = Feed(bank_rows(kind))
    if kind == "dtmf":
        bank = engine.ToneBank(engine.DTMF, N_CH, trace=True)
        dets = [orc.Dtmf(0) for _ in range(N_CH)]
        for c in range(1, N_CH, 2):
            bank.set_channel_params(c, filter_dialtone=1)
            dets[c].parms(filter_dialtone=1)
        nb, total = 8, True
    elif kind == "bell":
        bank = engine.ToneBank(engine.BELL_MF, N_CH, trace=True)
        dets = [orc.BellMf(0) for _ in range(N_CH)]
        nb, total = 6, False
    elif kind == "st":
        desc = ll.st_desc(orc.SuperToneDesc)
        fac = list(desc.fac)
        bank = engine.ToneBank(engine.SUPER_TONE, N_CH, bin_fac=fac, trace=True)
        dets = [orc.SuperTone(desc) for _ in range(N_CH)]
        nb, total = len(fac), True
    else:
        bank = engine.ToneBank(engine.R2_MF, N_CH, r2_fwd=(kind == "r2f"), trace=True)
        dets = [orc.R2Mf(kind == "r2f", True) for _ in range(N_CH)]
        nb, total = 6, False
    n_blocks = 0
    hits = 0
    for k, m, lens in ticks(N_CH, True):
        full, [(frame, segs)] = feed.frames(m, lens)
        if lens is None:
            bank.rx_host(frame)
        else:
            bank.rx_host_var(frame, lens)
        want = [list(d.rx(segs[c])) if full[c] else [] for c, d in enumerate(dets)]
        blk = bank.blocks() if full.max() > 0 else np.zeros(0, engine.BLOCK_DTYPE)
        tr = bank.trace(max_blocks=m//64 + 4) if blk.size else None
        got = [[] for _ in range(N_CH)]
        for r in blk:
            got[r["channel"]].append(r)
        for c in range(N_CH):
            assert len(got[c]) == len(want[c]), (kind, c, k, len(got[c]), len(want[c]))
            for j, (r, ob) in enumerate(zip(got[c], want[c])):
                assert r["block"] == j and r["hit"] == ob["hit"] and r["code"] == ob["aux"], (kind, c, k, j, r, ob["hit"], ob["aux"])
                e = tr[j, :, c]
                assert np.array_equal(words(e[:nb]), words(ob["e"][:nb])), (kind, "energies", c, k, j)
                if total:
                    assert words(e[-1:])[0] == words([ob["total_energy"]])[0], (kind, "total", c, k, j)
                hits += int(ob["hit"] > 0 or (kind == "st" and ob["hit"] >= 0))
            n_blocks += len(want[c])
    assert n_blocks > 50*N_CH and hits > 0, (n_blocks, hits)
    for c, d in enumerate(dets):
        if kind == "dtmf":
            f, i = bank.get_state(c)
            s = d.snapshot()
            assert np.array_equal(words(f[0:8]), words(s["v2"])) and np.array_equal(words(f[8:16]), words(s["v3"])), c
            assert words(f[16:17])[0] == words([s["energy"]])[0], c
            assert np.array_equal(words(f[17:19]), words(s["z350"])) and np.array_equal(words(f[19:21]), words(s["z440"])), c
            assert (i[0], i[1], i[2], i[3]) == (s["current_sample"], s["last_hit"], s["in_digit"], s["duration"]), (c, i, s)
        elif kind == "bell":
            f, i = bank.get_state(c)
            s = d.snapshot()
            assert np.array_equal(words(f[0:6]), words(s["v2"])) and np.array_equal(words(f[6:12]), words(s["v3"])), c
            assert i[0] == s["current_sample"], c
            assert [i[1], i[2], i[3] & 0xFF, (i[3] >> 8) & 0xFF, (i[3] >> 16) & 0xFF] == list(s["hits"]), (c, i, s["hits"])
