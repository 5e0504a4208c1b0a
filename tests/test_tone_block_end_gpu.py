"""GPU parity for the block-end piece of the streaming tone kernels' hot loop (tone_fast.hpp): the two halves of the piece that
holds a block end (pairs_head_asm / pairs_tail_asm), finish(), the plain decision with its key look-up, the record's hand-over
to the first or second record slot, and the fall-back to the general decision.  Compared as tests/test_tone_hot_loop_gpu.py
compares (its reference makers are used): records, the running block energy and every state word against oracle.restated, bit
for bit, with trace off so that the plain decision is what runs -- and once with trace on, for the Goertzel energies of every
block.  Every test of a bank runs under spangpu_tune_tone_kernel()'s three forced variants (the general kernel, the streaming kernel with
a loader wave and without); the kernel several banks share has tests of its own below.  References are made once per module."""
import ctypes as C
import zlib

import numpy as np
import pytest

import synth
import test_tone_hot_loop_gpu as hl

pytestmark = pytest.mark.gpu

_FAMILY = {1: "general", 2: "loader", 3: "stream"}


@pytest.fixture(params=[1, 2, 3], ids=lambda v: _FAMILY[v])
def tone_kernel(request, built):
    """Every test that runs a bank runs under each kernel family spangpu_tune_tone_kernel() can force, one lane per channel."""
    from spandsp_amd import engine
    engine.tune_lanes_per_channel(1)
    engine.tune_tone_kernel(request.param)
    yield request.param
    engine.tune_lanes_per_channel(0)
    engine.tune_tone_kernel(0)
    while _OPEN:
        _OPEN.pop().close()


_OPEN = []


def _bank(*args, **kwargs):
    """A ToneBank that the tone_kernel fixture closes behind the test."""
    from spandsp_amd import engine
    _OPEN.append(engine.ToneBank(*args, **kwargs))
    return _OPEN[-1]


N_BIG = 330                     # a workgroup and a partial one
N_SMALL = 70                    # one full wave and a ragged one
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _sig():
    return _cached("sig", lambda: synth.dtmf_channels(N_BIG, 160*20, seed=5201)[0])


def _some(n_ch):
    """The channels whose state is read back: all of a small bank, of a big one the edges of its waves and every seventh."""
    if n_ch <= 128:
        return list(range(n_ch))
    return sorted(set([0, 63, 64, 127, 128, 255, 256, 319, 320, n_ch - 1] + list(range(3, n_ch, 7))))


def _state_check(bank, snap, channels, what):
    for c in channels:
        f, i = bank.get_state(c)
        v2, v3, energy, cs, last_hit, in_digit, duration = snap[c]
        assert hl.same_f32(f[0:8], v2) and hl.same_f32(f[8:16], v3), (what, "v2 v3", c)
        assert hl.same_f32(f[16:17], [energy]), (what, "energy", c)
        assert (i[0], i[1], i[2], i[3]) == (cs, last_hit, in_digit, duration), (what, "ints", c, i, snap[c][3:])


# (first call, second call): the first sets the block phase, the second holds the block ends looked at
#   102 - 2k, 160: the block end 2k samples into the first piece -- behind pair k of it, k = 1 .. 15; k = 16 (a 70-sample call):
#                  on the piece's last pair; k = 0: a whole block first, the end then in the fourth piece
#   74, 160:       block ends behind samples 28 and 130: two in one call, both record slots, the second behind the FIRST pair of the
#                  frame's LAST piece
#   44, 160:       ... behind samples 58 and 160: the second on the last pair of the last piece
#   62, 152:       ... behind 40 and 142: the second in the short last piece of a 152-sample call (the general loop takes that one)
#   102, 320 and 56, 320: three block ends in one call (records past the second are stored from the block end itself)
_PHASES = [(102 - 2*k, 160) for k in range(17)] + [(74, 160), (44, 160), (62, 152), (102, 320), (56, 320)]


def _phase_reference(first, second):
    def make():
        sig = _sig()[:, :first + second]
        return hl._dtmf_reference(sig, [first, second], snaps_after=(1, 2))
    return _cached(("phase", first, second), make)


@pytest.mark.parametrize("n_ch", [N_SMALL, N_BIG])
def test_block_end_at_every_pair_of_a_piece(built, tone_kernel, n_ch):
    from spandsp_amd import engine
    sig = _sig()
    most = 0
    for first, second in _PHASES:
        ref = _phase_reference(first, second)
        bank = _bank(engine.DTMF, n_ch)
        pos = 0
        for t, n in enumerate((first, second)):
            bank.rx_host(sig[:n_ch, pos:pos + n])
            pos += n
            blk = bank.blocks()
            assert np.array_equal(hl.got_rows(blk), hl._rows(ref["ticks"][t], n_ch)), (first, second, t)
            most = max(most, int(blk["block"].max()) + 1 if blk.size else 0)
            _state_check(bank, ref["snaps"][t + 1], _some(n_ch), (first, second, t))
        bank.close()
    assert most == 3


def _digest(states):
    h = 0
    for f, i in states:
        h = zlib.crc32(np.ascontiguousarray(i, np.int32).tobytes(), zlib.crc32(np.ascontiguousarray(f, np.float32).tobytes(), h))
    return h


def _snap_as_state(s):
    v2, v3, energy, cs, last_hit, in_digit, duration = s
    return np.concatenate([v2, v3, [energy]]).astype(np.float32), np.array([cs, last_hit, in_digit, duration], np.int32)


@pytest.mark.parametrize("n_ch", [N_SMALL, N_BIG])
def test_twenty_ticks(built, tone_kernel, n_ch):
    """Twenty consecutive 160-sample ticks from rest: twenty block phases of the 51-frame cycle, one and two block ends a tick
    in turn.  Per tick the rows, and a digest over the state words of the channels read back, against the oracle's."""
    from spandsp_amd import engine
    sig = _sig()
    ref = _cached("twenty", lambda: hl._dtmf_reference(sig, [160], snaps_after=tuple(range(1, 21))))
    bank = _bank(engine.DTMF, n_ch)
    chans = _some(n_ch)
    digits = [""]*n_ch
    for t in range(20):
        bank.rx_host(sig[:n_ch, 160*t:160*(t + 1)])
        blk = bank.blocks()
        assert np.array_equal(hl.got_rows(blk), hl._rows(ref["ticks"][t], n_ch)), t
        hl._dtmf_digits(digits, blk)
        got = _digest([(f[:17], i) for f, i in (bank.get_state(c) for c in chans)])
        want = _digest([_snap_as_state(ref["snaps"][t + 1][c]) for c in chans])
        print("tick %2d: state digest %08x, oracle %08x" % (t + 1, got, want))
        if got != want:
            _state_check(bank, ref["snaps"][t + 1], chans, "tick %d" % (t + 1))     # (says which word)
        assert got == want, t
    assert digits == ref["digits"][:n_ch]
    assert sum(len(d) for d in digits) > n_ch//4


def test_goertzel_energies_of_every_block(built, tone_kernel):
    """The same twenty ticks with trace on: the general decision behind the same two halves and the same finish(), and the
    eight Goertzel energies and the block energy of every block against the oracle's."""
    from oracle import restated as orc
    from spandsp_amd import engine
    n_ch = N_SMALL
    sig = _sig()

    def make():
        dets = [orc.Dtmf(0) for _ in range(n_ch)]
        return [[d.rx(sig[c, 160*t:160*(t + 1)]) for c, d in enumerate(dets)] for t in range(20)]
    want = _cached("energies", make)
    bank = _bank(engine.DTMF, n_ch, trace=True)
    for t in range(20):
        bank.rx_host(sig[:n_ch, 160*t:160*(t + 1)])
        blk = bank.blocks()
        tr = bank.trace()
        k = 0
        for c in range(n_ch):
            for j, ob in enumerate(want[t][c]):
                r = blk[k]
                assert (r["channel"], r["block"], r["hit"], r["code"]) == (c, j, ob["hit"], ob["aux"]), (t, c, j)
                assert np.array_equal(tr[j, :8, c].view(np.uint32), ob["e"][:8].view(np.uint32)), (t, c, j)
                k += 1
        assert k == len(blk)


@pytest.mark.parametrize("poison", ["nan", "inf"])
def test_fall_back_to_the_general_decision(built, tone_kernel, poison):
    """A channel whose imported state makes one of its energies a NaN (or +infinity: then v2*v3*fac is one too and their
    difference a NaN) sends its wave to the general decision for that block.  Every other channel -- those of the same wave
    among them -- must come out as the oracle has it, and the poisoned one as the general kernel has it."""
    from spandsp_amd import engine
    n_ch = N_BIG
    sig = _sig()
    ref = _cached("twenty", lambda: hl._dtmf_reference(sig, [160], snaps_after=tuple(range(1, 21))))
    victim = 70 + 11                # in the second wave of the first workgroup
    bank = _bank(engine.DTMF, n_ch)
    engine.tune_tone_kernel(1)
    general = _bank(engine.DTMF, n_ch)
    engine.tune_tone_kernel(tone_kernel)
    for t in range(3):
        if t == 1:
            for b in (bank, general):
                f, i = b.get_state(victim)
                f[3] = np.float32(np.nan if poison == "nan" else np.inf)
                b.set_state(victim, f, i)
        frame = sig[:n_ch, 160*t:160*(t + 1)]
        bank.rx_host(frame)
        engine.tune_tone_kernel(1)
        general.rx_host(frame)
        engine.tune_tone_kernel(tone_kernel)
        blk = bank.blocks()
        assert blk.tobytes() == general.blocks().tobytes(), t
        others = blk[blk["channel"] != victim]
        want = hl._rows(ref["ticks"][t], n_ch)
        assert np.array_equal(hl.got_rows(others), want[want[:, 0] != victim]), t
        _state_check(bank, ref["snaps"][t + 1], [c for c in _some(n_ch) + list(range(64, 128)) if c != victim], (poison, t))
        fa, ia = bank.get_state(victim)
        fb, ib = general.get_state(victim)
        assert hl.same_f32(fa, fb) and np.array_equal(ia, ib), t


def test_ties_and_signed_zeros_in_the_key_look_up(built):
    """DtmfDet::decide_plain() against DtmfDet::decide() through the debug hook, on energies drawn from four values only -- the
    peak, the same value again, +0 and -0 -- in every one of the 4^8 arrangements: every pair, triple and quadruple of tones
    tied for the peak, a peak equal to its runner-up to the last bit, and groups that are all zeros of either sign (which
    compare equal, as the reference's float compares have them).  Twice: a peak that passes every test with the block energy
    given, and one that fails the threshold."""
    from spandsp_amd import engine
    L = engine.lib()
    L.spangpu_debug_decide.restype = C.c_int
    L.spangpu_debug_decide.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    n = 4**8
    idx = (np.arange(n)[:, None] >> (2*np.arange(8))) & 3
    rng = np.random.default_rng(5202)
    keys = np.frombuffer(b"\x00123A456B789C*0#D", np.uint8)
    for peak in (np.float32(4.0e9), np.float32(1.0e8)):
        vals = np.array([peak, peak, 0.0, -0.0], np.float32)
        vals[1] = peak                                  # (a second register with the same bits)
        e = np.ascontiguousarray(vals[idx])
        for scale in (0.0, 1.0e-4):
            energy = np.full(n, peak*scale, np.float32)
            w0 = ((keys[rng.integers(0, 17, n)].astype(np.uint32) << 16) | (keys[rng.integers(0, 17, n)].astype(np.uint32) << 24))
            w1 = rng.integers(0, 1000, n).astype(np.int32)
            out = np.zeros((6, n), np.uint32)
            rc = L.spangpu_debug_decide(engine.DTMF, e.ctypes.data, energy.ctypes.data, w0.ctypes.data, w1.ctypes.data, out.ctypes.data, n)
            assert rc == 0
            bad = np.nonzero((out[0] != out[3]) | (out[1] != out[4]) | (out[2] != out[5]))[0]
            assert bad.size == 0, (float(peak), scale, bad[:5], e[bad[:2]], [hex(int(x)) for x in out[:, bad[0]]])
            if peak > 1.0e9:
                assert int(((out[0] & 0xFF) != 0).sum()) > 100      # lone peaks in both groups are digits


# ---- the other detectors that share the segment loop and finish() ---------------------------------------------------
def _mf_reference(kind, sig, sizes):
    from oracle import restated as orc
    dets = [orc.BellMf(0) if kind == "bell" else orc.R2Mf(True, True) for _ in range(sig.shape[0])]
    ticks = []
    snaps = []
    for pos, n in hl.ticks_of(sig.shape[1], sizes):
        ticks.append([[(int(b["hit"]), int(b["aux"])) for b in d.rx(sig[c, pos:pos + n])] for c, d in enumerate(dets)])
        snaps.append([d.snapshot() for d in dets])
    return ticks, snaps


def _mf_state_check(bank, snap, n_ch, bell, what):
    for c in range(n_ch):
        f, i = bank.get_state(c)
        s = snap[c]
        assert hl.same_f32(f[0:6], s["v2"]) and hl.same_f32(f[6:12], s["v3"]) and i[0] == s["current_sample"], (what, c)
        if bell:
            hits = [i[1], i[2], i[3] & 0xFF, (i[3] >> 8) & 0xFF, (i[3] >> 16) & 0xFF]
            assert hits == list(s["hits"]), (what, c, i, s["hits"])


@pytest.mark.parametrize("first", [118, 104, 88])
def test_bell_mf_block_end_positions(built, tone_kernel, first):
    """120-sample blocks: after a first call of 118 / 104 / 88 samples the block ends behind the first, the eighth and the last
    pair of the next call's first piece; then four ticks more."""
    from spandsp_amd import engine
    n_ch = N_SMALL
    sizes = [first] + 5*[160]
    sig = _cached("bell-sig", lambda: synth.bell_mf_channels(n_ch, 118 + 5*160, seed=5203)[0])[:, :sum(sizes)]
    ticks, snaps = _cached(("bell", first), lambda: _mf_reference("bell", sig, sizes))
    bank = _bank(engine.BELL_MF, n_ch)
    for t, (pos, n) in enumerate(hl.ticks_of(sum(sizes), sizes)):
        bank.rx_host(sig[:, pos:pos + n])
        assert np.array_equal(hl.got_rows(bank.blocks()), hl._rows(ticks[t], n_ch)), (first, t)
        _mf_state_check(bank, snaps[t], n_ch, True, (first, t))


def test_r2_mf_odd_block_ends(built, tone_kernel):
    """133-sample blocks end on odd samples every other block: those leave the hot loop for the general code."""
    from spandsp_amd import engine
    n_ch = N_SMALL
    sig = _cached("r2-sig", lambda: synth.r2_mf_channels(n_ch, 160*20, seed=5204, fwd=True)[0])
    ticks, snaps = _cached("r2", lambda: _mf_reference("r2", sig, [160]))
    bank = _bank(engine.R2_MF, n_ch, r2_fwd=True)
    hits = 0
    for t in range(20):
        bank.rx_host(sig[:, 160*t:160*(t + 1)])
        blk = bank.blocks()
        assert np.array_equal(hl.got_rows(blk), hl._rows(ticks[t], n_ch)), t
        _mf_state_check(bank, snaps[t], n_ch, False, t)
        hits += int((blk["hit"] != 0).sum())
    assert hits > n_ch


# (f1 Hz, f2 Hz, min ms, max ms) per element; four pitches make a MultiDet<4, true> bank, six a MultiDet<8, true> one
_TONES4 = [[(400, 0, 700, 0)], [(1100, 0, 400, 600), (0, 0, 2800, 3200)], [(350, 440, 400, 0)]]
_HZ4 = [400, 1100, 350, 440]
_HZ8 = [400, 1100, 350, 440, 480, 620]


@pytest.mark.parametrize("n_pitch", [4, 6])
def test_super_tone_banks_with_a_cadence_plan(built, tone_kernel, n_pitch):
    """Super-tone banks of four and of eight bins per lane with cadences attached: the matcher's inputs are the block decisions,
    its tone and segment reports per tick are compared with the oracle's super_tone_rx()."""
    from oracle import restated as orc
    from spandsp_amd import engine
    n_ch = N_SMALL
    n_ticks = 100
    tones = _TONES4 if n_pitch == 4 else hl._TONES
    hz = _HZ4 if n_pitch == 4 else _HZ8

    def make():
        sig = _cached("cadence-sig", lambda: synth.cadence_plan_channels(n_ch, 160*n_ticks, 5205, hl._PLANS))
        od = orc.SuperToneDesc()
        for tone in tones:
            t = od.add_tone()
            for f1, f2, lo, hi in tone:
                od.add_element(t, f1, f2, lo, hi)
        dets = [orc.SuperTone(od, True) for _ in range(n_ch)]
        ticks = []
        for t in range(n_ticks):
            row = []
            for c, d in enumerate(dets):
                d.rx(sig[c, 160*t:160*(t + 1)], want_blocks=False)
                row.append([tuple(int(x) for x in e) for e in d.sink.events()])
                d.sink.clear()
            ticks.append(row)
        return sig, list(od.fac), ticks
    sig, fac, ticks = _cached(("cadence", n_pitch), make)
    assert len(fac) == len(hz)
    bins = {0: -1}
    bins.update({f: i for i, f in enumerate(hz)})
    bank = _bank(engine.SUPER_TONE, n_ch, bin_fac=fac)
    bank.set_cadences([[(bins[f1], bins[f2], lo, hi) for f1, f2, lo, hi in t] for t in tones], want_segments=True)
    total = 0
    for t in range(n_ticks):
        bank.rx_host(np.ascontiguousarray(sig[:, 160*t:160*(t + 1)]))
        got = bank.cadence_events()
        assert got == ticks[t], t
        total += sum(len(e) for e in got)
    assert total > n_ch


def test_banks_sharing_a_launch(built, tone_kernel):
    """spangpu_banks_rx(): a DTMF, a Bell MF, an R2 MF and a super-tone bank advanced by one launch of the kernel they share,
    twenty ticks: the DTMF bank against the oracle, the others against banks advanced by launches of their own."""
    from spandsp_amd import engine
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    n = [N_BIG, N_SMALL, N_SMALL, 33]
    sig = _sig()
    ref = _cached("twenty", lambda: hl._dtmf_reference(sig, [160], snaps_after=tuple(range(1, 21))))
    sigs = [sig, _cached("bell-sig20", lambda: synth.bell_mf_channels(n[1], 160*20, seed=5206)[0]),
            _cached("r2-sig", lambda: synth.r2_mf_channels(n[2], 160*20, seed=5204, fwd=True)[0]),
            _cached("cp-sig", lambda: synth.call_progress_channels(n[3], 160*20, seed=5207))]
    fac = [engine.goertzel_fac(f) for f in (350.0, 400.0, 440.0, 480.0, 620.0, 950.0, 1100.0, 1400.0)]

    def make():
        return [_bank(engine.DTMF, n[0]), _bank(engine.BELL_MF, n[1]),
                _bank(engine.R2_MF, n[2], r2_fwd=True), _bank(engine.SUPER_TONE, n[3], bin_fac=fac)]
    sep = make()
    fused = make()
    for b in fused[1:]:
        b.share_stream(fused[0])
    bufs = []
    for x in sigs:
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), x.shape[0]*160*2) == 0
        bufs.append(p)
    try:
        for t in range(20):
            for b, x, p in zip(sep, sigs, bufs):
                frame = np.ascontiguousarray(x[:, 160*t:160*(t + 1)])
                b.rx_host(frame)
                fused[0].sync()
                assert hip.hipMemcpy(p, frame.ctypes.data, frame.nbytes, 1) == 0
            engine.banks_rx_device(fused, [p.value for p in bufs], 160)
            for b in fused:
                b.sync()
            for b0, b1 in zip(sep, fused):
                assert b0.blocks().tobytes() == b1.blocks().tobytes(), t
            assert np.array_equal(hl.got_rows(fused[0].blocks()), hl._rows(ref["ticks"][t], n[0])), t
        _state_check(fused[0], ref["snaps"][20], _some(n[0]), "shared launch")
        for b0, b1, nn in zip(sep, fused, n):
            for c in (0, nn//2, nn - 1):
                f0, i0 = b0.get_state(c)
                f1, i1 = b1.get_state(c)
                assert hl.same_f32(f0, f1) and np.array_equal(i0, i1), c
    finally:
        for p in bufs:
            hip.hipFree(p)
