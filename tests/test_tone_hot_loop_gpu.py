"""GPU parity for the hot segment loop of the streaming tone kernels (tone_fast.hpp): a wave runs its common segments and
its whole segments with a block end on a pair boundary in a loop of their own and hands every other segment to the general
code.  Everything here is compared with oracle.restated bit for bit -- records as hit and code, the flags through the digits
and reports they stand for, state through get_state() -- with trace off and bank-wide thresholds, so that the plain block-end
decision and the hot loop are what runs.  References are computed once per module and shared by the kernel variants."""
import ctypes as C
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

# (lanes per channel, kernel family), as in test_tone_gpu.py: the general kernel under both lane mappings, the streaming
# kernels with a loader wave per workgroup and without, the latter also with two lanes per channel
_KERNELS = [(1, 1), (2, 1), (1, 2), (1, 3), (2, 3)]
_FAMILY = {1: "general", 2: "loader", 3: "stream"}


@pytest.fixture(params=_KERNELS, ids=lambda p: "lpc%d-%s" % (p[0], _FAMILY[p[1]]), autouse=True)
def lanes_per_channel(request, built):
    """Every test runs under every kernel family and lane mapping the library can pick."""
    from spandsp_amd import engine
    lpc, variant = request.param
    engine.tune_lanes_per_channel(lpc)
    engine.tune_tone_kernel(variant)
    yield lpc
    engine.tune_lanes_per_channel(0)
    engine.tune_tone_kernel(0)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_f32(a, b):
    a = np.atleast_1d(np.asarray(a, np.float32))
    b = np.atleast_1d(np.asarray(b, np.float32))
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# The call lengths of the hand-over cases: a short last segment (152, 32, 64, 96), a parity flip and its return (161, 159),
# and calls long enough for record rows 2 and 3 (320)
CYCLE = [160, 152, 160, 161, 160, 159, 320, 32, 64, 96]


def ticks_of(total, sizes):
    pos = 0
    i = 0
    while pos < total:
        n = min(sizes[i % len(sizes)], total - pos)
        yield pos, n
        pos += n
        i += 1


def got_rows(blk):
    return np.stack([blk["channel"], blk["block"], blk["hit"], blk["code"]], axis=1).astype(np.int64).reshape(-1, 4)


# --------------------------------------------------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------------------------------------------------
def _dtmf_snap(d):
    s = d.snapshot()
    return (s["v2"].copy(), s["v3"].copy(), np.float32(s["energy"]), s["current_sample"], s["last_hit"], s["in_digit"], s["duration"])


def _dtmf_reference(sig, sizes, snaps_after=()):
    """Per tick the rows every channel's dtmf_rx() made, snapshots of all detectors after the ticks named, and the digits."""
    from oracle import restated as orc
    dets = [orc.Dtmf(0) for _ in range(sig.shape[0])]
    ticks = []
    snaps = {}
    for t, (pos, n) in enumerate(ticks_of(sig.shape[1], sizes)):
        ticks.append([[(int(b["hit"]), int(b["aux"])) for b in d.rx(sig[c, pos:pos + n])] for c, d in enumerate(dets)])
        if t + 1 in snaps_after:
            snaps[t + 1] = [_dtmf_snap(d) for d in dets]
    snaps["end"] = [_dtmf_snap(d) for d in dets]
    return {"ticks": ticks, "snaps": snaps, "digits": [d.get() for d in dets]}


def _rows(tick, n_ch):
    rows = [(c, j, h, a) for c in range(n_ch) for j, (h, a) in enumerate(tick[c])]
    return np.array(rows, np.int64).reshape(-1, 4)


def _dtmf_state_check(bank, snap, n_ch, what):
    for c in range(n_ch):
        f, i = bank.get_state(c)
        v2, v3, energy, cs, last_hit, in_digit, duration = snap[c]
        assert same_f32(f[0:8], v2), (what, "v2", c)
        assert same_f32(f[8:16], v3), (what, "v3", c)
        assert same_f32(f[16:17], [energy]), (what, "energy", c)
        assert (i[0], i[1], i[2], i[3]) == (cs, last_hit, in_digit, duration), (what, "ints", c, i, snap[c][3:])


def _dtmf_digits(digits, blk):
    from spandsp_amd import engine
    for r in blk[((blk["flags"] & engine.BLK_CHANGE) != 0) & (blk["code"] != 0)]:
        digits[r["channel"]] += chr(int(r["code"]))


def _dtmf_base():
    """320 DTMF lines of 60 ticks, and what 320 reference detectors make of them tick by tick."""
    def make():
        sig, _ = synth.dtmf_channels(320, 160*60, seed=4101)
        return sig, _dtmf_reference(sig, [160], snaps_after=(1, 7, 51, 60))
    return _cached("dtmf-base", make)


# --------------------------------------------------------------------------------------------------------------------
# 1. every block-end position
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ch", [320, 300])
def test_every_block_end_position(built, n_ch):
    """60 consecutive 160-sample ticks of DTMF: the 102-sample block's phase repeats after 51 ticks, so the block end visits
    every segment of a frame and every pair index in it (and every odd split, which leaves the hot loop).  320 channels are a
    full workgroup and one with one live and three idle consumer waves; 300 end in a part-filled wave."""
    from spandsp_amd import engine
    sig, ref = _dtmf_base()
    bank = engine.ToneBank(engine.DTMF, n_ch)
    digits = [""]*n_ch
    for t in range(60):
        bank.rx_host(sig[:n_ch, 160*t:160*(t + 1)])
        blk = bank.blocks()
        assert np.array_equal(got_rows(blk), _rows(ref["ticks"][t], n_ch)), t
        _dtmf_digits(digits, blk)
        if t + 1 in (1, 7, 51, 60):
            _dtmf_state_check(bank, ref["snaps"][t + 1], n_ch, "tick %d" % (t + 1))
    assert digits == ref["digits"][:n_ch]
    assert sum(len(d) for d in digits) > n_ch


# --------------------------------------------------------------------------------------------------------------------
# 2. hand-overs between the hot loop and the general one
# --------------------------------------------------------------------------------------------------------------------
N_HAND = 130                    # two full waves and a third with two channels
T_HAND = 4*sum(CYCLE)           # four turns of the cycle


def test_hand_overs_dtmf(built):
    """(A call of 56 samples first: the 320-sample call of the first turn then starts 90 samples into a block and ends four.)"""
    from spandsp_amd import engine
    sizes = [56] + 4*CYCLE

    def make():
        sig, _ = synth.dtmf_channels(N_HAND, sum(sizes), seed=4102)
        return sig, _dtmf_reference(sig, sizes)
    sig, ref = _cached("dtmf-hand", make)
    bank = engine.ToneBank(engine.DTMF, N_HAND)
    digits = [""]*N_HAND
    most = 0
    for t, (pos, n) in enumerate(ticks_of(sum(sizes), sizes)):
        bank.rx_host(sig[:, pos:pos + n])
        blk = bank.blocks()
        assert np.array_equal(got_rows(blk), _rows(ref["ticks"][t], N_HAND)), (t, n)
        _dtmf_digits(digits, blk)
        most = max(most, int(blk["block"].max()) + 1 if blk.size else 0)
    _dtmf_state_check(bank, ref["snaps"]["end"], N_HAND, "end")
    assert digits == ref["digits"]
    assert most == 4                    # record rows 2 and 3 were stored from the block end itself


def _mf_reference(kind, sig, fwd=True):
    from oracle import restated as orc
    dets = [orc.BellMf(0) if kind == "bell" else orc.R2Mf(fwd, True) for _ in range(sig.shape[0])]
    ticks = [[[(int(b["hit"]), int(b["aux"])) for b in d.rx(sig[c, pos:pos + n])] for c, d in enumerate(dets)]
             for pos, n in ticks_of(sig.shape[1], CYCLE)]
    snaps = [d.snapshot() for d in dets]
    if kind == "bell":
        reports = [d.get() for d in dets]
    else:
        reports = [[(int(e["a"]), int(e["b"]), int(e["c"])) for e in d.sink.events()] for d in dets]
    return {"ticks": ticks, "snaps": snaps, "reports": reports}


def test_hand_overs_bell_mf(built):
    """The 120-sample block: three and three quarter segments."""
    from spandsp_amd import engine

    def make():
        sig, _ = synth.bell_mf_channels(N_HAND, T_HAND, seed=4103)
        return sig, _mf_reference("bell", sig)
    sig, ref = _cached("bell-hand", make)
    bank = engine.ToneBank(engine.BELL_MF, N_HAND)
    digits = [""]*N_HAND
    for t, (pos, n) in enumerate(ticks_of(T_HAND, CYCLE)):
        bank.rx_host(sig[:, pos:pos + n])
        blk = bank.blocks()
        assert np.array_equal(got_rows(blk), _rows(ref["ticks"][t], N_HAND)), (t, n)
        for r in blk[(blk["flags"] & engine.BLK_REPORT) != 0]:
            digits[r["channel"]] += chr(int(r["code"]))
    assert digits == ref["reports"]
    assert sum(len(d) for d in digits) > N_HAND//4
    for c, s in enumerate(ref["snaps"]):
        f, i = bank.get_state(c)
        assert same_f32(f[0:6], s["v2"]) and same_f32(f[6:12], s["v3"]), c
        hits = [i[1], i[2], i[3] & 0xFF, (i[3] >> 8) & 0xFF, (i[3] >> 16) & 0xFF]
        assert i[0] == s["current_sample"] and hits == list(s["hits"]), (c, i, s["hits"])


def test_hand_overs_r2_mf(built):
    """The odd 133-sample block flips the parity of the split every block: one call leaves the hot loop and comes back."""
    from spandsp_amd import engine

    def make():
        sig, _ = synth.r2_mf_channels(N_HAND, T_HAND, seed=4104, fwd=True)
        return sig, _mf_reference("r2", sig)
    sig, ref = _cached("r2-hand", make)
    bank = engine.ToneBank(engine.R2_MF, N_HAND, r2_fwd=True)
    events = [[] for _ in range(N_HAND)]
    for t, (pos, n) in enumerate(ticks_of(T_HAND, CYCLE)):
        bank.rx_host(sig[:, pos:pos + n])
        blk = bank.blocks()
        assert np.array_equal(got_rows(blk), _rows(ref["ticks"][t], N_HAND)), (t, n)
        for r in blk[(blk["flags"] & engine.BLK_REPORT) != 0]:
            events[r["channel"]].append((int(r["code"]), -10 if r["code"] else -99, 0))
    assert events == ref["reports"]
    assert sum(len(e) for e in events) > N_HAND//4
    for c, s in enumerate(ref["snaps"]):
        f, i = bank.get_state(c)
        assert same_f32(f[0:6], s["v2"]) and same_f32(f[6:12], s["v3"]) and i[0] == s["current_sample"], c


N_GOERTZEL = 70
BLOCK_GOERTZEL = 110            # three segments and seven pairs: the split lands on a pair boundary until a call of odd length


def _goertzel_reference(sig, freqs):
    from oracle import restated as orc
    energies = []               # [channel][block] -> float32[len(freqs)]
    states = []
    for c in range(sig.shape[0]):
        gs = [orc.Goertzel(f, BLOCK_GOERTZEL) for f in freqs]
        per_block = []
        pos = 0
        while pos + BLOCK_GOERTZEL <= sig.shape[1]:
            for g in gs:
                assert g.update(sig[c, pos:pos + BLOCK_GOERTZEL]) == BLOCK_GOERTZEL
            per_block.append(np.array([g.result() for g in gs], np.float32))
            pos += BLOCK_GOERTZEL
        for g in gs:
            g.update(sig[c, pos:])
        energies.append(per_block)
        states.append((np.array([g.buf[0:4].view(np.float32)[0] for g in gs], np.float32),
                       np.array([g.buf[4:8].view(np.float32)[0] for g in gs], np.float32), sig.shape[1] - pos))
    return energies, states


@pytest.mark.parametrize("n_bins", [4, 6, 8, 12, 16])
def test_hand_overs_goertzel_bank(built, n_bins):
    """Generic banks: 4, 6 and 8 bins take their block ends through the asm body, 12 and 16 leave the hot loop for them."""
    from spandsp_amd import engine
    freqs = [350.0 + 97.0*i for i in range(n_bins)]

    def make():
        sig = _cached("goertzel-sig", lambda: synth.call_progress_channels(N_GOERTZEL, T_HAND, seed=4105))
        return sig, _goertzel_reference(sig, freqs)
    sig, (energies, states) = _cached("goertzel-%d" % n_bins, make)
    bank = engine.ToneBank(engine.GOERTZEL, N_GOERTZEL, bin_fac=[engine.goertzel_fac(f) for f in freqs], block_len=BLOCK_GOERTZEL)
    got = [[] for _ in range(N_GOERTZEL)]
    for pos, n in ticks_of(T_HAND, CYCLE):
        bank.rx_host(sig[:, pos:pos + n])
        blk = bank.blocks()
        if blk.size:
            tr = bank.trace()
            for r in blk:
                got[r["channel"]].append(tr[r["block"], :n_bins, r["channel"]].copy())
    for c in range(N_GOERTZEL):
        assert len(got[c]) == len(energies[c]), c
        for k, (x, y) in enumerate(zip(got[c], energies[c])):
            assert same_f32(x, y), (c, k)
        f, i = bank.get_state(c)
        v2, v3, cs = states[c]
        assert same_f32(f[0:n_bins], v2) and same_f32(f[bank.nbins:bank.nbins + n_bins], v3) and i[0] == cs, c


# --------------------------------------------------------------------------------------------------------------------
# 3. divergent block phases
# --------------------------------------------------------------------------------------------------------------------
def test_divergent_phases_and_back(built):
    """A ragged rx_var call puts one channel of each wave out of phase; whole calls then run in the general loop.  51 ticks
    later the others' block phase is zero again, and resetting the odd channels makes every wave uniform: the hot loop again."""
    from oracle import restated as orc
    from spandsp_amd import engine
    n_ch = 130
    victims = [5, 64 + 40, 129]
    n_ticks = 1 + 51 + 8

    def make():
        sig, _ = synth.dtmf_channels(n_ch, 160*n_ticks, seed=4106)
        dets = [orc.Dtmf(0) for _ in range(n_ch)]
        pos = np.zeros(n_ch, np.int64)
        ticks = []
        snaps = {}
        for t in range(n_ticks):
            lens = np.full(n_ch, 160, np.int32)
            if t == 0:
                lens[:] = 0
                lens[victims] = 37
            if t == 52:
                for c in victims:
                    dets[c] = orc.Dtmf(0)
            ticks.append([[(int(b["hit"]), int(b["aux"])) for b in d.rx(sig[c, pos[c]:pos[c] + lens[c]])] if lens[c] else []
                          for c, d in enumerate(dets)])
            pos += lens
            if t in (51, n_ticks - 1):
                snaps[t] = [_dtmf_snap(d) for d in dets]
        return sig, ticks, snaps
    sig, ticks, snaps = _cached("divergent", make)
    bank = engine.ToneBank(engine.DTMF, n_ch)
    pos = np.zeros(n_ch, np.int64)
    for t in range(n_ticks):
        lens = np.full(n_ch, 160, np.int32)
        if t == 0:
            lens[:] = 0
            lens[victims] = 37
        if t == 52:
            for c in victims:
                bank.reset_channel(c)
        frames = np.zeros((n_ch, 160), np.int16)
        for c in range(n_ch):
            frames[c, :lens[c]] = sig[c, pos[c]:pos[c] + lens[c]]
        if t == 0:
            bank.rx_host_var(frames, lens)
        else:
            bank.rx_host(frames)
        pos += lens
        assert np.array_equal(got_rows(bank.blocks()), _rows(ticks[t], n_ch)), t
        if t in snaps:
            _dtmf_state_check(bank, snaps[t], n_ch, "tick %d" % t)
    f, i = bank.get_state(0)
    assert i[0] == bank.get_state(victims[0])[1][0]         # one phase again


# --------------------------------------------------------------------------------------------------------------------
# 4. active mask
# --------------------------------------------------------------------------------------------------------------------
def test_active_mask(built):
    """rx_var with lengths 0 / 160: channels sitting a call out, a wave with no live channel (it only keeps the workgroup's
    barriers), and the bank's part-filled tail wave masked in part and whole."""
    from oracle import restated as orc
    from spandsp_amd import engine
    n_ch = 300
    n_ticks = 30

    def masks():
        rng = np.random.default_rng(4107)
        out = []
        for t in range(n_ticks):
            lens = np.where(rng.random(n_ch) < 0.25, 0, 160).astype(np.int32)
            if t % 4 == 1:
                lens[64:128] = 0                    # a whole wave of the first workgroup
            if t % 5 == 2:
                lens[256:] = 0                      # the tail wave: the second workgroup has no live wave at all
            if t % 7 == 3:
                lens[:] = 0
                lens[[3, 299]] = 160
            out.append(lens)
        return out

    def make():
        sig, _ = synth.dtmf_channels(n_ch, 160*n_ticks, seed=4107)
        dets = [orc.Dtmf(0) for _ in range(n_ch)]
        pos = np.zeros(n_ch, np.int64)
        ticks = []
        for lens in masks():
            ticks.append([[(int(b["hit"]), int(b["aux"])) for b in d.rx(sig[c, pos[c]:pos[c] + 160])] if lens[c] else []
                          for c, d in enumerate(dets)])
            pos += lens
        return sig, ticks, [_dtmf_snap(d) for d in dets], [d.get() for d in dets]
    sig, ticks, snap, want_digits = _cached("mask", make)
    bank = engine.ToneBank(engine.DTMF, n_ch)
    pos = np.zeros(n_ch, np.int64)
    digits = [""]*n_ch
    rng = np.random.default_rng(1)
    for t, lens in enumerate(masks()):
        frames = rng.integers(-20000, 20000, (n_ch, 160)).astype(np.int16)      # rows of channels sitting out are never read
        for c in np.nonzero(lens)[0]:
            frames[c] = sig[c, pos[c]:pos[c] + 160]
        bank.rx_host_var(frames, lens)
        pos += lens
        blk = bank.blocks()
        assert np.array_equal(got_rows(blk), _rows(ticks[t], n_ch)), t
        _dtmf_digits(digits, blk)
    _dtmf_state_check(bank, snap, n_ch, "mask")
    assert digits == want_digits


# --------------------------------------------------------------------------------------------------------------------
# 5. other ways in
# --------------------------------------------------------------------------------------------------------------------
def test_queue_mode_second_launch_starts_past_workgroup_zero(built):
    """1088 channels are five workgroups: in queue mode the second launch covers workgroups 2 .. 4 (wg0 = 2).  Against one
    launch, and the first 320 channels against the oracle."""
    from spandsp_amd import engine
    base, ref = _dtmf_base()
    n_ch = 1088
    sig = np.ascontiguousarray(np.tile(base, (4, 1))[:n_ch])
    one = engine.ToneBank(engine.DTMF, n_ch)
    two = engine.ToneBank(engine.DTMF, n_ch)
    one.set_queues(1)
    two.set_queues(2)
    for t in range(20):
        fr = sig[:, 160*t:160*(t + 1)]
        one.rx_host(fr)
        two.rx_host(fr)
        r1 = one.blocks()
        r2 = two.blocks()
        assert r1.tobytes() == r2.tobytes(), t
        assert np.array_equal(got_rows(r2[r2["channel"] < 320]), _rows(ref["ticks"][t], 320)), t
    for c in (0, 511, 512, 700, n_ch - 1):
        f1, i1 = one.get_state(c)
        f2, i2 = two.get_state(c)
        assert same_f32(f1, f2) and np.array_equal(i1, i2), c
    two.set_queues(1)


def _g711_encode(x, table):
    """Some G.711 code whose decoded value is nearest to x (test input only; the decode is what is under test)."""
    order = np.argsort(table.astype(np.int32), kind="stable")
    vals = table[order].astype(np.int32)
    pos = np.clip(np.searchsorted(vals, x.astype(np.int32)), 1, 255)
    lower = (x - vals[pos - 1]) <= (vals[pos] - x)
    return order[np.where(lower, pos - 1, pos)].astype(np.uint8)


@pytest.mark.parametrize("law", ["alaw", "ulaw"])
def test_g711_block_ends_reach_the_general_loop(built, law):
    """G.711 input has no asm body: its common segments run in the hot loop, every segment with a block end in the general
    one.  Against the decoded PCM through the linear kernel, and that against the oracle."""
    from spandsp_amd import engine
    table = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g711_decode.npz"))[law]
    code = engine.G711_ALAW if law == "alaw" else engine.G711_ULAW
    n_ch = 150
    n_ticks = 30

    def make():
        sig, _ = synth.dtmf_channels(n_ch, 160*n_ticks, seed=4108)
        codes = _g711_encode(sig, table)
        lin = table[codes].astype(np.int16)
        return codes, lin, _dtmf_reference(lin, [160])
    codes, lin, ref = _cached("g711-" + law, make)
    a = engine.ToneBank(engine.DTMF, n_ch)
    b = engine.ToneBank(engine.DTMF, n_ch)
    for t in range(n_ticks):
        a.rx_host(lin[:, 160*t:160*(t + 1)])
        b.rx_host_g711(codes[:, 160*t:160*(t + 1)], code)
        b.sync()
        ra = a.blocks()
        rb = b.blocks()
        assert ra.tobytes() == rb.tobytes(), t
        assert np.array_equal(got_rows(rb), _rows(ref["ticks"][t], n_ch)), t
    _dtmf_state_check(b, ref["snaps"]["end"], n_ch, law)
    assert sum(len(d) for d in ref["digits"]) > n_ch//2


# (f1 Hz, f2 Hz, min ms, max ms) per element, and the lines' plans, as in test_cadence_gpu.py
_TONES = [
    [(400, 0, 700, 0)],
    [(1100, 0, 400, 600), (0, 0, 2800, 3200)],
    [(350, 440, 400, 0)],
    [(480, 620, 450, 550), (0, 0, 450, 550)],
]
_PLANS = [
    [(400, 0, 1500)],
    [(1100, 0, 500), (0, 0, 3000)],
    [(350, 440, 1200), (0, 0, 300)],
    [(480, 620, 500), (0, 0, 500)],
    [(620, 0, 300), (0, 0, 200)],
]


def test_super_tone_bank_with_its_cadence_matcher(built):
    """A small super-tone bank whose cadences are matched in the streaming kernel's epilogue: the tone and segment reports of
    every channel, tick by tick, against the oracle's super_tone_rx()."""
    from oracle import restated as orc
    from spandsp_amd import engine
    n_ch = 70
    n_ticks = 150                       # 3 s of line

    def desc():
        od = orc.SuperToneDesc()
        for tone in _TONES:
            t = od.add_tone()
            for f1, f2, lo, hi in tone:
                od.add_element(t, f1, f2, lo, hi)
        return od

    def make():
        sig = synth.cadence_plan_channels(n_ch, 160*n_ticks, 4109, _PLANS)
        od = desc()
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
    sig, fac, ticks = _cached("cadence", make)
    hz = [400, 1100, 350, 440, 480, 620]            # the order the descriptor met them in
    assert len(fac) == len(hz)
    bins = {0: -1}
    bins.update({f: i for i, f in enumerate(hz)})
    bank = engine.ToneBank(engine.SUPER_TONE, n_ch, bin_fac=fac)
    bank.set_cadences([[(bins[f1], bins[f2], lo, hi) for f1, f2, lo, hi in t] for t in _TONES], want_segments=True)
    total = 0
    for t in range(n_ticks):
        bank.rx_host(np.ascontiguousarray(sig[:, 160*t:160*(t + 1)]))
        got = bank.cadence_events()
        assert got == ticks[t], t
        total += sum(len(e) for e in got)
    assert total > 3*n_ch


def test_records_buffer_of_the_callers(built):
    """spangpu_bank_set_records_buffer(): the record words of a tick (rows 0 and 1 from the write-back) in a caller's device
    buffer are the oracle's hits and codes and the flags spangpu_bank_blocks() reports."""
    from spandsp_amd import engine
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    sig, ref = _dtmf_base()
    n_ch = 300
    bank = engine.ToneBank(engine.DTMF, n_ch)
    buf = C.c_void_p()
    nbytes = 2*n_ch*4
    assert hip.hipMalloc(C.byref(buf), 2*nbytes) == 0
    words = np.zeros(2*n_ch, np.uint32)
    try:
        for t in range(15):
            at = C.c_void_p(buf.value + (t % 2)*nbytes)
            bank.set_records_buffer(at, nbytes)
            bank.rx_host(sig[:n_ch, 160*t:160*(t + 1)])
            blk = bank.blocks()
            assert np.array_equal(got_rows(blk), _rows(ref["ticks"][t], n_ch)), t
            nb = len(blk)//n_ch
            assert nb*n_ch == len(blk) and 1 <= nb <= 2
            assert hip.hipMemcpy(words.ctypes.data, at, nbytes, 2) == 0
            want = (blk["hit"].astype(np.uint32) | (blk["code"].astype(np.uint32) << 8) | (blk["flags"].astype(np.uint32) << 16)).reshape(n_ch, nb).T
            assert np.array_equal(words[:nb*n_ch].reshape(nb, n_ch), want), t
    finally:
        bank.set_records_buffer(None, 0)
        hip.hipFree(buf)
