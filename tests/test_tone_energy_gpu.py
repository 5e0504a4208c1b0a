"""GPU parity for the common segment's asm body of the streaming tone kernels (tone_fast.hpp, pairs_common_asm): the block
energy's squares and adds stand in the issue gaps of the recurrence instead of behind it, and must still be the reference's
operations in the reference's order -- energy += x*x per sample, in sample order (dtmf.c:199, super_tone_rx.c:467).

Every float is compared with oracle.restated as a uint32 pattern, after EVERY call, under the streaming kernels with a loader
wave and without.  The shapes are the smallest at which the change can go wrong:

  * 70 channels: one full wave and a wave of six live lanes;
  * calls of 32, 64, 160, 160, 96, 160 samples.  For DTMF's 102-sample block that is: a call that is all common segments
    (64), a common segment in each of the five positions of a 160-sample call, a block end in a call's first segment and in its
    last (and in a 32-sample call's only one).  The 120- and 128-sample blocks of the other banks meet the same calls at
    other phases; the 128-sample block always ends on a segment's last sample, the asm body's business with p = 16;
  * line 0 is a square wave of +-32 767: its squares are 1.07e9 and the running sum passes 2^24 with the first sample, so
    every add rounds and any other order of the adds shows; line 1 is near the noise floor (|x| <= 3); the rest are DTMF lines.

Banks: DTMF (NP = 4, energy), super-tone banks of 4 and 8 monitored frequencies -- the generic Goertzel bank with a block
energy, NP = 2 and 4 -- and Bell MF (NP = 3, no energy: the same body without the energy's instructions)."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

N_CH = 70
CALLS = [32, 64, 160, 160, 96, 160]
TOTAL = sum(CALLS)

_FAMILY = {2: "loader", 3: "stream"}


@pytest.fixture(params=[2, 3], ids=lambda v: _FAMILY[v], autouse=True)
def tone_kernel(request, built):
    from spandsp_amd import engine
    engine.tune_lanes_per_channel(1)
    engine.tune_tone_kernel(request.param)
    yield request.param
    engine.tune_lanes_per_channel(0)
    engine.tune_tone_kernel(0)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def bits(a):
    return np.ascontiguousarray(np.atleast_1d(np.asarray(a, np.float32))).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def lines():
    """int16 [N_CH, TOTAL]: the full-scale square wave, the line at the noise floor, DTMF lines."""
    def make():
        sig, _ = synth.dtmf_channels(N_CH, TOTAL, seed=4201)
        sig = np.array(sig, np.int16)
        sig[0] = np.where((np.arange(TOTAL)//4) % 2 == 0, 32767, -32767)        # 1 kHz
        sig[1] = np.random.default_rng(4202).integers(-3, 4, TOTAL)
        sig[1, ::7] = 1                                                         # (never all zero inside a call)
        return np.ascontiguousarray(sig)
    return _cached("lines", make)


def calls():
    pos = 0
    for n in CALLS:
        yield pos, n
        pos += n


def got_rows(blk):
    return np.stack([blk["channel"], blk["block"], blk["hit"], blk["code"]], axis=1).astype(np.int64).reshape(-1, 4)


def want_rows(tick):
    rows = [(c, j, h, a) for c in range(N_CH) for j, (h, a) in enumerate(tick[c])]
    return np.array(rows, np.int64).reshape(-1, 4)


# --------------------------------------------------------------------------------------------------------------------
# references (oracle.restated on the CPU, once per module): per call, every line's state words and block rows
# --------------------------------------------------------------------------------------------------------------------
def dtmf_reference():
    def make():
        from oracle import restated as orc
        sig = lines()
        dets = [orc.Dtmf(0) for _ in range(N_CH)]
        out = []
        for pos, n in calls():
            rows = [[(int(b["hit"]), int(b["aux"])) for b in d.rx(sig[c, pos:pos + n])] for c, d in enumerate(dets)]
            snaps = [d.snapshot() for d in dets]
            out.append({"rows": rows,
                        "v2": np.array([s["v2"] for s in snaps], np.float32), "v3": np.array([s["v3"] for s in snaps], np.float32),
                        "energy": np.array([np.float32(s["energy"]) for s in snaps], np.float32),
                        "ints": [(s["current_sample"], s["last_hit"], s["in_digit"], s["duration"]) for s in snaps]})
        return out
    return _cached("dtmf", make)


# orc_st_t (oracle/oracle.h): desc pointer, energy, four ints, eleven segments of three ints, v2[64], v3[64]
_ST_ENERGY = 8
_ST_CS = 8 + 4 + 2*4
_ST_V2 = 8 + 4 + 4*4 + 11*12
_ST_V3 = _ST_V2 + 64*4

_ST_PAIRS = [(350, 440), (480, 620), (697, 1209), (941, 1633)]      # (the last two: DTMF rows and columns, what the lines carry)


def st_desc(n_bins):
    from oracle import restated as orc
    d = orc.SuperToneDesc()
    for f1, f2 in _ST_PAIRS[:n_bins//2]:
        t = d.add_tone()
        d.add_element(t, f1, f2, 300, 0)
    assert d.monitored == n_bins
    return d


def st_reference(n_bins):
    def make():
        from oracle import restated as orc
        sig = lines()
        desc = st_desc(n_bins)
        dets = [orc.SuperTone(desc) for _ in range(N_CH)]
        out = []
        blocks = 0
        for pos, n in calls():
            for c, d in enumerate(dets):
                done = int(d.rx(sig[c, pos:pos + n], want_blocks=False))
                if c == 0:
                    blocks += done
            out.append({"energy": np.array([d.buf[_ST_ENERGY:_ST_ENERGY + 4].view(np.float32)[0] for d in dets], np.float32),
                        "v2": np.array([d.buf[_ST_V2:_ST_V2 + 4*n_bins].view(np.float32) for d in dets], np.float32),
                        "v3": np.array([d.buf[_ST_V3:_ST_V3 + 4*n_bins].view(np.float32) for d in dets], np.float32),
                        "cs": [int(d.buf[_ST_CS:_ST_CS + 4].view(np.int32)[0]) for d in dets]})
        return desc, out, blocks
    return _cached("st-%d" % n_bins, make)


def bell_reference():
    def make():
        from oracle import restated as orc
        sig = lines()
        dets = [orc.BellMf(0) for _ in range(N_CH)]
        out = []
        for pos, n in calls():
            rows = [[(int(b["hit"]), int(b["aux"])) for b in d.rx(sig[c, pos:pos + n])] for c, d in enumerate(dets)]
            snaps = [d.snapshot() for d in dets]
            out.append({"rows": rows, "v2": np.array([s["v2"] for s in snaps], np.float32), "v3": np.array([s["v3"] for s in snaps], np.float32),
                        "cs": [s["current_sample"] for s in snaps], "hits": [list(s["hits"]) for s in snaps]})
        return out
    return _cached("bell", make)


# --------------------------------------------------------------------------------------------------------------------
# the references alone: no comparison below is vacuous
# --------------------------------------------------------------------------------------------------------------------
def check_reference_is_not_vacuous(ref, blocks, energy):
    assert blocks >= 1
    if energy:
        for k, r in enumerate(ref):
            assert np.all(np.isfinite(r["energy"])), k
        # a call that ends on a block end leaves zero behind; every line has a running energy after most calls
        live = [k for k, r in enumerate(ref) if np.all(bits(r["energy"]) != 0)]
        assert len(live) >= 4, live
        assert ref[live[0]]["energy"][0] > 2.0**24 and ref[live[0]]["energy"][1] < 2.0**12       # the loud line and the quiet one


# --------------------------------------------------------------------------------------------------------------------
# the banks
# --------------------------------------------------------------------------------------------------------------------
def test_dtmf_energy_state_and_records(built):
    from spandsp_amd import engine
    sig = lines()
    ref = dtmf_reference()
    check_reference_is_not_vacuous(ref, sum(len(r["rows"][0]) for r in ref), True)
    assert sum(len(r["rows"][0]) for r in ref) == TOTAL//102
    bank = engine.ToneBank(engine.DTMF, N_CH)
    for k, (pos, n) in enumerate(calls()):
        bank.rx_host(sig[:, pos:pos + n])
        assert np.array_equal(got_rows(bank.blocks()), want_rows(ref[k]["rows"])), (k, n)
        for c in range(N_CH):
            f, i = bank.get_state(c)
            assert same_bits(f[16:17], ref[k]["energy"][c:c + 1]), (k, n, c, "energy", bits(f[16:17]), bits(ref[k]["energy"][c:c + 1]))
            assert same_bits(f[0:8], ref[k]["v2"][c]), (k, n, c, "v2")
            assert same_bits(f[8:16], ref[k]["v3"][c]), (k, n, c, "v3")
            assert (i[0], i[1], i[2], i[3]) == ref[k]["ints"][c], (k, n, c, i, ref[k]["ints"][c])


@pytest.mark.parametrize("n_bins", [4, 8])
def test_goertzel_bank_energy(built, n_bins):
    """The bank of n_bins generic Goertzel bins with a block energy (the super-tone detector's): NP = n_bins/2."""
    from spandsp_amd import engine
    sig = lines()
    desc, ref, blocks = st_reference(n_bins)
    check_reference_is_not_vacuous(ref, blocks, True)
    bank = engine.ToneBank(engine.SUPER_TONE, N_CH, bin_fac=list(desc.fac))
    nb = bank.nbins
    assert nb == n_bins
    for k, (pos, n) in enumerate(calls()):
        bank.rx_host(sig[:, pos:pos + n])
        for c in range(N_CH):
            f, i = bank.get_state(c)
            assert same_bits(f[2*nb:2*nb + 1], ref[k]["energy"][c:c + 1]), (k, n, c, "energy", bits(f[2*nb:2*nb + 1]), bits(ref[k]["energy"][c:c + 1]))
            assert same_bits(f[0:n_bins], ref[k]["v2"][c]), (k, n, c, "v2")
            assert same_bits(f[nb:nb + n_bins], ref[k]["v3"][c]), (k, n, c, "v3")
            assert i[0] == ref[k]["cs"][c], (k, n, c, i)


def test_bell_mf_state_and_records(built):
    """No energy, NP = 3: the body without the energy's instructions leaves state and records what they were."""
    from spandsp_amd import engine
    sig = lines()
    ref = bell_reference()
    check_reference_is_not_vacuous(ref, sum(len(r["rows"][0]) for r in ref), False)
    assert sum(len(r["rows"][0]) for r in ref) == TOTAL//120
    assert any(np.any(bits(r["v2"]) != 0) for r in ref)
    bank = engine.ToneBank(engine.BELL_MF, N_CH)
    for k, (pos, n) in enumerate(calls()):
        bank.rx_host(sig[:, pos:pos + n])
        assert np.array_equal(got_rows(bank.blocks()), want_rows(ref[k]["rows"])), (k, n)
        for c in range(N_CH):
            f, i = bank.get_state(c)
            assert same_bits(f[0:6], ref[k]["v2"][c]), (k, n, c, "v2")
            assert same_bits(f[6:12], ref[k]["v3"][c]), (k, n, c, "v3")
            hits = [i[1], i[2], i[3] & 0xFF, (i[3] >> 8) & 0xFF, (i[3] >> 16) & 0xFF]
            assert i[0] == ref[k]["cs"][c] and hits == ref[k]["hits"][c], (k, n, c, i, ref[k]["hits"][c])
