"""The V.29, V.27ter and V.17 receiver banks, cold, on lines at and beyond full scale (tests/loud_modem_lines.py) against the
oracle, which tests/test_loud_modems.py holds to the reference on exactly these lines, and against the reference's committed
results directly (tests/golden/loud_modems.npz).

Every other modem test feeds a modulator's own signal.  Here a bank of 70 channels (four full waves of the quads and of the
<16> one-lane kernels and a ragged one) carries, side by side in a wave, lanes whose carrier detector flaps (minus_rail: a
restart inside the kernel every 84 to 122 samples, carrier up and down within one short call), lanes PARKED after a failed
training, lanes cycling through up / failed / down on gated tones, and lanes training on the modem's own overdriven
transmission (V.27ter 2400 on a 2100 Hz tone as well).  V.29's carrier cutoffs stay at the init default.  All ten bit rates,
under the quads (mapping 0), the one-lane kernels (mapping 1) and the mapping flipped between calls; every channel's
put_bit / status stream after every call, the state words (floats as bit patterns) of a check set every ninth call and at
every flip, of every channel at the end.

On the bank's 70 rows the oracle gives, at every rate of a modem alike unless said: 6 flapping rows (759 carrier ups in all at
V.29, 552 at V.27ter and V.17), 342 calls (V.29; 324 the others) in which one channel reports carrier up and carrier down, 12
rows on gated tones with 20 or 21 up / failed / down cycles each, 47 rows PARKED at the end (V.27ter 4800: 49, 2400: 46), 3
trained rows (V.27ter 4800: 6, 2400: 4), and bits delivered: V.29 46 932 / 35 208 / 23 472, V.27ter 33 228 / 9 090, V.17
20 898 / 17 415 / 13 932 / 10 449 / 7 050.  No line had to be changed to meet a condition.

The full-wave one-lane kernels (65 536 channels and more) replay the rows' first 4 800 samples; spangpu_modem_fillin() is
held to the reference's xxx_rx_fillin() on lost packets before the carrier, in training, in the data and behind a failed
training (fill-ins of 160 samples, which leave the symbol phase where it was, and of 97, which do not).

On an MI355X the 73 tests pass, the slowest (test_loud_bank_matches_oracle[v29_9600-quads], with the rows' oracle runs) in
0.44 s; no kernel needed a fix.  Three one-line changes in a scratch build, one per modem, and the suite without its soak runs:
  the V.29 quad's in-kernel restart leaving last_sample stale     2 old tests fail (an offset bank, a runaway bank), 10 new
  V.27ter one-lane: the detector's low run wiped at >= 120, not > 120   11 old (one-lane, QAM tap, full-wave banks), 9 new
  the V.17 quad sending a PARKED lane's samples on to its filters  18 old (every bank with a failed training), 20 new
and 5 FAX front-end tests, whose modem the log does not name.  The new failures start at call 0 on minus_rail (the first
two) and at the first state check of a PARKED row (carrier phase).
"""
import time

import numpy as np
import pytest

import loud_lines as ll
import loud_modem_lines as lm
import test_modem_lane_mappings_gpu as lanes
import test_modem_offset_gpu as off

pytestmark = pytest.mark.gpu

N_CH = 70
RATE_IDS = [lm.rate_id(r) for r in lm.RATES]
LAUNCHES = {"quads": lambda i: 0, "one_lane": lambda i: 1, "flips": lanes.flip_mapping}
_cache = {}


@pytest.fixture(scope="module")
def golden(built):
    """a sample that rounds the other way on this platform shows as that, not as a kernel mismatch"""
    lm.use_tables()
    g = lm.load()
    assert np.array_equal(lm.line_crcs(), g["line_crcs"]), "the lines generated here are not the fixture's"
    return ll.unpack(g)


def bank_case(name, rate):
    """The bank's 70 rows and every row's oracle run on the uneven call schedule, computed once for the three launch choices;
    what the rows are is asserted on the oracle's results."""
    key = (name, rate)
    if key not in _cache:
        lm.use_tables()
        sig = lm.modem_rows(name, rate, N_CH)
        names = lm.row_names(name, rate, N_CH)
        want = [off.oracle_calls(name, rate, sig[c], ll.CHUNKS) for c in range(N_CH)]
        ups = [sum(int(np.count_nonzero(ev == -2)) for ev, _, _ in w) for w in want]
        flapping = [c for c in range(N_CH) if ups[c] >= 40]
        parked = [c for c in range(N_CH) if int(want[c][-1][2][lm.STAGE]) == lm.PARKED[name]]
        trained = [c for c in range(N_CH) if any(-4 in ev for ev, _, _ in want[c])]
        both = [(c, i) for c in range(N_CH) for i, (ev, _, _) in enumerate(want[c]) if -2 in ev and -1 in ev]
        n_bits = sum(int(np.count_nonzero(ev >= 0)) for w in want for ev, _, _ in w)
        finite = all(lm.non_finite(w[-1][1]) == 0 for w in want)
        print("%s %d: %d flapping rows (%d carrier ups), %d PARKED, %d trained, %d calls with carrier up and down, %d bits"
              % (name, rate, len(flapping), sum(ups[c] for c in flapping), len(parked), len(trained), len(both), n_bits))
        assert len(flapping) >= 6 and set(names[c] for c in flapping) == {"minus_rail", "impulses"}, flapping
        assert len(parked) >= N_CH//3 and len(trained) >= 3 and both and finite, (len(parked), trained, len(both), finite)
        assert {names[c] for c in trained} >= {"own_x8"}, trained
        # in one wave of either family (16 channels): a flapping lane, a PARKED one and one that trains
        assert any({c//16 for c in flapping} & {c//16 for c in parked} & {c//16 for c in trained})
        _cache[key] = (sig, names, None, want)
    return _cache[key]


@pytest.mark.parametrize("launch", list(LAUNCHES))
@pytest.mark.parametrize("name,rate", lm.RATES, ids=RATE_IDS)
def test_loud_bank_matches_oracle(built, golden, name, rate, launch):
    case = bank_case(name, rate)
    seen = lanes.run_offset_case(name, rate, ll.N, ll.CHUNKS, LAUNCHES[launch], case)
    assert seen == {"quads": {0}, "one_lane": {1}, "flips": {1, 4}}[launch]


# ---- the reference's committed results, no oracle in the loop --------------------------------------------------------------
@pytest.mark.parametrize("mapping", [0, 1], ids=["quads", "one_lane"])
@pytest.mark.parametrize("name,rate", lm.RATES, ids=RATE_IDS)
def test_loud_golden_direct(built, golden, name, rate, mapping):
    """every un-rotated line on 3 channels of one bank: per call the CRC of each channel's events, the status codes, the bit
    count, the words at the end"""
    named = lm.modem_lines(name, rate)
    sig = np.stack([x for _, x in named for _ in range(3)])
    n = len(sig)
    bank = off.make_bank(name, n, rate)
    status = [[] for _ in range(n)]
    n_bits = [0]*n
    try:
        with lanes.modem_mapping(mapping):
            for i, (pos, m) in enumerate(ll.calls()):
                bank.rx_host(sig[:, pos:pos + m])
                for c, ev in enumerate(bank.events()):
                    want = golden["rx/%s_%d/%s" % (name, rate, named[c//3][0])]
                    assert (ll.crc(ev) if len(ev) else 0) == int(want["call_crcs"][i]), (named[c//3][0], c, i, ev[:16])
                    status[c] += [int(v) for v in ev[ev < 0]]
                    n_bits[c] += int(np.count_nonzero(ev >= 0))
            for c in range(n):
                want = golden["rx/%s_%d/%s" % (name, rate, named[c//3][0])]
                assert status[c] == [int(v) for v in want["status"]] and n_bits[c] == int(want["sums"][0]), (named[c//3][0], c)
                lanes.check_state(bank, c, want["fwords"], want["iwords"], (name, rate, named[c//3][0]))
    finally:
        bank.close()


# ---- bank scale: the full-wave one-lane kernels ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rate", [("v29", 9600), ("v27ter", 4800), ("v17", 14400)], ids=["v29_9600", "v27ter_4800", "v17_14400"])
def test_full_wave_kernels_on_loud_lines(built, golden, name, rate):
    """65 536 channels and more (the <64> kernels; neither the last workgroup nor the last wave full): channel c carries row
    c mod 70 of the small bank, the first 4 800 samples on 160-sample calls.  Every channel's events must be those of its row
    in a 70-channel bank run beside it (itself held to the oracle), the final words of 64 spread channels the oracle's.
    On an MI355X: 0.2 to 0.4 s a modem."""
    span, chunk = 4800, 160
    sig = bank_case(name, rate)[0][:, :span]
    want = [off.oracle_calls(name, rate, sig[c], (chunk,)) for c in range(N_CH)]
    n_ch = lanes.FULL_WAVE_CH[name]
    pick = np.arange(n_ch) % N_CH
    t0 = time.perf_counter()
    small = off.make_bank(name, N_CH, rate)
    big = off.make_bank(name, n_ch, rate)
    total = 0
    try:
        for i, k in enumerate(range(0, span, chunk)):
            frame = sig[:, k:k + chunk]
            small.rx_host(frame)
            big.rx_host(frame[pick])
            counts, rows = lanes.raw_events(small)
            for c in range(N_CH):
                assert np.array_equal(rows[c, :counts[c]], want[c][i][0]), (name, rate, "70-channel bank", c, i)
            got_n, raw = lanes.raw_events(big)
            bad = np.flatnonzero(got_n != counts[pick])
            assert bad.size == 0, (name, rate, "event counts", i, bad[:8], got_n[bad[:4]], counts[pick[bad[:4]]])
            w = int(counts.max())
            assert raw.shape[1] >= w
            if w:
                diff = (raw[:, :w] != rows[pick, :w]) & (np.arange(w)[None, :] < got_n[:, None])
                bad = np.flatnonzero(diff.any(axis=1))
                assert bad.size == 0, (name, rate, "events", i, bad[:8])
            total += int(counts.sum())
        for c in np.linspace(0, n_ch - 1, 64).astype(int):
            lanes.check_state(big, int(c), want[pick[c]][-1][1], want[pick[c]][-1][2], (name, rate, n_ch, "end"))
    finally:
        big.close()
        small.close()
    assert total > 500, total
    print("%s %d: %d channels, %d events on the 70 rows, %.2f s" % (name, rate, n_ch, total, time.perf_counter() - t0))


# ---- lost packets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", [0, 1], ids=["quads", "one_lane"])
@pytest.mark.parametrize("name,rate", lm.RATES, ids=RATE_IDS)
def test_fillin_matches_reference(built, golden, name, rate, mapping):
    """spangpu_modem_fillin() in place of a call (or of its first 97 samples) on 3-channel banks: the events, the words right
    after the fill-in and the words at the end are the reference's (its xxx_rx_fillin(), recorded in the fixture)."""
    from spandsp_amd import engine
    clean = lm.clean_input(name, rate)
    for point in lm.FILLIN_POINTS:
        want = golden["fillin/%s_%d/%s" % (name, rate, point)]
        at, lost = (int(v) for v in want["at"])
        x = ll.line("sine2280") if point == "parked" else clean
        bank = off.make_bank(name, 3, rate)
        ev = [[] for _ in range(3)]
        try:
            with lanes.modem_mapping(mapping):
                for i, k in enumerate(range(0, len(x), 160)):
                    blk = x[k:k + 160]
                    if i == at:
                        for c in range(3):
                            assert engine.lib().spangpu_modem_fillin(bank.h, c, lost) == 0
                        for c in range(3):
                            lanes.check_state(bank, c, want["fwords_after"], want["iwords_after"], (name, rate, point, "after"))
                        blk = blk[lost:]
                    if len(blk):
                        bank.rx_host(np.stack([blk, blk, blk]))
                        for c, e in enumerate(bank.events()):
                            ev[c].append(e)
                for c in range(3):
                    assert np.array_equal(np.concatenate(ev[c]), want["events"]), (name, rate, point, c)
                    lanes.check_state(bank, c, want["fwords"], want["iwords"], (name, rate, point, "end"))
        finally:
            bank.close()
