"""What the lines and schedules of feed_ticks.py reach, on the oracle alone (no GPU): test_feed_ticks_gpu.py compares the
pipelined feeds with these results, and a comparison proves little on ticks in which nothing happens.  Asserted here: the
schedules hold the tick lengths and the slot reuse they are there for, the collect patterns never overrun the ring, and the
oracle's results contain the events each family's comparison is about."""
import numpy as np
import pytest

import feed_ticks as ft


def test_schedules_hold_the_ticks_they_are_for():
    cuts = ft.cuts_of(ft.XFEED_SCHEDULE, ft.XFEED_TICKS)
    assert 40 <= len(cuts) <= 60 and max(cuts) == ft.XFEED_MAX and min(cuts) == 1
    assert set(cuts) >= {400, 1, 7, 333, 160, 159, 161, 8, 2, 64, 5}
    for depth in ft.DEPTHS:
        assert ft.slot_reuse(cuts, depth), depth              # a 1- or 2-sample tick in a slot that held 400 samples
    for kind, block in ft.TONE_BLOCK.items():
        cuts = ft.cuts_of(ft.tone_schedule(kind), ft.TONE_TICKS)
        assert 40 <= len(cuts) <= 60 and max(cuts) == ft.TONE_MAX
        assert set(cuts) >= {1024, 1, 7, 64, 160, 333, block - 1}
        assert any(a == b == 1024 for a, b in zip(cuts, cuts[1:]))
        assert sum(ft.tone_schedule(kind)) % block == 0
        ends = [t for t in range(1, len(cuts)) if cuts[t] == 1 and cuts[t - 1] == block - 1]
        starts = ft.starts_of(cuts)
        assert len(ends) >= 4 and all(int(starts[t] + 1) % block == 0 and int(starts[t - 1]) % block == 0 for t in ends)


@pytest.mark.parametrize("depth", ft.DEPTHS)
def test_collect_plans_keep_a_slot_free(depth):
    for ticks in (ft.TONE_TICKS, ft.XFEED_TICKS):
        plan = ft.collect_plan(depth, ticks)
        out = most = 0
        for k in plan:
            assert out < depth                                  # acquire finds a free slot
            out += 1
            most = max(most, out)
            assert 0 <= k <= out
            out -= k
        assert most == depth                                    # ... and the ring does fill
        if depth == 8:
            assert len(set(plan)) >= 4 and plan.count(0) > ticks//4
        elif depth > 1:
            assert all(k == (1 if t >= depth - 1 else 0) for t, k in enumerate(plan))      # lag depth - 1


@pytest.mark.parametrize("kind,law", [("dtmf", 0), ("dtmf", 1), ("dtmf", 2), ("bell", 0), ("r2", 0)])
def test_tone_lines_reach(built, kind, law):
    case = ft.tone_case(kind, law)
    per_tick = [[len(s) for s in row] for row in case.digits]
    assert any(max(row) >= 2 for row, n in zip(per_tick, case.cuts) if n == 1024)          # two entries for one channel in a tick
    assert any(max(row) == 0 for row in per_tick)                                          # a tick with none in the whole bank
    delivering = sum(1 for c in range(ft.TONE_CHANNELS) if any(row[c] for row in per_tick))
    assert delivering >= ft.TONE_CHANNELS//2, delivering
    ends = case.block_end_ticks()
    assert len(ends) >= 4
    assert all(sum(per_tick[t]) > 0 for t in ends[1:]), [sum(per_tick[t]) for t in ends]   # (no digit can be accepted in the first block)
    others = [t for t, n in enumerate(case.cuts) if n == 1 and t not in ends]
    assert others and all(sum(per_tick[t]) == 0 for t in others)                           # no block end, no decision


@pytest.mark.parametrize("taps,mode,hpf,law", [(128, 0x01, False, 0), (128, 0x67, True, 0), (128, 0x67, True, 1), (128, 0x67, True, 2),
                                               (32, 0x01, False, 2)])
def test_echo_lines_reach(built, taps, mode, hpf, law):
    case = ft.echo_case(taps, mode, hpf, law)
    snaps = [d.snapshot() for d in case.dets]
    assert any(s["tap_set"] != 0 for s in snaps)
    assert any(np.any(s["taps32"]) for s in snaps)
    assert any(n <= 2 and np.any(x) for n, x in zip(case.cuts, case.clean_pcm))
    if law:
        for t, n in enumerate(case.cuts):
            a = int(case.starts[t])
            if a >= 8000:
                assert np.any(case.clean[t] != case.wire_rx[:, a:a + n]), t                 # the canceller did something in this tick


@pytest.mark.parametrize("name,rate", ft.MODEMS)
def test_modem_lines_reach(built, name, rate):
    case = ft.modem_case(name, rate)
    reports = np.zeros(ft.N_CH, np.int64)
    short = two = False
    for t, n in enumerate(case.cuts):
        for c in range(ft.N_CH):
            ev = case.events[t][c]
            k = int((ev < 0).sum())
            reports[c] += k
            short = short or (n < 8 and len(ev) > 0)
            two = two or (n == 400 and k >= 2)
    assert reports.min() >= 5, (reports.min(), int(reports.argmin()))      # carrier up, training, trained, carrier down, up again
    assert short and two


@pytest.mark.parametrize("name,rate,max_samples", ft.SHORT_MODEMS)
def test_short_modem_ticks_reach(built, name, rate, max_samples):
    """The ticks of the feed made for 1 .. 8 samples fall into the data of the call: bits on most channels, and on some channel in
    a 1-sample tick."""
    case = ft.short_modem_case(name, rate, max_samples)
    assert max(case.cuts) == max_samples and min(case.cuts) == 1 and len(case.cuts) == ft.SHORT_TICKS
    bits_of = np.array([[int((ev >= 0).sum()) for ev in row] for row in case.events])
    assert int((bits_of.sum(axis=0) > 0).sum()) >= ft.N_CH//2
    assert any(n == 1 and bits_of[t].max() > 0 for t, n in enumerate(case.cuts))
    assert bits_of.sum() >= sum(case.cuts)*rate//8000*ft.N_CH//2
