"""The three pipelined feeds (spangpu_feed_*, spangpu_echo_feed_*, spangpu_modem_feed_*: csrc/feed_api.hip) on uneven ticks, at
every ring depth and both ways up, against the oracle (oracle.restated, pinned to the reference by test_oracle_pin.py) fed the same
lines in the same cuts.  Ticks are 1 to 400 samples long (tone: to 1024) in slots that held a longer tick before, every slot is
poisoned at full scale over its whole stride before a tick is written, and ticks are collected at once, `depth` - 1 ticks behind,
or in a seeded irregular pattern (feed_ticks.py; what the lines reach is asserted without a GPU in test_feed_ticks.py).  No call is
made on a bank while a tick is outstanding: state is read after the last collect."""
import functools

import numpy as np
import pytest

import echo_lines
import feed_ticks as ft

pytestmark = pytest.mark.gpu


# ---- tone ------------------------------------------------------------------------------------------------------------------
def tone_bank(engine, kind):
    if kind == "dtmf":
        return engine.ToneBank(engine.DTMF, ft.TONE_CHANNELS)
    if kind == "bell":
        return engine.ToneBank(engine.BELL_MF, ft.TONE_CHANNELS)
    return engine.ToneBank(engine.R2_MF, ft.TONE_CHANNELS, r2_fwd=True)


@functools.lru_cache(maxsize=None)
def serial_entries(kind, law):
    """What the oracle has no word for -- the block index of an entry -- from the serial path fed the same cuts: rx_host() and the
    records of blocks() in which the detector accepted a digit (DTMF: BLK_CHANGE, dtmf.c:318-340; Bell MF and R2 MF: BLK_REPORT,
    bell_r2_mf.c:629-655 and :869-875; with a code)."""
    from spandsp_amd import engine
    case = ft.tone_case(kind, law)
    accept = engine.BLK_CHANGE if kind == "dtmf" else engine.BLK_REPORT
    out = []
    with ft.closing_in_order(tone_bank(engine, kind)) as own:
        bank = own.objs[0]
        for t, n in enumerate(case.cuts):
            a = int(case.starts[t])
            if law:
                codes = np.ascontiguousarray(case.wire[:, a:a + n])
                bank.rx_host_g711(codes, law)
            else:
                bank.rx_host(case.wire[:, a:a + n])
            blk = bank.blocks()
            out.append(sorted((int(r["channel"]), int(r["code"]), int(r["block"])) for r in blk if (r["flags"] & accept) and r["code"]))
    return out


def run_tone(kind, law, depth, edges=False):
    from spandsp_amd import engine
    case = ft.tone_case(kind, law)
    want = serial_entries(kind, law)
    with ft.closing_in_order(tone_bank(engine, kind)) as own:
        feed = own(engine.Feed(own.objs[0], ft.TONE_MAX, law=law, depth=depth))
        got, _ = ft.drive(ft.ToneOps(engine, feed, case.wire), case.cuts, ft.collect_plan(depth, len(case.cuts)), depth, ft.TONE_MAX,
                          edges=edges)
    assert len(got) == len(case.cuts)
    for t, n in enumerate(case.cuts):
        per_ch = {}
        for c, d, b in sorted(got[t], key=lambda e: (e[0], e[2])):
            per_ch[c] = per_ch.get(c, "") + chr(d)
        assert per_ch == {c: s for c, s in enumerate(case.digits[t]) if s}, (kind, law, depth, "digits against the oracle", t, n)
        assert got[t] == want[t], (kind, law, depth, "entries against the serial path", t, n)
    # (test_feed_ticks.py holds these on the oracle's side; here, that they arrived)
    assert any(len(got[t]) for t in case.block_end_ticks())
    assert sum(len(g) for g in got) >= ft.TONE_CHANNELS//2


@pytest.mark.parametrize("law", [0, 1, 2], ids=["pcm", "alaw", "ulaw"])
def test_dtmf_feed_on_uneven_ticks(built, law):
    run_tone("dtmf", law, 3)


@pytest.mark.parametrize("depth", [1, 2, 8])
def test_dtmf_feed_at_other_depths(built, depth):
    run_tone("dtmf", 0, depth)


@pytest.mark.parametrize("kind", ["bell", "r2"])
def test_mf_feeds_on_uneven_ticks(built, kind):
    """Bell MF and R2 MF (forward) banks behind a feed.  (Their digit lists were empty before this test: the list kernel asked
    for BLK_CHANGE, which only the DTMF detector sets -- with 200 lines sending digits, not one entry in 50 ticks.)"""
    run_tone(kind, 0, 3)


# ---- echo ------------------------------------------------------------------------------------------------------------------
def run_echo(taps, mode, hpf, law, depth, edges=False):
    from spandsp_amd import engine
    case = ft.echo_case(taps, mode, hpf, law)
    what = (taps, hex(mode), hpf, law, depth)
    with ft.closing_in_order(engine.EchoBank(ft.N_CH, taps, mode)) as own:
        bank = own.objs[0]
        feed = own(engine.EchoFeed(bank, ft.XFEED_MAX, law=law, depth=depth, use_hpf_tx=hpf))
        got, said = ft.drive(ft.EchoOps(engine, feed, case.wire_tx, case.wire_rx), case.cuts, ft.collect_plan(depth, len(case.cuts)), depth,
                             ft.XFEED_MAX, hold=depth >= 5, edges=edges)
        assert said == case.cuts, (what, "samples per channel of the ticks collected")
        for t, n in enumerate(case.cuts):
            bad = np.nonzero(got[t] != case.clean[t])
            assert bad[0].size == 0, (what, "clean rows", t, n, bad[0][:4], bad[1][:4])
        echo_lines.compare_state(bank, case.dets, what)


@pytest.mark.parametrize("depth", [1, 2, 3, 8])
def test_echo_feed_on_uneven_ticks(built, depth):
    run_echo(128, 0x01, False, 0, depth)


@pytest.mark.parametrize("law", [0, 1, 2], ids=["pcm", "alaw", "ulaw"])
def test_echo_feed_full_mode_and_tx_hpf(built, law):
    run_echo(128, 0x67, True, law, 3)


def test_echo_feed_short_canceller_five_deep(built):
    run_echo(32, 0x01, False, 2, 5)


def test_echo_feed_rows_come_up_by_kernel(built, monkeypatch):
    monkeypatch.setenv("SPANGPU_FEED_D2H", "kernel")            # read when the feed is created
    run_echo(128, 0x67, True, 0, 3)


def test_echo_feed_on_plain_streams(built, monkeypatch):
    monkeypatch.setenv("SPANGPU_FEED_PRIORITY", "0")
    run_echo(128, 0x67, True, 2, 3)


# ---- modem -----------------------------------------------------------------------------------------------------------------
def modem_state_check(bank, state, what):
    from test_oracle_pin import bits
    for c in range(ft.N_CH):
        f, w = bank.get_state(c)
        bad = np.nonzero(w != state[c][1])[0]
        assert bad.size == 0, (what, "int words", c, bad[:8])
        bad = np.nonzero(bits(f) != state[c][0])[0]
        assert bad.size == 0, (what, "float words", c, bad[:8])


def run_modem(name, rate, depth, edges=False):
    from spandsp_amd import engine
    case = ft.modem_case(name, rate)                            # (sets the oracle's tables: use_golden_modem_tables())
    what = (name, rate, depth)
    with ft.closing_in_order(ft.modem_bank(engine, name, rate)) as own:
        bank = own.objs[0]
        feed = own(engine.ModemFeed(bank, ft.XFEED_MAX, rate, depth=depth))
        got, said = ft.drive(ft.ModemOps(engine, feed, case.sig), case.cuts, ft.collect_plan(depth, len(case.cuts)), depth, ft.XFEED_MAX,
                             hold=depth >= 5, edges=edges)
        assert said == case.cuts, (what, "samples per channel of the ticks collected")
        for t, n in enumerate(case.cuts):
            for c in range(ft.N_CH):
                assert np.array_equal(got[t][c], case.events[t][c]), (what, "events", t, n, c)
        modem_state_check(bank, case.state, what)


@pytest.mark.parametrize("depth", [1, 2, 3, 8])
def test_v29_feed_on_uneven_ticks(built, depth):
    run_modem("v29", 9600, depth)


@pytest.mark.parametrize("name,rate", ft.MODEMS[1:])
def test_modem_feeds_on_uneven_ticks(built, name, rate):
    run_modem(name, rate, 3)


def test_modem_feed_rows_come_up_by_dma(built, monkeypatch):
    monkeypatch.setenv("SPANGPU_FEED_D2H", "dma")
    run_modem("v29", 9600, 3)


def test_modem_feed_on_priority_streams(built, monkeypatch):
    monkeypatch.setenv("SPANGPU_FEED_PRIORITY", "1")
    run_modem("v17", 14400, 3)


@pytest.mark.parametrize("name,rate,max_samples", ft.SHORT_MODEMS)
def test_modem_feed_made_for_short_ticks(built, name, rate, max_samples):
    """A feed whose slots and packed rows are sized for ticks of 8 samples, or of one: it takes the bank over from a 400-sample feed
    once the receivers have trained, and brings back their data bits a few at a time."""
    from spandsp_amd import engine
    case = ft.short_modem_case(name, rate, max_samples)
    base = case.base
    what = (name, rate, max_samples)
    with ft.closing_in_order(ft.modem_bank(engine, name, rate)) as own:
        bank = own.objs[0]
        feed = engine.ModemFeed(bank, ft.XFEED_MAX, rate, depth=3)
        try:
            got, _ = ft.drive(ft.ModemOps(engine, feed, base.sig), base.cuts[:case.lead], ft.collect_plan(3, case.lead), 3, ft.XFEED_MAX)
        finally:
            feed.close()
        for t in range(case.lead):
            for c in range(ft.N_CH):
                assert np.array_equal(got[t][c], base.events[t][c]), (what, "lead", t, c)
        small = own(engine.ModemFeed(bank, max_samples, rate, depth=3))
        assert small.wpc < feed.wpc
        got, said = ft.drive(ft.ModemOps(engine, small, base.sig), case.cuts, ft.collect_plan(3, len(case.cuts)), 3, max_samples,
                             edges=True, origin=case.origin)
        assert said == case.cuts
        for t, n in enumerate(case.cuts):
            for c in range(ft.N_CH):
                assert np.array_equal(got[t][c], case.events[t][c]), (what, "events", t, n, c)
        modem_state_check(bank, case.state, what)


# ---- the tick loops in C -----------------------------------------------------------------------------------------------------
def fill_slots(ops, case, depth):
    """One tick into every slot (the first `depth` cuts over the poison), collected; -> what each slot now holds, whole rows."""
    held = []
    for t in range(depth):
        bufs = ops.acquire()
        for b in bufs:
            ft.poison(b, ops.law)
        ops.write(bufs, int(case.starts[t]), case.cuts[t])
        held.append([b.copy() for b in bufs])
        ops.commit(case.cuts[t])
    while ops.collect() is not None:
        pass
    return held


def written_out_loop(ops, samples, ticks, lag):
    got = []
    for _ in range(ticks):
        ops.acquire()                                           # the slot keeps what it holds
        ops.commit(samples)
        if ops.outstanding() > lag:
            got.append(ops.collect())
    while ops.outstanding():
        got.append(ops.collect())
    return got


def refused_runs(engine, ops, feed, samples, depth):
    with pytest.raises(engine.SpanGpuError):
        feed.run(samples, 1, depth)                             # lag must leave a slot free
    with pytest.raises(engine.SpanGpuError):
        feed.run(samples, 1, 0)
    ops.acquire()
    ops.commit(samples)
    with pytest.raises(engine.SpanGpuError):
        feed.run(samples, 1, 1)                                 # a tick outstanding
    assert ops.outstanding() == 1 and ops.collect() is not None and ops.collect() is None


@pytest.mark.parametrize("depth,lag,law", [(3, 2, 0), (5, 1, 2)])
def test_echo_feed_run_is_the_same_loop_in_c(built, depth, lag, law):
    """spangpu_echo_feed_run() over what the slots hold, with ticks shorter than the slots: the state of a second bank driven by
    the loop written out -- and of oracle cancellers fed the same rows."""
    from oracle import restated as orc
    from spandsp_amd import engine
    taps, mode, hpf, samples, ticks = 128, 0x67, True, 333, 11
    case = ft.echo_case(taps, mode, hpf, law)
    dets = [orc.EchoCan(taps, mode) for _ in range(ft.N_CH)]
    digests = []
    for use_c in (True, False):
        with ft.closing_in_order(engine.EchoBank(ft.N_CH, taps, mode)) as own:
            bank = own.objs[0]
            feed = own(engine.EchoFeed(bank, ft.XFEED_MAX, law=law, depth=depth, use_hpf_tx=hpf))
            ops = ft.EchoOps(engine, feed, case.wire_tx, case.wire_rx)
            held = fill_slots(ops, case, depth)
            if use_c:
                assert feed.run(samples, ticks, lag) > 0.0
                rows = [[ft.decode(law, x) if law else x for x in h] for h in held]
                for c, d in enumerate(dets):
                    for t in range(depth):
                        a, n = int(case.starts[t]), case.cuts[t]
                        d.run(case.tx[c, a:a + n], case.rx[c, a:a + n], hpf)
                    for i in range(ticks):
                        d.run(rows[i % depth][0][c, :samples], rows[i % depth][1][c, :samples], hpf)
            else:
                got = written_out_loop(ops, samples, ticks, lag)
                assert [n for _, n, _ in got] == [samples]*ticks
            echo_lines.compare_state(bank, dets, ("run" if use_c else "loop", depth, lag, law))
            digests.append([echo_lines.state_digest(bank, c) for c in range(ft.N_CH)])
            refused_runs(engine, ops, feed, samples, depth)
    assert digests[0] == digests[1]


@pytest.mark.parametrize("depth,lag", [(3, 2), (5, 1)])
def test_modem_feed_run_is_the_same_loop_in_c(built, depth, lag):
    from oracle import restated as orc
    from spandsp_amd import engine
    from test_oracle_pin import bits
    name, rate, samples, ticks = "v29", 9600, 333, 11
    case = ft.modem_case(name, rate)
    state = None
    words = []
    for use_c in (True, False):
        with ft.closing_in_order(ft.modem_bank(engine, name, rate)) as own:
            bank = own.objs[0]
            feed = own(engine.ModemFeed(bank, ft.XFEED_MAX, rate, depth=depth))
            ops = ft.ModemOps(engine, feed, case.sig)
            held = fill_slots(ops, case, depth)
            if use_c:
                ms, seen = feed.run(samples, ticks, lag)
                assert ms > 0.0 and seen >= 0
                state = []
                for c in range(ft.N_CH):
                    o = orc.V29(rate)
                    for t in range(depth):
                        a = int(case.starts[t])
                        o.rx(case.sig[c, a:a + case.cuts[t]])
                    for i in range(ticks):
                        o.rx(held[i % depth][0][c, :samples])
                    f, w = o.snapshot()
                    state.append((bits(f).copy(), w))
            else:
                got = written_out_loop(ops, samples, ticks, lag)
                assert [n for _, n, _ in got] == [samples]*ticks
            modem_state_check(bank, state, ("run" if use_c else "loop", depth, lag))
            words.append([np.concatenate([bits(f), w.view(np.uint32)]) for f, w in (bank.get_state(c) for c in range(ft.N_CH))])
            refused_runs(engine, ops, feed, samples, depth)
    assert all(np.array_equal(a, b) for a, b in zip(*words))


# ---- the edges of the contract -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("family", ["tone", "echo", "modem"])
def test_refusals_consume_no_slot_and_disturb_no_tick(built, family, depth):
    """commit(0), commit(max_samples + 1), acquire and commit with every slot taken, collect on an empty feed: every one an error
    return (or None), around every tick of a run that still equals the oracle's."""
    if family == "tone":
        run_tone("dtmf", 0, depth, edges=True)
    elif family == "echo":
        run_echo(128, 0x01, False, 0, depth, edges=True)
    else:
        run_modem("v29", 9600, depth, edges=True)


def test_feeds_refused_at_create(built):
    from spandsp_amd import engine
    with ft.closing_in_order(engine.ToneBank(engine.DTMF, 8), engine.EchoBank(8, 32, 0x01), engine.V29Bank(8, 9600)) as own:
        tone, echo, modem = own.objs
        for depth in (0, 9):
            with pytest.raises(engine.SpanGpuError):
                engine.Feed(tone, 160, depth=depth)
            with pytest.raises(engine.SpanGpuError):
                engine.EchoFeed(echo, 160, depth=depth)
            with pytest.raises(engine.SpanGpuError):
                engine.ModemFeed(modem, 160, 9600, depth=depth)
        with pytest.raises(engine.SpanGpuError):
            engine.Feed(tone, 1025, depth=2)                    # more blocks in a tick than an entry's block field counts
        with pytest.raises(engine.SpanGpuError):
            engine.Feed(tone, 160, depth=2, device=1)           # the bank lives on device 0
        # the largest and the smallest feeds there are: nothing to collect, and gone again
        for feed in (own(engine.Feed(tone, 1024, depth=8)), own(engine.EchoFeed(echo, 1, depth=1)), own(engine.ModemFeed(modem, 1, 9600, depth=8))):
            assert feed.collect() is None


def test_tone_feed_run_refusals(built):
    """spangpu_feed_run() with lag = depth, lag 0 and a tick outstanding: refused, and that tick is there to collect, once."""
    from spandsp_amd import engine
    case = ft.tone_case("dtmf", 0)
    with ft.closing_in_order(tone_bank(engine, "dtmf")) as own:
        feed = own(engine.Feed(own.objs[0], ft.TONE_MAX, depth=3))
        refused_runs(engine, ft.ToneOps(engine, feed, case.wire), feed, 160, 3)
        ms, digits = feed.run(160, 4, 2)
        assert ms > 0.0 and digits >= 0 and feed.outstanding() == 0


def other_family_refused(engine, echo_feed, modem_feed):
    """every echo call on the modem feed and every modem call on the echo feed: SPANGPU_ERR_BAD_ARG or NULL, nothing written,
    and neither feed's count of outstanding ticks moves"""
    import ctypes as C
    L = engine.lib()
    bad_arg = -2
    before = echo_feed.outstanding(), modem_feed.outstanding()
    a, b = C.c_void_p(), C.c_void_p()
    ms, bits = C.c_double(-1.0), C.c_longlong(-1)
    assert L.spangpu_echo_feed_acquire(modem_feed.h, C.byref(a), C.byref(b)) == bad_arg
    assert L.spangpu_echo_feed_commit(modem_feed.h, 160) == bad_arg
    assert L.spangpu_echo_feed_collect(modem_feed.h, C.byref(a)) == bad_arg
    assert L.spangpu_echo_feed_run(modem_feed.h, 160, 2, 1, C.byref(ms)) == bad_arg
    assert not L.spangpu_modem_feed_acquire(echo_feed.h)
    assert L.spangpu_modem_feed_commit(echo_feed.h, 160) == bad_arg
    assert L.spangpu_modem_feed_collect(echo_feed.h, C.byref(a), C.byref(b)) == bad_arg
    assert L.spangpu_modem_feed_run(echo_feed.h, 160, 2, 1, C.byref(ms), C.byref(bits)) == bad_arg
    assert not a.value and not b.value and ms.value == -1.0 and bits.value == -1
    assert (echo_feed.outstanding(), modem_feed.outstanding()) == before


def test_feeds_refuse_the_other_family(built):
    """An echo feed and a modem feed are one struct behind two names (include/spangpu.h).  The other family's calls are refused
    with nothing outstanding (where a run gets as far as its first commit) and around ticks in flight, and the ticks are the
    oracle's."""
    from spandsp_amd import engine
    taps, mode, ticks = 128, 0x01, 3
    ec, mc = ft.echo_case(taps, mode, False, 0), ft.modem_case("v29", 9600)
    with ft.closing_in_order(engine.EchoBank(ft.N_CH, taps, mode), ft.modem_bank(engine, "v29", 9600)) as own:
        echo_feed = own(engine.EchoFeed(own.objs[0], ft.XFEED_MAX, depth=3))
        modem_feed = own(engine.ModemFeed(own.objs[1], ft.XFEED_MAX, 9600, depth=3))
        sides = [(ft.EchoOps(engine, echo_feed, ec.wire_tx, ec.wire_rx), ec), (ft.ModemOps(engine, modem_feed, mc.sig), mc)]
        other_family_refused(engine, echo_feed, modem_feed)
        for t in range(ticks):
            for ops, case in sides:
                bufs = ops.acquire()
                for buf in bufs:
                    ft.poison(buf, 0)
                ops.write(bufs, int(case.starts[t]), case.cuts[t])
                ops.commit(case.cuts[t])
            other_family_refused(engine, echo_feed, modem_feed)
            assert echo_feed.outstanding() == t + 1 and modem_feed.outstanding() == t + 1
        for t in range(ticks):
            clean, n, _ = sides[0][0].collect()
            assert n == ec.cuts[t] and np.array_equal(clean, ec.clean[t]), ("clean rows", t)
            events, n, _ = sides[1][0].collect()
            assert n == mc.cuts[t]
            for c in range(ft.N_CH):
                assert np.array_equal(events[c], mc.events[t][c]), ("events", t, c)
        other_family_refused(engine, echo_feed, modem_feed)


# ---- a feed destroyed under its ticks ------------------------------------------------------------------------------------------
DESTROY_DEPTH = 3


def fill_and_destroy(engine, feed, ops, case):
    """A tick into every slot, none collected, and the feed destroyed: destroy waits for the way down, the bank and the way up
    before it frees, so it returns with the bank's state that of `depth` ticks."""
    for t in range(DESTROY_DEPTH):
        bufs = ops.acquire()
        for buf in bufs:
            ft.poison(buf, ops.law)
        ops.write(bufs, int(case.starts[t]), case.cuts[t])
        ops.commit(case.cuts[t])
    assert ops.outstanding() == DESTROY_DEPTH
    feed.close()
    assert not feed.h
    return int(case.starts[DESTROY_DEPTH]), case.cuts[DESTROY_DEPTH]


def test_tone_feed_destroyed_with_every_slot_taken(built):
    """... and the next tick through the serial path makes the records it makes behind `depth` serial ticks."""
    from spandsp_amd import engine
    case = ft.tone_case("dtmf", 0)
    want = serial_entries("dtmf", 0)[DESTROY_DEPTH]
    assert want
    with ft.closing_in_order(tone_bank(engine, "dtmf")) as own:
        bank = own.objs[0]
        feed = own(engine.Feed(bank, ft.TONE_MAX, depth=DESTROY_DEPTH))
        a, n = fill_and_destroy(engine, feed, ft.ToneOps(engine, feed, case.wire), case)
        bank.rx_host(case.wire[:, a:a + n])
        got = sorted((int(r["channel"]), int(r["code"]), int(r["block"])) for r in bank.blocks() if (r["flags"] & engine.BLK_CHANGE) and r["code"])
        assert got == want


def test_echo_feed_destroyed_with_every_slot_taken(built):
    from oracle import restated as orc
    from spandsp_amd import engine
    taps, mode = 128, 0x01
    case = ft.echo_case(taps, mode, False, 0)
    dets = [orc.EchoCan(taps, mode) for _ in range(ft.N_CH)]
    for t in range(DESTROY_DEPTH):
        a, n = int(case.starts[t]), case.cuts[t]
        for c, d in enumerate(dets):
            d.run(case.tx[c, a:a + n], case.rx[c, a:a + n], False)
    with ft.closing_in_order(engine.EchoBank(ft.N_CH, taps, mode)) as own:
        bank = own.objs[0]
        feed = own(engine.EchoFeed(bank, ft.XFEED_MAX, depth=DESTROY_DEPTH))
        a, n = fill_and_destroy(engine, feed, ft.EchoOps(engine, feed, case.wire_tx, case.wire_rx), case)
        echo_lines.compare_state(bank, dets, "behind a destroyed feed")
        clean = bank.update_host(case.tx[:, a:a + n], case.rx[:, a:a + n])
        assert np.array_equal(clean, case.clean_pcm[DESTROY_DEPTH])


def test_modem_feed_destroyed_with_every_slot_taken(built):
    from oracle import restated as orc
    from spandsp_amd import engine
    from test_oracle_pin import bits
    name, rate = "v29", 9600
    case = ft.modem_case(name, rate)
    state = []
    for c in range(ft.N_CH):
        o = orc.V29(rate)
        for t in range(DESTROY_DEPTH):
            a = int(case.starts[t])
            o.rx(case.sig[c, a:a + case.cuts[t]])
        f, w = o.snapshot()
        state.append((bits(f).copy(), w))
    with ft.closing_in_order(ft.modem_bank(engine, name, rate)) as own:
        bank = own.objs[0]
        feed = own(engine.ModemFeed(bank, ft.XFEED_MAX, rate, depth=DESTROY_DEPTH))
        a, n = fill_and_destroy(engine, feed, ft.ModemOps(engine, feed, case.sig), case)
        modem_state_check(bank, state, "behind a destroyed feed")
        bank.rx_host(case.sig[:, a:a + n])
        events = bank.events()
        for c in range(ft.N_CH):
            assert np.array_equal(events[c], case.events[DESTROY_DEPTH][c]), ("the next serial tick", c)
