"""The modem receivers' one-channel-per-lane kernels (csrc/v29_dev.hpp, v27ter_dev.hpp, v17_dev.hpp) off their fixed points.

spangpu_modem_rx() runs one of five launches per modem (modem_api.hip): the four-lane quad kernel (below 65 536 channels,
or under spangpu_tune_modem_mapping(4) at any size), the full-wave one-lane kernel <64, false, WPB, 16, true> (65 536
channels and more), the one-lane kernels <32> and <16> (mapping 1 below 65 536 channels) and <16, true> (the QAM tap on).
test_modem_offset_gpu.py proves the quads on impaired lines (carrier and clock offsets, failed training, ragged calls);
here the same lines go through every other launch, and the mapping is flipped between calls of one bank: the state words
(get_state / set_state, include/spangpu_refstate.h) are one interface, so either family must pick up where the other left
off.  Every channel's put_bit / status stream after every call and the state words (floats as bit patterns) must equal
the oracle's.  The mapping is process-wide: every test puts it back to 0, whatever happens."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import test_modem_offset_gpu as off
from test_oracle_pin import MODEM_OFFSET_CASES, MODEM_OFFSET_GOLDEN, bits, modem_offset_name, use_v17_tx_tables

pytestmark = pytest.mark.gpu

# test_offset_bank_matches_oracle's cases: (modem, bit rate, samples of signal, call lengths)
OFFSET_CASES = [("v29", 9600, 20000, (160,)), ("v29", 7200, 12000, (400, 3, 1, 97)), ("v29", 4800, 12000, (160,)),
                ("v27ter", 4800, 20000, (160,)), ("v27ter", 2400, 16000, (400, 3, 1, 97)),
                ("v17", 14400, 22000, (160,)), ("v17", 9600, 18000, (400, 3, 1, 97)), ("v17", 7200, 18000, (160,))]
ODD = [c for c in OFFSET_CASES if len(c[3]) > 1]            # one per modem: the odd-chunk schedule
N_CH = 70                                                   # 4 full waves of the <16> kernels and a ragged fifth
CHECK = [0, 1, 5, 9, 15, 16, 31, 32, 63, 64, N_CH - 1]

_cache = {}


@contextlib.contextmanager
def modem_mapping(mapping):
    from spandsp_amd import engine
    engine.tune_modem_mapping(mapping)
    try:
        yield
    finally:
        engine.tune_modem_mapping(0)


def offset_lines(name, bit_rate, n_ch, n_signal, seed):
    """offset_channels() and the per-line V.29 signal cutoffs test_offset_bank_matches_oracle gives them (level - 12 dB)."""
    key = ("lines", name, bit_rate, n_ch, n_signal, seed)
    if key not in _cache:
        sig, lines = off.offset_channels(name, bit_rate, n_ch, n_signal, seed)
        cutoffs = np.array([ln[4] - 12.0 for ln in lines], np.float32) if name == "v29" else None
        _cache[key] = (sig, lines, cutoffs)
    return _cache[key]


def offset_case(name, bit_rate, n_signal, chunks):
    """The 70-channel population of test_offset_bank_matches_oracle and every channel's oracle_calls(), computed once for
    all the tests of this module that use it."""
    key = ("want", name, bit_rate, n_signal, chunks)
    if key not in _cache:
        sig, lines, cutoffs = offset_lines(name, bit_rate, N_CH, n_signal, bit_rate + len(name))
        want = [off.oracle_calls(name, bit_rate, sig[c], chunks, None if cutoffs is None else cutoffs[c]) for c in range(N_CH)]
        _cache[key] = (sig, lines, cutoffs, want)
    return _cache[key]


def check_state(bank, c, want_f, want_w, what):
    f, w = bank.get_state(c)
    bad_w = np.nonzero(w != want_w)[0]
    assert bad_w.size == 0, what + ("int words", c, bad_w[:8])
    bad_f = np.nonzero(bits(f) != want_f)[0]
    assert bad_f.size == 0, what + ("float words", c, bad_f[:8])


def run_offset_case(name, bit_rate, n_signal, chunks, mapping_of_call, case=None):
    """Feed the population call by call, the mapping of call i being mapping_of_call(i); every channel's events after every
    call, the state words of CHECK every ninth call and whenever the mapping changes, of every channel at the end."""
    sig, lines, cutoffs, want = case or offset_case(name, bit_rate, n_signal, chunks)
    bank = off.make_bank(name, N_CH, bit_rate, cutoffs)
    trained, failed = set(), set()
    seen = set()
    k = i = 0
    try:
        while k < sig.shape[1]:
            n = chunks[i % len(chunks)]
            m = mapping_of_call(i)
            seen.add(m)
            with modem_mapping(m):
                bank.rx_host(sig[:, k:k + n])
            got = bank.events()
            for c in range(N_CH):
                assert np.array_equal(got[c], want[c][i][0]), (name, bit_rate, "events", c, i, m, lines[c])
                trained.update([c] if -4 in got[c] else [])
                failed.update([c] if -5 in got[c] else [])
            last = k + n >= sig.shape[1]
            if i % 9 == 0 or mapping_of_call(i + 1) != m or last:
                for c in (range(N_CH) if last else CHECK):
                    check_state(bank, c, want[c][i][1], want[c][i][2], (name, bit_rate, i, m, lines[c]))
            k += n
            i += 1
    finally:
        bank.close()
    # the population is what it claims to be: most lines train with their loops off centre, the far-off ones give up
    assert case is not None or len(trained) >= N_CH*3//4 and len(failed) >= N_CH//16, (len(trained), len(failed))
    return seen


@pytest.mark.parametrize("name,bit_rate,n_signal,chunks", OFFSET_CASES)
def test_offset_one_lane_kernels_match_oracle(built, name, bit_rate, n_signal, chunks):
    """test_offset_bank_matches_oracle under mapping 1: the <16> kernels, the last workgroup ragged."""
    use_v17_tx_tables(built)
    assert run_offset_case(name, bit_rate, n_signal, chunks, lambda i: 1) == {1}


@pytest.mark.parametrize("case", [MODEM_OFFSET_CASES[i] for i in MODEM_OFFSET_GOLDEN], ids=modem_offset_name)
def test_offset_golden_direct_one_lane(built, case):
    """The real reference's committed outputs on impaired lines straight against the <16> kernels."""
    with modem_mapping(1):
        off.test_offset_golden_direct(built, case)


# irregular stretches of calls, the mapping alternating 1, 4, 1, ...
FLIP_PERIODS = (3, 1, 7, 2, 5, 11, 1, 4, 9, 2, 6, 13, 1, 1, 8, 3)


def flip_mapping(i):
    edge = 0
    for j in range(10000):
        edge += FLIP_PERIODS[j % len(FLIP_PERIODS)]
        if i < edge:
            return 1 if j % 2 == 0 else 4
    return 1


@pytest.mark.parametrize("name,bit_rate,n_signal,chunks", ODD)
def test_mapping_flips_between_calls_match_one_oracle_run(built, name, bit_rate, n_signal, chunks):
    """One bank, its calls alternating between the one-lane kernels and the quads through training and data: each family
    picks up the other's state words mid-baud, mid-training and mid-data, and nothing shows (one uninterrupted oracle run)."""
    use_v17_tx_tables(built)
    assert run_offset_case(name, bit_rate, n_signal, chunks, flip_mapping) == {1, 4}


def garbage_case(name, bit_rate, n_signal, chunks):
    """The offset population with every third line, from a point in or after its training, hit by full-scale garbage (noise, a square wave, the
    line clipped): the equaliser runs away to infinity and on to NaN, and the state words hold NaNs (written back as the
    reference holds them, 0xFFC00000)."""
    key = ("garbage", name, bit_rate, n_signal, chunks)
    if key not in _cache:
        sig, lines, cutoffs = offset_lines(name, bit_rate, N_CH, n_signal, bit_rate + len(name))
        sig = sig.copy()
        rng = np.random.default_rng(bit_rate + 17)
        onset = 9000 if name == "v17" else 6000             # (after V.29's and V.17's training, in V.27ter 2400's)
        for c in range(0, N_CH, 3):
            x = sig[c, onset:]
            kind = (c//3) % 3
            if kind == 0:
                x[:] = rng.integers(-32768, 32768, len(x))
            elif kind == 1:
                x[:] = np.where((np.arange(len(x))//3) % 2, 32767, -32768)
            else:
                x[:] = np.clip(x.astype(np.int32)*60, -32768, 32767)
        want = [off.oracle_calls(name, bit_rate, sig[c], chunks, None if cutoffs is None else cutoffs[c]) for c in range(N_CH)]
        n_nan = sum(bool(np.any((w[-1][1] & 0x7FFFFFFF) > 0x7F800000)) for w in want)
        _cache[key] = ((sig, lines, cutoffs, want), n_nan)
    return _cache[key]


@pytest.mark.parametrize("flips", [False, True], ids=["one_lane", "flips"])
@pytest.mark.parametrize("name,bit_rate,n_signal,chunks", ODD)
def test_runaway_equalisers_nan_state_words(built, name, bit_rate, n_signal, chunks, flips):
    """Receivers whose equaliser has run away: the events of a NaN-filled receiver and its NaN state words (bit for bit)
    from the one-lane kernels, and -- with the mapping flipped between calls -- NaN words handed from one family to the
    other."""
    use_v17_tx_tables(built)
    case, n_nan = garbage_case(name, bit_rate, n_signal, chunks)
    assert n_nan >= N_CH//6, n_nan                           # the population is what it claims to be
    seen = run_offset_case(name, bit_rate, n_signal, chunks, flip_mapping if flips else (lambda i: 1), case)
    assert seen == ({1, 4} if flips else {1})


def _orc_restart(name, o, bit_rate, train_flag):
    from oracle.restated import lib as olib
    if name == "v29":
        return olib().orc_v29_restart(o.p, bit_rate, train_flag)
    if name == "v27ter":
        return olib().orc_v27ter_restart(o.p, bit_rate, train_flag)
    return o.restart(bit_rate, train_flag)


# (modem, bank rate, samples of signal, rate of the restart_ex channels)
VAR_CASES = [("v29", 9600, 12000, 7200), ("v27ter", 4800, 12000, 4800), ("v17", 14400, 20000, 14400)]


@pytest.mark.parametrize("name,bit_rate,n_signal,ex_rate", VAR_CASES)
def test_one_lane_var_ticks_and_restarts_match_oracle(built, name, bit_rate, n_signal, ex_rate):
    """spangpu_modem_rx_var() on the <16> kernels with the offset lines: channels that sit ticks out (a whole wave of them
    now and then), short frames of 1, 3 and 97 samples (lanes entering a baud-aligned round mid-baud), spangpu_modem_restart()
    of a few channels mid-stream, spangpu_modem_restart_ex() of others -- V.29 to another rate, V.27ter and V.17 with their
    train flag (V.17's short train; a V.17 or V.27ter bank runs one rate, the library refuses another).  Every channel is held
    against an oracle receiver fed its own calls only.  spangpu_modem_fillin() is not here: the oracle has no fill-in of the
    modem receivers to follow it with (tests/test_loud_modems_gpu.py holds it to the reference's recorded results)."""
    from spandsp_amd import engine
    use_v17_tx_tables(built)
    sig, lines, cutoffs = offset_lines(name, bit_rate, N_CH, n_signal, seed=bit_rate + 3*len(name) + 1)
    dets = [off.make_oracle(name, bit_rate, None if cutoffs is None else cutoffs[c]) for c in range(N_CH)]
    bank = off.make_bank(name, N_CH, bit_rate, cutoffs)
    rng = np.random.default_rng(bit_rate + 11)
    n_ticks = sig.shape[1]//160
    restart_at, restart_ch = n_ticks*2//5, (2, 17, 33, 50, N_CH - 1)
    ex_at, ex_ch = n_ticks*3//5, (7, 40, 64)
    pos = np.zeros(N_CH, np.int64)
    total = short = sat_out = 0
    trained = set()
    tick = 0
    try:
        with modem_mapping(1):
            while (pos < sig.shape[1]).any() and tick < 3*n_ticks:
                lens = np.where(rng.random(N_CH) < 0.15, 0, 160)
                if tick % 3 == 1:
                    pick = rng.random(N_CH) < 0.25
                    lens[pick] = rng.choice([1, 3, 97], int(pick.sum()))
                if tick % 7 == 3:
                    lens[16:32] = 0                 # a whole wave of the <16> kernels sits the tick out
                lens = np.minimum(lens, sig.shape[1] - pos).astype(np.int32)
                frames = rng.integers(-9000, 9000, (N_CH, 160)).astype(np.int16)       # beyond lens[c] a row is never read
                for c in range(N_CH):
                    frames[c, :lens[c]] = sig[c, pos[c]:pos[c] + lens[c]]
                if lens.any():
                    bank.rx_host_var(frames, lens)
                    got = bank.events()
                    for c in range(N_CH):
                        d = dets[c]
                        d.sink.clear()
                        if lens[c]:
                            d.rx(sig[c, pos[c]:pos[c] + lens[c]])
                        want = d.sink.events()["a"].astype(np.int8)
                        assert np.array_equal(got[c], want), (name, "events", c, tick, int(lens[c]), lines[c])
                        total += len(want)
                        trained.update([c] if -4 in want else [])
                short += int(np.count_nonzero((lens > 0) & (lens < 160)))
                sat_out += int(np.count_nonzero(lens == 0))
                pos += lens
                if tick == restart_at:
                    for c in restart_ch:
                        bank.restart(c)
                        assert _orc_restart(name, dets[c], bit_rate, 0) == 0
                if tick == ex_at:
                    for c in ex_ch:
                        assert engine.lib().spangpu_modem_restart_ex(bank.h, c, ex_rate, 1) == 0
                        assert _orc_restart(name, dets[c], ex_rate, 1) == 0
                if tick % 10 == 0 or tick in (restart_at, ex_at):
                    for c in CHECK + list(restart_ch + ex_ch):
                        fo, wo = dets[c].snapshot()
                        check_state(bank, c, bits(fo), wo, (name, tick))
                tick += 1
        for c in range(N_CH):
            fo, wo = dets[c].snapshot()
            check_state(bank, c, bits(fo), wo, (name, "end"))
    finally:
        bank.close()
    assert total > 100*N_CH and short > 5*N_CH and sat_out > 20*N_CH, (total, short, sat_out)
    assert len(trained) >= N_CH//2, len(trained)


QAM_CASES = [("v29", 7200, 12000, (160, 400, 3, 1, 97)), ("v27ter", 2400, 16000, (160, 400, 3, 1, 97)),
             ("v17", 9600, 18000, (160, 400, 3, 1, 97))]


@pytest.mark.parametrize("name,bit_rate,n_signal,chunks", QAM_CASES)
def test_qam_tap_kernel_on_offset_lines(built, name, bit_rate, n_signal, chunks):
    """<16, true> (the kernel every bank runs once its QAM tap is on) on the offset lines: every channel's qam_report calls
    (constellation point and target as bit patterns; V.27ter's timing hop reports, more of them with the clock off) at the
    reference's place in the put_bit stream, the events and the state words."""
    from oracle import restated as orc
    use_v17_tx_tables(built)
    n_ch = 45
    sig, lines, cutoffs = offset_lines(name, bit_rate, n_ch, n_signal, seed=bit_rate + 5*len(name) + 2)
    orcs = [off.make_oracle(name, bit_rate, None if cutoffs is None else cutoffs[c]) for c in range(n_ch)]
    for o in orcs:
        o.tap_qam()
    bank = off.make_bank(name, n_ch, bit_rate, cutoffs)
    bank.qam_tap(True)
    k = i = 0
    n_rep = hops = 0
    try:
        while k < sig.shape[1]:
            n = chunks[i % len(chunks)]
            bank.rx_host(sig[:, k:k + n])
            got_ev = bank.events()
            got_q = bank.qam_reports()
            for c, o in enumerate(orcs):
                o.sink.clear()
                o.rx(sig[c, k:k + n])
                ev = o.sink.events()
                assert np.array_equal(got_ev[c], ev["a"][ev["kind"] == 3].astype(np.int8)), (name, bit_rate, "events", c, i, lines[c])
                want = orc.qam_stream(ev)
                assert got_q[c].shape == want.shape, (name, bit_rate, "report count", c, i, got_q[c].shape, want.shape, lines[c])
                bad = np.nonzero(np.any(got_q[c] != want, axis=1))[0]
                assert bad.size == 0, (name, bit_rate, "reports", c, i, bad[:4], got_q[c][bad[:2]], want[bad[:2]], lines[c])
                n_rep += len(want)
                hops += int(np.count_nonzero(want[:, 1]))
            if i % 9 == 0 or k + n >= sig.shape[1]:
                for c in (0, 5, 9, 16, n_ch - 1):
                    fo, wo = orcs[c].snapshot()
                    check_state(bank, c, bits(fo), wo, (name, bit_rate, "state", i))
            k += n
            i += 1
    finally:
        bank.close()
    assert n_rep > 500*n_ch, n_rep
    if name == "v27ter":
        assert hops > 0


# ---- bank scale: the full-wave kernels, the forced quads above 64 K channels, the <32> kernels -----------------------------
V_LINES = 61
# (modem, bit rate, samples of signal): rates the nominal full-size tests (test_full_size_gpu.py) do not run
SCALE_CASES = [("v29", 7200, 12000), ("v27ter", 2400, 12000), ("v17", 9600, 14000)]
FULL_WAVE_CH = {"v29": 65536 + 64*4 + 5, "v27ter": 65536 + 64*4 + 5, "v17": 65536 + 64 + 50}
QUAD_STRETCH = range(44, 60)            # calls of the full-wave bank that run under mapping 4
VAR_TICK = 30


def scale_plan(n_total):
    """Per call, the samples each of the V lines takes: mostly 160, ragged calls in training and in data, and one tick in
    which a line's replicas sit out or take a short frame by the line's index (one oracle run per line holds for them all)."""
    ragged = {5: 400, 6: 3, 7: 1, 8: 97, 70: 3, 71: 1, 72: 97, 73: 400}
    v = np.arange(V_LINES)
    plan = []
    done = 0
    while done < n_total:
        i = len(plan)
        if i == VAR_TICK:
            plan.append(np.where(v % 4 == 1, 0, np.where(v % 4 == 2, 97, 160)))
        else:
            plan.append(np.full(V_LINES, ragged.get(i, 160)))
        done += int(plan[-1].max())
    return plan


def scale_case(name, bit_rate, n_signal):
    """The V distinct offset lines and each line's oracle run through scale_plan(): per call a [V, width] matrix of the
    events and their counts, the state words."""
    key = ("scale", name, bit_rate, n_signal)
    if key not in _cache:
        sig, lines, cutoffs = offset_lines(name, bit_rate, V_LINES, n_signal, seed=bit_rate + 7*len(name) + 3)
        plan = scale_plan(sig.shape[1])
        base = np.concatenate([sig, np.zeros((V_LINES, 512), np.int16)], axis=1)
        dets = [off.make_oracle(name, bit_rate, None if cutoffs is None else cutoffs[v]) for v in range(V_LINES)]
        pos = np.zeros(V_LINES, np.int64)
        calls = []
        trained, failed = set(), set()
        for lens in plan:
            n = int(lens.max())
            frames = np.zeros((V_LINES, n), np.int16)
            evs = []
            for v, o in enumerate(dets):
                frames[v, :lens[v]] = base[v, pos[v]:pos[v] + lens[v]]
                o.sink.clear()
                if lens[v]:
                    o.rx(frames[v, :lens[v]])
                evs.append(o.sink.events()["a"].astype(np.int8))
                trained.update([v] if -4 in evs[-1] else [])
                failed.update([v] if -5 in evs[-1] else [])
            counts = np.array([len(e) for e in evs], np.int32)
            rows = np.zeros((V_LINES, max(1, counts.max())), np.int8)
            for v, e in enumerate(evs):
                rows[v, :len(e)] = e
            snaps = [o.snapshot() for o in dets]
            calls.append((lens, frames, counts, rows, [bits(f) for f, _ in snaps], [w for _, w in snaps]))
            pos += lens
        assert len(trained) >= V_LINES*3//4 and len(failed) >= V_LINES//16, (len(trained), len(failed))
        _cache[key] = (lines, cutoffs, calls)
    return _cache[key]


def raw_events(bank):
    """spangpu_modem_events() as it comes: counts[n_ch] and the [n_ch, cap] matrix."""
    from spandsp_amd import engine
    ev = C.c_void_p()
    cnt = C.c_void_p()
    cap = engine._check(engine.lib().spangpu_modem_events(bank.h, C.byref(ev), C.byref(cnt)))
    counts = np.frombuffer((C.c_char*(4*bank.n)).from_address(cnt.value), dtype=np.int32).copy()
    raw = np.frombuffer((C.c_char*(cap*bank.n)).from_address(ev.value), dtype=np.int8).reshape(bank.n, cap)
    return counts, raw


def run_scale_case(name, bit_rate, n_signal, n_ch, mapping_of_call, state_ch):
    """Every channel c replays line pick[c] = (7c) % V; every channel's events of every call against its line's, in one
    vectorised comparison, and the state words of state_ch whenever the mapping changes and at the end."""
    use_v17_tx_tables(True)
    lines, cutoffs, calls = scale_case(name, bit_rate, n_signal)
    pick = (np.arange(n_ch)*7) % V_LINES
    bank = off.make_bank(name, n_ch, bit_rate, None if cutoffs is None else cutoffs[pick])
    seen = set()
    try:
        for i, (lens, frames, counts, rows, fwords, iwords) in enumerate(calls):
            m = mapping_of_call(i)
            seen.add(m)
            with modem_mapping(m):
                if (lens == lens.max()).all():
                    bank.rx_host(frames[pick])
                else:
                    bank.rx_host_var(frames[pick], lens[pick])
            got_n, raw = raw_events(bank)
            bad = np.flatnonzero(got_n != counts[pick])
            assert bad.size == 0, (name, bit_rate, n_ch, "event counts", i, m, bad[:8], got_n[bad[:4]], counts[pick[bad[:4]]])
            w = int(counts.max())
            assert raw.shape[1] >= w
            if w:
                diff = (raw[:, :w] != rows[pick, :w]) & (np.arange(w)[None, :] < got_n[:, None])
                bad = np.flatnonzero(diff.any(axis=1))
                assert bad.size == 0, (name, bit_rate, n_ch, "events", i, m, bad[:8], lines[pick[bad[0]]])
            if i + 1 == len(calls) or mapping_of_call(i + 1) != m or i == VAR_TICK:
                for c in state_ch:
                    check_state(bank, c, fwords[pick[c]], iwords[pick[c]], (name, bit_rate, n_ch, i, m))
    finally:
        bank.close()
    return seen


def spread(n_ch, fixed):
    return sorted(set(fixed + [n_ch - 1] + list(np.linspace(1, n_ch - 2, 30).astype(int))))


@pytest.mark.parametrize("name,bit_rate,n_signal", SCALE_CASES)
def test_full_wave_kernels_on_offset_lines(built, name, bit_rate, n_signal):
    """The full-wave one-lane kernels on a bank that fills neither its last workgroup nor its last wave, the impaired lines
    at a rate the nominal full-size tests leave out, ragged calls and a var tick; for a stretch of calls in the middle the
    same bank runs the quads (mapping 4 holds at every size), then the full-wave kernels again."""
    n_ch = FULL_WAVE_CH[name]
    seen = run_scale_case(name, bit_rate, n_signal, n_ch, lambda i: 4 if i in QUAD_STRETCH else 0,
                          spread(n_ch, [0, 63, 64, 65535, 65536]))
    assert seen == {0, 4}


@pytest.mark.parametrize("name,bit_rate,n_signal", SCALE_CASES)
def test_one_lane_32_kernels_on_offset_lines(built, name, bit_rate, n_signal):
    """Mapping 1 between 32 768 and 65 535 channels: the <32> kernels, the last wave ragged."""
    n_ch = 32768 + 37
    assert run_scale_case(name, bit_rate, n_signal, n_ch, lambda i: 1, spread(n_ch, [0, 31, 32, 63, 64, 32767, 32768])) == {1}
