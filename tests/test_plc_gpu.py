"""The packet loss concealment banks on the GPU, for equality with what the reference's plc.c produced (tests/golden/plc.npz,
written by tests/golden/make_golden_plc.py): rows and the 404 state words after every call, on the nine lines under the
fixture's schedule with every lane in step, staggered so that every tick mixes heard lines, gaps that go on and gaps that
start, and with one lone lane starting its gaps among lanes that only hear; what is written past a line's length; rows in
device memory and wide strides; state moved between lines in mid-gap, restart and the words set_state refuses; and conceal
behind a GSM 06.10 decoder bank on one stream.  The reference's float arithmetic is reproduced operation by operation: every
comparison is equality.

The base shape is 72 lines: a full wave and a partial one; line c runs fixture line c mod 9."""
import ctypes as C

import numpy as np
import pytest

import gsm0610_lines as GL
import plc_lines as PL
from spandsp_amd import engine
from test_g726_gpu import DevBytes

pytestmark = pytest.mark.gpu

N = 72
BAD = -2
SENT = np.int16(PL.SENTINEL)


@pytest.fixture(scope="module")
def fx():
    g = PL.load()
    return {"sched": PL.sched_cases(g), "heard": PL.heard_case(g), "dec": PL.dec_cases(g)}


def round8(n):
    return (n + 7) & ~7


def check_row(row, lost, n, want, who, most=None):
    """a row after its call: the samples, and what may have changed past them (of a host caller's row the call's max_samples
    come back, so nothing changes past those)"""
    assert np.array_equal(row[:n], want), (who, np.flatnonzero(row[:n] != want)[:4])
    if lost:
        # zeros up to the 16-byte boundary past the length, nothing beyond it
        edge = round8(n) if most is None else min(round8(n), most)
        assert not row[n:edge].any() and (row[edge:] == SENT).all(), who
    else:
        assert (row[n:] == SENT).all(), who


def run_ticks(bank, plan, ticks, most, device=None, stride=None):
    """plan[c] = (case, first tick): line c runs its case's calls from that tick on and sits out before and after.  Every tick's
    rows and, for every line, its state words against the fixture; a line that sits out keeps its row and its words."""
    n = bank.n
    width = most if stride is None else stride//2
    for k in range(ticks):
        rows = np.full((n, width), SENT, np.int16)
        lens = np.zeros(n, np.int32)
        lost = np.zeros(n, np.int32)
        calls = [None]*n
        for c, (case, first) in enumerate(plan):
            j = k - first
            if 0 <= j < len(case.calls):
                calls[c] = case.calls[j]
                lost[c], lens[c] = calls[c][0], calls[c][1]
                rows[c, :lens[c]] = calls[c][2]
        before = {c: bank.get_state(c) for c in range(n) if calls[c] is None}
        if device is None:
            out = bank.run_host(rows, most, lens, lost)
            assert out is rows
        else:
            device.put(rows)
            bank.run_device(device.ptr, 2*width, most, lens, lost)
            bank.sync()
            out = device.get((n, width), np.int16)
        for c in range(n):
            who = (plan[c][0].name, c, k)
            if calls[c] is None:
                assert (out[c] == SENT).all() and np.array_equal(bank.get_state(c), before[c]), who
                continue
            check_row(out[c], lost[c], lens[c], calls[c][3], who)
            got = bank.get_state(c)
            assert np.array_equal(got, calls[c][4]), (who, np.flatnonzero(got != calls[c][4])[:6])


MOST = max(n for _, n in PL.SCHEDULE)


@pytest.mark.parametrize("n", [N, 1])
def test_every_lane_together(built, fx, n):
    # (the one-line bank runs the voiced line)
    plan = [(fx["sched"][c % 9], 0) for c in range(N)] if n == N else [(fx["sched"][6], 0)]
    bank = engine.PlcBank(n)
    assert bank.words == PL.WORDS and not bank.get_state(0).any()
    run_ticks(bank, plan, len(PL.SCHEDULE), MOST)


def test_staggered(built, fx):
    plan = [(fx["sched"][c % 9], c % 4) for c in range(N)]
    # gap starts fall on 16 to 18 lanes of the full wave in the ticks where they fall on any, and every tick but the ends
    # mixes heard lines with lost ones
    starts = [k for k, (lost, _) in enumerate(PL.SCHEDULE) if lost and (k == 0 or not PL.SCHEDULE[k - 1][0])]
    per_tick = {}
    for c in range(64):
        for s in starts:
            per_tick[s + c % 4] = per_tick.get(s + c % 4, 0) + 1
    assert min(per_tick.values()) >= 16 and max(per_tick.values()) <= 2*18
    run_ticks(engine.PlcBank(N), plan, len(PL.SCHEDULE) + 3, MOST)


@pytest.mark.parametrize("lone", [37, 0, 63, 64])
def test_exactly_one_lane_starts(built, fx, lone):
    plan = [(fx["sched"][6] if c == lone else fx["heard"], 0) for c in range(N)]
    run_ticks(engine.PlcBank(N), plan, len(PL.SCHEDULE), MOST)


def test_rows_in_device_memory_and_wide_strides(built, fx):
    plan = [(fx["sched"][c % 9], 0) for c in range(N)]
    # host rows wider than the call: the sentinels of run_ticks reach to the row's end
    run_ticks(engine.PlcBank(N), plan, 8, MOST, stride=2*(MOST + 37))
    # rows in device memory, the row exactly (320 samples) and then 1024 bytes apart; every byte of the block is looked at
    for stride in (2*MOST, 1024):
        dev = DevBytes(N*stride)
        try:
            run_ticks(engine.PlcBank(N), plan, len(PL.SCHEDULE), MOST, device=dev, stride=stride)
        finally:
            dev.free()


def test_lens_and_lost_left_out(built, fx):
    """NULL lens: max_samples for all; NULL lost: nobody"""
    case = fx["sched"][7]
    bank = engine.PlcBank(N)
    for k in (0, 1):
        rows = np.tile(case.calls[k][2], (N, 1))
        out = bank.run_host(rows, 160)
        assert (out == case.calls[k][3]).all()
    assert all(np.array_equal(bank.get_state(c), case.calls[1][4]) for c in range(N))
    rows = np.full((N, 160), SENT, np.int16)
    out = bank.run_host(rows, 160, lost=np.ones(N, np.int32))
    want = case.calls[2]
    assert want[0] == 1 and (out == want[3]).all() and all(np.array_equal(bank.get_state(c), want[4]) for c in range(N))
    # a call nobody brings anything to, and one of no samples, change nothing
    before = bank.get_state(5)
    rows = np.full((N, 160), SENT, np.int16)
    bank.run_host(rows, 160, lens=np.zeros(N, np.int32), lost=np.ones(N, np.int32))
    bank.run_host(rows, 0)
    assert (rows == SENT).all() and np.array_equal(bank.get_state(5), before)


def test_state_moves_between_lines(built, fx):
    case = fx["sched"][6]
    bank = engine.PlcBank(N)
    other = engine.PlcBank(3)
    # line 3 up to the middle of the long gap (after its second fill-in), then on as line 70, and as line 1 of another bank
    cut = 19
    assert [lost for lost, _ in PL.SCHEDULE[cut - 2:cut + 2]] == [1, 1, 1, 1]
    plan = [(fx["heard"], 0)]*N
    plan[3] = (case, 0)
    run_ticks(bank, plan, cut, MOST)
    w = bank.get_state(3)
    assert w[PL.W_MISSING] == 320 and np.array_equal(w, case.calls[cut - 1][4])
    bank.set_state(70, w)
    other.set_state(1, w)
    assert np.array_equal(bank.get_state(70), w) and np.array_equal(other.get_state(1), w)
    for b, ch in ((bank, 70), (other, 1)):
        for lost, n, row, out, words in case.calls[cut:]:
            rows = np.full((b.n, round8(n) + 8), SENT, np.int16)
            rows[ch, :n] = row
            lens = np.zeros(b.n, np.int32)
            lens[ch] = n
            flags = np.full(b.n, lost, np.int32)
            b.run_host(rows, n, lens, flags)
            check_row(rows[ch], lost, n, out, (ch, n), most=n)
            assert np.array_equal(b.get_state(ch), words)
    # restart: plc_init()
    bank.restart(70)
    assert not bank.get_state(70).any() and bank.get_state(3).any()
    rows = np.full((N, 160), SENT, np.int16)
    rows[70] = case.calls[0][2]
    lens = np.zeros(N, np.int32)
    lens[70] = 160
    bank.run_host(rows, 160, lens)
    assert np.array_equal(bank.get_state(70), case.calls[0][4])


def test_set_state_refuses_words_no_concealer_holds(built, fx):
    bank = engine.PlcBank(8)
    good = fx["sched"][6].calls[2][4].copy()
    assert good[PL.W_MISSING] == 160 and 40 <= good[PL.W_PITCH] <= 120
    bank.set_state(2, good)
    L = engine.lib()

    def refused(edit):
        w = good.copy()
        edit(w)
        rc = L.spangpu_plc_set_state(bank.h, 2, w.ctypes.data)
        assert rc in (0, BAD) and np.array_equal(bank.get_state(2), good if rc == BAD else w)
        bank.set_state(2, good)
        return rc == BAD

    def put(i, v):
        def edit(w):
            w[i] = v
        return edit

    assert refused(put(PL.W_BUF_PTR, -1)) and refused(put(PL.W_BUF_PTR, 281))
    # (280 is what an append that exactly fills the ring leaves in the reference, and the fixture holds such words)
    assert any(w[PL.W_BUF_PTR] == 280 for c in fx["dec"] + [fx["heard"]] for _, _, _, _, w in c.calls)
    assert not refused(put(PL.W_BUF_PTR, 280))
    assert refused(put(PL.W_HISTORY + 7, 32768)) and refused(put(PL.W_HISTORY + 279, -32769))
    assert refused(put(PL.W_MISSING, -1))
    assert refused(put(PL.W_PITCH, 39)) and refused(put(PL.W_PITCH, 121))
    assert refused(put(PL.W_OFFSET, -1)) and refused(put(PL.W_OFFSET, int(good[PL.W_PITCH])))

    def idle(w):
        w[:PL.W_HISTORY] = 0

    def idle_offset(w):
        w[:PL.W_HISTORY] = 0
        w[PL.W_OFFSET] = 1

    # with nothing missing any pitch will do (plc_init() leaves 0), and then the offset is 0
    assert not refused(idle) and refused(idle_offset)
    for ch in (-1, 8):
        assert L.spangpu_plc_set_state(bank.h, ch, good.ctypes.data) == BAD and L.spangpu_plc_get_state(bank.h, ch, good.ctypes.data) == BAD
        assert L.spangpu_plc_restart(bank.h, ch) == BAD
    assert L.spangpu_plc_channels(bank.h) == 8


def test_bad_calls_are_refused_before_anything_is_queued(built, fx):
    bank = engine.PlcBank(8)
    L = engine.lib()
    good = fx["sched"][6].calls[2][4]
    for c in range(8):
        bank.set_state(c, good)
    rows = np.full((8, 160), SENT, np.int16)
    dev = DevBytes(8*320 + 64)
    counts = DevBytes(8*4)
    try:
        dev.put(rows)
        p, H, D = rows.ctypes.data, engine.MEM_HOST, engine.MEM_DEVICE
        lens = np.full(8, 160, np.int32)
        ones = np.ones(8, np.int32)
        table = [(None, H, 320, None, 160), (p, 7, 320, None, 160), (p, H, 320, None, -1), (p, H, 320, None, (1 << 24) + 1),
                 (p, H, 318, None, 160), (dev.ptr.value + 2, D, 320, None, 160), (dev.ptr, D, 328, None, 160), (dev.ptr, D, 304, None, 160),
                 (dev.ptr, D, 320, None, 161)]
        for amp, kind, stride, ln, most in table:
            assert L.spangpu_plc_run(bank.h, amp, kind, stride, ln, ones.ctypes.data, most) == BAD, (kind, stride, most)
        for bad in (161, -1):
            lens[5] = bad
            assert L.spangpu_plc_run(bank.h, p, H, 320, lens.ctypes.data, ones.ctypes.data, 160) == BAD
            assert L.spangpu_plc_conceal(bank.h, dev.ptr, 320, counts.ptr, lens.ctypes.data, 160, 160) == BAD
        ctable = [(None, 320, counts.ptr, 160, 160), (dev.ptr, 320, None, 160, 160), (dev.ptr, 320, counts.ptr, 161, 160),
                  (dev.ptr, 320, counts.ptr, -1, 160), (dev.ptr, 320, counts.ptr, 160, -1), (dev.ptr.value + 2, 320, counts.ptr, 160, 160),
                  (dev.ptr, 328, counts.ptr, 160, 160), (dev.ptr, 304, counts.ptr, 160, 160)]
        for amp, stride, cn, fill, most in ctable:
            assert L.spangpu_plc_conceal(bank.h, amp, stride, cn, None, fill, most) == BAD, (stride, fill, most)
        bank.sync()
        assert (rows == SENT).all() and (dev.get((8, 160), np.int16) == SENT).all()
        assert all(np.array_equal(bank.get_state(c), good) for c in range(8))
    finally:
        dev.free()
        counts.free()


def test_conceal_behind_a_decoder_on_one_stream(built, fx):
    """GSM 06.10 VoIP frames in, a length of 0 on the lost ticks; decode and conceal on one stream with nothing read on the
    host between them.  Line c runs decoded line c mod 5; the last line fills in nothing and so sits the lost ticks out."""
    pcm_all, codes_all = PL.load_gsm_pcm()
    cases = fx["dec"]
    idle = N - 1
    dec = engine.Gsm0610Bank(N, engine.GSM0610_DECODER, GL.VOIP)
    plc = engine.PlcBank(N)
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    dec.set_stream(stream)
    plc.set_stream(stream)
    cstride, pstride = 48, 2*PL.FRAME
    codes, pcm = DevBytes(N*cstride), DevBytes(N*pstride)
    fill = np.full(N, PL.FRAME, np.int32)
    fill[idle] = 0
    try:
        frame = 0
        pcm.put(np.full((N, PL.FRAME), SENT, np.int16))
        for k, lost in enumerate(PL.DEC_TICKS):
            rows = np.zeros((N, cstride), np.uint8)
            if not lost:
                for c in range(N):
                    rows[c, :33] = codes_all[c % 5][33*frame:33*(frame + 1)]
                frame += 1
            codes.put(rows)
            before = plc.get_state(idle)
            row_before = pcm.get((N, PL.FRAME), np.int16)[idle]
            dec.decode_device(codes.ptr, cstride, 33, pcm.ptr, pstride, lens=np.full(N, 0 if lost else 33, np.int32))
            # (all lines the same fill on the even ticks: the call's other form)
            if k % 2 == 0 or lost:
                plc.conceal(pcm.ptr, pstride, dec.counts_dev(), PL.FRAME, fill_lens=fill)
            else:
                plc.conceal(pcm.ptr, pstride, dec.counts_dev(), PL.FRAME, fill_samples=PL.FRAME)
            plc.sync()
            out = pcm.get((N, PL.FRAME), np.int16)
            for c in range(N - 1):
                call = cases[c % 5].calls[k]
                assert call[0] == lost and np.array_equal(out[c], call[3]), (c, k, np.flatnonzero(out[c] != call[3])[:4])
            if lost:
                assert np.array_equal(out[idle], row_before) and np.array_equal(plc.get_state(idle), before), k
            else:
                assert np.array_equal(out[idle], pcm_all[idle % 5][PL.FRAME*(frame - 1):PL.FRAME*frame]), k
            for c in list(range(0, N - 1, 7)) + [63, 64, 70]:
                assert np.array_equal(plc.get_state(c), cases[c % 5].calls[k][4]), (c, k)
        assert frame == 12
    finally:
        plc.close()
        dec.close()
        codes.free()
        pcm.free()
        hip.hipStreamDestroy(stream)
