"""The FAX transmit front-end banks on the GPU against tests/golden/faxtx.npz: what the reference's fax_modems sent under
fax_tx()'s loop, tick by tick -- the row, what fax_tx() returned, the SEND_STEP_COMPLETE and empty-queue underflow counts, the
handler installed afterwards and transmit -- and, at the end of a channel's case, the front-end words and the framer's words
and buffer.  Everything is compared for equality."""
import ctypes

import numpy as np
import pytest

import faxtx_cases as TC
from hdlc_cases import DeviceBytes

pytestmark = pytest.mark.gpu

N = 70          # two blocks of the 64-lane kernels, the last one partial; a partial second workgroup of the FSK and tone kernels
FILL = 0x5A5A   # what a row holds before a tick: nothing of it may survive inside the row, all of it outside


@pytest.fixture(scope="module")
def cases(built):
    return TC.load()[0]


class Line:
    """One channel's script as the bank's calls; remembers what it queued for the framer, for a move to another bank."""

    def __init__(self, c):
        self.c = c
        self.kind = None
        self.queued = []

    def begin(self, bank, ch):
        if int(self.c["cfg"][0]):
            bank.set_tep_mode(ch, True)

    def apply(self, bank, ch, t):
        from spandsp_amd import engine
        c = self.c
        for _, op, a, b, cc, d in TC.ops_of(c, t):
            if op == TC.SET:
                bank.set_tx_type(ch, a, b, cc, d)
                self.kind = {TC.V17: engine.V17, TC.V29: engine.V29, TC.V27TER: engine.V27TER}.get(a, self.kind)
            elif op == TC.RESTART:
                bank.restart(ch)
            elif op == TC.TEP:
                bank.set_tep_mode(ch, a)
            elif op == TC.Q_FRAME:
                self.queue(bank, ch, ("frame", c["frame_list"][a], b))
            elif op == TC.Q_FLAGS:
                self.queue(bank, ch, ("flags", a, 0))
            elif op == TC.Q_END:
                self.queue(bank, ch, ("end", 0, 0))
            elif op == TC.BITS:
                assert bank.fast_bank(self.kind).put_bits([c["bits"][a:a + b]], first=ch)[0] == b
            elif op == TC.EOD:
                bank.fast_bank(self.kind).end_of_data(ch)

    def queue(self, bank, ch, cmd, remember=True):
        fr = bank.framer()
        if cmd[0] == "frame":
            res = fr.frames([cmd[1]], first=ch, corrupt=[cmd[2]])
        elif cmd[0] == "flags":
            res = fr.flags(cmd[1], first=ch, n=1)
        else:
            res = fr.end(first=ch, n=1)
        assert res[0] == 0
        if remember:
            self.queued.append(cmd)


def check_tick(c, t, row, status, ch, where):
    lens, steps, under, handler, transmit = status
    assert np.array_equal(row, c["rows"][t]), (where, "row", int(np.argmax(row != c["rows"][t])))
    got = (int(lens[ch]), int(steps[ch]), int(under[ch]), int(handler[ch]), int(transmit[ch]))
    want = (int(c["lens"][t]), int(c["steps"][t]), int(c["under"][t]), int(c["handler"][t]), int(c["transmit"][t]))
    assert got == want, (where, got, want)


def check_end(bank, ch, c, where):
    from spandsp_amd import engine
    w = bank.get_words(ch)
    got = [int(w[engine.FAXTX_W_SIL_REMAINING]), int(w[engine.FAXTX_W_SIL_TOTAL]), int(w[engine.FAXTX_W_CURRENT_TX_TYPE]),
           int(w[engine.FAXTX_W_FAST_MODEM])]
    assert got == [int(x) for x in c["end"]], (where, got)
    fr = bank.framer()
    assert np.array_equal(fr.get_state(ch)[:16], c["hdlc"]), (where, "framer words")
    assert np.array_equal(fr.get_buffer(ch), c["buffer"]), (where, "framer buffer")


def run_plan(bank, group, samples, device_rows):
    """Channel ch runs case ch mod len(group), started ch // len(group) ticks late.  Returns the ticks compared."""
    plan = [(Line(group[ch % len(group)][1]), ch // len(group), group[ch % len(group)][0]) for ch in range(N)]
    total = max(int(line.c["cfg"][1]) + delay for line, delay, _ in plan) + 1
    stride = samples + 3                # no multiple of 8: rows start at every alignment
    dev = DeviceBytes(N*stride*2) if device_rows else None
    checked = 0
    for T in range(total):
        for ch, (line, delay, _) in enumerate(plan):
            t = T - delay
            if t == 0:
                line.begin(bank, ch)
            if 0 <= t < int(line.c["cfg"][1]):
                line.apply(bank, ch, t)
        if device_rows:
            dev.upload(np.full(N*stride, FILL, np.int16))
            bank.tx_device(dev.ptr, samples, stride)
            bank.sync()
            full = dev.download(np.int16).reshape(N, stride)
            assert (full[:, samples:] == FILL).all(), "a sample outside a row was written"
            rows = full[:, :samples]
        else:
            rows = bank.tx_host(samples)
        status = bank.status()
        for ch, (line, delay, name) in enumerate(plan):
            t = T - delay
            c = line.c
            if 0 <= t < int(c["cfg"][1]):
                check_tick(c, t, rows[ch], status, ch, (name, ch, t))
                checked += 1
                if t == int(c["cfg"][1]) - 1:
                    check_end(bank, ch, c, (name, ch))
            else:
                # a channel that has not started or has finished is silent and says nothing
                assert not rows[ch].any() and status[0][ch] == 0 and status[1][ch] == 0 and status[2][ch] == 0 and status[4][ch] == 0, (name, ch, t)
    if dev:
        dev.free()
    return checked


@pytest.mark.parametrize("device_rows", [False, True])
@pytest.mark.parametrize("samples", [160, 200, 163])
def test_every_case_tick_by_tick(cases, samples, device_rows):
    from spandsp_amd import engine
    group = [(name, c) for name, c in cases if int(c["cfg"][2]) == samples]
    assert group
    bank = engine.FaxTxFrontEnd(N, max_samples=samples)
    checked = run_plan(bank, group, samples, device_rows)
    assert checked == sum(int(group[ch % len(group)][1]["cfg"][1]) for ch in range(N))
    bank.close()


def move(src, dst, a, b, line):
    """One line from channel a of src to channel b of dst, through the words and the inner banks' state calls; what waits in the
    framer's queue is queued again."""
    from spandsp_amd import engine
    for tone in (engine.MCT_ANS, engine.MCT_FAX_CNG):
        dst.tone_bank(tone).set_state(b, src.tone_bank(tone).get_state(a))
    dst.v21_bank().set_state(b, src.v21_bank().get_state(a))
    for kind in (engine.V27TER, engine.V29, engine.V17):
        dst.fast_bank(kind).set_state(b, src.fast_bank(kind).get_state(a))
        dst.fast_bank(kind).set_ring(b, src.fast_bank(kind).get_ring(a))
    fs, fd = src.framer(), dst.framer()
    w = fs.get_state(a).copy()
    waiting = int(w[17])
    w[16] = 0
    w[17] = 0
    fd.set_state(b, w)
    fd.set_buffer(b, fs.get_buffer(a))
    for cmd in (line.queued[len(line.queued) - waiting:] if waiting else []):
        line.queue(dst, b, cmd, remember=False)
    dst.set_words(b, src.get_words(a))


@pytest.mark.parametrize("name,moves", [("v21_160", {2: 5, 40: 2}), ("v29_9600_hdlc", {2: 1, 20: 6})])
def test_a_line_moves_to_a_fresh_bank_in_mid_silence_and_mid_frame(cases, name, moves):
    """get_words / set_words and the inner banks' state calls: the line goes on identically."""
    from spandsp_amd import engine
    c = dict(cases)[name]
    line = Line(c)
    bank, ch = engine.FaxTxFrontEnd(8, max_samples=160), 3
    line.begin(bank, ch)
    moved = 0
    for t in range(int(c["cfg"][1])):
        if t in moves:
            # (in mid-silence the sender has not begun; in mid-frame the framer holds a frame and a position in it)
            w = bank.get_words(ch)
            assert (w[engine.FAXTX_W_HANDLER] == engine.FAXTX_SILENCE and w[engine.FAXTX_W_SIL_REMAINING] > 0) if moved == 0 \
                else (bank.framer().get_state(ch)[10] > 0)
            fresh = engine.FaxTxFrontEnd(8, max_samples=160)
            move(bank, fresh, ch, moves[t], line)
            bank.close()
            bank, ch = fresh, moves[t]
            moved += 1
        line.apply(bank, ch, t)
        rows = bank.tx_host(160)
        check_tick(c, t, rows[ch], bank.status(), ch, (name, t))
    check_end(bank, ch, c, name)
    assert moved == 2
    bank.close()


def test_refusals_change_nothing(cases):
    from spandsp_amd import engine
    L = engine.lib()
    bank = engine.FaxTxFrontEnd(4, kinds_mask=engine.FAXFE_V29, max_samples=160)
    bank.set_tx_type(1, engine.T30_MODEM_PAUSE, 0, 40, 0)
    before = bank.get_words(1).copy()
    assert L.spangpu_faxtx_set_tx_type(bank.h, 1, engine.T30_MODEM_V34HDX, 0, 0, 0) == -6
    assert L.spangpu_faxtx_set_tx_type(bank.h, 1, engine.T30_MODEM_V17, 14400, 0, 0) == -6        # not in kinds_mask
    assert L.spangpu_faxtx_set_tx_type(bank.h, 1, engine.T30_MODEM_V29, 14400, 0, 0) == -2        # a rate V.29 does not have
    assert L.spangpu_faxtx_set_tx_type(bank.h, 4, engine.T30_MODEM_V21, 300, 0, 1) == -2
    assert L.spangpu_faxtx_set_tx_type(bank.h, 1, 10, 0, 0, 0) == -2
    assert np.array_equal(bank.get_words(1), before)
    bad = before.copy()
    bad[engine.FAXTX_W_HANDLER] = engine.FAXTX_FAST
    bad[engine.FAXTX_W_FAST_MODEM] = engine.FAX_MODEM_V17_TX         # a bank this front end does not have
    assert L.spangpu_faxtx_set_words(bank.h, 1, bad.ctypes.data) == -2
    bad = before.copy()
    bad[engine.FAXTX_W_HANDLER] = engine.FAXTX_V21
    bad[engine.FAXTX_W_NEXT_HANDLER] = engine.FAXTX_FAST            # a next handler behind a sender
    assert L.spangpu_faxtx_set_words(bank.h, 1, bad.ctypes.data) == -2
    assert np.array_equal(bank.get_words(1), before)
    assert bank.fast_bank(engine.V17) is None and bank.fast_bank(engine.V29) is not None
    assert L.spangpu_faxtx_tx(bank.h, np.zeros((4, 161), np.int16).ctypes.data, 0, 161, 161) == -2
    assert L.spangpu_faxtx_set_stream(bank.h, None) == -2
    rows = bank.tx_host(160)
    assert not rows.any() and list(bank.status()[0]) == [0, 160, 0, 0]
    bank.close()


def test_loop_into_the_receive_front_end_on_one_stream(cases):
    """FaxTxFrontEnd rows in device memory feed FaxFrontEnd.rx_device; the receive bank's records per tick equal what the
    reference's receiving object said of the reference's sender."""
    from spandsp_amd import engine
    c = dict(cases)["loop"]
    hip = ctypes.CDLL("libamdhip64.so")
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
    tx = engine.FaxTxFrontEnd(N, kinds_mask=engine.FAXFE_V29, max_samples=160)
    rx = engine.FaxFrontEnd(N, kinds_mask=engine.FAXFE_V29, max_samples=160)
    tx.set_stream(stream)
    rx.set_stream(stream)
    dev = DeviceBytes(N*160*2)
    lines = [Line(c) for _ in range(N)]
    ticks = int(c["cfg"][1])
    delays = [ch % 3 for ch in range(N)]
    frames = 0
    for T in range(ticks + 2):
        for ch in range(N):
            t = T - delays[ch]
            if 0 <= t < ticks:
                lines[ch].apply(tx, ch, t)
                for op in c["rx_ops"]:
                    if op[0] == t and op[1] == 1:
                        rx.start_slow_modem(ch, int(op[2]))
                    elif op[0] == t:
                        rx.start_fast_modem(ch, int(op[2]), int(op[3]), bool(op[4]), bool(op[5]))
        tx.tx_device(dev.ptr, 160, 160)
        rx.rx_device(dev.ptr, 160, 160)
        got = rx.frames()
        handler, frx = rx.handlers()
        for ch in range(N):
            t = T - delays[ch]
            if not 0 <= t < ticks:
                continue
            want = []
            octets = TC.tick(c, "rx_bytes", t)
            at = 0
            for r in TC.tick(c, "rx_recs", t):
                r = int(r)
                if r < 0:
                    want.append(r)
                else:
                    want.append((r & 0xFFFF, bool(r >> 16), bytes(octets[at:at + (r & 0xFFFF)])))
                    at += r & 0xFFFF
            have = [x if isinstance(x, (int, np.integer)) else (int(x[0]), bool(x[1]), bytes(x[2])) for x in got[ch]]
            assert have == want, (ch, t, have, want)
            assert (int(handler[ch]), int(frx[ch])) == (int(c["rx_handler"][t]), int(c["rx_frx"][t])), (ch, t)
            frames += sum(1 for x in want if not isinstance(x, int) and x[1])
    assert frames == 4*N
    tx.close()
    rx.close()
    dev.free()
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    assert hip.hipStreamDestroy(stream) == 0
