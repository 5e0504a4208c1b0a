"""The HDLC framing banks on the GPU, for equality with what the reference's hdlc.c produced (tests/golden/hdlc.npz, written
by tests/golden/make_golden_hdlc.py).  Banks of 130 channels -- two full waves and a partial one; channel c runs fixture case
c mod n_cases and enters it (c div n_cases) mod 3 calls late, sitting the calls before that out, so the lanes of a wave sit
in different cases, branches and buffer positions.  Everything is integer arithmetic: no tolerance anywhere."""
import numpy as np
import pytest

import hdlc_cases as HC
from spandsp_amd import engine

pytestmark = pytest.mark.gpu

N = 130
HR_CRC_BYTES, HR_MAX_FRAME_LEN, HR_REPORT_BAD, HR_THRESHOLD, HR_INTERVAL, HR_LEN = 0, 1, 2, 3, 11, 12
HT_LEN, HT_POS, HT_Q_HEAD, HT_Q_COUNT = 10, 11, 16, 17


@pytest.fixture(scope="module")
def cases():
    return HC.load()


def late(c, n_cases):
    return (c//n_cases) % 3


def configure_rx(bank, c, case):
    """the case's hdlc_rx_init() arguments and settings on one channel of a bank created with others"""
    w = bank.get_state(c)
    w[HR_CRC_BYTES] = 4 if case.crc32 else 2
    w[HR_REPORT_BAD] = case.bad
    w[HR_THRESHOLD] = case.thr
    bank.set_state(c, w)
    if case.max_len >= 0:
        bank.set_max_frame_len(c, case.max_len)
    bank.set_octet_counting_report_interval(c, case.interval)


def unpack_bits(row, n):
    return np.unpackbits(row, bitorder="little")[:n]


def offer(bank, c, op):
    call, kind, arg, corrupt, res, data = op
    if kind == HC.FRAME:
        got = bank.frames([data], first=c, corrupt=[corrupt])
    elif kind == HC.FLAGS:
        got = bank.flags(arg, first=c, n=1)
    elif kind == HC.ABORT:
        got = bank.abort(first=c, n=1)
    else:
        got = bank.end(first=c, n=1)
    assert got[0] == res, (c, op[:5], got)


def test_sender_cases_equal_the_reference(built, cases):
    g, tx, rx, rxb = cases
    # one bank per (CRC, inter_frame_flags, depth) would put a case in every lane of a wave: instead the settings are words
    bank = engine.HdlcTxBank(N, crc32=False, inter_frame_flags=1, queue_depth=4)
    depth_of = {}
    for c in range(N):
        case = tx[c % len(tx)]
        w = bank.get_state(c)
        w[0], w[1] = (4 if case.crc32 else 2), case.iff
        w[12] = -1 if case.crc32 else 0xFFFF
        bank.set_state(c, w)
        depth_of[c] = case.depth
    # (the queue of the bank is 4 deep; a case recorded with 3 slots is offered its commands while 3 are queued at most)
    steps = max(c.calls for c in tx) + 2
    bits_seen = 0
    for t in range(steps):
        want = np.zeros(N, np.int32)
        for c in range(N):
            case = tx[c % len(tx)]
            k = t - late(c, len(tx))
            if 0 <= k < case.calls:
                for op in case.ops:
                    if op[0] == k:
                        if bank.queued(c) >= depth_of[c]:
                            assert op[4] == -1, (c, op[:5])
                        else:
                            offer(bank, c, op)
                want[c] = case.want(k)
        before = {c: bank.get_state(c) for c in (0, 5, N - 1) if want[c] == 0}
        bits, lens = bank.get_bits_host(want)
        events = bank.events()
        for c in range(N):
            case = tx[c % len(tx)]
            k = t - late(c, len(tx))
            if not 0 <= k < case.calls:
                assert lens[c] == 0 and not [e for e in events if e[0] == c], (c, t)
                continue
            assert lens[c] == case.lens[k], (c, k, lens[c], case.lens[k])
            assert np.array_equal(unpack_bits(bits[c], lens[c]), case.bits[k]), (c, k)
            mine = [kind for ch, kind in events if ch == c]
            expect = ([case.under[k]] if case.under[k] else []) + ([HC.END_OF_DATA] if case.ended[k] else [])
            assert mine == expect, (c, k, mine, expect)
            assert np.array_equal(bank.get_state(c)[:HC.TX_REF_WORDS], case.words[k]), (c, k)
            bits_seen += int(lens[c])
        for c, w in before.items():
            assert np.array_equal(bank.get_state(c), w), (c, t)
    assert bits_seen == sum(sum(tx[c % len(tx)].lens) for c in range(N))


def run_rx_bank(bank, case_of, elem=np.int16, octets=False, check_words=True):
    """every channel through its case; case_of(c) = (case, calls late)"""
    steps = max(case_of(c)[0].calls + case_of(c)[1] for c in range(N))
    delivered = 0
    for t in range(steps):
        active = {}
        for c in range(N):
            case, d = case_of(c)
            k = t - d
            if 0 <= k < case.calls:
                active[c] = (case, k)
                for call, value in case.midops:
                    if call == k:
                        bank.set_max_frame_len(c, value)
        cap = max(len(case.entries[k]) for case, k in active.values())
        if t % 2:
            cap = (cap + 15) & ~15          # rows of whole 16-byte pieces on odd steps, ragged ones on even steps
        rows = np.zeros((N, cap), np.uint8 if octets else elem)
        counts = np.zeros(N, np.int32)
        for c, (case, k) in active.items():
            counts[c] = len(case.entries[k])
            rows[c, :counts[c]] = case.entries[k]
        idle = [c for c in (1, 64, N - 1) if c not in active]
        before = {c: (bank.get_state(c), bank.get_buffer(c)) for c in idle}
        if octets:
            bank.put_host(rows, counts)
        else:
            bank.put_events_host(rows, counts)
        recs = bank.records()
        for c in range(N):
            if c not in active:
                assert recs[c] == [], (c, t)
                continue
            case, k = active[c]
            assert recs[c] == case.records[k], (case.name, c, k, recs[c], case.records[k])
            delivered += len(recs[c])
            if check_words:
                assert np.array_equal(bank.get_state(c), case.words[k]), (case.name, c, k)
            if k == case.calls - 1:
                assert np.array_equal(bank.get_stats(c), case.words[k][13:18]), (case.name, c)
                assert np.array_equal(bank.get_buffer(c), case.buffer), (case.name, c)
        for c, (w, b) in before.items():
            assert np.array_equal(bank.get_state(c), w) and np.array_equal(bank.get_buffer(c), b), (c, t)
    return delivered


def test_receiver_cases_equal_the_reference(built, cases):
    g, tx, rx, rxb = cases
    bank = engine.HdlcRxBank(N)
    for c in range(N):
        configure_rx(bank, c, rx[c % len(rx)])
    delivered = run_rx_bank(bank, lambda c: (rx[c % len(rx)], late(c, len(rx))))
    assert delivered == sum(sum(len(r) for r in rx[c % len(rx)].recs) for c in range(N)) > 0


def test_int8_int16_and_octet_forms_give_the_same_records(built, cases):
    g, tx, rx, rxb = cases
    # the streams that are whole octets of bits, cut into calls of whole octets: as events of either width, and as octets
    as_events = []
    for case in rxb:
        twin = HC.RxCase(g, [r.name for r in rx].index(case.name), octets=True)
        twin.entries = [np.unpackbits(e) for e in case.entries]
        as_events.append(twin)
    total = None
    for form in ("int8", "int16", "octets"):
        bank = engine.HdlcRxBank(N)
        src = rxb if form == "octets" else as_events
        for c in range(N):
            configure_rx(bank, c, src[c % len(src)])
        # (hdlc_rx_put_byte() keeps the coming bits in the low octet of raw_bit_stream: the words are the octet form's)
        got = run_rx_bank(bank, lambda c: (src[c % len(src)], late(c, len(src))), elem=np.int8 if form == "int8" else np.int16,
                          octets=(form == "octets"), check_words=(form == "octets"))
        assert total is None or got == total
        total = got
    assert total > 0


def test_state_and_buffer_move_to_a_fresh_bank_in_mid_frame(built, cases):
    g, tx, rx, rxb = cases
    # receiver: the long clean streams, stopped where a frame is under way
    case = next(c for c in rx if c.name == "clean_1_2")
    stop = next(k for k in range(20, case.calls) if case.words[k][HR_LEN] > 40)
    a = engine.HdlcRxBank(N, crc32=True, framing_ok_threshold=2)
    for k in range(stop + 1):
        rows = np.zeros((N, len(case.entries[k])), np.int16)
        rows[:] = case.entries[k]
        a.put_events_host(rows)
    b = engine.HdlcRxBank(N)
    for c in range(N):
        b.set_state(c, a.get_state(3))
        b.set_buffer(c, a.get_buffer(3))
    frames = 0
    for k in range(stop + 1, case.calls):
        rows = np.zeros((N, len(case.entries[k])), np.int16)
        rows[:] = case.entries[k]
        b.put_events_host(rows)
        recs = b.records()
        for c in (0, 63, 64, N - 1):
            assert recs[c] == case.records[k] and np.array_equal(b.get_state(c), case.words[k]), (c, k)
        assert all(r == recs[0] for r in recs)
        frames += len(recs[0])
    assert frames > 0
    # sender: stopped inside a frame with nothing queued; the moved channels go on as the ones left behind do (which
    # test_sender_cases_equal_the_reference holds to the reference)
    frame = bytes(range(256))[1:]
    a = engine.HdlcTxBank(N, crc32=True, inter_frame_flags=2, queue_depth=2)
    assert list(a.flags(3)) == [0]*N and list(a.frames([frame]*N)) == [0]*N
    for want in (331, 192, 9):
        a.get_bits_host(want)
    w = a.get_state(7)
    assert w[HT_LEN] == 255 and 0 < w[HT_POS] < 255 and w[HT_Q_COUNT] == 0
    b = engine.HdlcTxBank(N, queue_depth=2)
    for c in range(N):
        b.set_state(c, w)
        b.set_buffer(c, a.get_buffer(7))
    for k, want in enumerate((7, 331, 24, 331, 331, 331, 331, 331, 192, 1, 64)):
        if k == 3:
            assert list(a.frames([frame[:9]]*N, corrupt=[1]*N)) == [0]*N and list(b.frames([frame[:9]]*N, corrupt=[1]*N)) == [0]*N
        bits_a, lens_a = a.get_bits_host(want)
        bits_b, lens_b = b.get_bits_host(want)
        assert np.array_equal(lens_a, lens_b) and (lens_a == want).all() and np.array_equal(bits_a, bits_b), k
        assert (bits_a == bits_a[0]).all()
        assert a.events() == b.events()
        for c in (0, 64, N - 1):
            assert np.array_equal(a.get_state(c), b.get_state(c)), (c, k)
    assert a.get_state(0)[HT_LEN] == 0 and len(a.events()) == 0


def test_settings_of_one_channel_leave_its_neighbours_alone(built, cases):
    g, tx, rx, rxb = cases
    case = next(c for c in rx if c.name == "clean_0_1")
    bank = engine.HdlcRxBank(N)
    for k in range(12):
        rows = np.zeros((N, len(case.entries[k])), np.int16)
        rows[:] = case.entries[k]
        bank.put_events_host(rows)
    ref = bank.get_state(0)
    assert np.array_equal(ref, case.words[11]) and ref[HR_LEN] > 0
    bank.restart(65)
    bank.set_max_frame_len(66, 10)
    bank.set_octet_counting_report_interval(67, 20)
    for c in (0, 64, 68, N - 1):
        assert np.array_equal(bank.get_state(c), ref), c
    w = bank.get_state(65)
    changed = [i for i in range(HC.RX_WORDS) if w[i] != ref[i]]
    assert set(changed) <= {4, 5, 6, 7, 8, 9, 10, 12} and w[HR_LEN] == 0 and w[5] == 0 and w[6] == 0
    w = bank.get_state(66)
    assert w[HR_MAX_FRAME_LEN] == 12 and [i for i in range(HC.RX_WORDS) if w[i] != ref[i]] == [HR_MAX_FRAME_LEN]
    w = bank.get_state(67)
    assert w[HR_INTERVAL] == 20 and [i for i in range(HC.RX_WORDS) if w[i] != ref[i]] == [HR_INTERVAL]
    bank.set_max_frame_len(-1, 1000)
    assert all(bank.get_state(c)[HR_MAX_FRAME_LEN] == 404 for c in (0, 66, N - 1))
    # the sender's
    txb = engine.HdlcTxBank(N, queue_depth=2)
    assert list(txb.frames([b"\x01\x02\x03"]*N)) == [0]*N
    assert list(txb.flags(5)) == [0]*N and list(txb.abort()) == [-1]*N
    txb.get_bits_host(12)
    ref = txb.get_state(0)
    txb.restart(65)
    txb.set_max_frame_len(66, 2)
    for c in (0, 64, 67, N - 1):
        assert np.array_equal(txb.get_state(c), ref), c
    w = txb.get_state(65)
    assert w[HT_LEN] == 0 and w[HT_Q_COUNT] == 0 and txb.queued(65) == 0 and txb.queued(64) == 1
    assert list(txb.frames([b"\x01\x02\x03"]*3, first=65)) == [0, -1, 0]
    assert txb.get_state(66)[3] == 2
    # a frame as long as the buffer is taken, one octet more is not, and an overfull queue refuses
    big = engine.HdlcTxBank(2, queue_depth=1)
    assert list(big.frames([bytes(400), bytes(401)])) == [0, -1]
    assert list(big.frames([bytes(1), bytes(1)])) == [-1, 0]


def test_device_rows_in_and_out(built, cases):
    """the device forms: a sender's bits and lengths stay in device memory, and a receiver takes the block layout of
    spangpu_modem_copy_events() -- int32 counts[n], int8 events[n][per_channel] -- from there"""
    g, tx, rx, rxb = cases
    case = next(c for c in rx if c.name == "status")
    bank = engine.HdlcRxBank(N, report_bad_frames=True, framing_ok_threshold=2)
    per = 336
    dev = HC.DeviceBytes(4*N + N*per)
    for k in range(case.calls):
        n = len(case.entries[k])
        block = np.zeros(4*N + N*per, np.uint8)
        counts = np.full(N, n, np.int32)
        counts[5] = 0
        block[:4*N] = counts.view(np.uint8)
        ev = block[4*N:].view(np.int8).reshape(N, per)
        ev[:, :n] = case.entries[k].astype(np.int8)
        dev.upload(block)
        bank.put_modem_events(dev.ptr, per)
        recs = bank.records()
        assert recs[5] == [] and recs[4] == case.records[k] and recs[N - 1] == case.records[k], k
    assert np.array_equal(bank.get_state(N - 1), case.words[-1])
    dev.free()
    txc = tx[0]
    sender = engine.HdlcTxBank(N, crc32=bool(txc.crc32), inter_frame_flags=txc.iff, queue_depth=txc.depth)
    stride = 48
    bits, lens = HC.DeviceBytes(N*stride), HC.DeviceBytes(4*N)
    for k in range(12):
        for op in txc.ops:
            if op[0] == k:
                for c in (0, N - 1):
                    offer(sender, c, op)
        want = txc.want(k)
        sender.get_bits_device(bits.ptr, stride, want, lens.ptr)
        sender.sync()
        host, hl = bits.download().reshape(N, stride), lens.download(np.int32)
        for c in (0, N - 1):
            assert hl[c] == txc.lens[k] and np.array_equal(unpack_bits(host[c], hl[c]), txc.bits[k]), (c, k)
    bits.free()
    lens.free()


class Loop:
    """What the two device loops share: one stream for every bank, device rows for bits, PCM and events, the fixture's
    frames queued behind its preamble on every channel, and the comparison of a tick's records."""

    def __init__(self, g, which, per, elem_bytes):
        import ctypes
        self.ticks, self.preamble, self.crc32, self.thr = (int(x) for x in g["loop_%s_cfg" % which])
        ends = np.cumsum([0] + [int(x) for x in g["loop_%s_framelens" % which]])
        data = g["loop_%s_frames" % which].tobytes()
        self.frames = [data[ends[i]:ends[i + 1]] for i in range(len(ends) - 1)]
        nrecs = np.cumsum([0] + [int(x) for x in g["loop_%s_nrecs" % which]])
        recs, by, at = g["loop_%s_recs" % which], g["loop_%s_bytes" % which].tobytes(), 0
        self.records = []
        for t in range(self.ticks):
            out = []
            for r in recs[nrecs[t]:nrecs[t + 1]]:
                r = int(r)
                if r < 0:
                    out.append(r)
                else:
                    out.append((r & 0xFFFF, bool(r & 0x10000), by[at:at + (r & 0xFFFF)]))
                    at += r & 0xFFFF
            self.records.append(out)
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.stream = ctypes.c_void_p()
        assert self.hip.hipStreamCreate(ctypes.byref(self.stream)) == 0
        self.stride = 32                            # 256 bits a tick at the most (V.29 9600: 192)
        self.per = per
        self.bits, self.lens = HC.DeviceBytes(N*self.stride), HC.DeviceBytes(4*N)
        self.pcm = HC.DeviceBytes(N*160*2)
        self.block = HC.DeviceBytes(4*N + N*per*elem_bytes)
        self.sender = engine.HdlcTxBank(N, crc32=bool(self.crc32), inter_frame_flags=1, queue_depth=8)
        self.receiver = engine.HdlcRxBank(N, crc32=bool(self.crc32), framing_ok_threshold=self.thr)
        assert list(self.sender.flags(self.preamble)) == [0]*N
        for f in self.frames:
            assert list(self.sender.frames([f]*N)) == [0]*N
        self.delivered = []

    def on_one_stream(self, *banks):
        for b in (self.sender, self.receiver) + banks:
            b.set_stream(self.stream)

    def check(self, t):
        recs = self.receiver.records()
        assert recs[0] == self.records[t], (t, recs[0], self.records[t])
        # every channel carries the same call: replicas of one line
        assert all(r == recs[0] for r in recs), t
        self.delivered += [r[2] for r in recs[0] if not isinstance(r, int) and r[1]]

    def close(self, *banks):
        assert self.delivered == self.frames
        for b in (self.sender, self.receiver) + banks:
            b.sync()
            b.close()
        for d in (self.bits, self.lens, self.pcm, self.block):
            d.free()
        self.hip.hipStreamDestroy(self.stream)


def test_v21_loop_on_the_device_equals_the_reference(built, cases):
    """HDLC sender -> FSK sender's bit ring -> V.21 channel 2 -> FSK receiver, synchronous -> its events -> HDLC receiver:
    nothing but the record lists crosses to the host, and they are the reference's loop's, tick for tick."""
    g = cases[0]
    loop = Loop(g, "fsk", per=16, elem_bytes=2)
    tx = engine.FskTxBank(engine.FSK_V21CH2, N, bit_source=engine.FSKTX_QUEUE, queue_bits=256)
    rx = engine.FskBank(engine.FSK_V21CH2, N, engine.FSK_FRAME_MODE_SYNC)
    loop.on_one_stream(tx, rx)
    frac = 0
    for t in range(loop.ticks):
        want = engine.fsktx_bits_due(30000, frac, 160)
        frac = (frac + 160*30000) % 800000
        loop.sender.get_bits_device(loop.bits.ptr, loop.stride, want, loop.lens.ptr)
        tx.put_bits_device(loop.bits.ptr, loop.stride, loop.lens.ptr)
        tx.tx_device(loop.pcm.ptr, 160, 160)
        rx.rx_device(loop.pcm.ptr, 160, 160)
        rx.copy_events(loop.block.ptr, loop.block.n, loop.per)
        loop.receiver.put_events_device(loop.block.ptr.value + 4*N, 2, loop.per, loop.block.ptr)
        loop.check(t)
    assert loop.sender.events() == [] and tx.queued(0) == 0 and tx.queued(N - 1) == 0
    loop.close(tx, rx)


def test_v29_loop_on_the_device_equals_the_reference(built, cases):
    """HDLC sender -> V.29 sender's bit ring -> V.29 9600 -> V.29 receiver -> its events -> HDLC receiver, the training
    reports passing through the framer; bits per tick from the sender's cursor."""
    g = cases[0]
    loop = Loop(g, "v29", per=208, elem_bytes=1)
    tx = engine.V29TxBank(N, 9600, False, bit_source=engine.MODEMTX_QUEUE, queue_bits=512)
    rx = engine.V29Bank(N, 9600)
    loop.on_one_stream(tx, rx)
    cursor = engine.ModemTxCursor(engine.V29, 9600)
    for t in range(loop.ticks):
        want = cursor.advance(160)
        loop.sender.get_bits_device(loop.bits.ptr, loop.stride, want, loop.lens.ptr)
        tx.put_bits_device(loop.bits.ptr, loop.stride, loop.lens.ptr)
        tx.tx_device(loop.pcm.ptr, 160, 160)
        rx.rx_device(loop.pcm.ptr, 160, 160)
        rx.copy_events(loop.block.ptr.value, loop.block.n, loop.per)
        loop.receiver.put_modem_events(loop.block.ptr, loop.per)
        loop.check(t)
    assert tx.queued(0) == 0 and tx.queued(N - 1) == 0
    loop.close(tx, rx)
