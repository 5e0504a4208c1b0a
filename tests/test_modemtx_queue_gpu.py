"""The modem transmitter banks carrying a caller's data (bit source SPANGPU_MODEMTX_QUEUE) and the v29_tx / v27ter_tx / v17_tx
entry points by name, against live objects of the real reference fed the same bits: every int16 sample, every returned length,
every status call and state words 0 .. 30 equal, no tolerance."""
import ctypes

import numpy as np
import pytest

import modemtx_ref as mr

pytestmark = pytest.mark.gpu

# training_step (state word 25) at the end of the training and at the end of the shutdown
TRAINING_END = {"v29": 480 + 48 + 128 + 384 + 48, "v27ter": 320 + 32 + 50 + 1074 + 8, "v17": 528 + 256 + 2976 + 64 + 48}
SHUTDOWN_END = {"v29": TRAINING_END["v29"] + 32, "v27ter": TRAINING_END["v27ter"] + 32, "v17": TRAINING_END["v17"] + 32 + 48}


def make_bank(engine, modem, n, bit_rate, tep, queue_bits):
    cls = {"v29": engine.V29TxBank, "v27ter": engine.V27terTxBank, "v17": engine.V17TxBank}[modem]
    return cls(n, bit_rate, tep, bit_source=engine.MODEMTX_QUEUE, queue_bits=queue_bits)


@pytest.mark.parametrize("modem,bit_rate,tep,short_train", mr.CASES)
def test_queue_bank_equals_reference_objects(built, modem, bit_rate, tep, short_train):
    """70 channels (a full wave and a partial block) on rings of 64 bits, which wrap and run dry: payloads of every length
    around a symbol's edge arrive in pieces between the calls, some channels sit out a round and idle on ones mid-data, and
    each channel is told of the end of its data once its last piece is in.  Every call and every channel is compared, to three
    calls past the last channel's shutdown; then two channels are restarted with bits still in their rings."""
    from spandsp_amd import engine
    n = 70
    bps = mr.BITS_PER_SYMBOL[(modem, bit_rate)]
    rng = np.random.default_rng(bit_rate + len(modem) + tep)
    lengths = [0, 1, bps - 1, bps, 37, 203, 64, 65, 100, 500]
    pending = [list(rng.integers(0, 2, lengths[c % 10] + (c//10 if c % 10 >= 4 else 0))) for c in range(n)]
    bank = make_bank(engine, modem, n, bit_rate, tep, 64)
    feeds = [mr.BitFeed() for _ in range(n)]
    status = [[] for _ in range(n)]
    refs = [mr.RefModemTx(modem, bit_rate, tep, feeds[c], status[c].append) for c in range(n)]
    if short_train:
        for c in range(n):
            bank.restart(c, bit_rate, tep, short_train=True)
            refs[c].restart(bit_rate, tep, True)
    told = [False]*n
    quiet = np.zeros(n, int)            # calls that returned 0
    phases = {"data": 0, "shutdown": 0, "after": 0}
    seen_all = set()

    def one_call(k, m):
        pcm, lens = bank.tx(m, lens=True)
        ev = bank.events()
        for c in range(n):
            del status[c][:]
            want, got = refs[c].tx(m)
            assert lens[c] == got, (k, c, lens[c], got)
            assert np.array_equal(pcm[c], want), (k, c)
            assert [kind for ch, kind in ev if ch == c] == status[c], (k, c, ev, status[c])
            w = bank.get_state(c)
            assert np.array_equal(w[:31], refs[c].snapshot()), (k, c)
            quiet[c] += (got == 0)
            if w[24] == 0:
                phases["data"] += 1
                seen_all.add((c, 0))
            elif w[25] >= SHUTDOWN_END[modem]:
                phases["after"] += 1
                seen_all.add((c, 2))
            elif w[25] > TRAINING_END[modem] + 1:
                phases["shutdown"] += 1
                seen_all.add((c, 1))
        assert all(0 <= ch < n for ch, _ in ev)

    k = 0
    while quiet.min() < 3:
        assert k < 600
        # the next pieces: 8 .. 36 bits by channel, or what its ring has room for; every third round a channel sits out.  (The
        # sizes differ so that the channels' data end in different calls of the schedule, some of them in its short ones.)
        who = [c for c in range(n) if pending[c] and (k + c) % 3 != 0]
        if who:
            lo, hi = who[0], who[-1] + 1
            pieces = [pending[c][:8 + 7*(c % 5)] if c in who else [] for c in range(lo, hi)]
            acc = bank.put_bits(pieces, first=lo)
            for c in range(lo, hi):
                a = int(acc[c - lo])
                assert 0 <= a <= len(pieces[c - lo])
                feeds[c].bits += [int(b) for b in pending[c][:a]]
                del pending[c][:a]
        for c in range(n):
            if not pending[c] and not told[c]:
                bank.end_of_data(c)
                feeds[c].end_of_data = True
                told[c] = True
        if k % 7 == 0:
            for c in (0, 5, 69):
                assert bank.queued(c) == len(feeds[c].bits), (k, c)
        one_call(k, mr.SCHEDULE[k % len(mr.SCHEDULE)])
        k += 1
    assert all(f.calls > 0 for f in feeds)
    assert min(phases.values()) > 0, phases
    # state words were compared in the data, in mid-shutdown (a matter of where the calls end: some channel's did) and after it
    assert {(5, 0), (5, 2), (9, 0), (9, 2)} <= seen_all and any(ph == 1 for _, ph in seen_all)
    # two channels start again; what was left in their rings (put after the shutdown, never sent) must not be sent now
    again = (3, 66)
    bank.put_bits([[0, 1, 0, 0, 1, 0, 0, 0]*4], first=3)
    bank.put_bits([[0]*20], first=66)
    assert bank.queued(3) == 32 and bank.queued(66) == 20
    for c in again:
        bank.restart(c, bit_rate, False)
        refs[c].restart(bit_rate, False)
        feeds[c].end_of_data = False
        assert bank.queued(c) == 0
    for j in range(8 if modem != "v17" else 12):
        one_call(k + j, 1024)
    for c in again:
        assert bank.get_state(c)[24] == 0, c            # through the training again, sending ones from an empty ring
    for c in range(n):
        if c not in again:
            assert quiet[c] >= 3 + 8
    bank.close()


def rx_loop(engine, modem, bit_rate, frames):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    n, samples, payload_bits = 8, 160, 400
    rng = np.random.default_rng(bit_rate)
    payload = rng.integers(0, 2, (n, payload_bits))
    tx = make_bank(engine, modem, n, bit_rate, False, 512)
    assert list(tx.put_bits([list(p) for p in payload])) == [payload_bits]*n
    for c in range(n):
        tx.end_of_data(c)
    rx = {"v29": engine.V29Bank, "v27ter": engine.V27terBank, "v17": engine.V17Bank}[modem](n, bit_rate)
    buf = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(buf), n*samples*2) == 0
    got = [[] for _ in range(n)]
    for _ in range(frames):
        tx.tx_device(buf, samples, samples)
        tx.sync()
        rx.rx_device(buf, samples, samples)
        for c, e in enumerate(rx.events()):
            got[c].extend(int(v) for v in e)
    hip.hipFree(buf)
    for c in range(n):
        ev = got[c]
        assert -4 in ev, c                                  # SIG_STATUS_TRAINING_SUCCEEDED
        after = ev[ev.index(-4) + 1:]
        assert -1 in after, c                               # SIG_STATUS_CARRIER_DOWN, after the shutdown
        data = [b for b in after[:after.index(-1)] if b >= 0]
        want = [int(b) for b in payload[c]]
        hit = [k for k in range(len(data) - payload_bits + 1) if data[k:k + payload_bits] == want]
        print("%s channel %d: %d data bits after training, payload at %s" % (modem, c, len(data), hit[:1]))
        assert hit, (c, len(data))
        # in front of the payload there is nothing but the ones that end the training
        assert all(b == 1 for b in data[:hit[0]]), c


def test_v29_queue_tx_feeds_v29_rx_bits_in_equal_bits_out(built):
    from spandsp_amd import engine
    rx_loop(engine, "v29", 9600, 24)


def test_v27ter_queue_tx_feeds_v27ter_rx_bits_in_equal_bits_out(built):
    from spandsp_amd import engine
    rx_loop(engine, "v27ter", 4800, 60)


def test_v17_queue_tx_feeds_v17_rx_bits_in_equal_bits_out(built):
    from spandsp_amd import engine
    rx_loop(engine, "v17", 14400, 85)


@pytest.mark.parametrize("modem,bit_rate,tep", [("v29", 9600, False), ("v29", 4800, True), ("v27ter", 4800, False), ("v27ter", 2400, False),
                                                ("v17", 14400, False), ("v17", 7200, True)])
def test_senders_by_name_equal_reference_objects(built, modem, bit_rate, tep):
    """v29_tx / v27ter_tx / v17_tx objects of this library beside the reference's, each side with callbacks that write one log
    of get_bit and status calls: the samples, the return values and the interleaved logs are equal -- through set_get_bit()
    while training and in the data, _power(), the end of the data, the shutdown, and a _restart() after it."""
    from spandsp_amd import engine

    class Side:
        def __init__(self, make):
            self.log = []
            self.bits = []
            self.end = False
            self.obj = make(self.source("a"), lambda code: self.log.append(("status", code)))

        def source(self, tag):
            def get_bit():
                bit = self.bits.pop(0) if self.bits else (mr.END_OF_DATA if self.end else 1)
                self.log.append((tag, bit))
                return bit
            return get_bit

    ours = Side(lambda g, s: engine.ModemTxObject(modem + "_tx", bit_rate, tep, g, s))
    theirs = Side(lambda g, s: mr.RefModemTx(modem, bit_rate, tep, g, s))
    sides = (ours, theirs)
    rng = np.random.default_rng(bit_rate)
    calls = [0]

    def both(what):
        for s in sides:
            what(s)

    def run(m):
        a, ra = ours.obj.tx(m)
        b, rb = theirs.obj.tx(m)
        calls[0] += 1
        assert ra == rb, (calls[0], m, ra, rb)
        assert np.array_equal(a, b), (calls[0], m)
        assert ours.log == theirs.log, (calls[0], m, ours.log[-6:], theirs.log[-6:])
        return ra

    def in_data():
        return any(tag != "status" for tag, _ in ours.log)

    payload = [int(b) for b in rng.integers(0, 2, 700)]
    both(lambda s: s.bits.extend(payload))
    run(160)
    both(lambda s: s.obj.set_get_bit(s.source("b")))            # while training: takes effect when the data begins
    both(lambda s: s.obj.power(-20.5))
    k = 0
    while not in_data():
        run(mr.SCHEDULE[k % len(mr.SCHEDULE)])
        k += 1
        assert k < 200
    assert ours.log[0][0] == "b"
    both(lambda s: s.obj.set_get_bit(s.source("c")))            # in the data: at once
    run(77)
    assert ours.log[-1][0] == "c"
    both(lambda s: setattr(s, "end", True))
    run(5000)                                                    # longer than one launch of an object
    quiet = 0
    while quiet < 3:
        quiet += (run(mr.SCHEDULE[k % len(mr.SCHEDULE)]) == 0)
        k += 1
        assert k < 400
    assert ("status", mr.END_OF_DATA) in ours.log
    assert (("status", mr.SHUTDOWN_COMPLETE) in ours.log) == (modem != "v17")
    n_log = len(ours.log)
    # a restart after the shutdown: training again, then the new data to its end
    both(lambda s: s.obj.restart(bit_rate, False, True) if modem == "v17" else s.obj.restart(bit_rate, False))
    both(lambda s: s.bits.extend(payload[:101]))
    quiet = 0
    while quiet < 2:
        quiet += (run(1024) == 0)
        k += 1
        assert k < 500
    # the 101 bits, the get_bit that answered END_OF_DATA, its status call and, but for V.17, the end of the shutdown
    assert len(ours.log) == n_log + 101 + 2 + (1 if modem != "v17" else 0)
    ours.obj.close()
