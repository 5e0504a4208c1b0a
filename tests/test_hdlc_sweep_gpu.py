"""The HDLC framing banks on the GPU against the live reference, at bank scale: 1 061 generated lines (16 full waves and a
partial one of 37; tests/hdlc_sweep.py) through a receiver bank in its three forms and through a sender bank, every wave
mixing every family, configuration and call length, with the reference's framer run on the same input through
oracle/ref_hdlc.py.  Everything is equality: every line's records and octets of every call, a sender's bits, lengths,
underflow and end-of-data events and the results of its offers, every line's state words, statistics and 404 buffer octets
after the last call, and after every call the words of the probe lines (c % 61 == 0, each wave's first and last lane) and of
the lines that sit the call out, which must be as they were, buffer included.

The kernels have no cross-lane step: beyond what the host-compiled program reaches (tests/test_hdlc_sweep.py, forty times
these lines), a wave adds the divergence of its lanes and the side-by-side stores of their frame buffers, and sixteen mixed
waves show both."""
import time

import numpy as np
import pytest

import hdlc_sweep as H
from codec_sweep import WAVE
from spandsp_amd import engine
from test_g726_gpu import DevBytes

pytestmark = pytest.mark.gpu

N = H.N_GPU
HT_Q_HEAD, HT_Q_COUNT = 16, 17
BANK_DEPTH = 8


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_hdlc
    if not ref_hdlc.available():
        pytest.fail("oracle/_ref/libspandsp_hdlc_ref.so is not here: `make -C oracle ref` builds it where the reference's sources "
                    "are, and it travels with the tree; without it the sweep has nothing to compare with")
    return ref_hdlc


@pytest.fixture(autouse=True)
def timed(request):
    t0 = time.time()
    yield
    print("%s: %.2f s" % (request.node.name, time.time() - t0))


def differ(r, what, i, k, got, want):
    """the first difference of two item lists, named in full"""
    got, want = list(got), list(want)
    m = min(len(got), len(want))
    j = next((j for j in range(m) if got[j] != want[j]), m)
    fam = H.FAMILIES[int(r["fam"][i])] if "fam" in r else "-"
    pytest.fail("%s %s: family %s, configuration %s, line %d (wave %d, lane %d), call %d, %s %d: got %s, the reference has %s; %d against %d items "
                "(seed %#x)" % (r["family"], r.get("form", ""), fam, tuple(r["cfgs"][i].tolist()), i, i//WAVE, i % WAVE, k, what, j,
                                got[j] if j < len(got) else None, want[j] if j < len(want) else None, len(got), len(want), r["seed"]))


def same(r, what, i, k, got, want):
    if not np.array_equal(got, want):
        differ(r, what, i, k, np.asarray(got).tolist(), np.asarray(want).tolist())


def left_out_cap(lens):
    """no call leaves a quarter of the lines out"""
    assert ((lens == 0).mean(axis=1) < 0.25).all(), (lens == 0).mean(axis=1)


def round16(n):
    return (n + 15) & ~15


# ---- receivers -----------------------------------------------------------------------------------------------------------

def rx_bank(r):
    """one bank for all the lines: hdlc_rx_init()'s arguments are words of a channel, the settings go through the calls"""
    bank = engine.HdlcRxBank(N)
    for i, (crc32, bad, thr, _, _) in enumerate(r["cfgs"].tolist()):
        w = bank.get_state(i)
        w[H.HR_CRC_BYTES], w[H.HR_REPORT_BAD], w[H.HR_THRESHOLD] = (4 if crc32 else 2), bad, thr
        bank.set_state(i, w)
    return bank


def rx_control(bank, i, op, value):
    if op == H.OP_MAX_FRAME_LEN:
        bank.set_max_frame_len(i, value)
    elif op == H.OP_REPORT_INTERVAL:
        bank.set_octet_counting_report_interval(i, value)
    else:
        bank.restart(i)


def flat(row):
    """a call's records as items: a status code, or a frame's length, its ok flag and its octets"""
    out = []
    for rec in row:
        out += [rec] if isinstance(rec, int) else [rec[0], int(rec[1])] + list(rec[2])
    return out


def run_rx(r, put):
    """Every line of sweep r through one bank, call by call; put(bank, k, rows_of) feeds call k, where rows_of(width, dtype)
    makes the [n][width] rows of the call with every line's entries at the front."""
    lens = r["lens"]
    calls, n = lens.shape
    left_out_cap(lens)
    bank = rx_bank(r)
    for i in range(n):
        for call, op, value in r["ops"][i]:
            if call < 0:
                rx_control(bank, i, op, value)
    mid = {}
    for i in range(n):
        for call, op, value in r["ops"][i]:
            if call >= 0:
                mid.setdefault(call, []).append((i, op, value))
    want_recs = [H.records_of(r, i) for i in range(n)]
    at = np.zeros(n, np.int64)
    for k in range(calls):
        for i, op, value in mid.get(k, []):
            assert lens[k, i] > 0
            rx_control(bank, i, op, value)
        out = np.flatnonzero(lens[k] == 0).tolist()
        before = {i: (bank.get_state(i), bank.get_buffer(i)) for i in out}

        def rows_of(width, dtype):
            rows = np.zeros((n, width), dtype)
            for i in range(n):
                rows[i, :lens[k, i]] = r["data"][i][at[i]:at[i] + lens[k, i]]
            return rows

        put(bank, k, rows_of)
        at += lens[k]
        recs = bank.records()
        for i in range(n):
            if recs[i] != want_recs[i][k]:
                differ(r, "record item", i, k, flat(recs[i]), flat(want_recs[i][k]))
        for i in np.flatnonzero(r["want"][k]).tolist():
            same(r, "state word", i, k, bank.get_state(i), r["words"][i][k])
        for i, (w, b) in before.items():
            same(r, "state word of a line sitting out", i, k, bank.get_state(i), w)
            same(r, "buffer octet of a line sitting out", i, k, bank.get_buffer(i), b)
    for i in range(n):
        assert at[i] == len(r["data"][i])
        same(r, "state word at the end", i, calls - 1, bank.get_state(i), r["final"][i])
        same(r, "statistic", i, calls - 1, bank.get_stats(i), r["final"][i][H.HR_RX_BYTES:])
        same(r, "buffer octet", i, calls - 1, bank.get_buffer(i), r["buffer"][i])
    bank.close()


def test_receivers_int16_events_from_host_rows(built, ref):
    """rows as wide as the call's longest line: ragged widths, few of them whole 16-byte pieces"""
    r = H.sweep_rx()
    widths = r["lens"].max(axis=1)
    assert (widths % 8 != 0).sum() >= len(widths)//2

    def put(bank, k, rows_of):
        bank.put_events_host(rows_of(int(widths[k]), np.int16), r["lens"][k])

    run_rx(r, put)


def test_receivers_int8_events_from_device_rows(built, ref):
    """rows on 16-byte boundaries and padded to 16, so that the 16-byte path and its tail both run; the counts in device memory,
    every fourth line's above the row: the clamp makes it the row, and the reference was given the row"""
    r = H.sweep_rx(form="int8")
    lens, full = r["lens"], r["full"]
    assert 0.2 < full.mean() <= 0.25 and (lens % 16 != 0).mean() > 0.5
    most = round16(int(lens.max()))
    dev, counts = DevBytes(N*most), DevBytes(4*N)
    assert dev.ptr.value % 16 == 0

    def put(bank, k, rows_of):
        width = round16(int(lens[k].max()))
        assert (lens[k, full] == width).all()
        dev.put(rows_of(width, np.int8))
        counts.put(np.where(full, width + 1 + 1000*(np.arange(N) % 3), lens[k]).astype(np.int32))
        bank.put_events_device(dev.ptr, 1, width, counts.ptr)

    try:
        run_rx(r, put)
    finally:
        dev.free()
        counts.free()


def test_receivers_octets(built, ref):
    r = H.sweep_rx(form="octets")

    def put(bank, k, rows_of):
        bank.put_host(rows_of(int(r["lens"][k].max()), np.uint8), r["lens"][k])

    run_rx(r, put)


# ---- senders -------------------------------------------------------------------------------------------------------------

def test_senders(built, ref):
    """Offers through frames(), flags(), abort() and end() with their results; bits through get_bits_host() and, on alternate
    calls, get_bits_device().  The bank's queues are 8 deep; a line of a shallower queue is offered a command only while fewer
    than its depth are queued, and where the reference refused one for want of room the bank's fill is that depth."""
    r = H.sweep_tx()
    wants, cfgs = r["wants"], r["cfgs"]
    calls, n = wants.shape
    left_out_cap(wants)
    assert set(cfgs[:, 2]) == set(range(1, BANK_DEPTH + 1))
    bank = engine.HdlcTxBank(N, queue_depth=BANK_DEPTH)
    for i, (crc32, iff, depth, ml) in enumerate(cfgs.tolist()):
        w = bank.get_state(i)
        w[H.HT_CRC_BYTES], w[H.HT_IFF], w[H.HT_CRC] = (4 if crc32 else 2), iff, (-1 if crc32 else 0xFFFF)
        bank.set_state(i, w)
        if ml >= 0:
            bank.set_max_frame_len(i, ml)
    stride = 80                                     # 600 bits a call at the most
    dbits, dlens = DevBytes(N*stride), DevBytes(4*N)
    # the script of every line: per call its offers with what the reference answered, and the frames' octets
    script = [[[] for _ in range(calls)] for _ in range(n)]
    for i in range(n):
        at = 0
        for j, (k, kind, arg, corrupt) in enumerate(r["ops"][i].tolist()):
            data = r["opbytes"][i][at:at + arg].tobytes() if kind == H.FRAME else b""
            at += arg if kind == H.FRAME else 0
            script[i][k].append((j, kind, arg, corrupt, int(r["results"][i][j]), data))
    bit_at = np.zeros(n, np.int64)
    offered = refused_full = 0
    try:
        for k in range(calls):
            for rnd in range(max(len(script[i][k]) for i in range(n))):
                frames, who = [None]*n, []
                for i in range(n):
                    if rnd >= len(script[i][k]):
                        continue
                    j, kind, arg, corrupt, res, data = script[i][k][rnd]
                    limit = cfgs[i, 3] if cfgs[i, 3] >= 0 else 400
                    if res != 0 and not (kind == H.FRAME and arg > limit) and cfgs[i, 2] < BANK_DEPTH:
                        # refused for want of room in a queue shallower than the bank's
                        if bank.queued(i) != cfgs[i, 2]:
                            differ(r, "queue fill where the reference's is full, offer", i, k, [j, bank.queued(i)], [j, cfgs[i, 2]])
                        refused_full += 1
                        continue
                    offered += 1
                    if kind == H.FRAME:
                        frames[i] = data
                        who.append((i, j, corrupt, res))
                    else:
                        got = {H.FLAGS: lambda: bank.flags(arg, first=i, n=1), H.ABORT: lambda: bank.abort(first=i, n=1),
                               H.END: lambda: bank.end(first=i, n=1)}[kind]()[0]
                        if got != res:
                            differ(r, "result of offer", i, k, [j, got], [j, res])
                if who:
                    corrupt = np.zeros(n, np.int32)
                    for i, j, c, res in who:
                        corrupt[i] = c
                    got = bank.frames(frames, corrupt=corrupt)
                    for i, j, c, res in who:
                        if got[i] != res:
                            differ(r, "result of offer", i, k, [j, got[i]], [j, res])
            out = np.flatnonzero(wants[k] == 0).tolist()
            before = {i: (bank.get_state(i), bank.get_buffer(i)) for i in out}
            if k % 2 == 0:
                bits, lens = bank.get_bits_host(wants[k])
            else:
                bank.get_bits_device(dbits.ptr, stride, 0, dlens.ptr, want=wants[k])
                bank.sync()
                bits, lens = dbits.get((n, stride)), dlens.get(n, np.int32)
            if not np.array_equal(lens, r["lens"][k]):
                i = int(np.flatnonzero(lens != r["lens"][k])[0])
                differ(r, "bits of the call", i, k, lens[i:i + 1], r["lens"][k][i:i + 1])
            events = {}
            for ch, kind in bank.events():
                events.setdefault(ch, []).append(kind)
            for i in range(n):
                m = int(lens[i])
                got = np.unpackbits(bits[i, :(m + 7)//8], bitorder="little")[:m]
                same(r, "bit", i, k, got, r["bits"][i][bit_at[i]:bit_at[i] + m])
                expect = ([int(r["under"][k, i])] if r["under"][k, i] else []) + ([-7] if r["ended"][k, i] else [])
                if events.get(i, []) != expect:
                    differ(r, "underflow and end-of-data event", i, k, events.get(i, []), expect)
            bit_at += lens
            for i in np.flatnonzero(r["want"][k]).tolist():
                same(r, "state word", i, k, bank.get_state(i)[:H.TX_WORDS], r["words"][i][k])
            # a channel that wants nothing keeps its state and its queue
            for i, (w, b) in before.items():
                same(r, "state or queue word of a line sitting out", i, k, bank.get_state(i), w)
                same(r, "buffer octet of a line sitting out", i, k, bank.get_buffer(i), b)
        for i in range(n):
            assert bit_at[i] == len(r["bits"][i])
            same(r, "state word at the end", i, calls - 1, bank.get_state(i)[:H.TX_WORDS], r["final"][i])
        assert offered > 20000 and refused_full > 1000, (offered, refused_full)
    finally:
        dbits.free()
        dlens.free()
        bank.close()
