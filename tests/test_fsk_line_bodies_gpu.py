"""The seams of the bodies the FSK line families share -- fsk_pair_body() (csrc/fsk_dev.hpp) under fsk_rx, v18_rx and adsi_rx,
ftx_rounds() (csrc/fskmod_dev.hpp) under fsk_tx, v18_tx and adsi_tx -- where the family suites do not reach: rows that lie in
device memory one sample past a 16-byte boundary with an odd stride (the element-access copies of both bodies, which ADSI
never ran and the others ran for 37 samples only), a tail group of 6 channels behind a full one, per-channel lengths of 0, 1,
7, 9 and the whole call on the first and last lanes of both groups, and calls long enough for a second trip of the
modulator's round loop with queues that run dry inside it.  The other side of every comparison is a twin bank given the same
calls through host arrays (the aligned copies), which the family suites pin to the reference; everything is integer
arithmetic, so every comparison is for equality."""
import ctypes as C

import numpy as np
import pytest

import adsi_lines as AL
import fsktx_ref as fr

pytestmark = pytest.mark.gpu

N = 70                          # a full group of 64 and a tail of 6; for the senders' 16 per wave, a second, partial workgroup
CALLS = [8, 37, 160, 401]
STRIDE = 411                    # odd: no row but the first can start on a 16-byte boundary, and the first is put off it
RX_WATCHED = (0, 63, 64, 69)
TX_WATCHED = (0, 15, 16, 63, 64, 69)
POISON = 0x5555
V18_MODE = 0x0002               # Weitbrecht 45.45
FSK_1200 = 2                    # preset_fsk_specs[]: V.23 channel 1


class OddRows:
    """[N][STRIDE] int16 in device memory, row 0 starting one sample past the allocation's 256-byte aligned base; a sample
    ahead of row 0 and some behind the last row are there to be found untouched.  The memory is hipMalloc's, from the HIP
    runtime the library itself runs on (fsktx_ref.DeviceRows)."""

    def __init__(self):
        self.mem = fr.DeviceRows(N, STRIDE + 1)         # N*STRIDE + 70 samples, and N lengths
        assert self.mem.ptr.value % 16 == 0
        self.ptr = C.c_void_p(self.mem.ptr.value + 2)
        self.lens_ptr = self.mem.lens
        self.stride = STRIDE

    def put(self, block):
        flat = np.full(N*(STRIDE + 1), POISON, np.int16)
        flat[1:1 + N*STRIDE].reshape(N, STRIDE)[:, :block.shape[1]] = block
        assert self.mem.hip.hipMemcpy(self.mem.ptr, flat.ctypes.data, flat.nbytes, 1) == 0

    def poison(self):
        assert self.mem.hip.hipMemset(self.mem.lens, 0xFF, N*4) == 0
        self.mem.fill(0x55)                             # (and waits for both)

    def back(self):
        flat = self.mem.rows().reshape(-1)
        return flat[1:1 + N*STRIDE].reshape(N, STRIDE).copy(), flat[:1].copy(), flat[1 + N*STRIDE:].copy(), self.mem.lengths()

    def free(self):
        self.mem.free()


def lengths_of(k, m):
    """The lengths of call k of m samples: whole but on the watched channels, which take 0, 1, 7, 9 and the whole call in turn"""
    lens = np.full(N, m, np.int32)
    for j, c in enumerate(RX_WATCHED):
        lens[c] = min((0, 1, 7, 9, m)[(k + j) % 5], m)
    return lens


# ---- the lines: what each family's sender bank makes of a short text or message ------------------------------------------

def fsk_line(engine):
    rng = np.random.default_rng(1200)
    tx = engine.FskTxBank(FSK_1200, N, engine.FSKTX_QUEUE, queue_bits=512)
    bits = [rng.integers(0, 2, 300 + c).astype(np.uint8) for c in range(N)]
    assert list(tx.put_bits(bits)) == [len(b) for b in bits]
    for c in range(N):
        tx.end_of_data(c)
    rows, lens = tx.tx_host(4096)
    tx.close()
    assert (lens > 1900).all() and (lens < 4096).all()           # the carrier ends inside the line
    return rows


def v18_line(engine):
    tx = engine.V18Bank(V18_MODE, N)
    texts = [(b"HI", b"OK 2", b"A1", b"73")[c % 4] for c in range(N)]
    assert list(tx.put(texts)) == [len(t) for t in texts]
    parts = []
    for _ in range(120):
        rows, lens = tx.tx_host(160)
        parts.append(rows.copy())
        if not lens.any():
            break
    else:
        raise AssertionError("the senders did not end")
    tx.close()
    return np.concatenate(parts, axis=1)


def adsi_line(engine):
    tx = engine.AdsiTxBank([AL.CLIP], N)
    for c in range(N):
        tx.send_alert_tone(c)
        tx.set_preamble(c, 40, 30, -1, -1)
    msgs = [AL.number_message(AL.CLIP, b"555%04d" % c, b"Line %d" % c) for c in range(N)]
    assert list(tx.put_message(msgs)) == [len(m) for m in msgs]
    parts = []
    for _ in range(60):
        rows, lens = tx.tx_host(160)
        parts.append(rows.copy())
        if not lens.any():
            break
    else:
        raise AssertionError("the senders did not end")
    tx.close()
    return np.concatenate(parts, axis=1)


def fsk_pair(engine):
    return [engine.FskBank(FSK_1200, N, engine.FSK_FRAME_MODE_ASYNC) for _ in range(2)]


def v18_pair(engine):
    banks = [engine.V18Bank(V18_MODE, N) for _ in range(2)]
    # a suppression timer that runs out after a few calls on some channels, two watched ones among them: the body steps it
    # by each channel's own length ahead of the samples
    for b in banks:
        for c in (0, 5, 64, 66):
            w = b.get_state(c)
            w[engine.V18_W_RX_SUPPRESSION] = 150 + 11*c
            b.set_state(c, w)
    return banks


def adsi_pair(engine):
    return [engine.AdsiRxBank([AL.CLIP], N) for _ in range(2)]


RECEIVERS = {
    # the line, the twin banks, the entry point for per-channel lengths, what was heard in the last call, the calls to make
    "fsk": (fsk_line, fsk_pair, "spangpu_fsk_rx_var", lambda b: [e.tolist() for e in b.events()], 40),
    "v18": (v18_line, v18_pair, "spangpu_v18_rx_var", lambda b: b.text(), 280),
    "adsi": (adsi_line, adsi_pair, "spangpu_adsi_rx_var", lambda b: b.messages(), 280),
}


@pytest.mark.parametrize("family", list(RECEIVERS))
def test_receivers_on_unaligned_device_rows(built, family):
    from spandsp_amd import engine
    make_line, make_pair, entry, heard, n_calls = RECEIVERS[family]
    line = make_line(engine)
    line = np.concatenate([line, np.zeros((N, n_calls*max(CALLS)), np.int16)], axis=1)
    dev_bank, host_bank = make_pair(engine)
    rx_var = getattr(engine.lib(), entry)
    rows = OddRows()
    pos = np.zeros(N, np.int64)
    total = [0]*N
    for k in range(n_calls):
        m = CALLS[k % len(CALLS)]
        lens = lengths_of(k, m)
        block = np.zeros((N, m), np.int16)
        for c in range(N):
            block[c, :lens[c]] = line[c, pos[c]:pos[c] + lens[c]]
        pos += lens
        rows.put(block)
        engine._check(rx_var(dev_bank.h, rows.ptr, engine.MEM_DEVICE, lens.ctypes.data, m, rows.stride))
        host_bank.rx_host_var(block, lens)
        got, want = heard(dev_bank), heard(host_bank)
        assert got == want, (family, k, m, [c for c in range(N) if got[c] != want[c]][:5])
        for c in range(N):
            total[c] += len(want[c])
        if k % len(CALLS) == len(CALLS) - 1 or k == n_calls - 1:
            for c in RX_WATCHED:
                assert np.array_equal(dev_bank.get_state(c), host_bank.get_state(c)), (family, k, c)
    # the twins agreed on something: every channel heard its line, the watched ones included
    assert all(t > 0 for t in total), (family, [c for c in range(N) if total[c] == 0])
    for c in range(N):
        assert np.array_equal(dev_bank.get_state(c), host_bank.get_state(c)), (family, c)
    rows.free()
    dev_bank.close()
    host_bank.close()


# ---- senders --------------------------------------------------------------------------------------------------------------

def fsktx_twins(engine):
    """A 1200 baud sender from its queue, end of data set: 401 samples are some 60 bit boundaries, more than the 32 runs of a
    round, and the queues run dry at once (0), in the 160-sample call (10), in the first round of the first 401-sample call (40),
    in its second round (70, 80), in the second round of the second 401-sample call (160) and never (400)."""
    rng = np.random.default_rng(401)
    counts = [(70, 10, 40, 80, 400, 0, 160)[c % 7] for c in range(N)]
    bits = [rng.integers(0, 2, k).astype(np.uint8) for k in counts]
    banks = [engine.FskTxBank(FSK_1200, N, engine.FSKTX_QUEUE, queue_bits=512) for _ in range(2)]
    for b in banks:
        assert list(b.put_bits(bits)) == counts
        for c in range(N):
            b.end_of_data(c)
    feeds = [fr.BitFeed() for _ in range(N)]
    for c in range(N):
        feeds[c].bits = [int(x) for x in bits[c]]
        feeds[c].end_of_data = True
    refs = [fr.RefFskTx(FSK_1200, get_bit=feeds[c]) for c in range(N)]
    return banks, refs


def v18tx_twins(engine):
    """Texts of 0 to 5 characters, with and without a shift ahead of them: a channel nothing was put into is never asked, the
    others shut down in different calls"""
    texts = [(b"", b"E", b"HI", b"A1", b"OK 2", b"3", b"73 DE", b"T5")[c % 8] for c in range(N)]
    banks = [engine.V18Bank(V18_MODE, N) for _ in range(2)]
    for b in banks:
        for c in range(N):
            if texts[c]:
                assert int(b.put([texts[c]], first=c)[0]) == len(texts[c])
    return banks, None


def adsitx_twins(engine):
    """The four standards cycled, messages of different lengths, the alert tone ahead of every third, short preambles on every
    fifth, nothing put into every seventh"""
    banks = [engine.AdsiTxBank(AL.STANDARDS, N) for _ in range(2)]
    for b in banks:
        for c in range(N):
            if c % 3 == 0:
                b.send_alert_tone(c)
            if c % 5 == 0:
                b.set_preamble(c, 40, 20, 7, -1)
            if c % 7 != 6:
                msg = AL.number_message(AL.STANDARDS[c % 4], b"5%d" % c, b"L"*(c % 9))
                assert int(b.put_message([msg], first=c)[0]) == len(msg)
    return banks, None


SENDERS = {"fsktx": (fsktx_twins, 2), "v18": (v18tx_twins, 20), "adsi": (adsitx_twins, 12)}


@pytest.mark.parametrize("family", list(SENDERS))
def test_senders_into_unaligned_device_rows(built, family):
    from spandsp_amd import engine
    make, rounds = SENDERS[family]
    (dev_bank, host_bank), refs = make(engine)
    rows = OddRows()
    ended_inside = {m: 0 for m in CALLS}
    second_round = 0            # ends past the first round of a 401-sample call at 1200 baud: 32 runs are less than 32*7 samples
    for k in range(rounds*len(CALLS)):
        m = CALLS[k % len(CALLS)]
        rows.poison()
        dev_bank.tx_device(rows.ptr, rows.stride, m, rows.lens_ptr)
        dev_bank.sync()
        got, before, after, got_lens = rows.back()
        want, want_lens = host_bank.tx_host(m)
        assert np.array_equal(got_lens, want_lens), (family, k, m, np.nonzero(got_lens != want_lens)[0][:5])
        bad = [c for c in range(N) if not np.array_equal(got[c, :m], want[c])]
        assert not bad, (family, k, m, bad[:5])
        # nothing but the call's samples was written: not the sample ahead of row 0, not the rows' tails, not past the last row
        assert (got[:, m:] == POISON).all() and (before == POISON).all() and (after == POISON).all(), (family, k, m)
        if family == "fsktx":
            assert list(dev_bank.events()) == list(host_bank.events()), (family, k)
        if refs:
            for c in range(N):
                ref_row, ref_len = refs[c].tx(m)
                assert want_lens[c] == ref_len and np.array_equal(got[c, :m], ref_row), (family, k, m, c)
        for c in TX_WATCHED:
            assert np.array_equal(dev_bank.get_state(c), host_bank.get_state(c)), (family, k, c)
        ended_inside[m] += int(((want_lens > 0) & (want_lens < m)).sum())
        second_round += int(((want_lens > 32*7) & (want_lens < m)).sum())
    # senders did end inside a 401-sample call; the 1200 baud ones past the 32 runs of its first round too
    assert ended_inside[401] > 0, (family, ended_inside)
    assert second_round >= 2 or family != "fsktx", (family, second_round)
    for c in range(N):
        assert np.array_equal(dev_bank.get_state(c), host_bank.get_state(c)), (family, c)
    rows.free()
    dev_bank.close()
    host_bank.close()
