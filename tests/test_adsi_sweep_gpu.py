"""The ADSI sweep on the GPU (tests/adsi_sweep.py; its CPU half is tests/test_adsi_sweep.py): banks of 1 061 caller-ID lines
against the live reference behind oracle/ref_adsi.py, for equality throughout.

  * receivers from host rows with per-channel lengths: the messages and counts of every call, the framer's and the
    demodulator's words of the probe lines after every call and of every line at the end, the message buffer at the end; a
    line that sits a call out keeps its state; no count above msg_capacity();
  * receivers from device rows on 160-sample ticks, at a stride wider than the row: the same;
  * senders: the samples of every call with the zeros behind the returned length, the lengths, every put's return, the 24
    words of the probes after every call and of every line at the end, the message bytes.

The `fast` family is among the receiver lines: on it the reference completes more messages in a call than the record used to
have room for, and the read-out failed the whole bank with SPANGPU_ERR_STATE (profiles/adsi_sweep.md).

Only oracle/_ref/libspandsp_adsi_ref.so is used, never the reference's sources."""
import ctypes as C

import numpy as np
import pytest

import adsi_sweep as S
import fsktx_ref
from oracle import ref_adsi
from spandsp_amd import engine

pytestmark = pytest.mark.gpu

N = S.N_GPU
STANDARDS = [S.standard_of(c) for c in range(N)]
RX_HEAD = 6                     # ADR_STANDARD .. ADR_FRAMING_ERRORS
FSK_AT = 8                      # kAdsiRxWords: the demodulator's words follow the framer's


@pytest.fixture(autouse=True)
def adsi_ref():
    assert ref_adsi.available(), "oracle/_ref/libspandsp_adsi_ref.so has not travelled with the tree"


def where(line, call, what, family=True):
    return "family %s, line %d (standard %d), call %d: %s" % (S.FAMILIES[int(S.family_of(line))] if family else "sender", line,
                                                              S.standard_of(line), call, what)


def by_call(q, calls):
    out = [[] for _ in range(calls)]
    for k, m in q["msgs"]:
        out[k].append(m)
    return out


def check_receivers(r, feed):
    """feed(bank, k) gives call k to the bank; everything the bank then has against the reference's"""
    lens = r["lens"]
    calls = len(lens)
    want = [by_call(q, calls) for q in r["ref"]]
    bank = engine.AdsiRxBank(STANDARDS, N)
    last = {c: bank.get_state(c) for c in S.PROBES}
    delivered = 0
    for k in range(calls):
        feed(bank, k)
        got = bank.messages()
        for c in range(N):
            if got[c] != want[c][k]:
                raise AssertionError(where(c, k, "messages %r, the reference has %r" % (got[c], want[c][k])))
            assert len(got[c]) <= bank.msg_capacity(int(lens[k, c])), where(c, k, "%d messages, above msg_capacity()" % len(got[c]))
            delivered += len(got[c])
        for c in S.PROBES:
            w = bank.get_state(c)
            q = r["ref"][c]
            assert np.array_equal(w[:RX_HEAD], q["words"][k]), where(c, k, "framer words %s, the reference has %s" % (w[:RX_HEAD], q["words"][k]))
            assert np.array_equal(w[FSK_AT:FSK_AT + ref_adsi.FSK_WORDS], q["fsk_words"][k]), where(c, k, "demodulator words")
            if lens[k, c] == 0:
                assert np.array_equal(w, last[c]), where(c, k, "sat the call out, and its state changed")
            last[c] = w
    for c in range(N):
        w = bank.get_state(c)
        q = r["ref"][c]
        assert np.array_equal(w[:RX_HEAD], q["words"][-1]), where(c, calls, "framer words %s, the reference has %s" % (w[:RX_HEAD], q["words"][-1]))
        assert np.array_equal(w[FSK_AT:FSK_AT + ref_adsi.FSK_WORDS], q["fsk_words"][-1]), where(c, calls, "demodulator words")
        assert np.array_equal(bank.get_message(c), q["msg"]), where(c, calls, "msg[]")
    assert delivered == sum(len(q["msgs"]) for q in r["ref"]) > 1000
    # (behind the calls: a bank whose capacity is too small fails in them, with what its read-out says)
    assert [bank.msg_capacity(n) for n in (0, 1, 119, 120, 160, 1024)] == [int(S.capacity(n)) for n in (0, 1, 119, 120, 160, 1024)]
    return bank


def test_receivers_from_host_rows_with_per_channel_lengths(built):
    r = S.sweep_rx()
    rows, lens = r["rows"], r["lens"]
    at = np.zeros(N, np.int64)
    idx = np.arange(1024)[None, :]

    def feed(bank, k):
        n = max(1, int(lens[k].max()))
        take = np.minimum(at[:, None] + idx[:, :n], rows.shape[1] - 1)
        amp = np.where(idx[:, :n] < lens[k][:, None], np.take_along_axis(rows, take, axis=1), 0).astype(np.int16)
        bank.rx_host_var(amp, lens[k])
        at[:] += lens[k]

    check_receivers(r, feed)
    # the lines aimed at the capacity came through: calls with more messages than the record used to hold
    assert S.coverage_rx(r)["over_old_capacity"] >= 300


def test_receivers_from_device_rows_on_ticks(built):
    r = S.sweep_rx(ticks=True)
    rows = r["rows"]
    stride = S.TICK + 24                # wider than the row
    dev = fsktx_ref.DeviceRows(N, stride)
    host = np.full((N, stride), 0x5A5A, np.int16)

    def feed(bank, k):
        host[:, :S.TICK] = rows[:, k*S.TICK:(k + 1)*S.TICK]
        assert dev.hip.hipMemcpy(dev.ptr, C.c_void_p(host.ctypes.data), host.nbytes, 1) == 0
        bank.rx_device(dev.ptr, S.TICK, stride)

    try:
        check_receivers(r, feed)
    finally:
        dev.free()
    assert S.coverage_rx(r)["over_old_capacity"] >= 90


def test_senders(built):
    r = S.sweep_tx()
    lens = r["lens"]
    starts = np.concatenate([[0], np.cumsum(lens)])
    ref_pcm = np.stack([q[0] for q in r["ref"]])
    ref_lens = np.stack([q[1] for q in r["ref"]])
    bank = engine.AdsiTxBank(STANDARDS, N)
    nxt = [0]*N
    for k in range(len(lens)):
        for c in range(N):
            ops, _, msgs = r["scripts"][c]
            results = r["ref"][c][2]
            while nxt[c] < len(ops) and ops[nxt[c]][0] <= k:
                o = ops[nxt[c]]
                if o[1] == S.OP_PUT:
                    m = r["scripts"][c][1][o[2]:o[2] + o[3]]
                    got = int(bank.put_message([m], first=c)[0])
                    assert got == results[nxt[c]], where(c, k, "a put of %d bytes returned %d, the reference %d" % (len(m), got, results[nxt[c]]), False)
                elif o[1] == S.OP_PREAMBLE:
                    bank.set_preamble(c, o[2], o[3], o[4], o[5])
                elif o[1] == S.OP_ALERT:
                    bank.send_alert_tone(c)
                elif o[1] == S.OP_SHUT_DOWN:
                    w = bank.get_state(c)
                    w[S.FT_SHUTDOWN] = 1
                    bank.set_state(c, w)
                else:
                    bank.restart(c, S.standard_of(c))
                nxt[c] += 1
        n = int(lens[k])
        pcm, got_lens = bank.tx_host(n)
        if not np.array_equal(got_lens, ref_lens[:, k]):
            c = int(np.nonzero(got_lens != ref_lens[:, k])[0][0])
            raise AssertionError(where(c, k, "returned length %d, the reference's %d" % (got_lens[c], ref_lens[c, k]), False))
        want = ref_pcm[:, starts[k]:starts[k] + n]
        if not np.array_equal(pcm, want):
            c, j = [int(x[0]) for x in np.nonzero(pcm != want)]
            raise AssertionError(where(c, k, "sample %d of %d (returned length %d) is %d, the reference's %d"
                                       % (j, n, got_lens[c], pcm[c, j], want[c, j]), False))
        for c in S.PROBES:
            w = bank.get_state(c)[:ref_adsi.TX_WORDS]
            assert np.array_equal(w, r["ref"][c][3][k]), where(c, k, "words %s, the reference has %s" % (w, r["ref"][c][3][k]), False)
    assert all(nxt[c] == len(r["scripts"][c][0]) for c in range(N))
    for c in range(N):
        w = bank.get_state(c)[:ref_adsi.TX_WORDS]
        q = r["ref"][c]
        assert np.array_equal(w, q[3][-1]), where(c, len(lens), "words %s, the reference has %s" % (w, q[3][-1]), False)
        assert np.array_equal(bank.get_message(c), q[4]), where(c, len(lens), "msg[]", False)
