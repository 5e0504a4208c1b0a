"""The modem receiver, echo canceller and sharded banks on the shared host core (spandsp_amd/csrc/bank_host.hip, shard_core.hpp),
through engine.py: a modem bank fed host rows and its twin fed device rows are replicas of each other across regrowth of the
frame staging (whose rows are a multiple of 8 samples long, whatever the call), with one length for all channels and with a
length per channel; a bank that is handed a caller's stream and then told to make its own again computes what a twin that never
changed streams computes; the channels of a sharded set are dealt in whole waves; and a sharded set that has queued nothing
says so.  The values themselves are pinned to the reference by the family suites; here two banks of this library are compared,
bit for bit."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 70                          # one full wave and a ragged tail; by the default mapping a quad bank of five waves, the last partial
CALLS = (161, 80, 240, 7)       # 161 and 7: no multiple of 8, the staging rows are longer than the call; 80, 240, 7: grow, grow, reuse
PAD = 3                         # a host caller's rows are this much longer than the call
WATCH = (0, 63, 64, 69)
ERR_STATE = -5                  # SPANGPU_ERR_STATE (include/spangpu.h)
# Samples both twins take from device rows before CALLS, so that the receivers are past their training in the 240-sample call.
# A receiver of the oracle fed the oracle's transmitter, 80 samples a call, delivers its first data bit by sample 2160 (V.29
# 9600), 11280 (V.17 14400, the long training) and 5920 (V.27ter 4800), whatever the scrambler seed.
KINDS = {"v29": ("V29TxBank", "V29Bank", 9600, 2400), "v17": ("V17TxBank", "V17Bank", 14400, 11600),
         "v27ter": ("V27terTxBank", "V27terBank", 4800, 6200)}


def signal(engine, kind):
    """[N][lead-in + CALLS] from the transmitter bank: every channel its own scrambler seed"""
    seeds = np.array([(c*37 + 5) & 0x7FFF for c in range(N)], np.uint32)
    tx = getattr(engine, KINDS[kind][0])(N, KINDS[kind][2], seeds=seeds)
    sig = tx.tx_host(KINDS[kind][3] + sum(CALLS))
    tx.close()
    return sig


def twins(engine, kind, sig):
    """two receiver banks that have taken the lead-in from device rows: neither has staged a host frame yet"""
    import torch
    lead = KINDS[kind][3]
    rows = torch.from_numpy(np.ascontiguousarray(sig[:, :lead])).cuda()
    torch.cuda.synchronize()
    banks = [getattr(engine, KINDS[kind][1])(N, KINDS[kind][2]) for _ in range(2)]
    for b in banks:
        b.rx_device(rows.data_ptr(), lead, lead)
        b.sync()
    return banks


def host_rows(sig, at, m):
    rows = np.full((N, m + PAD), 0x5555, np.int16)
    rows[:, :m] = sig[:, at:at + m]
    return rows


def device_rows(sig, at, m):
    """rows of another stride than the host twin's, so that nothing but the samples is shared"""
    import torch
    t = torch.full((N, m + 5), 0x2AAA, dtype=torch.int16, device="cuda")
    t[:, :m] = torch.from_numpy(np.ascontiguousarray(sig[:, at:at + m])).cuda()
    torch.cuda.synchronize()
    return t


def same(host, dev, what):
    eh, ed = host.events(), dev.events()
    assert [len(e) for e in eh] == [len(e) for e in ed], what
    assert all(np.array_equal(a, b) for a, b in zip(eh, ed)), what
    for c in WATCH:
        (fh, ih), (fd, id_) = host.get_state(c), dev.get_state(c)
        assert np.array_equal(fh.view(np.uint32), fd.view(np.uint32)) and np.array_equal(ih, id_), (what, c)
    return ed


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_modem_host_frames_equal_device_frames(built, kind):
    from spandsp_amd import engine
    sig = signal(engine, kind)
    host, dev = twins(engine, kind, sig)
    at = KINDS[kind][3]
    for m in CALLS:
        rows = host_rows(sig, at, m)
        engine._check(engine.lib().spangpu_modem_rx(host.h, rows.ctypes.data, engine.MEM_HOST, m, m + PAD))
        t = device_rows(sig, at, m)
        dev.rx_device(t.data_ptr(), m, m + 5)
        events = same(host, dev, (kind, m))
        if m == 240:
            # the precondition of the comparison: the receivers are past their training, the calls compared carry data
            assert any((e >= 0).any() for e in events), kind
        at += m
    host.close()
    dev.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_modem_host_lengths_equal_device_lengths(built, kind):
    from spandsp_amd import engine
    sig = signal(engine, kind)
    host, dev = twins(engine, kind, sig)
    at = KINDS[kind][3]
    rng = np.random.default_rng(7)
    for m in CALLS:
        lens = rng.integers(0, m + 1, N).astype(np.int32)
        lens[[0, 63, 64, 69]] = (m, 0, 1, m)            # the whole call, none of it, one sample
        rows = host_rows(sig, at, m)
        engine._check(engine.lib().spangpu_modem_rx_var(host.h, rows.ctypes.data, engine.MEM_HOST, lens.ctypes.data, m, m + PAD))
        t = device_rows(sig, at, m)
        engine._check(engine.lib().spangpu_modem_rx_var(dev.h, ctypes.c_void_p(t.data_ptr()), engine.MEM_DEVICE, lens.ctypes.data, m, m + 5))
        same(host, dev, (kind, m))
        at += m                                         # (a channel that took less simply loses the rest: both twins alike)
    host.close()
    dev.close()


def test_modem_stream_hand_over(built):
    import torch
    from spandsp_amd import engine
    sig = signal(engine, "v29")
    moved, still = twins(engine, "v29", sig)
    mine = torch.cuda.Stream()
    at = KINDS["v29"][3]
    for k, stream in enumerate((mine.cuda_stream, None)):
        moved.set_stream(stream)
        if stream is None:
            assert moved.get_stream() != 0 and moved.get_stream() != mine.cuda_stream
        else:
            assert moved.get_stream() == mine.cuda_stream
        m = CALLS[k]
        for b in (moved, still):
            b.rx_host(sig[:, at:at + m])
        same(moved, still, ("stream", k))
        at += m
    moved.close()
    still.close()


def test_echo_stream_hand_over(built):
    import torch
    from spandsp_amd import engine
    rng = np.random.default_rng(5)
    tx = rng.integers(-8000, 8000, (N, 2*160)).astype(np.int16)
    rx = (tx//4 + rng.integers(-50, 50, tx.shape)).astype(np.int16)
    moved, still = (engine.EchoBank(N, 128, 1) for _ in range(2))
    mine = torch.cuda.Stream()
    for k, stream in enumerate((mine.cuda_stream, None)):
        moved.set_stream(stream)
        if stream is None:
            assert moved.get_stream() != 0 and moved.get_stream() != mine.cuda_stream
        else:
            assert moved.get_stream() == mine.cuda_stream
        got = [b.update_host(tx[:, 160*k:160*(k + 1)], rx[:, 160*k:160*(k + 1)]) for b in (moved, still)]
        assert np.array_equal(np.asarray(got[0]), np.asarray(got[1])), k
        for c in WATCH:
            a, b = moved.get_state(c), still.get_state(c)
            assert a.keys() == b.keys() and all(np.array_equal(a[f], b[f]) for f in a), (k, c)
    moved.close()
    still.close()


def deal_channels(n_channels, n_shards):
    """The dealing rule: contiguous ranges of whole waves (64 channels), as evenly as they go, while what is left allows it --
    every shard behind keeps at least a channel -- and the last shard takes the rest."""
    per = -(-(-(-n_channels//n_shards))//64)*64
    first, at = [], 0
    for i in range(n_shards):
        first.append(at)
        behind = n_shards - 1 - i
        mine = min(per, n_channels - at - behind)
        if mine >= 64:
            mine -= mine % 64
        at += (n_channels - at) if behind == 0 else max(mine, 1)
    return first, [b - a for a, b in zip(first, first[1:] + [n_channels])]


def sharded(engine, family):
    if family == "tone":
        return engine.ShardedToneBank(engine.DTMF, 200, [0, 0, 0])
    if family == "echo":
        return engine.ShardedEchoBank(200, 128, 1, [0, 0, 0])
    return engine.ShardedModemBank(engine.V29, 200, 9600, [0, 0, 0])


@pytest.mark.parametrize("family", ["tone", "echo", "modem"])
def test_shards_are_dealt_in_whole_waves(built, family):
    from spandsp_amd import engine
    first, counts = deal_channels(200, 3)
    assert (first, counts) == ([0, 128, 192], [128, 64, 8])
    sh = sharded(engine, family)
    assert [sh.info(i).first_channel for i in range(3)] == first and [sh.info(i).n_channels for i in range(3)] == counts
    assert [(r[1], r[2]) for r in sh.ranges] == list(zip(first, counts))
    sh.close()


@pytest.mark.parametrize("family", ["tone", "echo", "modem"])
def test_shards_report_nothing_before_a_step(built, family):
    from spandsp_amd import engine
    sh = sharded(engine, family)
    lib = engine.lib()
    out, dev = ctypes.c_void_p(), ctypes.c_int()
    if family == "tone":
        rc = lib.spangpu_shard_digits_device(sh.h, None, ctypes.byref(out), ctypes.byref(dev), None)
    elif family == "echo":
        rc = lib.spangpu_echo_shard_erle_device(sh.h, None, ctypes.byref(out), ctypes.byref(dev))
    else:
        counts = np.zeros(200, np.int32)
        events = np.zeros((200, 64), np.int8)
        rc = lib.spangpu_modem_shard_events_host(sh.h, counts.ctypes.data, events.ctypes.data)
    assert rc == ERR_STATE
    sh.close()
