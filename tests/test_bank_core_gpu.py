"""The host plumbing the sender and side-receiver banks share (spandsp_amd/csrc/bank_host.hip), through engine.py: a bank called
with host arrays and its twin called with device tensors are replicas of each other across regrowth of the frame staging,
a caller's stream stays the caller's, and an edit of one channel's words touches that channel alone.  The values themselves are
pinned to the reference by the family suites; here two banks of this library are compared, bit for bit."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 70                      # lane-per-channel kernels: a full group of 64 and a tail of 6; 16-per-wave senders: a second, partial workgroup
CALLS = (8, 40, 8, 37)      # the staging grows, is reused, is reused by a smaller frame, takes an odd length
WATCH = (0, 63, 64, 69)
WARM = 2100                 # V.29 with the caller's data: past the training, so that the end of the data is reached in CALLS
# samples both twins send before CALLS, so that the frames compared carry signal: ANS opens with 200 ms of silence
# (modem_connect_tones.c), V.29 training with 48 bauds of it (v29tx.c)
WARMUP = {"mcttx": 1600, "v29_lfsr": 200, "v29_queue": WARM}


def seeds():
    return np.array([(c*37 + 5) & 0x7FFF for c in range(N)], np.uint32)


def frame_in():
    return np.random.default_rng(11).integers(-3000, 3000, (N, 64)).astype(np.int16)


class Dev:
    """Rows of int16 in device tensors: stride 40 (8-sample accesses), and 41 for the last call (element accesses)."""

    def __init__(self):
        import torch
        self.torch = torch
        self.lens = torch.full((N,), -1, dtype=torch.int32, device="cuda")

    def rows(self, k, fill=None):
        stride = 41 if k == len(CALLS) - 1 else 40
        t = self.torch.full((N, stride), 0x5555, dtype=self.torch.int16, device="cuda")
        if fill is not None:
            t[:, :fill.shape[1]] = self.torch.from_numpy(np.array(fill, np.int16)).cuda()
        self.torch.cuda.synchronize()
        return t, stride

    def back(self, t, m):
        self.torch.cuda.synchronize()
        return t.cpu().numpy()[:, :m].copy(), self.lens.cpu().numpy().copy()


def sigtone_tx_device(engine, bank, ptr, m, stride):
    """SigToneTxBank.tx_host()'s loop for rows in device memory: a request is simply acknowledged."""
    pending = engine._check(engine.lib().spangpu_sigtone_tx(bank.h, ptr, engine.MEM_DEVICE, m, stride))
    while pending > 0:
        pending = engine._check(engine.lib().spangpu_sigtone_tx_continue(bank.h, ptr, engine.MEM_DEVICE, stride))


def make_sender(engine, name):
    if name == "dtmf":
        b = engine.TxBank(engine.TX_DTMF, N)
        assert b.put("159#") == 0
    elif name == "fsktx":
        b = engine.FskTxBank(engine.FSK_V21CH2, N, engine.FSKTX_LFSR, seeds())
    elif name == "mcttx":
        b = engine.MctTxBank(engine.MCT_ANS, N)
    elif name == "v18":
        b = engine.V18Bank(engine.V18_MODE_WEITBRECHT_5BIT_4545, N)
        assert (b.put([b"HELLO 123"]*N) >= 0).all()
    elif name == "v29_lfsr":
        b = engine.V29TxBank(N, seeds=seeds())
    elif name == "v29_queue":
        # channel c has (0, 40, 80, 400)[c % 4] bits and is told that no more will come: the first kind ends its shutdown inside CALLS
        b = engine.V29TxBank(N, bit_source=engine.MODEMTX_QUEUE, queue_bits=512)
        rng = np.random.default_rng(3)
        acc = b.put_bits([rng.integers(0, 2, (0, 40, 80, 400)[c % 4]) for c in range(N)])
        assert [int(a) for a in acc] == [(0, 40, 80, 400)[c % 4] for c in range(N)]
        for c in range(N):
            b.end_of_data(c)
    elif name == "sigtone":
        b = engine.SigToneTxBank(engine.SIG_TONE_2280HZ, N)
        b.set_mode(engine.SIG_TONE_1_PRESENT | engine.SIG_TONE_TX_PASSTHROUGH, 0)
    else:
        b = engine.AwgnBank(np.arange(N, dtype=np.int32)*7 + 1, np.full(N, -20.0, np.float32))
    return b


def host_call(engine, name, b, m):
    """(rows, lens or None) of one call with host arrays"""
    if name in ("v29_lfsr", "v29_queue"):
        return b.tx_host(m, lens=True)
    if name == "sigtone":
        return b.tx_host(frame_in()[:, :m]), None
    if name == "awgn":
        return b.tx_host(m), None
    return b.tx_host(m)


def device_call(engine, name, b, dev, k, m):
    if name == "sigtone":
        t, stride = dev.rows(k, frame_in()[:, :m])
        sigtone_tx_device(engine, b, t.data_ptr(), m, stride)
        return dev.back(t, m)[0], None
    t, stride = dev.rows(k)
    if name == "awgn":
        b.tx_device(t.data_ptr(), stride, m)
        b.sync()
        return dev.back(t, m)[0], None
    b.tx_device(t.data_ptr(), stride, m, dev.lens.data_ptr())
    b.sync()
    return dev.back(t, m)


SENDERS = ("dtmf", "fsktx", "mcttx", "v18", "v29_lfsr", "v29_queue", "sigtone", "awgn")


@functools.lru_cache(maxsize=None)
def sender_run(name):
    """The frames of CALLS from the bank called with host arrays, after they were found equal to its twin's."""
    from spandsp_amd import engine
    host, twin = make_sender(engine, name), make_sender(engine, name)
    dev = Dev()
    if name in WARMUP:
        t = dev.torch.zeros((N, WARMUP[name]), dtype=dev.torch.int16, device="cuda")
        for b in (host, twin):
            b.tx_device(t.data_ptr(), WARMUP[name], WARMUP[name])
            b.sync()
    frames = []
    for k, m in enumerate(CALLS):
        rows, lens = host_call(engine, name, host, m)
        rows_d, lens_d = device_call(engine, name, twin, dev, k, m)
        assert rows.shape == (N, m)
        assert np.array_equal(rows, rows_d), (name, k, np.argwhere(rows != rows_d)[:4])
        if lens is not None:
            assert np.array_equal(lens, lens_d), (name, k, lens, lens_d)
        if name == "v29_queue" and k == 2:
            # (by ModemTxCursor: with nothing queued the shutdown is over before this call starts, with 40 bits it is not)
            assert lens[0] == 0 and lens[1] == m, lens[:4]
        rows.setflags(write=False)
        frames.append(rows)
    for c in WATCH:
        assert np.array_equal(host.get_state(c), twin.get_state(c)), (name, c)
    assert any(f.any() for f in frames), name
    host.close()
    twin.close()
    return tuple(frames)


@pytest.mark.parametrize("name", SENDERS)
def test_sender_host_and_device_callers_agree(built, name):
    sender_run(name)


def make_receiver(engine, name):
    if name == "fsk":
        return engine.FskBank(engine.FSK_V21CH2, N, engine.FSK_FRAME_MODE_ASYNC), "fsktx"
    if name == "mct":
        return engine.MctBank(engine.MCT_ANS, N), "mcttx"
    if name == "sigtone":
        b = engine.SigToneRxBank(engine.SIG_TONE_2280HZ, N)
        b.set_mode(engine.SIG_TONE_RX_PASSTHROUGH)
        return b, "sigtone"
    return engine.V18Bank(engine.V18_MODE_WEITBRECHT_5BIT_4545, N), "v18"


def heard(name, b):
    if name == "v18":
        return b.text()
    return [np.asarray(e).tolist() for e in b.events()]


@pytest.mark.parametrize("name", ["fsk", "mct", "sigtone", "v18"])
def test_receiver_host_and_device_callers_agree(built, name):
    from spandsp_amd import engine
    host, source = make_receiver(engine, name)
    twin, _ = make_receiver(engine, name)
    frames = sender_run(source)
    dev = Dev()
    for k, m in enumerate(CALLS):
        left = host.rx_host(frames[k])
        t, stride = dev.rows(k, frames[k])
        twin.rx_device(t.data_ptr(), m, stride)
        twin.sync()
        assert heard(name, host) == heard(name, twin), (name, k)
        if name == "sigtone":
            assert np.array_equal(left, dev.back(t, m)[0]), k       # the frame as the receivers left it
    for c in WATCH:
        assert np.array_equal(host.get_state(c), twin.get_state(c)), (name, c)
    host.close()
    twin.close()


def one_call(engine, kind, b):
    if kind in SENDERS:
        host_call(engine, kind, b, 8)
    else:
        b.rx_host(np.zeros((N, 8), np.int16))


BANKS = SENDERS + ("rx_fsk", "rx_mct", "rx_sigtone")


def make_bank(engine, kind):
    return make_receiver(engine, kind[3:])[0] if kind.startswith("rx_") else make_sender(engine, kind)


@pytest.mark.parametrize("kind", BANKS)
def test_a_callers_stream_stays_the_callers(built, kind):
    import torch
    from spandsp_amd import engine
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    b = make_bank(engine, kind)
    for s in streams:
        if kind == "sigtone":
            engine._check(engine.lib().spangpu_sigtone_tx_set_stream(b.h, ctypes.c_void_p(s.cuda_stream)))
        else:
            b.set_stream(ctypes.c_void_p(s.cuda_stream))
        one_call(engine, kind, b)
    b.close()
    for s in streams:
        with torch.cuda.stream(s):
            x = torch.arange(16, device="cuda")*2
        s.synchronize()
        assert int(x.sum()) == 240
    # a bank that made its own stream takes it along: every round's return codes are checked by the wrappers
    for _ in range(32):
        make_bank(engine, kind).close()


def changed(before, after):
    return set(np.nonzero(np.asarray(before) != np.asarray(after))[0].tolist())


def test_windowed_word_edits_touch_one_channel(built):
    from spandsp_amd import engine
    FT_SCALING, FT_SHUTDOWN = 3, 7              # fsktx_dev.hpp
    VT_BASE_GAIN, VT_GAIN = 1, 2                # modemtx_dev.hpp
    b = engine.FskTxBank(engine.FSK_V21CH2, N, engine.FSKTX_LFSR, seeds())
    b.tx_host(40)                               # phases, baud fractions and registers that a restart has something to reset in
    before = {c: b.get_state(c) for c in (0, 1, 68, 69)}
    b.power(0, -23.0)
    b.restart(69, engine.FSK_V23CH1)
    after = {c: b.get_state(c) for c in (0, 1, 68, 69)}
    assert changed(before[1], after[1]) == set() and changed(before[68], after[68]) == set()
    assert changed(before[0], after[0]) == {FT_SCALING}
    diff = changed(before[69], after[69])
    assert diff and diff <= set(range(FT_SHUTDOWN + 1)), diff
    b.close()

    v = engine.V29TxBank(N, seeds=seeds())
    v.tx_host(40)
    before = {c: v.get_state(c) for c in (63, 64, 65)}
    v.power(64, -20.0)
    after = {c: v.get_state(c) for c in (63, 64, 65)}
    assert changed(before[63], after[63]) == set() and changed(before[65], after[65]) == set()
    assert changed(before[64], after[64]) == {VT_BASE_GAIN, VT_GAIN}
    v.close()

    q = engine.V29TxBank(N, bit_source=engine.MODEMTX_QUEUE, queue_bits=512)
    q.put_bits([[1, 0]*10, [1, 1, 0]*10, [0, 1]*20], first=4)
    before = {c: q.get_state(c) for c in (4, 5, 6)}
    q.end_of_data(5)
    assert [q.queued(c) for c in (3, 4, 5, 6, 7)] == [0, 20, 30, 40, 0]
    for c in (4, 5, 6):
        assert changed(before[c], q.get_state(c)) == set()
    # channel 5 alone was told: its neighbours are still waiting for more data when their rings run dry
    q.tx_host(WARM + 200, lens=True)
    ended = [ch for ch, what in q.events() if what == engine.MODEMTX_END_OF_DATA]
    q.tx_host(400, lens=True)
    ended += [ch for ch, what in q.events() if what == engine.MODEMTX_END_OF_DATA]
    assert ended == [5], ended
    q.close()
