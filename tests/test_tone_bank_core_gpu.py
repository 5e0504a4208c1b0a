"""The tone bank on the shared host core (spandsp_amd/csrc/tone_api.hip, tone_rx.hip on bank_host.hpp), through engine.py: a
bank fed host frames -- channel-major, sample-major and G.711 bytes in turn, through the one staging block -- and its twin fed
device rows of another stride are replicas of each other across regrowth of that block, with one length for all channels and
with a length per channel; a bank that is handed a caller's stream and then told to make its own again computes what a twin
that never changed streams computes, in queue mode too; and spangpu_banks_own_queues() refuses a bank listed twice without
touching a bank, and leaves distinct banks computing what their twins compute.  The values themselves are pinned to the
oracle by the tone suites; here two banks of this library are compared, bit for bit."""
import os

import numpy as np
import pytest

import g726_lines
import synth

pytestmark = pytest.mark.gpu

N = 70                              # one full wave and a ragged tail
CALLS = (161, 80, 240, 7, 160)      # 161 and 7 are no multiple of 8: staged channel-major rows are longer than the call
FORMATS = ("channel-major", "alaw", "sample-major")     # ... of the host bank, cycled over CALLS: the one staging block, in int16
                                    # units, must hold 11 768, 2 808, 16 808, 568, 5 608: grow, reuse, grow (free and allocate), reuse, reuse
QUEUE_N = 1030                      # channels of the queue-mode bank: five workgroups, so its launches are split over two streams
PAD = 3                             # a host caller's rows are this much longer than the call
WATCH = (0, 63, 64, 69)
TOTAL = 1280                        # samples per channel: the longest test takes 8 calls of 160
SUPER_FREQS = (350.0, 400.0, 440.0, 480.0, 620.0, 950.0, 1100.0, 1400.0, 1800.0, 2100.0, 2400.0, 2600.0)     # the 12-bin kernel
KINDS = ("dtmf", "super12")


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch has its GPU context before this module's first bank is made, as in the soak and the collective tests"""
    import torch
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def lines():
    """kind -> (samples [N][TOTAL], their A-law codes): the samples are what the reference's decoder makes of the codes, so a
    call may take either and mean the same line"""
    table = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g711_decode.npz"))["alaw"]
    out = {}
    for kind, sig in (("dtmf", synth.dtmf_channels(N, TOTAL, seed=71)[0]), ("super12", synth.call_progress_channels(N, TOTAL, seed=72))):
        codes = g726_lines.linear_to_alaw(sig)
        lin = np.ascontiguousarray(table[codes], np.int16)
        lin.setflags(write=False)
        codes.setflags(write=False)
        out[kind] = (lin, codes)
    return out


def make(engine, kind, n=N):
    if kind == "dtmf":
        return engine.ToneBank(engine.DTMF, n)
    return engine.ToneBank(engine.SUPER_TONE, n, bin_fac=[engine.goertzel_fac(f) for f in SUPER_FREQS])


def device_rows(x, m, fill):
    """rows of another stride than a host caller's, so that nothing but the samples is shared"""
    import torch
    t = torch.full((N, m + 5), fill, dtype=torch.uint8 if x.dtype == np.uint8 else torch.int16, device="cuda")
    t[:, :m] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    return t


def same(a, b, what):
    ra, rb = a.blocks(), b.blocks()
    assert ra.tobytes() == rb.tobytes(), what
    for c in WATCH:
        (fa, ia), (fb, ib) = a.get_state(c), b.get_state(c)
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and np.array_equal(ia, ib), (what, c)
    return rb


def state_of(bank):
    return [(f.view(np.uint32).copy(), i.copy()) for f, i in (bank.get_state(c) for c in WATCH)]


def same_state(a, b):
    return all(np.array_equal(fa, fb) and np.array_equal(ia, ib) for (fa, ia), (fb, ib) in zip(a, b))


@pytest.mark.parametrize("kind", KINDS)
def test_host_frames_of_every_format_equal_device_frames(built, lines, kind):
    from spandsp_amd import engine
    lib = engine.lib()
    lin, codes = lines[kind]
    host, dev = make(engine, kind), make(engine, kind)
    at = 0
    valid = hits = 0
    for k, m in enumerate(CALLS):
        fmt = FORMATS[k % 3]
        if fmt == "alaw":
            rows = np.full((N, m + PAD), 0x55, np.uint8)
            rows[:, :m] = codes[:, at:at + m]
            engine._check(lib.spangpu_bank_rx_g711(host.h, rows.ctypes.data, engine.MEM_HOST, engine.G711_ALAW, m, m + PAD))
            t = device_rows(codes[:, at:at + m], m, 0x2A)
            dev.rx_device_g711(t.data_ptr(), engine.G711_ALAW, m, m + 5)
        else:
            if fmt == "channel-major":
                rows = np.full((N, m + PAD), 0x5555, np.int16)
                rows[:, :m] = lin[:, at:at + m]
                layout, stride = engine.CHANNEL_MAJOR, m + PAD
            else:
                rows = np.full((m, N + PAD), 0x5555, np.int16)
                rows[:, :N] = lin[:, at:at + m].T
                layout, stride = engine.SAMPLE_MAJOR, N + PAD
            engine._check(lib.spangpu_bank_rx(host.h, rows.ctypes.data, engine.MEM_HOST, layout, m, stride))
            t = device_rows(lin[:, at:at + m], m, 0x2AAA)
            dev.rx_device(t.data_ptr(), m, m + 5)
        host.sync()
        blocks = same(host, dev, (kind, k, m, fmt))
        valid += len(blocks)
        hits += int((blocks["hit"] > 0).sum() if kind == "dtmf" else (blocks["hit"] >= 0).sum())       # (a super-tone bank: the bin, -1 = none)
        at += m
    # the precondition of the comparison: blocks ended in these calls, and some of them found their tones
    assert valid > 4*N and hits > 0, (kind, valid, hits)
    host.close()
    dev.close()


@pytest.mark.parametrize("kind", KINDS)
def test_host_lengths_equal_device_lengths(built, lines, kind):
    from spandsp_amd import engine
    lib = engine.lib()
    lin, _ = lines[kind]
    host, dev = make(engine, kind), make(engine, kind)
    rng = np.random.default_rng(9)
    m = 160
    at = 0
    for tick in ("ragged", "equal", "ragged", "zero", "ragged", "equal-short", "ragged"):
        # a fresh array every tick: the library's pinned copy of the last one is at another address with other lengths
        if tick == "ragged":
            lens = rng.choice(np.array([0, 7, 80, 160], np.int32), N)
            lens[[0, 63, 64, 69]] = (160, 0, 7, 80)
        else:
            lens = np.full(N, {"equal": 160, "zero": 0, "equal-short": 80}[tick], np.int32)
        before = state_of(host)
        rows = np.full((N, m + PAD), 0x5555, np.int16)
        rows[:, :m] = lin[:, at:at + m]
        engine._check(lib.spangpu_bank_rx_var(host.h, rows.ctypes.data, engine.MEM_HOST, lens.ctypes.data, m, m + PAD))
        host.sync()
        t = device_rows(lin[:, at:at + m], m, 0x2AAA)
        dev.rx_device_var(t.data_ptr(), lens.copy(), m, m + 5)
        same(host, dev, (kind, tick))
        if tick == "zero":
            assert same_state(before, state_of(host)), kind
        else:
            assert not same_state(before, state_of(host)), (kind, tick)
        at += m                                         # (a channel that took less simply loses the rest: both twins alike)
    # a length above max_samples is refused before anything is queued
    before = state_of(host)
    lens = np.full(N, 80, np.int32)
    lens[64] = m + 1
    with pytest.raises(engine.SpanGpuError):
        host.rx_host_var(lin[:, at:at + m], lens)
    with pytest.raises(engine.SpanGpuError):
        dev.rx_device_var(t.data_ptr(), lens, m, m + 5)
    assert same_state(before, state_of(host))
    same(host, dev, (kind, "refused"))
    host.close()
    dev.close()


@pytest.mark.parametrize("queues", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_stream_hand_over(built, lines, kind, queues):
    import torch
    from spandsp_amd import engine
    # queue mode: a bank large enough for split launches (launch_bank() asks for four workgroups), so that the hand-over finds the
    # second stream busy; its channels are the 70 lines over and over
    n = QUEUE_N if queues == 2 else N
    lin = lines[kind][0][np.arange(n) % N]
    moved, still = make(engine, kind, n), make(engine, kind, n)
    assert moved.set_queues(queues) == queues
    rows = torch.from_numpy(np.ascontiguousarray(lin)).cuda()       # device rows 16 bytes aligned: the streaming kernel, which splits
    torch.cuda.synchronize()
    mine = torch.cuda.Stream()

    def tick(at, compare):
        for b in (moved, still):
            b.rx_device(rows.data_ptr() + 2*at, 160, TOTAL)
        if compare:
            same(moved, still, (kind, queues, at))

    # every hand-over comes straight behind a launch, with no call in between that would join the second stream first
    tick(0, False)
    at = 160
    for stream in (mine.cuda_stream, None):
        moved.set_stream(stream)
        if stream is None:
            assert moved.get_stream() != 0 and moved.get_stream() != mine.cuda_stream
        else:
            assert moved.get_stream() == mine.cuda_stream
        tick(at, True)
        tick(at + 160, False)
        at += 320
    same(moved, still, (kind, queues, "end"))
    moved.close()
    still.close()


def test_banks_own_queues(built, lines):
    from spandsp_amd import engine
    lin = lines["dtmf"][0]
    banks = [make(engine, "dtmf") for _ in range(3)]
    twins = [make(engine, "dtmf") for _ in range(3)]

    def step(which, at):
        for k in which:
            for b in (banks[k], twins[k]):
                b.rx_host(lin[:, at:at + 160])
            same(banks[k], twins[k], (k, at))

    step(range(3), 0)
    streams = [b.get_stream() for b in banks]
    with pytest.raises(engine.SpanGpuError):
        engine.banks_own_queues([banks[0], banks[0]])
    assert [b.get_stream() for b in banks] == streams
    step((0, 2), 160)
    proven = engine.banks_own_queues(banks)
    assert 1 <= proven <= 3
    assert len({b.get_stream() for b in banks}) == 3
    step(range(3), 320)
    for b in banks + twins:
        b.close()
