"""The GSM 06.10 codec banks on the GPU, for equality with what the reference's gsm0610_*.c produced (tests/golden/gsm0610.npz,
written by tests/golden/make_golden_gsm0610.py): codes, samples, counts and state words call for call on the five lines and the
random code bytes, per-channel lengths of 0 to 3 frames, strides and rows in device memory, set_packing, restart and state
moved between channels and banks, and a device-resident chain from PCM rows to PCM rows.  Everything is integer arithmetic:
every comparison is equality.

The base shape is 72 channels: a full wave and a partial one; channel c has packing c mod 3 and line (c div 3) mod 5 (or the
random bytes), so every wave mixes the three packings and the 72 channels hold every case."""
import numpy as np
import pytest

import gsm0610_lines as GL
from spandsp_amd import engine
from test_g726_gpu import DevBytes

pytestmark = pytest.mark.gpu

N = 72
BAD = -2


@pytest.fixture(scope="module")
def cases():
    return {(c.kind, c.packing, c.line): c for c in GL.cases(GL.load())}


def packing_of(c):
    return GL.PACKINGS[c % 3]


def line_of(c, with_rnd):
    k = (c//3) % (6 if with_rnd else 5)
    return "rnd" if k == 5 else k


def bank_of(kind, n=N, packings=GL.PACKINGS):
    return engine.Gsm0610Bank(n, kind, list(packings))


def run_cases(bank, kind, chans, lens_of=None, check_words=True):
    """Every channel of `bank` through its case (chans[c]) on the fixture's schedule -- or the frames lens_of(c) gives per call
    -- with per-channel lengths; each call's outputs and counts, and on the fixture's schedule every channel's state words,
    against the fixture."""
    n = bank.n
    dtype = np.int16 if kind == GL.ENCODE else np.uint8

    def items(c, frames):
        p = chans[c].packing
        return frames*GL.FRAME if kind == GL.ENCODE else frames*GL.unit_bytes(p)//(2 if p == GL.WAV49 else 1)

    def made(c, frames):
        p = chans[c].packing
        return frames*GL.FRAME if kind == GL.DECODE else frames*GL.unit_bytes(p)//(2 if p == GL.WAV49 else 1)

    frames_of = [GL.calls(GL.N_FRAMES, chans[c].packing) if lens_of is None else lens_of(c) for c in range(n)]
    at, got = [0]*n, [0]*n
    ticks = max(len(x) for x in frames_of)
    most = max(items(c, f) for c in range(n) for f in frames_of[c])
    for k in range(ticks):
        fr = [x[k] if k < len(x) else 0 for x in frames_of]
        lens = np.array([items(c, fr[c]) for c in range(n)], np.int32)
        rows = np.zeros((n, most), dtype)
        for c in range(n):
            rows[c, :lens[c]] = np.asarray(chans[c].data)[at[c]:at[c] + lens[c]]
        before = [bank.get_state(c) for c in range(n) if fr[c] == 0]
        out, counts = bank.encode_host(rows, most, lens) if kind == GL.ENCODE else bank.decode_host(rows, most, lens)
        sat_out = iter(before)
        for c in range(n):
            case = chans[c]
            assert counts[c] == made(c, fr[c]), (case.name, c, k)
            if lens_of is None and k < len(case.calls):
                assert lens[c] == case.calls[k][0] and counts[c] == case.calls[k][1], (case.name, c, k)
            want = np.asarray(case.want)[got[c]:got[c] + counts[c]]
            assert np.array_equal(out[c, :counts[c]], want), (case.name, c, k, np.flatnonzero(out[c, :len(want)] != want)[:4])
            at[c] += int(lens[c])
            got[c] += int(counts[c])
            if fr[c] == 0:
                # a channel that sits a call out keeps its state
                assert np.array_equal(bank.get_state(c), next(sat_out)), (case.name, c, k)
            elif lens_of is None and check_words:
                assert np.array_equal(bank.get_state(c), case.calls[k][2]), (case.name, c, k)
    for c in range(n):
        assert at[c] == len(chans[c].data) and got[c] == len(chans[c].want), (chans[c].name, c)
        assert np.array_equal(bank.get_state(c), chans[c].calls[-1][2]), (chans[c].name, c)


@pytest.mark.parametrize("n", [N, 1])
def test_encoder_parity(built, cases, n):
    # (the one-channel bank runs the VoIP case of the pulse train: channel 0 of the big one has no packing)
    chans = [cases[(GL.ENCODE, packing_of(c), line_of(c, False))] for c in range(N)] if n == N else [cases[(GL.ENCODE, GL.VOIP, 1)]]
    assert n == 1 or {(c.packing, c.line) for c in chans} == {(p, li) for p in GL.PACKINGS for li in range(5)}
    bank = engine.Gsm0610Bank(n, GL.ENCODE, [c.packing for c in chans])
    assert all(np.array_equal(bank.get_state(c), GL.load()["init"][chans[c].packing]) for c in range(n))
    run_cases(bank, GL.ENCODE, chans)


@pytest.mark.parametrize("n", [N, 1])
def test_decoder_parity(built, cases, n):
    # (the sixth "line" is the random code bytes: lags outside 40 .. 120 keep the last lag)
    chans = [cases[(GL.DECODE, packing_of(c), line_of(c, True))] for c in range(N)] if n == N else [cases[(GL.DECODE, GL.WAV49, "rnd")]]
    assert n == 1 or {(c.packing, c.line) for c in chans} == {(p, li) for p in GL.PACKINGS for li in (0, 1, 2, 3, 4, "rnd")}
    bank = engine.Gsm0610Bank(n, GL.DECODE, [c.packing for c in chans])
    run_cases(bank, GL.DECODE, chans)


def test_the_other_directions_call_is_refused(built):
    enc, dec = bank_of(GL.ENCODE, 8), bank_of(GL.DECODE, 8)
    with pytest.raises(engine.SpanGpuError):
        enc.decode_host(np.zeros((8, 4940), np.uint8), 4940)
    with pytest.raises(engine.SpanGpuError):
        dec.encode_host(np.zeros((8, 320), np.int16), 320)


# frames per call: 0, 1, 2 and 3 in one call, the rotations of one list, so that every channel has taken its 12 frames at the
# end; a WAV49 channel takes pairs: 0, 2 and 4
VAR = (1, 0, 3, 2, 0, 2, 1, 3)
VAR_WAV49 = (2, 0, 4, 2, 0, 4)


def rotated(c):
    v = VAR_WAV49 if packing_of(c) == GL.WAV49 else VAR
    r = (c//3) % len(v)
    return list(v[r:] + v[:r])


@pytest.mark.parametrize("kind", [GL.ENCODE, GL.DECODE])
def test_per_channel_lengths(built, cases, kind):
    chans = [cases[(kind, packing_of(c), line_of(c, False))] for c in range(N)]
    bank = engine.Gsm0610Bank(N, kind, [c.packing for c in chans])
    assert {f for c in range(N) for f in rotated(c)} == {0, 1, 2, 3, 4} and all(sum(rotated(c)) == GL.N_FRAMES for c in range(N))
    run_cases(bank, kind, chans, lens_of=rotated)
    # a call nobody brings anything to leaves counts of zero and the state alone
    before = [bank.get_state(c) for c in range(N)]
    zero = np.zeros(N, np.int32)
    if kind == GL.ENCODE:
        out, counts = bank.encode_host(np.zeros((N, 320), np.int16), 320, zero)
    else:
        out, counts = bank.decode_host(np.zeros((N, 4940), np.uint8), 4940, zero)
    assert not counts.any() and all(np.array_equal(bank.get_state(c), before[c]) for c in range(N))
    # a partial frame: refused before anything is queued, and every channel is as it was
    L = engine.lib()
    if kind == GL.ENCODE:
        rows = np.ones((N, 320), np.int16)
        codes = np.zeros((N, 160), np.uint8)
        tail = (codes.ctypes.data, engine.MEM_HOST, 160, None)

        def call(lens, most):
            return L.spangpu_gsm0610_encode(bank.h, rows.ctypes.data, engine.MEM_HOST, 640, None if lens is None else lens.ctypes.data, most, *tail)

        lens = np.full(N, 320, np.int32)
        for c, v in ((64, 159), (64, 161), (1, 160), (65, 1)):      # channel 1 and 64: WAV49 takes 320; 65: VoIP
            bad = lens.copy()
            bad[c] = v
            assert packing_of(1) == packing_of(64) == GL.WAV49 and call(bad, 320) == BAD, (c, v)
        assert call(None, 160) == BAD and call(None, 319) == BAD        # (160 for all: not a WAV49 pair)
        ok = np.zeros(N, np.int32)
        ok[65] = 160
        assert call(ok, 320) == 0
        before[65] = bank.get_state(65)
    else:
        rows = np.ones((N, 4940), np.uint8)
        pcm = np.zeros((N, 160*150), np.int16)
        tail = (pcm.ctypes.data, engine.MEM_HOST, pcm.strides[0], None)

        def call(lens, most):
            return L.spangpu_gsm0610_decode(bank.h, rows.ctypes.data, engine.MEM_HOST, 4940, None if lens is None else lens.ctypes.data, most, *tail)

        lens = np.array([GL.unit_bytes(packing_of(c)) for c in range(N)], np.int32)
        assert call(lens, 76) == 0
        before = [bank.get_state(c) for c in range(N)]
        for c, v in ((0, 75), (1, 33), (2, 65), (64, 64), (65, 34), (66, 77)):
            bad = lens.copy()
            bad[c] = v
            assert call(bad, 77) == BAD, (c, v)
        assert call(None, 76) == BAD and call(None, 33) == BAD and call(None, 65) == BAD    # no length is whole for all three
        assert call(None, 4940*33) == BAD                                                  # (76*65*33 would be, past the row)
    assert all(np.array_equal(bank.get_state(c), before[c]) for c in range(N))


def test_strides_and_device_rows(built, cases):
    chans = [cases[(GL.ENCODE, packing_of(c), line_of(c, False))] for c in range(N)]
    n = 320
    rows = np.array([c.data[:n] for c in chans], np.int16)
    want_bytes = np.array([GL.unit_bytes(packing_of(c))*(1 if packing_of(c) == GL.WAV49 else 2) for c in range(N)], np.int32)
    ref_codes = np.zeros((N, 152), np.uint8)
    for c in range(N):
        ref_codes[c, :want_bytes[c]] = chans[c].want[:want_bytes[c]]
    dchans = [cases[(GL.DECODE, packing_of(c), line_of(c, False))] for c in range(N)]
    # host rows wider than the call
    wide = np.full((N, n + 37), 0x5AA5, np.int16)
    wide[:, :n] = rows
    bank = bank_of(GL.ENCODE)
    assert bank.encode_capacity(n) == 152 and bank.encode_capacity(160) == 76 and bank.encode_capacity(159) == 0
    codes, counts = bank.encode_host(wide, n)
    assert np.array_equal(counts, want_bytes)
    for c in range(N):
        assert np.array_equal(codes[c, :counts[c]], ref_codes[c, :counts[c]]), c
    # device rows wider than the call: strides of 1024, 256 and 1024 bytes, every byte of the output rows 0xA5 beforehand
    L = engine.lib()
    pcm, out, back = DevBytes(N*1024), DevBytes(N*256), DevBytes(N*2048)
    try:
        padded = np.zeros((N, 512), np.int16)
        padded[:, :n] = rows
        pcm.put(padded)
        out.put(np.full((N, 256), 0xA5, np.uint8))
        back.put(np.full((N, 2048), 0xA5, np.uint8))
        bank = bank_of(GL.ENCODE)
        counts = bank.encode_device(pcm.ptr, 1024, n, out.ptr, 256, counts=True)
        got = out.get((N, 256))
        assert np.array_equal(counts, want_bytes)
        for c in range(N):
            assert np.array_equal(got[c, :counts[c]], ref_codes[c, :counts[c]]), c
            # nothing past the 16-byte boundary behind a row's count
            assert (got[c, (counts[c] + 15) & ~15:] == 0xA5).all(), c
            # ... and zeros up to it
            assert not got[c, counts[c]:(counts[c] + 15) & ~15].any(), c
        dec = bank_of(GL.DECODE)
        assert dec.decode_capacity(152) == 640 and dec.decode_capacity(65) == 320 and dec.decode_capacity(32) == 0
        # (152 bytes are four VoIP frames to a decoder that is told no lengths: a PCM row of 1 280 bytes)
        assert L.spangpu_gsm0610_decode(dec.h, out.ptr, engine.MEM_DEVICE, 256, None, 152, back.ptr, engine.MEM_DEVICE, 1024, None) == BAD
        samples = dec.decode_device(out.ptr, 256, 152, back.ptr, 2048, lens=counts, counts=True)
        got = back.get((N, 2048))
        assert (samples == n).all()
        for c in range(N):
            assert np.array_equal(got[c, :2*n].view(np.int16), dchans[c].want[:n]), c
            assert (got[c, 2*n:] == 0xA5).all(), c
        words = bank.get_state(7)
        # refused: a stride that is no multiple of 16, a base that is not, a stride shorter than the row rounded up to 16
        args = (None, n, out.ptr, engine.MEM_DEVICE, 256, None)
        assert L.spangpu_gsm0610_encode(bank.h, pcm.ptr, engine.MEM_DEVICE, 648, *args) == BAD
        assert L.spangpu_gsm0610_encode(bank.h, pcm.ptr.value + 8, engine.MEM_DEVICE, 1024, *args) == BAD
        assert L.spangpu_gsm0610_encode(bank.h, pcm.ptr, engine.MEM_DEVICE, 624, *args) == BAD
        assert L.spangpu_gsm0610_encode(bank.h, pcm.ptr, engine.MEM_DEVICE, 1024, None, n, out.ptr, engine.MEM_DEVICE, 144, None) == BAD
        assert L.spangpu_gsm0610_encode(bank.h, pcm.ptr, engine.MEM_DEVICE, 1024, None, n, out.ptr.value + 4, engine.MEM_DEVICE, 256, None) == BAD
        assert L.spangpu_gsm0610_decode(dec.h, out.ptr, engine.MEM_DEVICE, 250, counts.ctypes.data, 152, back.ptr, engine.MEM_DEVICE, 2048, None) == BAD
        # a host stride shorter than the row, a bad memory kind
        spare = np.zeros((N, 256), np.uint8)
        assert L.spangpu_gsm0610_encode(bank.h, rows.ctypes.data, engine.MEM_HOST, 2*n - 1, None, n, spare.ctypes.data, engine.MEM_HOST, 256, None) == BAD
        assert L.spangpu_gsm0610_encode(bank.h, rows.ctypes.data, 7, 2*n, None, n, spare.ctypes.data, engine.MEM_HOST, 256, None) == BAD
        assert L.spangpu_gsm0610_encode(bank.h, rows.ctypes.data, engine.MEM_HOST, 2*n, None, n, spare.ctypes.data, engine.MEM_HOST, 151, None) == BAD
        # a refused call changes nothing
        assert np.array_equal(bank.get_state(7), words)
    finally:
        pcm.free()
        out.free()
        back.free()
    # the capacities of one-packing banks
    assert bank_of(GL.ENCODE, 8, [GL.VOIP]).encode_capacity(480) == 99 and bank_of(GL.ENCODE, 8, [GL.WAV49]).encode_capacity(480) == 65
    assert bank_of(GL.DECODE, 8, [GL.VOIP]).decode_capacity(99) == 480 and bank_of(GL.DECODE, 8, [GL.NONE]).decode_capacity(99) == 160


def test_set_packing_restart_and_state_moved(built, cases):
    """The parameters do not depend on the packing, so a stream that changes packing between calls is the fixture's streams
    spliced; a restarted channel equals a fresh one; a stream moved to another channel or bank goes on where it was."""
    line = 1
    enc = {p: cases[(GL.ENCODE, p, line)] for p in GL.PACKINGS}
    dec = {p: cases[(GL.DECODE, p, line)] for p in GL.PACKINGS}
    pcm = np.asarray(enc[GL.VOIP].data, np.int16)
    bank = bank_of(GL.ENCODE, 6, [GL.VOIP, GL.NONE])

    def feed(b, chans, first, frames):
        rows = np.zeros((b.n, frames*160), np.int16)
        lens = np.zeros(b.n, np.int32)
        for c in chans:
            rows[c] = pcm[first*160:(first + frames)*160]
            lens[c] = frames*160
        return b.encode_host(rows, frames*160, lens)

    # frames 0-1 as VoIP on channels 0 and 2; then channel 0 turns to WAV49 for frames 2-5, then to NONE for 6-7
    out, counts = feed(bank, (0, 2), 0, 2)
    assert counts[0] == 66 and np.array_equal(out[0, :66], enc[GL.VOIP].want[:66]) and np.array_equal(out[2, :66], out[0, :66])
    bank.set_packing(0, GL.WAV49)
    w = bank.get_state(0)
    assert w[GL.W_PACKING] == GL.WAV49 and np.array_equal(w[1:], bank.get_state(2)[1:])
    assert bank.encode_capacity(320) == 152             # channels 1, 3, 5 are unpacked
    out, counts = feed(bank, (0,), 2, 4)
    assert counts[0] == 130 and np.array_equal(out[0, :130], enc[GL.WAV49].want[65:195]) and not counts[1:].any()
    bank.set_packing(0, GL.NONE)
    out, counts = feed(bank, (0,), 6, 2)
    assert counts[0] == 152 and np.array_equal(out[0, :152], enc[GL.NONE].want[6*76:8*76])
    # the words after 8 frames are the fixture's after its calls of 1, 3, 2, 1 (7 frames) and 2, 4, 2 (8 frames): WAV49's fifth
    want = enc[GL.WAV49].calls[2][2].copy()
    want[GL.W_PACKING] = GL.NONE
    assert np.array_equal(bank.get_state(0), want)
    # the stream moves to channel 5 of another bank and goes on there: frames 8-11
    other = bank_of(GL.ENCODE, 6, [GL.WAV49])
    other.set_state(5, bank.get_state(0))
    assert other.encode_capacity(320) == 152            # (a NONE channel among the WAV49 ones now)
    out, counts = feed(other, (5,), 8, 4)
    assert counts[5] == 304 and np.array_equal(out[5, :304], enc[GL.NONE].want[8*76:]) and not counts[:5].any()
    want = enc[GL.NONE].calls[-1][2]
    assert np.array_equal(other.get_state(5), want)
    # channel 2 starts over in mid-stream, as WAV49: it equals a fresh channel from here on
    bank.restart(2, GL.WAV49)
    fresh = bank_of(GL.ENCODE, 1, [GL.WAV49])
    assert np.array_equal(bank.get_state(2), fresh.get_state(0)) and np.array_equal(fresh.get_state(0), GL.load()["init"][GL.WAV49])
    out, counts = feed(bank, (2,), 0, 2)
    assert counts[2] == 65 and np.array_equal(out[2, :65], enc[GL.WAV49].want[:65])
    assert np.array_equal(bank.get_state(2), enc[GL.WAV49].calls[0][2])
    # the decoder's side: VoIP frames 0-3 on channel 0, the state to channel 3, which goes on with frames 4-5 as WAV49 bytes
    d = bank_of(GL.DECODE, 4, [GL.VOIP])
    rows = np.zeros((4, 132), np.uint8)
    rows[0] = dec[GL.VOIP].data[:132]
    out, counts = d.decode_host(rows, 132, np.array([132, 0, 0, 0], np.int32))
    assert counts[0] == 640 and np.array_equal(out[0, :640], dec[GL.VOIP].want[:640])
    w = d.get_state(0)
    assert np.array_equal(w, dec[GL.VOIP].calls[1][2])
    d.set_state(3, w)
    d.set_packing(3, GL.WAV49)
    rows[:] = 0
    rows[3, :65] = dec[GL.WAV49].data[130:195]
    out, counts = d.decode_host(rows, 132, np.array([0, 0, 0, 65], np.int32))
    assert counts[3] == 320 and np.array_equal(out[3, :320], dec[GL.WAV49].want[640:960])
    want = dec[GL.VOIP].calls[2][2].copy()
    want[GL.W_PACKING] = GL.WAV49
    assert np.array_equal(d.get_state(3), want)
    # what is refused: words no codec could have left, packings outside the three
    for word, value in ((GL.W_PACKING, 3), (GL.W_PACKING, -1), (GL.W_J, 2), (GL.W_J, -1), (GL.W_NRP, 39), (GL.W_NRP, 121)):
        bad = w.copy()
        bad[word] = value
        with pytest.raises(engine.SpanGpuError):
            d.set_state(1, bad)
    for call in (d.restart, d.set_packing):
        for p in (3, -1):
            with pytest.raises(engine.SpanGpuError):
                call(1, p)
    with pytest.raises(engine.SpanGpuError):
        d.set_packing(4, GL.VOIP)
    assert np.array_equal(d.get_state(1), GL.load()["init"][GL.VOIP])


def test_device_resident_chain(built, cases):
    """PCM rows in HBM -> encoder bank -> codes in HBM -> decoder bank -> int16 rows, call for call on one stream, the
    lengths of the decoder from the encoder's counts of the fixture; nothing comes back but the rows to compare."""
    n, frames = N, 4
    chans = [cases[(GL.ENCODE, packing_of(c), line_of(c, False))] for c in range(n)]
    dchans = [cases[(GL.DECODE, packing_of(c), line_of(c, False))] for c in range(n)]
    enc = engine.Gsm0610Bank(n, GL.ENCODE, [c.packing for c in chans])
    dec = engine.Gsm0610Bank(n, GL.DECODE, [c.packing for c in chans])
    samples = frames*GL.FRAME
    cap = enc.encode_capacity(samples)
    # (304 bytes are nine VoIP frames to a decoder that is told no lengths: the PCM row holds the worst channel's)
    row = dec.decode_capacity(cap)
    assert cap == 4*76 and row == 9*160
    bytes_of = np.array([GL.unit_bytes(packing_of(c))*frames//(2 if packing_of(c) == GL.WAV49 else 1) for c in range(n)], np.int32)
    a, codes, b = DevBytes(n*samples*2), DevBytes(n*cap), DevBytes(n*row*2)
    try:
        for k in range(GL.N_FRAMES//frames):
            a.put(np.array([c.data[k*samples:(k + 1)*samples] for c in chans], np.int16))
            enc.encode_device(a.ptr, 2*samples, samples, codes.ptr, cap)
            enc.sync()              # (the two banks have streams of their own)
            dec.decode_device(codes.ptr, cap, cap, b.ptr, 2*row, lens=bytes_of)
            dec.sync()
            got = b.get((n, row), np.int16)
            for c in range(n):
                assert np.array_equal(got[c, :samples], dchans[c].want[k*samples:(k + 1)*samples]), (c, k)
        for c in range(n):
            assert np.array_equal(enc.get_state(c), chans[c].calls[-1][2]) and np.array_equal(dec.get_state(c), dchans[c].calls[-1][2]), c
    finally:
        for d in (a, codes, b):
            d.free()
