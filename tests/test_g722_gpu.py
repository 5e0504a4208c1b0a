"""The G.722 codec banks on the GPU, for equality with what the reference's g722.c produced (tests/golden/g722.npz, written by
tests/golden/make_golden_g722.py): codes, packed bytes, samples, counts and state words call for call on the three lines and
the random-byte line, per-channel lengths, strides and rows in device memory, restart and state moved between channels, a
device-resident chain of 4 096 8 kHz lines between a DTMF sender bank and a DTMF receiver bank, and one of 16 kHz lines.
Everything is integer arithmetic: every comparison is equality.

The base shape is 72 channels: a full wave and a partial one; channel c runs configuration c mod 12, so every wave mixes the
three rates, both sample rates and both packings, and every configuration sits in both waves."""
import ctypes as C

import numpy as np
import pytest

import g722_lines as GL
from spandsp_amd import engine
from test_g726_gpu import DevBytes

pytestmark = pytest.mark.gpu

N = 72
PROBE = (0, 1, 2, 3, 63, 64, N - 1)         # the channels whose state words are read back after every call
BAD = -2


@pytest.fixture(scope="module")
def cases():
    return {(c.kind, c.rate, c.eight_k, c.packed, c.line): c for c in GL.cases(GL.load())}


def config(c):
    return GL.CONFIGS[c % len(GL.CONFIGS)]


def bank_of(kind, n=N, configs=GL.CONFIGS):
    return engine.G722Bank(n, kind, [r for r, _, _ in configs], [GL.options_of(e, p) for _, e, p in configs])


def run_cases(bank, kind, chans, schedule_of=None, probe=PROBE):
    """Every channel of `bank` through its case (chans[c]) on the fixture's schedule -- or schedule_of(c) -- with per-channel
    lengths; each call's outputs, counts and, on the probe channels, state words against the fixture."""
    n = bank.n
    lens_of = [[k[0] for k in chans[c].calls] if schedule_of is None else schedule_of(c) for c in range(n)]
    data = [np.asarray(chans[c].data, np.int16 if kind == GL.ENCODE else np.uint8) for c in range(n)]
    at = [0]*n          # items consumed
    got = [0]*n         # items produced
    ticks = max(len(x) for x in lens_of)
    most = max(max(x) for x in lens_of)
    most += most & 1
    for k in range(ticks):
        lens = np.array([x[k] if k < len(x) else 0 for x in lens_of], np.int32)
        rows = np.zeros((n, most), data[0].dtype)
        for c in range(n):
            rows[c, :lens[c]] = data[c][at[c]:at[c] + lens[c]]
        out, counts = bank.encode_host(rows, most, lens) if kind == GL.ENCODE else bank.decode_host(rows, most, lens)
        for c in range(n):
            case = chans[c]
            if schedule_of is None and k < len(case.calls):
                assert counts[c] == case.calls[k][1], (case.name, c, k)
            elif k >= len(lens_of[c]):
                assert counts[c] == 0, (case.name, c, k)
            else:
                assert counts[c] == case.made(at[c] + int(lens[c])) - case.made(at[c]), (case.name, c, k)
            items = out[c, :counts[c]]
            want = np.asarray(case.want)[got[c]:got[c] + counts[c]]
            assert np.array_equal(items, want), (case.name, c, k, np.flatnonzero(items[:len(want)] != want[:len(items)])[:4])
            at[c] += int(lens[c])
            got[c] += int(counts[c])
        if schedule_of is None:
            for c in probe:
                # (a channel past its last call sits the tick out: its words are still those of its last call)
                j = min(k, len(chans[c].calls) - 1)
                assert np.array_equal(bank.get_state(c), chans[c].calls[j][2]), (chans[c].name, c, k)
    for c in range(n):
        assert at[c] == len(chans[c].data) and got[c] == len(chans[c].want), (chans[c].name, c)


@pytest.mark.parametrize("line", [0, 1, 2])
def test_encoder_parity(built, cases, line):
    bank = bank_of(GL.ENCODE)
    chans = [cases[(GL.ENCODE,) + config(c) + (line,)] for c in range(N)]
    run_cases(bank, GL.ENCODE, chans)
    for c in range(N):
        assert np.array_equal(bank.get_state(c), chans[c].calls[-1][2]), c


@pytest.mark.parametrize("line", [0, 1, 2, "rnd"])
def test_decoder_parity(built, cases, line):
    # ("rnd": bytes with bits set above the code width, which an unpacked decoder ignores)
    bank = bank_of(GL.DECODE)
    chans = [cases[(GL.DECODE,) + config(c) + (line,)] for c in range(N)]
    run_cases(bank, GL.DECODE, chans)
    for c in range(N):
        assert np.array_equal(bank.get_state(c), chans[c].calls[-1][2]), c


def test_the_other_directions_call_is_refused(built):
    enc, dec = bank_of(GL.ENCODE, 8), bank_of(GL.DECODE, 8)
    with pytest.raises(engine.SpanGpuError):
        enc.decode_host(np.zeros((8, 16), np.uint8), 16)
    with pytest.raises(engine.SpanGpuError):
        dec.encode_host(np.zeros((8, 16), np.int16), 16)


# lengths with zeros (a channel sits calls out), 1, odd and long entries; the rotations of one list, so that every channel has
# taken the same total at the end.  A 16 kHz encoder takes twice each: pairs.
VAR = (1, 0, 3, 5, 0, 7, 2, 11, 160, 6, 4, 1, 0, 0, 33, 9)


def rotated(c):
    r = (c//12*5 + c) % len(VAR)
    return list(VAR[r:] + VAR[:r])


class Head:
    """the head of a case: `taken` items in, what they make out"""

    def __init__(self, case, taken):
        self.kind, self.rate, self.eight_k, self.packed, self.line, self.name = case.kind, case.rate, case.eight_k, case.packed, case.line, case.name
        self.bps, self.per = GL.bits_of(case.rate), 1 if case.eight_k else 2
        self.packs = case.packed and case.rate != 64000
        self.data = case.data[:taken]
        self.want = case.want[:self.made(taken)]
        self.calls = []

    def made(self, taken):
        """items out of `taken` items in, however they were cut into calls"""
        if self.kind == GL.ENCODE:
            codes = taken//self.per
            return codes*self.bps//8 if self.packs else codes
        # a call ends with the code for which its last byte was read: the cut does not change the stream
        if taken == 0:
            return 0
        return self.per*((8*(taken - 1))//self.bps + 1 if self.packs else taken)


# The same lengths tick after tick, and the ways out of that state (the kept-lengths short cut of a bank's call): A, unequal
# lengths of 0 .. 11 out of VAR; A again from a fresh array; B, A with channel 64 alone changed; E, the same for everybody,
# brought as an array (an even number of samples: the one entry a 16 kHz encoder does not take twice); A; nobody brings
# anything; A.
SMALL = tuple(v for v in VAR if v <= 11)
EQUAL = 8


def kept(c):
    a = SMALL[(c//12*5 + c) % len(SMALL)]
    return [a, a, (a + 7) % 12 if c == 64 else a, None, a, 0, a]


@pytest.mark.parametrize("kind,lens_of", [pytest.param(GL.ENCODE, rotated, id=str(GL.ENCODE)), pytest.param(GL.DECODE, rotated, id=str(GL.DECODE)),
                                          pytest.param(GL.ENCODE, kept, id="kept-%s" % GL.ENCODE), pytest.param(GL.DECODE, kept, id="kept-%s" % GL.DECODE)])
def test_per_channel_lengths(built, cases, kind, lens_of):
    bank = bank_of(kind)

    def schedule(c):
        twice = kind == GL.ENCODE and not config(c)[1]
        return [EQUAL if v is None else 2*v if twice else v for v in lens_of(c)]

    heads = [Head(cases[(kind,) + config(c) + (0,)], sum(schedule(c))) for c in range(N)]
    run_cases(bank, kind, heads, schedule_of=schedule)
    # a channel that sat calls out equals its twins, which sat other calls out: same stream (checked above against the
    # fixture), same state
    for c in range(12, N if lens_of is rotated else 0):
        assert np.array_equal(bank.get_state(c), bank.get_state(c % 12)), c
    # ... and a tick nobody brings anything to leaves counts of zero and the state alone
    before = [bank.get_state(c) for c in range(N)]
    zero = np.zeros(N, np.int32)
    if kind == GL.ENCODE:
        out, counts = bank.encode_host(np.zeros((N, 16), np.int16), 8, zero)
    else:
        out, counts = bank.decode_host(np.zeros((N, 16), np.uint8), 8, zero)
    assert not counts.any() and all(np.array_equal(bank.get_state(c), before[c]) for c in range(N))
    if kind == GL.ENCODE:
        # an odd length on a 16 kHz encoder: refused before anything is queued, and every channel is as it was
        L = engine.lib()
        rows = np.ones((N, 16), np.int16)
        codes = np.zeros((N, 16), np.uint8)
        lens = np.full(N, 8, np.int32)
        lens[64] = 7                # configuration 4: 56000, 16 kHz
        assert not config(64)[1]
        args = (codes.ctypes.data, engine.MEM_HOST, 16, None)
        assert L.spangpu_g722_encode(bank.h, rows.ctypes.data, engine.MEM_HOST, 32, lens.ctypes.data, 8, *args) == BAD
        assert L.spangpu_g722_encode(bank.h, rows.ctypes.data, engine.MEM_HOST, 32, None, 7, *args) == BAD
        assert all(np.array_equal(bank.get_state(c), before[c]) for c in range(N))
        # (an 8 kHz encoder takes it)
        lens[:] = 0
        lens[2] = 7
        assert config(2)[1]
        assert L.spangpu_g722_encode(bank.h, rows.ctypes.data, engine.MEM_HOST, 32, lens.ctypes.data, 8, *args) == 0


def test_strides_and_device_rows(built, cases):
    chans = [cases[(GL.ENCODE,) + config(c) + (0,)] for c in range(N)]
    n = 160
    rows = np.zeros((N, n), np.int16)
    for c in range(N):
        rows[c] = chans[c].data[:n]
    ref_codes, ref_counts = bank_of(GL.ENCODE).encode_host(rows, n)
    assert set(ref_counts.tolist()) == {60, 70, 80, 120, 140, 160}
    ref_pcm, ref_samples = bank_of(GL.DECODE).decode_host(ref_codes, ref_codes.shape[1], ref_counts)
    # host rows wider than the call
    wide = np.full((N, n + 37), 0x5AA5, np.int16)
    wide[:, :n] = rows
    bank = bank_of(GL.ENCODE)
    codes, counts = bank.encode_host(wide, n)
    assert np.array_equal(counts, ref_counts)
    for c in range(N):
        assert np.array_equal(codes[c, :counts[c]], ref_codes[c, :counts[c]]), c
    # device rows wider than the call: strides of 512, 256 and 1024 bytes, every byte of the output rows 0xA5 beforehand
    L = engine.lib()
    pcm, out, back = DevBytes(N*512), DevBytes(N*256), DevBytes(N*1024)
    try:
        padded = np.zeros((N, 256), np.int16)
        padded[:, :n] = rows
        pcm.put(padded)
        out.put(np.full((N, 256), 0xA5, np.uint8))
        back.put(np.full((N, 1024), 0xA5, np.uint8))
        bank = bank_of(GL.ENCODE)
        assert bank.encode_capacity(n) == 160
        counts = bank.encode_device(pcm.ptr, 512, n, out.ptr, 256, counts=True)
        got = out.get((N, 256))
        assert np.array_equal(counts, ref_counts)
        for c in range(N):
            assert np.array_equal(got[c, :counts[c]], ref_codes[c, :counts[c]]), c
            # nothing past the 16-byte boundary behind a row's count: the guard bytes beyond the capacity among them
            assert (got[c, (counts[c] + 15) & ~15:] == 0xA5).all(), c
        dec = bank_of(GL.DECODE)
        cap = dec.decode_capacity(160)
        assert cap == 2*((7 + 8*160)//6) and 2*cap <= 1024
        samples = dec.decode_device(out.ptr, 256, 160, back.ptr, 1024, lens=counts, counts=True)
        got = back.get((N, 1024))
        assert np.array_equal(samples, ref_samples)
        for c in range(N):
            assert np.array_equal(got[c, :2*samples[c]].view(np.int16), ref_pcm[c, :samples[c]]), c
            assert (got[c, (2*samples[c] + 15) & ~15:] == 0xA5).all(), c
        words = bank.get_state(7)
        # refused: a stride that is no multiple of 16, a base that is not, a stride shorter than the row rounded up to 16
        args = (None, n, out.ptr, engine.MEM_DEVICE, 256, None)
        assert L.spangpu_g722_encode(bank.h, pcm.ptr, engine.MEM_DEVICE, 328, *args) == BAD
        assert L.spangpu_g722_encode(bank.h, pcm.ptr.value + 8, engine.MEM_DEVICE, 512, *args) == BAD
        assert L.spangpu_g722_encode(bank.h, pcm.ptr, engine.MEM_DEVICE, 304, *args) == BAD
        assert L.spangpu_g722_encode(bank.h, pcm.ptr, engine.MEM_DEVICE, 512, None, n, out.ptr, engine.MEM_DEVICE, 144, None) == BAD
        assert L.spangpu_g722_encode(bank.h, pcm.ptr, engine.MEM_DEVICE, 512, None, n, out.ptr.value + 4, engine.MEM_DEVICE, 256, None) == BAD
        assert L.spangpu_g722_decode(dec.h, out.ptr, engine.MEM_DEVICE, 250, None, n, back.ptr, engine.MEM_DEVICE, 1024, None) == BAD
        # (160 bytes decode to 428 samples on the worst channel: 856 bytes a row)
        assert L.spangpu_g722_decode(dec.h, out.ptr, engine.MEM_DEVICE, 256, None, n, back.ptr, engine.MEM_DEVICE, 848, None) == BAD
        # a host stride shorter than the row, a bad memory kind
        spare = np.zeros((N, 256), np.uint8)
        assert L.spangpu_g722_encode(bank.h, rows.ctypes.data, engine.MEM_HOST, 2*n - 1, None, n, spare.ctypes.data, engine.MEM_HOST, 256, None) == BAD
        assert L.spangpu_g722_encode(bank.h, rows.ctypes.data, 7, 2*n, None, n, spare.ctypes.data, engine.MEM_HOST, 256, None) == BAD
        assert L.spangpu_g722_encode(bank.h, rows.ctypes.data, engine.MEM_HOST, 2*n, None, n, spare.ctypes.data, engine.MEM_HOST, 159, None) == BAD
        # a refused call changes nothing
        assert np.array_equal(bank.get_state(7), words)
    finally:
        pcm.free()
        out.free()
        back.free()
    # the capacities of one-configuration banks: waiting bits included
    assert bank_of(GL.ENCODE, 8, [(56000, 1, 1)]).encode_capacity(161) == 141 and bank_of(GL.ENCODE, 8, [(48000, 0, 1)]).encode_capacity(162) == 61
    assert bank_of(GL.DECODE, 8, [(48000, 1, 1)]).decode_capacity(10) == 14 and bank_of(GL.DECODE, 8, [(64000, 0, 1)]).decode_capacity(10) == 20


def test_restart_and_state_moved_between_channels(built, cases):
    # six encoders at 56 kbit/s, 8 kHz, packed: 161 samples leave 7 bits waiting
    cfg = (56000, 1, 1)
    case = cases[(GL.ENCODE,) + cfg + (0,)]
    bank = bank_of(GL.ENCODE, 6, [cfg, (64000, 0, 0)])         # channels 1, 3, 5 are another codec altogether
    data = np.asarray(case.data, np.int16)

    def feed(start, n, chans):
        rows = np.zeros((6, n + (n & 1)), np.int16)
        lens = np.zeros(6, np.int32)
        for c in chans:
            rows[c, :n] = data[start:start + n]
            lens[c] = n
        return bank.encode_host(rows, n + (n & 1), lens)

    out, counts = feed(0, 161, (0, 2))
    assert counts[0] == 140 and np.array_equal(out[0, :140], case.want[:140]) and np.array_equal(out[2, :140], case.want[:140])
    w = bank.get_state(0)
    assert w[GL.W_BITS] == 7 and np.array_equal(w, case.calls[1][2])
    # the stream of channel 0 moves to channel 5 (a 64 kbit/s 16 kHz channel until now) and goes on there, waiting bits included
    bank.set_state(5, w)
    # ... and channel 2 starts over in mid-stream: it equals a fresh channel (4) from here on
    bank.restart(2, cfg[0], GL.options_of(cfg[1], cfg[2]))
    assert np.array_equal(bank.get_state(2), bank.get_state(4))
    out, counts = feed(161, 87, (5,))
    made = (248*7)//8 - 140
    assert counts[5] == made and np.array_equal(out[5, :made], case.want[140:140 + made])
    assert not counts[[0, 1, 2, 3, 4]].any()
    out, counts = feed(0, 161, (2, 4))
    assert np.array_equal(out[2, :140], case.want[:140]) and np.array_equal(out[4, :140], case.want[:140])
    assert np.array_equal(bank.get_state(2), case.calls[1][2]) and np.array_equal(bank.get_state(4), case.calls[1][2])
    # the decoder's side of the same move, at 48 kbit/s, 16 kHz, packed, with the QMF histories part of the way round their
    # rings: after the fixture's first three calls (160 + 1 + 7 bytes) a whole code waits
    dcfg = (48000, 0, 1)
    dcase = cases[(GL.DECODE,) + dcfg + (0,)]
    dec = bank_of(GL.DECODE, 4, [dcfg])
    n0 = sum(k[0] for k in dcase.calls[:3])
    made0 = sum(k[1] for k in dcase.calls[:3])
    rows = np.zeros((4, 176), np.uint8)
    rows[0, :n0] = dcase.data[:n0]
    pcm, counts = dec.decode_host(rows, 176, np.array([n0, 0, 0, 0], np.int32))
    assert counts[0] == made0 and np.array_equal(pcm[0, :made0], dcase.want[:made0])
    w = dec.get_state(0)
    assert np.array_equal(w, dcase.calls[2][2]) and w[GL.W_BITS] >= 6 and w[GL.W_PTR] != 0
    dec.set_state(3, w)
    n1, made1 = dcase.calls[3][0], dcase.calls[3][1]
    rows[:] = 0
    rows[3, :n1] = dcase.data[n0:n0 + n1]
    pcm, counts = dec.decode_host(rows, 176, np.array([0, 0, 0, n1], np.int32))
    assert counts[3] == made1 and np.array_equal(pcm[3, :made1], dcase.want[made0:made0 + made1])
    assert np.array_equal(dec.get_state(3), dcase.calls[3][2])
    # what set_state refuses: words no codec could have left
    for word, value in ((GL.W_BPS, 5), (GL.W_BITS, 8), (GL.W_PTR, 12), (GL.W_PTR, -1), (GL.W_PACKED, 2), (GL.W_EIGHT_K, -1)):
        bad = w.copy()
        bad[word] = value
        with pytest.raises(engine.SpanGpuError):
            dec.set_state(1, bad)
    with pytest.raises(engine.SpanGpuError):
        dec.restart(1, 32000, 0)
    with pytest.raises(engine.SpanGpuError):
        dec.restart(1, 64000, 4)


def test_device_resident_chain_to_a_dtmf_bank(built):
    """DTMF sender bank -> encoder bank -> decoder bank -> DTMF receiver bank at 4 096 8 kHz lines, 30 ticks, on one stream,
    every hop in device memory, against the same chain hop by hop through host memory.  A packed decoder keeps the last code of
    its first tick for the second one: its lines bring the receiver 159 samples, then 160."""
    n, tick, ticks = 4096, 160, 30
    configs = [(r, 1, p) for r in GL.RATES for p in (0, 1)]
    digs = ["159D", "2*80", "#A4C6", "7B3", "0000", "91", "D#*", "852"]
    mine = [digs[(c//6) % 8] for c in range(n)]
    L = engine.lib()
    packed = np.array([bool(configs[c % 6][2]) and configs[c % 6][0] != 64000 for c in range(n)])
    bytes_of = np.array([tick*GL.bits_of(configs[c % 6][0])//8 if packed[c] else tick for c in range(n)], np.int32)

    def chain(device):
        tx = engine.TxBank(engine.TX_DTMF, n)
        rx = engine.ToneBank(engine.DTMF, n)
        enc, dec = bank_of(GL.ENCODE, n, configs), bank_of(GL.DECODE, n, configs)
        stream = L.spangpu_bank_get_stream(rx.h)
        for b in (tx, enc, dec):
            b.set_stream(stream)
        assert not tx.put_each(mine).any()
        cap = enc.encode_capacity(tick)
        row = (dec.decode_capacity(cap) + 7) & ~7           # samples of a decoded row: a multiple of 16 bytes
        assert cap == tick and dec.decode_capacity(cap) == (7 + 8*tick)//6
        got = [""]*n
        trace = []
        if device:
            a, codes, b = DevBytes(n*tick*2), DevBytes(n*cap), DevBytes(n*row*2)
        try:
            for k in range(ticks):
                samples_of = np.where(packed & (k == 0), tick - 1, tick).astype(np.int32)
                if device:
                    tx.tx_device(a.ptr, tick, tick)
                    enc.encode_device(a.ptr, 2*tick, tick, codes.ptr, cap)
                    dec.decode_device(codes.ptr, cap, cap, b.ptr, 2*row, lens=bytes_of)
                    rx.rx_device_var(b.ptr.value, samples_of, tick, row)
                    rx.sync()
                    if k in (0, 1, ticks - 1):
                        counts = np.zeros(n, np.int32)
                        assert a.hip.hipMemcpy(counts.ctypes.data, dec.counts_dev(), counts.nbytes, 2) == 0
                        assert np.array_equal(counts, samples_of)
                        trace.append((a.get((n, tick), np.int16), codes.get((n, cap)), b.get((n, row), np.int16)))
                else:
                    pcm, _ = tx.tx_host(tick)
                    cd, counts = enc.encode_host(pcm, tick)
                    assert np.array_equal(counts, bytes_of)
                    out, samples = dec.decode_host(cd, cap, bytes_of)
                    assert np.array_equal(samples, samples_of)
                    back = np.zeros((n, row), np.int16)
                    back[:, :out.shape[1]] = out
                    rx.rx_host_var(back[:, :tick], samples_of)
                    if k in (0, 1, ticks - 1):
                        trace.append((pcm, cd, back))
                for r in rx.blocks():
                    if (r["flags"] & engine.BLK_CHANGE) and r["code"]:
                        got[r["channel"]] += chr(r["code"])
            final = [(c, enc.get_state(c), dec.get_state(c)) for c in (0, 1, 2, 3, 4, 5, 63, 64, 2049, n - 1)]
        finally:
            if device:
                for d in (a, codes, b):
                    d.free()
        return got, trace, final

    got_d, trace_d, final_d = chain(True)
    got_h, trace_h, final_h = chain(False)
    assert got_d == got_h
    for k, ((pa, ca, ba), (pb, cb, bb)) in zip((0, 1, ticks - 1), zip(trace_d, trace_h)):
        made = np.where(packed & (k == 0), tick - 1, tick)
        assert np.array_equal(pa, pb)
        for c in range(n):
            assert np.array_equal(ca[c, :bytes_of[c]], cb[c, :bytes_of[c]]), c
            assert np.array_equal(ba[c, :made[c]], bb[c, :made[c]]), c
    for (c, e1, d1), (_, e2, d2) in zip(final_d, final_h):
        assert np.array_equal(e1, e2) and np.array_equal(d1, d2), c
    # replicas: lines with the same configuration and digits are identical (c and c + 48)
    for k, (pa, ca, ba) in zip((0, 1, ticks - 1), trace_d):
        made = np.where(packed & (k == 0), tick - 1, tick)
        for c in range(48, n):
            assert np.array_equal(ba[c, :made[c]], ba[c - 48, :made[c]]) and np.array_equal(ca[c, :bytes_of[c]], ca[c - 48, :bytes_of[c]]), c
    assert got_d[48:] == got_d[:-48]
    # the chain carries the signal: some line delivers the digits it was given
    assert any(g == m for g, m in zip(got_d, mine))


def test_device_resident_chain_at_16_khz(built):
    """encode -> decode of 16 kHz lines, the codes staying in device memory, against the same through host memory."""
    n, tick, ticks = 256, 320, 8
    configs = [(r, 0, p) for r in GL.RATES for p in (0, 1)]
    lines = GL.lines()
    src = np.array([np.roll(lines[c % 3], 7*c)[:tick*ticks] for c in range(n)], np.int16)
    packed = np.array([bool(configs[c % 6][2]) and configs[c % 6][0] != 64000 for c in range(n)])
    bytes_of = np.array([(tick//2)*GL.bits_of(configs[c % 6][0])//8 if packed[c] else tick//2 for c in range(n)], np.int32)

    def chain(device):
        enc, dec = bank_of(GL.ENCODE, n, configs), bank_of(GL.DECODE, n, configs)
        cap = enc.encode_capacity(tick)
        row = (dec.decode_capacity(cap) + 7) & ~7
        assert cap == tick//2
        outs = []
        if device:
            a, codes, b = DevBytes(n*tick*2), DevBytes(n*cap), DevBytes(n*row*2)
        try:
            for k in range(ticks):
                samples_of = np.where(packed & (k == 0), tick - 2, tick).astype(np.int32)
                rows = np.ascontiguousarray(src[:, k*tick:(k + 1)*tick])
                if device:
                    a.put(rows)
                    enc.encode_device(a.ptr, 2*tick, tick, codes.ptr, cap)
                    enc.sync()          # (the two banks have streams of their own)
                    samples = dec.decode_device(codes.ptr, cap, cap, b.ptr, 2*row, lens=bytes_of, counts=True)
                    out = b.get((n, row), np.int16)
                else:
                    cd, counts = enc.encode_host(rows, tick)
                    assert np.array_equal(counts, bytes_of)
                    out, samples = dec.decode_host(cd, cap, bytes_of)
                assert np.array_equal(samples, samples_of)
                outs.append([out[c, :samples[c]].copy() for c in range(n)])
            final = [(enc.get_state(c), dec.get_state(c)) for c in range(n)]
        finally:
            if device:
                for d in (a, codes, b):
                    d.free()
        return outs, final

    outs_d, final_d = chain(True)
    outs_h, final_h = chain(False)
    for k in range(ticks):
        for c in range(n):
            assert np.array_equal(outs_d[k][c], outs_h[k][c]), (k, c)
    for c in range(n):
        assert np.array_equal(final_d[c][0], final_h[c][0]) and np.array_equal(final_d[c][1], final_h[c][1]), c
