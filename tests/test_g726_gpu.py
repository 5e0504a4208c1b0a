"""The G.726 codec banks on the GPU, for equality with what the reference's g726.c produced (tests/golden/g726.npz, written by
tests/golden/make_golden_g726.py): codes, packed bytes, samples, counts and state words call for call on the three lines and
the random-code line, per-channel lengths, strides, restart and state moved between channels, and a device-resident chain
of 4 096 lines in front of a DTMF receiver bank.  Everything is integer arithmetic: every comparison is equality.

The base shape is 72 channels: a full wave and a partial one; channel c runs configuration c mod 36, so every wave holds
all four rates, three codings and three packings, and every configuration sits in both."""
import ctypes as C

import numpy as np
import pytest

import g726_lines as GL
from spandsp_amd import engine

pytestmark = pytest.mark.gpu

N = 72
PROBE = (0, 1, 2, 3, 63, 64, N - 1)         # the channels whose state words are read back after every call


@pytest.fixture(scope="module")
def cases():
    return {(c.kind, c.rate, c.coding, c.packing, c.line): c for c in GL.cases(GL.load())}


def config(c):
    return GL.CONFIGS[c % len(GL.CONFIGS)]


def bank_of(n=N, configs=GL.CONFIGS):
    r, c, p = zip(*configs)
    return engine.G726Bank(n, r, c, p)


def el(coding):
    return 2 if coding == GL.LINEAR else 1


def as_bytes(items, coding, kind):
    """a case's input items as the bytes of a row"""
    if kind == GL.ENCODE and coding == GL.LINEAR:
        return np.asarray(items, np.int16).view(np.uint8)
    return np.asarray(items, np.uint8)


def out_items(row_bytes, count, coding, kind):
    """`count` items of an output row: codes are bytes, PCM is int16 or G.711 bytes"""
    if kind == GL.DECODE and coding == GL.LINEAR:
        return row_bytes[:2*count].view(np.int16)
    return row_bytes[:count]


def run_cases(bank, kind, chans, schedule_of=None, probe=PROBE):
    """Every channel of `bank` through its case (chans[c]) on the fixture's schedule -- or schedule_of(c) -- with per-channel
    lengths; each call's outputs, counts and, on the probe channels, state words against the fixture.  Returns ticks made."""
    n = bank.n
    lens_of = [[k[0] for k in chans[c].calls] if schedule_of is None else schedule_of(c) for c in range(n)]
    data = [as_bytes(chans[c].data, chans[c].coding, kind) for c in range(n)]
    at = [0]*n          # items consumed
    got = [0]*n         # items produced
    ticks = max(len(x) for x in lens_of)
    most = max(max(x) for x in lens_of)
    width = 2*most if kind == GL.ENCODE else most
    for k in range(ticks):
        lens = np.array([x[k] if k < len(x) else 0 for x in lens_of], np.int32)
        rows = np.zeros((n, width), np.uint8)
        for c in range(n):
            w = el(chans[c].coding) if kind == GL.ENCODE else 1
            rows[c, :lens[c]*w] = data[c][at[c]*w:(at[c] + lens[c])*w]
        if kind == GL.ENCODE:
            out, counts = bank.encode_host(rows, most, lens)
        else:
            out, counts = bank.decode_host(rows, most, lens)
        for c in range(n):
            case = chans[c]
            if schedule_of is None and k < len(case.calls):
                assert counts[c] == case.calls[k][1], (case.name, c, k)
            elif k >= len(lens_of[c]):
                assert counts[c] == 0, (case.name, c, k)
            else:
                assert counts[c] == case.made(at[c] + int(lens[c])) - case.made(at[c]), (case.name, c, k)
            items = out_items(out[c], int(counts[c]), case.coding, kind)
            want = np.asarray(case.want)[got[c]:got[c] + counts[c]]
            assert np.array_equal(items, want), (case.name, c, k, np.flatnonzero(items[:len(want)] != want[:len(items)])[:4])
            at[c] += int(lens[c])
            got[c] += int(counts[c])
        if schedule_of is None:
            for c in probe:
                # (a channel past its last call sits the tick out: its words are still those of its last call)
                j = min(k, len(chans[c].calls) - 1)
                words = chans[c].calls[j][2]
                if words is not None:
                    assert np.array_equal(bank.get_state(c), words), (chans[c].name, c, k)
    for c in range(n):
        assert at[c] == len(chans[c].data) and got[c] == len(chans[c].want), (chans[c].name, c)
    return ticks


@pytest.mark.parametrize("line", [0, 1, 2])
def test_encoder_parity(built, cases, line):
    bank = bank_of()
    chans = [cases[(GL.ENCODE,) + config(c) + (line,)] for c in range(N)]
    run_cases(bank, GL.ENCODE, chans)
    for c in range(N):
        assert np.array_equal(bank.get_state(c), chans[c].calls[-1][2]), c


@pytest.mark.parametrize("line", [0, 1, 2])
def test_decoder_parity(built, cases, line):
    bank = bank_of()
    chans = [cases[(GL.DECODE,) + config(c) + (line,)] for c in range(N)]
    run_cases(bank, GL.DECODE, chans)
    for c in range(N):
        assert np.array_equal(bank.get_state(c), chans[c].calls[-1][2]), c


def test_decoder_parity_on_random_codes(built, cases):
    # bytes with bits set above the code width, which an unpacked decoder drops: the 12 unpacked configurations
    configs = [(r, c, GL.PACK_NONE) for r in GL.RATES for c in GL.CODINGS]
    bank = bank_of(N, configs)
    chans = [cases[(GL.DECODE,) + configs[c % 12] + ("rnd",)] for c in range(N)]
    run_cases(bank, GL.DECODE, chans)


# lengths that leave every residue a rate can leave (an odd number of 3- or 5-bit codes, 1 .. 7 of them), a channel that
# sits calls out, and a long call; the rotations of one list, so that every channel has taken the same total at the end
VAR = (1, 0, 3, 5, 0, 7, 2, 11, 160, 6, 4, 1, 0, 0, 33, 9)


def rotated(c):
    r = (c//36*5 + c) % len(VAR)
    return list(VAR[r:] + VAR[:r])


# The same lengths tick after tick, and the ways out of that state (the kept-lengths short cut of a bank's call): A, unequal
# lengths of 0 .. 11 out of VAR; A again from a fresh array; B, A with channel 64 alone changed; E, the same for everybody,
# brought as an array; A; nobody brings anything; A.
SMALL = tuple(v for v in VAR if v <= 11)
EQUAL = 8


def kept(c):
    a = SMALL[(c//36*5 + c) % len(SMALL)]
    return [a, a, (a + 7) % 12 if c == 64 else a, EQUAL, a, 0, a]


@pytest.mark.parametrize("kind,schedule_of", [pytest.param(GL.ENCODE, rotated, id=str(GL.ENCODE)), pytest.param(GL.DECODE, rotated, id=str(GL.DECODE)),
                                              pytest.param(GL.ENCODE, kept, id="kept-%s" % GL.ENCODE), pytest.param(GL.DECODE, kept, id="kept-%s" % GL.DECODE)])
def test_per_channel_lengths(built, cases, kind, schedule_of):
    bank = bank_of()
    chans = [cases[(kind,) + config(c) + (0,)] for c in range(N)]

    class Head:
        """the head of a case: `total` items in, what they make out"""
        def __init__(self, case, total):
            bps = case.rate//8000
            self.kind, self.rate, self.coding, self.packing, self.line, self.name = case.kind, case.rate, case.coding, case.packing, case.line, case.name
            self.data = case.data[:total]
            self.bits = (1, 1) if case.packing == GL.PACK_NONE else (bps, 8) if kind == GL.ENCODE else (8, bps)
            self.want = case.want[:self.made(total)]
            self.calls = []

        def made(self, taken):
            """items out of `taken` items in, however they were cut into calls"""
            return taken*self.bits[0]//self.bits[1]

    heads = [Head(x, sum(schedule_of(c))) for c, x in enumerate(chans)]
    assert run_cases(bank, kind, heads, schedule_of=schedule_of) == len(schedule_of(0))
    # every residue the rate can leave was left behind by some call, in both packings
    if kind == GL.ENCODE and schedule_of is rotated:
        for bps, reach in ((2, {2, 4, 6}), (3, set(range(1, 8))), (4, {4}), (5, set(range(1, 8)))):
            seen = {(sum(rotated(c)[:k])*bps) % 8 for c in range(N) if config(c)[0] == 8000*bps for k in range(len(VAR))}
            assert seen >= reach, (bps, seen)
    # a channel that sat calls out equals its twin in the other wave position class, which sat other calls out: same stream
    # (checked above against the fixture), same state
    for c in range(36 if schedule_of is rotated else 0):
        assert np.array_equal(bank.get_state(c), bank.get_state(c + 36)), c
    # ... and a tick nobody brings anything to leaves counts of zero and the state alone
    before = bank.get_state(5)
    rows = np.zeros((N, 16), np.uint8)
    zero = np.zeros(N, np.int32)
    out, counts = bank.encode_host(rows, 8, zero) if kind == GL.ENCODE else bank.decode_host(rows, 8, zero)
    assert not counts.any() and np.array_equal(bank.get_state(5), before)


class DevBytes:
    """bytes in HBM"""

    def __init__(self, nbytes):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.nbytes = nbytes
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), nbytes) == 0
        assert self.hip.hipMemset(self.ptr, 0, nbytes) == 0

    def put(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes and self.hip.hipMemcpy(self.ptr, a.ctypes.data, a.nbytes, 1) == 0

    def get(self, shape, dtype=np.uint8):
        a = np.zeros(shape, dtype)
        assert a.nbytes <= self.nbytes and self.hip.hipMemcpy(a.ctypes.data, self.ptr, a.nbytes, 2) == 0
        return a

    def free(self):
        self.hip.hipFree(self.ptr)


def test_strides(built, cases):
    chans = [cases[(GL.ENCODE,) + config(c) + (0,)] for c in range(N)]
    n = 160
    rows = np.zeros((N, 2*n), np.uint8)
    for c in range(N):
        w = el(chans[c].coding)
        rows[c, :n*w] = as_bytes(chans[c].data, chans[c].coding, GL.ENCODE)[:n*w]
    ref_codes, ref_counts = bank_of().encode_host(rows, n)
    # host rows wider than the call
    wide = np.full((N, 2*n + 37), 0xA5, np.uint8)
    wide[:, :2*n] = rows
    bank = bank_of()
    codes, counts = bank.encode_host(wide, n)
    assert np.array_equal(counts, ref_counts)
    for c in range(N):
        assert np.array_equal(codes[c, :counts[c]], ref_codes[c, :counts[c]]), c
    # device rows wider than the call: strides of 512 and 256 bytes
    L = engine.lib()
    pcm, out = DevBytes(N*512), DevBytes(N*256)
    try:
        padded = np.zeros((N, 512), np.uint8)
        padded[:, :2*n] = rows
        pcm.put(padded)
        bank = bank_of()
        counts = bank.encode_device(pcm.ptr, 512, n, out.ptr, 256, counts=True)
        got = out.get((N, 256))
        assert np.array_equal(counts, ref_counts)
        for c in range(N):
            assert np.array_equal(got[c, :counts[c]], ref_codes[c, :counts[c]]), c
            # nothing past the 16-byte boundary behind a row's count
            assert not got[c, (counts[c] + 15) & ~15:].any(), c
        words = bank.get_state(7)
        # refused: a stride that is no multiple of 16, a base that is not, a stride shorter than the row rounded up to 16
        BAD = -2
        args = (None, n, out.ptr, engine.MEM_DEVICE, 256, None)
        assert L.spangpu_g726_encode(bank.h, pcm.ptr, engine.MEM_DEVICE, 328, *args) == BAD
        assert L.spangpu_g726_encode(bank.h, pcm.ptr.value + 8, engine.MEM_DEVICE, 512, *args) == BAD
        assert L.spangpu_g726_encode(bank.h, pcm.ptr, engine.MEM_DEVICE, 304, *args) == BAD
        assert L.spangpu_g726_encode(bank.h, pcm.ptr, engine.MEM_DEVICE, 512, None, n, out.ptr, engine.MEM_DEVICE, 152, None) == BAD
        assert L.spangpu_g726_encode(bank.h, pcm.ptr, engine.MEM_DEVICE, 512, None, n, out.ptr.value + 4, engine.MEM_DEVICE, 256, None) == BAD
        assert L.spangpu_g726_decode(bank.h, out.ptr, engine.MEM_DEVICE, 250, None, n, pcm.ptr, engine.MEM_DEVICE, 512, None) == BAD
        # (160 bytes decode to 640 samples at 16 kbit/s: 1280 bytes a row)
        assert L.spangpu_g726_decode(bank.h, out.ptr, engine.MEM_DEVICE, 256, None, n, pcm.ptr, engine.MEM_DEVICE, 512, None) == BAD
        # a host stride shorter than the row, a bad memory kind
        spare = np.zeros((N, 256), np.uint8)
        assert L.spangpu_g726_encode(bank.h, rows.ctypes.data, engine.MEM_HOST, 2*n - 1, None, n, spare.ctypes.data, engine.MEM_HOST, 256, None) == BAD
        assert L.spangpu_g726_encode(bank.h, rows.ctypes.data, 7, 2*n, None, n, spare.ctypes.data, engine.MEM_HOST, 256, None) == BAD
        assert L.spangpu_g726_encode(bank.h, rows.ctypes.data, engine.MEM_HOST, 2*n, None, n, spare.ctypes.data, engine.MEM_HOST, 159, None) == BAD
        # a refused call changes nothing
        assert np.array_equal(bank.get_state(7), words)
    finally:
        pcm.free()
        out.free()
    assert bank.encode_capacity(n) == 160 and bank.decode_capacity(n) == 640
    assert bank_of(8, [(40000, 1, 2)]).encode_capacity(161) == 101 and bank_of(8, [(24000, 0, 1)]).decode_capacity(10) == 27


def test_restart_and_state_moved_between_channels(built, cases):
    # six channels at 24 kbit/s, A-law, left-packed: 161 samples leave 3 bits of residue
    cfg = (24000, GL.ALAW, GL.PACK_LEFT)
    case = cases[(GL.ENCODE,) + cfg + (0,)]
    bank = bank_of(6, [cfg, (32000, GL.LINEAR, GL.PACK_NONE)])         # channels 1, 3, 5 are another codec altogether
    data = np.asarray(case.data, np.uint8)

    def feed(start, n, chans):
        rows = np.zeros((6, 2*n), np.uint8)
        lens = np.zeros(6, np.int32)
        for c in chans:
            rows[c, :n] = data[start:start + n]
            lens[c] = n
        out, counts = bank.encode_host(rows, n, lens)
        return out, counts

    out, counts = feed(0, 161, (0, 2))
    assert counts[0] == 60 and np.array_equal(out[0, :60], case.want[:60]) and np.array_equal(out[2, :60], case.want[:60])
    w = bank.get_state(0)
    assert w[GL.W_RESIDUE] == 3 and np.array_equal(w, case.calls[1][2])
    # the stream of channel 0 moves to channel 5 (a 32 kbit/s linear channel until now) and goes on there, residue included
    bank.set_state(5, w)
    # ... and channel 2 starts over in mid-stream: it equals a fresh channel (4) from here on
    bank.restart(2, *cfg)
    assert np.array_equal(bank.get_state(2), bank.get_state(4))
    out, counts = feed(161, 87, (5,))
    made = (248*3)//8 - 60
    assert counts[5] == made and np.array_equal(out[5, :made], case.want[60:60 + made])
    assert not counts[[0, 1, 2, 3, 4]].any()
    out, counts = feed(0, 161, (2, 4))
    assert np.array_equal(out[2, :60], case.want[:60]) and np.array_equal(out[4, :60], case.want[:60])
    assert np.array_equal(bank.get_state(2), case.calls[1][2]) and np.array_equal(bank.get_state(4), case.calls[1][2])
    # the decoder's side of the same move: 7 bytes of 3-bit codes leave 2 bits behind
    dcase = cases[(GL.DECODE,) + cfg + (0,)]
    dec = bank_of(4, [cfg])
    rows = np.zeros((4, 16), np.uint8)
    rows[0, :7] = dcase.data[:7]
    pcm, counts = dec.decode_host(rows, 7, np.array([7, 0, 0, 0], np.int32))
    assert counts[0] == 18 and np.array_equal(pcm[0, :18], dcase.want[:18])
    w = dec.get_state(0)
    assert w[GL.W_RESIDUE] == 2
    dec.set_state(3, w)
    rows[3, :9] = dcase.data[7:16]
    pcm, counts = dec.decode_host(rows, 9, np.array([0, 0, 0, 9], np.int32))
    assert counts[3] == (16*8)//3 - 18 and np.array_equal(pcm[3, :counts[3]], dcase.want[18:18 + counts[3]])
    # what set_state refuses: words g726_init() could not have made
    bad = w.copy()
    bad[28] = 5
    with pytest.raises(engine.SpanGpuError):
        dec.set_state(1, bad)
    bad = w.copy()
    bad[GL.W_RESIDUE] = 9
    with pytest.raises(engine.SpanGpuError):
        dec.set_state(1, bad)
    with pytest.raises(engine.SpanGpuError):
        dec.restart(1, 8000, 0, 0)


def test_device_resident_chain(built):
    """DTMF sender bank -> encode -> decode -> DTMF receiver bank at 4 096 lines, every hop in device memory, against the
    same chain hop by hop through host memory; then a decoder's counts straight into an FSK receiver's per-channel lengths."""
    n, tick, ticks = 4096, 160, 30
    configs = [(r, GL.LINEAR, p) for r in GL.RATES for p in GL.PACKINGS]        # the rows of a DTMF bank are int16
    digs = ["159D", "2*80", "#A4C6", "7B3", "0000", "91", "D#*", "852"]
    mine = [digs[(c//12) % 8] for c in range(n)]
    L = engine.lib()

    def chain(device):
        tx = engine.TxBank(engine.TX_DTMF, n)
        rx = engine.ToneBank(engine.DTMF, n)
        enc, dec = bank_of(n, configs), bank_of(n, configs)
        stream = L.spangpu_bank_get_stream(rx.h)
        for b in (tx, enc, dec):
            b.set_stream(stream)
        assert not tx.put_each(mine).any()
        cap = enc.encode_capacity(tick)
        assert cap == tick and dec.decode_capacity(cap) == 4*tick
        bytes_of = np.array([tick*(config12(c)[0]//8000)//8 if config12(c)[2] else tick for c in range(n)], np.int32)
        got = [""]*n
        trace = []
        if device:
            a, codes, b = DevBytes(n*tick*2), DevBytes(n*cap), DevBytes(n*4*tick*2)
        try:
            for k in range(ticks):
                if device:
                    tx.tx_device(a.ptr, tick, tick)
                    enc.encode_device(a.ptr, 2*tick, tick, codes.ptr, cap)
                    dec.decode_device(codes.ptr, cap, cap, b.ptr, 8*tick, lens=bytes_of)
                    rx.rx_device(b.ptr.value, tick, 4*tick)
                    rx.sync()
                    if k in (0, 3, ticks - 1):
                        trace.append((a.get((n, tick), np.int16), codes.get((n, cap)), b.get((n, 4*tick), np.int16)[:, :tick]))
                else:
                    pcm, _ = tx.tx_host(tick)
                    cd, counts = enc.encode_host(pcm, tick)
                    assert np.array_equal(counts, bytes_of)
                    out, samples = dec.decode_host(cd, cap, bytes_of)
                    assert (samples == tick).all()
                    back = np.ascontiguousarray(out.view(np.int16)[:, :tick])
                    rx.rx_host(back)
                    if k in (0, 3, ticks - 1):
                        trace.append((pcm, cd, back))
                for r in rx.blocks():
                    if (r["flags"] & engine.BLK_CHANGE) and r["code"]:
                        got[r["channel"]] += chr(r["code"])
            counts_dev = dec.counts_dev()
            final = [(c, enc.get_state(c), dec.get_state(c)) for c in (0, 1, 63, 64, 2049, n - 1)]
        finally:
            if device:
                for d in (a, codes, b):
                    d.free()
        assert counts_dev
        return got, trace, final

    def config12(c):
        return configs[c % 12]

    got_d, trace_d, final_d = chain(True)
    got_h, trace_h, final_h = chain(False)
    assert got_d == got_h
    bytes_of = np.array([tick*(config12(c)[0]//8000)//8 if config12(c)[2] else tick for c in range(n)])
    for (pa, ca, ba), (pb, cb, bb) in zip(trace_d, trace_h):
        assert np.array_equal(pa, pb) and np.array_equal(ba, bb)
        for c in range(n):
            assert np.array_equal(ca[c, :bytes_of[c]], cb[c, :bytes_of[c]]), c
    for (c, e1, d1), (_, e2, d2) in zip(final_d, final_h):
        assert np.array_equal(e1, e2) and np.array_equal(d1, d2), c
    # replicas: lines with the same configuration and digits are identical (c and c + 96)
    for pa, ca, ba in trace_d:
        for c in range(96, n):
            assert np.array_equal(ba[c], ba[c - 96]) and np.array_equal(ca[c, :bytes_of[c]], ca[c - 96, :bytes_of[c]]), c
    assert got_d[96:] == got_d[:-96]
    # the chain carries the signal: some line delivers the digits it was given
    assert any(g == m for g, m in zip(got_d, mine))


def test_decoder_counts_feed_an_fsk_receiver(built, cases):
    """The samples a decoder made, per channel, go to spangpu_fsk_rx_lens_dev() from device memory, with no read-back: the
    receiver's events equal those of a receiver given the same rows and lengths from the host."""
    n = N
    configs = [(r, GL.LINEAR, p) for r in GL.RATES for p in GL.PACKINGS]
    dec = bank_of(n, configs)
    fsk_d = engine.FskBank(engine.FSK_V21CH1, n)
    fsk_h = engine.FskBank(engine.FSK_V21CH1, n)
    L = engine.lib()
    chans = [cases[(GL.DECODE,) + configs[c % 12] + (0,)] for c in range(n)]
    nbytes = 80
    rows = np.zeros((n, nbytes), np.uint8)
    lens = np.array([(c*7) % (nbytes + 1) for c in range(n)], np.int32)
    for c in range(n):
        rows[c, :lens[c]] = chans[c].data[:lens[c]]
    cap = dec.decode_capacity(nbytes)
    codes, pcm = DevBytes(n*nbytes), DevBytes(n*cap*2)
    try:
        codes.put(rows)
        dec.decode_device(codes.ptr, nbytes, nbytes, pcm.ptr, 2*cap, lens=lens)
        dec.sync()          # (the two banks have streams of their own)
        engine._check(L.spangpu_fsk_rx_lens_dev(fsk_d.h, pcm.ptr, engine.MEM_DEVICE, cap, cap, dec.counts_dev()))
        ev_d = fsk_d.events()
        host = pcm.get((n, cap), np.int16)
        counts = np.zeros(n, np.int32)
        assert codes.hip.hipMemcpy(counts.ctypes.data, dec.counts_dev(), counts.nbytes, 2) == 0
    finally:
        codes.free()
        pcm.free()
    want = np.array([lens[c] if configs[c % 12][2] == 0 else lens[c]*8//(configs[c % 12][0]//8000) for c in range(n)])
    assert np.array_equal(counts, want) and (counts == 0).any() and counts.max() > nbytes
    fsk_h.rx_host_var(host, counts)
    ev_h = fsk_h.events()
    assert len(ev_d) == len(ev_h) == n
    for c in range(n):
        assert np.array_equal(ev_d[c], ev_h[c]), c
    for c in PROBE:
        assert np.array_equal(fsk_d.get_state(c), fsk_h.get_state(c)), c
