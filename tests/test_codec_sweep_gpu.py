"""The codec and concealment banks on the GPU against the live reference, at bank scale: 4 133 generated lines (64 full waves
and a partial one of 37; tests/codec_sweep.py) through the G.726, G.722 and GSM 06.10 banks and the packet loss concealment
bank, every wave mixing every configuration, signal family and call length, with the reference's own functions run on the
same input through oracle/ref_codecs.py.  Everything is equality: every output item and count of every call of every line,
every line's state words after the last call, and after every call the words of the probe lines (c % 61 == 0, each wave's
first and last lane) and of the lines that sit the call out (length 0: nothing made, row and words unchanged).  The codecs' rows
lie in device memory, where what a call may write behind a row's items is laid down (include/spangpu.h), and is checked.

What this reaches that the host-compiled programs cannot: the wave-wide parts of the kernels -- the concealer's pitch search
over the lanes whose gap starts in the same call, the G.726 tandem path a lane runs because a neighbour needs it -- and the
data-dependent addressing of the row windows and of the GSM working memory."""
import ctypes as C
import time

import numpy as np
import pytest

import codec_sweep as S
import g722_lines as G2
import g726_lines as G6
import gsm0610_lines as GS
import plc_lines as PL
from spandsp_amd import engine
from test_g726_gpu import DevBytes

pytestmark = pytest.mark.gpu

N = S.N_GPU
SENT = np.int16(PL.SENTINEL)


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_codecs
    if not ref_codecs.available():
        pytest.fail("oracle/_ref/libspandsp_codecs_ref.so is not here: `make -C oracle ref` builds it where the reference's sources "
                    "are, and it travels with the tree; without it the sweep has nothing to compare with")
    return ref_codecs


@pytest.fixture(autouse=True)
def timed(request):
    t0 = time.time()
    yield
    print("%s: %.2f s" % (request.node.name, time.time() - t0))


def differ(r, what, i, k, got, want):
    """the first difference of two item arrays, named in full"""
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    m = min(len(got), len(want))
    d = np.flatnonzero(got[:m] != want[:m])
    j = int(d[0]) if len(d) else m
    cfg = tuple(r["cfgs"][i].tolist()) if "cfgs" in r else ()
    pytest.fail("%s %s: configuration %s, line %d (wave %d, lane %d), call %d, %s %d: got %s, the reference has %s; %d against %d items "
                "(seed %#x)" % (r["family"], {0: "encode", 1: "decode"}.get(r.get("kind"), ""), cfg, i, i//S.WAVE, i % S.WAVE, k, what, j,
                                got[j] if j < len(got) else None, want[j] if j < len(want) else None, len(got), len(want), r["seed"]))


def check_words(r, bank, k, key="words"):
    """after call k: the words of every line they are asked of (the probes, the lines sitting out, and at the end all)"""
    for i in np.flatnonzero(r["want"][k]).tolist():
        got, want = bank.get_state(i), r[key][i][k]
        if not np.array_equal(got, want):
            differ(r, "state word", i, k, got, want)


def left_out_cap(lens):
    """no call leaves a quarter of the lines out"""
    assert ((lens == 0).mean(axis=1) < 0.25).all(), (lens == 0).mean(axis=1)


FILL = 0xA5


def round16(n):
    return (n + 15) & ~15


def run_codec(r, bank, encode, el_in, out_dtype):
    """Every line of sweep r through `bank`, call by call, on rows in device memory: the input rows the call's width rounded up
    to 16 bytes apart, the output rows the bank's capacity.  el_in[i]: bytes an input item of line i takes; out_dtype(i): what
    an output item of line i is.  Of an output row the items are compared, and what lies behind them: bytes past the 16-byte
    boundary behind the count are as they were, and the whole row of a line that sits the call out."""
    lens = r["lens"]
    left_out_cap(lens)
    n = lens.shape[1]
    most = int(lens.max())
    data = [np.ascontiguousarray(d).view(np.uint8) for d in r["data"]]
    dtypes = [out_dtype(i) for i in range(n)]
    size = np.array([dt.itemsize for dt in dtypes])
    in_stride = round16(most*int(max(el_in)))
    cap = bank.encode_capacity(most) if encode else bank.decode_capacity(most)
    out_stride = round16(max(16, cap*int(size.max())))
    din, dout = DevBytes(n*in_stride), DevBytes(n*out_stride)
    at = np.zeros(n, np.int64)
    got = np.zeros(n, np.int64)
    cols = np.arange(out_stride)[None, :]
    try:
        for k in range(len(lens)):
            rows = np.zeros((n, in_stride), np.uint8)
            nbytes = lens[k]*el_in
            for i in range(n):
                rows[i, :nbytes[i]] = data[i][at[i]:at[i] + nbytes[i]]
            at += nbytes
            din.put(rows)
            dout.put(np.full((n, out_stride), FILL, np.uint8))
            call = bank.encode_device if encode else bank.decode_device
            counts = call(din.ptr, in_stride, most, dout.ptr, out_stride, lens=lens[k], counts=True)
            out = dout.get((n, out_stride))
            if not np.array_equal(counts, r["counts"][k]):
                i = int(np.flatnonzero(counts != r["counts"][k])[0])
                differ(r, "count", i, k, counts[i:i + 1], r["counts"][k][i:i + 1])
            for i in np.flatnonzero(counts).tolist():
                c = int(counts[i])
                items = out[i, :c*size[i]].view(dtypes[i])
                want = r["out"][i][got[i]:got[i] + c]
                if not np.array_equal(items, want):
                    differ(r, "output item", i, k, items, want)
            got += counts
            # (a line that brings something and makes nothing may have written its first chunk)
            edge = np.where(lens[k] == 0, 0, np.maximum(16, (counts*size + 15) & ~15))
            kept = (out == FILL) | (cols < edge[:, None])
            if not kept.all():
                i = int(np.flatnonzero(~kept.all(axis=1))[0])
                differ(r, "row of a line sitting out, byte" if lens[k, i] == 0 else "past the count's 16-byte boundary, byte", i, k,
                       np.where(cols[0] < edge[i], FILL, out[i]), np.full(out_stride, FILL))
            check_words(r, bank, k)
    finally:
        din.free()
        dout.free()
    for i in range(n):
        assert at[i] == len(data[i]) and got[i] == len(r["out"][i]), (r["family"], i)


U8, I16 = np.dtype(np.uint8), np.dtype(np.int16)


def test_g726_encode(built, ref):
    r = S.sweep_g726(G6.ENCODE)
    cfgs = r["cfgs"]
    assert all(len({tuple(c) for c in cfgs[w:w + S.WAVE].tolist()}) == 36 for w in range(0, N - S.WAVE, S.WAVE))
    assert 900 <= r["lens"].sum(axis=0).mean() <= 1100
    bank = engine.G726Bank(N, cfgs[:, 0], cfgs[:, 1], cfgs[:, 2])
    el = np.where(cfgs[:, 1] == G6.LINEAR, 2, 1)
    run_codec(r, bank, True, el, lambda i: U8)


def test_g726_decode(built, ref):
    """the reference encoder's codes on odd lines, any bytes on even lines"""
    r = S.sweep_g726(G6.DECODE)
    cfgs = r["cfgs"]
    bank = engine.G726Bank(N, cfgs[:, 0], cfgs[:, 1], cfgs[:, 2])
    run_codec(r, bank, False, np.ones(N, np.int64), lambda i: I16 if cfgs[i, 1] == G6.LINEAR else U8)


def g722_bank(direction, cfgs):
    return engine.G722Bank(N, direction, cfgs[:, 0], [G2.options_of(int(e), int(p)) for _, e, p in cfgs])


def test_g722_encode(built, ref):
    r = S.sweep_g722(G2.ENCODE)
    cfgs = r["cfgs"]
    assert all(len({tuple(c) for c in cfgs[w:w + S.WAVE].tolist()}) == 12 for w in range(0, N - S.WAVE, S.WAVE))
    run_codec(r, g722_bank(engine.G722_ENCODER, cfgs), True, np.full(N, 2, np.int64), lambda i: U8)


def test_g722_decode(built, ref):
    r = S.sweep_g722(G2.DECODE)
    run_codec(r, g722_bank(engine.G722_DECODER, r["cfgs"]), False, np.ones(N, np.int64), lambda i: I16)


def test_gsm0610_encode(built, ref):
    r = S.sweep_gsm0610(GS.ENCODE)
    bank = engine.Gsm0610Bank(N, engine.GSM0610_ENCODER, r["cfgs"][:, 0])
    run_codec(r, bank, True, np.full(N, 2, np.int64), lambda i: U8)


def test_gsm0610_decode(built, ref):
    r = S.sweep_gsm0610(GS.DECODE)
    bank = engine.Gsm0610Bank(N, engine.GSM0610_DECODER, r["cfgs"][:, 0])
    run_codec(r, bank, False, np.ones(N, np.int64), lambda i: I16)


def round8(n):
    return (n + 7) & ~7


@pytest.mark.parametrize("where", ["host", "device"])
def test_plc(built, ref, where):
    """run_host on rows of the call's width; run_device on rows in device memory 1 024 bytes apart, every byte of the block
    looked at.  What lies past a line's length: sentinels as they were, but for the zeros a filled-in row carries up to its
    16-byte boundary."""
    r = S.sweep_plc()
    lens, lost = r["lens"], r["lost"]
    left_out_cap(lens)
    most = int(lens.max())
    width = most if where == "host" else 512
    bank = engine.PlcBank(N)
    dev = DevBytes(N*2*width) if where == "device" else None
    at = np.zeros(N, np.int64)
    try:
        for k in range(len(lens)):
            rows = np.full((N, width), SENT, np.int16)
            want = np.full((N, width), SENT, np.int16)
            for i in range(N):
                ln = lens[k, i]
                if ln:
                    rows[i, :ln] = r["data"][i][at[i]:at[i] + ln]
                    want[i, :ln] = r["out"][i][at[i]:at[i] + ln]
                    if lost[k, i]:
                        want[i, ln:min(round8(ln), most)] = 0
            at += lens[k]
            if dev is None:
                out = bank.run_host(rows, most, lens[k], lost[k])
            else:
                dev.put(rows)
                bank.run_device(dev.ptr, 2*width, most, lens[k], lost[k])
                bank.sync()
                out = dev.get((N, width), np.int16)
            if not np.array_equal(out, want):
                i = int(np.flatnonzero((out != want).any(axis=1))[0])
                differ(r, "%s row (length %d), sample" % ("lost" if lost[k, i] else "heard", lens[k, i]), i, k, out[i], want[i])
            check_words(r, bank, k)
    finally:
        if dev is not None:
            dev.free()


def test_decode_then_conceal(built, ref):
    """A GSM 06.10 VoIP decoder bank and conceal() on one stream for 16 ticks; a random subset of the lines brings nothing each
    tick (length 0: the decoder leaves the row alone and the concealer fills it in); nothing is read on the host between the
    two launches."""
    r = S.sweep_chain()
    lost = r["lost"]
    assert 0 < lost.mean(axis=1).min() and lost.mean(axis=1).max() < 1
    dec = engine.Gsm0610Bank(N, engine.GSM0610_DECODER, GS.VOIP)
    plc = engine.PlcBank(N)
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    dec.set_stream(stream)
    plc.set_stream(stream)
    cstride, pstride = 48, 2*PL.FRAME
    codes, pcm = DevBytes(N*cstride), DevBytes(N*pstride)
    want = np.array(r["out"], np.int16)
    frame = np.zeros(N, np.int64)
    try:
        pcm.put(np.full((N, PL.FRAME), SENT, np.int16))
        for k in range(len(lost)):
            rows = np.zeros((N, cstride), np.uint8)
            for i in np.flatnonzero(lost[k] == 0).tolist():
                rows[i, :33] = r["data"][i][33*frame[i]:33*frame[i] + 33]
            frame += lost[k] == 0
            codes.put(rows)
            dec.decode_device(codes.ptr, cstride, 33, pcm.ptr, pstride, lens=np.where(lost[k], 0, 33).astype(np.int32))
            plc.conceal(pcm.ptr, pstride, dec.counts_dev(), PL.FRAME, fill_samples=PL.FRAME)
            plc.sync()
            out = pcm.get((N, PL.FRAME), np.int16)
            if not np.array_equal(out, want[:, k]):
                i = int(np.flatnonzero((out != want[:, k]).any(axis=1))[0])
                differ(r, "%s tick, sample" % ("lost" if lost[k, i] else "heard"), i, k, out[i], want[i, k])
            check_words(r, plc, k)
            check_words(r, dec, k, "dec_words")
        assert all(33*frame[i] == len(r["data"][i]) for i in range(N))
    finally:
        plc.close()
        dec.close()
        codes.free()
        pcm.free()
        hip.hipStreamDestroy(stream)
