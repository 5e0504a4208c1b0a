"""Writes tests/golden/g722.npz from the live reference.  g722.c is not among the modules of oracle/_ref/libspandsp_ref.so,
so it is compiled here with vector_int.c and alloc.c, in a temporary directory, with the strict flags of oracle/Makefile,
and nothing compiled is kept.  The fixture holds data only; the lines come from tests/g722_lines.py.  <k> is
"<rate>_<eight_k>_<packed>"; G722_PACKED means nothing at 64000, so those streams are stored once, after the generator has
asserted that they equal the unpacked ones.

  offsets             [0 encoder, 1 decoder][word][offset, size] of the state fields the banks' state words map to, in that
                      order, measured by a compiler on the reference's private header;
  enc_schedule_16k, enc_schedule_8k, dec_schedule
                      the call lengths cycled by every case: samples for the encoders, bytes for the decoders;
  line_crcs           CRC-32 of the three lines as generated;
  init                [configuration][0 encoder, 1 decoder][74] the state words g722_*_init() leaves, in the order of CONFIGS;
  codes_<k>           [line][bytes] what the encoder makes of the line;
  ecounts_<k>         [line][call] the bytes each call returned; ewords_<k> [line][call][74] the state words after it (int16:
                      every word fits, asserted);
  pcm_<k>             [line][samples] what the decoder makes of codes_<k>; dcounts_<k>, dwords_<k> as above;
  rnd_<k>, rndcounts_<k>, rndwords_<k>
                      the decoder on g722_lines.random_bytes(), whose bytes have bits set above the code width.

Run from the repository root:  python tests/golden/make_golden_g722.py [reference source dir]"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import g722_lines as gl  # noqa: E402

GOLDEN = os.path.join(HERE, "g722.npz")
STRICT = ["-std=gnu99", "-O2", "-ffp-contract=off", "-fPIC", "-fwrapv"]
DEFS = ["-DHAVE_MATH_H", "-DHAVE_STDBOOL_H", "-DHAVE_SINF", "-DHAVE_COSF", "-DHAVE_TANF", "-DHAVE_ASINF", "-DHAVE_ACOSF", "-DHAVE_ATANF",
        "-DHAVE_ATAN2F", "-DHAVE_CEILF", "-DHAVE_FLOORF", "-DHAVE_POWF", "-DHAVE_EXPF", "-DHAVE_LOGF", "-DHAVE_LOG10F", "-DHAVE_LRINT",
        "-DHAVE_LRINTF", "-DHAVE_LONG_DOUBLE", "-DHAVE_MALLOC_H", "-DHAVE_ALIGNED_ALLOC", "-DHAVE_UNISTD_H", "-DHAVE_STDLIB_H",
        "-DHAVE_STRING_H", "-DHAVE_INTTYPES_H", "-DHAVE_STDINT_H", "-DHAVE_TGMATH_H"]
BAND = ["nb", "det", "s", "sz", "r"] + ["p[%d]" % i for i in range(2)] + ["a[%d]" % i for i in range(2)] + ["b[%d]" % i for i in range(6)] \
    + ["d[%d]" % i for i in range(7)]


def fields(kind):
    """the order of the banks' state words (g722_dev.hpp: G2_*)"""
    io = "out" if kind == gl.ENCODE else "in"
    return (["packed", "eight_k", "bits_per_sample"] + ["x[%d]" % i for i in range(12)] + ["y[%d]" % i for i in range(12)] + ["ptr"]
            + ["band[%d].%s" % (b, f) for b in range(2) for f in BAND] + [io + "_buffer", io + "_bits"])


def build_reference(ref_src, d):
    so = os.path.join(d, "libg722_ref.so")
    subprocess.run(["gcc"] + STRICT + DEFS + ["-I" + ref_src, "-shared", "-o", so] + [os.path.join(ref_src, f) for f in ("g722.c", "vector_int.c", "alloc.c")]
                   + ["-lm"], check=True)
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>", "#include <stdbool.h>",
             '#include "spandsp/telephony.h"', '#include "spandsp/g722.h"', '#include "spandsp/private/g722.h"', "int main(void) {"]
    for kind, t in ((gl.ENCODE, "g722_encode_state_t"), (gl.DECODE, "g722_decode_state_t")):
        for f in fields(kind):
            lines.append('printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *) 0)->%s));' % (t, f, t, f))
    lines.append("return 0; }")
    src = os.path.join(d, "off.c")
    open(src, "w").write("\n".join(lines) + "\n")
    exe = os.path.join(d, "off")
    subprocess.run(["gcc", "-std=gnu99"] + DEFS + ["-I" + ref_src, src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    offsets = np.array([[int(x) for x in ln.split()] for ln in out.strip().splitlines()], np.int32).reshape(2, gl.WORDS, 2)
    L = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    for side in ("encode", "decode"):
        for name, res, args in [("init", vp, [vp, ci, ci]), ("free", ci, [vp]), ("release", ci, [vp]), ("", ci, [vp, vp, vp, ci])]:
            f = getattr(L, "g722_" + side + ("_" + name if name else ""))
            f.restype = res
            f.argtypes = args
    return L, offsets


class Ref:
    def __init__(self, L, offsets, kind, rate, options):
        self.L, self.kind, self.offs = L, kind, offsets[kind]
        self.side = "g722_encode" if kind == gl.ENCODE else "g722_decode"
        self.s = getattr(L, self.side + "_init")(None, rate, options)
        assert self.s

    def words(self):
        out = [int.from_bytes(C.string_at(self.s + int(off), int(size)), "little", signed=True) & 0xFFFFFFFF for off, size in self.offs]
        return np.array(out, np.uint32).view(np.int32)

    def run(self, data):
        if self.kind == gl.ENCODE:
            row = np.ascontiguousarray(data, np.int16)
            out = np.zeros(len(row) + 8, np.uint8)
            n = self.L.g722_encode(self.s, out.ctypes.data, row.ctypes.data, len(row))
        else:
            row = np.ascontiguousarray(data, np.uint8)
            out = np.zeros(4*len(row) + 16, np.int16)
            n = self.L.g722_decode(self.s, out.ctypes.data, row.ctypes.data, len(row))
        assert 0 <= n <= len(out)
        return out[:n].copy()

    def free(self):
        assert getattr(self.L, self.side + "_release")(self.s) == 0
        getattr(self.L, self.side + "_free")(self.s)


def by_calls(ref, data, schedule):
    """data through the codec on a schedule: the outputs back to back, the count and the state words of every call"""
    outs, counts, ws = [], [], []
    at = 0
    for n in gl.calls(len(data), schedule):
        o = ref.run(data[at:at + n])
        at += n
        outs.append(o)
        counts.append(len(o))
        ws.append(ref.words())
    w = np.array(ws, np.int32)
    assert np.array_equal(w.astype(np.int16).astype(np.int32), w), "a state word does not fit an int16"
    return np.concatenate(outs), np.array(counts, np.int32), w.astype(np.int16)


def streams(L, offsets, rate, eight_k, packed):
    opts = gl.options_of(eight_k, packed)
    S = {n: [] for n in ("codes", "ecounts", "ewords", "pcm", "dcounts", "dwords")}
    for line in gl.lines():
        r = Ref(L, offsets, gl.ENCODE, rate, opts)
        codes, counts, words = by_calls(r, line, gl.enc_schedule(eight_k))
        r.free()
        S["codes"].append(codes)
        S["ecounts"].append(counts)
        S["ewords"].append(words)
        r = Ref(L, offsets, gl.DECODE, rate, opts)
        pcm, counts, words = by_calls(r, codes, gl.DEC_SCHEDULE)
        r.free()
        S["pcm"].append(pcm)
        S["dcounts"].append(counts)
        S["dwords"].append(words)
    out = {n: np.array(v) for n, v in S.items()}
    noise = gl.random_bytes(rate, eight_k, packed)
    assert int(noise.max()) >> gl.bits_of(rate) or rate == 64000
    r = Ref(L, offsets, gl.DECODE, rate, opts)
    out["rnd"], out["rndcounts"], out["rndwords"] = by_calls(r, noise, gl.DEC_SCHEDULE)
    r.free()
    return out


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    with tempfile.TemporaryDirectory() as d:
        L, offsets = build_reference(ref_src, d)
        out = {"offsets": offsets, "enc_schedule_16k": np.array(gl.ENC_SCHEDULE_16K, np.int32), "enc_schedule_8k": np.array(gl.ENC_SCHEDULE_8K, np.int32),
               "dec_schedule": np.array(gl.DEC_SCHEDULE, np.int32), "line_crcs": gl.line_crcs()}
        init = []
        for rate, eight_k, packed in gl.CONFIGS:
            pair = []
            for kind in (gl.ENCODE, gl.DECODE):
                r = Ref(L, offsets, kind, rate, gl.options_of(eight_k, packed))
                pair.append(r.words())
                r.free()
            init.append(pair)
        out["init"] = np.array(init, np.int32)
        # the reference maps a rate it does not know to 8 bits
        r = Ref(L, offsets, gl.ENCODE, 8000, 0)
        assert r.words()[gl.W_BPS] == 8
        r.free()
        for rate, eight_k, packed in gl.CONFIGS:
            S = streams(L, offsets, rate, eight_k, packed)
            k = gl.key(*gl.stored(rate, eight_k, packed))
            if (rate, eight_k, packed) != gl.stored(rate, eight_k, packed):
                # (the noise of a configuration stored under another one is that one's)
                assert all(np.array_equal(S[n], out["%s_%s" % (n, k)]) for n in S if not n.startswith("rnd")), (rate, eight_k, packed)
                continue
            for n, v in S.items():
                out["%s_%s" % (n, k)] = v
            print(rate, eight_k, packed, "done:", S["codes"].shape[1], "bytes,", S["pcm"].shape[1], "samples")
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
    assert os.path.getsize(GOLDEN) <= 478071


if __name__ == "__main__":
    main()
