"""Writes tests/golden/gsm0610.npz from the live reference.  The GSM 06.10 codec is not among the modules of
oracle/_ref/libspandsp_ref.so, so gsm0610_*.c and alloc.c are compiled here, in a temporary directory, with the strict flags
of oracle/Makefile (the plain C paths: no MMX), and nothing compiled is kept.  The fixture holds data only; the lines come
from tests/gsm0610_lines.py.  <k> is "none", "wav49" or "voip".

  offsets             [word][offset, size] of the state fields the banks' state words map to, in that order, measured by a
                      compiler on the reference's private header;
  schedule, schedule_wav49
                      the frames a call, cycled by every case;
  line_crcs           CRC-32 of the five lines as generated;
  init                [packing][160] the state words gsm0610_init() leaves;
  codes_<k>           [line][bytes] what the encoder makes of the line;
  ecounts_<k>         [line][call] the bytes each call returned; ewords_<k> [line][call][160] the state words after it;
  pcm_<k>             [line][samples] what the decoder makes of codes_<k>; dcounts_<k>, dwords_<k> as above;
  rnd_<k>, rndcounts_<k>, rndwords_<k>
                      the decoder on gsm0610_lines.random_codes().

Run from the repository root:  python tests/golden/make_golden_gsm0610.py [reference source dir]"""
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

import gsm0610_lines as gl  # noqa: E402

GOLDEN = os.path.join(HERE, "gsm0610.npz")
STRICT = ["-std=gnu99", "-O2", "-ffp-contract=off", "-fPIC", "-fwrapv"]
DEFS = ["-DHAVE_MATH_H", "-DHAVE_STDBOOL_H", "-DHAVE_SINF", "-DHAVE_COSF", "-DHAVE_TANF", "-DHAVE_ASINF", "-DHAVE_ACOSF", "-DHAVE_ATANF",
        "-DHAVE_ATAN2F", "-DHAVE_CEILF", "-DHAVE_FLOORF", "-DHAVE_POWF", "-DHAVE_EXPF", "-DHAVE_LOGF", "-DHAVE_LOG10F", "-DHAVE_LRINT",
        "-DHAVE_LRINTF", "-DHAVE_LONG_DOUBLE", "-DHAVE_MALLOC_H", "-DHAVE_ALIGNED_ALLOC", "-DHAVE_UNISTD_H", "-DHAVE_STDLIB_H",
        "-DHAVE_STRING_H", "-DHAVE_INTTYPES_H", "-DHAVE_STDINT_H", "-DHAVE_TGMATH_H"]
SOURCES = ["gsm0610_%s.c" % n for n in ("encode", "decode", "lpc", "long_term", "preprocess", "rpe", "short_term")] + ["alloc.c"]
FIELDS = (["packing"] + ["dp0[%d]" % i for i in range(120)] + ["z1", "L_z2", "mp"] + ["u[%d]" % i for i in range(8)]
          + ["LARpp[%d][%d]" % (a, i) for a in range(2) for i in range(8)] + ["j", "nrp"] + ["v[%d]" % i for i in range(9)] + ["msr"])


def build_reference(ref_src, d):
    so = os.path.join(d, "libgsm0610_ref.so")
    subprocess.run(["gcc"] + STRICT + DEFS + ["-I" + ref_src, "-shared", "-o", so] + [os.path.join(ref_src, f) for f in SOURCES] + ["-lm"], check=True)
    text = ["#include <stdio.h>", "#include <stddef.h>", "#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>", "#include <stdbool.h>",
            '#include "spandsp/telephony.h"', '#include "spandsp/gsm0610.h"', '#include "spandsp/private/gsm0610.h"', "int main(void) {"]
    for f in FIELDS:
        text.append('printf("%%zu %%zu\\n", offsetof(gsm0610_state_t, %s), sizeof(((gsm0610_state_t *) 0)->%s));' % (f, f))
    text.append("return 0; }")
    src = os.path.join(d, "off.c")
    open(src, "w").write("\n".join(text) + "\n")
    exe = os.path.join(d, "off")
    subprocess.run(["gcc", "-std=gnu99"] + DEFS + ["-I" + ref_src, src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    offsets = np.array([[int(x) for x in ln.split()] for ln in out.strip().splitlines()], np.int32).reshape(gl.WORDS, 2)
    L = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    for name, res, args in [("init", vp, [vp, ci]), ("free", ci, [vp]), ("release", ci, [vp]), ("encode", ci, [vp, vp, vp, ci]),
                            ("decode", ci, [vp, vp, vp, ci])]:
        f = getattr(L, "gsm0610_" + name)
        f.restype = res
        f.argtypes = args
    return L, offsets


class Ref:
    def __init__(self, L, offsets, kind, packing):
        self.L, self.kind, self.offs = L, kind, offsets
        self.s = L.gsm0610_init(None, packing)
        assert self.s

    def words(self):
        out = [int.from_bytes(C.string_at(self.s + int(off), int(size)), "little", signed=True) & 0xFFFFFFFF for off, size in self.offs]
        return np.array(out, np.uint32).view(np.int32)

    def run(self, data):
        if self.kind == gl.ENCODE:
            row = np.ascontiguousarray(data, np.int16)
            out = np.zeros(len(row) + 80, np.uint8)
            n = self.L.gsm0610_encode(self.s, out.ctypes.data, row.ctypes.data, len(row))
        else:
            row = np.ascontiguousarray(data, np.uint8)
            out = np.zeros(10*len(row) + 320, np.int16)
            n = self.L.gsm0610_decode(self.s, out.ctypes.data, row.ctypes.data, len(row))
        assert 0 <= n <= len(out)
        return out[:n].copy()

    def free(self):
        assert self.L.gsm0610_release(self.s) == 0
        self.L.gsm0610_free(self.s)


def by_calls(ref, data, lens):
    outs, counts, ws = [], [], []
    at = 0
    for n in lens:
        o = ref.run(data[at:at + n])
        at += n
        outs.append(o)
        counts.append(len(o))
        ws.append(ref.words())
    assert at == len(data)
    return np.concatenate(outs), np.array(counts, np.int32), np.array(ws, np.int32)


def streams(L, offsets, packing):
    frames = gl.calls(gl.N_FRAMES, packing)
    elens = [f*gl.FRAME for f in frames]
    dlens = [f*gl.unit_bytes(packing)//(2 if packing == gl.WAV49 else 1) for f in frames]
    S = {n: [] for n in ("codes", "ecounts", "ewords", "pcm", "dcounts", "dwords")}
    for line in gl.lines():
        r = Ref(L, offsets, gl.ENCODE, packing)
        codes, counts, words = by_calls(r, line, elens)
        r.free()
        S["codes"].append(codes)
        S["ecounts"].append(counts)
        S["ewords"].append(words)
        r = Ref(L, offsets, gl.DECODE, packing)
        pcm, counts, words = by_calls(r, codes, dlens)
        r.free()
        S["pcm"].append(pcm)
        S["dcounts"].append(counts)
        S["dwords"].append(words)
    out = {n: np.array(v) for n, v in S.items()}
    r = Ref(L, offsets, gl.DECODE, packing)
    out["rnd"], out["rndcounts"], out["rndwords"] = by_calls(r, gl.random_codes(packing), dlens)
    r.free()
    return out


def check_coverage(g):
    c = gl.coverage(g)
    assert c["bc"] == {0, 1, 2, 3} and c["Mc"] == {0, 1, 2, 3}, c
    assert {40, 120} <= c["Nc"] and {0, 63} <= c["xmaxc"] and c["xMc"] == set(range(8)), c
    assert c["zero_frame"] and c["rnd_lags_out"] >= 1, c
    return c


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    with tempfile.TemporaryDirectory() as d:
        L, offsets = build_reference(ref_src, d)
        out = {"offsets": offsets, "schedule": np.array(gl.SCHEDULE, np.int32), "schedule_wav49": np.array(gl.SCHEDULE_WAV49, np.int32),
               "line_crcs": gl.line_crcs()}
        init = []
        for p in gl.PACKINGS:
            r = Ref(L, offsets, gl.ENCODE, p)
            init.append(r.words())
            r.free()
        out["init"] = np.array(init, np.int32)
        for p in gl.PACKINGS:
            for n, v in streams(L, offsets, p).items():
                out["%s_%s" % (n, gl.key(p))] = v
            print(gl.key(p), "done:", out["codes_" + gl.key(p)].shape[1], "bytes,", out["pcm_" + gl.key(p)].shape[1], "samples")
    # the three packings carry the same parameters
    for li in range(5):
        assert np.array_equal(gl.pack_voip_stream(out["codes_none"][li]), out["codes_voip"][li])
        assert np.array_equal(gl.pack_wav49_stream(out["codes_none"][li]), out["codes_wav49"][li])
    c = check_coverage(out)
    print("coverage: Nc %d values, xmaxc %d values, %d lags out of range in the random VoIP frames" % (len(c["Nc"]), len(c["xmaxc"]), c["rnd_lags_out"]))
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
    assert os.path.getsize(GOLDEN) < 335200


if __name__ == "__main__":
    main()
