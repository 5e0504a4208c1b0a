"""Writes tests/golden/plc.npz from the live reference.  The packet loss concealer is not among the modules of
oracle/_ref/libspandsp_ref.so, so plc.c, vector_int.c and alloc.c are compiled here, in a temporary directory, with the strict
flags of oracle/Makefile, and nothing compiled is kept.  The fixture holds data only; the lines and the schedules come from
tests/plc_lines.py, the decoded lines from tests/golden/gsm0610.npz.  <g> is "sched" (the nine lines under SCHEDULE), "heard"
(one line under the same lengths with nothing lost) or "dec" (the five decoded lines under DEC_TICKS).

  offsets             [word][offset, size] of the state fields the banks' state words map to, in that order, measured by a
                      compiler on the reference's private header;
  schedule, dec_ticks the calls, as plc_lines has them;
  line_crcs           CRC-32 of the nine lines as generated;
  <g>_out             [line][samples] the rows after each call, one behind the other;
  <g>_scal            [line][call][4] missing_samples, pitch_offset, pitch, buf_ptr after each call;
  <g>_pb              [line][call][120] pitchbuf as bit patterns; <g>_hist [line][call][280] the history ring as it lies.

Run from the repository root:  python tests/golden/make_golden_plc.py [reference source dir]"""
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

import plc_lines as pl  # noqa: E402

GOLDEN = os.path.join(HERE, "plc.npz")
STRICT = ["-std=gnu99", "-O2", "-ffp-contract=off", "-fPIC", "-fwrapv"]
DEFS = ["-DHAVE_MATH_H", "-DHAVE_STDBOOL_H", "-DHAVE_SINF", "-DHAVE_COSF", "-DHAVE_TANF", "-DHAVE_ASINF", "-DHAVE_ACOSF", "-DHAVE_ATANF",
        "-DHAVE_ATAN2F", "-DHAVE_CEILF", "-DHAVE_FLOORF", "-DHAVE_POWF", "-DHAVE_EXPF", "-DHAVE_LOGF", "-DHAVE_LOG10F", "-DHAVE_LRINT",
        "-DHAVE_LRINTF", "-DHAVE_LONG_DOUBLE", "-DHAVE_MALLOC_H", "-DHAVE_ALIGNED_ALLOC", "-DHAVE_UNISTD_H", "-DHAVE_STDLIB_H",
        "-DHAVE_STRING_H", "-DHAVE_INTTYPES_H", "-DHAVE_STDINT_H", "-DHAVE_TGMATH_H"]
SOURCES = ["plc.c", "vector_int.c", "alloc.c"]
FIELDS = (["missing_samples", "pitch_offset", "pitch"] + ["pitchbuf[%d]" % i for i in range(120)] + ["history[%d]" % i for i in range(280)]
          + ["buf_ptr"])


def build_reference(ref_src, d):
    so = os.path.join(d, "libplc_ref.so")
    subprocess.run(["gcc"] + STRICT + DEFS + ["-I" + ref_src, "-shared", "-o", so] + [os.path.join(ref_src, f) for f in SOURCES] + ["-lm"], check=True)
    text = ["#include <stdio.h>", "#include <stddef.h>", "#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>", "#include <stdbool.h>",
            '#include "spandsp/telephony.h"', '#include "spandsp/plc.h"', '#include "spandsp/private/plc.h"', "int main(void) {"]
    for f in FIELDS:
        text.append('printf("%%zu %%zu\\n", offsetof(plc_state_t, %s), sizeof(((plc_state_t *) 0)->%s));' % (f, f))
    text.append("return 0; }")
    src = os.path.join(d, "off.c")
    open(src, "w").write("\n".join(text) + "\n")
    exe = os.path.join(d, "off")
    subprocess.run(["gcc", "-std=gnu99"] + DEFS + ["-I" + ref_src, src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    offsets = np.array([[int(x) for x in ln.split()] for ln in out.strip().splitlines()], np.int32).reshape(pl.WORDS, 2)
    L = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    for name, res, args in [("init", vp, [vp]), ("free", ci, [vp]), ("release", ci, [vp]), ("rx", ci, [vp, vp, ci]), ("fillin", ci, [vp, vp, ci])]:
        f = getattr(L, "plc_" + name)
        f.restype = res
        f.argtypes = args
    return L, offsets


class Ref:
    def __init__(self, L, offsets):
        self.L, self.offs = L, offsets
        self.s = L.plc_init(None)
        assert self.s

    def words(self):
        # (a float's bit pattern and a sign-extended int16_t alike: the field's bytes as a signed integer)
        out = [int.from_bytes(C.string_at(self.s + int(off), int(size)), "little", signed=True) & 0xFFFFFFFF for off, size in self.offs]
        return np.array(out, np.uint32).view(np.int32)

    def call(self, lost, row):
        row = np.ascontiguousarray(row, np.int16).copy()
        n = (self.L.plc_fillin if lost else self.L.plc_rx)(self.s, row.ctypes.data, len(row))
        assert n == len(row)
        return row

    def free(self):
        assert self.L.plc_release(self.s) == 0
        self.L.plc_free(self.s)


def run_group(L, offsets, schedule, ins):
    G = {n: [] for n in ("out", "scal", "pb", "hist")}
    for rows in ins:
        r = Ref(L, offsets)
        assert not r.words().any()
        outs, scal, pb, hist = [], [], [], []
        for (lost, n), row in zip(schedule, rows):
            assert len(row) == n
            outs.append(r.call(lost, row))
            a, b, c = pl.split_words(r.words())
            scal.append(a)
            pb.append(b)
            hist.append(c)
        r.free()
        G["out"].append(np.concatenate(outs))
        G["scal"].append(scal)
        G["pb"].append(pb)
        G["hist"].append(hist)
    return {"out": np.array(G["out"], np.int16), "scal": np.array(G["scal"], np.int32), "pb": np.array(G["pb"], np.int32),
            "hist": np.array(G["hist"], np.int16)}


def generate(ref_src):
    """the fixture's arrays from a fresh build of the reference"""
    with tempfile.TemporaryDirectory() as d:
        L, offsets = build_reference(ref_src, d)
        out = {"offsets": offsets, "schedule": np.array(pl.SCHEDULE, np.int32), "dec_ticks": np.array(pl.DEC_TICKS, np.int32),
               "line_crcs": pl.line_crcs()}
        the_lines = pl.lines()
        pcm, _ = pl.load_gsm_pcm()
        groups = (("sched", pl.SCHEDULE, [pl.rows_in(x, pl.SCHEDULE) for x in the_lines]),
                  ("heard", pl.HEARD_ONLY, [pl.rows_in(the_lines[pl.HEARD_LINE], pl.HEARD_ONLY)]),
                  ("dec", pl.dec_schedule(), [pl.dec_rows_in(pcm[i]) for i in range(pl.DEC_LINES)]))
        for key, schedule, ins in groups:
            for n, v in run_group(L, offsets, schedule, ins).items():
                out["%s_%s" % (key, n)] = v
    return out


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    out = generate(ref_src)
    c = pl.coverage(pl.sched_cases(out))
    print("coverage: pitches %s, ties %s, buf_ptr at the end %s" % (sorted(c["pitches"]), sorted(set(c["ties"])), sorted(c["buf_ptr_end"])))
    pl.check_coverage(c)
    assert not pl.heard_case(out).calls[-1][4][pl.W_MISSING] and all(k[4][pl.W_PITCH] == 0 for k in pl.heard_case(out).calls)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
    assert os.path.getsize(GOLDEN) <= pl.MAX_FIXTURE_BYTES


if __name__ == "__main__":
    main()
