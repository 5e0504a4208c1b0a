"""Writes tests/golden/g726.npz from the live reference.  g726.c is not among the modules of oracle/_ref/libspandsp_ref.so,
so it is compiled here, in a temporary directory, with the flags of oracle/Makefile (STRICT + DEFS), linked against that
library (g711, bitstream, alloc), and nothing compiled is kept.  The fixture holds data only; the lines come from
tests/g726_lines.py.  Arrays are stacked per rate to keep the archive small: [coding] is 0 linear, 1 u-law, 2 A-law,
[line] is 0 ten segments, 1 gated 3900 Hz, 2 modulated 300 Hz, <p> is 1 (left) or 2 (right).

  offsets             [word][offset, size] of the g726_state_t fields the banks' state words map to, in that order, measured
                      by a compiler on the reference's private header;
  schedule            the call lengths cycled by every case: samples for the encoder, bytes for the decoder;
  line_crcs           CRC-32 of the three lines as generated;
  init                [rate] the state words g726_init() leaves (linear, unpacked);
  codes_<rate>        [coding][line][4000] the encoder's codes, unpacked, one per byte;
  words_<rate>        [coding][line][call][30] the state words after every call of that encoder -- and of the unpacked decoder
                      fed those codes on the same schedule, which the generator asserts are the same words;
  out_lin_<rate>      [line][4000] int16: what the decoder makes of the codes; out_law_<rate> [coding - 1][line][4000] G.711 bytes;
  packed<p>_<rate>    [coding][line][bytes] the same codes packed;
  pkmeta<p>_<rate>    [coding][line][call][bytes returned, bs.bitstream, bs.residue] of the packing encoder (its other words
                      are words_<rate>: packing does not touch them, asserted);
  upcounts<p>_<rate>  [coding][line][call] the samples each call of the unpacking decoder made of packed<p> (the samples are the
                      head of out_*: a stream may end on a code cut short);
  finals_<rate>       [p - 1][coding][line][0 encoder, 1 decoder][30] the packed codecs' words at the end;
  rnd_lin_<rate>      [1000] int16, rnd_law_<rate> [coding - 1][1000]: the unpacked decoder on g726_lines.random_bytes(), whose
                      bytes have bits set above the code width; rnd_words_<rate> [coding][call][30].

The generator steps the reference one sample at a time as well and asserts that the corners of update() the lines were
chosen for (both clamps of a[1], both limits of a[0], both limits of yu, the transition reset, both zero forms of dq[0]) appear.

Run from the repository root:  python tests/golden/make_golden_g726.py [reference source dir]"""
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

import g726_lines as gl  # noqa: E402

GOLDEN = os.path.join(HERE, "g726.npz")
STRICT = ["-std=gnu99", "-O2", "-ffp-contract=off", "-fPIC", "-fwrapv"]
DEFS = ["-DHAVE_MATH_H", "-DHAVE_STDBOOL_H", "-DHAVE_SINF", "-DHAVE_COSF", "-DHAVE_TANF", "-DHAVE_ASINF", "-DHAVE_ACOSF", "-DHAVE_ATANF",
        "-DHAVE_ATAN2F", "-DHAVE_CEILF", "-DHAVE_FLOORF", "-DHAVE_POWF", "-DHAVE_EXPF", "-DHAVE_LOGF", "-DHAVE_LOG10F", "-DHAVE_LRINT",
        "-DHAVE_LRINTF", "-DHAVE_LONG_DOUBLE", "-DHAVE_MALLOC_H", "-DHAVE_ALIGNED_ALLOC", "-DHAVE_UNISTD_H", "-DHAVE_STDLIB_H",
        "-DHAVE_STRING_H", "-DHAVE_INTTYPES_H", "-DHAVE_STDINT_H", "-DHAVE_TGMATH_H"]
# the order of the banks' state words (g726_dev.hpp: G7_*)
FIELDS = (["yl", "yu", "dms", "dml", "ap"] + ["a[%d]" % i for i in range(2)] + ["b[%d]" % i for i in range(6)]
          + ["pk[%d]" % i for i in range(2)] + ["dq[%d]" % i for i in range(6)] + ["sr[%d]" % i for i in range(2)]
          + ["td", "bs.bitstream", "bs.residue", "rate", "ext_coding", "bits_per_sample", "packing"])
HEADERS = ("telephony", "alloc", "bitstream", "g726", "private/bitstream", "private/g726")
W = {name: i for i, name in enumerate(FIELDS)}


def build_reference(ref_src, d):
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    so = os.path.join(d, "libg726_ref.so")
    subprocess.run(["gcc"] + STRICT + DEFS + ["-I" + os.path.join(ref_dir, "gen"), "-I" + ref_src, "-shared", "-o", so,
                    os.path.join(ref_src, "g726.c"), "-L" + ref_dir, "-lspandsp_ref", "-Wl,-rpath," + ref_dir, "-lm"], check=True)
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>",
             "#include <stdbool.h>"] + ['#include "spandsp/%s.h"' % h for h in HEADERS] + ["int main(void) {"]
    for f in FIELDS:
        lines.append('printf("%%zu %%zu\\n", offsetof(g726_state_t, %s), sizeof(((g726_state_t *) 0)->%s));' % (f, f))
    lines.append("return 0; }")
    src = os.path.join(d, "off.c")
    open(src, "w").write("\n".join(lines) + "\n")
    exe = os.path.join(d, "off")
    subprocess.run(["gcc", "-std=gnu99"] + DEFS + ["-I" + os.path.join(ref_dir, "gen"), "-I" + ref_src, src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    offsets = np.array([[int(x) for x in ln.split()] for ln in out.strip().splitlines()], np.int32)
    C.CDLL(os.path.join(ref_dir, "libspandsp_ref.so"), mode=C.RTLD_GLOBAL)
    L = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    for name, res, args in [("g726_init", vp, [vp, ci, ci, ci]), ("g726_free", ci, [vp]), ("g726_release", ci, [vp]),
                            ("g726_encode", ci, [vp, vp, vp, ci]), ("g726_decode", ci, [vp, vp, vp, ci])]:
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    return L, offsets


class Ref:
    def __init__(self, L, offsets, rate, coding, packing):
        self.L, self.offs, self.coding = L, offsets, coding
        self.s = L.g726_init(None, rate, coding, packing)
        assert self.s

    def words(self):
        # signed fields sign-extended, the bit stream as the 32 bits it is
        out = [int.from_bytes(C.string_at(self.s + int(off), int(size)), "little", signed=True) & 0xFFFFFFFF for off, size in self.offs]
        return np.array(out, np.uint32).view(np.int32)

    def encode(self, row):
        row = np.ascontiguousarray(row)
        out = np.zeros(len(row) + 8, np.uint8)
        n = self.L.g726_encode(self.s, out.ctypes.data, row.ctypes.data, len(row))
        return out[:n].copy()

    def decode(self, data):
        data = np.ascontiguousarray(data, np.uint8)
        out = np.zeros(4*len(data) + 8, gl.pcm_dtype(self.coding))
        n = self.L.g726_decode(self.s, out.ctypes.data, data.ctypes.data, len(data))
        return out[:n].copy()

    def free(self):
        self.L.g726_free(self.s)


def by_calls(fn, data, words):
    """data through fn on the fixture's schedule: the outputs back to back, the count and the state words of every call"""
    outs, counts, ws = [], [], []
    at = 0
    for n in gl.calls(len(data)):
        o = fn(data[at:at + n])
        at += n
        outs.append(o)
        counts.append(len(o))
        ws.append(words())
    return np.concatenate(outs), np.array(counts, np.int32), np.array(ws, np.int32)


class Seen:
    """the corners of update(), looked for on the reference's state after every single sample"""
    NAMES = ("a1_max", "a1_min", "a0_max", "a0_min", "yu_min", "yu_max", "transition", "dq_plus_zero", "dq_minus_zero")

    def __init__(self):
        self.where = {n: [] for n in self.NAMES}

    def note(self, name, tag):
        if tag not in self.where[name]:
            self.where[name].append(tag)

    def step_through(self, ref, feed, items, tag):
        td_before = 0
        for i in range(len(items)):
            feed(items[i:i + 1])
            w = ref.words()
            a0, a1 = int(w[W["a[0]"]]), int(w[W["a[1]"]])
            if a1 == 12288:
                self.note("a1_max", tag)
            if a1 == -12288:
                self.note("a1_min", tag)
            if a0 == 15360 - a1 and a0 != 0:
                self.note("a0_max", tag)
            if a0 == -(15360 - a1):
                self.note("a0_min", tag)
            if i > 0 and int(w[W["yu"]]) == 544:
                self.note("yu_min", tag)
            if int(w[W["yu"]]) == 5120:
                self.note("yu_max", tag)
            coeffs = [int(w[W["a[%d]" % k]]) for k in range(2)] + [int(w[W["b[%d]" % k]]) for k in range(6)]
            if td_before == 1 and int(w[W["ap"]]) == 256 and not any(coeffs):
                self.note("transition", tag)
            if int(w[W["dq[0]"]]) == 0x20:
                self.note("dq_plus_zero", tag)
            if int(w[W["dq[0]"]]) == 0xFC20 - 0x10000:
                self.note("dq_minus_zero", tag)
            td_before = int(w[W["td"]])


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    lines = gl.lines()
    seen = Seen()
    with tempfile.TemporaryDirectory() as d:
        L, offsets = build_reference(ref_src, d)
        assert L.g726_init(None, 8000, 0, 0) is None and L.g726_init(None, 48000, 0, 0) is None
        out = {"offsets": offsets, "schedule": np.array(gl.SCHEDULE, np.int32), "line_crcs": gl.line_crcs()}
        init = []
        for rate in gl.RATES:
            r = Ref(L, offsets, rate, gl.LINEAR, gl.PACK_NONE)
            init.append(r.words())
            assert L.g726_release(r.s) == 0
            r.free()
        out["init"] = np.array(init, np.int32)
        core = [i for i, f in enumerate(FIELDS) if f not in ("bs.bitstream", "bs.residue", "packing")]
        for rate in gl.RATES:
            S = {n: [] for n in ("codes", "words", "out", "packed1", "packed2", "pkmeta1", "pkmeta2", "upcounts1", "upcounts2",
                                 "fin1", "fin2", "rnd", "rnd_words")}
            for coding in gl.CODINGS:
                per = {n: [] for n in S}
                for li, line in enumerate(lines):
                    k = gl.key(rate, coding, li)
                    row = gl.pcm_row(line, coding)
                    r = Ref(L, offsets, rate, coding, gl.PACK_NONE)
                    codes, counts, words = by_calls(r.encode, row, r.words)
                    r.free()
                    assert len(codes) == len(row) and int(codes.max()) < (1 << (rate//8000))
                    r = Ref(L, offsets, rate, coding, gl.PACK_NONE)
                    pcm, counts, dwords = by_calls(r.decode, codes, r.words)
                    r.free()
                    assert len(pcm) == len(codes) and np.array_equal(dwords, words)
                    per["codes"].append(codes)
                    per["words"].append(words)
                    per["out"].append(pcm)
                    # the corners, one sample at a time
                    r = Ref(L, offsets, rate, coding, gl.PACK_NONE)
                    seen.step_through(r, r.encode, row, k)
                    assert np.array_equal(r.words(), words[-1])
                    r.free()
                    for p in (gl.PACK_LEFT, gl.PACK_RIGHT):
                        r = Ref(L, offsets, rate, coding, p)
                        packed, counts, pwords = by_calls(r.encode, row, r.words)
                        r.free()
                        assert np.array_equal(pwords[:, core], words[:, core])
                        per["packed%d" % p].append(packed)
                        per["pkmeta%d" % p].append(np.column_stack([counts, pwords[:, W["bs.bitstream"]], pwords[:, W["bs.residue"]]]))
                        r = Ref(L, offsets, rate, coding, p)
                        pcm2, counts2, uwords = by_calls(r.decode, packed, r.words)
                        r.free()
                        # (a packed stream may end on a code cut short: the decoder gives what is whole)
                        assert np.array_equal(pcm2, pcm[:len(pcm2)]) and len(pcm) - len(pcm2) < 8
                        per["upcounts%d" % p].append(counts2)
                        per["fin%d" % p].append(np.array([pwords[-1], uwords[-1]], np.int32))
                # the random-code line, the decoder alone
                noise = gl.random_bytes(rate, coding)
                assert int(noise.max()) >= (1 << (rate//8000))
                r = Ref(L, offsets, rate, coding, gl.PACK_NONE)
                pcm, counts, dwords = by_calls(r.decode, noise, r.words)
                r.free()
                S["rnd"].append(pcm)
                S["rnd_words"].append(dwords)
                r = Ref(L, offsets, rate, coding, gl.PACK_NONE)
                seen.step_through(r, r.decode, noise, gl.key(rate, coding, "rnd"))
                r.free()
                for n in per:
                    if per[n]:
                        S[n].append(np.array(per[n]))
                print(rate, coding, "done")
            for n in ("codes", "words", "packed1", "packed2", "pkmeta1", "pkmeta2", "upcounts1", "upcounts2", "rnd_words"):
                out["%s_%d" % (n, rate)] = np.array(S[n])
            out["out_lin_%d" % rate] = S["out"][0]
            out["out_law_%d" % rate] = np.array(S["out"][1:])
            out["rnd_lin_%d" % rate] = S["rnd"][0]
            out["rnd_law_%d" % rate] = np.array(S["rnd"][1:])
            out["finals_%d" % rate] = np.array([S["fin1"], S["fin2"]], np.int32)
    for name in Seen.NAMES:
        print("%-14s %3d cases, first %s" % (name, len(seen.where[name]), seen.where[name][:3]))
    missing = [n for n in Seen.NAMES if not seen.where[n]]
    assert not missing, "no line shows %s: lengthen or reseed a line in tests/g726_lines.py" % missing
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
    assert os.path.getsize(GOLDEN) <= 478071


if __name__ == "__main__":
    main()
