"""The lines of the IMA and OKI ADPCM fixtures (tests/golden/ima_adpcm.npz, oki_adpcm.npz), the configurations the tests
share, generated lines for the sweeps, and the one place that builds and drives the live reference (the fixture generator
and the CPU sweep both use it).  Deterministic: numpy's sine and a 32-bit linear congruential generator, nothing else.

A case is one codec: family, direction, configuration, the input items, the output items, and per call (length, count, the
state words after it).  Decoders of a configuration whose calls are packets (IMA with chunk_size == 0: a header per call;
VDVI: bits reset and padded per call) are fed the encoder's calls one for one; every other stream is cut on SCHEDULE, and
may be cut any other way (Case.recut).
"""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np

from g726_lines import Lcg

IMA, OKI = 0, 1
ENCODE, DECODE = 0, 1
IMA4, DVI4, VDVI = 0, 1, 2
CHUNK = 64                      # the non-zero chunk size of the fixtures: only its being non-zero matters
IMA_CONFIGS = tuple((v, k) for v in (IMA4, DVI4, VDVI) for k in (0, CHUNK))
OKI_CONFIGS = ((32000, 0), (24000, 0))
CONFIGS = {IMA: IMA_CONFIGS, OKI: OKI_CONFIGS}
NAMES = {IMA: "ima_adpcm", OKI: "oki_adpcm"}
SCHEDULE = (1, 2, 3, 7, 15, 16, 17, 33, 160, 161)
IMA_FIELDS = ["variant", "chunk_size", "last", "step_index", "ima_byte", "bits"]
OKI_FIELDS = ["bit_rate", "last", "step_index", "oki_byte"] + ["history[%d]" % i for i in range(32)] + ["ptr", "mark", "phase"]
FIELDS = {IMA: IMA_FIELDS, OKI: OKI_FIELDS}
UNSIGNED = {"ima_byte", "oki_byte"}
WORDS = {IMA: len(IMA_FIELDS), OKI: len(OKI_FIELDS)}
W_IMA = {n: i for i, n in enumerate(IMA_FIELDS)}
W_OKI = {n: i for i, n in enumerate(OKI_FIELDS)}
VDVI_BITS = (2, 3, 4, 5, 6, 7, 8, 8)
STRICT = ["-std=gnu99", "-O2", "-ffp-contract=off", "-fPIC", "-fwrapv"]
DEFS = ["-DHAVE_MATH_H", "-DHAVE_STDBOOL_H", "-DHAVE_SINF", "-DHAVE_COSF", "-DHAVE_TANF", "-DHAVE_ASINF", "-DHAVE_ACOSF", "-DHAVE_ATANF",
        "-DHAVE_ATAN2F", "-DHAVE_CEILF", "-DHAVE_FLOORF", "-DHAVE_POWF", "-DHAVE_EXPF", "-DHAVE_LOGF", "-DHAVE_LOG10F", "-DHAVE_LRINT",
        "-DHAVE_LRINTF", "-DHAVE_LONG_DOUBLE", "-DHAVE_MALLOC_H", "-DHAVE_ALIGNED_ALLOC", "-DHAVE_UNISTD_H", "-DHAVE_STDLIB_H",
        "-DHAVE_STRING_H", "-DHAVE_INTTYPES_H", "-DHAVE_STDINT_H", "-DHAVE_TGMATH_H"]

# cutoff_coeffs[] of the reference's rate converter, as decimal text: the restatement of its sums below is this module's own
_HALF = """-3.648392e-4 5.062391e-4 1.206247e-3 1.804452e-3 1.691750e-3 4.083405e-4 -1.931085e-3 -4.452107e-3 -5.794821e-3 -4.778489e-3
-1.161266e-3 3.928504e-3 8.259786e-3 9.500425e-3 6.512800e-3 2.227856e-4 -6.531275e-3 -1.026843e-2 -8.718062e-3 -2.280487e-3 5.817733e-3
1.096777e-2 9.634404e-3 1.569301e-3 -9.522632e-3 -1.748273e-2 -1.684408e-2 -6.100054e-3 1.071206e-2 2.525209e-2 2.871779e-2 1.664411e-2
-7.706268e-3 -3.331083e-2 -4.521249e-2 -3.085962e-2 1.373653e-2 8.089593e-2 1.529060e-1 2.080487e-1 2.286834e-1"""
_half = [np.float32(x) for x in _HALF.split()]
COEFFS = np.array(_half + _half[-2::-1], np.float32)
assert len(COEFFS) == 81


def calls(total, schedule=SCHEDULE):
    """the call lengths that take `total` items on a schedule, cycled; the last one is what is left"""
    out, k = [], 0
    while total > 0:
        n = min(schedule[k % len(schedule)], total)
        out.append(n)
        total -= n
        k += 1
    return out


def _tone(freq, amp, n):
    t = np.arange(n, dtype=np.float64)
    return amp*np.sin(2.0*np.pi*freq*t/8000.0)


def _to_int16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def line():
    """the encoders' line: silence (step_index to 0), full-scale squares (to the top, both rails), full-scale noise and signs
    (the 24 kbit/s encoder's sum outside int16), tones, quiet noise"""
    rng = Lcg(0xADC3)
    k = np.arange(300)
    segs = [np.zeros(200),
            np.where((k % 6) < 3, 32767.0, -32768.0),
            rng.int16(300).astype(np.float64),
            np.where(rng.int16(300) < 0, -32768.0, 32767.0),
            _tone(697, 8000.0, 300) + _tone(1209, 8000.0, 300),
            np.where((k % 40) < 20, 32767.0, -32768.0),
            rng.int16(200)/64.0,
            np.zeros(120),
            _tone(2100, 20000.0, 200)]
    return _to_int16(np.concatenate(segs))


def random_bytes(family, a, b, n=1200):
    return Lcg(0xC0DE + 7*family + (a + 3*b if family == IMA else 0)).bytes(n)


def is_packets(family, a, b):
    return family == IMA and (b == 0 or a == VDVI)


def random_packets(family, a, b):
    """the random-code line of a decoder: (bytes, call lengths).  Under a header every call is 4 bytes longer than the schedule's
    and begins with one whose step_index is in the table."""
    noise = random_bytes(family, a, b)
    if not (family == IMA and b == 0):
        return noise, calls(len(noise))
    out, lens, at, k = [], [], 0, 0
    while at + 4 < len(noise):
        n = min(SCHEDULE[k % len(SCHEDULE)], len(noise) - at - 4)
        head = noise[at:at + 4].copy()
        head[2] = head[2] % 89
        out.append(np.concatenate([head, noise[at + 4:at + 4 + n]]))
        lens.append(4 + n)
        at += 4 + n
        k += 1
    return np.concatenate(out), lens


# ---- the live reference --------------------------------------------------------------------------------------------------

def build_reference(ref_src, d):
    """ima_adpcm.c, oki_adpcm.c and alloc.c of the reference compiled into directory d with STRICT + DEFS of oracle/Makefile;
    returns (library, {family: offsets [word][offset, size]}), the offsets measured by a compiler on the private headers"""
    so = os.path.join(d, "libadpcm_ref.so")
    subprocess.run(["gcc"] + STRICT + DEFS + ["-I" + ref_src, "-shared", "-o", so] + [os.path.join(ref_src, f) for f in ("ima_adpcm.c", "oki_adpcm.c", "alloc.c")]
                   + ["-lm"], check=True)
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>", "#include <stdbool.h>"]
    lines += ['#include "spandsp/%s.h"' % h for h in ("telephony", "ima_adpcm", "oki_adpcm", "private/ima_adpcm", "private/oki_adpcm")]
    lines.append("int main(void) {")
    for family in (IMA, OKI):
        t = NAMES[family] + "_state_t"
        for f in FIELDS[family]:
            lines.append('printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *) 0)->%s));' % (t, f, t, f))
    lines.append("return 0; }")
    src = os.path.join(d, "off.c")
    open(src, "w").write("\n".join(lines) + "\n")
    exe = os.path.join(d, "off")
    subprocess.run(["gcc", "-std=gnu99"] + DEFS + ["-I" + ref_src, src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    offs = np.array([[int(x) for x in ln.split()] for ln in out.strip().splitlines()], np.int32)
    L = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    for fam, init_args in (("ima_adpcm", [vp, ci, ci]), ("oki_adpcm", [vp, ci])):
        for name, res, args in [("init", vp, init_args), ("free", ci, [vp]), ("release", ci, [vp]), ("encode", ci, [vp, vp, vp, ci]),
                                ("decode", ci, [vp, vp, vp, ci])]:
            f = getattr(L, "%s_%s" % (fam, name))
            f.restype = res
            f.argtypes = args
    return L, {IMA: offs[:WORDS[IMA]], OKI: offs[WORDS[IMA]:]}


class Ref:
    """one object of the reference"""

    def __init__(self, L, offsets, family, a, b=0):
        self.L, self.family, self.offs = L, family, offsets[family]
        self.pre = NAMES[family]
        self.s = L.ima_adpcm_init(None, a, b) if family == IMA else L.oki_adpcm_init(None, a)
        assert self.s

    def words(self):
        out = []
        for name, (off, size) in zip(FIELDS[self.family], self.offs):
            out.append(int.from_bytes(C.string_at(self.s + int(off), int(size)), "little", signed=name not in UNSIGNED) & 0xFFFFFFFF)
        return np.array(out, np.uint32).view(np.int32)

    def encode(self, amp):
        amp = np.ascontiguousarray(amp, np.int16)
        out = np.zeros(len(amp) + 16, np.uint8)
        n = getattr(self.L, self.pre + "_encode")(self.s, out.ctypes.data, amp.ctypes.data, len(amp))
        return out[:n].copy()

    def decode(self, data):
        data = np.ascontiguousarray(data, np.uint8)
        out = np.zeros(4*len(data) + 16, np.int16)
        n = getattr(self.L, self.pre + "_decode")(self.s, out.ctypes.data, data.ctypes.data, len(data))
        return out[:n].copy()

    def free(self):
        getattr(self.L, self.pre + "_free")(self.s)


class Case:
    def __init__(self, family, kind, a, b, tag, data, want, calls, recut, entry_phase=0):
        self.family, self.kind, self.a, self.b, self.tag = family, kind, a, b, tag
        self.data, self.want, self.calls, self.recut = data, want, calls, recut
        self.entry_phase = entry_phase          # OKI: `phase` before the first call, where it is not init's 0

    @property
    def name(self):
        return "%s_%s_%d_%d_%s" % (NAMES[self.family], "dec" if self.kind else "enc", self.a, self.b, self.tag)


def run_reference(L, offsets, family, kind, a, b, tag, data, lens, recut, entry_phase=0):
    """the case the reference makes of `data` cut into calls of `lens`"""
    r = Ref(L, offsets, family, a, b)
    if entry_phase:
        C.memmove(r.s + int(r.offs[W_OKI["phase"]][0]), C.byref(C.c_int(entry_phase)), 4)
    fn = r.decode if kind else r.encode
    outs, cs, at = [], [], 0
    for n in lens:
        o = fn(data[at:at + n])
        at += n
        outs.append(o)
        cs.append((n, len(o), r.words()))
    r.free()
    want = np.concatenate(outs) if outs else np.zeros(0, np.int16 if kind else np.uint8)
    return Case(family, kind, a, b, tag, np.asarray(data), want, cs, recut, entry_phase)


def reference_cases(L, offsets, family, a, b, amp, tag, lens=None):
    """an encoder on `amp` and the decoder of what it makes"""
    lens = lens or calls(len(amp))
    packets = is_packets(family, a, b)
    enc = run_reference(L, offsets, family, ENCODE, a, b, tag, amp, lens, not packets)
    dlens = [c[1] for c in enc.calls if c[1] > 0] if packets else calls(len(enc.want))
    dec = run_reference(L, offsets, family, DECODE, a, b, tag, enc.want, dlens, not packets)
    return enc, dec


# ---- the fixtures as cases -----------------------------------------------------------------------------------------------

TAGS = ["line", "rnd", "phase1"]


def load(family, path=None):
    return np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", NAMES[family] + ".npz"))


def store(the_cases):
    """the arrays of a fixture: the encoders' line once, then per case its input (decoders), output and calls"""
    out = {"line": line(), "line_crc": np.array([zlib.crc32(line().tobytes())], np.uint32), "schedule": np.array(SCHEDULE, np.int32)}
    index = []
    for i, c in enumerate(the_cases):
        index.append([c.family, c.kind, c.a, c.b, TAGS.index(c.tag), 1 if c.recut else 0, c.entry_phase])
        if c.kind == DECODE:
            out["data%d" % i] = np.asarray(c.data, np.uint8)
        out["want%d" % i] = np.asarray(c.want)
        out["calls%d" % i] = np.array([[n, cnt] + list(w) for n, cnt, w in c.calls], np.int32)
    out["index"] = np.array(index, np.int32)
    return out


def cases(g):
    assert int(g["line_crc"][0]) == zlib.crc32(line().tobytes()), "the line generated here is not the fixture's"
    out = []
    for i, (family, kind, a, b, tag, recut, entry) in enumerate(g["index"].tolist()):
        data = g["data%d" % i] if kind == DECODE else line()
        cs = [(int(r[0]), int(r[1]), r[2:].copy()) for r in g["calls%d" % i]]
        out.append(Case(family, kind, a, b, TAGS[tag], data, g["want%d" % i], cs, bool(recut), entry))
    return out


def dump_text(path, the_cases):
    """the cases as the stand-alone host program reads them (tests/c_callers/adpcm_host.cpp)"""
    with open(path, "w") as f:
        for c in the_cases:
            f.write("C %d %d %d %d %d %d %d %d %d\n" % (c.family, c.kind, c.a, c.b, 1 if c.recut else 0, c.entry_phase, len(c.data), len(c.want),
                                                      len(c.calls)))
            f.write(" ".join(map(str, np.asarray(c.data).astype(np.int64).tolist())) + "\n")
            f.write(" ".join(map(str, np.asarray(c.want).astype(np.int64).tolist())) + "\n")
            for n, count, w in c.calls:
                f.write("%d %d %s\n" % (n, count, " ".join(map(str, np.asarray(w).astype(np.int64).tolist()))))
        f.write("E\n")
    return len(the_cases)


# ---- what the fixtures have to reach ---------------------------------------------------------------------------------------

def narrow(v):
    """(int16_t) of a binary32 value as the reference's x86-64 build does it: to int32 toward zero, then the low 16 bits"""
    t = int(v)
    return ((t + 0x8000) & 0xFFFF) - 0x8000


def oki24_decoder_sums(hist6k, entry_phase=0):
    """this module's restatement of the 24 kbit/s decoder's sums, in binary32 and the reference's tap order: the 6 kHz samples
    (what a 32 kbit/s decoder makes of the same nibbles) in, z*4.0f of every 8 kHz sample out.  The call ends with the last nibble."""
    h = [np.float32(0)]*32
    ptr, phase, out, k = 0, entry_phase, [], 0
    four = np.float32(4.0)
    while k < len(hist6k):
        if phase:
            h[ptr] = np.float32(int(hist6k[k]))
            ptr = (ptr + 1) & 31
            k += 1
        z = np.float32(0.0)
        x = ptr - 1
        for l in range(77 + phase, -1, -4):
            z = np.float32(z + np.float32(COEFFS[l]*h[x & 31]))
            x -= 1
        out.append(np.float32(z*four))
        phase = (phase + 1) & 3
    return out


def oki24_encoder_sums(amp):
    """... and the encoder's: z*3.0f of every sample that is coded, from a fresh state"""
    h = [np.float32(0)]*32
    ptr, phase, out, n = 0, 0, [], 0
    three = np.float32(3.0)
    while n < len(amp):
        if phase > 2:
            h[ptr] = np.float32(int(amp[n]))
            ptr = (ptr + 1) & 31
            phase = 0
            n += 1
            if n >= len(amp):
                break
        h[ptr] = np.float32(int(amp[n]))
        ptr = (ptr + 1) & 31
        z = np.float32(0.0)
        x = ptr - 1
        for l in range(80 - phase, -1, -3):
            z = np.float32(z + np.float32(COEFFS[l]*h[x & 31]))
            x -= 1
        out.append(np.float32(z*three))
        phase += 1
        n += 1
    return out


def _nibbles(data, low_first=False):
    d = np.asarray(data, np.int64)
    pair = np.stack([d & 15, d >> 4] if low_first else [d >> 4, d & 15], axis=1)
    return pair.ravel()


def coverage_ima(cs):
    """name -> bool over the cases of the IMA fixture"""
    by = {(c.kind, c.a, c.b, c.tag): c for c in cs}
    got = {}
    steps = set()
    for c in cs:
        steps |= {int(w[W_IMA["step_index"]]) for _, _, w in c.calls}
    got["step_index 0"] = 0 in steps
    got["step_index 88"] = 88 in steps
    outs = np.concatenate([c.want for c in cs if c.kind == DECODE])
    got["saturate16 at +32767"] = bool((outs == 32767).any())
    got["saturate16 at -32768"] = bool((outs == -32768).any())
    # DVI4 without headers carries the codes bare: the VDVI encoder on the same line makes the same ones (encode() and its
    # state do not know the packing), and the VDVI decoder of that stream takes them back
    enc = by[(ENCODE, DVI4, CHUNK, "line")]
    codes = _nibbles(enc.want)
    got["every VDVI code encoded"] = set(codes.tolist()) == set(range(16)) and (ENCODE, VDVI, CHUNK, "line") in by
    dec = by[(DECODE, VDVI, CHUNK, "line")]
    got["every VDVI code decoded"] = set(codes.tolist()) == set(range(16)) and len(dec.want) >= len(line())
    pads, at = set(), 0
    for n, count, _ in by[(ENCODE, VDVI, CHUNK, "line")].calls:
        bits = int(sum(VDVI_BITS[int(x) & 7] for x in codes[at:at + n]))
        at += n
        assert count == (bits + 7)//8
        pads.add((-bits) % 8)
    got["VDVI pad lengths 1 .. 7"] = pads >= set(range(1, 8))
    for name, v in (("IMA4", IMA4), ("DVI4", DVI4)):
        got["an odd nibble carried, " + name] = any(int(w[W_IMA["bits"]]) & 1 for _, _, w in by[(ENCODE, v, CHUNK, "line")].calls[:-1])
    got["every configuration, both directions, and a random line per decoder"] = all(
        (k, v, ch, t) in by for v, ch in IMA_CONFIGS for k, t in ((ENCODE, "line"), (DECODE, "line"), (DECODE, "rnd")))
    return got


def coverage_oki(cs):
    by = {(c.kind, c.a, c.tag): c for c in cs}
    got = {}
    steps = set()
    for c in cs:
        steps |= {int(w[W_OKI["step_index"]]) for _, _, w in c.calls}
    got["step_index 0"] = 0 in steps
    got["step_index 48"] = 48 in steps
    outs = np.concatenate([c.want for c in cs if c.kind == DECODE and c.a == 32000])
    got["clamp at 2047"] = bool((outs == 2047*16).any())
    got["clamp at -2048"] = bool((outs == -2048*16).any())
    got["an odd nibble carried"] = any(int(w[W_OKI["mark"]]) & 1 for _, _, w in by[(ENCODE, 32000, "line")].calls[:-1])
    for kind, name in ((ENCODE, "encoder"), (DECODE, "decoder")):
        c = by[(kind, 24000, "line")]
        # (what a call finds is what init, the call before it or a set_state left: no call of the decoder leaves phase 1 behind,
        # its calls end on a nibble taken, so one case of the fixture begins there)
        entries = {0} | {int(w[W_OKI["phase"]]) for _, _, w in c.calls[:-1]}
        entries |= {x.entry_phase for x in cs if x.kind == kind and x.a == 24000}
        got["every entry phase of the 24k " + name] = entries == {0, 1, 2, 3}
        ptrs = [int(w[W_OKI["ptr"]]) for _, _, w in c.calls]
        got["ptr wrapping, " + name] = any(q < p for p, q in zip(ptrs, ptrs[1:]))
    # the sums restated: they give the fixture's samples and codes, and some lie outside int16 before the narrowing
    dec24 = by[(DECODE, 24000, "rnd")]
    dec32 = by[(DECODE, 32000, "rnd")]
    assert np.array_equal(dec24.data, dec32.data)
    z = oki24_decoder_sums(dec32.want)
    mine = np.array([narrow(v) for v in z], np.int64)
    assert np.array_equal(mine, dec24.want.astype(np.int64)), "the restated decoder sums are not the fixture's samples"
    got["a 24k decoder sample outside int16 before narrowing"] = any(abs(int(v)) > 32768 for v in z)
    z = oki24_encoder_sums(line())
    got["a 24k encoder input outside int16 before narrowing"] = any(abs(int(v)) > 32768 for v in z)
    got["both rates, both directions, and a random line per decoder"] = all(
        (k, r, t) in by for r in (32000, 24000) for k, t in ((ENCODE, "line"), (DECODE, "line"), (DECODE, "rnd")))
    return got


COVERAGE = {IMA: coverage_ima, OKI: coverage_oki}


# ---- generated lines: random configurations, random call cuts, amplitudes from silence to full scale -----------------------

def generated_inputs(family, count, seed, longest=400):
    """(a, b, amp, lens) per line"""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        a, b = CONFIGS[family][rng.randint(len(CONFIGS[family]))]
        if family == IMA and b:
            b = int(rng.randint(1, 1000))
        n = int(rng.randint(1, longest + 1))
        kind = rng.randint(5)
        scale = 0.0 if kind == 0 else 32767.0*10.0**(-4.5*rng.rand()) if kind < 4 else 32767.0
        t = np.arange(n)
        shape = rng.randint(3)
        if shape == 0:
            x = scale*(2.0*rng.rand(n) - 1.0)
        elif shape == 1:
            x = scale*np.sin(2.0*np.pi*rng.uniform(50.0, 3900.0)*t/8000.0 + rng.rand())
        else:
            x = scale*np.where(rng.rand(n) < 0.5, -1.0, 1.0) - (0.5 if kind == 4 else 0.0)
        amp = _to_int16(x)
        lens, left = [], n
        while left > 0:
            k = int(min(left, rng.randint(1, 1 + max(1, min(left, 170)))))
            lens.append(k)
            left -= k
        out.append((a, b, amp, lens))
    return out


def generated_cases(L, offsets, family, count, seed):
    """an encoder and a decoder per generated line, the decoder of every third one on random bytes instead of the codes"""
    out = []
    rng = np.random.RandomState(seed ^ 0x5EED)
    for i, (a, b, amp, lens) in enumerate(generated_inputs(family, count, seed)):
        enc, dec = reference_cases(L, offsets, family, a, b, amp, "g%d" % i, lens)
        if i % 3 == 2:
            noise = rng.randint(0, 256, len(dec.data) + 8).astype(np.uint8)
            if family == IMA and b == 0:
                dlens, at = [], 0
                while len(noise) - at >= 5:
                    k = int(min(len(noise) - at, rng.randint(5, 60)))
                    noise[at + 2] %= 89
                    dlens.append(k)
                    at += k
                noise = noise[:at]
            else:
                dlens = calls(len(noise), (int(rng.randint(1, 50)), int(rng.randint(1, 9)), 3))
            dec = run_reference(L, offsets, family, DECODE, a, b, "g%dr" % i, noise, dlens, not is_packets(family, a, b))
        out += [enc, dec]
    return out


# ---- the host-compiled step functions as a yardstick for a bank (tests/test_adpcm_gpu.py) ----------------------------------

def build_host_program(out_dir, sanitize=True):
    """tests/c_callers/adpcm_host.cpp: csrc/adpcm_dev.hpp for the host"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(out_dir, "adpcm_host")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-O1", "-g"]
    cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    cmd += [os.path.join(root, "tests", "c_callers", "adpcm_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    return exe


def host_cases(exe, work_dir, todo):
    """todo: (family, kind, a, b, data, lens) each; returns the cases the host-compiled functions make of them"""
    blank = [Case(f, k, a, b, "h%d" % i, np.asarray(d), np.zeros(0, np.int64), [(n, 0, np.zeros(WORDS[f], np.int32)) for n in lens], False)
             for i, (f, k, a, b, d, lens) in enumerate(todo)]
    path = os.path.join(work_dir, "host_in.txt")
    dump_text(path, blank)
    p = subprocess.run([exe, "--run", path], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = p.stdout.splitlines()
    at = 0
    for c in blank:
        head = rows[at].split()
        assert head[0] == "O"
        c.want = np.array(head[2:], np.int64).astype(np.int16 if c.kind == DECODE else np.uint8)
        assert len(c.want) == int(head[1])
        at += 1
        calls_made = []
        for n, _, _ in c.calls:
            k = rows[at].split()
            assert k[0] == "K"
            calls_made.append((n, int(k[1]), np.array(k[2:], np.int64).astype(np.int32)))
            at += 1
        c.calls = calls_made
    assert at == len(rows)
    return blank
