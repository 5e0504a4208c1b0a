"""The lines of the G.722 fixture (tests/golden/g722.npz) and the bank configurations the tests share.  The lines are the
heads of the G.726 fixture's (g726_lines.lines(): numpy's sine and a 32-bit linear congruential generator, nothing else);
the fixture stores a CRC of every line, so a platform on which a sample rounds the other way shows as that, not as a codec
mismatch.

  lines()          three int16 lines of 3 000 samples: the ten-segment line, the gated 3900 Hz line, the modulated 300 Hz line
                   (a 16 kHz channel takes them as 16 kHz samples, an 8 kHz one as 8 kHz samples: test signals either way)
  random_bytes()   600 bytes of noise for one configuration: the decoder's random-byte line
  CONFIGS          the 12 (rate, eight_k, packed) configurations, in the order the banks of the tests cycle them
"""
import os
import zlib

import numpy as np

import g726_lines as G6

RATES = (48000, 56000, 64000)
EIGHT_K, PACKED = 1, 2                  # G722_SAMPLE_RATE_8000, G722_PACKED
CONFIGS = tuple((r, e, p) for r in RATES for e in (0, 1) for p in (0, 1))
ENC_SCHEDULE_16K = (160, 2, 14, 80, 334)        # samples: a 16 kHz encoder takes pairs
ENC_SCHEDULE_8K = (160, 1, 7, 80, 333)          # samples
DEC_SCHEDULE = (160, 1, 7, 80, 333)             # bytes
N = 3000
N_RANDOM = 600
WORDS = 74
W_PACKED, W_EIGHT_K, W_BPS, W_X0, W_Y0, W_PTR, W_BAND0, W_BAND1, W_BUFFER, W_BITS = 0, 1, 2, 3, 15, 27, 28, 50, 72, 73
ENCODE, DECODE = 0, 1


def bits_of(rate):
    return {48000: 6, 56000: 7, 64000: 8}[rate]


def options_of(eight_k, packed):
    return (EIGHT_K if eight_k else 0) | (PACKED if packed else 0)


def stored(rate, eight_k, packed):
    """the configuration whose streams the fixture holds for this one: G722_PACKED means nothing at 64000"""
    return (rate, eight_k, 0 if rate == 64000 else packed)


def lines():
    return [np.ascontiguousarray(x[:N]) for x in G6.lines()]


def line_crcs():
    return np.array([zlib.crc32(x.tobytes()) for x in lines()], np.uint32)


def random_bytes(rate, eight_k, packed):
    return G6.Lcg(0x722 + rate + options_of(eight_k, packed)).bytes(N_RANDOM)


def enc_schedule(eight_k):
    return ENC_SCHEDULE_8K if eight_k else ENC_SCHEDULE_16K


calls = G6.calls


def key(rate, eight_k, packed):
    return "%d_%d_%d" % (rate, eight_k, packed)


class Case:
    """One codec of the fixture: kind, configuration, the input items (samples or bytes), the output items, and per call
    (len, count, the 74 state words after it)."""

    def __init__(self, kind, rate, eight_k, packed, line, data, want, calls):
        self.kind, self.rate, self.eight_k, self.packed, self.line = kind, rate, eight_k, packed, line
        self.data, self.want, self.calls = data, want, calls

    @property
    def config(self):
        return (self.rate, self.eight_k, self.packed)

    @property
    def name(self):
        return "%s_%d_%d_%d_%s" % ("dec" if self.kind else "enc", self.rate, self.eight_k, self.packed, self.line)


def load(path=None):
    return np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g722.npz"))


def cases(g):
    out = []
    the_lines = lines()
    assert np.array_equal(line_crcs(), g["line_crcs"]), "the lines generated here are not the fixture's"
    for rate, eight_k, packed in CONFIGS:
        k = key(*stored(rate, eight_k, packed))
        for li in range(3):
            row = the_lines[li]
            codes = g["codes_" + k][li]
            pcm = g["pcm_" + k][li]
            ew = g["ewords_" + k][li].astype(np.int32)
            dw = g["dwords_" + k][li].astype(np.int32)
            elens = calls(len(row), enc_schedule(eight_k))
            dlens = calls(len(codes), DEC_SCHEDULE)
            out.append(Case(ENCODE, rate, eight_k, packed, li, row, codes, [(n, int(c), w) for n, c, w in zip(elens, g["ecounts_" + k][li], ew)]))
            out.append(Case(DECODE, rate, eight_k, packed, li, codes, pcm, [(n, int(c), w) for n, c, w in zip(dlens, g["dcounts_" + k][li], dw)]))
        noise = random_bytes(*stored(rate, eight_k, packed))
        rw = g["rndwords_" + k].astype(np.int32)
        out.append(Case(DECODE, rate, eight_k, packed, "rnd", noise, g["rnd_" + k],
                        [(n, int(c), w) for n, c, w in zip(calls(len(noise), DEC_SCHEDULE), g["rndcounts_" + k], rw)]))
    return out


def dump_text(path, the_cases):
    """the cases as the stand-alone host program reads them (tests/c_callers/g722_host.cpp)"""
    with open(path, "w") as f:
        for c in the_cases:
            f.write("C %d %d %d %d %d %d\n" % (c.kind, c.rate, options_of(c.eight_k, c.packed), len(c.data), len(c.want), len(c.calls)))
            f.write(" ".join(map(str, np.asarray(c.data).astype(np.int64).tolist())) + "\n")
            f.write(" ".join(map(str, np.asarray(c.want).astype(np.int64).tolist())) + "\n")
            for n, count, w in c.calls:
                f.write("%d %d %s\n" % (n, count, " ".join(map(str, np.asarray(w).astype(np.int64).tolist()))))
        f.write("E\n")
    return len(the_cases)
