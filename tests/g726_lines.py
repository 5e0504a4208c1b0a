"""The lines of the G.726 fixture (tests/golden/g726.npz) and the bank configurations the tests share.  Deterministic:
numpy's sine and a 32-bit linear congruential generator, nothing else; the fixture stores a CRC of every line, so a
platform on which a sample rounds the other way shows as that, not as a codec mismatch.

  lines()          three int16 lines of 4 000 samples: the ten-segment line, the gated 3900 Hz line, the modulated 300 Hz line
  random_bytes()   1 000 bytes of noise for one (rate, coding): the decoder's random-code line
  pcm_row()        a line in a coding: int16, or G.711 bytes (G.711 is restated here in numpy)
  CONFIGS          the 36 (rate, coding, packing) configurations, in the order the banks of the tests cycle them
"""
import os
import zlib

import numpy as np

RATES = (16000, 24000, 32000, 40000)
LINEAR, ULAW, ALAW = 0, 1, 2
PACK_NONE, PACK_LEFT, PACK_RIGHT = 0, 1, 2
CODINGS = (LINEAR, ULAW, ALAW)
PACKINGS = (PACK_NONE, PACK_LEFT, PACK_RIGHT)
CONFIGS = tuple((r, c, p) for r in RATES for c in CODINGS for p in PACKINGS)
SCHEDULE = (160, 1, 7, 80, 333)         # the fixture's calls: samples for the encoder, bytes for the decoder
N = 4000
SEG = 400


class Lcg:
    """x <- 1664525 x + 1013904223 mod 2^32; a sample is the top 16 bits"""

    def __init__(self, seed):
        self.x = seed & 0xFFFFFFFF

    def int16(self, n):
        out = np.empty(n, np.int64)
        x = self.x
        for i in range(n):
            x = (x*1664525 + 1013904223) & 0xFFFFFFFF
            out[i] = (x >> 16) - 65536 if x & 0x80000000 else x >> 16
        self.x = x
        return out

    def bytes(self, n):
        return (self.int16(n) & 0xFF).astype(np.uint8)


def _tone(freq, amp, n, start=0):
    t = np.arange(start, start + n, dtype=np.float64)
    return amp*np.sin(2.0*np.pi*freq*t/8000.0)


def _gated_3900(n):
    gate = ((np.arange(n)//200) % 2 == 0).astype(np.float64)
    return _tone(3900, 30000.0, n)*gate


def _modulated_300(n, rng):
    t = np.arange(n, dtype=np.float64)
    am = 1.0 + 0.9*np.sin(2.0*np.pi*3.0*t/8000.0)
    return _tone(300, 3000.0, n)*am + rng.int16(n)/40.0


def _fsk(n):
    freq = np.where((np.arange(n)//27) % 2 == 0, 1650.0, 1850.0)
    phase = np.cumsum(2.0*np.pi*freq/8000.0)
    return 10000.0*np.sin(phase)


def _to_int16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def lines():
    rng = Lcg(0x6726)
    k = np.arange(SEG)
    segs = [np.zeros(SEG),
            _tone(697, 8000.0, SEG) + _tone(1209, 8000.0, SEG),
            _tone(2100, 20000.0, SEG),
            np.where((k % 6) < 3, 32767.0, -32768.0),
            rng.int16(SEG).astype(np.float64),
            rng.int16(SEG)/64.0,
            _fsk(SEG),
            _gated_3900(SEG),
            np.where(k % 2 == 0, 32767.0, -32768.0),
            _modulated_300(SEG, rng)]
    ten = _to_int16(np.concatenate(segs))
    gated = _to_int16(_gated_3900(N))
    modulated = _to_int16(_modulated_300(N, Lcg(0x300)))
    return [ten, gated, modulated]


def line_crcs():
    return np.array([zlib.crc32(x.tobytes()) for x in lines()], np.uint32)


def random_bytes(rate, coding):
    return Lcg(0xC0DE + rate + coding).bytes(1000)


# ---- G.711 (ITU-T G.711; the same segment arithmetic every implementation uses) ----------------------------------------

def _top_bit(x):
    return np.floor(np.log2(np.maximum(x, 1))).astype(np.int64)


def linear_to_ulaw(x):
    x = np.asarray(x, np.int64)
    mask = np.where(x >= 0, 0xFF, 0x7F)
    mag = 0x84 + np.abs(x)
    seg = _top_bit(mag | 0xFF) - 7
    v = np.where(seg >= 8, 0x7F, (seg << 4) | ((mag >> np.minimum(seg + 3, 30)) & 0xF))
    return (v ^ mask).astype(np.uint8)


def linear_to_alaw(x):
    x = np.asarray(x, np.int64)
    mask = np.where(x >= 0, 0xD5, 0x55)
    mag = np.where(x >= 0, x, -x - 1)
    seg = _top_bit(mag | 0xFF) - 7
    v = np.where(seg >= 8, 0x7F, (seg << 4) | ((mag >> np.where(seg > 0, np.minimum(seg + 3, 30), 4)) & 0xF))
    return (v ^ mask).astype(np.uint8)


def pcm_row(line, coding):
    """what a channel of this coding finds in its PCM row for the line"""
    if coding == ULAW:
        return linear_to_ulaw(line)
    if coding == ALAW:
        return linear_to_alaw(line)
    return np.asarray(line, np.int16)


def pcm_dtype(coding):
    return np.int16 if coding == LINEAR else np.uint8


def calls(total, schedule=SCHEDULE):
    """the call lengths that take `total` items on a schedule, cycled; the last one is what is left"""
    out, k = [], 0
    while total > 0:
        n = min(schedule[k % len(schedule)], total)
        out.append(n)
        total -= n
        k += 1
    return out


def key(rate, coding, line):
    return "%d_%d_%s" % (rate, coding, line)


# ---- the fixture as cases ------------------------------------------------------------------------------------------------

W_BITSTREAM, W_RESIDUE, W_PACKING, WORDS = 24, 25, 29, 30
ENCODE, DECODE = 0, 1


class Case:
    """One codec of the fixture: kind, configuration, the input items, the output items, and per call (len, count, the state
    words after it or None where the fixture has none)."""

    def __init__(self, kind, rate, coding, packing, line, data, want, calls):
        self.kind, self.rate, self.coding, self.packing, self.line = kind, rate, coding, packing, line
        self.data, self.want, self.calls = data, want, calls

    @property
    def name(self):
        return "%s_%d_%d_%d_%s" % ("dec" if self.kind else "enc", self.rate, self.coding, self.packing, self.line)


def load(path=None):
    return np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g726.npz"))


def cases(g):
    out = []
    the_lines = lines()
    assert np.array_equal(line_crcs(), g["line_crcs"]), "the lines generated here are not the fixture's"
    for rate in RATES:
        for coding in CODINGS:
            for li in range(3):
                row = pcm_row(the_lines[li], coding)
                codes = g["codes_%d" % rate][coding][li]
                words = g["words_%d" % rate][coding][li]
                pcm = g["out_lin_%d" % rate][li] if coding == LINEAR else g["out_law_%d" % rate][coding - 1][li]
                lens = calls(len(row))
                out.append(Case(ENCODE, rate, coding, PACK_NONE, li, row, codes, [(n, n, w) for n, w in zip(lens, words)]))
                out.append(Case(DECODE, rate, coding, PACK_NONE, li, codes, pcm, [(n, n, w) for n, w in zip(lens, words)]))
                for p in (PACK_LEFT, PACK_RIGHT):
                    packed = g["packed%d_%d" % (p, rate)][coding][li]
                    meta = g["pkmeta%d_%d" % (p, rate)][coding][li]
                    fin = g["finals_%d" % rate][p - 1][coding][li]
                    # the packing encoder's words: the unpacked encoder's, with its own bit stream words
                    pw = words.copy()
                    pw[:, W_BITSTREAM] = meta[:, 1]
                    pw[:, W_RESIDUE] = meta[:, 2]
                    pw[:, W_PACKING] = p
                    assert np.array_equal(pw[-1], fin[0])
                    out.append(Case(ENCODE, rate, coding, p, li, row, packed, [(n, int(c), w) for n, c, w in zip(lens, meta[:, 0], pw)]))
                    counts = g["upcounts%d_%d" % (p, rate)][coding][li]
                    blens = calls(len(packed))
                    dcalls = [(n, int(c), None) for n, c in zip(blens, counts)]
                    dcalls[-1] = (dcalls[-1][0], dcalls[-1][1], fin[1])
                    out.append(Case(DECODE, rate, coding, p, li, packed, pcm[:int(counts.sum())], dcalls))
            noise = random_bytes(rate, coding)
            pcm = g["rnd_lin_%d" % rate] if coding == LINEAR else g["rnd_law_%d" % rate][coding - 1]
            lens = calls(len(noise))
            out.append(Case(DECODE, rate, coding, PACK_NONE, "rnd", noise, pcm, [(n, n, w) for n, w in zip(lens, g["rnd_words_%d" % rate][coding])]))
    return out


def dump_text(path, the_cases):
    """the cases as the stand-alone host program reads them (tests/c_callers/g726_host.cpp)"""
    with open(path, "w") as f:
        for c in the_cases:
            f.write("C %d %d %d %d %d %d %d\n" % (c.kind, c.rate, c.coding, c.packing, len(c.data), len(c.want), len(c.calls)))
            f.write(" ".join(map(str, np.asarray(c.data).astype(np.int64).tolist())) + "\n")
            f.write(" ".join(map(str, np.asarray(c.want).astype(np.int64).tolist())) + "\n")
            for n, count, w in c.calls:
                if w is None:
                    f.write("%d %d 0\n" % (n, count))
                else:
                    f.write("%d %d 1 %s\n" % (n, count, " ".join(map(str, np.asarray(w).astype(np.int64).tolist()))))
        f.write("E\n")
    return len(the_cases)
