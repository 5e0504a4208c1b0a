"""The lines of the GSM 06.10 fixture (tests/golden/gsm0610.npz) and what the tests of the banks share.  Numpy's sine, double
arithmetic and a 32-bit linear congruential generator, nothing else; the fixture stores a CRC of every line, so a platform
on which a sample rounds the other way shows as that, not as a codec mismatch.

  lines()          five int16 lines of 12 frames: silence then a full-scale square, a pulse train whose period sweeps the lags,
                   noise of +-8, full-scale noise, a decaying 440 Hz tone
  random_codes()   per packing, code bytes no encoder made: 12 VoIP frames, 6 WAV49 pairs, 12 unpacked frames whose bytes are
                   masked to the parameters' widths (wider ones are undefined in the reference)
  PACKINGS         NONE, WAV49, VOIP with the reference's values
"""
import os
import zlib

import numpy as np

NONE, WAV49, VOIP = 0, 1, 2
PACKINGS = (NONE, WAV49, VOIP)
FRAME = 160
N_FRAMES = 12
N = FRAME*N_FRAMES
WORDS = 160
W_PACKING, W_DP0, W_Z1, W_LZ2, W_MP, W_U0, W_LARPP, W_J, W_NRP, W_V0, W_MSR = 0, 1, 121, 122, 123, 124, 132, 148, 149, 150, 159
ENCODE, DECODE = 0, 1
SCHEDULE = (1, 3, 2)                # frames a call, cycled
SCHEDULE_WAV49 = (2, 4, 2)
SEED = 12345
# the widths of a frame's 76 parameters in stream order: LARc[8], then per subframe Nc, bc, Mc, xmaxc, xMc[13]
WIDTHS = (6, 6, 5, 5, 4, 4, 3, 3) + ((7, 2, 2, 6) + (3,)*13)*4
# where a subframe's parameters are in an unpacked frame
P_NC, P_BC, P_MC, P_XMAXC, P_XMC = 0, 1, 2, 3, 4


def unit_samples(packing):
    return 320 if packing == WAV49 else 160


def unit_bytes(packing):
    return {NONE: 76, WAV49: 65, VOIP: 33}[packing]


def schedule(packing):
    return SCHEDULE_WAV49 if packing == WAV49 else SCHEDULE


class Lcg:
    def __init__(self, seed):
        self.x = seed & 0xFFFFFFFF

    def r(self):
        self.x = (self.x*1664525 + 1013904223) & 0xFFFFFFFF
        return self.x >> 16


def _generate():
    g = Lcg(SEED)
    i = np.arange(N)
    square = np.where((i >> 3) & 1, 32767, -32768)
    square[:320] = 0
    pulses = np.zeros(N)
    at, period = 0, 40
    while at < N:
        pulses[at] = 2000 + 14*at
        at += period
        period += 3
        if period > 125:
            period = 38
    train = np.zeros(N)
    y1 = y2 = 0.0
    for k in range(N):
        y = pulses[k] + 1.6*y1 - 0.81*y2
        y = min(max(y, -32768.0), 32767.0)
        train[k] = y
        y2, y1 = y1, y
    small = np.array([g.r() % 17 - 8 for _ in range(N)])
    full = np.array([g.r() for _ in range(N)], np.uint16).view(np.int16)
    tone = np.trunc(10000.0*(1.0 - i/1920.0)*np.sin(2.0*np.pi*440.0*i/8000.0))
    the_lines = [np.ascontiguousarray(x).astype(np.int16) for x in (square, np.trunc(train), small, full, tone)]
    rnd = {VOIP: np.array([g.r() & 0xFF for _ in range(12*33)], np.uint8),
           WAV49: np.array([g.r() & 0xFF for _ in range(6*65)], np.uint8),
           NONE: np.array([g.r() & ((1 << WIDTHS[k % 76]) - 1) for k in range(12*76)], np.uint8)}
    return the_lines, rnd


_CACHE = []


def _all():
    if not _CACHE:
        _CACHE.append(_generate())
    return _CACHE[0]


def lines():
    return [x.copy() for x in _all()[0]]


def random_codes(packing):
    return _all()[1][packing].copy()


def line_crcs():
    return np.array([zlib.crc32(x.tobytes()) for x in lines()], np.uint32)


def calls(n_frames, packing):
    """the frames of every call of the schedule"""
    sched = schedule(packing)
    out, k = [], 0
    while n_frames > 0:
        n = min(sched[k % len(sched)], n_frames)
        out.append(n)
        n_frames -= n
        k += 1
    return out


def key(packing):
    return {NONE: "none", WAV49: "wav49", VOIP: "voip"}[packing]


def params_of(unpacked):
    """an unpacked stream as [frame][76]"""
    return np.asarray(unpacked).reshape(-1, 76)


def subframes(unpacked):
    """[frame*4][17]: Nc, bc, Mc, xmaxc, xMc[13]"""
    return params_of(unpacked)[:, 8:].reshape(-1, 17)


class Case:
    """One codec of the fixture: kind, packing, the input items (samples or bytes), the output items, and per call
    (len, count, the 160 state words after it)."""

    def __init__(self, kind, packing, line, data, want, the_calls):
        self.kind, self.packing, self.line = kind, packing, line
        self.data, self.want, self.calls = data, want, the_calls

    @property
    def name(self):
        return "%s_%s_%s" % ("dec" if self.kind else "enc", key(self.packing), self.line)


def load(path=None):
    return np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gsm0610.npz"))


def cases(g):
    out = []
    the_lines = lines()
    assert np.array_equal(line_crcs(), g["line_crcs"]), "the lines generated here are not the fixture's"
    for p in PACKINGS:
        k = key(p)
        frames = calls(N_FRAMES, p)
        elens = [f*FRAME for f in frames]
        dlens = [f*unit_bytes(p)//(2 if p == WAV49 else 1) for f in frames]
        for li in range(len(the_lines)):
            codes, pcm = g["codes_" + k][li], g["pcm_" + k][li]
            out.append(Case(ENCODE, p, li, the_lines[li], codes, [(n, int(c), w) for n, c, w in zip(elens, g["ecounts_" + k][li], g["ewords_" + k][li])]))
            out.append(Case(DECODE, p, li, codes, pcm, [(n, int(c), w) for n, c, w in zip(dlens, g["dcounts_" + k][li], g["dwords_" + k][li])]))
        noise = random_codes(p)
        out.append(Case(DECODE, p, "rnd", noise, g["rnd_" + k], [(n, int(c), w) for n, c, w in zip(dlens, g["rndcounts_" + k], g["rndwords_" + k])]))
    return out


def dump_text(path, the_cases):
    """the cases as the stand-alone host program reads them (tests/c_callers/gsm0610_host.cpp)"""
    with open(path, "w") as f:
        for c in the_cases:
            f.write("C %d %d %d %d %d\n" % (c.kind, c.packing, len(c.data), len(c.want), len(c.calls)))
            f.write(" ".join(map(str, np.asarray(c.data).astype(np.int64).tolist())) + "\n")
            f.write(" ".join(map(str, np.asarray(c.want).astype(np.int64).tolist())) + "\n")
            for n, count, w in c.calls:
                f.write("%d %d %s\n" % (n, count, " ".join(map(str, np.asarray(w).astype(np.int64).tolist()))))
        f.write("E\n")
    return len(the_cases)


def coverage(g):
    """what the fixture has to cover, as a dict of facts (the generator and tests/test_gsm0610.py assert on it)"""
    sub = np.concatenate([subframes(g["codes_none"][li]) for li in range(5)])
    rnd = params_of(unpack_voip_stream(random_codes(VOIP)))[:, 8:].reshape(-1, 17)
    return {"bc": set(sub[:, P_BC].tolist()), "Mc": set(sub[:, P_MC].tolist()), "Nc": set(sub[:, P_NC].tolist()),
            "xmaxc": set(sub[:, P_XMAXC].tolist()), "xMc": set(sub[:, P_XMC:].reshape(-1).tolist()),
            "zero_frame": any(not x[f*FRAME:(f + 1)*FRAME].any() for x in lines() for f in range(N_FRAMES)),
            "rnd_lags_out": int(np.count_nonzero((rnd[:, P_NC] < 40) | (rnd[:, P_NC] > 120)))}


def unpack_voip_stream(codes):
    """33-byte frames to unpacked parameters, from the layout: the nibble, then the parameters, first bit on top"""
    out = []
    for f in np.asarray(codes, np.uint8).reshape(-1, 33):
        bits = np.unpackbits(f)[4:]
        at = 0
        for w in WIDTHS:
            out.append(int("".join(map(str, bits[at:at + w].tolist())), 2))
            at += w
    return np.array(out, np.uint8)


def pack_voip_stream(params):
    out = []
    for f in params_of(params):
        bits = "1101" + "".join(format(int(v) & ((1 << w) - 1), "0%db" % w) for v, w in zip(f, WIDTHS))
        out.extend(int(bits[i:i + 8], 2) for i in range(0, 264, 8))
    return np.array(out, np.uint8)


def pack_wav49_stream(params):
    """pairs of frames to 65 bytes: the parameters of both, first bit at the bottom"""
    out = []
    for pair in params_of(params).reshape(-1, 2, 76):
        bits = "".join(format(int(v) & ((1 << w) - 1), "0%db" % w)[::-1] for f in pair for v, w in zip(f, WIDTHS))
        out.extend(int(bits[i:i + 8][::-1], 2) for i in range(0, 520, 8))
    return np.array(out, np.uint8)
