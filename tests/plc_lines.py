"""The lines and schedules of the packet loss concealment fixture (tests/golden/plc.npz) and what the tests of the banks share.
Numpy's sine, double arithmetic and a 32-bit linear congruential generator, nothing else; the fixture stores a CRC of every
line, so a platform on which a sample rounds the other way shows as that, not as a mismatch of the concealer.

  lines()       nine int16 lines of 4000 samples (NAMES): silence, a square of period 50, a saw of period 30, sines of period
                40, 120 and 133.3, a voiced sound of period 73.4 in noise, full-scale noise, and a square of period 97 on the rails
  SCHEDULE      the (lost, len) calls every line goes through; a heard call takes the line's samples at the stream's time
  DEC_TICKS     the ticks of the decoded-line cases (the five decoded VoIP lines of tests/golden/gsm0610.npz): 1 is a lost
                tick, filled in for 160 samples, and the decoder's next frame arrives a tick later
"""
import os
import zlib

import numpy as np

WORDS = 404
W_MISSING, W_OFFSET, W_PITCH, W_PITCHBUF, W_HISTORY, W_BUF_PTR = 0, 1, 2, 3, 123, 403
HIST, SPAN, LAG_FIRST, LAG_LAST = 280, 160, 40, 120
N = 4000
SEED = 2718
NAMES = ("silence", "square50", "saw30", "sine40", "sine120", "sine133", "voiced", "noise_fs", "rails")
SCHEDULE = ((0, 160), (0, 160), (1, 160), (0, 160), (0, 7), (1, 5), (1, 3), (0, 4), (0, 160), (1, 160), (1, 160), (1, 160), (0, 160),
            (0, 320), (1, 33), (0, 9), (0, 151), (1, 160), (1, 160), (1, 160), (1, 160), (0, 3), (0, 160), (0, 1), (1, 1), (0, 161))
HEARD_ONLY = tuple((0, n) for _, n in SCHEDULE)
HEARD_LINE = 6                      # the line of the heard-only case
FRAME = 160
DEC_TICKS = (0, 0, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0)
DEC_LINES = 5
MAX_FIXTURE_BYTES = 478071


class Lcg:
    def __init__(self, seed):
        self.x = seed & 0xFFFFFFFF

    def r(self):
        self.x = (self.x*1664525 + 1013904223) & 0xFFFFFFFF
        return self.x >> 16


def _generate():
    g = Lcg(SEED)
    t = np.arange(N)
    silence = np.zeros(N)
    square50 = np.where(t % 50 < 25, 8000, -8000)
    saw30 = ((t % 30) - 15)*1000
    sine40 = np.rint(12000.0*np.sin(2.0*np.pi*t/40.0))
    sine120 = np.rint(12000.0*np.sin(2.0*np.pi*t/120.0))
    sine133 = np.rint(12000.0*np.sin(2.0*np.pi*t/133.3))
    # (a sum of twelve uniforms stands for the Gaussian)
    gauss = np.array([sum(g.r() for _ in range(12))/65536.0 - 6.0 for _ in range(N)])
    voiced = np.rint(6000.0*sum(np.sin(2.0*np.pi*k*t/73.4 + k)/k for k in range(1, 8)) + 300.0*gauss)
    voiced = np.clip(voiced, -32768, 32767)
    noise_fs = np.array([g.r() for _ in range(N)], np.uint16).view(np.int16)
    rails = np.where(t % 97 < 48, 32767, -32768)
    return [np.ascontiguousarray(x).astype(np.int16) for x in (silence, square50, saw30, sine40, sine120, sine133, voiced, noise_fs, rails)]


_CACHE = []


def lines():
    if not _CACHE:
        _CACHE.append(_generate())
    return [x.copy() for x in _CACHE[0]]


def line_crcs():
    return np.array([zlib.crc32(x.tobytes()) for x in lines()], np.uint32)


class Case:
    """One concealer of the fixture: per call (lost, len, the row going in -- the line's samples, or the sentinel where the
    call is a fill-in --, the row coming out, the 404 words after it)."""

    def __init__(self, name, line, calls):
        self.name, self.line, self.calls = name, line, calls


SENTINEL = 0x5A5A


def rows_in(line, schedule):
    """What each call is given: a heard call the line's samples at the stream's time, a lost one a row of sentinels"""
    out, t = [], 0
    for lost, n in schedule:
        out.append(np.full(n, SENTINEL, np.int16) if lost else line[t:t + n].copy())
        t += n
    assert t <= len(line)
    return out


def dec_schedule():
    return tuple((lost, FRAME) for lost in DEC_TICKS)


def dec_rows_in(pcm):
    """the decoded line's frames on the ticks that are heard, in order"""
    out, f = [], 0
    for lost in DEC_TICKS:
        if lost:
            out.append(np.full(FRAME, SENTINEL, np.int16))
        else:
            out.append(np.asarray(pcm[f*FRAME:(f + 1)*FRAME], np.int16).copy())
            f += 1
    assert f*FRAME == len(pcm)
    return out


def load(path=None):
    return np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plc.npz"))


def load_gsm_pcm():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gsm0610.npz"))
    return g["pcm_voip"], g["codes_voip"]


def words_of(scal, pb, hist):
    w = np.zeros(WORDS, np.int32)
    w[:3] = scal[:3]
    w[W_PITCHBUF:W_HISTORY] = pb
    w[W_HISTORY:W_BUF_PTR] = hist
    w[W_BUF_PTR] = scal[3]
    return w


def split_words(w):
    """(scalars [4], pitchbuf bits [120], history [280]) of 404 words: how the fixture stores them"""
    w = np.asarray(w, np.int32)
    return (np.array([w[0], w[1], w[2], w[W_BUF_PTR]], np.int32), w[W_PITCHBUF:W_HISTORY].copy(), w[W_HISTORY:W_BUF_PTR].astype(np.int16))


def _group(g, key, names, schedule, ins):
    out = []
    for li, name in enumerate(names):
        flat = g[key + "_out"][li]
        calls, at = [], 0
        for k, (lost, n) in enumerate(schedule):
            w = words_of(g[key + "_scal"][li][k], g[key + "_pb"][li][k], g[key + "_hist"][li][k])
            calls.append((lost, n, ins[li][k], flat[at:at + n].copy(), w))
            at += n
        assert at == len(flat)
        out.append(Case("%s_%s" % (key, name), li, calls))
    return out


def sched_cases(g):
    the_lines = lines()
    assert np.array_equal(line_crcs(), g["line_crcs"]), "the lines generated here are not the fixture's"
    assert tuple(map(tuple, g["schedule"].tolist())) == SCHEDULE and tuple(g["dec_ticks"].tolist()) == DEC_TICKS
    return _group(g, "sched", NAMES, SCHEDULE, [rows_in(x, SCHEDULE) for x in the_lines])


def heard_case(g):
    return _group(g, "heard", [NAMES[HEARD_LINE]], HEARD_ONLY, [rows_in(lines()[HEARD_LINE], HEARD_ONLY)])[0]


def dec_cases(g):
    pcm, _ = load_gsm_pcm()
    return _group(g, "dec", ["line%d" % i for i in range(DEC_LINES)], dec_schedule(), [dec_rows_in(pcm[i]) for i in range(DEC_LINES)])


def cases(g):
    return sched_cases(g) + [heard_case(g)] + dec_cases(g)


def dump_text(path, the_cases):
    """the cases as the stand-alone host program reads them (tests/c_callers/plc_host.cpp)"""
    with open(path, "w") as f:
        for c in the_cases:
            f.write("C %d\n" % len(c.calls))
            for lost, n, row, out, w in c.calls:
                f.write("%d %d\n" % (lost, n))
                f.write(" ".join(map(str, row.astype(np.int64).tolist())) + "\n")
                f.write(" ".join(map(str, out.astype(np.int64).tolist())) + "\n")
                f.write(" ".join(map(str, np.asarray(w).astype(np.int64).tolist())) + "\n")
        f.write("E\n")
    return len(the_cases)


def time_order(w):
    """the last 280 samples of a line's words, oldest first"""
    return np.roll(np.asarray(w[W_HISTORY:W_BUF_PTR], np.int64), -int(w[W_BUF_PTR]))


def lag_sums(w):
    """the 81 sums of the pitch search on a line's words"""
    a = time_order(w)
    return np.array([np.abs(a[lag:lag + SPAN] - a[:SPAN]).sum() for lag in range(LAG_FIRST, LAG_LAST + 1)])


def coverage(the_cases):
    """what the fixture has to cover, as a dict of facts (the generator and tests/test_plc.py assert on it)"""
    c = {"pitches": set(), "ties": [], "lowest_wins": True, "cross_401": False, "dead_call": False, "short_start": False, "short_heard": False,
         "long_heard": False, "odd_buf_ptr": False, "rails": set(), "buf_ptr_end": set()}
    for case in the_cases:
        prev = np.zeros(WORDS, np.int32)
        for lost, n, _, out, w in case.calls:
            m0 = int(prev[W_MISSING])
            if lost and m0 == 0:
                sums = lag_sums(prev)
                tied = np.nonzero(sums == sums.min())[0] + LAG_FIRST
                c["ties"].append(len(tied))
                c["lowest_wins"] = c["lowest_wins"] and int(w[W_PITCH]) == int(tied[0])
                c["pitches"].add(int(w[W_PITCH]))
                c["short_start"] = c["short_start"] or n < (int(w[W_PITCH]) >> 2)
            if lost:
                c["rails"] |= {int(v) for v in (32767, -32768) if (out == v).any()}
                if m0 > 0 and m0 < 401 < m0 + n:
                    # 401 samples of a gap go through the gain, not 400: the offset into the cycle says which
                    k = 401 - m0
                    c["cross_401"] = c["cross_401"] or (out[:k].any() and not out[k:].any()
                                                        and int(w[W_OFFSET]) == (int(prev[W_OFFSET]) + k) % int(w[W_PITCH]))
                c["dead_call"] = c["dead_call"] or (m0 > 401 and not out.any())
            else:
                c["short_heard"] = c["short_heard"] or (m0 > 0 and n < (int(prev[W_PITCH]) >> 2))
                c["long_heard"] = c["long_heard"] or n >= HIST
            c["odd_buf_ptr"] = c["odd_buf_ptr"] or bool(w[W_BUF_PTR] & 1)
            prev = w
        c["buf_ptr_end"].add(int(prev[W_BUF_PTR]))
    return c


def check_coverage(c):
    assert {40, 120} <= c["pitches"] and len(c["pitches"] - {40, 120}) >= 3, c["pitches"]
    assert any(3 <= k < 81 for k in c["ties"]) and 81 in c["ties"] and c["lowest_wins"], c["ties"]
    assert c["cross_401"] and c["dead_call"] and c["short_start"] and c["short_heard"] and c["long_heard"] and c["odd_buf_ptr"], c
    assert c["rails"] == {32767, -32768}, c["rails"]
