"""The generated lines, configurations and call schedules of the codec sweep (tests/test_codec_sweep.py on the CPU,
tests/test_codec_sweep_gpu.py on the GPU): thousands of lines for the G.726, G.722 and GSM 06.10 codec banks and the packet
loss concealment bank, each compared with the live reference (oracle/ref_codecs.py).  Numpy's sine, double arithmetic and
32-bit linear congruential generators, nothing else, and fixed seeds: what is generated here is the same everywhere, so none
of it is committed.  (Should a platform round a sample of a sine the other way, both sides of every comparison still see the
same line; only the exact pins of the coverage test would say so.)

  lines(n, samples, seed)       [n][samples] int16; line i is of family FAMILIES[family_of(i)]: every 64 consecutive lines hold all
  configs(family, n)            per line: the configuration, cycled, so that every wave mixes all of them
  schedule_*(...)               per call, per line: lengths (and, for the concealer, the lost flags)
  random_bytes(n, count, seed)  [n][count] uint8
  coverage_*(...)               what the reference reached on these inputs, from its outputs and state words alone
  PINNED                        lines a sweep once failed on: (family, seed, line), kept in the sweep by name
"""
import numpy as np

import g722_lines as G2
import g726_lines as G6
import gsm0610_lines as GS
import plc_lines as PL

SEED = 0x5EED
WAVE = 64
N_GPU = 64*WAVE + 37                # 64 full waves and a partial one
FAMILIES = ("noise", "sine", "overdriven", "square", "dc_noise", "bursts", "pulses", "voiced", "tone_stops", "rail_runs", "chirp",
            "two_tone", "small", "nyquist_lf")
DEAL = 13                           # lines are dealt in rounds of 13 (coprime to the 36, 12 and 3 configurations); the last place
                                    # of a round goes to "small" and "nyquist_lf" in turn
PINNED = ()                         # (family, seed, line): nothing has failed yet
_M = np.uint64(0xFFFFFFFF)


_JUMP = [np.zeros(0, np.uint64), np.zeros(0, np.uint64)]


def _jump(count):
    """x_k = A_k x_0 + C_k mod 2^32 for k = 1 .. count"""
    if len(_JUMP[0]) < count:
        a, c, A, Cs = 1, 0, [], []
        for _ in range(count):
            a, c = (a*1664525) & 0xFFFFFFFF, (c*1664525 + 1013904223) & 0xFFFFFFFF
            A.append(a)
            Cs.append(c)
        _JUMP[0], _JUMP[1] = np.array(A, np.uint64), np.array(Cs, np.uint64)
    return _JUMP[0][:count], _JUMP[1][:count]


class Lcg:
    """n streams of x <- 1664525 x + 1013904223 mod 2^32, side by side; a draw is the top 16 bits"""

    def __init__(self, seeds):
        self.x = np.asarray(seeds, np.uint64) & _M

    def u16(self, count):
        A, Cs = _jump(count)
        x = (self.x[:, None]*A[None, :] + Cs[None, :]) & _M
        self.x = x[:, -1].copy()
        return (x >> np.uint64(16)).astype(np.int64)


def seeds_of(n, seed, salt=0):
    """one well-mixed 32-bit seed a line"""
    i = np.arange(n, dtype=np.uint64)
    x = (i*np.uint64(2654435761) + np.uint64((seed*40503 + salt*9176 + 12345) & 0xFFFFFFFF)) & _M
    x ^= x >> np.uint64(15)
    x = (x*np.uint64(2246822519)) & _M
    x ^= x >> np.uint64(13)
    return x


def family_of(i):
    """the index in FAMILIES of line i (a number or an array)"""
    i = np.asarray(i)
    return np.where((i % DEAL == DEAL - 1) & ((i//DEAL) % 2 == 1), DEAL, i % DEAL)


def _i16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


_lines_cache = {}


def lines(n, samples, seed=SEED):
    key = (n, samples, seed)
    if key not in _lines_cache:
        _lines_cache.clear()
        _lines_cache[key] = _lines(n, samples, seed)
        _lines_cache[key].setflags(write=False)
    return _lines_cache[key]


def _lines(n, samples, seed):
    g = Lcg(seeds_of(n, seed))
    P = g.u16(8)
    u = g.u16(samples)
    nz = u - 32768                                  # full-scale noise
    t = np.arange(samples, dtype=np.float64)[None, :]
    ti = np.arange(samples)[None, :]
    out = np.zeros((n, samples), np.int16)
    fam = family_of(np.arange(n))

    def rows(name):
        idx = np.flatnonzero(fam == FAMILIES.index(name))
        return idx, P[idx], nz[idx]

    idx, p, z = rows("noise")
    out[idx] = z >> (p[:, :1] % 16)
    idx, p, z = rows("sine")
    period = 16 + p[:, :1] % 201
    amp = np.minimum(32768.0, (1 << (p[:, 1:2] % 16))*(1.0 + p[:, 2:3]/65536.0))
    out[idx] = _i16(amp*np.sin(2.0*np.pi*t/period + p[:, 3:4]/65536.0))
    idx, p, z = rows("overdriven")
    period = 16 + p[:, :1] % 201
    out[idx] = _i16((40000.0 + 3.0*p[:, 1:2])*np.sin(2.0*np.pi*t/period))
    idx, p, z = rows("square")
    period = 2 + p[:, :1] % 199
    out[idx] = np.where((ti + p[:, 1:2]) % period < period//2, 32767, -32768)
    idx, p, z = rows("dc_noise")
    out[idx] = _i16((z >> (2 + p[:, 1:2] % 12)) + (p[:, :1] - 32768))
    idx, p, z = rows("bursts")
    frame = ti//160
    level = np.take_along_axis(u[idx], np.minimum(frame*160, samples - 1), axis=1) % 16
    out[idx] = np.where((frame + p[:, :1]) % 2 == 0, 0, z >> level)
    idx, p, z = rows("pulses")
    gap = 40 + p[:, :1] % 200
    out[idx] = np.where(u[idx] % gap == 0, np.roll(z, 1, axis=1), 0)
    idx, p, z = rows("voiced")
    period = 40.0 + (p[:, :1] % 8100)/100.0
    amp = 2000.0 + p[:, 2:3] % 20000
    v = sum(np.sin(2.0*np.pi*k*t/period + k)/k for k in (1, 2, 3))
    out[idx] = _i16(amp*v + (z >> (4 + p[:, 1:2] % 8)))
    idx, p, z = rows("tone_stops")
    freq = 3000.0 + p[:, :1] % 990
    run = 150 + p[:, 2:3] % 500
    out[idx] = _i16((5000.0 + p[:, 1:2] % 27000)*np.sin(2.0*np.pi*freq*t/8000.0)*((ti//run) % 2 == 0))
    idx, p, z = rows("rail_runs")
    run = 1 + p[:, :1] % 40
    sign = np.take_along_axis(z, ti//run, axis=1)
    # (a third of these lines rest at zero between runs)
    out[idx] = np.where((p[:, 1:2] % 3 == 0) & (sign & 3 == 0), 0, np.where(sign >= 0, 32767, -32768))
    idx, p, z = rows("chirp")
    period = 38.0 + (84.0*t/samples + p[:, :1] % 84) % 84.0
    out[idx] = _i16((1000.0 + p[:, 1:2] % 29000)*np.sin(np.cumsum(2.0*np.pi/period, axis=1)) + (z >> 8))
    idx, p, z = rows("two_tone")
    am = 1.0 + 0.9*np.sin(2.0*np.pi*(1 + p[:, 2:3] % 9)*t/8000.0)
    out[idx] = _i16((500.0 + p[:, 3:4] % 12000)*am*(np.sin(2.0*np.pi*(300 + p[:, :1] % 700)*t/8000.0)
                                                   + np.sin(2.0*np.pi*(1200 + p[:, 1:2] % 900)*t/8000.0)) + (z >> 10))
    idx, p, z = rows("small")
    out[idx] = (u[idx] & 15) - 8
    # an alternation at half the sample rate on a slow sine: the pole pair of a predictor at both ends of the real axis
    idx, p, z = rows("nyquist_lf")
    alt = np.where(ti % 2 == 0, 1.0, -1.0)*(2000.0 + p[:, :1] % 8000)
    out[idx] = _i16(alt + (4000.0 + p[:, 1:2] % 16000)*np.sin(2.0*np.pi*t/(50 + p[:, 2:3] % 200)))
    return out


def random_bytes(n, count, seed=SEED):
    return (Lcg(seeds_of(n, seed, 1)).u16(count) & 0xFF).astype(np.uint8)


def random_gsm_codes(packings, units, seed=SEED):
    """[n][units*76] bytes no encoder made: any bytes, but for the unpacked lines, masked to the parameters' widths (wider ones
    are undefined in the reference)"""
    b = random_bytes(len(packings), units*76, seed + 1)
    mask = np.tile((1 << np.array(GS.WIDTHS)) - 1, units).astype(np.uint8)
    b[np.asarray(packings) == GS.NONE] &= mask
    return b


def configs(family, n):
    """[n][...] the configuration of every line: consecutive lines cycle the family's list"""
    table = {"g726": G6.CONFIGS, "g722": G2.CONFIGS, "gsm0610": tuple((p,) for p in GS.PACKINGS)}[family]
    return np.array([table[i % len(table)] for i in range(n)], np.int32)


# ---- schedules -----------------------------------------------------------------------------------------------------------

def schedule_lengths(n, calls, seed, most=250, even=None):
    """[calls][n] lengths for the G.726 and G.722 banks: an eighth of the calls a line sits out (0), a quarter are 1 .. 16 items
    (every packing residue), the rest 1 .. most; never in step across a wave.  even[i]: line i takes pairs (a 16 kHz G.722
    encoder)."""
    r = Lcg(seeds_of(n, seed, 2)).u16(2*calls)
    kind, size = r[:, :calls] % 8, r[:, calls:]
    lens = np.where(kind == 0, 0, np.where(kind <= 2, 1 + size % 16, 1 + size % most))
    if even is not None:
        lens = np.where(np.asarray(even, bool)[:, None], lens & ~1, lens)
    return np.ascontiguousarray(lens.T.astype(np.int32))


def schedule_gsm(packings, calls, seed):
    """[calls][n] units a call: 0 (an eighth of the calls) .. 3, under WAV49 0 .. 2 (a unit is two frames there)"""
    packings = np.asarray(packings)
    r = Lcg(seeds_of(len(packings), seed, 3)).u16(2*calls)
    kind, size = r[:, :calls] % 8, r[:, calls:]
    units = np.where(kind == 0, 0, 1 + size % np.where(packings == GS.WAV49, 2, 3)[:, None])
    return np.ascontiguousarray(units.T.astype(np.int32))


def cut(avail, lens):
    """lens [calls][n] held to what a line has: where a line's lengths add up to more than avail[i] items, they shrink in
    proportion (the calls' ends move to floor(end*avail/total)), so that no line runs dry before the last call"""
    ends = np.cumsum(lens.astype(np.int64), axis=0)
    total = np.maximum(ends[-1], 1)
    avail = np.minimum(np.asarray(avail, np.int64), ends[-1])
    ends = ends*avail[None, :]//total[None, :]
    return np.diff(ends, axis=0, prepend=0).astype(np.int32)


def schedule_plc(n, calls, seed):
    """(lens [calls][n], lost [calls][n]).  Lengths: three quarters 160, a sixteenth 0 (the line sits the call out), the rest
    1 .. 320 with short ones favoured.  Gaps last 1 .. 6 calls; how many lanes of a wave start one is governed per (wave, call)
    by a density that is 0, 1/64, 1/8 or 3/4, so that a wave's call has no starting lane, a lone one, a few or most."""
    r = Lcg(seeds_of(n, seed, 4)).u16(4*calls).reshape(n, 4, calls)
    waves = (n + WAVE - 1)//WAVE
    d = Lcg(seeds_of(waves, seed, 5)).u16(calls) % 8
    density = np.choose(d, [0, 1024, 1024, 8192, 8192, 8192, 49152, 49152])         # of 65536
    lens = np.where(r[:, 0] % 16 == 0, 0, np.where(r[:, 0] % 4 != 1, 160, np.where(r[:, 1] % 2 == 0, 1 + r[:, 2] % 30, 1 + r[:, 2] % 320)))
    lost = np.zeros((n, calls), np.int32)
    left = np.zeros(n, np.int64)
    wave_of = np.arange(n)//WAVE
    for k in range(calls):
        start = (left == 0) & (r[:, 3, k] < density[wave_of, k])
        left = np.where(start, 1 + r[:, 1, k] % 6, left)
        lost[:, k] = left > 0
        left = np.maximum(left - 1, 0)
    return np.ascontiguousarray(lens.T.astype(np.int32)), np.ascontiguousarray(lost.T)


def probes(n):
    """the lines whose state words are compared after every call: c % 61 == 0 and each wave's first and last lane"""
    c = np.arange(n)
    return np.flatnonzero((c % 61 == 0) | (c % WAVE == 0) | (c % WAVE == WAVE - 1) | (c == n - 1))


# ---- what the reference reached ------------------------------------------------------------------------------------------

def coverage_g726(cfgs, codes, words):
    """cfgs [n][3]; codes[i]: the encoder's output bytes of an UNPACKED line (None for the others); words [n][calls][30]"""
    c = {"codes": {}, "td_set_and_cleared": 0, "yu_min": 0, "yu_max": 0, "a1_clamp": set(), "waves_mixed": True}
    for rate in G6.RATES:
        c["codes"][rate] = set()
    for i, (rate, coding, packing) in enumerate(cfgs.tolist()):
        if packing == G6.PACK_NONE:
            c["codes"][rate] |= set(np.unique(codes[i]).tolist())
        w = words[i]
        td = w[:, 23]
        on = np.flatnonzero(td == 1)
        c["td_set_and_cleared"] += bool(len(on) and (td[on[0]:] == 0).any())
        c["yu_min"] += bool((w[1:, 1] == 544).any())
        c["yu_max"] += bool((w[:, 1] == 5120).any())
        c["a1_clamp"] |= {int(v) for v in (12288, -12288) if (w[:, 6] == v).any()}
    n = len(cfgs)
    for w0 in range(0, n - WAVE + 1, WAVE):
        part = cfgs[w0:w0 + WAVE]
        c["waves_mixed"] = c["waves_mixed"] and len(set(part[:, 1])) == 3 and len(set(part[:, 2])) == 3 and len(set(part[:, 0])) == 4
    return c


def coverage_g722(cfgs, codes, pcm, words):
    """codes[i]: the encoder's bytes of a line whose stream is one code a byte (None for packed 48000 / 56000 lines); pcm[i]:
    the decoder's samples; words [n][calls][74] of the encoder"""
    c = {"low": {r: set() for r in G2.RATES}, "high": set(), "rails": set(), "nb_low": set()}
    for i, (rate, eight_k, packed) in enumerate(cfgs.tolist()):
        if codes[i] is not None:
            bits = G2.bits_of(rate)
            v = np.unique(codes[i]).astype(np.int64)
            c["low"][rate] |= set((v & ((1 << (bits - 2)) - 1)).tolist())
            c["high"] |= set(((v >> (bits - 2)) & 3).tolist())
        c["rails"] |= {int(v) for v in (32767, -32768) if (pcm[i] == v).any()}
        nb = words[i][:, G2.W_BAND0]
        c["nb_low"] |= {int(v) for v in (0, 18432) if (nb == v).any()}
    return c


LAR_MIC = (-32, -32, -16, -16, -8, -8, -4, -4)         # GSM 06.10 table 5.1: LARc[i] is coded 0 .. MAC - MIC
LAR_MAC = (31, 31, 15, 15, 7, 7, 3, 3)


def coverage_gsm0610(packings, pcm_in, lens, codes, words, rnd_codes):
    """codes[i]: the encoder's bytes (read where the line is unpacked); words [n][calls][160] of the encoder; rnd_codes[i]: the
    random bytes a decoder took (read where unpacked); pcm_in/lens: what went in, for the frame of zeros"""
    sub, lar, rnd = [], [], []
    for i, p in enumerate(np.asarray(packings).tolist()):
        if p == GS.NONE:
            f = GS.params_of(codes[i])
            lar.append(f[:, :8])
            sub.append(f[:, 8:].reshape(-1, 17))
            rnd.append(GS.params_of(rnd_codes[i])[:, 8:].reshape(-1, 17))
    sub, lar, rnd = np.concatenate(sub), np.concatenate(lar), np.concatenate(rnd)
    took = lens.sum(axis=0)
    zero = False
    for i in np.flatnonzero(family_of(np.arange(len(took))) == FAMILIES.index("bursts")):
        fr = pcm_in[i, :took[i] - took[i] % 160].reshape(-1, 160)
        zero = zero or bool((~fr.any(axis=1)).any())
    lz2 = words[:, :, GS.W_LZ2]
    return {"Nc": set(sub[:, GS.P_NC].tolist()), "bc": set(sub[:, GS.P_BC].tolist()), "Mc": set(sub[:, GS.P_MC].tolist()),
            "xmaxc": set(sub[:, GS.P_XMAXC].tolist()), "xMc": set(sub[:, GS.P_XMC:].reshape(-1).tolist()),
            "zero_frame": zero, "rnd_lags_out": int(np.count_nonzero((rnd[:, GS.P_NC] < 40) | (rnd[:, GS.P_NC] > 120))),
            "L_z2_wide": int(np.count_nonzero(np.abs(lz2.astype(np.int64)) > 32767)),
            "LARc_min": tuple(int(lar[:, k].min()) for k in range(8)), "LARc_max": tuple(int(lar[:, k].max()) for k in range(8))}


_LAG_INDEX = (np.arange(PL.LAG_FIRST, PL.LAG_LAST + 1)[:, None] + np.arange(PL.SPAN)[None, :])


def lag_sums(w):
    """the 81 sums of the pitch search on a line's words (plc_lines.lag_sums, in one step)"""
    a = PL.time_order(w)
    return np.abs(a[_LAG_INDEX] - a[None, :PL.SPAN]).sum(axis=1)


def coverage_plc_new(n, calls):
    return {"pitches": set(), "tied_searches": 0, "lowest_wins": True, "rails": set(), "cross_401": 0, "short_heard_after_gap": 0,
            "start_off_zero": 0, "starts": np.zeros(((n + WAVE - 1)//WAVE, calls), np.int32)}


def coverage_plc_line(c, i, lens, lost, rows_out, words):
    """line i into c: lens, lost [calls]; rows_out: the line's rows after their calls, one behind the other; words [calls][404]"""
    zero = np.zeros(PL.WORDS, np.int32)
    at = 0
    for k in range(len(lens)):
        ln = int(lens[k])
        if ln == 0:
            continue
        prev = words[k - 1] if k else zero
        w = words[k]
        m0 = int(prev[PL.W_MISSING])
        out = rows_out[at:at + ln]
        at += ln
        if lost[k]:
            if m0 == 0:
                c["starts"][i//WAVE, k] += 1
                c["pitches"].add(int(w[PL.W_PITCH]))
                c["start_off_zero"] += int(prev[PL.W_BUF_PTR]) != 0
                sums = lag_sums(prev)
                tied = np.flatnonzero(sums == sums.min()) + PL.LAG_FIRST
                c["tied_searches"] += len(tied) > 1
                c["lowest_wins"] = c["lowest_wins"] and int(w[PL.W_PITCH]) == int(tied[0])
            c["rails"] |= {int(v) for v in (32767, -32768) if (out == v).any()}
            c["cross_401"] += 0 < m0 < 401 < m0 + ln
        else:
            c["short_heard_after_gap"] += m0 > 0 and ln < (int(prev[PL.W_PITCH]) >> 2)


# ---- the sweeps: what goes in, and what the reference makes of it ----------------------------------------------------------
# Each sweep_*() returns a dict: "cfgs", "data" (per line, the items going in, one call behind the other), "lens" [calls][n],
# and from the reference "out" (per line, the items coming out), "counts" [calls][n], "final" [n][W] the words after the last
# call, "words" (per line, {call: the words after it}: every call of a probe line -- of all lines with every_all --, and on any
# line the calls it sits out and the last).

SAMPLES = 4096
G726_CALLS, G722_CALLS, GSM_CALLS, PLC_CALLS, CHAIN_TICKS = 8, 8, 6, 24, 16
MOST = 400                          # the longest call of a G.726 or G.722 line: about 1 000 items a line over 8 calls


def _ref():
    from oracle import ref_codecs
    return ref_codecs


def wanted(lens, every_all=False):
    """[calls][n]: the calls after which a line's words are compared"""
    calls, n = lens.shape
    want = lens == 0
    want[-1] = True
    want[:, np.arange(n) if every_all else probes(n)] = True
    return want


def _run_lines(fn, lens, every_all):
    """fn(i, mask) -> (out, counts, words) for every line"""
    want = wanted(lens, every_all)
    outs, counts, final, words = [], [], [], []
    for i in range(lens.shape[1]):
        o, c, w = fn(i, want[:, i])
        outs.append(o)
        counts.append(c)
        words.append(dict(zip(np.flatnonzero(want[:, i]).tolist(), w)))
        final.append(w[-1])
    return {"out": outs, "counts": np.ascontiguousarray(np.array(counts, np.int32).T), "final": np.array(final, np.int32), "words": words,
            "want": want}


def sweep_g726(kind, n=N_GPU, seed=SEED, every_all=False, calls=G726_CALLS, ref=True, samples=SAMPLES):
    R = _ref()
    cfgs = configs("g726", n)
    pcm = lines(n, samples, seed)
    enc_lens = schedule_lengths(n, calls, seed, MOST)
    assert int(enc_lens.sum(axis=0).max()) <= samples
    rows = [G6.pcm_row(pcm[i, :int(enc_lens[:, i].sum())], int(cfgs[i, 1])) for i in range(n)]
    if kind == G6.ENCODE:
        data, lens = rows, enc_lens
    else:
        # odd lines: the reference encoder's codes, cut into calls of their own; even lines: any bytes
        noise = random_bytes(n, MOST//2*calls, seed)
        data = [R.run_g726(G6.ENCODE, *cfgs[i].tolist(), rows[i], enc_lens[:, i])[0] if i & 1 else noise[i] for i in range(n)]
        lens = cut([len(d) for d in data], schedule_lengths(n, calls, seed + 1, MOST//2))
        data = [d[:int(lens[:, i].sum())] for i, d in enumerate(data)]
    r = _run_lines(lambda i, m: R.run_g726(kind, *cfgs[i].tolist(), data[i], lens[:, i], want=m), lens, every_all) if ref else {}
    r.update(cfgs=cfgs, data=data, lens=lens, family="g726", kind=kind, seed=seed)
    return r


def sweep_g722(kind, n=N_GPU, seed=SEED, every_all=False, calls=G722_CALLS, ref=True, samples=SAMPLES):
    R = _ref()
    cfgs = configs("g722", n)
    opts = [G2.options_of(int(e), int(p)) for _, e, p in cfgs]
    pcm = lines(n, samples, seed)
    enc_lens = schedule_lengths(n, calls, seed + 2, MOST, even=cfgs[:, 1] == 0)
    assert int(enc_lens.sum(axis=0).max()) <= samples
    rows = [pcm[i, :int(enc_lens[:, i].sum())] for i in range(n)]
    if kind == G2.ENCODE:
        data, lens = rows, enc_lens
    else:
        noise = random_bytes(n, MOST//2*calls, seed + 2)
        data = [R.run_g722(G2.ENCODE, int(cfgs[i, 0]), opts[i], rows[i], enc_lens[:, i])[0] if i & 1 else noise[i] for i in range(n)]
        lens = cut([len(d) for d in data], schedule_lengths(n, calls, seed + 3, MOST//2))
        data = [d[:int(lens[:, i].sum())] for i, d in enumerate(data)]
    r = _run_lines(lambda i, m: R.run_g722(kind, int(cfgs[i, 0]), opts[i], data[i], lens[:, i], want=m), lens, every_all) if ref else {}
    r.update(cfgs=cfgs, data=data, lens=lens, family="g722", kind=kind, seed=seed)
    return r


def sweep_gsm0610(kind, n=N_GPU, seed=SEED, every_all=False, calls=GSM_CALLS, ref=True, samples=SAMPLES):
    R = _ref()
    cfgs = configs("gsm0610", n)
    packings = cfgs[:, 0]
    pcm = lines(n, samples, seed)
    units = schedule_gsm(packings, calls, seed)
    unit_in = np.array([GS.unit_samples(p) for p in packings.tolist()])
    unit_bytes = np.array([GS.unit_bytes(p) for p in packings.tolist()])
    enc_lens = (units*unit_in[None, :]).astype(np.int32)
    assert int(enc_lens.sum(axis=0).max()) <= samples
    rows = [pcm[i, :int(enc_lens[:, i].sum())] for i in range(n)]
    if kind == GS.ENCODE:
        data, lens = rows, enc_lens
    else:
        # odd lines: the reference encoder's codes in calls of other sizes; even lines: random codes
        other = schedule_gsm(packings, calls, seed + 1)
        noise = random_gsm_codes(packings, 3*calls, seed)
        data = [R.run_gsm0610(GS.ENCODE, int(packings[i]), rows[i], enc_lens[:, i])[0] if i & 1 else noise[i] for i in range(n)]
        lens = (cut([len(d)//unit_bytes[i] for i, d in enumerate(data)], other)*unit_bytes[None, :]).astype(np.int32)
        data = [d[:int(lens[:, i].sum())] for i, d in enumerate(data)]
    r = _run_lines(lambda i, m: R.run_gsm0610(kind, int(packings[i]), data[i], lens[:, i], want=m), lens, every_all) if ref else {}
    r.update(cfgs=cfgs, data=data, lens=lens, family="gsm0610", kind=kind, seed=seed)
    return r


def plc_rows_in(line, lens, lost):
    """what each call of a line is given, one call behind the other: a heard call the line's samples at the stream's time (the
    line goes round), a lost one sentinels"""
    t = np.arange(int(lens.sum())) % len(line)
    out = line[t].copy()
    at = 0
    for ln, gone in zip(lens.tolist(), lost.tolist()):
        if gone:
            out[at:at + ln] = PL.SENTINEL
        at += ln
    return out


def sweep_plc(n=N_GPU, seed=SEED, every_all=False, calls=PLC_CALLS, ref=True, samples=SAMPLES):
    R = _ref()
    pcm = lines(n, samples, seed)
    lens, lost = schedule_plc(n, calls, seed)
    data = [plc_rows_in(pcm[i], lens[:, i], lost[:, i]) for i in range(n)]

    def one(i, m):
        out, w = R.run_plc(data[i], lens[:, i], lost[:, i], want=m)
        return out, lens[:, i], w

    r = _run_lines(one, lens, every_all) if ref else {}
    r.update(data=data, lens=lens, lost=lost, family="plc", seed=seed)
    return r


def sweep_chain(n=N_GPU, seed=SEED, every_all=False):
    """a VoIP decoder in front of a concealer for CHAIN_TICKS ticks: per tick a random subset of the lines brings nothing.
    "data": per line the frames of the ticks it brings one on, the reference encoder's; "out": [ticks][160] rows;
    "final"/"words": the concealer's words, "dec_final"/"dec_words": the decoder's."""
    R = _ref()
    pcm = lines(n, SAMPLES, seed)
    _, lost = schedule_plc(n, CHAIN_TICKS, seed + 7)
    heard = (lost == 0).sum(axis=0)
    data = [R.run_gsm0610(GS.ENCODE, GS.VOIP, pcm[i, :160*int(heard[i])], [160*int(heard[i])])[0] for i in range(n)]
    want = wanted(np.ones_like(lost), every_all)
    r = {"out": [], "final": [], "words": [], "dec_final": [], "dec_words": [], "want": want}
    for i in range(n):
        out, dw, pw = R.run_gsm_plc(data[i], lost[:, i], want=want[:, i])
        ks = np.flatnonzero(want[:, i]).tolist()
        r["out"].append(out)
        r["words"].append(dict(zip(ks, pw)))
        r["dec_words"].append(dict(zip(ks, dw)))
        r["final"].append(pw[-1])
        r["dec_final"].append(dw[-1])
    r["final"], r["dec_final"] = np.array(r["final"], np.int32), np.array(r["dec_final"], np.int32)
    r.update(data=data, lost=lost, family="chain", seed=seed)
    return r


def all_words(r):
    """[n][calls][W] of a sweep made with every_all"""
    return np.array([[w[k] for k in range(r["want"].shape[0])] for w in r["words"]], np.int32)


FAMILY_CODE = {"g726": 0, "g722": 1, "gsm0610": 2, "plc": 3}


def write_sweep(path, sweeps):
    """the inputs of some sweeps as the stand-alone program reads them (tests/c_callers/codec_sweep_host.cpp); returns the
    records written"""
    records = 0
    with open(path, "wb") as f:
        f.write(np.array([0x53574550, sum(s["lens"].shape[1] for s in sweeps)], np.int32).tobytes())
        for s in sweeps:
            lens = s["lens"]
            calls, n = lens.shape
            lost = s.get("lost", np.zeros_like(lens))
            for i in range(n):
                cfg = (s["cfgs"][i].tolist() + [0, 0])[:3] if "cfgs" in s else [0, 0, 0]
                if s["family"] == "g722":
                    cfg = [cfg[0], G2.options_of(cfg[1], cfg[2]), 0]
                raw = np.ascontiguousarray(s["data"][i]).tobytes()
                f.write(np.array([FAMILY_CODE[s["family"]], s.get("kind", 0)] + cfg + [i, calls, len(raw)], np.int32).tobytes())
                f.write(np.ascontiguousarray(lens[:, i], np.int32).tobytes())
                f.write(np.ascontiguousarray(lost[:, i], np.int32).tobytes())
                f.write(raw + b"\0"*(-len(raw) % 4))
                records += 1
    return records
