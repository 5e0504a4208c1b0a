"""The codec sweep without a GPU (tests/codec_sweep.py; its GPU half is tests/test_codec_sweep_gpu.py).

  * What the sweep's own inputs make the reference do, from the reference's outputs and state words alone: the corners of the
    G.726, G.722 and GSM 06.10 codecs and of the packet loss concealer that the lines, configurations and schedules reach on the
    4 133 lines of the GPU sweep.  The sets are pinned exactly, so that an edit of the generator cannot shrink them unseen; the
    counts are floors at about half of what the generator reaches today.
  * The kernels' per-sample, per-frame and per-line functions compiled for the host into one stand-alone program
    (tests/c_callers/codec_sweep_host.cpp), built with the address and undefined-behaviour sanitizers and linked against the
    reference library, over ten times the GPU sweep's lines: every output item, count and state word after every call equals
    what the reference, called by the same program on the same input, has.

All of it needs oracle/_ref/libspandsp_codecs_ref.so (oracle/Makefile builds it where the reference's sources are)."""
import os
import re
import subprocess
import time

import numpy as np
import pytest

import codec_sweep as S
import g722_lines as G2
import g726_lines as G6
import gsm0610_lines as GS
from oracle import ref_codecs
from test_c_callers import REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (where the reference's sources are, a library that is missing is a build that failed, and the tests say so by failing)
pytestmark = pytest.mark.skipif(not ref_codecs.available() and not os.path.isdir(REF),
                                reason="oracle/_ref/libspandsp_codecs_ref.so is not built (no reference sources here)")

N = S.N_GPU
# the CPU sweep: CHUNKS generations of N lines, each with a seed of its own; fewer calls a line than on the GPU
CHUNKS = 10
CPU_CALLS = {"g726": 3, "g722": 3, "gsm0610": 2, "plc": 8}
CPU_SAMPLES = 1536                  # a line of the CPU sweep: 3 calls of up to 400 items, 2 of up to 640


@pytest.fixture(autouse=True)
def codecs_ref():
    assert ref_codecs.available(), "the reference's sources are here, but `make -C oracle ref` has not made %s" % ref_codecs.CODECS_SO


def test_generator_is_deterministic_and_deals_every_family_to_every_wave():
    a = S._lines(200, 512, S.SEED)
    assert np.array_equal(a, S._lines(200, 512, S.SEED)) and not np.array_equal(a, S._lines(200, 512, S.SEED + 1))
    assert len(S.FAMILIES) <= S.WAVE and len(set(S.FAMILIES)) == len(S.FAMILIES)
    x = S.lines(N, S.SAMPLES)
    assert x.dtype == np.int16 and x.shape == (N, S.SAMPLES)
    # the rails, and lines that never leave zero's neighbourhood
    assert (x == -32768).any() and (x == 32767).any() and (np.abs(x.astype(np.int32)).max(axis=1) <= 8).any()
    for family, count in (("g726", 36), ("g722", 12), ("gsm0610", 3)):
        cfgs = S.configs(family, N)
        assert all(len({tuple(c) for c in cfgs[w:w + S.WAVE].tolist()}) == count for w in range(0, N, S.WAVE) if w + S.WAVE <= N)
    assert not S.PINNED


def left_out(lens):
    return float((lens == 0).mean(axis=1).max())


def test_coverage_g726():
    enc = S.sweep_g726(G6.ENCODE, every_all=True)
    dec = S.sweep_g726(G6.DECODE)
    c = S.coverage_g726(enc["cfgs"], enc["out"], S.all_words(enc))
    # every code an encoder can make: the all-zero code is one it never makes at 24, 32 and 40 kbit/s (the decoders take it
    # from the random bytes of the even lines)
    assert c["codes"] == {16000: set(range(4)), 24000: set(range(1, 8)), 32000: set(range(1, 16)), 40000: set(range(1, 32))}, c["codes"]
    assert c["td_set_and_cleared"] >= 340 and c["yu_min"] >= 670 and c["yu_max"] >= 160, c
    assert c["a1_clamp"] == {-12288, 12288}, c["a1_clamp"]
    assert c["waves_mixed"]
    rnd = np.concatenate([dec["data"][i] for i in range(0, N, 2) if enc["cfgs"][i, 2] == G6.PACK_NONE])
    assert set(np.unique(rnd).tolist()) == set(range(256))
    # lengths: some in every residue class of 8, a few long ones, and under a quarter of the lines out of any call
    assert 0 < left_out(enc["lens"]) < 0.25 and 0 < left_out(dec["lens"]) < 0.25
    assert {int(v) % 8 for v in np.unique(enc["lens"])} == set(range(8)) and enc["lens"].max() == S.MOST
    assert 900 <= enc["lens"].sum(axis=0).mean() <= 1100


def test_coverage_g722():
    enc = S.sweep_g722(G2.ENCODE, every_all=True)
    dec = S.sweep_g722(G2.DECODE)
    one_a_byte = [enc["out"][i] if (p == 0 or r == 64000) else None for i, (r, e, p) in enumerate(enc["cfgs"].tolist())]
    c = S.coverage_g722(enc["cfgs"], one_a_byte, dec["out"], S.all_words(enc))
    # every low-band code an encoder can make (the lowest 4, 2 and 1 of 64, 32 and 16 are never sent), every high-band code
    assert c["low"] == {48000: set(range(1, 16)), 56000: set(range(2, 32)), 64000: set(range(4, 64))}, c["low"]
    assert c["high"] == {0, 1, 2, 3}
    assert c["rails"] == {32767, -32768}
    assert c["nb_low"] == {0, 18432}
    assert {(int(e), int(p)) for _, e, p in enc["cfgs"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert 0 < left_out(enc["lens"]) < 0.25 and 0 < left_out(dec["lens"]) < 0.25
    # a 16 kHz encoder takes pairs; an 8 kHz one takes odd lengths too
    assert not (enc["lens"][:, enc["cfgs"][:, 1] == 0] & 1).any() and (enc["lens"][:, enc["cfgs"][:, 1] == 1] & 1).any()


def test_coverage_gsm0610():
    enc = S.sweep_gsm0610(GS.ENCODE, every_all=True)
    dec = S.sweep_gsm0610(GS.DECODE)
    c = S.coverage_gsm0610(enc["cfgs"][:, 0], S.lines(N, S.SAMPLES), enc["lens"], enc["out"], S.all_words(enc), dec["data"])
    assert c["Nc"] == set(range(40, 121)) and c["bc"] == {0, 1, 2, 3} and c["Mc"] == {0, 1, 2, 3}
    assert c["xmaxc"] == set(range(64)) and c["xMc"] == set(range(8))
    assert c["zero_frame"] and c["rnd_lags_out"] >= 5000 and c["L_z2_wide"] >= 11000, c
    # each LARc[i] at its MAC - MIC, and at 0 but for LARc[1], which these lines take no lower than 2
    assert c["LARc_max"] == tuple(mac - mic for mic, mac in zip(S.LAR_MIC, S.LAR_MAC)), c["LARc_max"]
    assert c["LARc_min"] == (0, 2, 0, 0, 0, 0, 0, 0), c["LARc_min"]
    assert 0 < left_out(enc["lens"]) < 0.25 and 0 < left_out(dec["lens"]) < 0.25
    units = enc["lens"]//np.array([GS.unit_samples(p) for p in enc["cfgs"][:, 0].tolist()])[None, :]
    assert set(np.unique(units).tolist()) == {0, 1, 2, 3}


def test_coverage_plc():
    r = S.sweep_plc(every_all=True)
    c = S.coverage_plc_new(N, S.PLC_CALLS)
    for i in range(N):
        S.coverage_plc_line(c, i, r["lens"][:, i], r["lost"][:, i], r["out"][i], r["words"][i])
    assert c["pitches"] == set(range(40, 121)), sorted(set(range(40, 121)) - c["pitches"])
    assert c["tied_searches"] >= 1400 and c["lowest_wins"], c["tied_searches"]
    assert c["rails"] == {32767, -32768}
    assert c["cross_401"] >= 3400 and c["short_heard_after_gap"] >= 330 and c["start_off_zero"] >= 5000, c
    # per wave and call, the lanes whose gap starts: none, a lone one, at least half a wave
    starts = c["starts"][:N//S.WAVE]
    assert (starts == 0).sum() >= 180 and (starts == 1).sum() >= 110 and (starts >= 32).sum() >= 60, starts
    assert 0 < left_out(r["lens"]) < 0.25
    assert (r["lens"] == 160).mean() > 0.5 and r["lens"].max() == 320 and r["lens"][r["lens"] > 0].min() == 1


def test_step_functions_against_the_reference_under_sanitizers(tmp_path):
    exe = os.path.join(str(tmp_path), "codec_sweep_host")
    ref_dir = os.path.dirname(ref_codecs.CODECS_SO)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           os.path.join(ROOT, "tests", "c_callers", "codec_sweep_host.cpp"), "-o", exe, "-L" + ref_dir, "-lspandsp_codecs_ref",
           "-Wl,-rpath," + ref_dir]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    t0 = time.time()
    running, outs = [], []
    jobs = max(1, min(8, os.cpu_count() or 1))

    def collect(proc):
        out, _ = proc.communicate()
        outs.append(out)
        assert proc.returncode == 0 and "Sanitizer" not in out and "runtime error" not in out, out[-3000:]

    for chunk in range(CHUNKS):
        seed = S.SEED + 1000*chunk
        sweeps = [S.sweep_g726(G6.ENCODE, N, seed, calls=CPU_CALLS["g726"], ref=False, samples=CPU_SAMPLES), S.sweep_g726(G6.DECODE, N, seed, calls=CPU_CALLS["g726"], ref=False, samples=CPU_SAMPLES),
                  S.sweep_g722(G2.ENCODE, N, seed, calls=CPU_CALLS["g722"], ref=False, samples=CPU_SAMPLES), S.sweep_g722(G2.DECODE, N, seed, calls=CPU_CALLS["g722"], ref=False, samples=CPU_SAMPLES),
                  S.sweep_gsm0610(GS.ENCODE, N, seed, calls=CPU_CALLS["gsm0610"], ref=False, samples=CPU_SAMPLES),
                  S.sweep_gsm0610(GS.DECODE, N, seed, calls=CPU_CALLS["gsm0610"], ref=False, samples=CPU_SAMPLES), S.sweep_plc(N, seed, calls=CPU_CALLS["plc"], ref=False, samples=CPU_SAMPLES)]
        path = os.path.join(str(tmp_path), "sweep%d.bin" % chunk)
        assert S.write_sweep(path, sweeps) == 7*N
        while len(running) >= jobs:
            collect(running.pop(0))
        running.append(subprocess.Popen([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    while running:
        collect(running.pop(0))
    for path in os.listdir(str(tmp_path)):
        if path.endswith(".bin"):
            os.remove(os.path.join(str(tmp_path), path))
    lines_done = {f: 0 for f in S.FAMILY_CODE}
    items = dict(lines_done)
    searches = tied = 0
    for out in outs:
        assert "ok %d lines" % (7*N) in out, out[-3000:]
        for f, a, b in re.findall(r"^(\w+): (\d+) lines, \d+ calls, (\d+) items$", out, re.M):
            lines_done[f] += int(a)
            items[f] += int(b)
        m = re.search(r"searches: (\d+), with tied lags (\d+)", out)
        searches, tied = searches + int(m.group(1)), tied + int(m.group(2))
    print("codec sweep on the host: %s lines, %s items, %d searches (%d tied), %.1f s" % (lines_done, items, searches, tied, time.time() - t0))
    # ten times the GPU sweep's lines in every family (the codecs have an encoder and a decoder sweep each)
    assert lines_done == {"g726": 2*CHUNKS*N, "g722": 2*CHUNKS*N, "gsm0610": 2*CHUNKS*N, "plc": CHUNKS*N}
    assert CHUNKS >= 10 and searches >= 10000 and tied >= 1000
