"""The ADSI sweep without a GPU (tests/adsi_sweep.py; its GPU half is tests/test_adsi_sweep_gpu.py).

  * What the sweep's own inputs make the reference do, from the reference's messages, counts and state words alone: the
    corners of adsi_rx_put_bit(), adsi_tx_put_message() and adsi_tx() that the 1 061 lines of the GPU sweep reach.  The counts
    are floors at about half of what the generator reaches today (profiles/adsi_sweep.md), the sets are pinned exactly.
    Among them is the defect the sweep was written for: on the `fast` lines the reference delivers more messages in a call than
    spangpu_adsi_rx_msg_capacity() used to allow for.
  * The conditions the schedules keep: no call leaves a quarter of the lines out, no line is longer than keeps a GPU test to
    a few seconds.
  * The framers of csrc/adsi_frame.hpp compiled for the host into one stand-alone program (tests/c_callers/adsi_frame_host.cpp),
    built with the address and undefined-behaviour sanitizers and linked against the reference library, over ten times the GPU
    sweep's lines: every message, count and framer word after every call, the buffer at the end, every sender bit, put return
    and word equal what the reference, called by the same program on the same input, has.

All of it needs oracle/_ref/libspandsp_adsi_ref.so (oracle/Makefile builds it where the reference's sources are)."""
import os
import re
import subprocess
import time

import numpy as np
import pytest

import adsi_lines as AL
import adsi_sweep as S
from oracle import ref_adsi
from test_c_callers import REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (where the reference's sources are, a library that is missing is a build that failed, and the tests say so by failing)
pytestmark = pytest.mark.skipif(not ref_adsi.available() and not os.path.isdir(REF),
                                reason="oracle/_ref/libspandsp_adsi_ref.so is not built (no reference sources here)")

N = S.N_GPU
CHUNKS = 10                     # the host sweep: chunks of N receiver and N sender lines, each with a seed of its own


@pytest.fixture(autouse=True)
def adsi_ref():
    assert ref_adsi.available(), "the reference's sources are here, but `make -C oracle ref` has not made %s" % ref_adsi.ADSI_SO


@pytest.fixture(scope="module")
def rx():
    return S.sweep_rx()


@pytest.fixture(scope="module")
def tx():
    return S.sweep_tx()


def test_generator_is_deterministic_and_deals_every_family_to_every_wave():
    a = [S.rx_line(i, S.SEED) for i in range(36)]
    b = [S.rx_line(i, S.SEED) for i in range(36)]
    c = [S.rx_line(i, S.SEED + 1) for i in range(36)]
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not any(np.array_equal(x, y) for x, y in zip(a, c))
    assert S.tx_script(5) == S.tx_script(5) != S.tx_script(5, S.SEED + 1)
    assert len(set(S.FAMILIES)) == S.DEAL and np.gcd(S.DEAL, 4) == 1 and N == 16*S.WAVE + 37
    i = np.arange(N)
    pairs = S.family_of(i)*4 + i % 4
    # every family in every standard (more than one, that is) in any 64 consecutive lines
    assert all(len(set(pairs[w:w + 64].tolist())) == 4*S.DEAL for w in range(N - 64))
    assert [S.standard_of(c) for c in range(8)] == list(AL.STANDARDS)*2
    assert not S.PINNED


def test_messages_cover_every_length_edge():
    d = S.Draws(12345)
    for s in AL.STANDARDS:
        mask = 0x7F if s == AL.JCLIP else 0xFF
        assert len(S.message(d, s, "none")) == 2
        e = S.message(d, s, "empty")
        assert len(e) == 4 and e[3] == 0
        assert len(S.message(d, s, "longest")) == S.LONGEST[s] and S.packed(s, S.message(d, s, "longest")) != -1
        assert len(S.message(d, s, "over")) == S.LONGEST[s] + 1
        from spandsp_amd import engine
        assert engine.adsi_pack_message(s, S.message(d, s, "over")) == -1
        six = S.message(d, s, "sixteen")
        p = S.packed(s, six)
        assert 0x10 in six and len(p) > 16 + 3
        assert AL.DLE in S.message(d, s, "dle")
        assert all(b <= mask for b in S.message(d, s, "fields")[:1])
    # J-CLIP's stuffed length byte: a message whose length less 2 is 0x10 has it doubled on the line
    m = bytes([0x40, 0]) + bytes(range(0x20, 0x30))
    assert len(m) - 2 == 0x10 and [b & 0x7F for b in S.packed(AL.JCLIP, m)[6:8]] == [0x10, 0x10]


def test_no_call_leaves_a_quarter_of_the_lines_out_and_no_line_is_long():
    lens = S.rx_schedule(N)
    assert lens.shape == (S.RX_CALLS, N)
    assert 0 < S.left_out(lens) < 0.25, S.left_out(lens)
    # never in step across a wave
    assert all(len(set(lens[k, w:w + S.WAVE].tolist())) > 16 for k in range(len(lens)) for w in range(0, N - S.WAVE, S.WAVE))
    share = [(lens == 0).mean(), ((lens >= 1) & (lens <= 16)).mean()]
    assert 0.11 < share[0] < 0.14 and 0.25 < share[1] < 0.28 and lens.max() == 1024 and lens.min() == 0, share
    # a line is at most 64 calls of 1 024 samples, 128 ticks or 60 sender calls of 400: seconds of line, a few launches each
    assert lens.sum(axis=0).max() <= 40000 and S.RX_TICKS*S.TICK <= 20480 and S.TX_CALLS <= 60
    t = S.tx_schedule()
    assert len(t) == S.TX_CALLS and 1 <= t.min() and t.max() <= 400 and set((np.cumsum(t) % 8).tolist()) == set(range(8))


def test_coverage_receivers(rx):
    c = S.coverage_rx(rx)
    print("receiver coverage:", c)
    assert all(c["delivered"][s] >= v for s, v in ((AL.CLASS, 2700), (AL.CLIP, 2700), (AL.ACLIP, 2500), (AL.JCLIP, 750))), c["delivered"]
    # a sum failure and a CRC failure: the line's first message is lost, the good one right behind it arrives
    assert c["bad_check"][False] >= 9 and c["bad_check"][True] >= 3, c["bad_check"]
    assert c["framing_error_lines"] >= 220
    # a restart by 11 marks (and by 12), and none by 10 (or by 9)
    marks = c["marks"]
    assert marks.get((11, 1), 0) >= 2 and marks.get((12, 1), 0) >= 4 and marks.get((10, 2), 0) >= 4 and marks.get((9, 2), 0) >= 3, marks
    assert not any(marks.get(k, 0) for k in ((11, 2), (12, 2), (10, 1), (9, 1))), marks
    assert c["len_256_lines"] >= 4
    assert c["multi_calls"] >= 2000 and c["most"] >= 7
    # the defect: calls in which the reference delivers more than samples*1200/240000 + 1 messages
    assert c["over_old_capacity"] >= 300, c["over_old_capacity"]
    reach = c["fast_reach"]
    print("fast family, reached k of cap: " + ", ".join("%d of %d" % (reach[k], k) for k in sorted(reach)))
    assert reach[2] == 2 and reach[9] >= 7
    # on plain ticks of 160 samples too: two messages where the old capacity said one
    t = S.coverage_rx(S.sweep_rx(ticks=True))
    print("receiver coverage on ticks:", t)
    assert t["over_old_capacity"] >= 90 and t["most"] == 2 and t["len_256_lines"] >= 4


def test_coverage_senders(tx):
    c = S.coverage_tx(tx)
    print("sender coverage:", c)
    assert c["put"][0] >= 1900 and c["put"][-1] >= 360 and c["put"][1] >= 1400, c["put"]
    assert c["refused_restarts"] >= 320 and c["restarts"] >= 88
    assert c["part_tone_part_modem"] >= 570 and c["tone_in_message"] >= 590 and c["off_on_empty_call"] >= 40
    assert c["off_by_the_rule_alone"] >= 90
    assert c["tone_ends_mod_8"] == set(range(8))
    assert c["preamble_signs"] == {(j, s) for j in range(4) for s in (-1, 0, 1)}


def frames_on_the_host(tmp_path, source=None, chunks=CHUNKS):
    """builds the program (from `source`: a copy of the tree's, for the mutation checks) and runs every chunk; the outputs"""
    exe = os.path.join(str(tmp_path), "adsi_frame_host")
    ref_dir = os.path.dirname(ref_adsi.ADSI_SO)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           source or os.path.join(ROOT, "tests", "c_callers", "adsi_frame_host.cpp"), "-o", exe, "-L" + ref_dir, "-lspandsp_adsi_ref",
           "-Wl,-rpath," + ref_dir]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    running, outs = [], []
    jobs = max(1, min(8, os.cpu_count() or 1))

    def collect(entry):
        proc, path = entry
        out, _ = proc.communicate()
        os.remove(path)
        outs.append(out)
        assert proc.returncode == 0 and "Sanitizer" not in out and "runtime error" not in out, out[-3000:]

    for chunk in range(chunks):
        seed = S.SEED + 1000*chunk
        path = os.path.join(str(tmp_path), "sweep%d.bin" % chunk)
        assert S.write_sweep(path, S.rx_lines(N, seed), S.sweep_tx(N, seed, ref=False)) == 2*N
        while len(running) >= jobs:
            collect(running.pop(0))
        running.append((subprocess.Popen([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), path))
    while running:
        collect(running.pop(0))
    return outs


def test_framers_against_the_reference_under_sanitizers(tmp_path):
    t0 = time.time()
    outs = frames_on_the_host(tmp_path)
    done = {"rx": [0, 0, 0], "tx": [0, 0, 0]}
    reach = (0, 1)
    for out in outs:
        assert re.search(r"^ok \d+ lines$", out, re.M), out[-3000:]
        for f, a, b, c in re.findall(r"^(\w+): (\d+) lines, (\d+) calls, (\d+) items$", out, re.M):
            done[f] = [x + int(y) for x, y in zip(done[f], (a, b, c))]
        m = re.search(r"fullest record: (\d+) of (\d+)", out)
        mine, best = int(m.group(1))*reach[1], reach[0]*int(m.group(2))
        if mine > best or (mine == best and int(m.group(1)) > reach[0]):
            reach = (int(m.group(1)), int(m.group(2)))
    print("ADSI framers on the host: lines, calls, items %s; fullest record %d of %d; %.1f s" % (done, reach[0], reach[1], time.time() - t0))
    assert done["rx"][0] == done["tx"][0] == CHUNKS*N >= 10000
    # a record filled to its capacity: the bound is reached, at a capacity above 1
    assert reach[0] == reach[1] >= 2
