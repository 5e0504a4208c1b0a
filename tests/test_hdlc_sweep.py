"""The HDLC sweep without a GPU (tests/hdlc_sweep.py; its GPU half is tests/test_hdlc_sweep_gpu.py).

  * What the sweep's own inputs make the reference do, from the reference's records and state words alone: the corners of
    hdlc_rx_put_bit(), hdlc_rx_put() and hdlc_tx_get_bit() that the lines, configurations and schedules reach on the 1 061
    lines of the GPU sweep.  The sets are pinned exactly, so that an edit of the generator cannot shrink them unseen; the counts
    are floors at about half of what the generator reaches today (profiles/hdlc_sweep.md).
  * The condition the schedules keep: no call leaves a quarter of the lines out.
  * The step functions of csrc/hdlc_dev.hpp compiled for the host into one stand-alone program
    (tests/c_callers/hdlc_sweep_host.cpp), built with the address and undefined-behaviour sanitizers and linked against the
    reference library, over forty times the GPU sweep's receiver lines and twenty times its sender lines: every record, octet,
    count, bit and state word after every call and the buffer at the end equal what the reference, called by the same program
    on the same input, has, and every call of the reference stays within hdlc_rx_capacity().

All of it needs oracle/_ref/libspandsp_hdlc_ref.so (oracle/Makefile builds it where the reference's sources are)."""
import os
import re
import subprocess
import time

import numpy as np
import pytest

import hdlc_sweep as H
from oracle import ref_hdlc
from test_c_callers import REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (where the reference's sources are, a library that is missing is a build that failed, and the tests say so by failing)
pytestmark = pytest.mark.skipif(not ref_hdlc.available() and not os.path.isdir(REF),
                                reason="oracle/_ref/libspandsp_hdlc_ref.so is not built (no reference sources here)")

N = H.N_GPU
# the CPU sweep: chunks of N lines, each with a seed of its own
RX_CHUNKS, OCTET_CHUNKS, TX_CHUNKS = 40, 8, 20


@pytest.fixture(autouse=True)
def hdlc_ref():
    assert ref_hdlc.available(), "the reference's sources are here, but `make -C oracle ref` has not made %s" % ref_hdlc.HDLC_SO


def test_generator_is_deterministic_and_deals_every_family_to_every_wave():
    a, _ = H.rx_lines(64, H.SEED, sent=lambda i: np.ones(100, np.int16))
    b, _ = H.rx_lines(64, H.SEED, sent=lambda i: np.ones(100, np.int16))
    c, _ = H.rx_lines(64, H.SEED + 1, sent=lambda i: np.ones(100, np.int16))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not all(np.array_equal(x, y) for x, y in zip(a, c))
    assert all(len(x) >= H.EVENTS >= 6000 for x in a)
    assert len(set(H.FAMILIES)) == H.DEAL <= H.WAVE and np.gcd(H.DEAL, 288) == 1
    fam = H.family_of(np.arange(N))
    assert all(set(fam[w:w + 64].tolist()) == set(range(H.DEAL)) for w in range(N - 64))
    cfgs = H.rx_configs(N)
    for w in range(0, N - H.WAVE + 1, H.WAVE):
        part = cfgs[w:w + H.WAVE]
        assert set(part[:, 0]) == {0, 1} and set(part[:, 1]) == {0, 1} and len(set(part[:, 2])) >= 4 and set(part[:, 4]) == {0, 1, 2, 20}
    assert set(cfgs[:, 2]) == {1, 2, 3, 4, 5, 6} and 0.25 < (cfgs[:, 3] >= 0).mean() < 0.45
    t = H.tx_lines(N)[0]
    assert set(t[:, 0]) == {0, 1} and set(t[:, 1]) == {1, 2, 3, 4, 5} and set(t[:, 2]) == set(range(1, 9)) and (t[:, 3] >= 2).any()
    assert not H.PINNED


def test_no_call_leaves_a_quarter_of_the_lines_out():
    """the schedules' condition: in every call of every sweep at least three quarters of the lines take part (and some do not),
    with lengths never in step across a wave"""
    for form in ("int16", "int8", "octets"):
        lens = H.sweep_rx(form=form, ref=False)["lens"]
        assert 0 < H.left_out(lens) < 0.25, (form, H.left_out(lens))
        assert all(len(set(lens[k, w:w + H.WAVE].tolist())) > 16 for k in range(len(lens)) for w in range(0, N - H.WAVE, H.WAVE)), form
    lens = H.sweep_rx(ref=False)["lens"]
    assert lens.max() > 1000 and {1, 2, 7, 8, 9, 16} <= set(np.unique(lens).tolist())
    assert H.sweep_rx(form="octets", ref=False)["lens"].max() == 128
    wants = H.sweep_tx(ref=False)["wants"]
    assert 0 < H.left_out(wants) < 0.25 and wants.max() == 600 and set(range(17)) <= set(np.unique(wants).tolist())


def test_coverage_receivers():
    r = H.sweep_rx(every_all=True)
    c = H.coverage_rx(r)
    print("receiver coverage:", {k: v for k, v in c.items() if k != "good"})
    # every report a receiver can make: carrier down and up, training in progress, succeeded and failed, framing OK, end of
    # data, abort, octet report
    assert c["statuses"] == {-1, -2, -3, -4, -5, -6, -7, -8, -11}, c["statuses"]
    # good frames at every length edge on the wire: crc_bytes (a frame of no octets), crc_bytes + 1, 399 .. 404
    assert {0, 1} | set(range(397, 403)) <= c["good"][2] and {0, 1} | set(range(395, 401)) <= c["good"][4], c["good"]
    assert max(c["good"][2]) == 402 and max(c["good"][4]) == 400
    # bad frames of the three kinds: the CRC, the length (below the CRC's size), a flag out of step with the octets
    assert c["bad_crc"] >= 50 and c["bad_short"] >= 170 and c["bad_misaligned"] >= 80, c
    assert c["crc_error_lines"] >= 160 and c["length_error_lines"] >= 210, c
    assert c["len_0"] >= 6000 and c["len_405"] >= 1000, c
    assert c["counting_by_abort"] >= 400 and c["counting_by_overlong"] >= 170, c
    # the capacities: every call of every line within them, and the lines aimed at them come close
    for form in ("int16", "int8", "octets"):
        q = r if form == "int16" else H.sweep_rx(form=form)
        ok, recs, octets = H.within_capacity(q)
        print("capacity, %s: records to %.3f, octets to %.3f" % (form, recs, octets))
        assert ok and octets > 0.98 and (recs == 1.0 or form == "octets"), (form, recs, octets)
    # mid-stream operations of each kind, ahead of calls with a length only
    mid = [o for i in range(N) for o in r["ops"][i] if o[0] >= 0]
    assert {o[1] for o in mid} == {H.OP_MAX_FRAME_LEN, H.OP_REPORT_INTERVAL, H.OP_RESTART} and len(mid) >= 150
    assert all(r["lens"][o[0], i] > 0 for i in range(N) for o in r["ops"][i] if o[0] >= 0)


def test_coverage_senders():
    r = H.sweep_tx(every_all=True)
    c = H.coverage_tx(r)
    print("sender coverage:", {k: v for k, v in c.items() if k not in ("frame_lens", "flag_counts")})
    # the stuffing's residue at a frame's end, and with it the rotation of the idle octet
    assert c["residues"] == set(range(8)), c["residues"]
    assert c["idle_octets"] == {(0x7E7E >> k) & 0xFF for k in range(8)}, c["idle_octets"]
    assert c["corrupt_after_shorter"] >= 400 and c["corrupt_after_longer"] >= 370, c
    # the underflow handler on an empty queue, and on a queue that holds each kind of command; the same between calls
    assert c["underflows_empty"] >= 2700, c
    assert all(c["taken_by_handler"][k] >= v for k, v in ((H.FRAME, 2100), (H.FLAGS, 800), (H.ABORT, 590), (H.END, 290))), c
    assert all(c["taken_between_calls"][k] >= v for k, v in ((H.FRAME, 4200), (H.FLAGS, 1200), (H.ABORT, 860), (H.END, 450))), c
    assert c["flag_counts"] == set(range(-5, 41)), c["flag_counts"]
    assert {1, 2, 3, 399, 400} <= c["frame_lens"] and max(c["frame_lens"]) == 400
    assert c["refused"] >= 7000 and c["refused_too_long"] >= 490 and c["ended"] >= 1000 and c["pos_400"] >= 650, c


def sweep_on_the_host(tmp_path, source=None):
    """builds the program (from `source`: a copy of the tree's, for the mutation checks) and runs every chunk; the outputs"""
    exe = os.path.join(str(tmp_path), "hdlc_sweep_host")
    ref_dir = os.path.dirname(ref_hdlc.HDLC_SO)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           source or os.path.join(ROOT, "tests", "c_callers", "hdlc_sweep_host.cpp"), "-o", exe, "-L" + ref_dir, "-lspandsp_hdlc_ref",
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

    for chunk in range(max(RX_CHUNKS, TX_CHUNKS)):
        seed = H.SEED + 1000*chunk
        sweeps = []
        if chunk < RX_CHUNKS:
            sweeps.append(H.sweep_rx(N, seed, ref=False))
        if chunk < OCTET_CHUNKS:
            sweeps.append(H.sweep_rx(N, seed, form="octets", ref=False))
        if chunk < TX_CHUNKS:
            sweeps.append(H.sweep_tx(N, seed, ref=False))
        path = os.path.join(str(tmp_path), "sweep%d.bin" % chunk)
        assert H.write_sweep(path, sweeps) == len(sweeps)*N
        while len(running) >= jobs:
            collect(running.pop(0))
        running.append((subprocess.Popen([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), path))
    while running:
        collect(running.pop(0))
    return outs


def test_step_functions_against_the_reference_under_sanitizers(tmp_path):
    t0 = time.time()
    outs = sweep_on_the_host(tmp_path)
    done = {"rx_events": [0, 0, 0], "rx_octets": [0, 0, 0], "tx": [0, 0, 0]}
    reach = [0, 0]
    for out in outs:
        assert re.search(r"^ok \d+ lines$", out, re.M), out[-3000:]
        for f, a, b, c in re.findall(r"^(\w+): (\d+) lines, (\d+) calls, (\d+) items$", out, re.M):
            done[f] = [x + int(y) for x, y in zip(done[f], (a, b, c))]
        m = re.search(r"capacity reached to (\d+) and (\d+) of 1000", out)
        reach = [max(reach[0], int(m.group(1))), max(reach[1], int(m.group(2)))]
    print("HDLC sweep on the host: lines, calls, items %s; capacity reached to %s of 1000; %.1f s" % (done, reach, time.time() - t0))
    assert done["rx_events"][0] == RX_CHUNKS*N and done["rx_octets"][0] == OCTET_CHUNKS*N and done["tx"][0] == TX_CHUNKS*N
    assert done["rx_events"][0] >= 40000 and done["tx"][0] >= 20000
    # the streams aimed at the capacities reach the record capacity exactly and come within a hundredth of the octets'
    assert reach[0] == 1000 and reach[1] >= 990
