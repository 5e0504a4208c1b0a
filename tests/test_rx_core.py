"""The pure parts of the receivers' shared host plumbing, on the host.

spandsp_amd/csrc/bank_host.hpp is the one place where the per-channel lengths of an _rx_var call are checked against
0..max_samples (the longest, and whether all are equal, decide what a bank family launches) and where a row of result counts
is scanned for the columns to bring back and for a count above the capacity; neither makes a GPU call, so
tests/c_callers/rx_core.cpp drives them over 1 .. 200 channels -- all-zero and all-equal lengths, one length out of range at
the first, a middle and the last channel, counts at, below and above the capacity -- under -fsanitize=address,undefined (host
code only, a program of its own).  The program checks itself and exits non-zero on a miss."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_rx_core_lengths_check_and_count_scan(tmp_path):
    exe = os.path.join(str(tmp_path), "rx_core")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include"), "-I" + os.path.join(ROOT, "spandsp_amd", "csrc"),
           os.path.join(ROOT, "tests", "c_callers", "rx_core.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    p = subprocess.run([exe], capture_output=True, text=True)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "cases: ok" in out and "Sanitizer" not in out and "runtime error" not in out, out
