"""The arithmetic of the sets of banks over several devices, on the host.

spandsp_amd/csrc/shard_core.hpp is the one place where the channels of a sharded tone, echo canceller or modem bank are dealt
over the devices and where a collecting slot is put back into the whole bank's channel order; it makes no GPU call, so
tests/c_callers/shard_deal.cpp drives it with 1 .. 64 shards and channel counts up to a few thousand -- ranges contiguous, at
least a channel each, whole waves while the remainder allows, summing to the bank -- under -fsanitize=address,undefined (host
code only, a program of its own).  The program checks itself and exits non-zero on a miss."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_shard_core_dealing_and_reordering(tmp_path):
    exe = os.path.join(str(tmp_path), "shard_deal")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include"), "-I" + os.path.join(ROOT, "spandsp_amd", "csrc"),
           os.path.join(ROOT, "tests", "c_callers", "shard_deal.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    p = subprocess.run([exe], capture_output=True, text=True)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "cases: ok" in out and "Sanitizer" not in out and "runtime error" not in out, out
