"""The echo canceller groups as a C compiler and as threads see them.

tests/c_callers/echo_group.c -- 1 024 echo_can_state_t objects attached to one group, staged by 16 pthreads that each own their
objects, 50 ticks, the tick run by whichever thread completes the set; then the same lines from one thread into a fresh group:
the CRC-32 of all clean samples must agree -- is compiled `gcc -std=c99 -pedantic -Wall -Wextra -Werror` and as C++ against
include/ alone, and runs on the GPU.  Without a GPU the same program is linked with csrc/shim_echo.c itself and a stub bank
(tests/echo_bank_stub.c) under -fsanitize=thread: the staging, the lock and the hand-over of the tick must give the sanitizer
nothing to report.  (Host code only: no sanitizer touches device code.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_callers")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "spandsp_amd")


def run(cmd, env=None):
    p = subprocess.run(cmd, capture_output=True, text=True, env=env)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    return p.stdout + p.stderr


def build(name, out_dir):
    """(the flags of tests/test_c_callers.py, plus the thread library)"""
    src = os.path.join(SRC, name + ".c")
    obj = os.path.join(out_dir, name + ".o")
    exe = os.path.join(out_dir, name)
    run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + INC, "-c", src, "-o", obj])
    run(["g++", "-std=c++11", "-x", "c++", "-Wall", "-Wextra", "-Werror", "-I" + INC, "-c", src, "-o", obj + "pp"])
    run(["gcc", "-o", exe, obj, "-L" + LIBDIR, "-lspangpu_prims", "-lspangpu", "-lm", "-lpthread", "-Wl,-rpath," + LIBDIR])
    return exe


def test_echo_group_caller_compiles_and_links(built, tmp_path):
    build("echo_group", str(tmp_path))


def test_echo_group_staging_is_race_free(tmp_path):
    """shim_echo.c under ThreadSanitizer, against the stub bank: 16 threads, 1 024 objects, 50 ticks, no report."""
    exe = os.path.join(str(tmp_path), "echo_group_tsan")
    run(["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=thread", "-Wall", "-Wextra", "-Werror", "-I" + INC,
         os.path.join(SRC, "echo_group.c"), os.path.join(ROOT, "spandsp_amd", "csrc", "shim_echo.c"),
         os.path.join(ROOT, "tests", "echo_bank_stub.c"), "-o", exe, "-lpthread"])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    out = run([exe, "1024", "16", "50"], env=env)
    assert "echo_group: 1024 objects" in out and "ThreadSanitizer" not in out, out


@pytest.mark.gpu
def test_echo_group_caller_runs(built, tmp_path):
    exe = build("echo_group", str(tmp_path))
    out = run([exe])
    assert "echo_group: 1024 objects, 50 ticks" in out
