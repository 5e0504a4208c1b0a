"""The sender objects as a C compiler sees them: tests/c_callers/fsk_tx_objects.c -- fsk_tx, modem_connect_tones_tx and async_tx
by name, with a counting get_bit and a status handler -- is compiled `gcc -std=c99 -pedantic -Wall -Wextra -Werror` and as
C++ against include/ alone, and runs on the GPU: call counts, the end-of-data sequence and the return values."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_callers")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "spandsp_amd")


def run(cmd):
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    return p.stdout + p.stderr


def build(name, out_dir):
    src = os.path.join(SRC, name + ".c")
    obj = os.path.join(out_dir, name + ".o")
    exe = os.path.join(out_dir, name)
    run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + INC, "-c", src, "-o", obj])
    run(["g++", "-std=c++11", "-x", "c++", "-Wall", "-Wextra", "-Werror", "-I" + INC, "-c", src, "-o", obj + "pp"])
    run(["gcc", "-o", exe, obj, "-L" + LIBDIR, "-lspangpu", "-lm", "-Wl,-rpath," + LIBDIR])
    return exe


def test_fsk_tx_objects_caller_compiles_and_links(built, tmp_path):
    build("fsk_tx_objects", str(tmp_path))


@pytest.mark.gpu
def test_fsk_tx_objects_caller_runs(built, tmp_path):
    out = run([build("fsk_tx_objects", str(tmp_path))])
    assert "fsk_tx_objects: ok" in out, out
