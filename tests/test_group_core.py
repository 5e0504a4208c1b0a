"""The staging protocol of the channel groups, on the host.

spandsp_amd/csrc/shim_group.h is the one place where "an object stages a frame a tick, the tick runs when the last attached
object has staged or at the flush, callbacks may stage again" is written; the tone, modem, line and echo shims include it.  It
depends on no bank, so tests/c_callers/group_core.c drives it with fake run / deliver hooks: when the tick runs and with which
lengths, a second frame, a failing run, staging from inside a delivery, release, two threads after one slot, and four threads
staging 50 ticks -- under -fsanitize=thread (host code only).  The program checks itself and exits non-zero on a miss."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_core_protocol_and_threads(tmp_path):
    exe = os.path.join(str(tmp_path), "group_core")
    cmd = ["gcc", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-fsanitize=thread", "-O1", "-g",
           "-I" + os.path.join(ROOT, "spandsp_amd", "csrc"), os.path.join(ROOT, "tests", "c_callers", "group_core.c"),
           "-o", exe, "-lpthread"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    p = subprocess.run([exe], capture_output=True, text=True, env=env)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "group_core: 8 channels, 4 threads, 50 ticks: ok" in out and "ThreadSanitizer" not in out, out
