"""The lone spandsp-named objects -- one object on a private one-channel bank -- on the host.

spandsp_amd/csrc/shim_object.h is the one place where an object's life (caller storage or the heap, release, free), its
grow-only row, the codec and sender piece loops and the bit puller are written; the codec, v18, adsi, FSK, connect tone, modem
and digit sender shims include it.  tests/c_callers/lone_objects.c drives those shims over a stand-in bank
(tests/lone_bank_stub.c) that prints every bank call, under -fsanitize=address,undefined (host code only, a program of its
own), and prints every return value, a checksum of what the caller's buffer got and whether the bytes behind it were left
alone.  The transcript must equal tests/golden/lone_objects.txt: the bank-call sequence of every shim call, the order of
get_bit, status and bank calls, and "storage unchanged" after every failed init."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spandsp_amd", "csrc")
SHIMS = ["shim_g726.c", "shim_g722.c", "shim_gsm0610.c", "shim_v18.c", "shim_adsi.c", "shim_fsktx.c", "shim_modemtx.c", "shim_fsk.c",
         "adsi_host.c"]


def test_lone_objects_transcript(tmp_path):
    exe = os.path.join(str(tmp_path), "lone_objects")
    cmd = ["gcc", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC] + [os.path.join(CSRC, f) for f in SHIMS]
    cmd += [os.path.join(ROOT, "tests", "lone_bank_stub.c"), os.path.join(ROOT, "tests", "c_callers", "lone_objects.c"),
            "-o", exe, "-lm", "-lpthread"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr
    want = open(os.path.join(ROOT, "tests", "golden", "lone_objects.txt")).read()
    got = p.stdout.splitlines()
    for i, (g, w) in enumerate(zip(got, want.splitlines())):
        assert g == w, "line %d" % (i + 1)
    assert p.stdout == want
    assert "storage changed" not in p.stdout and "WRITTEN" not in p.stdout
    assert got[-1] == "live banks at the end: 0"
