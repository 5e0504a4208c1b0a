"""The packet loss concealment banks without a GPU: the exported names, the by-name prototypes against the reference's plc.h, the
C ABI's behaviour where there is no device, what the committed fixture has to cover and how large it may be, the fixture
against a fresh run of its generator where the reference is present, and the kernel's per-line functions (csrc/plc_dev.hpp)
compiled for the host into a stand-alone program, built with the address and undefined-behaviour sanitizers, that runs every
case of the fixture one line at a time: samples and the 404 state words equal the reference's after every call, the pitch
search gives the same lag in two orders of combination, and a second cut of every stream's heard stretches gives the same
samples."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import plc_lines as PL
from spandsp_amd import engine
from test_c_callers import REF, _prototypes, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE, BAD_ARG = -1, -2
NAMES = {"plc_" + n for n in ("init", "release", "free", "rx", "fillin")}
CALLS = ["create", "destroy", "channels", "set_stream", "sync", "run", "conceal", "restart", "state_words", "get_state", "set_state"]
BANK_NAMES = {"spangpu_plc_" + c for c in CALLS}


@pytest.fixture(scope="module")
def golden():
    return PL.load()


def test_symbols_are_exported(built):
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines()}
    assert len(NAMES) == 5 and not (NAMES | BANK_NAMES) - have, sorted((NAMES | BANK_NAMES) - have)
    assert {n for n in have if re.match(r"(spangpu_)?plc_", n)} == NAMES | BANK_NAMES


def test_every_entry_point_is_declared(built):
    text = open(os.path.join(ROOT, "include", "spangpu.h")).read()
    declared = set(re.findall(r"SPANGPU_API\s+[\w\s\*]+?\b(spangpu_plc_\w+)\s*\(", text))
    assert declared == BANK_NAMES
    assert {p[0] for p in _prototypes("spangpu_spandsp.h", "SPANGPU_PLC_API")} == NAMES
    # ... and out of the way of the check over the fixed list of reference headers (tests/test_c_callers.py)
    assert not NAMES & {p[0] for p in _prototypes("spangpu_spandsp.h", "SPANGPU_API")}


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference's headers are not here (GPU box)")
def test_plc_prototypes_are_the_references(built, tmp_path):
    ref_text = open(os.path.join(REF, "spandsp", "plc.h")).read()
    declared = set(re.findall(r"SPAN_DECLARE\([^)]*\)\s*(\w+)\s*\(", ref_text))
    assert declared == NAMES
    lines = ["#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>", "#include <stdio.h>", "#include <stdbool.h>"]
    for h in ("telephony", "plc"):
        lines.append('#include "spandsp/%s.h"' % h)
    for name, ret, args in _prototypes("spangpu_spandsp.h", "SPANGPU_PLC_API"):
        lines.append("static %s (*chk_%s)(%s) = %s;" % (ret, name, args, name))
    lines.append("int main(void) { return 0; }")
    src = os.path.join(str(tmp_path), "plc_proto_check.c")
    open(src, "w").write("\n".join(lines) + "\n")
    run(["gcc", "-std=gnu99", "-fsyntax-only", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-Wno-unused-variable",
         "-DHAVE_STDBOOL_H", "-DHAVE_INTTYPES_H", "-DHAVE_STDINT_H", "-I" + REF, src])
    # the sizes the state words are laid out by are the reference's
    for name, value in (("PLC_PITCH_MIN", 120), ("PLC_PITCH_MAX", 40), ("CORRELATION_SPAN", 160)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", ref_text)
        assert m and int(m.group(1)) == value, name
    assert (PL.LAG_FIRST, PL.LAG_LAST, PL.SPAN, PL.HIST) == (40, 120, 160, 280)


def _create(n):
    h = C.c_void_p()
    return engine.lib().spangpu_plc_create(C.byref(h), 0, n), h


def test_no_device_is_an_error_not_a_fallback(built):
    L = engine.lib()
    rc, h = _create(8)
    if engine.device_count() > 0:
        assert rc == 0 and h.value
        L.spangpu_plc_destroy(h)
    else:
        assert rc == NO_DEVICE and not h.value
        L.plc_init.restype = C.c_void_p
        L.plc_init.argtypes = [C.c_void_p]
        assert L.plc_init(None) is None
        with pytest.raises(engine.SpanGpuError) as ei:
            engine.PlcBank(8)
        assert ei.value.code == NO_DEVICE


def test_bad_arguments_are_refused(built):
    L = engine.lib()
    for n in (0, -1):
        rc, h = _create(n)
        assert rc == BAD_ARG and not h.value
    assert L.spangpu_plc_create(None, 0, 8) == BAD_ARG
    for call in (L.spangpu_plc_channels, L.spangpu_plc_sync, L.spangpu_plc_state_words):
        assert call(None) == BAD_ARG
    assert L.spangpu_plc_set_stream(None, None) == BAD_ARG
    row = np.zeros(160, np.int16)
    assert L.spangpu_plc_run(None, row.ctypes.data, engine.MEM_HOST, 320, None, None, 160) == BAD_ARG
    assert L.spangpu_plc_conceal(None, row.ctypes.data, 320, row.ctypes.data, None, 160, 160) == BAD_ARG
    assert L.spangpu_plc_restart(None, 0) == BAD_ARG
    assert L.spangpu_plc_get_state(None, 0, None) == BAD_ARG and L.spangpu_plc_set_state(None, 0, None) == BAD_ARG
    L.spangpu_plc_destroy(None)
    # the by-name calls on nothing
    for f in (L.plc_rx, L.plc_fillin):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        assert f(None, row.ctypes.data, 160) == 0
    L.plc_release.argtypes = L.plc_free.argtypes = [C.c_void_p]
    assert L.plc_release(None) == 0 and L.plc_free(None) == 0


def test_fixture_covers_what_it_has_to(golden):
    g = golden
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "plc.npz")) <= PL.MAX_FIXTURE_BYTES == 478071
    # data only: integer arrays, nothing pickled (np.load refuses those by default) and nothing else
    assert all(g[k].dtype.kind in "iu" for k in g.files)
    assert sum(n for _, n in PL.SCHEDULE) == 2938 <= PL.N and len(PL.NAMES) == 9
    cs = PL.sched_cases(g)
    assert len(cs) == 9 and all(len(c.calls) == len(PL.SCHEDULE) for c in cs)
    assert all(len(w) == PL.WORDS == 404 and len(out) == n for c in PL.cases(g) for _, n, _, out, w in c.calls)
    # the words are the reference's fields in the reference's order: three ints, 120 floats, 280 int16_t, an int
    off = g["offsets"]
    assert off.shape == (404, 2) and (np.diff(off[:, 0]) > 0).all()
    assert off[:, 1].tolist() == [4]*3 + [4]*120 + [2]*280 + [4]
    c = PL.coverage(cs)
    PL.check_coverage(c)
    assert c["buf_ptr_end"] == {162}
    # the heard-only case hears everything: no gap, no pitch, the same lengths
    h = PL.heard_case(g)
    assert [n for _, n, _, _, _ in h.calls] == [n for _, n in PL.SCHEDULE]
    assert all(not lost and np.array_equal(row, out) and not w[:PL.W_HISTORY].any() for lost, _, row, out, w in h.calls)
    # the decoded-line cases: whole frames, at least two gaps, one of them three frames long, twelve frames heard
    ticks = "".join(map(str, PL.DEC_TICKS))
    assert "0111" in ticks and len(re.findall(r"1+", ticks)) >= 2 and ticks.count("0") == 12
    d = PL.dec_cases(g)
    assert len(d) == 5 and all(len(x.calls) == len(PL.DEC_TICKS) for x in d)


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference is not here (GPU box)")
def test_fixture_is_what_the_generator_makes(golden):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_golden_plc
    finally:
        sys.path.pop(0)
    fresh = make_golden_plc.generate(REF)
    assert sorted(fresh) == sorted(golden.files)
    for k in golden.files:
        assert fresh[k].dtype == golden[k].dtype and np.array_equal(fresh[k], golden[k]), k


def test_line_functions_on_the_host_under_sanitizers(built, golden, tmp_path):
    exe = os.path.join(str(tmp_path), "plc_host")
    data = os.path.join(str(tmp_path), "cases.txt")
    n = PL.dump_text(data, PL.cases(golden))
    assert n == 15
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           os.path.join(ROOT, "tests", "c_callers", "plc_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    p = subprocess.run([exe, data], capture_output=True, text=True)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "ok %d cases" % n in out, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    m = re.search(r"searches: (\d+), the most lags tied (\d+)", out)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) == 81, out
