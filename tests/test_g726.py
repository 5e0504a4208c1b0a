"""The G.726 codec banks without a GPU: the exported names, the by-name prototypes against the reference's g726.h, the C
ABI's behaviour where there is no device, and the kernels' per-sample functions (csrc/g726_dev.hpp) compiled for the host
into a stand-alone program, built with the address and undefined-behaviour sanitizers, that runs every case of the
committed fixture one lane at a time: codes, packed bytes, samples, counts and state words equal the reference's, a second
cut of every stream into calls gives the same stream, and the capacity functions are reached and never passed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import g726_lines as GL
from spandsp_amd import engine
from test_c_callers import REF, _prototypes, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE, BAD_ARG = -1, -2
NAMES = {"g726_init", "g726_release", "g726_free", "g726_encode", "g726_decode"}
CALLS = ["create", "destroy", "channels", "set_stream", "sync", "encode", "decode", "encode_capacity", "decode_capacity", "counts_dev",
         "restart", "state_words", "get_state", "set_state"]
BANK_NAMES = {"spangpu_g726_" + c for c in CALLS}


@pytest.fixture(scope="module")
def golden():
    return GL.load()


def test_symbols_are_exported(built):
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines()}
    assert not (NAMES | BANK_NAMES) - have, sorted((NAMES | BANK_NAMES) - have)
    assert {n for n in have if "g726" in n.lower() and not n.startswith("_Z")} == NAMES | BANK_NAMES


def test_every_entry_point_is_declared(built):
    text = open(os.path.join(ROOT, "include", "spangpu.h")).read()
    declared = set(re.findall(r"SPANGPU_API\s+[\w\s\*]+?\b(spangpu_g726_\w+)\s*\(", text))
    assert declared == BANK_NAMES
    assert {p[0] for p in _prototypes("spangpu_spandsp.h", "SPANGPU_G726_API")} == NAMES
    # ... and out of the way of the check over the fixed list of reference headers (tests/test_c_callers.py)
    assert not NAMES & {p[0] for p in _prototypes("spangpu_spandsp.h", "SPANGPU_API")}


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference's headers are not here (GPU box)")
def test_g726_prototypes_are_the_references(built, tmp_path):
    ref_text = open(os.path.join(REF, "spandsp", "g726.h")).read()
    declared = set(re.findall(r"SPAN_DECLARE\([^)]*\)\s*(\w+)\s*\(", ref_text))
    assert declared == NAMES
    lines = ["#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>", "#include <stdio.h>", "#include <stdbool.h>"]
    for h in ("telephony", "g726"):
        lines.append('#include "spandsp/%s.h"' % h)
    for name, ret, args in _prototypes("spangpu_spandsp.h", "SPANGPU_G726_API"):
        lines.append("static %s (*chk_%s)(%s) = %s;" % (ret, name, args, name))
    lines.append("int main(void) { return 0; }")
    src = os.path.join(str(tmp_path), "g726_proto_check.c")
    open(src, "w").write("\n".join(lines) + "\n")
    run(["gcc", "-std=gnu99", "-fsyntax-only", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-Wno-unused-variable",
         "-DHAVE_STDBOOL_H", "-DHAVE_INTTYPES_H", "-DHAVE_STDINT_H", "-I" + REF, src])
    # the enums a caller's source names have the reference's values
    mine = open(os.path.join(ROOT, "include", "spangpu_spandsp.h")).read()
    for name in ("G726_ENCODING_LINEAR", "G726_ENCODING_ULAW", "G726_ENCODING_ALAW", "G726_PACKING_NONE", "G726_PACKING_LEFT", "G726_PACKING_RIGHT"):
        assert name in mine and name in ref_text
    assert (engine.G726_LINEAR, engine.G726_ULAW, engine.G726_ALAW) == (0, 1, 2)
    assert (engine.G726_PACKING_NONE, engine.G726_PACKING_LEFT, engine.G726_PACKING_RIGHT) == (0, 1, 2)


def _create(n, rates, codings, packings):
    r, c, p = (np.asarray(v, np.int32) for v in (rates, codings, packings))
    h = C.c_void_p()
    return engine.lib().spangpu_g726_create(C.byref(h), 0, n, r.ctypes.data, c.ctypes.data, p.ctypes.data, len(r)), h


def test_no_device_is_an_error_not_a_fallback(built):
    L = engine.lib()
    rc, h = _create(8, [32000], [0], [2])
    if engine.device_count() > 0:
        assert rc == 0 and h.value
        L.spangpu_g726_destroy(h)
    else:
        assert rc == NO_DEVICE and not h.value
        L.g726_init.restype = C.c_void_p
        L.g726_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        assert L.g726_init(None, 32000, 0, 0) is None


def test_bad_arguments_are_refused(built):
    L = engine.lib()
    # the rates g726_init() refuses, codings and packings outside the enums: before any device is looked for
    for rates, codings, packings in (([8000], [0], [0]), ([48000], [0], [0]), ([32000, 0], [0, 0], [0, 0]), ([32000], [3], [0]),
                                     ([32000], [-1], [0]), ([32000], [0], [3]), ([32000], [0], [-1])):
        rc, h = _create(8, rates, codings, packings)
        assert rc == BAD_ARG and not h.value, (rates, codings, packings)
    rc, h = _create(0, [32000], [0], [0])
    assert rc == BAD_ARG
    r = np.array([32000], np.int32)
    h = C.c_void_p()
    assert L.spangpu_g726_create(None, 0, 8, r.ctypes.data, r.ctypes.data, r.ctypes.data, 1) == BAD_ARG
    assert L.spangpu_g726_create(C.byref(h), 0, 8, None, r.ctypes.data, r.ctypes.data, 1) == BAD_ARG
    assert L.spangpu_g726_create(C.byref(h), 0, 8, r.ctypes.data, r.ctypes.data, r.ctypes.data, 0) == BAD_ARG
    for call in (L.spangpu_g726_channels, L.spangpu_g726_sync, L.spangpu_g726_state_words):
        assert call(None) == BAD_ARG
    assert L.spangpu_g726_set_stream(None, None) == BAD_ARG
    assert L.spangpu_g726_encode(None, None, 0, 0, None, 8, None, 0, 0, None) == BAD_ARG
    assert L.spangpu_g726_decode(None, None, 0, 0, None, 8, None, 0, 0, None) == BAD_ARG
    assert L.spangpu_g726_encode_capacity(None, 8) == BAD_ARG and L.spangpu_g726_decode_capacity(None, 8) == BAD_ARG
    assert L.spangpu_g726_counts_dev(None) is None
    assert L.spangpu_g726_restart(None, 0, 32000, 0, 0) == BAD_ARG
    assert L.spangpu_g726_get_state(None, 0, None) == BAD_ARG and L.spangpu_g726_set_state(None, 0, None) == BAD_ARG
    L.spangpu_g726_destroy(None)
    # the by-name calls on nothing
    L.g726_init.restype = C.c_void_p
    L.g726_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    for rate in (0, 8000, 64000):
        assert L.g726_init(None, rate, 0, 0) is None
    assert L.g726_release(None) == 0 and L.g726_free(None) == 0
    assert L.g726_encode(None, None, None, 8) == 0 and L.g726_decode(None, None, None, 8) == 0


def test_fixture_covers_what_it_has_to(golden):
    g = golden
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g726.npz")) <= 478071
    cs = GL.cases(g)
    assert {(c.rate, c.coding, c.packing) for c in cs if c.kind == GL.ENCODE} == set(GL.CONFIGS)
    assert {(c.rate, c.coding, c.packing) for c in cs if c.kind == GL.DECODE} == set(GL.CONFIGS)
    assert len([c for c in cs if c.line == "rnd"]) == 12
    for rate, words in zip(GL.RATES, g["init"]):
        assert words[0] == 34816 and words[1] == 544 and words[26] == rate and words[28] == rate//8000
        # bytes of the random line with bits above the code width
        assert all(int(GL.random_bytes(rate, c).max()) >> (rate//8000) for c in GL.CODINGS)
    # calls that leave every residue 1 .. 7 behind, in both packings
    for p in (1, 2):
        seen = set()
        for rate in GL.RATES:
            seen |= set(g["pkmeta%d_%d" % (p, rate)][..., 2].ravel().tolist())
        assert seen >= set(range(8)), (p, seen)


def test_step_functions_on_the_host_under_sanitizers(built, golden, tmp_path):
    exe = os.path.join(str(tmp_path), "g726_host")
    data = os.path.join(str(tmp_path), "cases.txt")
    n = GL.dump_text(data, GL.cases(golden))
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           os.path.join(ROOT, "tests", "c_callers", "g726_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    p = subprocess.run([exe, data], capture_output=True, text=True)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "ok %d cases" % n in out, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    # some call reached each capacity function exactly or within one unit; none passed it (the program stops on that)
    m = re.search(r"capacity slack: encode (\d+), decode (\d+)", out)
    assert m and int(m.group(1)) <= 1 and int(m.group(2)) <= 1, out
