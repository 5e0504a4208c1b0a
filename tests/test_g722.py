"""The G.722 codec banks without a GPU: the exported names, the by-name prototypes against the reference's g722.h, the C
ABI's behaviour where there is no device, what the committed fixture has to cover, and the kernels' per-code functions
(csrc/g722_dev.hpp) compiled for the host into a stand-alone program, built with the address and undefined-behaviour
sanitizers, that runs every case of the fixture one lane at a time: codes, packed bytes, samples, counts and state words
equal the reference's after every call, a second cut of every stream into calls gives the same stream, and the capacity
functions are reached and never passed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import g722_lines as GL
from spandsp_amd import engine
from test_c_callers import REF, _prototypes, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE, BAD_ARG = -1, -2
NAMES = {"g722_%s%s" % (side, call) for side in ("encode", "decode") for call in ("_init", "_release", "_free", "")}
CALLS = ["create", "destroy", "channels", "set_stream", "sync", "encode", "decode", "encode_capacity", "decode_capacity", "counts_dev",
         "restart", "state_words", "get_state", "set_state"]
BANK_NAMES = {"spangpu_g722_" + c for c in CALLS}


@pytest.fixture(scope="module")
def golden():
    return GL.load()


def test_symbols_are_exported(built):
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines()}
    assert len(NAMES) == 8 and not (NAMES | BANK_NAMES) - have, sorted((NAMES | BANK_NAMES) - have)
    assert {n for n in have if "g722" in n.lower() and not n.startswith("_Z")} == NAMES | BANK_NAMES


def test_every_entry_point_is_declared(built):
    text = open(os.path.join(ROOT, "include", "spangpu.h")).read()
    declared = set(re.findall(r"SPANGPU_API\s+[\w\s\*]+?\b(spangpu_g722_\w+)\s*\(", text))
    assert declared == BANK_NAMES
    assert {p[0] for p in _prototypes("spangpu_spandsp.h", "SPANGPU_G722_API")} == NAMES
    # ... and out of the way of the check over the fixed list of reference headers (tests/test_c_callers.py)
    assert not NAMES & {p[0] for p in _prototypes("spangpu_spandsp.h", "SPANGPU_API")}


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference's headers are not here (GPU box)")
def test_g722_prototypes_are_the_references(built, tmp_path):
    ref_text = open(os.path.join(REF, "spandsp", "g722.h")).read()
    declared = set(re.findall(r"SPAN_DECLARE\([^)]*\)\s*(\w+)\s*\(", ref_text))
    assert declared == NAMES
    lines = ["#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>", "#include <stdio.h>", "#include <stdbool.h>"]
    for h in ("telephony", "g722"):
        lines.append('#include "spandsp/%s.h"' % h)
    for name, ret, args in _prototypes("spangpu_spandsp.h", "SPANGPU_G722_API"):
        lines.append("static %s (*chk_%s)(%s) = %s;" % (ret, name, args, name))
    lines.append("int main(void) { return 0; }")
    src = os.path.join(str(tmp_path), "g722_proto_check.c")
    open(src, "w").write("\n".join(lines) + "\n")
    run(["gcc", "-std=gnu99", "-fsyntax-only", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-Wno-unused-variable",
         "-DHAVE_STDBOOL_H", "-DHAVE_INTTYPES_H", "-DHAVE_STDINT_H", "-I" + REF, src])
    # the enums a caller's source names have the reference's values
    mine = open(os.path.join(ROOT, "include", "spangpu_spandsp.h")).read()
    for name, value in (("G722_SAMPLE_RATE_8000", 1), ("G722_PACKED", 2)):
        for text in (mine, ref_text):
            m = re.search(name + r"\s*=\s*(\w+)", text)
            assert m and int(m.group(1), 0) == value, name
    assert (engine.G722_SAMPLE_RATE_8000, engine.G722_PACKED) == (1, 2)


def _create(n, direction, rates, options):
    r, o = (np.asarray(v, np.int32) for v in (rates, options))
    h = C.c_void_p()
    return engine.lib().spangpu_g722_create(C.byref(h), 0, n, direction, r.ctypes.data, o.ctypes.data, len(r)), h


def _by_name(L):
    for side in ("encode", "decode"):
        f = getattr(L, "g722_%s_init" % side)
        f.restype = C.c_void_p
        f.argtypes = [C.c_void_p, C.c_int, C.c_int]


def test_no_device_is_an_error_not_a_fallback(built):
    L = engine.lib()
    rc, h = _create(8, engine.G722_ENCODER, [56000], [3])
    if engine.device_count() > 0:
        assert rc == 0 and h.value
        L.spangpu_g722_destroy(h)
    else:
        assert rc == NO_DEVICE and not h.value
        _by_name(L)
        assert L.g722_encode_init(None, 64000, 0) is None and L.g722_decode_init(None, 64000, 0) is None


def test_bad_arguments_are_refused(built):
    L = engine.lib()
    # rates outside the three (the bank is stricter than g722_*_init()), option bits outside 0x3, a direction that is none:
    # before any device is looked for
    for direction, rates, options in ((0, [8000], [0]), (1, [32000], [0]), (0, [64000, 0], [0, 0]), (0, [64000], [4]), (1, [48000], [-1]),
                                      (0, [56000, 56000], [3, 8]), (2, [64000], [0]), (-1, [64000], [0])):
        rc, h = _create(8, direction, rates, options)
        assert rc == BAD_ARG and not h.value, (direction, rates, options)
    rc, h = _create(0, 0, [64000], [0])
    assert rc == BAD_ARG
    r = np.array([64000], np.int32)
    o = np.array([0], np.int32)
    h = C.c_void_p()
    assert L.spangpu_g722_create(None, 0, 8, 0, r.ctypes.data, o.ctypes.data, 1) == BAD_ARG
    assert L.spangpu_g722_create(C.byref(h), 0, 8, 0, None, o.ctypes.data, 1) == BAD_ARG
    assert L.spangpu_g722_create(C.byref(h), 0, 8, 0, r.ctypes.data, None, 1) == BAD_ARG
    assert L.spangpu_g722_create(C.byref(h), 0, 8, 0, r.ctypes.data, o.ctypes.data, 0) == BAD_ARG
    for call in (L.spangpu_g722_channels, L.spangpu_g722_sync, L.spangpu_g722_state_words):
        assert call(None) == BAD_ARG
    assert L.spangpu_g722_set_stream(None, None) == BAD_ARG
    assert L.spangpu_g722_encode(None, None, 0, 0, None, 8, None, 0, 0, None) == BAD_ARG
    assert L.spangpu_g722_decode(None, None, 0, 0, None, 8, None, 0, 0, None) == BAD_ARG
    assert L.spangpu_g722_encode_capacity(None, 8) == BAD_ARG and L.spangpu_g722_decode_capacity(None, 8) == BAD_ARG
    assert L.spangpu_g722_counts_dev(None) is None
    assert L.spangpu_g722_restart(None, 0, 64000, 0) == BAD_ARG
    assert L.spangpu_g722_get_state(None, 0, None) == BAD_ARG and L.spangpu_g722_set_state(None, 0, None) == BAD_ARG
    L.spangpu_g722_destroy(None)
    # the by-name calls on nothing
    assert L.g722_encode_release(None) == 0 and L.g722_encode_free(None) == 0
    assert L.g722_decode_release(None) == 0 and L.g722_decode_free(None) == 0
    assert L.g722_encode(None, None, None, 8) == 0 and L.g722_decode(None, None, None, 8) == 0


def test_fixture_covers_what_it_has_to(golden):
    g = golden
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g722.npz")) <= 478071
    cs = GL.cases(g)
    assert len(GL.CONFIGS) == 12
    for kind in (GL.ENCODE, GL.DECODE):
        for line in (0, 1, 2):
            assert {c.config for c in cs if c.kind == kind and c.line == line} == set(GL.CONFIGS)
    assert {c.config for c in cs if c.line == "rnd" and c.kind == GL.DECODE} == set(GL.CONFIGS)
    # every call has its count and its 74 words
    assert all(len(w) == GL.WORDS for c in cs for _, _, w in c.calls)
    # the words g722_*_init() leaves
    for (rate, eight_k, packed), pair in zip(GL.CONFIGS, g["init"]):
        for w in pair:
            assert (w[GL.W_PACKED], w[GL.W_EIGHT_K], w[GL.W_BPS]) == (int(packed and rate != 64000), eight_k, GL.bits_of(rate))
            assert w[GL.W_BAND0 + 1] == 32 and w[GL.W_BAND1 + 1] == 8 and np.count_nonzero(w) == 3 + eight_k + int(packed and rate != 64000)
    # bytes of the random lines with bits above the code width
    assert all(int(GL.random_bytes(r, e, p).max()) >> GL.bits_of(r) for r, e, p in GL.CONFIGS if r != 64000)
    # 16 kHz encoders are called with pairs only; the 8 kHz ones with 1 and 7 samples as well
    assert all(n % 2 == 0 for n in GL.ENC_SCHEDULE_16K) and {1, 7} <= set(GL.ENC_SCHEDULE_8K)
    assert all(n % 2 == 0 for c in cs if c.kind == GL.ENCODE and not c.eight_k for n, _, _ in c.calls)
    # the bits a packing encoder's call leaves waiting: every value the width can leave
    for rate, reach in ((48000, {0, 2, 4, 6}), (56000, set(range(8)))):
        seen = {int(w[GL.W_BITS]) for c in cs if c.kind == GL.ENCODE and c.rate == rate and c.packed for _, _, w in c.calls}
        assert seen == reach, (rate, seen)
    # a packed decoder's call that ends with a whole code still buffered
    kept = [c.name for c in cs if c.kind == GL.DECODE and c.packed and c.rate != 64000 for _, _, w in c.calls if w[GL.W_BITS] >= GL.bits_of(c.rate)]
    assert len(kept) >= 12, len(kept)
    # the rings have been round more than once, and a call has ended at a ptr other than 0
    assert any(w[GL.W_PTR] for c in cs if not c.eight_k for _, _, w in c.calls)
    # unpacked at 64000 is what G722_PACKED gives there
    assert GL.stored(64000, 0, 1) == (64000, 0, 0)


def test_step_functions_on_the_host_under_sanitizers(built, golden, tmp_path):
    exe = os.path.join(str(tmp_path), "g722_host")
    data = os.path.join(str(tmp_path), "cases.txt")
    n = GL.dump_text(data, GL.cases(golden))
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           os.path.join(ROOT, "tests", "c_callers", "g722_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    p = subprocess.run([exe, data], capture_output=True, text=True)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "ok %d cases" % n in out, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    # some call reached each capacity function within one code; none passed it (the program stops on that)
    m = re.search(r"capacity slack: encode (\d+), decode (\d+)", out)
    assert m and int(m.group(1)) <= 1 and int(m.group(2)) <= 1, out
