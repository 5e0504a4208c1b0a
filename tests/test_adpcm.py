"""The IMA and OKI ADPCM codec banks without a GPU: the exported names, the by-name prototypes against the reference's
ima_adpcm.h and oki_adpcm.h, the C ABI's behaviour where there is no device, what the committed fixtures reach, the by-name
objects over a stand-in bank, and the kernels' per-item functions and per-call bodies (csrc/adpcm_dev.hpp) compiled for the
host into a stand-alone program, built with the address and undefined-behaviour sanitizers, that runs every case of the
fixtures one lane at a time: outputs, counts and state words equal the reference's, a second cut of every stream that may be
cut gives the same stream, the three documented deviations behave as documented, and the capacity functions are reached
and never passed.  Where the reference is at hand, 2 000 generated lines per family go through the same program against it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adpcm_lines as AL
from spandsp_amd import engine
from test_c_callers import REF, _prototypes, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spandsp_amd", "csrc")
NO_DEVICE, BAD_ARG = -1, -2
FAMILIES = ("ima_adpcm", "oki_adpcm")
NAMES = {f: {"%s_%s" % (f, c) for c in ("init", "release", "free", "encode", "decode")} for f in FAMILIES}
CALLS = ["create", "destroy", "channels", "set_stream", "sync", "encode", "decode", "encode_capacity", "decode_capacity", "counts_dev",
         "restart", "state_words", "get_state", "set_state"]
BANK_NAMES = {f: {"spangpu_%s_%s" % (f, c) for c in CALLS} for f in FAMILIES}
SWEEP_LINES = 2000


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """csrc/adpcm_dev.hpp for the host, under the sanitizers: tests/c_callers/adpcm_host.cpp"""
    return AL.build_host_program(str(tmp_path_factory.mktemp("adpcm_host")))


def run_cases(exe, path, n):
    """the host program over the cases dumped at `path`; returns the four capacity slacks"""
    p = subprocess.run([exe, path], capture_output=True, text=True)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "ok %d cases" % n in out, out[-3000:]
    assert "Sanitizer" not in out and "runtime error" not in out, out[-3000:]
    m = re.search(r"capacity slack: ima encode (-?\d+), ima decode (-?\d+), oki encode (-?\d+), oki decode (-?\d+)", out)
    assert m, out
    return [int(x) for x in m.groups()]


def test_symbols_are_exported(built):
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines()}
    for f in FAMILIES:
        want = NAMES[f] | BANK_NAMES[f]
        assert len(want) == 19 and not want - have, sorted(want - have)
        assert {n for n in have if f in n.lower() and not n.startswith("_Z")} == want


def test_every_entry_point_is_declared(built):
    text = open(os.path.join(ROOT, "include", "spangpu.h")).read()
    for f in FAMILIES:
        declared = set(re.findall(r"SPANGPU_API\s+[\w\s\*]+?\b(spangpu_%s_\w+)\s*\(" % f, text))
        assert declared == BANK_NAMES[f]
    assert {p[0] for p in _prototypes("spangpu_spandsp.h", "SPANGPU_ADPCM_API")} == NAMES["ima_adpcm"] | NAMES["oki_adpcm"]
    # ... and out of the way of the check over the fixed list of reference headers (tests/test_c_callers.py)
    assert not (NAMES["ima_adpcm"] | NAMES["oki_adpcm"]) & {p[0] for p in _prototypes("spangpu_spandsp.h", "SPANGPU_API")}


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference's headers are not here (GPU box)")
def test_adpcm_prototypes_are_the_references(built, tmp_path):
    declared = set()
    for f in FAMILIES:
        ref_text = open(os.path.join(REF, "spandsp", f + ".h")).read()
        here = set(re.findall(r"SPAN_DECLARE\([^)]*\)\s*(\w+)\s*\(", ref_text))
        assert here == NAMES[f]
        declared |= here
    lines = ["#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>", "#include <stdio.h>", "#include <stdbool.h>"]
    for h in ("telephony", "ima_adpcm", "oki_adpcm"):
        lines.append('#include "spandsp/%s.h"' % h)
    protos = _prototypes("spangpu_spandsp.h", "SPANGPU_ADPCM_API")
    assert {p[0] for p in protos} == declared
    for name, ret, args in protos:
        lines.append("static %s (*chk_%s)(%s) = %s;" % (ret, name, args, name))
    # the enum a caller's source names has the reference's values
    lines.append("typedef char chk_enum[(IMA_ADPCM_IMA4 == 0  &&  IMA_ADPCM_DVI4 == 1  &&  IMA_ADPCM_VDVI == 2)  ?  1  :  -1];")
    lines.append("int main(void) { return 0; }")
    src = os.path.join(str(tmp_path), "adpcm_proto_check.c")
    open(src, "w").write("\n".join(lines) + "\n")
    run(["gcc", "-std=gnu99", "-fsyntax-only", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-Wno-unused-variable",
         "-DHAVE_STDBOOL_H", "-DHAVE_INTTYPES_H", "-DHAVE_STDINT_H", "-I" + REF, src])
    mine = open(os.path.join(ROOT, "include", "spangpu_spandsp.h")).read()
    assert re.search(r"IMA_ADPCM_IMA4 = 0,\s*IMA_ADPCM_DVI4 = 1,\s*IMA_ADPCM_VDVI = 2", mine)
    assert (engine.IMA_ADPCM_IMA4, engine.IMA_ADPCM_DVI4, engine.IMA_ADPCM_VDVI) == (0, 1, 2)


def _ima(n, variants, chunks, count=None):
    v, k = (np.asarray(x, np.int32) for x in (variants, chunks))
    h = C.c_void_p()
    return engine.lib().spangpu_ima_adpcm_create(C.byref(h), 0, n, v.ctypes.data, k.ctypes.data, len(v) if count is None else count), h


def _oki(n, rates, count=None):
    r = np.asarray(rates, np.int32)
    h = C.c_void_p()
    return engine.lib().spangpu_oki_adpcm_create(C.byref(h), 0, n, r.ctypes.data, len(r) if count is None else count), h


def test_no_device_is_an_error_not_a_fallback(built):
    L = engine.lib()
    L.ima_adpcm_init.restype = C.c_void_p
    L.ima_adpcm_init.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.oki_adpcm_init.restype = C.c_void_p
    L.oki_adpcm_init.argtypes = [C.c_void_p, C.c_int]
    for (rc, h), destroy in ((_ima(8, [1], [0]), L.spangpu_ima_adpcm_destroy), (_oki(8, [32000, 24000]), L.spangpu_oki_adpcm_destroy)):
        if engine.device_count() > 0:
            assert rc == 0 and h.value
            destroy(h)
        else:
            assert rc == NO_DEVICE and not h.value
    if engine.device_count() == 0:
        assert L.ima_adpcm_init(None, 1, 0) is None and L.oki_adpcm_init(None, 32000) is None
        for make in (lambda: engine.ImaAdpcmBank(8), lambda: engine.OkiAdpcmBank(8, [32000, 24000])):
            with pytest.raises(engine.SpanGpuError) as ei:
                make()
            assert ei.value.code == NO_DEVICE


def test_bad_arguments_are_refused(built):
    L = engine.lib()
    # before any device is looked for: a variant outside the three, the rates oki_adpcm_init() refuses
    for variants, chunks in (([3], [0]), ([-1], [0]), ([0, 1, 2, 3], [0, 0, 0, 0])):
        rc, h = _ima(8, variants, chunks)
        assert rc == BAD_ARG and not h.value, variants
    for rates in ([0], [16000], [40000], [8000], [32000, 24001]):
        rc, h = _oki(8, rates)
        assert rc == BAD_ARG and not h.value, rates
    assert _ima(0, [0], [0])[0] == BAD_ARG and _oki(0, [32000])[0] == BAD_ARG
    assert _ima(-1, [0], [0])[0] == BAD_ARG and _oki(-1, [32000])[0] == BAD_ARG
    assert _ima(8, [0], [0], 0)[0] == BAD_ARG and _oki(8, [32000], 0)[0] == BAD_ARG
    r = np.array([0], np.int32)
    h = C.c_void_p()
    assert L.spangpu_ima_adpcm_create(None, 0, 8, r.ctypes.data, r.ctypes.data, 1) == BAD_ARG
    assert L.spangpu_ima_adpcm_create(C.byref(h), 0, 8, None, r.ctypes.data, 1) == BAD_ARG
    assert L.spangpu_ima_adpcm_create(C.byref(h), 0, 8, r.ctypes.data, None, 1) == BAD_ARG
    assert L.spangpu_oki_adpcm_create(None, 0, 8, r.ctypes.data, 1) == BAD_ARG
    assert L.spangpu_oki_adpcm_create(C.byref(h), 0, 8, None, 1) == BAD_ARG
    for f in FAMILIES:
        g = lambda name: getattr(L, "spangpu_%s_%s" % (f, name))  # noqa: E731
        for name in ("channels", "sync", "state_words"):
            assert g(name)(None) == BAD_ARG
        assert g("set_stream")(None, None) == BAD_ARG
        assert g("encode")(None, None, 0, 0, None, 8, None, 0, 0, None) == BAD_ARG
        assert g("decode")(None, None, 0, 0, None, 8, None, 0, 0, None) == BAD_ARG
        assert g("encode_capacity")(None, 8) == BAD_ARG and g("decode_capacity")(None, 8) == BAD_ARG
        assert g("counts_dev")(None) is None
        assert g("get_state")(None, 0, None) == BAD_ARG and g("set_state")(None, 0, None) == BAD_ARG
        g("destroy")(None)
    assert L.spangpu_ima_adpcm_restart(None, 0, 0, 0) == BAD_ARG and L.spangpu_oki_adpcm_restart(None, 0, 32000) == BAD_ARG
    # the by-name calls on nothing
    L.ima_adpcm_init.restype = C.c_void_p
    L.ima_adpcm_init.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.oki_adpcm_init.restype = C.c_void_p
    L.oki_adpcm_init.argtypes = [C.c_void_p, C.c_int]
    assert L.ima_adpcm_init(None, 3, 0) is None and L.ima_adpcm_init(None, -1, 64) is None
    for rate in (0, 16000, 64000):
        assert L.oki_adpcm_init(None, rate) is None
    for f in FAMILIES:
        assert getattr(L, f + "_release")(None) == 0 and getattr(L, f + "_free")(None) == 0
        assert getattr(L, f + "_encode")(None, None, None, 8) == 0 and getattr(L, f + "_decode")(None, None, None, 8) == 0


@pytest.mark.parametrize("family", [AL.IMA, AL.OKI])
def test_fixture_covers_what_it_has_to(family):
    name = AL.NAMES[family]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) <= 478071
    g = AL.load(family)
    cs = AL.cases(g)
    assert tuple(g["schedule"].tolist()) == AL.SCHEDULE and g["offsets"].shape == (AL.WORDS[family], 2)
    got = AL.COVERAGE[family](cs)
    assert len(got) >= 10 and all(got.values()), [n for n, ok in got.items() if not ok]
    # clear of where the bank and the reference part: no call of length 0, no short header call, no header step_index above 88
    for c in cs:
        at = 0
        for n, count, w in c.calls:
            assert n > 0
            if family == AL.IMA and c.kind == AL.DECODE and c.b == 0:
                assert n >= 4 and int(c.data[at + 2]) <= 88
            at += n
        assert at == len(c.data)


def test_step_functions_on_the_host_under_sanitizers(host_program, tmp_path):
    cs = AL.cases(AL.load(AL.IMA)) + AL.cases(AL.load(AL.OKI))
    data = os.path.join(str(tmp_path), "cases.txt")
    n = AL.dump_text(data, cs)
    assert n == 25 and sum(1 for c in cs if c.recut) >= 12
    # some call reached each capacity function exactly or within one unit; none passed it (the program stops on that)
    assert all(0 <= s <= 1 for s in run_cases(host_program, data, n))


def test_by_name_objects_transcript(tmp_path):
    """csrc/shim_adpcm.c over the stand-in bank of tests/adpcm_bank_stub.c, in the manner of tests/test_lone_objects.py: life in
    caller storage and on the heap, failed init leaving storage unchanged, pieces of 0, 1, 4095, 4096, 4097 and 8195 (the shim
    built with a piece of 4096 instead of 2^24, so that the loop is walked), and NULL."""
    exe = os.path.join(str(tmp_path), "adpcm_objects")
    cmd = ["gcc", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           "-DADPCM_PIECE=4096", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "shim_adpcm.c"),
           os.path.join(ROOT, "tests", "adpcm_bank_stub.c"), os.path.join(ROOT, "tests", "c_callers", "adpcm_objects.c"), "-o", exe, "-lm"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr
    want = open(os.path.join(ROOT, "tests", "golden", "adpcm_objects.txt")).read()
    got = p.stdout.splitlines()
    for i, (g, w) in enumerate(zip(got, want.splitlines())):
        assert g == w, "line %d" % (i + 1)
    assert p.stdout == want
    assert "storage changed" not in p.stdout and "WRITTEN" not in p.stdout
    assert p.stdout.count("storage unchanged after failed init") == 2
    assert got[-1] == "live banks at the end: 0"


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference is not here (GPU box)")
@pytest.mark.parametrize("family", [AL.IMA, AL.OKI])
def test_generated_lines_against_the_live_reference(host_program, tmp_path, family):
    """2 000 generated lines a family (random configurations, random call cuts, amplitudes from silence to full scale; every
    third decoder on random bytes) through the host-compiled step functions against the reference, built here as the fixture
    generator builds it.  Everything must be equal."""
    L, offsets = AL.build_reference(REF, str(tmp_path))
    cs = AL.generated_cases(L, offsets, family, SWEEP_LINES, 0xAD9C + family)
    assert len(cs) == 2*SWEEP_LINES and {(c.a, bool(c.b)) for c in cs} == {(a, bool(b)) for a, b in AL.CONFIGS[family]}
    data = os.path.join(str(tmp_path), "sweep.txt")
    n = AL.dump_text(data, cs)
    slack = run_cases(host_program, data, n)
    assert all(s >= 0 for s in slack)
