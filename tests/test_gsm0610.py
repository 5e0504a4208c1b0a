"""The GSM 06.10 codec banks without a GPU: the exported names, the by-name prototypes against the reference's gsm0610.h, the C
ABI's behaviour where there is no device, what the committed fixture has to cover, the host packers and unpackers against the
fixture's bytes and fields, and the kernels' per-frame functions (csrc/gsm0610_dev.hpp) compiled for the host into a
stand-alone program, built with the address and undefined-behaviour sanitizers, that runs every case of the fixture one lane
at a time: codes, samples, counts and state words equal the reference's after every call, a second cut of every stream into
calls gives the same stream, and the capacity functions are reached and never passed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gsm0610_lines as GL
from spandsp_amd import engine
from test_c_callers import REF, _prototypes, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE, BAD_ARG = -1, -2
NAMES = {"gsm0610_" + n for n in ("init", "release", "free", "set_packing", "encode", "decode", "pack_none", "pack_wav49", "pack_voip",
                                  "unpack_none", "unpack_wav49", "unpack_voip")}
CALLS = ["create", "destroy", "channels", "set_stream", "sync", "encode", "decode", "encode_capacity", "decode_capacity", "counts_dev",
         "set_packing", "restart", "state_words", "get_state", "set_state"]
BANK_NAMES = {"spangpu_gsm0610_" + c for c in CALLS}


class Frame(C.Structure):
    _fields_ = [("LARc", C.c_int16*8), ("Nc", C.c_int16*4), ("bc", C.c_int16*4), ("Mc", C.c_int16*4), ("xmaxc", C.c_int16*4),
                ("xMc", (C.c_int16*13)*4)]


@pytest.fixture(scope="module")
def golden():
    return GL.load()


def test_symbols_are_exported(built):
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines()}
    assert len(NAMES) == 12 and not (NAMES | BANK_NAMES) - have, sorted((NAMES | BANK_NAMES) - have)
    assert {n for n in have if "gsm0610" in n.lower() and not n.startswith("_Z")} == NAMES | BANK_NAMES


def test_every_entry_point_is_declared(built):
    text = open(os.path.join(ROOT, "include", "spangpu.h")).read()
    declared = set(re.findall(r"SPANGPU_API\s+[\w\s\*]+?\b(spangpu_gsm0610_\w+)\s*\(", text))
    assert declared == BANK_NAMES
    assert {p[0] for p in _prototypes("spangpu_spandsp.h", "SPANGPU_GSM0610_API")} == NAMES
    # ... and out of the way of the check over the fixed list of reference headers (tests/test_c_callers.py)
    assert not NAMES & {p[0] for p in _prototypes("spangpu_spandsp.h", "SPANGPU_API")}


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference's headers are not here (GPU box)")
def test_gsm0610_prototypes_are_the_references(built, tmp_path):
    ref_text = open(os.path.join(REF, "spandsp", "gsm0610.h")).read()
    declared = set(re.findall(r"SPAN_DECLARE\([^)]*\)\s*(\w+)\s*\(", ref_text))
    assert declared == NAMES
    lines = ["#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>", "#include <stdio.h>", "#include <stdbool.h>"]
    for h in ("telephony", "gsm0610"):
        lines.append('#include "spandsp/%s.h"' % h)
    for name, ret, args in _prototypes("spangpu_spandsp.h", "SPANGPU_GSM0610_API"):
        lines.append("static %s (*chk_%s)(%s) = %s;" % (ret, name, args, name))
    lines.append("int main(void) { return 0; }")
    src = os.path.join(str(tmp_path), "gsm0610_proto_check.c")
    open(src, "w").write("\n".join(lines) + "\n")
    run(["gcc", "-std=gnu99", "-fsyntax-only", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-Wno-unused-variable",
         "-DHAVE_STDBOOL_H", "-DHAVE_INTTYPES_H", "-DHAVE_STDINT_H", "-I" + REF, src])
    # the enum a caller's source names has the reference's values (the reference leaves them to the order; written out here)
    mine = open(os.path.join(ROOT, "include", "spangpu_spandsp.h")).read()
    for name, value in (("GSM0610_PACKING_NONE", 0), ("GSM0610_PACKING_WAV49", 1), ("GSM0610_PACKING_VOIP", 2)):
        m = re.search(name + r"\s*=\s*(\w+)", mine)
        assert m and int(m.group(1), 0) == value, name
    m = re.search(r"enum\s*\{\s*GSM0610_PACKING_NONE,\s*GSM0610_PACKING_WAV49,\s*GSM0610_PACKING_VOIP\s*\}", ref_text)
    assert m, "the reference's packing enum is not NONE, WAV49, VOIP from zero"
    assert (engine.GSM0610_PACKING_NONE, engine.GSM0610_PACKING_WAV49, engine.GSM0610_PACKING_VOIP) == (GL.NONE, GL.WAV49, GL.VOIP) == (0, 1, 2)
    # gsm0610_frame_t has the reference's fields in the reference's order
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*gsm0610_frame_t;", ref_text).group(1)
    mine_body = re.search(r"typedef struct\s*\{([^}]*)\}\s*gsm0610_frame_t;", mine).group(1)
    assert re.findall(r"int16_t\s+(\w+(?:\[\d+\])+);", body) == re.findall(r"int16_t\s+(\w+(?:\[\d+\])+);", mine_body) != []


def _create(n, direction, packings):
    p = np.asarray(packings, np.int32)
    h = C.c_void_p()
    return engine.lib().spangpu_gsm0610_create(C.byref(h), 0, n, direction, p.ctypes.data, len(p)), h


def test_no_device_is_an_error_not_a_fallback(built):
    L = engine.lib()
    rc, h = _create(8, engine.GSM0610_ENCODER, [GL.VOIP])
    if engine.device_count() > 0:
        assert rc == 0 and h.value
        L.spangpu_gsm0610_destroy(h)
    else:
        assert rc == NO_DEVICE and not h.value
        L.gsm0610_init.restype = C.c_void_p
        L.gsm0610_init.argtypes = [C.c_void_p, C.c_int]
        assert L.gsm0610_init(None, GL.VOIP) is None


def test_bad_arguments_are_refused(built):
    L = engine.lib()
    # a packing outside the three, a direction that is none: before any device is looked for
    for direction, packings in ((0, [3]), (1, [-1]), (0, [0, 1, 2, 7]), (2, [0]), (-1, [2])):
        rc, h = _create(8, direction, packings)
        assert rc == BAD_ARG and not h.value, (direction, packings)
    rc, h = _create(0, 0, [0])
    assert rc == BAD_ARG
    p = np.array([0], np.int32)
    h = C.c_void_p()
    assert L.spangpu_gsm0610_create(None, 0, 8, 0, p.ctypes.data, 1) == BAD_ARG
    assert L.spangpu_gsm0610_create(C.byref(h), 0, 8, 0, None, 1) == BAD_ARG
    assert L.spangpu_gsm0610_create(C.byref(h), 0, 8, 0, p.ctypes.data, 0) == BAD_ARG
    for call in (L.spangpu_gsm0610_channels, L.spangpu_gsm0610_sync, L.spangpu_gsm0610_state_words):
        assert call(None) == BAD_ARG
    assert L.spangpu_gsm0610_set_stream(None, None) == BAD_ARG
    assert L.spangpu_gsm0610_encode(None, None, 0, 0, None, 160, None, 0, 0, None) == BAD_ARG
    assert L.spangpu_gsm0610_decode(None, None, 0, 0, None, 33, None, 0, 0, None) == BAD_ARG
    assert L.spangpu_gsm0610_encode_capacity(None, 160) == BAD_ARG and L.spangpu_gsm0610_decode_capacity(None, 33) == BAD_ARG
    assert L.spangpu_gsm0610_counts_dev(None) is None
    assert L.spangpu_gsm0610_restart(None, 0, 0) == BAD_ARG and L.spangpu_gsm0610_set_packing(None, 0, 0) == BAD_ARG
    assert L.spangpu_gsm0610_get_state(None, 0, None) == BAD_ARG and L.spangpu_gsm0610_set_state(None, 0, None) == BAD_ARG
    L.spangpu_gsm0610_destroy(None)
    # the by-name calls on nothing
    assert L.gsm0610_release(None) == 0 and L.gsm0610_free(None) == 0 and L.gsm0610_set_packing(None, 0) == -1
    assert L.gsm0610_encode(None, None, None, 160) == 0 and L.gsm0610_decode(None, None, None, 33) == 0


def test_fixture_covers_what_it_has_to(golden):
    g = golden
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "gsm0610.npz")) < 335200
    cs = GL.cases(g)
    for kind in (GL.ENCODE, GL.DECODE):
        for line in range(5):
            assert {c.packing for c in cs if c.kind == kind and c.line == line} == set(GL.PACKINGS)
    assert {c.packing for c in cs if c.line == "rnd" and c.kind == GL.DECODE} == set(GL.PACKINGS)
    # every call has its count and its 160 words, and the schedules are the issue's
    assert all(len(w) == GL.WORDS for c in cs for _, _, w in c.calls)
    assert tuple(g["schedule"]) == (1, 3, 2) and tuple(g["schedule_wav49"]) == (2, 4, 2)
    assert GL.calls(12, GL.VOIP) == [1, 3, 2, 1, 3, 2] and GL.calls(12, GL.WAV49) == [2, 4, 2, 2, 2]
    # the words gsm0610_init() leaves
    for p, w in zip(GL.PACKINGS, g["init"]):
        assert w[GL.W_PACKING] == p and w[GL.W_NRP] == 40 and np.count_nonzero(w) == 1 + (p != 0)
    # the parameters the five lines reach
    c = GL.coverage(g)
    assert c["bc"] == {0, 1, 2, 3} and c["Mc"] == {0, 1, 2, 3}
    assert {40, 120} <= c["Nc"] and min(c["Nc"]) == 40 and max(c["Nc"]) == 120
    assert {0, 63} <= c["xmaxc"]
    assert c["xMc"] == set(range(8))
    assert c["zero_frame"]
    assert c["rnd_lags_out"] >= 1
    # the random unpacked bytes are inside the parameters' widths; the packed ones are any bytes
    assert all(int(v) < (1 << GL.WIDTHS[k % 76]) for k, v in enumerate(GL.random_codes(GL.NONE)))
    # both sets of ratios and a lag other than the first one have been a call's last
    assert {int(w[GL.W_J]) for c in cs for _, _, w in c.calls} == {0, 1}
    assert any(w[GL.W_NRP] != 40 for c in cs if c.kind == GL.DECODE for _, _, w in c.calls)
    # a state word that needs its 32 bits
    assert any(abs(int(w[GL.W_LZ2])) > 32767 for c in cs if c.kind == GL.ENCODE for _, _, w in c.calls)


def _frame_of(params):
    f = Frame()
    p = [int(v) for v in params]
    for i in range(8):
        f.LARc[i] = p[i]
    for j in range(4):
        q = p[8 + 17*j:8 + 17*(j + 1)]
        f.Nc[j], f.bc[j], f.Mc[j], f.xmaxc[j] = q[:4]
        for i in range(13):
            f.xMc[j][i] = q[4 + i]
    return f


def _params_of(f):
    out = list(f.LARc)
    for j in range(4):
        out += [f.Nc[j], f.bc[j], f.Mc[j], f.xmaxc[j]] + list(f.xMc[j])
    return out


def test_host_packers_and_unpackers(built, golden):
    """The six pack / unpack names need no GPU: against the bytes the reference's encoders made and the fields they hold."""
    L = engine.lib()
    for li in range(5):
        params = GL.params_of(golden["codes_none"][li])
        voip = golden["codes_voip"][li].reshape(-1, 33)
        wav49 = golden["codes_wav49"][li].reshape(-1, 65)
        for k, p in enumerate(params):
            f = _frame_of(p)
            buf = (C.c_uint8*76)()
            assert L.gsm0610_pack_none(buf, C.byref(f)) == 76 and list(buf) == p.tolist()
            buf = (C.c_uint8*33)(*([0xFF]*33))
            assert L.gsm0610_pack_voip(buf, C.byref(f)) == 33 and list(buf) == voip[k].tolist(), (li, k)
            back = Frame()
            assert L.gsm0610_unpack_voip(C.byref(back), (C.c_uint8*33)(*voip[k].tolist())) == 33 and _params_of(back) == p.tolist()
            back = Frame()
            assert L.gsm0610_unpack_none(C.byref(back), (C.c_uint8*76)(*p.tolist())) == 76 and _params_of(back) == p.tolist()
        for k in range(len(params)//2):
            pair = (Frame*2)(_frame_of(params[2*k]), _frame_of(params[2*k + 1]))
            buf = (C.c_uint8*65)(*([0xFF]*65))
            assert L.gsm0610_pack_wav49(buf, pair) == 65 and list(buf) == wav49[k].tolist(), (li, k)
            back = (Frame*2)()
            assert L.gsm0610_unpack_wav49(back, (C.c_uint8*65)(*wav49[k].tolist())) == 65
            assert _params_of(back[0]) == params[2*k].tolist() and _params_of(back[1]) == params[2*k + 1].tolist()
    # any bytes: unpack(pack(unpack(bytes))) is unpack(bytes), and the packed bytes come back but for the VoIP nibble
    rnd = GL.random_codes(GL.VOIP).reshape(-1, 33)
    for row in rnd:
        f, buf = Frame(), (C.c_uint8*33)()
        L.gsm0610_unpack_voip(C.byref(f), (C.c_uint8*33)(*row.tolist()))
        L.gsm0610_pack_voip(buf, C.byref(f))
        assert list(buf)[1:] == row.tolist()[1:] and buf[0] == 0xD0 | (row[0] & 0xF)
        assert _params_of(f) == GL.unpack_voip_stream(row).tolist()
    for row in GL.random_codes(GL.WAV49).reshape(-1, 65):
        f, buf = (Frame*2)(), (C.c_uint8*65)()
        L.gsm0610_unpack_wav49(f, (C.c_uint8*65)(*row.tolist()))
        L.gsm0610_pack_wav49(buf, f)
        assert list(buf) == row.tolist()
    # a packer keeps a parameter's low bits: fields wider than their width pack as their low bits do
    wide = _frame_of([0x7FFF]*76)
    narrow = _frame_of([(1 << w) - 1 for w in GL.WIDTHS])
    a, b = (C.c_uint8*33)(), (C.c_uint8*33)()
    L.gsm0610_pack_voip(a, C.byref(wide))
    L.gsm0610_pack_voip(b, C.byref(narrow))
    assert list(a) == list(b)


def test_frame_functions_on_the_host_under_sanitizers(built, golden, tmp_path):
    exe = os.path.join(str(tmp_path), "gsm0610_host")
    data = os.path.join(str(tmp_path), "cases.txt")
    n = GL.dump_text(data, GL.cases(golden))
    assert n == 33
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           os.path.join(ROOT, "tests", "c_callers", "gsm0610_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    p = subprocess.run([exe, data], capture_output=True, text=True)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "ok %d cases" % n in out, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    # calls reached each capacity function; none passed it (the program stops on that)
    m = re.search(r"capacity reached: encode (\d+), decode (\d+) calls", out)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0, out
