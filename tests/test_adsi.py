"""The caller-ID banks without a GPU: the exported names, the by-name prototypes against the reference's adsi.h, the host-only
helpers (message packing, adsi_add_field, adsi_next_field) against the committed fixture byte for byte and return for
return -- through the library and through a stand-alone program built with the address and undefined-behaviour sanitizers
over csrc/adsi_host.c alone -- and the C ABI's behaviour where there is no device."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import adsi_lines as AL
from spandsp_amd import engine
from test_c_callers import REF, _prototypes, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "adsi_fsk.npz")
NO_DEVICE, BAD_ARG = -1, -2
NAMES = {"adsi_rx_get_logging_state", "adsi_rx_init", "adsi_rx_release", "adsi_rx_free", "adsi_rx", "adsi_tx_get_logging_state", "adsi_tx_init",
         "adsi_tx_release", "adsi_tx_free", "adsi_tx_set_preamble", "adsi_tx", "adsi_tx_send_alert_tone", "adsi_tx_put_message",
         "adsi_next_field", "adsi_add_field", "adsi_standard_to_str"}
TX_CALLS = ["create", "destroy", "channels", "set_stream", "sync", "put_message", "set_preamble", "send_alert_tone", "restart", "state_words",
            "get_state", "set_state", "get_message", "set_message"]
RX_CALLS = ["create", "destroy", "channels", "set_stream", "sync", "var", "messages", "msg_capacity", "restart", "state_words", "get_state",
            "set_state", "get_message", "set_message"]
CLIP_DTMF_FIELDS = [(ord("#"), b""), (ord("A"), b"0123456789"), (0, b"4455")]
TDD_FIELDS = [(0, b"Hello 123, ok? go"), (0, b"\n#9 z")]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def cases(g):
    """(standard, case name, the fields it was built from) for every pack_* entry of the fixture"""
    out = []
    for s in AL.STANDARDS:
        for name, fields in sorted(AL.FIELD_CASES.items()):
            out.append((s, name, fields(s)))
    return out + [(5, "cid", CLIP_DTMF_FIELDS), (6, "cid", TDD_FIELDS)]


def test_symbols_are_exported(built):
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines()}
    want = NAMES | {"spangpu_adsi_tx"} | {"spangpu_adsi_tx_" + c for c in TX_CALLS} | {"spangpu_adsi_rx"} | {"spangpu_adsi_rx_" + c for c in RX_CALLS}
    want |= {"spangpu_adsi_pack_message", "spangpu_adsi_add_field", "spangpu_adsi_next_field", "spangpu_adsi_standard_to_str"}
    assert not want - have, sorted(want - have)


def test_every_adsi_name_is_declared(built):
    assert {p[0] for p in _prototypes("spangpu_spandsp.h", "SPANGPU_ADSI_API")} == NAMES
    # ... and is out of the way of the check over the fixed list of reference headers (tests/test_c_callers.py does not
    # include adsi.h, so these names have a check of their own below)
    assert not NAMES & {p[0] for p in _prototypes("spangpu_spandsp.h", "SPANGPU_API")}


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference's headers are not here (GPU box)")
def test_adsi_prototypes_are_the_references(built, tmp_path):
    ref_text = open(os.path.join(REF, "spandsp", "adsi.h")).read()
    declared = set(re.findall(r"SPAN_DECLARE\([^)]*\)\s*(\w+)\s*\(", ref_text))
    assert declared == NAMES
    lines = ["#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>", "#include <stdio.h>", "#include <stdbool.h>"]
    for h in ("telephony", "logging", "async", "adsi"):
        lines.append('#include "spandsp/%s.h"' % h)
    for name, ret, args in _prototypes("spangpu_spandsp.h", "SPANGPU_ADSI_API"):
        lines.append("static %s (*chk_%s)(%s) = %s;" % (ret, name, args, name))
    lines.append("int main(void) { return 0; }")
    src = os.path.join(str(tmp_path), "adsi_proto_check.c")
    open(src, "w").write("\n".join(lines) + "\n")
    run(["gcc", "-std=gnu99", "-fsyntax-only", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-Wno-unused-variable",
         "-DHAVE_STDBOOL_H", "-DHAVE_INTTYPES_H", "-DHAVE_STDINT_H", "-I" + REF, src])


def test_helpers_equal_the_fixture(built, golden):
    g = golden
    seen = 0
    for s, name, fields in cases(g):
        key = "pack_%d_%s" % (s, name)
        msg = b""
        shift = [2 if s == 6 else 0]      # start_tx() schedules an explicit shift for a TDD sender
        for t, body in fields:
            msg = engine.adsi_add_field(s, msg, t, body, shift)
        assert msg == g[key + "_msg"].tobytes(), key
        if s <= 4:
            assert engine.adsi_pack_message(s, msg) == g[key + "_packed"].tobytes(), key
            walked = g[key + "_seen"].tobytes()
        else:
            walked = msg
        assert engine.adsi_fields(s, walked) == [tuple(int(x) for x in row) for row in g[key + "_walk"]], key
        assert len(g[key + "_walk"]) >= 2 and g[key + "_walk"][-1][0] < 0
        seen += 1
    assert seen == 18
    # the stuffing branch: a J-CLIP body of DLE (0x10) bytes has its length byte doubled
    packed = g["pack_4_dle_packed"]
    assert packed[6] & 0x7F == 0x10 and packed[7] & 0x7F == 0x10 and len(packed) == len(g["pack_4_dle_msg"]) + 10
    for s in AL.STANDARDS:
        (longest, over), (ok, refused) = g["tx_long_%d" % s]
        assert len(engine.adsi_pack_message(s, bytes((i*3 + 1) & 0x7F for i in range(longest)))) > longest and ok == longest
        assert engine.adsi_pack_message(s, bytes(over)) == -1 and refused == -1
    assert [engine.lib().spangpu_adsi_standard_to_str(s) for s in range(0, 8)] == [b"???", b"CLASS", b"CLIP", b"A-CLIP", b"J-CLIP", b"CLIP-DTMF",
                                                                                   b"TDD", b"???"]
    out = np.zeros(256, np.uint8)
    for args in ((0, b"ab", 2, 256), (5, b"ab", 2, 256), (1, b"a", 1, 256), (1, b"ab", 2, 255)):
        assert engine.lib().spangpu_adsi_pack_message(args[0], args[1], args[2], out.ctypes.data, args[3]) == BAD_ARG


def dump_cases(g, path):
    recs = []
    for s, name, fields in cases(g):
        key = "pack_%d_%s" % (s, name)
        msg = g[key + "_msg"].tobytes()
        r = struct.pack("<III", 1, s, len(fields))
        for t, body in fields:
            r += struct.pack("<II", t, len(body)) + body
        recs.append(r + struct.pack("<I", len(msg)) + msg)
        if s <= 4:
            packed = g[key + "_packed"].tobytes()
            recs.append(struct.pack("<III", 0, s, len(msg)) + msg + struct.pack("<i", len(packed)) + packed)
            walked = g[key + "_seen"].tobytes()
        else:
            walked = msg
        rows = g[key + "_walk"]
        recs.append(struct.pack("<III", 2, s, len(walked)) + walked + struct.pack("<I", len(rows)) + rows.astype("<i4").tobytes())
    for s in AL.STANDARDS:
        # the maximum lengths: the longest message each standard takes, and one byte more
        (longest, over), _ = g["tx_long_%d" % s]
        msg = bytes((i*3 + 1) & 0x7F for i in range(over))
        packed = engine.adsi_pack_message(s, msg[:longest])
        recs.append(struct.pack("<III", 0, s, longest) + msg[:longest] + struct.pack("<i", len(packed)) + packed)
        recs.append(struct.pack("<III", 0, s, over) + msg + struct.pack("<i", -1))
    open(path, "wb").write(struct.pack("<I", len(recs)) + b"".join(recs))
    return len(recs)


def test_stand_alone_program_under_sanitizers(built, golden, tmp_path):
    exe = os.path.join(str(tmp_path), "adsi_fields")
    data = os.path.join(str(tmp_path), "cases.bin")
    n = dump_cases(golden, data)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_callers", "adsi_fields.c"),
           os.path.join(ROOT, "spandsp_amd", "csrc", "adsi_host.c"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    p = subprocess.run([exe, data], capture_output=True, text=True)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "%d cases: ok" % n in out and "Sanitizer" not in out and "runtime error" not in out, out


def test_python_restatement_of_the_lines_equals_the_fixture(built, golden):
    # tests/adsi_lines.py renders the receiver lines from its own packing: it has to be the reference's
    for s in AL.STANDARDS:
        for name, fields in AL.FIELD_CASES.items():
            key = "pack_%d_%s" % (s, name)
            assert AL.build(s, fields(s)) == golden[key + "_msg"].tobytes()
            assert AL.pack(s, golden[key + "_msg"].tobytes()) == golden[key + "_packed"].tobytes()


def test_no_device_is_an_error_not_a_fallback(built):
    s = np.array([1, 2, 3, 4], np.int32)
    for create, destroy in ((engine.lib().spangpu_adsi_tx_create, engine.lib().spangpu_adsi_tx_destroy),
                            (engine.lib().spangpu_adsi_rx_create, engine.lib().spangpu_adsi_rx_destroy)):
        h = C.c_void_p()
        rc = create(C.byref(h), 0, 8, s.ctypes.data, 4)
        if engine.device_count() > 0:
            assert rc == 0 and h.value
            destroy(h)
        else:
            assert rc == NO_DEVICE and not h.value


def test_excluded_standards_are_refused(built):
    for bad in (0, 5, 6, 7):
        s = np.array([1, bad], np.int32)
        for create in (engine.lib().spangpu_adsi_tx_create, engine.lib().spangpu_adsi_rx_create):
            h = C.c_void_p()
            assert create(C.byref(h), 0, 8, s.ctypes.data, 2) == BAD_ARG
            assert not h.value
