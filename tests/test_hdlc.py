"""The HDLC framing banks without a GPU: the exported names and their declarations, the C ABI's behaviour where there is no
device, and the kernels' per-channel step functions (csrc/hdlc_dev.hpp) compiled for the host into a stand-alone program,
built with the address and undefined-behaviour sanitizers, that runs every sender and receiver case of the committed fixture
one lane at a time -- bits, records, octets, statistics and state words equal the reference's -- and then the streams the
capacity function is derived from."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hdlc_cases as HC
from spandsp_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE, BAD_ARG, UNSUPPORTED = -1, -2, -6
RX_CALLS = ["create", "destroy", "channels", "set_stream", "sync", "put_events", "put_modem_events", "put", "records", "capacity",
            "set_max_frame_len", "set_octet_counting_report_interval", "restart", "get_stats", "state_words", "get_state", "set_state",
            "get_buffer", "set_buffer"]
TX_CALLS = ["create", "destroy", "channels", "set_stream", "sync", "frames", "flags", "abort", "end", "queued", "set_max_frame_len", "restart",
            "get_bits", "events", "state_words", "get_state", "set_state", "get_buffer", "set_buffer"]
NAMES = {"spangpu_hdlc_rx_" + c for c in RX_CALLS} | {"spangpu_hdlc_tx_" + c for c in TX_CALLS}


@pytest.fixture(scope="module")
def cases():
    return HC.load()


def test_symbols_are_exported(built):
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines()}
    assert not NAMES - have, sorted(NAMES - have)
    # no other C name: the by-name hdlc_* calls are not part of these banks (the kernels' handles are C++ names, like the
    # other units')
    assert {n for n in have if "hdlc" in n.lower() and not n.startswith("_Z")} == NAMES


def test_every_entry_point_is_declared(built):
    text = open(os.path.join(ROOT, "include", "spangpu.h")).read()
    declared = set(re.findall(r"SPANGPU_API\s+[\w\s\*]+?\b(spangpu_hdlc_\w+)\s*\(", text))
    assert declared == NAMES
    assert "does not order the two streams" in text


def test_fixture_covers_what_it_has_to(cases):
    g, tx, rx, rxb = cases
    assert {(c.crc32, c.iff) for c in tx} >= {(0, 1), (1, 2), (0, 5)}
    lens = {arg for c in tx for _, kind, arg, _, res, _ in c.ops if kind == HC.FRAME and res == 0}
    assert lens >= {1, 2, 3, 255, 400}
    assert any(kind == HC.FRAME and arg == 401 and res == -1 for c in tx for _, kind, arg, _, res, _ in c.ops)
    kinds = {(kind, arg) for c in tx for _, kind, arg, _, res, _ in c.ops if res == 0}
    assert (HC.FLAGS, 32) in kinds and (HC.FLAGS, -3) in kinds and (HC.ABORT, 0) in kinds and (HC.END, 0) in kinds
    assert any(corrupt for c in tx for _, kind, _, corrupt, res, _ in c.ops if res == 0)
    assert sum(sum(c.under) for c in tx) > 0 and sum(sum(c.ended) for c in tx) >= 2
    assert {c.thr for c in rx} >= {1, 2, 5} and {c.interval for c in rx} >= {0, 1, 20} and {c.crc32 for c in rx} == {0, 1}
    codes = {r for c in rx for rs in c.recs for r in rs if r < 0}
    assert codes >= {-1, -2, -3, -4, -5, -6, -7, -8, -11}
    stats = np.array([c.words[-1][13:18] for c in rx])
    assert (stats.sum(axis=0) > 0).all()
    assert len(rxb) >= 5


def test_no_device_is_an_error_not_a_fallback(built):
    L = engine.lib()
    for create, destroy, args in ((L.spangpu_hdlc_rx_create, L.spangpu_hdlc_rx_destroy, (0, 0, 1)),
                                  (L.spangpu_hdlc_tx_create, L.spangpu_hdlc_tx_destroy, (0, 1, 0, 4))):
        h = C.c_void_p()
        rc = create(C.byref(h), 0, 8, *args)
        if engine.device_count() > 0:
            assert rc == 0 and h.value
            destroy(h)
        else:
            assert rc == NO_DEVICE and not h.value


def test_progressive_mode_and_bad_arguments_are_refused(built):
    L = engine.lib()
    h = C.c_void_p()
    assert L.spangpu_hdlc_tx_create(C.byref(h), 0, 8, 0, 1, 1, 4) == UNSUPPORTED and not h.value
    assert b"progressive" in L.spangpu_last_error()
    for args in ((0, 0, 1, 0, 4), (8, 0, 1, 0, 0), (8, 0, 1, 0, 1025), (-1, 0, 1, 0, 4)):
        assert L.spangpu_hdlc_tx_create(C.byref(h), 0, *args) == BAD_ARG and not h.value
    assert L.spangpu_hdlc_tx_create(None, 0, 8, 0, 1, 0, 4) == BAD_ARG
    assert L.spangpu_hdlc_rx_create(C.byref(h), 0, 0, 0, 0, 1) == BAD_ARG and not h.value
    assert L.spangpu_hdlc_rx_create(None, 0, 8, 0, 0, 1) == BAD_ARG
    r, y = C.c_int(0), C.c_int(0)
    assert L.spangpu_hdlc_rx_capacity(-1, C.byref(r), C.byref(y)) == BAD_ARG
    assert L.spangpu_hdlc_rx_capacity(8, None, C.byref(y)) == BAD_ARG
    for call in (L.spangpu_hdlc_rx_sync, L.spangpu_hdlc_tx_sync):
        assert call(None) == BAD_ARG
    assert L.spangpu_hdlc_rx_channels(None) == BAD_ARG and L.spangpu_hdlc_tx_channels(None) == BAD_ARG
    assert L.spangpu_hdlc_rx_put_events(None, 0, None, 1, 8, None) == BAD_ARG
    assert L.spangpu_hdlc_tx_get_bits(None, 0, None, 1, None, 8, None) == BAD_ARG


def test_capacity_is_the_documented_one(built):
    for events in (0, 1, 7, 8, 9, 192, 331, 1 << 20):
        assert engine.hdlc_rx_capacity(events) == (events + events//8 + 1, (403 + events//8 + 3) & ~3)


def test_step_functions_on_the_host_under_sanitizers(built, cases, tmp_path):
    g, tx, rx, rxb = cases
    exe = os.path.join(str(tmp_path), "hdlc_host")
    data = os.path.join(str(tmp_path), "cases.txt")
    n_tx, n_rx = HC.dump_text(data, tx, rx, rxb)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           os.path.join(ROOT, "tests", "c_callers", "hdlc_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    p = subprocess.run([exe, data], capture_output=True, text=True)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "ok %d sender cases" % n_tx in out and "%d receiver cases" % n_rx in out, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    # the streams the capacity is derived from reach it without passing it: one bit that completes an abort with the octet
    # count running is 2 records of 1 + 0 + 1, a carried frame delivered by one bit is 403 octets of 404
    m = re.search(r"capacity reached to (\d+) and (\d+) of 1000", out)
    assert m and int(m.group(1)) == 1000 and int(m.group(2)) == 403*1000//404, out
