"""The FAX transmit front-end banks without a GPU: the exported names and their declarations, the C ABI's behaviour where there
is no device, the situations tests/golden/faxtx.npz has to hold, and the per-channel step functions of
spandsp_amd/csrc/faxtx_dev.hpp -- with hdlc_tx_get_bit() of hdlc_dev.hpp as the senders' bit source -- run on the host, under
sanitizers, over every tick of the fixture."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import faxtx_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"spangpu_faxtx_" + n for n in (
    "create", "destroy", "channels", "set_stream", "sync", "set_tx_type", "restart", "set_tep_mode", "tx", "status", "framer",
    "fast_bank", "v21_bank", "tone_bank", "state_words", "get_words", "set_words")}
SPAN_NAMES = {"spangpu_txspans_modem", "spangpu_txspans_fsk", "spangpu_txspans_mct"}
LINE_NAMES = {"spangpu_txline_modem_set_state", "spangpu_txline_modem_ring_words", "spangpu_txline_modem_ring_rw", "spangpu_txline_modem_init",
              "spangpu_txline_fsk_set_state", "spangpu_txline_mct_set_state"}
ERR_NO_DEVICE, ERR_BAD_ARG, ERR_UNSUPPORTED = -1, -2, -6
SITUATIONS = ("pause_short_return", "ced_ends_in_mid_tick", "cng_replaced_by_v21", "v21_starts_at_120_of_tick_4", "silence_ends_on_a_rows_end",
              "odd_start_111", "v21_end_in_mid_tick_160", "v21_end_in_mid_tick_200", "v21_end_in_mid_tick_163", "v29_hdlc_shutdown_then_zero",
              "non_ecm_v29_7200", "non_ecm_v27ter_4800", "non_ecm_v27ter_2400", "v17_init_restart_short_train", "v29_v17_v29_init_each_time",
              "tep", "same_type_twice", "done", "loop", "restart_while_tone_runs")


@pytest.fixture(scope="module")
def cases():
    return TC.load()


def test_symbols_are_exported_and_declared(built):
    from spandsp_amd import engine
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3}
    assert {n for n in exported if "faxtx" in n and not n.startswith("_Z")} == NAMES
    assert {n for n in exported if n.startswith("spangpu_txspans_")} == SPAN_NAMES
    assert {n for n in exported if n.startswith("spangpu_txline_")} == LINE_NAMES
    text = open(os.path.join(ROOT, "include", "spangpu.h")).read()
    for prefix, names in (("faxtx", NAMES), ("txspans", SPAN_NAMES), ("txline", LINE_NAMES)):
        declared = set(re.findall(r"SPANGPU_API\s+[\w\s\*]+?\b(spangpu_%s_\w+)\s*\(" % prefix, text))
        assert declared == names, prefix
    L = engine.lib()
    for n in NAMES | SPAN_NAMES | LINE_NAMES:
        assert getattr(L, n).argtypes is not None, n


def test_receive_section_no_longer_lists_the_transmit_half():
    text = open(os.path.join(ROOT, "include", "spangpu.h")).read()
    assert "Not here: the transmit half" not in text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "FaxTxFrontEnd" in design or "spangpu_faxtx_t" in design


def test_no_device_and_bad_arguments(built):
    from spandsp_amd import engine
    L = engine.lib()
    h = C.c_void_p()
    every = engine.FAXFE_V27TER | engine.FAXFE_V29 | engine.FAXFE_V17
    for n_ch, mask, max_samples in ((4, 8, 160), (4, every | 16, 160), (4, -1, 160), (0, every, 160), (4, every, 0), (4, every, (1 << 24) + 1)):
        assert L.spangpu_faxtx_create(C.byref(h), 0, n_ch, mask, max_samples, 0) == ERR_BAD_ARG, (n_ch, mask, max_samples)
        assert not h.value
    assert L.spangpu_faxtx_create(None, 0, 4, every, 160, 0) == ERR_BAD_ARG
    for fn, args in (("set_tx_type", (None, 0, engine.T30_MODEM_V21, 300, 0, 1)), ("restart", (None, 0)), ("set_tep_mode", (None, 0, 1)),
                     ("tx", (None, None, 0, 160, 160)), ("status", (None, None, None, None, None, None)), ("set_stream", (None, None)),
                     ("sync", (None,)), ("get_words", (None, 0, None)), ("set_words", (None, 0, None)), ("channels", (None,)),
                     ("state_words", (None,))):
        assert getattr(L, "spangpu_faxtx_" + fn)(*args) == ERR_BAD_ARG, fn
    for fn, args in (("framer", (None,)), ("fast_bank", (None, engine.V29)), ("v21_bank", (None,)), ("tone_bank", (None, 2))):
        assert not getattr(L, "spangpu_faxtx_" + fn)(*args), fn
    assert L.spangpu_txspans_modem(None, None, 160, 160, None, 5, None, None, None, None) == ERR_BAD_ARG
    assert L.spangpu_txspans_fsk(None, None, 160, 160, None, 3, None, None, None) == ERR_BAD_ARG
    assert L.spangpu_txspans_mct(None, None, 160, 160, None, 1, None) == ERR_BAD_ARG
    for n in sorted(LINE_NAMES - {"spangpu_txline_modem_ring_words", "spangpu_txline_modem_ring_rw", "spangpu_txline_modem_init"}):
        assert getattr(L, n)(None, 0, None) == ERR_BAD_ARG, n
    assert L.spangpu_txline_modem_ring_words(None) == ERR_BAD_ARG
    assert L.spangpu_txline_modem_ring_rw(None, 0, None, 0) == ERR_BAD_ARG
    assert L.spangpu_txline_modem_init(None, 0, 9600, 0) == ERR_BAD_ARG
    if engine.device_count() <= 0:
        assert L.spangpu_faxtx_create(C.byref(h), 0, 4, every, 160, 0) == ERR_NO_DEVICE
        assert not h.value
        with pytest.raises(engine.SpanGpuError):
            engine.FaxTxFrontEnd(4)


def test_fixture_holds_every_situation(cases):
    cs, flags = cases
    assert set(flags) == set(SITUATIONS), sorted(set(flags) ^ set(SITUATIONS))
    assert all(v == 1 for v in flags.values()), flags
    assert os.path.getsize(TC.GOLDEN) <= 478071
    d = dict(cs)
    assert {int(c["cfg"][2]) for c in d.values()} == {160, 200, 163}
    # what the flags stand for, looked at again from the records
    c = d["v21_160"]
    assert [tuple(x) for x in TC.tick(c, "calls", 3)] == [(TC.H_SILENCE, 160, 120), (TC.H_V21, 40, 40)]
    c = d["v21_200"]
    assert [tuple(x) for x in TC.tick(c, "calls", 2)] == [(TC.H_SILENCE, 200, 200)] and c["handler"][2] == TC.H_SILENCE
    assert [tuple(x) for x in TC.tick(c, "calls", 3)] == [(TC.H_SILENCE, 200, 0), (TC.H_V21, 200, 200)]
    for name in ("v21_160", "v21_200", "v21_163"):
        assert d[name]["under"].sum() == 1 and -7 in d[name]["asked"]
    assert [int(p) for p, o in zip(d["v17"]["path"], d["v17"]["ops"]) if o[1] == TC.SET] == [2, 3, 3]
    assert int(d["v27ter_tep"]["cfg"][0]) == 1
    assert "rx_recs" in d["loop"] and [int(x) & 0xFFFF for x in d["loop"]["rx_recs"] if x >= 0x10000] == [5, 7, 40, 5]
    # no tick of any case has more than one sender call, and silence comes first: what the plan / senders / resolve sequence rests on
    for name, c in cs:
        for t in range(int(c["cfg"][1])):
            which = [int(x[0]) for x in TC.tick(c, "calls", t)]
            senders = [w for w in which if w != TC.H_SILENCE]
            assert len(senders) <= 1 and (not senders or which[-1] == senders[0]), (name, t, which)


def test_step_functions_and_bit_source_on_the_host_under_sanitizers(cases, tmp_path):
    cs, _ = cases
    exe = os.path.join(str(tmp_path), "faxtx_host")
    data = os.path.join(str(tmp_path), "cases.txt")
    n = TC.dump_text(data, cs)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           os.path.join(ROOT, "tests", "c_callers", "faxtx_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    p = subprocess.run([exe, data], capture_output=True, text=True)
    out = p.stdout + p.stderr
    bits = sum(len(c["asked"]) for _, c in cs)
    assert p.returncode == 0 and "ok %d cases" % n in out and "%d bits" % bits in out, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    assert bits > 5000
