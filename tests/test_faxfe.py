"""The FAX receive front-end banks without a GPU: the exported names and their declarations, the C ABI's behaviour where
there is no device, what tests/golden/faxfe.npz has to cover, and the per-channel route and dc_restore functions of
spandsp_amd/csrc/faxfe_dev.hpp run on the host, under sanitizers, over every tick of the fixture."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import faxfe_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"spangpu_faxfe_" + n for n in (
    "create", "destroy", "channels", "set_stream", "sync", "start_slow_modem", "start_fast_modem", "rx", "frames", "put_bits",
    "capacities", "handlers", "fast_bank", "v21_bank", "framer", "state_words", "get_words", "set_words")}
ERR_NO_DEVICE, ERR_BAD_ARG, ERR_UNSUPPORTED = -1, -2, -6


@pytest.fixture(scope="module")
def cases():
    return FC.load()


def test_symbols_are_exported_and_declared(built):
    from spandsp_amd import engine
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3}
    # (the kernels' handles are C++ names, like the other banks')
    assert {n for n in exported if "faxfe" in n and not n.startswith("_Z")} == NAMES
    assert {"spangpu_modem_rx_lens_dev", "spangpu_fsk_rx_lens_dev"} <= exported
    text = open(os.path.join(ROOT, "include", "spangpu.h")).read()
    declared = set(re.findall(r"SPANGPU_API\s+[\w\s\*]+?\b(spangpu_faxfe_\w+)\s*\(", text))
    assert declared == NAMES
    for n in ("spangpu_modem_rx_lens_dev", "spangpu_fsk_rx_lens_dev"):
        assert re.search(r"SPANGPU_API\s+int\s+%s\s*\(" % n, text), n
    # the engine binds every one
    L = engine.lib()
    for n in NAMES:
        assert getattr(L, n).argtypes is not None, n


def test_no_device_and_bad_arguments(built):
    from spandsp_amd import engine
    L = engine.lib()
    h = C.c_void_p()
    every = engine.FAXFE_V27TER | engine.FAXFE_V29 | engine.FAXFE_V17
    # refused before any device work: bad masks, sizes and a missing handle
    for n_ch, mask, max_samples in ((4, 0, 160), (4, 8, 160), (4, every | 16, 160), (4, -1, 160), (0, every, 160), (4, every, 0),
                                    (4, every, (1 << 24) + 1)):
        assert L.spangpu_faxfe_create(C.byref(h), 0, n_ch, mask, max_samples, 0) == ERR_BAD_ARG, (n_ch, mask, max_samples)
        assert not h.value
    assert L.spangpu_faxfe_create(None, 0, 4, every, 160, 0) == ERR_BAD_ARG
    for fn, args in (("start_slow_modem", (None, 0, engine.FAX_MODEM_V21_RX)), ("start_fast_modem", (None, 0, engine.FAX_MODEM_V29_RX, 9600, 0, 0)),
                     ("rx", (None, None, 0, 160, 160)), ("set_stream", (None, None)), ("sync", (None,)), ("handlers", (None, None, None)),
                     ("get_words", (None, 0, None)), ("set_words", (None, 0, None)), ("capacities", (None, None, None, None)),
                     ("channels", (None,)), ("state_words", (None,))):
        assert getattr(L, "spangpu_faxfe_" + fn)(*args) == ERR_BAD_ARG, fn
    for fn in ("fast_bank", "v21_bank", "framer"):
        assert not getattr(L, "spangpu_faxfe_" + fn)(*((None, engine.V29, 0) if fn == "fast_bank" else (None,)))
    assert L.spangpu_modem_rx_lens_dev(None, None, 1, 160, 160, None) == ERR_BAD_ARG
    assert L.spangpu_fsk_rx_lens_dev(None, None, 1, 160, 160, None) == ERR_BAD_ARG
    if engine.device_count() <= 0:
        assert L.spangpu_faxfe_create(C.byref(h), 0, 4, every, 160, 0) == ERR_NO_DEVICE
        assert not h.value
        with pytest.raises(engine.SpanGpuError):
            engine.FaxFrontEnd(4)


def test_fixture_covers_what_it_has_to(cases):
    cs, case11 = cases
    d = dict(cs)
    V21_RX, V17_RX, V27TER_RX, V29_RX = 12, 13, 14, 15
    reached = {}            # fast modem kind -> it reached FAST_ONLY
    paths = set()
    hdlc_modes = set()
    longest = 0
    stays, to_v21, bad_no_switch = False, False, False
    for name, c in cs:
        assert c["cfg"][1] == len(c["lens"]) == len(c["handler"]) and c["lens"].sum() == len(c["amp"])
        kind = 0
        for t in range(len(c["lens"])):
            for op, path in zip(c["ops"], c["path"]):
                if op[0] == t and op[1] == FC.FAST:
                    kind = int(op[2])
                    paths.add(int(path))
                    hdlc_modes.add(int(op[5]))
            if c["handler"][t] == FC.FAST_ONLY:
                reached[kind] = True
            before = c["handler"][t - 1] if t else FC.NONE
            if before == FC.FAST_AND_V21 and c["handler"][t] == FC.V21_ONLY:
                to_v21 = True
            recs = FC.tick(c, "recs", t)
            if ((recs >= 0) & (recs < 0x10000)).any() and not (recs >= 0x10000).any() and before == FC.FAST_AND_V21:
                assert c["handler"][t] == FC.FAST_AND_V21 and c["frx"][t] == 0, (name, t)
                bad_no_switch = True
        good = c["recs"][c["recs"] >= 0x10000] & 0xFFFF
        longest = max(longest, int(good.max(initial=0)))
        stays |= bool((c["handler"] == FC.FAST_AND_V21).all())
    assert reached == {V17_RX: True, V27TER_RX: True, V29_RX: True}
    assert to_v21 and stays and bad_no_switch
    assert paths == {1, 2} and hdlc_modes == {0, 1}
    assert longest >= 200
    assert any(c["cfg"][0] for _, c in cs) and any(c["dc"][0] != 0 for _, c in cs)
    assert any(len(set(c["lens"].tolist())) > 1 for _, c in cs)
    # case 11: training succeeded and a good frame inside one tick, and the handler ends on V.21 -- or its recorded absence
    assert case11 in (0, 1) and (case11 == 1) == ("same_tick" in d)
    if case11:
        c = d["same_tick"]
        t = int(np.nonzero(c["handler"] == FC.V21_ONLY)[0][0])
        assert c["handler"][t - 1] == FC.FAST_AND_V21 and FC.TRAINING_SUCCEEDED in FC.tick(c, "fast", t)
        assert (FC.tick(c, "recs", t) >= 0x10000).any()
    assert os.path.getsize(FC.GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "v17tx.npz"))


def test_route_and_dc_restore_on_the_host_under_sanitizers(built, cases, tmp_path):
    cs, _ = cases
    exe = os.path.join(str(tmp_path), "faxfe_host")
    data = os.path.join(str(tmp_path), "cases.txt")
    n = FC.dump_text(data, cs)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           os.path.join(ROOT, "tests", "c_callers", "faxfe_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    p = subprocess.run([exe, data], capture_output=True, text=True)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "ok %d cases" % n in out, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
