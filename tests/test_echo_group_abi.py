"""The echo group boundary without a GPU: the new names are exported and declared, and nothing is made without a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BANK_NAMES = ["spangpu_echo_update_var", "spangpu_echo_hpf_tx_channel", "spangpu_echo_reset_channel"]
GROUP_NAMES = ["spangpu_echo_group_create", "spangpu_echo_group_destroy", "spangpu_echo_group_flush", "spangpu_echo_group_ticks",
               "spangpu_echo_group_bank", "spangpu_echo_can_attach", "spangpu_echo_can_pending"]


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"SPANGPU_API\s+[^;(]*?\b(\w+)\s*\(", text))


def test_new_names_are_declared_and_exported(built):
    from spandsp_amd import engine
    L = C.CDLL(engine.LIB_PATH)
    assert set(BANK_NAMES) <= _declared("spangpu.h")
    assert set(GROUP_NAMES) <= _declared("spangpu_spandsp.h")
    for n in BANK_NAMES + GROUP_NAMES:
        assert hasattr(L, n), n
    engine.lib()                                            # ... and the harness binds them


def test_no_group_without_a_device(built):
    import pytest
    from spandsp_amd import engine
    if engine.device_count() > 0:
        pytest.skip("a GPU is visible")
    assert not engine.lib().spangpu_echo_group_create(0, 64, 128, 160)
    with pytest.raises(engine.SpanGpuError) as ei:
        engine.EchoGroup(64, 128, 160)
    assert ei.value.code == -1                              # SPANGPU_ERR_NO_DEVICE


def test_group_arguments_are_checked(built):
    from spandsp_amd import engine
    L = engine.lib()
    assert not L.spangpu_echo_group_create(0, 0, 128, 160)
    assert not L.spangpu_echo_group_create(0, 64, 128, 0)
    assert L.spangpu_echo_group_flush(None) == -2
    assert L.spangpu_echo_group_destroy(None) == 0
    assert L.spangpu_echo_group_ticks(None) == 0
    assert not L.spangpu_echo_group_bank(None)
    assert not L.spangpu_echo_can_attach(None, 0, 1)
    assert L.spangpu_echo_can_pending(None) == 0
