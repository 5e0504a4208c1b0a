"""The V.18 text banks without a GPU: the Baudot helpers against the real reference (tests/v18_ref.py) and the committed
fixture, and the C ABI's behaviour where there is no device."""
import ctypes as C

import numpy as np
import pytest

import v18_ref
from spandsp_amd import engine

NO_DEVICE, BAD_ARG = -1, -2
BANK_CALLS = ["create", "destroy", "channels", "set_stream", "sync", "put", "tx", "rx", "rx_var", "fillin", "text", "text_capacity", "restart",
              "state_words", "get_state", "set_state"]


def reference_line(mode, text):
    """(the 5-bit codes on the line, what the far end printed) for a fresh reference sender given `text`"""
    samples, _ = v18_ref.send_all(mode, text)
    far = v18_ref.RefV18(mode)
    printed = b"".join(far.rx(samples[k:k + 160]) for k in range(0, len(samples), 160))
    return v18_ref.line_codes(mode, samples), printed


def check_text(mode, text):
    codes, printed = reference_line(mode, text)
    ours, _ = engine.baudot_encode(text)
    assert np.array_equal(ours, codes), (text, ours, codes)
    back, _ = engine.baudot_decode(ours)
    assert back == printed, (text, back, printed)


@pytest.mark.skipif(not v18_ref.available(), reason="the live reference is not built here; the fixture test below covers the helpers")
def test_baudot_every_code_alone(built):
    for ch in range(128):
        check_text(v18_ref.MODES[ch % 3], bytes([ch]))


@pytest.mark.skipif(not v18_ref.available(), reason="the live reference is not built here; the fixture test below covers the helpers")
@pytest.mark.parametrize("mode", v18_ref.MODES)
def test_baudot_mixed_text(built, mode):
    check_text(mode, v18_ref.MIXED)
    rng = np.random.default_rng(mode)
    check_text(mode, v18_ref.seeded_text(rng, 100))


@pytest.mark.parametrize("mode", v18_ref.MODES)
def test_baudot_against_fixture(built, mode):
    g = v18_ref.golden()
    m = "%04x" % mode
    codes, shift = engine.baudot_encode(g["text_" + m].tobytes())
    assert np.array_equal(codes, g["codes_" + m])
    assert engine.baudot_decode(codes)[0] == g["far_" + m].tobytes()
    # the shift state carries from call to call
    a, s1 = engine.baudot_encode(b"AB1")
    b, s2 = engine.baudot_encode(b"2C", s1)
    assert list(a) == [0x1F, 0x03, 0x19, 0x1B, 0x17] and s1 == 1 and list(b) == [0x13, 0x1F, 0x0E] and s2 == 0


def test_baudot_bad_arguments(built):
    L = engine.lib()
    buf = (C.c_uint8*8)()
    st = C.c_int(0)
    assert L.spangpu_baudot_encode(None, 1, buf, 8, C.byref(st)) == BAD_ARG
    assert L.spangpu_baudot_encode(buf, 1, buf, 8, None) == BAD_ARG
    st.value = 3
    assert L.spangpu_baudot_encode(buf, 1, buf, 8, C.byref(st)) == BAD_ARG
    st.value = 2
    assert L.spangpu_baudot_decode(buf, 1, buf, C.byref(st)) == BAD_ARG
    txt = (C.c_uint8*4)(*b"A1B2")
    st.value = 2
    assert L.spangpu_baudot_encode(txt, 4, buf, 3, C.byref(st)) == BAD_ARG       # eight codes do not fit three


def test_exports(built):
    L = engine.lib()
    for name in BANK_CALLS:
        assert hasattr(L, "spangpu_v18_" + name), name
    assert hasattr(L, "spangpu_baudot_encode") and hasattr(L, "spangpu_baudot_decode")


def test_abi_without_a_device(built):
    L = engine.lib()
    h = C.c_void_p()
    one = (C.c_int32*1)(engine.V18_MODE_WEITBRECHT_5BIT_4545)
    # bad arguments are refused before the device is looked for
    assert L.spangpu_v18_create(None, 0, 4, one, 1, 0) == BAD_ARG
    assert L.spangpu_v18_create(C.byref(h), 0, 0, one, 1, 0) == BAD_ARG
    assert L.spangpu_v18_create(C.byref(h), 0, 4, None, 1, 0) == BAD_ARG
    assert L.spangpu_v18_create(C.byref(h), 0, 4, one, 2, 0) == BAD_ARG
    for bad in (0x0001, 0x0008, 0x0010, 0x0100, 0x1002):
        m = (C.c_int32*1)(bad)
        assert L.spangpu_v18_create(C.byref(h), 0, 4, m, 1, 0) == BAD_ARG, hex(bad)
    buf = (C.c_int16*160)()
    for rc in (L.spangpu_v18_channels(None), L.spangpu_v18_sync(None), L.spangpu_v18_put(None, 0, 1, buf, 1, buf, None),
               L.spangpu_v18_tx(None, 0, buf, 160, 160, None), L.spangpu_v18_rx(None, buf, 0, 160, 160),
               L.spangpu_v18_rx_var(None, buf, 0, buf, 160, 160), L.spangpu_v18_fillin(None, 0, 160), L.spangpu_v18_restart(None, 0, 2),
               L.spangpu_v18_get_state(None, 0, buf), L.spangpu_v18_set_state(None, 0, buf), L.spangpu_v18_state_words(None),
               L.spangpu_v18_set_stream(None, None), L.spangpu_v18_text_capacity(None, 160)):
        assert rc == BAD_ARG
    if engine.device_count() > 0:
        # a device is here: the same call makes a bank, and a device that does not exist is refused
        assert L.spangpu_v18_create(C.byref(h), 1 << 20, 4, one, 1, 0) == BAD_ARG and not h
        return
    assert L.spangpu_v18_create(C.byref(h), 0, 4, one, 1, 0) == NO_DEVICE and not h
    with pytest.raises(engine.SpanGpuError):
        engine.V18Bank(engine.V18_MODE_WEITBRECHT_5BIT_50, 4)
