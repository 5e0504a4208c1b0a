"""The FSK and connect tone transmitter banks without a device: the exported symbols, argument checks, and the two host
helpers -- spangpu_async_frame_bits() against the reference's async_tx_get_bit(), spangpu_fsktx_bits_due() against the
number of get_bit calls the reference's fsk_tx() makes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fsktx_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_sender_symbol_is_exported(built):
    from spandsp_amd import engine
    text = open(os.path.join(ROOT, "include", "spangpu.h")).read()
    names = sorted(set(re.findall(r"\b(spangpu_(?:fsktx|mcttx|async)_\w+)\s*\(", text)))
    assert len(names) == 27, names
    L = C.CDLL(engine.LIB_PATH)
    for n in names:
        assert hasattr(L, n), n
    by_name = ["fsk_tx_init", "fsk_tx_restart", "fsk_tx_power", "fsk_tx_set_get_bit", "fsk_tx_set_modem_status_handler",
               "fsk_tx_release", "fsk_tx_free", "fsk_tx", "modem_connect_tones_tx_init", "modem_connect_tones_tx_release",
               "modem_connect_tones_tx_free", "modem_connect_tones_tx", "async_tx_init", "async_tx_get_bit",
               "async_tx_presend_bits", "async_tx_release", "async_tx_free"]
    for n in by_name:
        assert hasattr(L, n), n


def test_create_without_a_device_and_bad_arguments(built):
    from spandsp_amd import engine
    makers = [lambda: engine.FskTxBank(engine.FSK_V21CH2, 64), lambda: engine.FskTxBank(engine.FSK_V21CH2, 64, engine.FSKTX_QUEUE),
              lambda: engine.MctTxBank(engine.MCT_ANSAM_PR, 64)]
    for make in makers:
        if engine.device_count() > 0:
            make().close()
        else:
            with pytest.raises(engine.SpanGpuError) as ei:
                make()
            assert ei.value.code == -1          # SPANGPU_ERR_NO_DEVICE
    bad = [lambda: engine.MctTxBank(0, 64), lambda: engine.MctTxBank(6, 64), lambda: engine.MctTxBank(7, 64),
           lambda: engine.MctTxBank(10, 64), lambda: engine.MctTxBank(engine.MCT_FAX_CNG, 0),
           lambda: engine.FskTxBank(engine.FSK_V21CH2, 0), lambda: engine.FskTxBank(engine.FSK_V21CH2, -3),
           lambda: engine.FskTxBank(engine.FSK_V21CH2, 64, 7), lambda: engine.FskTxBank(engine.FSK_V21CH2, 64, engine.FSKTX_QUEUE, None, 0),
           lambda: engine.async_frame_bits(4, 0, 1, b"a"), lambda: engine.async_frame_bits(9, 0, 1, b"a"),
           lambda: engine.async_frame_bits(8, 5, 1, b"a"), lambda: engine.async_frame_bits(8, 0, 0, b"a"),
           lambda: engine.fsktx_bits_due(0, 0, 160), lambda: engine.fsktx_bits_due(30000, 800000, 160),
           lambda: engine.fsktx_bits_due(30000, 0, -1)]
    for make in bad:
        with pytest.raises(engine.SpanGpuError) as ei:
            make()
        assert ei.value.code == -2, ei.value    # SPANGPU_ERR_BAD_ARG
    L = engine.lib()
    assert L.spangpu_fsktx_set_framing(None, 0, 8, 0, 1) == -2
    assert L.spangpu_fsktx_tx(None, 0, None, 0, 0, None) == -2
    assert L.spangpu_mcttx_tx(None, 0, None, 0, 0, None) == -2
    assert L.spangpu_fsktx_state_words() == 13 and L.spangpu_mcttx_state_words() == 4


@pytest.mark.parametrize("presend", [0, 5])
@pytest.mark.parametrize("stop_bits", [1, 2])
@pytest.mark.parametrize("parity", [0, 1, 2, 3])
@pytest.mark.parametrize("data_bits", [5, 6, 7, 8])
def test_async_frame_bits_are_the_references(built, data_bits, parity, stop_bits, presend):
    """All 256 byte values, then idle: the reference's async_tx_get_bit() with a get_byte that hands out the same bytes
    and then SIG_STATUS_LINK_IDLE.  presend_bits marks come first; the idle marks that follow are what an empty bit queue
    sends."""
    from spandsp_amd import engine
    data = bytes(range(256))
    mine = [1]*presend + list(engine.async_frame_bits(data_bits, parity, stop_bits, data)) + [1]*7
    a = fr.RefAsyncTx(data_bits, parity, stop_bits)
    a.presend(presend)
    a.put(data)
    want = [a.get_bit() for _ in range(len(mine))]
    assert len(mine) == presend + 256*(1 + data_bits + (1 if parity else 0) + stop_bits) + 7
    assert mine == want


@pytest.mark.parametrize("which", range(11))
def test_bits_due_counts_the_references_get_bit_calls(built, which):
    """From a fresh state and from the baud_frac earlier calls leave.  V.23 channel 1 and Bell 202 reach
    baud_frac == 800000 exactly at every 20th sample: the reference compares with >=."""
    from spandsp_amd import engine
    rate = fr.BAUD_RATES[which]
    lengths = [1, 5, 6, 7, 8, 20, 77, 160, 333, 1024]
    for n in lengths:
        feed = fr.BitFeed()
        tx = fr.RefFskTx(which, get_bit=feed)
        assert tx.tx(n)[1] == n
        assert engine.fsktx_bits_due(rate, 0, n) == feed.calls, (which, n)
    feed = fr.BitFeed()
    tx = fr.RefFskTx(which, get_bit=feed)
    frac = 0
    for n in lengths + lengths[::-1]:
        before = feed.calls
        assert tx.tx(n)[1] == n
        assert engine.fsktx_bits_due(rate, frac, n) == feed.calls - before, (which, n, frac)
        frac = (frac + n*rate) % 800000
    if which in (2, 6):
        assert engine.fsktx_bits_due(rate, 0, 19) == 2 and engine.fsktx_bits_due(rate, 0, 20) == 3
