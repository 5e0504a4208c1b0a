"""ctypes binding of oracle/_ref/libspandsp_codecs_ref.so -- the reference's G.726, G.722 and GSM 06.10 codecs and its packet
loss concealer, compiled where they lie by oracle/Makefile, behind the batch drivers of oracle/ref_glue/ref_glue_codecs.c.

TEST INFRASTRUCTURE ONLY -- see oracle/__init__.py.  The .so is built where the reference's sources are and travels with the
tree; the sources are never read at run time.

Every run_*() takes ONE line through a schedule of calls inside C and returns (outputs back to back, counts [calls], words).
want: None -- words is [W], the state words after the last call; True -- [calls][W], after every call; a mask [calls] --
[the calls asked for][W], in their order.
"""
import ctypes as C
import os

import numpy as np

from . import HERE

CODECS_SO = os.path.join(HERE, "_ref", "libspandsp_codecs_ref.so")
G726_WORDS, G722_WORDS, GSM0610_WORDS, PLC_WORDS = 30, 74, 160, 404
ENCODE, DECODE = 0, 1
GSM_FRAME = 160

_lib = []


def available():
    return os.path.exists(CODECS_SO)


def lib():
    if not _lib:
        L = C.CDLL(CODECS_SO)
        vp, ci = C.c_void_p, C.c_int
        sigs = {"glue_g726_run": (ci, [ci, ci, ci, ci, vp, vp, ci, vp, vp, vp, vp]),
                "glue_g722_run": (ci, [ci, ci, ci, vp, vp, ci, vp, vp, vp, vp]),
                "glue_gsm0610_run": (ci, [ci, ci, vp, vp, ci, vp, vp, vp, vp]),
                "glue_plc_run": (ci, [vp, vp, vp, ci, vp, vp]),
                "glue_gsm_plc_run": (ci, [vp, vp, ci, vp, vp, vp, vp]),
                "glue_codecs_state_words": (ci, [ci])}
        for name, (res, args) in sigs.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        assert [L.glue_codecs_state_words(k) for k in range(4)] == [G726_WORDS, G722_WORDS, GSM0610_WORDS, PLC_WORDS]
        _lib.append(L)
    return _lib[0]


def _p(a):
    return a.ctypes.data


def _words(n_calls, w, want):
    """(the array the words go to, the mask's address)"""
    if want is None or want is False:
        return np.zeros(w, np.int32), None, None
    mask = np.ones(n_calls, np.int32) if want is True else np.ascontiguousarray(np.asarray(want) != 0, np.int32)
    assert len(mask) == n_calls
    return np.zeros((int(mask.sum()), w), np.int32), mask, mask.ctypes.data


def run_g726(kind, rate, coding, packing, data, lens, want=None):
    """data: encode -- int16 samples (linear) or G.711 bytes; decode -- bytes.  Outputs: bytes, or int16 / G.711 bytes."""
    lens = np.ascontiguousarray(lens, np.int32)
    linear = coding == 0
    data = np.ascontiguousarray(data, np.int16 if (kind == ENCODE and linear) else np.uint8)
    assert int(lens.sum()) <= len(data)
    total = int(lens.sum())
    out = np.zeros((total if kind == ENCODE else 4*total) + 8, np.int16 if (kind == DECODE and linear) else np.uint8)
    counts = np.zeros(len(lens), np.int32)
    words, mask, mp = _words(len(lens), G726_WORDS, want)
    n = lib().glue_g726_run(kind, rate, coding, packing, _p(data), _p(lens), len(lens), _p(out), _p(counts), _p(words), mp)
    assert 0 <= n <= len(out) - 8, (n, rate, coding, packing)
    return out[:n], counts, words


def run_g722(kind, rate, options, data, lens, want=None):
    lens = np.ascontiguousarray(lens, np.int32)
    data = np.ascontiguousarray(data, np.int16 if kind == ENCODE else np.uint8)
    total = int(lens.sum())
    assert total <= len(data)
    out = np.zeros((total if kind == ENCODE else 3*total + 2*len(lens)) + 8, np.uint8 if kind == ENCODE else np.int16)
    counts = np.zeros(len(lens), np.int32)
    words, mask, mp = _words(len(lens), G722_WORDS, want)
    n = lib().glue_g722_run(kind, rate, options, _p(data), _p(lens), len(lens), _p(out), _p(counts), _p(words), mp)
    assert 0 <= n <= len(out) - 8, (n, rate, options)
    return out[:n], counts, words


def run_gsm0610(kind, packing, data, lens, want=None):
    """lens: whole units -- samples (160, 320 under WAV49) for the encoder, bytes (76, 65, 33) for the decoder"""
    lens = np.ascontiguousarray(lens, np.int32)
    data = np.ascontiguousarray(data, np.int16 if kind == ENCODE else np.uint8)
    total = int(lens.sum())
    assert total <= len(data)
    out = np.zeros((total if kind == ENCODE else 5*total) + 8, np.uint8 if kind == ENCODE else np.int16)
    counts = np.zeros(len(lens), np.int32)
    words, mask, mp = _words(len(lens), GSM0610_WORDS, want)
    n = lib().glue_gsm0610_run(kind, packing, _p(data), _p(lens), len(lens), _p(out), _p(counts), _p(words), mp)
    assert 0 <= n <= len(out) - 8, (n, packing)
    return out[:n], counts, words


def run_plc(rows, lens, lost, want=None):
    """rows: the calls' rows one behind the other (int16), what a lost call's row holds being of no account.  Returns (the rows
    after their calls, words)."""
    lens = np.ascontiguousarray(lens, np.int32)
    lost = np.ascontiguousarray(lost, np.int32)
    amp = np.array(rows, np.int16, order="C", copy=True)
    assert len(amp) == int(lens.sum()) and len(lost) == len(lens)
    words, mask, mp = _words(len(lens), PLC_WORDS, want)
    n = lib().glue_plc_run(_p(amp), _p(lens), _p(lost), len(lens), _p(words), mp)
    assert n == len(amp)
    return amp, words


def run_gsm_plc(codes, lost, want=None):
    """codes: the VoIP frames of the ticks that are not lost, 33 bytes each, in order.  Returns (rows [ticks][160], decoder
    words, concealer words)."""
    lost = np.ascontiguousarray(lost, np.int32)
    codes = np.ascontiguousarray(codes, np.uint8)
    heard = int((lost == 0).sum())
    assert len(codes) == 33*heard
    amp = np.zeros((len(lost), GSM_FRAME), np.int16)
    dw, mask, mp = _words(len(lost), GSM0610_WORDS, want)
    pw, _, _ = _words(len(lost), PLC_WORDS, want)
    n = lib().glue_gsm_plc_run(_p(codes), _p(lost), len(lost), _p(amp), _p(dw), _p(pw), mp)
    assert n == heard
    return amp, dw, pw
