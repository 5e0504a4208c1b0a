"""ctypes binding of oracle/_ref/libspandsp_adsi_ref.so -- the reference's caller-ID sender and receiver (adsi.c, crc.c and the
fsk, tone_generate, dds .. modules they call), compiled where it lies by oracle/Makefile, behind the batch drivers of
oracle/ref_glue/ref_glue_adsi.c.

TEST INFRASTRUCTURE ONLY -- see oracle/__init__.py.  The .so is built where the reference's sources are and travels with the
tree; the sources are never read at run time.

run_tx() and run_rx() take ONE line through a schedule of calls inside C and return the state words after every call.
"""
import ctypes as C
import os

import numpy as np

from . import HERE

ADSI_SO = os.path.join(HERE, "_ref", "libspandsp_adsi_ref.so")
TX_WORDS, RX_WORDS, FSK_WORDS, MSG = 24, 6, 28, 256
OP_PUT, OP_PREAMBLE, OP_ALERT, OP_RESTART, OP_SHUT_DOWN = 1, 2, 3, 4, 5          # a sender's operations
CLASS, CLIP, ACLIP, JCLIP = 1, 2, 3, 4

_lib = []


def available():
    return os.path.exists(ADSI_SO)


def lib():
    if not _lib:
        L = C.CDLL(ADSI_SO)
        vp, ci = C.c_void_p, C.c_int
        sigs = {"glue_adsi_tx_run": (ci, [ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp]),
                "glue_adsi_rx_run": (ci, [ci, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, vp]),
                "glue_adsi_runs_line": (ci, [ci, vp, ci, ci, ci, vp, ci]),
                "glue_adsi_tx_burst": (ci, [ci, vp, ci, ci, vp, vp, ci]),
                "glue_adsi_impair": (ci, [vp, ci, ci, ci, ci, ci]),
                "glue_adsi_words": (ci, [ci])}
        for name, (res, args) in sigs.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        assert [L.glue_adsi_words(k) for k in range(4)] == [TX_WORDS, RX_WORDS, FSK_WORDS, MSG]
        _lib.append(L)
    return _lib[0]


def _p(a):
    return a.ctypes.data


def run_tx(standard, ops, opbytes, lens):
    """ops: [(call, operation, a0, a1, a2, a3)] sorted by call, a put's a0 / a1 the offset and length of its message in
    opbytes; lens [calls].  Returns (pcm [sum(lens)], zero behind every call's returned length, returned lengths [calls],
    results [ops], words [calls][24], msg [256])."""
    lens = np.ascontiguousarray(lens, np.int32)
    ops = np.ascontiguousarray(np.array(ops, np.int32).reshape(-1, 6))
    opbytes = np.ascontiguousarray(np.frombuffer(bytes(opbytes) + b"\0", np.uint8))
    assert (np.diff(ops[:, 0]) >= 0).all() and (lens >= 0).all()
    pcm = np.zeros(int(lens.sum()) + 1, np.int16)
    out_lens, results = np.zeros(len(lens), np.int32), np.zeros(len(ops) + 1, np.int32)
    words, msg = np.zeros((len(lens), TX_WORDS), np.int32), np.zeros(MSG, np.uint8)
    n = lib().glue_adsi_tx_run(int(standard), _p(ops), len(ops), _p(opbytes), _p(lens), len(lens), _p(pcm), _p(out_lens), _p(results),
                               _p(words), _p(msg))
    assert 0 <= n == int(out_lens.sum()), n
    return pcm[:-1], out_lens, results[:-1], words, msg


def run_rx(standard, amp, lens, bits=False):
    """amp int16, lens [calls] (zeros allowed).  Returns a dict: msgs [(call, bytes)], counts [calls], words [calls][6],
    fsk_words [calls][28], msg [256], and with bits: bits (int8: 0, 1 or a status) and bit_counts [calls]."""
    lens = np.ascontiguousarray(lens, np.int32)
    amp = np.ascontiguousarray(amp, np.int16)
    total = int(lens.sum())
    assert total <= len(amp) and (lens >= 0).all()
    room = total//100 + 4               # (the bit clock allows a message in 120 samples)
    msgs, msg_lens, msg_calls = np.zeros((room, MSG), np.uint8), np.zeros(room, np.int32), np.zeros(room, np.int32)
    counts = np.zeros(len(lens), np.int32)
    words, fsk_words = np.zeros((len(lens), RX_WORDS), np.int32), np.zeros((len(lens), FSK_WORDS), np.int32)
    msg = np.zeros(MSG, np.uint8)
    bit_room = total//3 + 64
    b = np.zeros(bit_room, np.int8) if bits else None
    bit_counts = np.zeros(len(lens), np.int32)
    n = lib().glue_adsi_rx_run(int(standard), _p(amp), _p(lens), len(lens), _p(msgs), _p(msg_lens), _p(msg_calls), room, _p(counts),
                               _p(words), _p(fsk_words), _p(msg), None if b is None else _p(b), bit_room, _p(bit_counts))
    assert 0 <= n <= room and n == int(counts.sum()), n
    out = {"msgs": [(int(msg_calls[i]), msgs[i, :msg_lens[i]].tobytes()) for i in range(n)], "counts": counts, "words": words,
           "fsk_words": fsk_words, "msg": msg}
    if bits:
        out["bits"], out["bit_counts"] = b[:int(bit_counts.sum())].copy(), bit_counts
    return out


def runs_line(standard, runs, num=0, den=0):
    """(bit, samples) runs as a continuous-phase line at the preset's frequencies and level, times num/den (den 0: as it is)"""
    runs = np.ascontiguousarray(np.array(runs, np.int32).reshape(-1, 2))
    room = int(runs[:, 1].sum())
    amp = np.zeros(room + 1, np.int16)
    n = lib().glue_adsi_runs_line(int(standard), _p(runs), len(runs), int(num), int(den), _p(amp), room)
    assert n == room, n
    return amp[:n]


def tx_burst(standard, msg, alert=False, preamble=None):
    """the reference's own sender, from the put to the end of its signal"""
    m = np.frombuffer(bytes(msg), np.uint8).copy()
    pre = None if preamble is None else np.ascontiguousarray(preamble, np.int32)
    room = 160*400
    amp = np.zeros(room, np.int16)
    n = lib().glue_adsi_tx_burst(int(standard), _p(m), len(m), int(alert), None if pre is None else _p(pre), _p(amp), room)
    assert 0 < n < room, n
    return amp[:n].copy()


def impair(amp, num, den, seed=0, noise_dbm0=0):
    """amp*num/den with the reference's AWGN at noise_dbm0 (0 or above: none) on top; a new array"""
    out = np.ascontiguousarray(amp, np.int16).copy()
    assert lib().glue_adsi_impair(_p(out), len(out), int(num), int(den), int(seed), int(noise_dbm0)) == len(out)
    return out
