"""ctypes binding of oracle/_ref/libspandsp_hdlc_ref.so -- the reference's HDLC framer (hdlc.c, crc.c), compiled where it
lies by oracle/Makefile, behind the batch drivers of oracle/ref_glue/ref_glue_hdlc.c.

TEST INFRASTRUCTURE ONLY -- see oracle/__init__.py.  The .so is built where the reference's sources are and travels with the
tree; the sources are never read at run time.

run_rx() and run_tx() take ONE line through a schedule of calls inside C.  want: None -- words is [W], the state words after
the last call; True -- [calls][W], after every call; a mask [calls] -- [the calls asked for][W], in their order.
"""
import ctypes as C
import os

import numpy as np

from . import HERE

HDLC_SO = os.path.join(HERE, "_ref", "libspandsp_hdlc_ref.so")
RX_WORDS, TX_WORDS, BUFFER = 18, 16, 404
OP_MAX_FRAME_LEN, OP_REPORT_INTERVAL, OP_RESTART = 1, 2, 3          # a receiver's control operations
FRAME, FLAGS, ABORT, END = 1, 2, 3, 4                               # a sender's commands
FRAME_OK = 0x10000

_lib = []


def available():
    return os.path.exists(HDLC_SO)


def lib():
    if not _lib:
        L = C.CDLL(HDLC_SO)
        vp, ci = C.c_void_p, C.c_int
        sigs = {"glue_hdlc_rx_run": (ci, [ci, ci, ci, vp, ci, vp, ci, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp]),
                "glue_hdlc_tx_run": (ci, [ci, ci, ci, ci, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
                "glue_hdlc_state_words": (ci, [ci])}
        for name, (res, args) in sigs.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        assert [L.glue_hdlc_state_words(k) for k in range(2)] == [RX_WORDS, TX_WORDS]
        _lib.append(L)
    return _lib[0]


def _p(a):
    return a.ctypes.data


def _words(n_calls, w, want):
    """(the array the words go to, the mask's address)"""
    if want is None or want is False:
        return np.zeros(w, np.int32), None
    mask = np.ones(n_calls, np.int32) if want is True else np.ascontiguousarray(np.asarray(want) != 0, np.int32)
    assert len(mask) == n_calls
    return np.zeros((int(mask.sum()), w), np.int32), mask


def rx_capacity(events):
    """(records, octets) no call of `events` bits can exceed: the figures of hdlc_rx_capacity() (csrc/hdlc_dev.hpp), restated"""
    events = np.asarray(events, np.int64)
    return events + events//8 + 1, (403 + events//8 + 3) & ~3


def run_rx(crc32, report_bad_frames, threshold, events, lens, ops=(), octets=False, want=None):
    """events: int16 entries, or with octets uint8; lens [calls]; ops: [(call, operation, value)], call -1: behind the init.
    Returns (recs, bytes, n_recs [calls], n_bytes [calls], words, buffer [404])."""
    lens = np.ascontiguousarray(lens, np.int32)
    events = np.ascontiguousarray(events, np.uint8 if octets else np.int16)
    total = int(lens.sum())
    assert total <= len(events) and (lens >= 0).all()
    ops = np.ascontiguousarray(np.array(ops, np.int32).reshape(-1, 3))
    bits = total*(8 if octets else 1)
    # room: a record or two a bit at the most, and the carried-in frame of every call
    rec_room = 2*bits + 2*len(lens) + 8
    byte_room = bits//8 + 404*len(lens) + 8
    recs, by = np.zeros(rec_room, np.int32), np.zeros(byte_room, np.uint8)
    n_recs, n_bytes = np.zeros(len(lens), np.int32), np.zeros(len(lens), np.int32)
    words, mask = _words(len(lens), RX_WORDS, want)
    buffer = np.zeros(BUFFER, np.uint8)
    n = lib().glue_hdlc_rx_run(int(crc32), int(report_bad_frames), int(threshold), _p(events), int(octets), _p(lens), len(lens), _p(ops), len(ops),
                               _p(recs), rec_room, _p(by), byte_room, _p(n_recs), _p(n_bytes), _p(words), None if mask is None else _p(mask),
                               _p(buffer))
    assert n >= 0 and n == int(n_recs.sum()), n
    return recs[:n].copy(), by[:int(n_bytes.sum())].copy(), n_recs, n_bytes, words, buffer


def run_tx(crc32, inter_frame_flags, depth, max_frame_len, ops, opbytes, wants, want=None):
    """ops: [(call, command, argument, corrupt)] sorted by call; opbytes: the FRAME commands' octets back to back; wants
    [calls] bits; max_frame_len -1: not set.  Returns (bits one a byte, lens [calls], under [calls], ended [calls], taken
    [calls]: the kinds of command the call took, 1 << kind by the underflow handler and 0x100 << kind between calls, results
    [ops], words)."""
    wants = np.ascontiguousarray(wants, np.int32)
    ops = np.ascontiguousarray(np.array(ops, np.int32).reshape(-1, 4))
    opbytes = np.ascontiguousarray(opbytes, np.uint8)
    assert (np.diff(ops[:, 0]) >= 0).all() and int(ops[ops[:, 1] == FRAME, 2].sum()) == len(opbytes)
    bits = np.zeros(int(wants.sum()) + 8, np.uint8)
    lens, under, ended, taken = (np.zeros(len(wants), np.int32) for _ in range(4))
    results = np.zeros(len(ops), np.int32)
    words, mask = _words(len(wants), TX_WORDS, want)
    n = lib().glue_hdlc_tx_run(int(crc32), int(inter_frame_flags), int(depth), int(max_frame_len), _p(ops), _p(opbytes), len(ops), _p(wants),
                               len(wants), _p(bits), _p(lens), _p(under), _p(ended), _p(taken), _p(results), _p(words), None if mask is None else _p(mask),
                               None)
    assert 0 <= n == int(lens.sum()), n
    return bits[:n].copy(), lens, under, ended, taken, results, words
