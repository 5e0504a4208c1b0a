"""Writes tests/golden/hdlc.npz from the live reference.  hdlc.c and crc.c are not among the modules of
oracle/_ref/libspandsp_ref.so, so the two files are compiled here, in a temporary directory, with the flags of oracle/Makefile
(STRICT + DEFS), linked against that library, and nothing compiled is kept.  The fixture holds scripts, bit streams and
records only:

  offsets           [field][offset, size] of the hdlc_rx_state_t (RX_FIELDS) and hdlc_tx_state_t (TX_FIELDS) fields the banks'
                    state words map to, measured by a compiler on the reference's private header;
  schedule          the call lengths, in bits, cycled by every case;
  tx_<k>_cfg        crc32, inter_frame_flags, queue depth, calls;
  tx_<k>_ops        [op][call, command, argument, corrupt]: the commands offered to the queue ahead of that call (1 FRAME with
                    its length, 2 FLAGS with its count, 3 ABORT, 4 END), tx_<k>_opbytes the frames' octets back to back,
                    tx_<k>_results what each offer returned (-1: queue full, or a length the reference refuses);
  tx_<k>_bits       the bits produced, one per byte, all calls back to back; _lens per call, _under the underflow reports that
                    found the queue empty, _ended 1 where the call stopped on SIG_STATUS_END_OF_DATA, _words the state after
                    each call;
  rx_<k>_cfg        crc32, report_bad_frames, framing_ok_threshold, max_frame_len argument (-1: not set), report interval;
  rx_<k>_events     the stream: bits and SIG_STATUS_* codes (int16); cut into calls on the schedule; rx_<k>_midops
                    [call, len]: hdlc_rx_set_max_frame_len(len) ahead of that call;
  rx_<k>_recs       the handler calls, all calls back to back (>= 0: len | ok << 16, < 0: a status), _nrecs per call, _bytes
                    the frames' octets back to back, _words after each call, _buffer the 404 octets at the end;
  rxb_<k>_*         the same through hdlc_rx_put() for the streams that are whole octets of bits: _lens octets per call;
  loop_<m>_*        m = fsk: fsk_tx (V.21 channel 2) fed by hdlc_tx_get_bit -> fsk_rx, synchronous -> hdlc_rx_put_bit; m = v29:
                    v29_tx 9600 -> v29_rx -> hdlc_rx_put_bit, with the training reports passing through the framer; ticks of
                    160 samples.  _cfg: ticks, preamble flags, crc32, framing_ok_threshold; _frames / _framelens the frames
                    queued behind the preamble; _recs / _nrecs / _bytes the receiver's handler calls per tick.

The sender cases run the reference under the driver the bank's queue stands for: an underflow handler that pops one command
off a FIFO, and an owner who, between calls, offers the FIFO to a sender with no frame in progress until a frame is in.

Run from the repository root:  python tests/golden/make_golden_hdlc.py [reference source dir]"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(HERE, "hdlc.npz")
STRICT = ["-std=gnu99", "-O2", "-ffp-contract=off", "-fPIC", "-fwrapv"]
DEFS = ["-DHAVE_MATH_H", "-DHAVE_STDBOOL_H", "-DHAVE_SINF", "-DHAVE_COSF", "-DHAVE_TANF", "-DHAVE_ASINF", "-DHAVE_ACOSF", "-DHAVE_ATANF",
        "-DHAVE_ATAN2F", "-DHAVE_CEILF", "-DHAVE_FLOORF", "-DHAVE_POWF", "-DHAVE_EXPF", "-DHAVE_LOGF", "-DHAVE_LOG10F", "-DHAVE_LRINT",
        "-DHAVE_LRINTF", "-DHAVE_LONG_DOUBLE", "-DHAVE_MALLOC_H", "-DHAVE_ALIGNED_ALLOC", "-DHAVE_UNISTD_H", "-DHAVE_STDLIB_H",
        "-DHAVE_STRING_H", "-DHAVE_INTTYPES_H", "-DHAVE_STDINT_H", "-DHAVE_TGMATH_H"]
# the order of the banks' state words (hdlc_dev.hpp: HR_*, HT_*)
RX_FIELDS = ("crc_bytes", "max_frame_len", "report_bad_frames", "framing_ok_threshold", "framing_ok_announced", "flags_seen",
             "raw_bit_stream", "byte_in_progress", "num_bits", "octet_counting_mode", "octet_count", "octet_count_report_interval", "len",
             "rx_bytes", "rx_frames", "rx_crc_errors", "rx_length_errors", "rx_aborts", "buffer")
TX_FIELDS = ("crc_bytes", "inter_frame_flags", "progressive", "max_frame_len", "octets_in_progress", "num_bits", "idle_octet", "flag_octets",
             "abort_octets", "report_flag_underflow", "len", "pos", "crc", "byte", "bits", "tx_end", "buffer")
HEADERS = ("telephony", "alloc", "async", "crc", "hdlc", "private/hdlc")
SCHEDULE = (1, 7, 8, 9, 24, 192, 331)
BYTE_SCHEDULE = (1, 2, 3, 5, 24, 41)
FRAME, FLAGS, ABORT, END = 1, 2, 3, 4
FRAME_CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_int, C.c_int)
STATUS_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int)
UNDERFLOW_CB = C.CFUNCTYPE(None, C.c_void_p)


def build_reference(ref_src, d):
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    so = os.path.join(d, "libhdlc_ref.so")
    subprocess.run(["gcc"] + STRICT + DEFS + ["-I" + os.path.join(ref_dir, "gen"), "-I" + ref_src, "-shared", "-o", so,
                    os.path.join(ref_src, "hdlc.c"), os.path.join(ref_src, "crc.c"), "-L" + ref_dir, "-lspandsp_ref",
                    "-Wl,-rpath," + ref_dir, "-lm"], check=True)
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>",
             "#include <stdbool.h>"] + ['#include "spandsp/%s.h"' % h for h in HEADERS] + ["int main(void) {"]
    for typ, fields in (("hdlc_rx_state_t", RX_FIELDS), ("hdlc_tx_state_t", TX_FIELDS)):
        for f in fields:
            lines.append('printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *) 0)->%s));' % (typ, f, typ, f))
    lines.append("return 0; }")
    src = os.path.join(d, "off.c")
    open(src, "w").write("\n".join(lines) + "\n")
    exe = os.path.join(d, "off")
    subprocess.run(["gcc", "-std=gnu99"] + DEFS + ["-I" + ref_src, src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    offsets = np.array([[int(x) for x in ln.split()] for ln in out.strip().splitlines()], np.int32)
    C.CDLL(os.path.join(ref_dir, "libspandsp_ref.so"), mode=C.RTLD_GLOBAL)
    L = C.CDLL(so)
    vp, ci, cb = C.c_void_p, C.c_int, C.c_bool
    for name, res, args in [("hdlc_rx_init", vp, [vp, cb, cb, ci, vp, vp]), ("hdlc_rx_free", ci, [vp]), ("hdlc_rx_put_bit", None, [vp, ci]),
                            ("hdlc_rx_put", None, [vp, C.c_char_p, ci]), ("hdlc_rx_set_status_handler", None, [vp, vp, vp]),
                            ("hdlc_rx_set_max_frame_len", None, [vp, C.c_size_t]),
                            ("hdlc_rx_set_octet_counting_report_interval", None, [vp, ci]),
                            ("hdlc_tx_init", vp, [vp, cb, ci, cb, vp, vp]), ("hdlc_tx_free", ci, [vp]), ("hdlc_tx_get_bit", ci, [vp]),
                            ("hdlc_tx_frame", ci, [vp, C.c_char_p, C.c_size_t]), ("hdlc_tx_flags", ci, [vp, ci]), ("hdlc_tx_abort", ci, [vp]),
                            ("hdlc_tx_corrupt_frame", ci, [vp])]:
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    return L, offsets


def words_of(p, offs):
    out = [int.from_bytes(C.string_at(p + int(off), int(size)), "little") & 0xFFFFFFFF for off, size in offs]
    return np.array(out, np.uint32).view(np.int32)


# ---- senders ----------------------------------------------------------------------------------------------------------

def pattern(n, seed):
    """n octets that exercise the stuffing: runs of 0xFF, flags, 0x1F / 0xF8 at every alignment, and noise"""
    rng = np.random.RandomState(seed)
    special = [0xFF, 0x7E, 0x1F, 0xF8, 0xFF, 0xFF, 0x7E, 0x7E, 0x1F, 0x1F, 0xF8, 0xF8, 0x3E, 0x7C, 0xFB, 0xDF]
    out = []
    while len(out) < n:
        if rng.randint(3) == 0:
            out.extend(rng.randint(0, 256, rng.randint(1, 6)).tolist())
        else:
            k = rng.randint(len(special))
            out.extend(special[k:k + rng.randint(1, 5)])
    return bytes(out[:n])


def tx_cases():
    """(crc32, inter_frame_flags, depth, calls, [(call, command, argument: bytes or count, corrupt)])"""
    a = [(0, FLAGS, 32, 0), (0, FRAME, b"\xff\x13\x7e", 0), (9, FRAME, b"\x7e", 0), (9, FRAME, b"\xff\xff", 0),
         (9, FRAME, pattern(3, 1), 0), (12, FRAME, pattern(17, 2), 1), (13, FRAME, pattern(9, 3), 0), (13, FRAME, pattern(5, 4), 0),
         (13, FRAME, pattern(6, 5), 0), (27, ABORT, 0, 0), (28, FRAME, b"\x1f\xf8", 0), (30, END, 0, 0), (34, FRAME, b"\xf8", 0)]
    b = [(0, FLAGS, 2, 0), (0, FRAME, pattern(255, 6), 0), (2, FRAME, pattern(400, 7), 0), (2, FRAME, pattern(401, 8), 0),
         (3, FRAME, pattern(2, 9), 1), (5, FLAGS, -3, 0), (6, FRAME, pattern(3, 10), 0), (6, FRAME, pattern(1, 11), 0), (20, FLAGS, -3, 0),
         (40, FRAME, pattern(40, 12), 0), (72, ABORT, 0, 0), (73, END, 0, 0), (75, FRAME, pattern(41, 29), 0), (75, FLAGS, 3, 0),
         (75, FLAGS, -3, 0), (75, FRAME, pattern(255, 13), 1), (82, END, 0, 0), (82, FRAME, b"\xff", 0)]
    c = [(0, END, 0, 0), (1, FRAME, b"\xff", 0), (4, FRAME, b"\x7e\x7e", 0), (5, FRAME, b"\xff\xff\xff", 1), (5, ABORT, 0, 0),
         (5, FRAME, pattern(30, 14), 0), (5, FRAME, pattern(30, 15), 0), (12, FLAGS, 2, 0), (12, ABORT, 0, 0), (12, FLAGS, 0, 0),
         (13, FRAME, pattern(64, 16), 0), (19, FRAME, pattern(400, 17), 1), (20, FRAME, pattern(1, 18), 0), (33, END, 0, 0)]
    d = [(0, ABORT, 0, 0), (0, FRAME, pattern(3, 19), 0), (0, FRAME, pattern(3, 20), 0), (0, FRAME, pattern(3, 21), 0),
         (0, FRAME, pattern(3, 22), 0), (0, FRAME, pattern(3, 23), 0), (6, FRAME, pattern(255, 24), 0), (6, FRAME, pattern(2, 25), 0),
         (6, FLAGS, 32, 0), (6, FRAME, pattern(1, 26), 0), (7, FRAME, pattern(2, 27), 0), (20, END, 0, 0), (21, END, 0, 0),
         (22, FLAGS, 1, 0), (23, FRAME, pattern(7, 28), 0)]
    return [(0, 1, 3, 42, a), (1, 2, 4, 91, b), (0, 5, 3, 42, c), (1, 1, 4, 35, d)]


class TxDriver:
    """The reference sender with a FIFO behind its underflow handler."""

    def __init__(self, L, offs, crc32, iff, depth):
        self.L, self.offs, self.depth = L, offs, depth
        self.fifo = []
        self.under = 0
        self.cb = UNDERFLOW_CB(lambda _: self.handler())
        self.s = L.hdlc_tx_init(None, bool(crc32), iff, False, C.cast(self.cb, C.c_void_p), None)

    def words(self):
        return words_of(self.s, self.offs[:-1])

    def take(self):
        kind, arg, corrupt = self.fifo.pop(0)
        if kind == FRAME:
            if self.L.hdlc_tx_frame(self.s, arg, len(arg)) == 0 and corrupt:
                self.L.hdlc_tx_corrupt_frame(self.s)
        elif kind == FLAGS:
            self.L.hdlc_tx_flags(self.s, arg)
        elif kind == ABORT:
            self.L.hdlc_tx_abort(self.s)
        else:
            self.L.hdlc_tx_frame(self.s, None, 0)

    def handler(self):
        if self.fifo:
            self.take()
        else:
            self.under += 1

    def offer(self, kind, arg, corrupt):
        if len(self.fifo) >= self.depth or (kind == FRAME and len(arg) > int(self.words()[3])):
            return -1
        self.fifo.append((kind, arg, corrupt))
        return 0

    def offer_idle(self):
        while int(self.words()[10]) == 0 and self.fifo:
            self.take()

    def call(self, want):
        self.offer_idle()
        self.under = 0
        bits, ended = [], 0
        for _ in range(want):
            b = self.L.hdlc_tx_get_bit(self.s)
            if b < 0:
                assert b == -7
                ended = 1
                break
            bits.append(b)
        return bits, ended, self.under


def run_tx_case(L, offs, case):
    crc32, iff, depth, calls, ops = case
    D = TxDriver(L, offs, crc32, iff, depth)
    out = {"bits": [], "lens": [], "under": [], "ended": [], "words": [], "results": []}
    for k in range(calls):
        for call, kind, arg, corrupt in ops:
            if call == k:
                out["results"].append(D.offer(kind, arg, corrupt))
        bits, ended, under = D.call(SCHEDULE[k % len(SCHEDULE)])
        out["bits"].extend(bits)
        out["lens"].append(len(bits))
        out["under"].append(under)
        out["ended"].append(ended)
        out["words"].append(D.words())
    L.hdlc_tx_free(D.s)
    return out


# ---- receivers --------------------------------------------------------------------------------------------------------

def crc_of(data, crc32):
    crc = 0xFFFFFFFF if crc32 else 0xFFFF
    poly = 0xEDB88320 if crc32 else 0x8408
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ (poly if crc & 1 else 0)
    crc ^= 0xFFFFFFFF if crc32 else 0xFFFF
    return bytes((crc >> (8*i)) & 0xFF for i in range(4 if crc32 else 2))


FLAG_BITS = [0, 1, 1, 1, 1, 1, 1, 0]


def stuffed(octets):
    out, ones = [], 0
    for b in octets:
        for i in range(8):
            bit = (b >> i) & 1
            out.append(bit)
            ones = ones + 1 if bit else 0
            if ones == 5:
                out.append(0)
                ones = 0
    return out


def wire(frames, crc32, flags_before=2, flags_between=1, good_crc=True):
    """flags, then each frame with its CRC behind it and flags after it"""
    bits = FLAG_BITS*flags_before
    for f in frames:
        crc = crc_of(f, crc32)
        if not good_crc:
            crc = bytes(b ^ 0x55 for b in crc)
        bits = bits + stuffed(f + crc) + FLAG_BITS*flags_between
    return bits


def rx_cases(L, offs, rx_offs):
    """(name, crc32, report_bad_frames, threshold, max_frame_len or -1, interval, events, frames that must arrive or None)"""
    frames = [pattern(3, 31), pattern(1, 32), pattern(2, 33), pattern(255, 34), pattern(400, 35)]
    cases = []
    # the senders' own streams: what the reference sends, the reference must deliver
    for k, case in enumerate(tx_cases()):
        crc32, _, _, _, ops = case
        bits = run_tx_case(L, offs, case)["bits"]
        cases.append(("tx%d" % k, crc32, 1, 1 + k, -1, 0, bits, None))
    for crc32, bad, thr in ((0, 0, 1), (1, 0, 2), (0, 1, 5)):
        cases.append(("clean_%d_%d" % (crc32, thr), crc32, bad, thr, -1, 0, wire(frames, crc32, flags_before=thr + 1), frames))
    clean = wire(frames[:4], 0, flags_before=3, flags_between=2)
    for bad in (0, 1):
        hit = list(clean)
        for at in (5, 30, 61, 100, 333, 900, 901, 1500, len(hit) - 20, len(hit) - 3):
            hit[at] ^= 1
        cases.append(("biterr_%d" % bad, 0, bad, 2, -1, 0, hit, None))
    # a flag one bit out of step: in the preamble (before framing is OK) and between frames (after)
    for thr in (1, 2, 5):
        bits = FLAG_BITS*2 + [0] + FLAG_BITS*thr + [1, 0] + FLAG_BITS*(thr + 1) + stuffed(frames[0] + crc_of(frames[0], 0)) + FLAG_BITS + [0] \
            + FLAG_BITS + stuffed(frames[2] + crc_of(frames[2], 0)) + FLAG_BITS + [1] + FLAG_BITS + stuffed(frames[1] + crc_of(frames[1], 0)) \
            + FLAG_BITS*2
        cases.append(("slip_%d" % thr, 0, 1, thr, -1, 0, bits, None))
    # seven to fifteen ones between frames, and inside one
    bits = FLAG_BITS*3
    for ones in range(7, 16):
        bits = bits + stuffed(frames[0] + crc_of(frames[0], 0)) + FLAG_BITS + [0] + [1]*ones + [0] + FLAG_BITS
        bits = bits + stuffed(frames[2])[:11] + [1]*ones + [0] + FLAG_BITS*2
    cases.append(("ones", 0, 1, 2, -1, 7, bits, None))
    # the run of 0x7F: an abort every eight bits, with the octet count running
    run = [0, 1, 1, 1, 1, 1, 1, 1]*45
    for interval in (1, 20):
        bits = FLAG_BITS*2 + stuffed(frames[0] + crc_of(frames[0], 0)) + run + [0, 1, 0, 1, 1, 0, 0, 1]*50 + FLAG_BITS*2 \
            + stuffed(frames[1] + crc_of(frames[1], 0)) + FLAG_BITS
        cases.append(("aborts_%d" % interval, 0, 0, 1, -1, interval, bits, None))
    # frames shorter than the CRC, a bad one-octet frame every 16 bits
    for crc32, bad in ((0, 1), (1, 1), (0, 0)):
        bits = FLAG_BITS*2
        for n in (1, 1, 1, 1, 2, 3, 1, 4, 5, 1):
            bits = bits + stuffed(pattern(n, 40 + n)[:n]) + FLAG_BITS
        cases.append(("short_%d_%d" % (crc32, bad), crc32, bad, 1, -1, 1, bits, None))
    # frames around the buffer's end: 401 .. 410 octets on the wire, good CRCs, then a frame that fits
    for crc32, bad in ((0, 1), (0, 0), (1, 1)):
        crc_bytes = 4 if crc32 else 2
        long_frames = [pattern(n - crc_bytes, 50 + n) for n in (401, 404, 405, 410)]
        bits = FLAG_BITS*2
        for f in long_frames:
            bits = bits + stuffed(f + crc_of(f, crc32)) + FLAG_BITS + stuffed(frames[0] + crc_of(frames[0], crc32)) + FLAG_BITS
        cases.append(("long_%d_%d" % (crc32, bad), crc32, bad, 1, -1, 0, bits, None))
    # max_frame_len 10: short frames, then long ones over what they left in the buffer
    shorts = [pattern(n, 60 + n) for n in (10, 9, 3, 10)]
    bits = wire(shorts, 0) + stuffed(pattern(11, 70) + crc_of(pattern(11, 70), 0)) + FLAG_BITS + stuffed(pattern(40, 71)) + FLAG_BITS*2 \
        + stuffed(shorts[2] + crc_of(shorts[2], 0)) + FLAG_BITS
    for bad in (1, 0):
        cases.append(("stale_%d" % bad, 0, bad, 1, 10, 0, bits, None))
    cases.append(("stale_oct", 0, 1, 3, 10, 1, FLAG_BITS*2 + bits, None))
    # every SIG_STATUS_* code dropped between bits: -9, -10, -12 .. -17 and -40 are ignored, the others pass or reset
    base = wire(frames[:3] + [pattern(20, 72)], 0, flags_before=3)
    ev = list(base)
    for i, code in enumerate([-2, -3, -4, -9, -1, -5, -6, -7, -8, -10, -11, -12, -13, -14, -15, -16, -17, -40, -2, -4, -1]):
        ev.insert(7 + i*11 + (i % 3), code)
    cases.append(("status", 0, 1, 2, -1, 0, ev + base, None))
    # max_frame_len taken down ahead of call 12 (621 bits in), between the last octet of a frame and its flag: the flag finds
    # len above it.  The frame's length that puts the call boundary there is searched for.
    for n in range(30, 70):
        bits = wire([pattern(10, 80), pattern(n, 81), pattern(5, 82), pattern(11, 83), pattern(10, 84)], 0)
        trial = ("shrink_1", 0, 1, 1, -1, 0, bits, None, [(12, 10)])
        if run_rx_case(L, rx_offs, trial)[0]["words"][-1][16] > 0:
            break
    else:
        raise AssertionError("no frame length ends on the call boundary")
    for bad in (1, 0):
        cases.append(("shrink_%d" % bad, 0, bad, 1, -1, 0, bits, None, [(12, 10)]))
    return cases


class RxDriver:
    def __init__(self, L, offs, crc32, bad, thr, max_len, interval):
        self.L, self.offs = L, offs
        self.recs, self.bytes = [], []
        self.fcb = FRAME_CB(self.frame)
        self.scb = STATUS_CB(lambda _, code: self.recs.append(code))
        self.s = L.hdlc_rx_init(None, bool(crc32), bool(bad), thr, C.cast(self.fcb, C.c_void_p), None)
        L.hdlc_rx_set_status_handler(self.s, C.cast(self.scb, C.c_void_p), None)
        if max_len >= 0:
            L.hdlc_rx_set_max_frame_len(self.s, max_len)
        L.hdlc_rx_set_octet_counting_report_interval(self.s, interval)
        self.frames = []

    def frame(self, _, pkt, n, ok):
        assert 0 <= n <= 403
        self.recs.append(n | (0x10000 if ok else 0))
        data = bytes(pkt[:n])
        self.bytes.append(data)
        self.frames.append((data, bool(ok)))

    def words(self):
        return words_of(self.s, self.offs[:-1])

    def buffer(self):
        return np.frombuffer(C.string_at(self.s + int(self.offs[-1][0]), 404), np.uint8).copy()


def run_rx_case(L, offs, case, by_octets=False):
    name, crc32, bad, thr, max_len, interval, events, must = case[:8]
    midops = case[8] if len(case) > 8 else []
    D = RxDriver(L, offs, crc32, bad, thr, max_len, interval)
    nrecs, words, lens = [], [], []
    at, k = 0, 0
    if by_octets:
        octets = np.packbits(np.array(events, np.uint8)).tobytes()
        while at < len(octets):
            n = min(BYTE_SCHEDULE[k % len(BYTE_SCHEDULE)], len(octets) - at)
            before = len(D.recs)
            L.hdlc_rx_put(D.s, octets[at:at + n], n)
            nrecs.append(len(D.recs) - before)
            words.append(D.words())
            lens.append(n)
            at += n
            k += 1
    else:
        while at < len(events):
            n = min(SCHEDULE[k % len(SCHEDULE)], len(events) - at)
            for call, value in midops:
                if call == k:
                    L.hdlc_rx_set_max_frame_len(D.s, value)
            before = len(D.recs)
            for e in events[at:at + n]:
                L.hdlc_rx_put_bit(D.s, int(e))
            nrecs.append(len(D.recs) - before)
            words.append(D.words())
            lens.append(n)
            at += n
            k += 1
    if must is not None:
        assert [f for f, ok in D.frames if ok] == must, name
    out = {"cfg": np.array([crc32, bad, thr, max_len, interval], np.int32), "recs": np.array(D.recs, np.int32),
           "nrecs": np.array(nrecs, np.int32), "bytes": np.frombuffer(b"".join(D.bytes), np.uint8).copy(),
           "words": np.array(words, np.int32), "buffer": D.buffer(), "lens": np.array(lens, np.int32),
           "midops": np.array(midops, np.int32).reshape(-1, 2)}
    L.hdlc_rx_free(D.s)
    return out, D.frames


PUT_BIT = C.CFUNCTYPE(None, C.c_void_p, C.c_int)
LOOPS = {"fsk": (130, 32, 0, 2, [pattern(3, 90), pattern(23, 91), pattern(12, 92)]),
         "v29": (56, 10, 0, 1, [pattern(255, 93), pattern(255, 94), pattern(100, 95)])}


def run_loop(L, rx_off, tx_off, which):
    """sender -> modulator -> demodulator -> receiver in the reference, a tick at a time; the receiver's records per tick"""
    import fsktx_ref
    import modemtx_ref
    ticks, preamble, crc32, thr, frames = LOOPS[which]
    D = TxDriver(L, tx_off, crc32, 1, 8)
    assert D.offer(FLAGS, preamble, 0) == 0
    for f in frames:
        assert D.offer(FRAME, f, 0) == 0
    R = RxDriver(L, rx_off, crc32, 0, thr, -1, 0)
    put = PUT_BIT(lambda _, bit: L.hdlc_rx_put_bit(R.s, bit))
    get_bit = lambda: L.hdlc_tx_get_bit(D.s)
    ref = fsktx_ref.lib()
    if which == "fsk":
        tx = fsktx_ref.RefFskTx(1, get_bit=get_bit)             # preset_fsk_specs[1]: V.21 channel 2
        rx = ref.glue_fsk_rx_new(1, 1, C.cast(put, C.c_void_p), None)       # FSK_FRAME_MODE_SYNC
        rx_fn, free = ref.fsk_rx, ref.fsk_rx_free
    else:
        modemtx_ref.lib()
        tx = modemtx_ref.RefModemTx("v29", 9600, False, get_bit)
        ref.v29_rx_init.restype = C.c_void_p
        ref.v29_rx_init.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        rx = ref.v29_rx_init(None, 9600, C.cast(put, C.c_void_p), None)
        rx_fn, free = ref.v29_rx, ref.v29_rx_free
    nrecs = []
    for _ in range(ticks):
        D.offer_idle()
        row, got = tx.tx(160)
        assert got == 160
        before = len(R.recs)
        rx_fn(rx, row.ctypes.data, 160)
        nrecs.append(len(R.recs) - before)
    free(rx)
    # what was sent clean arrives
    assert [f for f, ok in R.frames if ok] == frames and all(ok for _, ok in R.frames), which
    print("loop", which, ticks, "ticks", len(R.recs), "records", R.recs[:8], "stats", R.words()[13:18])
    out = {"cfg": np.array([ticks, preamble, crc32, thr], np.int32), "frames": np.frombuffer(b"".join(frames), np.uint8).copy(),
           "framelens": np.array([len(f) for f in frames], np.int32), "recs": np.array(R.recs, np.int32), "nrecs": np.array(nrecs, np.int32),
           "bytes": np.frombuffer(b"".join(R.bytes), np.uint8).copy()}
    L.hdlc_tx_free(D.s)
    L.hdlc_rx_free(R.s)
    return out


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    with tempfile.TemporaryDirectory() as d:
        L, offsets = build_reference(ref_src, d)
        rx_off, tx_off = offsets[:len(RX_FIELDS)], offsets[len(RX_FIELDS):]
        out = {"offsets": offsets, "schedule": np.array(SCHEDULE, np.int32)}
        cases = tx_cases()
        out["tx_cases"] = np.array(len(cases), np.int32)
        for k, case in enumerate(cases):
            crc32, iff, depth, calls, ops = case
            r = run_tx_case(L, tx_off, case)
            key = "tx_%d_" % k
            out[key + "cfg"] = np.array([crc32, iff, depth, calls], np.int32)
            out[key + "ops"] = np.array([[call, kind, len(arg) if kind == FRAME else arg, corrupt] for call, kind, arg, corrupt in ops], np.int32)
            out[key + "opbytes"] = np.frombuffer(b"".join(arg for _, kind, arg, _ in ops if kind == FRAME), np.uint8).copy()
            out[key + "bits"] = np.array(r["bits"], np.uint8)
            for f in ("lens", "under", "ended", "words", "results"):
                out[key + f] = np.array(r[f], np.int32)
            print(key, calls, "calls", len(r["bits"]), "bits", "underflows", int(np.sum(r["under"])), "ends", int(np.sum(r["ended"])),
                  "refused", int(np.sum(np.array(r["results"]) < 0)))
            # the python framer the receiver streams are built with, against the reference's sender
            if k == 0:
                f0 = b"\xff\x13\x7e"
                mine = stuffed(f0 + crc_of(f0, 0))
                got = r["bits"][32*8:32*8 + len(mine)]
                assert got == mine, "the stuffing of this file is not the reference's"
        rcases = rx_cases(L, tx_off, rx_off)
        out["rx_names"] = np.array([c[0] for c in rcases])
        for k, case in enumerate(rcases):
            r, frames = run_rx_case(L, rx_off, case)
            if case[0].startswith("tx"):
                # every clean frame the reference sent, the reference delivers
                sent = [arg for _, kind, arg, corrupt in tx_cases()[int(case[0][2:])][4] if kind == FRAME and not corrupt and len(arg) <= 400]
                good = [f for f, ok in frames if ok]
                results = out["tx_%s_results" % case[0][2:]]
                ops = tx_cases()[int(case[0][2:])][4]
                queued = [arg for (_, kind, arg, corrupt), res in zip(ops, results) if kind == FRAME and not corrupt and res == 0]
                assert all(f in sent for f in good), case[0]
                # (a stream that opens without a preamble, or with fewer flags than the threshold, loses its first frames)
                assert len(good) > 0 and len(good) <= len(queued), (case[0], len(good), len(queued))
            key = "rx_%d_" % k
            out[key + "events"] = np.array(case[6], np.int16)
            for f in ("cfg", "recs", "nrecs", "bytes", "words", "buffer", "midops"):
                out[key + f] = r[f]
            print(key, case[0], len(case[6]), "events", len(r["recs"]), "records", len(r["bytes"]), "octets", "stats", r["words"][-1][13:18])
            if len(case[6]) % 8 == 0 and min(case[6]) >= 0 and len(case) == 8:
                rb, _ = run_rx_case(L, rx_off, case, by_octets=True)
                assert np.array_equal(rb["recs"], r["recs"]) and np.array_equal(rb["bytes"], r["bytes"]), case[0]
                for f in ("nrecs", "words", "lens", "buffer"):
                    out["rxb_%d_%s" % (k, f)] = rb[f]
        for which in ("fsk", "v29"):
            for f, v in run_loop(L, rx_off, tx_off, which).items():
                out["loop_%s_%s" % (which, f)] = v
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
