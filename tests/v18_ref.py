"""Live v18 objects of the real reference for the text bank tests: v18_init / v18_put / v18_tx / v18_rx / v18_rx_fillin through
the checker library oracle/ref.py opens, no glue.  The few fields the tests read out of a v18_state_t are found by their
offsets, which tests/golden/make_golden_v18.py measures with the reference's own headers and keeps in the fixture."""
import ctypes as C
import os

import numpy as np

import fsktx_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "v18_weitbrecht.npz")

MODES = (0x0002, 0x0200, 0x0004)                    # 45.45, 47.6, 50 baud
PRESET = {0x0002: 7, 0x0200: 9, 0x0004: 8}          # preset_fsk_specs[] entries
BAUD_X100 = {0x0002: 4545, 0x0200: 4760, 0x0004: 5000}
AUTOMODING_NONE = 1
FIELDS = ("tx_signal_on", "tx_draining", "baudot_tx_shift", "rx_suppression_timer", "baudot_rx_shift", "next_byte")
PUT_MSG = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_int)
PUT_BIT = C.CFUNCTYPE(None, C.c_void_p, C.c_int)

_declared = []
_golden = []


def available():
    from oracle import ref
    return ref.available()


def golden():
    if not _golden:
        _golden.append(np.load(GOLDEN))
    return _golden[0]


def lib():
    L = fsktx_ref.lib()
    if not _declared:
        vp, ci = C.c_void_p, C.c_int
        for name, res, args in [("v18_init", vp, [vp, C.c_bool, ci, ci, vp, vp, vp, vp]), ("v18_free", ci, [vp]),
                                ("v18_put", ci, [vp, C.c_char_p, ci]), ("v18_tx", ci, [vp, vp, ci]), ("v18_rx", ci, [vp, vp, ci]),
                                ("v18_rx_fillin", ci, [vp, ci]), ("fsk_rx_init", vp, [vp, vp, ci, vp, vp]),
                                ("fsk_rx_set_frame_parameters", None, [vp, ci, ci, ci]), ("fsk_rx", ci, [vp, vp, ci]),
                                ("fsk_rx_free", ci, [vp]), ("v18_get_current_mode", ci, [vp])]:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _declared.append(True)
    return L


class RefV18:
    """v18_init(NULL, calling_party, mode, V18_AUTOMODING_NONE, put_msg, ..).  rx() returns the characters put_msg delivered
    during the call, in order (each call delivers one)."""

    def __init__(self, mode, calling_party=False):
        self.got = []
        self.cb = PUT_MSG(lambda _, msg, n: self.got.append(bytes(msg[:n])))
        self.p = lib().v18_init(None, calling_party, mode, AUTOMODING_NONE, C.cast(self.cb, C.c_void_p), None, None, None)
        assert self.p

    def put(self, text):
        return lib().v18_put(self.p, bytes(text), len(text))

    def tx(self, n):
        row = np.zeros(max(n, 1), np.int16)
        got = lib().v18_tx(self.p, row.ctypes.data, n)
        return row[:n], got

    def rx(self, amp):
        amp = np.ascontiguousarray(amp, np.int16)
        self.got = []
        lib().v18_rx(self.p, amp.ctypes.data, len(amp))
        assert all(len(m) == 1 for m in self.got)
        return b"".join(self.got)

    def fillin(self, n):
        lib().v18_rx_fillin(self.p, n)

    def field(self, name):
        off, size = golden()["offsets"][FIELDS.index(name)]
        raw = C.string_at(self.p + int(off), int(size))
        return int.from_bytes(raw, "little", signed=True)

    def __del__(self):
        try:
            lib().v18_free(self.p)
        except Exception:
            pass


def line_codes(mode, samples):
    """The 5-bit codes a clean framed 5N2 reference fsk_rx makes of these samples."""
    codes = []
    cb = PUT_BIT(lambda _, v: codes.append(v) if v >= 0 else None)
    p = lib().fsk_rx_init(None, fsktx_ref.spec_ptr(PRESET[mode]), 2, C.cast(cb, C.c_void_p), None)
    lib().fsk_rx_set_frame_parameters(p, 5, 0, 2)
    amp = np.ascontiguousarray(samples, np.int16)
    lib().fsk_rx(p, amp.ctypes.data, len(amp))
    lib().fsk_rx_free(p)
    return np.array(codes, np.uint8)


def send_all(mode, text, tick=160, limit=4000):
    """A fresh reference sender given `text`, run to its end: (samples, lengths per call)."""
    s = RefV18(mode)
    assert s.put(text) == len(text)
    rows, lens = [], []
    for _ in range(limit):
        row, got = s.tx(tick)
        lens.append(got)
        rows.append(row[:got])
        if got < tick:
            break
    else:
        raise AssertionError("the sender did not end")
    return np.concatenate(rows), lens


def seeded_text(rng, n):
    """n bytes over all 128 codes"""
    return bytes(rng.integers(0, 128, n, dtype=np.uint8))


MIXED = b"Ab1?\x00 c\x7f2#\rD\n$e%~9\x01(f)G+h\x1b-8_Zz@[5]\t!q"
