"""Live objects of the real reference for the modem sender tests: v29_tx, v27ter_tx and v17_tx through the checker library
oracle/ref.py opens, with Python get_bit and status callbacks, and the few prototypes ref.py does not declare."""
import ctypes as C

import numpy as np

END_OF_DATA = -7            # SIG_STATUS_END_OF_DATA, async.h
SHUTDOWN_COMPLETE = -10
GET = C.CFUNCTYPE(C.c_int, C.c_void_p)
STATUS = C.CFUNCTYPE(None, C.c_void_p, C.c_int)

SCHEDULE = [160, 160, 77, 1, 8, 333, 160, 1024, 5, 160]
# (modem, bit rate, tep, short train): every rate family of the three senders, tep on and off, V.17's short training
CASES = [("v29", 9600, False, False), ("v29", 7200, True, False), ("v29", 4800, False, False),
         ("v27ter", 4800, False, False), ("v27ter", 2400, True, False),
         ("v17", 14400, False, False), ("v17", 7200, True, False), ("v17", 14400, False, True)]
BITS_PER_SYMBOL = {("v29", 9600): 4, ("v29", 7200): 3, ("v29", 4800): 2, ("v27ter", 4800): 3, ("v27ter", 2400): 2,
                   ("v17", 14400): 6, ("v17", 12000): 5, ("v17", 9600): 4, ("v17", 7200): 3, ("v17", 4800): 2}

_declared = []


def lib():
    from oracle import ref
    L = ref.lib()
    if not _declared:
        vp, ci, cb = C.c_void_p, C.c_int, C.c_bool
        for m in ("v29_tx", "v27ter_tx", "v17_tx"):
            for name, res, args in [("_init", vp, [vp, ci, cb, vp, vp]), ("_set_get_bit", None, [vp, vp, vp]),
                                    ("_set_modem_status_handler", None, [vp, vp, vp]), ("_power", None, [vp, C.c_float]),
                                    ("_free", ci, [vp]), ("", ci, [vp, vp, ci]),
                                    ("_restart", ci, [vp, ci, cb] + ([cb] if m == "v17_tx" else []))]:
                f = getattr(L, m + name)
                f.restype = res
                f.argtypes = args
        _declared.append(True)
    return L


class RefModemTx:
    """xxx_tx_init(NULL, bit_rate, tep, get_bit, NULL) of the real reference; get_bit() and status(code) are Python callables.
    V.17's short training is reached as a caller reaches it: v17_tx_restart(s, bit_rate, tep, true) after the init."""

    def __init__(self, modem, bit_rate, tep, get_bit, status=None, short_train=False):
        self.name = modem + "_tx"
        self.cb = GET(lambda _: get_bit())
        self.p = self._f("_init")(None, bit_rate, tep, C.cast(self.cb, C.c_void_p), None)
        assert self.p
        self.scb = None
        if status is not None:
            self.set_status(status)
        if short_train:
            self.restart(bit_rate, tep, True)

    def _f(self, fn):
        return getattr(lib(), self.name + fn)

    def set_get_bit(self, get_bit):
        keep = self.cb
        self.cb = GET(lambda _: get_bit())
        self._f("_set_get_bit")(self.p, C.cast(self.cb, C.c_void_p), None)
        del keep

    def set_status(self, status):
        self.scb = STATUS(lambda _, code: status(code))
        self._f("_set_modem_status_handler")(self.p, C.cast(self.scb, C.c_void_p), None)

    def power(self, dbm0):
        self._f("_power")(self.p, dbm0)

    def restart(self, bit_rate, tep, short_train=False):
        if self.name == "v17_tx":
            return self._f("_restart")(self.p, bit_rate, tep, short_train)
        return self._f("_restart")(self.p, bit_rate, tep)

    def tx(self, n):
        """(row of n samples, zero where none was written; returned length)"""
        row = np.zeros(max(1, n), np.int16)
        got = self._f("")(self.p, row.ctypes.data, n)
        return row[:n], got

    def snapshot(self):
        """state words 0 .. 30 in the layout of spangpu_modemtx_get_state()"""
        out = np.zeros(32, np.uint32)
        n = getattr(lib(), "glue_%s_snapshot" % self.name)(self.p, out.ctypes.data)
        assert n == 31
        return out[:n].copy()

    def __del__(self):
        try:
            self._f("_free")(self.p)
        except Exception:
            pass


class BitFeed:
    """A get_bit that serves what was put, then ones -- or SIG_STATUS_END_OF_DATA once end_of_data is set."""

    def __init__(self, bits=()):
        self.bits = list(bits)
        self.end_of_data = False
        self.calls = 0

    def __call__(self):
        self.calls += 1
        if self.bits:
            return self.bits.pop(0)
        return END_OF_DATA if self.end_of_data else 1
