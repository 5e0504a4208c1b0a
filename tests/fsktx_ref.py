"""Live objects of the real reference for the sender tests: fsk_tx, modem_connect_tones_tx and async_tx through the checker
library oracle/ref.py opens, with the few prototypes ref.py does not declare."""
import ctypes as C

import numpy as np

END_OF_DATA = -7            # SIG_STATUS_END_OF_DATA, async.h
SHUTDOWN_COMPLETE = -10
LINK_IDLE = -17
GET = C.CFUNCTYPE(C.c_int, C.c_void_p)
STATUS = C.CFUNCTYPE(None, C.c_void_p, C.c_int)
SPEC_BYTES = 32             # sizeof(fsk_spec_t): a name pointer and five ints

SCHEDULE = [160, 160, 77, 1, 8, 333, 160, 1024, 5, 160]
BAUD_RATES = [30000, 30000, 120000, 7500, 30000, 30000, 120000, 4545, 5000, 4760, 11000]

_declared = []


def lib():
    from oracle import ref
    L = ref.lib()
    if not _declared:
        vp, ci = C.c_void_p, C.c_int
        for name, res, args in [("fsk_tx_init", vp, [vp, vp, vp, vp]), ("fsk_tx_restart", ci, [vp, vp]),
                                ("fsk_tx_set_modem_status_handler", None, [vp, vp, vp]),
                                ("async_tx_init", vp, [vp, ci, ci, ci, C.c_bool, vp, vp]), ("async_tx_get_bit", ci, [vp]),
                                ("async_tx_presend_bits", None, [vp, ci]), ("async_tx_free", ci, [vp])]:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _declared.append(True)
    return L


def spec_ptr(which):
    return C.c_void_p(C.addressof(C.c_char.in_dll(lib(), "preset_fsk_specs")) + SPEC_BYTES*which)


class RefFskTx:
    """fsk_tx_init(NULL, &preset_fsk_specs[which], get_bit, user): get_bit is the checker's LFSR on `seed`, or a Python
    callable.  tx(n) runs fsk_tx() into a zero-filled row and returns (row, returned length)."""

    def __init__(self, which, seed=None, get_bit=None):
        L = lib()
        if get_bit is None:
            self.st = (C.c_uint32*1)(seed & 0x7FFF)
            self.p = L.fsk_tx_init(None, spec_ptr(which), L.glue_fn_prbs_get_bit(), C.cast(self.st, C.c_void_p))
        else:
            self.cb = GET(lambda _: get_bit())
            self.p = L.fsk_tx_init(None, spec_ptr(which), C.cast(self.cb, C.c_void_p), None)
        self.status = []
        self.scb = STATUS(lambda _, s: self.status.append(s))
        L.fsk_tx_set_modem_status_handler(self.p, C.cast(self.scb, C.c_void_p), None)

    def tx(self, n):
        row = np.zeros(n, np.int16)
        got = lib().fsk_tx(self.p, row.ctypes.data, n)
        return row, got

    def power(self, dbm0):
        lib().fsk_tx_power(self.p, dbm0)

    def restart(self, which):
        lib().fsk_tx_restart(self.p, spec_ptr(which))

    def __del__(self):
        try:
            lib().fsk_tx_free(self.p)
        except Exception:
            pass


class BitFeed:
    """A get_bit that serves what was put, then marks -- or SIG_STATUS_END_OF_DATA once end_of_data is set."""

    def __init__(self):
        self.bits = []
        self.end_of_data = False
        self.calls = 0

    def __call__(self):
        self.calls += 1
        if self.bits:
            return self.bits.pop(0)
        return END_OF_DATA if self.end_of_data else 1


class RefAsyncTx:
    """async_tx_init(NULL, data_bits, parity, stop_bits, false, get_byte, user) with a get_byte that hands out what was
    put and then SIG_STATUS_LINK_IDLE."""

    def __init__(self, data_bits, parity, stop_bits):
        self.bytes = []
        self.cb = GET(lambda _: self.bytes.pop(0) if self.bytes else LINK_IDLE)
        self.p = lib().async_tx_init(None, data_bits, parity, stop_bits, False, C.cast(self.cb, C.c_void_p), None)

    def put(self, data):
        self.bytes += list(data)

    def presend(self, bits):
        lib().async_tx_presend_bits(self.p, bits)

    def get_bit(self):
        return lib().async_tx_get_bit(self.p)

    def __del__(self):
        try:
            lib().async_tx_free(self.p)
        except Exception:
            pass


class RefMctTx:
    def __init__(self, tone_type):
        self.type = tone_type
        self.p = lib().modem_connect_tones_tx_init(None, tone_type)

    def restart(self):
        lib().modem_connect_tones_tx_free(self.p)
        self.p = lib().modem_connect_tones_tx_init(None, self.type)

    def tx(self, n):
        row = np.zeros(n, np.int16)
        got = lib().modem_connect_tones_tx(self.p, row.ctypes.data, n)
        return row, got

    def __del__(self):
        try:
            lib().modem_connect_tones_tx_free(self.p)
        except Exception:
            pass


class DeviceRows:
    """[n][stride] int16 in HBM, for the calls that take device pointers."""

    def __init__(self, n, stride):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.n, self.stride = n, stride
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), n*stride*2) == 0
        self.lens = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.lens), n*4) == 0

    def fill(self, byte):
        # (hipMemset of device memory returns before it has run, and the banks' streams do not wait for the null stream)
        assert self.hip.hipMemset(self.ptr, byte, self.n*self.stride*2) == 0
        assert self.hip.hipDeviceSynchronize() == 0

    def rows(self):
        host = np.zeros((self.n, self.stride), np.int16)
        assert self.hip.hipMemcpy(host.ctypes.data, self.ptr, host.nbytes, 2) == 0
        return host

    def lengths(self):
        host = np.zeros(self.n, np.int32)
        assert self.hip.hipMemcpy(host.ctypes.data, self.lens, host.nbytes, 2) == 0
        return host

    def free(self):
        self.hip.hipFree(self.ptr)
        self.hip.hipFree(self.lens)
