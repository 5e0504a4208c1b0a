"""Shared by the echo canceller tests of per-channel lengths and of echo groups: the line generator of
tests/test_echo_gpu.py (make_channels, copied: test files are not imported from), the state comparison against an oracle
object, a state digest, and rows in device memory."""
import ctypes
import zlib

import numpy as np


def make_channels(n_ch, n, taps, seed):
    """tx = noise (some channels get a tone burst), rx = echo through a random sparse path
    + near-end noise + double-talk bursts."""
    rng = np.random.default_rng(seed)
    tx = np.zeros((n_ch, n), np.int16)
    rx = np.zeros((n_ch, n), np.int16)
    t = np.arange(n)
    for c in range(n_ch):
        x = rng.normal(0, rng.uniform(800, 4000), n)
        if c % 3 == 1:
            a, b = sorted(rng.integers(n//4, n, 2))
            x[a:b] = 3000*np.sin(2*np.pi*rng.uniform(400, 2500)*t[a:b]/8000.0)       # narrow-band stretch
        if c % 5 == 4:
            x[:] = 0.3*x + 1500                                                     # DC offset for the HPFs
        h = np.zeros(taps)
        for k in rng.integers(0, taps, 5):
            h[k] = rng.uniform(-0.4, 0.4)
        y = np.convolve(x, h)[:n] + rng.normal(0, 15, n)
        if c % 2 == 0:
            a = int(rng.integers(n//5, n - 3000))
            y[a:a + 2500] += rng.normal(0, 7000, 2500)                               # double talk
        if c % 7 == 6:
            y *= 6.0                                                                 # gain > 1: drives the divergence zap
        tx[c] = np.clip(x, -32768, 32767).astype(np.int16)
        rx[c] = np.clip(y, -32768, 32767).astype(np.int16)
    return tx, rx


STATE_ARRAYS = ("last_acf", "taps32", "taps16", "history")


def same_state(g, o, fields):
    """None, or the first part of bank state g that differs from oracle snapshot o"""
    for key in fields:
        if g[key] != o[key]:
            return (key, g[key], o[key])
    for key in STATE_ARRAYS:
        if key in o and not np.array_equal(g[key], o[key]):
            return (key, np.nonzero(np.asarray(g[key]) != np.asarray(o[key])))
    return None


def compare_state(bank, dets, what, channels=None):
    """dets: {channel: oracle object} or a list of them"""
    from spandsp_amd import engine
    items = dets.items() if isinstance(dets, dict) else enumerate(dets)
    for c, d in items:
        if channels is not None and c not in channels:
            continue
        bad = same_state(bank.get_state(c), d.snapshot(), engine.ECHO_FIELDS)
        assert bad is None, (what, c, bad)


def state_digest(bank, channel):
    from spandsp_amd import engine
    g = bank.get_state(channel)
    crc = zlib.crc32(np.array([g[k] for k in engine.ECHO_FIELDS], np.int64).tobytes())
    for key in STATE_ARRAYS:
        crc = zlib.crc32(np.ascontiguousarray(g[key]).tobytes(), crc)
    return crc


class DeviceRows:
    """An int16 [n][stride] array in device memory (hipMalloc through the HIP runtime the library itself uses)."""
    _hip = None

    @classmethod
    def hip(cls):
        if cls._hip is None:
            h = ctypes.CDLL("libamdhip64.so")
            h.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
            h.hipFree.argtypes = [ctypes.c_void_p]
            h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            cls._hip = h
        return cls._hip

    def __init__(self, n, stride):
        self.shape = (n, stride)
        self.nbytes = n*stride*2
        self.p = ctypes.c_void_p()
        assert self.hip().hipMalloc(ctypes.byref(self.p), self.nbytes) == 0

    @property
    def ptr(self):
        return self.p.value

    def put(self, a):
        a = np.ascontiguousarray(a, np.int16)
        assert a.shape == self.shape
        assert self.hip().hipMemcpy(self.p, a.ctypes.data, self.nbytes, 1) == 0         # hipMemcpyHostToDevice

    def get(self):
        a = np.zeros(self.shape, np.int16)
        assert self.hip().hipMemcpy(a.ctypes.data, self.p, self.nbytes, 2) == 0         # hipMemcpyDeviceToHost
        return a

    def free(self):
        if self.p:
            self.hip().hipFree(self.p)
            self.p = ctypes.c_void_p()
