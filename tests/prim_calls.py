"""The fourteen spangpu_*_batch() primitives as a C caller sees them (include/spangpu.h:1555-1610), for the tests of their calling
convention: strides, shared rows, padded rows, host and device memory (tests/test_prim_extents.py, tests/test_prim_calls_gpu.py).
spandsp_amd/engine.py always passes stride == row and host memory; here every argument is laid out by hand.  Test infrastructure.

An argument is (name, dtype, words per element, row, may be shared, written, strided): the Python twin of the table in
spandsp_amd/csrc/prim_stage.hpp (tests/c_callers/prim_extents.cpp holds that table to the prototypes)."""
import ctypes as C

import numpy as np

MEM_HOST, MEM_DEVICE = 0, 1
NAN_MARK = 0x7FC0BEEF       # a quiet NaN with a payload: what the padding between float rows holds
I16_MARK = 0x7FFF


class Arg:
    def __init__(self, name, dtype, width, row, share=False, written=False, strided=False):
        self.name, self.dtype, self.width, self.row = name, np.dtype(dtype), width, row
        self.share, self.written, self.strided = share, written, strided

    def row_len(self, n):
        return {"n": n, "half": n//2, "one": 1}.get(self.row, self.row)

    def extent(self, stride, items, n):
        """the rule: elements the call touches"""
        row = self.row_len(n)
        if row == 0:
            return 0
        return row if stride == 0 else stride*(items - 1) + row


def _a(*a, **k):
    return Arg(*a, **k)


# call -> (arrays, the C parameters after `device` in order: an array's name, "<name>_stride", "items", "n", "mem", "scale",
# "phase_offset" (two floats, always host memory))
CALLS = {
    "vec_circular_dot_prodf": ([_a("x", "f4", 1, "n", share=True, strided=True), _a("y", "f4", 1, "n", share=True, strided=True),
                                _a("pos", "i4", 1, "one"), _a("z", "f4", 1, "one", written=True)],
                               ["x", "x_stride", "y", "y_stride", "pos", "z", "items", "n", "mem"]),
    "vec_circular_lmsf": ([_a("x", "f4", 1, "n", share=True, strided=True), _a("y", "f4", 1, "n", written=True, strided=True),
                           _a("pos", "i4", 1, "one"), _a("error", "f4", 1, "one")],
                          ["x", "x_stride", "y", "y_stride", "pos", "error", "items", "n", "mem"]),
    "cvec_circular_dot_prodf": ([_a("x", "f4", 2, "n", share=True, strided=True), _a("y", "f4", 2, "n", share=True, strided=True),
                                 _a("pos", "i4", 1, "one"), _a("z", "f4", 2, "one", written=True)],
                                ["x", "x_stride", "y", "y_stride", "pos", "z", "items", "n", "mem"]),
    "cvec_circular_lmsf": ([_a("x", "f4", 2, "n", share=True, strided=True), _a("y", "f4", 2, "n", written=True, strided=True),
                            _a("pos", "i4", 1, "one"), _a("error", "f4", 2, "one")],
                           ["x", "x_stride", "y", "y_stride", "pos", "error", "items", "n", "mem"]),
    "power_meter_update": ([_a("amp", "i2", 1, "n", share=True, strided=True), _a("reading", "i4", 1, "one", written=True),
                            _a("shift", "i4", 1, "one")],
                           ["amp", "amp_stride", "reading", "shift", "items", "n", "mem"]),
    "godard_ted_rx": ([_a("state", "u4", 1, 8, written=True), _a("desc", "u4", 1, 12, share=True, strided=True),
                       _a("samples", "f4", 1, "n", share=True, strided=True)],
                      ["state", "desc", "desc_stride", "samples", "samples_stride", "items", "n", "mem"]),
    "godard_ted_per_baud": ([_a("state", "u4", 1, 8, written=True), _a("desc", "u4", 1, 12, share=True, strided=True),
                             _a("correction", "i4", 1, "one", written=True)],
                            ["state", "desc", "desc_stride", "correction", "items", "mem"]),
    "periodogram": ([_a("coeffs", "f4", 2, "half", share=True, strided=True), _a("amp", "f4", 2, "n", share=True, strided=True),
                     _a("out", "f4", 2, "one", written=True)],
                    ["coeffs", "coeffs_stride", "amp", "amp_stride", "out", "items", "n", "mem"]),
    "periodogram_prepare": ([_a("amp", "f4", 2, "n", share=True, strided=True), _a("sum", "f4", 2, "half", written=True),
                             _a("diff", "f4", 2, "half", written=True)],
                            ["amp", "amp_stride", "sum", "diff", "items", "n", "mem"]),
    "periodogram_apply": ([_a("coeffs", "f4", 2, "half", share=True, strided=True), _a("sum", "f4", 2, "half"), _a("diff", "f4", 2, "half"),
                           _a("out", "f4", 2, "one", written=True)],
                          ["coeffs", "coeffs_stride", "sum", "diff", "out", "items", "n", "mem"]),
    "periodogram_freq_error": ([_a("last_result", "f4", 2, "one"), _a("result", "f4", 2, "one"), _a("out", "f4", 1, "one", written=True)],
                               ["phase_offset", "scale", "last_result", "result", "out", "items", "mem"]),
    "fixed_sqrt32": ([_a("x", "u4", 1, "one"), _a("out", "u2", 1, "one", written=True)], ["x", "out", "items", "mem"]),
    "dds_complexf": ([_a("phase_acc", "u4", 1, "one", written=True), _a("phase_rate", "i4", 1, "one"), _a("out", "f4", 2, "n", written=True)],
                     ["phase_acc", "phase_rate", "out", "items", "n", "mem"]),
    "arctan2": ([_a("y", "f4", 1, "one"), _a("x", "f4", 1, "one"), _a("out", "i4", 1, "one", written=True)], ["y", "x", "out", "items", "mem"]),
}


def args_of(call):
    return {a.name: a for a in CALLS[call][0]}


def bind(L):
    """argtypes of the fourteen entry points on a ctypes library"""
    for call, (arrays, params) in CALLS.items():
        names = {a.name for a in arrays}
        types = [C.c_int]
        for p in params:
            if p in names or p == "phase_offset":
                types.append(C.c_void_p)
            elif p.endswith("_stride"):
                types.append(C.c_longlong)
            elif p == "scale":
                types.append(C.c_float)
            else:
                types.append(C.c_int)
        f = getattr(L, "spangpu_%s_batch" % call)
        f.argtypes = types
        f.restype = C.c_int
    return L


def invoke(L, call, ptrs, strides, items, n, mem, scale=0.0, device=0):
    """ptrs: name -> address (phase_offset included where the call has one); strides: name -> elements"""
    argv = [device]
    for p in CALLS[call][1]:
        if p.endswith("_stride"):
            argv.append(int(strides[p[:-7]]))
        elif p == "items":
            argv.append(items)
        elif p == "n":
            argv.append(n)
        elif p == "mem":
            argv.append(mem)
        elif p == "scale":
            argv.append(float(scale))
        else:
            argv.append(int(ptrs[p]))
    return getattr(L, "spangpu_%s_batch" % call)(*argv)


def mark_of(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.dtype("i2"):
        return np.array([I16_MARK], "i2")[0]
    return np.array([NAN_MARK], "u4").view(dtype)[0]


def lay_out(arg, rows, stride, items, n, guard=0):
    """rows [items or 1][row*width] as the caller's array: `extent` elements, row i at i*stride, the padding between rows
    marked; then `guard` words of 0xA5 bytes behind the extent, in the same buffer.  Returns the flat buffer (words)."""
    w = arg.width
    row = arg.row_len(n)*w
    ext = arg.extent(stride, items, n)*w
    buf = np.empty(ext + guard, arg.dtype)
    buf[:ext] = mark_of(arg.dtype)
    buf[ext:].view(np.uint8)[:] = 0xA5
    if row:
        for i in range(1 if stride == 0 else items):
            buf[i*stride*w:i*stride*w + row] = rows[i]
    return buf


def rows_of(arg, buf, stride, items, n):
    """the rows back out of a laid out buffer, [items or 1][row*width]"""
    w = arg.width
    row = arg.row_len(n)*w
    k = 1 if stride == 0 else items
    return np.stack([buf[i*stride*w:i*stride*w + row] for i in range(k)]) if row else np.zeros((k, 0), arg.dtype)


def rest_of(arg, buf, stride, items, n):
    """everything of a laid out buffer that is no row: the padding, then the guard"""
    w = arg.width
    row = arg.row_len(n)*w
    keep = np.ones(len(buf), bool)
    for i in range(1 if stride == 0 else items):
        keep[i*stride*w:i*stride*w + row] = False
    return buf[keep]


class Hip:
    """hipMalloc'd blocks of exactly the bytes asked for, through the runtime the library uses"""

    def __init__(self):
        h = C.CDLL("libamdhip64.so")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        h.hipFree.argtypes = [C.c_void_p]
        self.h = h
        self.blocks = []

    def put(self, a):
        """a block as long as `a` (16 bytes where `a` is empty: a pointer the call can take), filled with it"""
        a = np.ascontiguousarray(a)
        nbytes = max(a.nbytes, 16) if a.nbytes == 0 else a.nbytes
        p = C.c_void_p()
        assert self.h.hipMalloc(C.byref(p), nbytes) == 0
        self.blocks.append(p)
        assert self.h.hipMemset(p, 0, nbytes) == 0 and self.h.hipDeviceSynchronize() == 0
        if a.nbytes:
            assert self.h.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p.value

    def get(self, ptr, like):
        """plain hipMemcpy, nothing waited for beforehand"""
        a = np.empty_like(like)
        if a.nbytes:
            assert self.h.hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0
        return a

    def free(self):
        for p in self.blocks:
            self.h.hipFree(p)
        self.blocks = []
