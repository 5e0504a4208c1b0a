"""The calling convention of the fourteen spangpu_*_batch() primitives on the GPU: padded strides, shared rows (stride 0), host
and device memory, item counts around the 64- and 256-lane blocks.

The value tests (test_prim_gpu.py, test_prim2_gpu.py, test_shim_prims_gpu.py) go through spandsp_amd/engine.py, which always
passes stride == row and host memory.  Here every call is made through ctypes with arrays laid out by hand (tests/prim_calls.py):
exactly the elements the rule of csrc/prim_stage.hpp gives (proven on the host in tests/test_prim_extents.py), device arrays
from hipMalloc of exactly that many bytes, the padding between rows marked (a NaN with a payload, 0x7FFF in int16 rows) and,
in host memory, a guard behind the extent in the same buffer.  Expected values come from the restatements the value tests
trust, computed on dense copies of the rows and never from a GPU call: the binary32 loops of test_prim_gpu.py,
prims2.Restated, godard_np() of test_shim_prims_gpu.py.  Bar: bit-exact, any NaN counting as NaN; the inputs hold no NaN, so a
padding element that reached a result shows."""
import numpy as np
import pytest

import prim_calls as PC
import prims2
from test_oracle_pin import use_golden_modem_tables
from test_prim_gpu import ref_clms, ref_cdot, ref_dot, ref_lms, ref_power
from test_shim_prims_gpu import godard_np

pytestmark = pytest.mark.gpu

MAX = 257
ITEMS = (1, 64, 65, 257)            # blocks are 64 lanes, 256 for fixed_sqrt32 and arctan2
ROWS = {"vec_circular_dot_prodf": (1, 27), "vec_circular_lmsf": (1, 27), "cvec_circular_dot_prodf": (1, 33), "cvec_circular_lmsf": (1, 33),
        "power_meter_update": (1, 160), "godard_ted_rx": (5,), "godard_ted_per_baud": (5,),
        "periodogram": (1, 2, 3, 33), "periodogram_prepare": (2, 3, 33), "periodogram_apply": (2, 3, 33),      # (an odd len never reads its middle sample)
        "periodogram_freq_error": (1,), "fixed_sqrt32": (1,), "dds_complexf": (1, 7), "arctan2": (1,)}
PAD = 3
PHASE_OFFSET = np.array([0.6, -0.8], np.float32)
SCALE = 31.5


@pytest.fixture(scope="module")
def L(built):
    from spandsp_amd import engine
    use_golden_modem_tables()
    return PC.bind(engine.lib())


def godard_words(rng, items):
    state = np.zeros((items, 8), np.uint32)
    state[:, :7] = rng.normal(0.0, 3.0, (items, 7)).astype(np.float32).view(np.uint32)
    state[:, 7] = rng.integers(-50, 50, items).astype(np.int32).view(np.uint32)
    desc = np.zeros((items, 12), np.uint32)
    desc[:, :9] = rng.normal(0.0, 1.0, (items, 9)).astype(np.float32).view(np.uint32)
    desc[:, 7] = np.abs(rng.normal(6.0, 2.0, items)).astype(np.float32).view(np.uint32)          # coarse trigger
    desc[:, 8] = np.abs(rng.normal(1.0, 0.5, items)).astype(np.float32).view(np.uint32)          # fine trigger
    desc[:, 9] = 15
    desc[:, 10] = 1
    return state, desc


def godard_item(state, desc, x, baud_at):
    """godard_np() on one item's words -> its eight state words and the return values"""
    d = desc.view(np.float32)
    dd = (d[0:3], d[3:6], d[6], d[7], d[8], int(desc[9]), int(desc[10]))
    s0 = list(state[:7].view(np.float32)) + [int(state[7:8].view(np.int32)[0])]
    wf, wt, wr = godard_np(s0, dd, x, baud_at)
    out = np.zeros(8, np.uint32)
    out[:7] = wf.view(np.uint32)
    out[7] = np.array([wt], np.int32).view(np.uint32)[0]
    return out, wr


_inputs = {}


def inputs(call, n):
    """dense rows [MAX][row*width] of every array of a call, outputs holding the mark; made once"""
    if (call, n) in _inputs:
        return _inputs[(call, n)]
    rng = np.random.default_rng(sorted(PC.CALLS).index(call)*1000 + n)
    d = {}
    for a in PC.CALLS[call][0]:
        shape = (MAX, a.row_len(n)*a.width)
        if a.name == "pos":
            d[a.name] = rng.integers(0, n + 1, shape).astype(np.int32)
            d[a.name][:2, 0] = [0, n]
        elif a.dtype == np.dtype("f4"):
            d[a.name] = rng.normal(0.0, 2.0, shape).astype(np.float32)
        elif a.dtype == np.dtype("i2"):
            d[a.name] = rng.integers(-32768, 32768, shape).astype(np.int16)
        elif a.name == "shift":
            d[a.name] = rng.integers(1, 12, shape).astype(np.int32)
        elif a.name == "reading":
            d[a.name] = rng.integers(0, 1 << 30, shape).astype(np.int32)
        else:
            d[a.name] = rng.integers(0, 1 << 8*a.dtype.itemsize, shape, dtype=np.uint64).astype("u%d" % a.dtype.itemsize).view(a.dtype)
        if a.written and a.name not in ("y", "reading", "state", "phase_acc"):
            d[a.name][:] = PC.mark_of(a.dtype)
    if call.startswith("godard"):
        d["state"], d["desc"] = godard_words(rng, MAX)
    if call == "godard_ted_per_baud":
        # the state a baud meets: after five samples, by the restatement
        d["first_state"] = d["state"]
        d["samples"] = rng.normal(0.0, 2.0, (MAX, n)).astype(np.float32)
    _inputs[(call, n)] = d
    return d


_wants = {}


def want(call, n, shared):
    """what the call leaves in its written arrays, dense rows [MAX][..], from the restatements; made once per set of shared rows"""
    key = (call, n, tuple(sorted(shared)))
    if key in _wants:
        return _wants[key]
    d = inputs(call, n)
    e = {k: (np.repeat(v[:1], MAX, 0) if k in shared else v) for k, v in d.items()}
    c64 = np.complex64
    R = prims2.Restated()
    with np.errstate(all="ignore"):
        if call == "vec_circular_dot_prodf":
            w = {"z": np.array([[ref_dot(e["x"][i], e["y"][i], int(e["pos"][i, 0]))] for i in range(MAX)], np.float32)}
        elif call == "vec_circular_lmsf":
            w = {"y": np.stack([ref_lms(e["x"][i], e["y"][i], int(e["pos"][i, 0]), e["error"][i, 0]) for i in range(MAX)])}
        elif call == "cvec_circular_dot_prodf":
            z = np.array([ref_cdot(e["x"][i].view(c64), e["y"][i].view(c64), int(e["pos"][i, 0])) for i in range(MAX)], c64)
            w = {"z": z.view(np.float32).reshape(MAX, 2)}
        elif call == "cvec_circular_lmsf":
            y = np.stack([ref_clms(e["x"][i].view(c64), e["y"][i].view(c64), int(e["pos"][i, 0]), e["error"][i].view(c64)[0]) for i in range(MAX)])
            w = {"y": y.astype(c64).view(np.float32).reshape(MAX, 2*n)}
        elif call == "power_meter_update":
            w = {"reading": np.array([[ref_power(e["amp"][i], e["reading"][i, 0], e["shift"][i, 0])] for i in range(MAX)], np.int32)}
        elif call == "godard_ted_rx":
            w = {"state": np.stack([godard_item(e["state"][i], e["desc"][i], e["samples"][i], set())[0] for i in range(MAX)])}
        elif call == "godard_ted_per_baud":
            both = [godard_item(e["first_state"][i], e["desc"][i], e["samples"][i], {n - 1}) for i in range(MAX)]
            w = {"state": np.stack([b[0] for b in both]), "correction": np.array([[b[1][0]] for b in both], np.int32)}
        elif call == "periodogram":
            w = {"out": R.periodogram(e["coeffs"].reshape(MAX, n//2, 2), e["amp"].reshape(MAX, n, 2), n)}
        elif call == "periodogram_prepare":
            s, df = R.prepare(e["amp"].reshape(MAX, n, 2), n)
            w = {"sum": s.reshape(MAX, -1), "diff": df.reshape(MAX, -1)}
        elif call == "periodogram_apply":
            w = {"out": R.apply(e["coeffs"].reshape(MAX, n//2, 2), e["sum"].reshape(MAX, n//2, 2), e["diff"].reshape(MAX, n//2, 2), n)}
        elif call == "periodogram_freq_error":
            w = {"out": R.freq_error(PHASE_OFFSET, SCALE, e["last_result"], e["result"]).reshape(MAX, 1)}
        elif call == "fixed_sqrt32":
            w = {"out": R.sqrt32(np.ascontiguousarray(e["x"][:, 0])).reshape(MAX, 1)}
        elif call == "dds_complexf":
            out, acc = R.dds(e["phase_acc"][:, 0].copy(), e["phase_rate"][:, 0].copy(), n)      # (the restatement advances its copy)
            w = {"out": out.reshape(MAX, 2*n), "phase_acc": acc.reshape(MAX, 1)}
        else:
            w = {"out": R.arctan2(np.ascontiguousarray(e["y"][:, 0]), np.ascontiguousarray(e["x"][:, 0])).reshape(MAX, 1)}
    _wants[key] = w
    return w


_baud = {}


def baud_data(n, shared):
    """the arrays of a per_baud case: the state a baud meets is the restatement's after the row of samples, under the
    descriptors the items will see"""
    key = (n, tuple(sorted(shared)))
    if key not in _baud:
        d = dict(inputs("godard_ted_per_baud", n))
        desc = np.repeat(d["desc"][:1], MAX, 0) if "desc" in shared else d["desc"]
        d["state"] = np.stack([godard_item(d["first_state"][i], desc[i], d["samples"][i], set())[0] for i in range(MAX)])
        _baud[key] = d
    return _baud[key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.dtype("f4"):
        return np.array_equal(prims2.nan_canon(a), prims2.nan_canon(b))
    return a.tobytes() == b.tobytes()


def variants(call):
    """the strides of a call's arrays as name -> 'row' | 'pad' | 0"""
    arrays = PC.CALLS[call][0]
    strided = [a.name for a in arrays if a.strided]
    share = [a.name for a in arrays if a.share]
    if not strided:
        return [{}]
    out = [{k: "row" for k in strided}, {k: "pad" for k in strided}]
    for k in share:                                                             # one argument at a time ...
        out.append({j: (0 if j == k else "pad") for j in strided})
    if len(share) > 1:                                                          # ... and all together
        out.append({j: (0 if j in share else "pad") for j in strided})
    return out


def run(L, call, items, n, how, mem, data=None, ret=0):
    """one call; checks what it must leave alone (read-only arrays, padding, guard) and returns the rows of every array after it"""
    arrays = PC.CALLS[call][0]
    d = data or inputs(call, n)
    strides, before, ptrs = {}, {}, {}
    hip = PC.Hip() if mem == PC.MEM_DEVICE else None
    for a in arrays:
        row = a.row_len(n)
        s = how.get(a.name, "row")
        strides[a.name] = row if s == "row" else row + PAD if s == "pad" else 0
        rows = d[a.name][:1 if strides[a.name] == 0 else items]
        before[a.name] = PC.lay_out(a, rows, strides[a.name], items, n, guard=0 if hip else 8)
    after = {k: v.copy() for k, v in before.items()}
    for a in arrays:
        ptrs[a.name] = hip.put(after[a.name]) if hip else after[a.name].ctypes.data
    ptrs["phase_offset"] = PHASE_OFFSET.ctypes.data                             # host memory in either case
    rc = PC.invoke(L, call, ptrs, strides, items, n, mem, SCALE)
    if hip:
        for a in arrays:
            after[a.name] = hip.get(ptrs[a.name], before[a.name])               # the call has waited: a plain copy sees the result
        hip.free()
    assert rc == ret, (call, items, n, how, mem, rc)
    rows = {}
    for a in arrays:
        s = strides[a.name]
        what = (call, a.name, items, n, how, mem)
        if not a.written:
            assert after[a.name].tobytes() == before[a.name].tobytes(), what
        # the padding between the rows and, in host memory, the guard behind the extent
        assert PC.rest_of(a, after[a.name], s, items, n).tobytes() == PC.rest_of(a, before[a.name], s, items, n).tobytes(), what
        rows[a.name] = PC.rows_of(a, after[a.name], s, items, n)
    return rows


@pytest.mark.parametrize("call", sorted(PC.CALLS))
def test_strides_shared_rows_and_memory_kinds(L, call):
    checked = 0
    for n in ROWS[call]:
        ret = n//2 if call == "periodogram_prepare" else 0
        for how in variants(call):
            shared = [k for k, s in how.items() if s == 0]
            if "coeffs" in how and n == 1 and how["coeffs"] == "row":
                shared.append("coeffs")                                         # (a row of none: its own stride is 0)
            w = want(call, n, shared)
            data = baud_data(n, shared) if call == "godard_ted_per_baud" else None
            for items in ITEMS:
                got = {mem: run(L, call, items, n, how, mem, data=data, ret=ret) for mem in (PC.MEM_HOST, PC.MEM_DEVICE)}
                for mem, rows in got.items():
                    for name, rows_want in w.items():
                        assert same_bits(rows[name], rows_want[:items]), (call, name, items, n, how, mem)
                        checked += 1
                # the arrays advanced in place (y, reading, state, phase_acc) and the outputs: device memory as host memory
                for name in w:
                    assert got[PC.MEM_HOST][name].tobytes() == got[PC.MEM_DEVICE][name].tobytes(), (call, name, items, n, how)
    assert checked >= 2*len(ITEMS)*len(ROWS[call])*len(variants(call))


@pytest.mark.parametrize("call", ["vec_circular_dot_prodf", "vec_circular_lmsf", "cvec_circular_dot_prodf", "cvec_circular_lmsf"])
def test_a_position_outside_its_row_in_device_memory(L, call):
    """Nobody reads device memory beforehand: the call is not refused, the item's dot product is NaN, its y row is untouched, and
    its neighbours in the same wave are right.  (In host memory the same call is refused.)"""
    n = ROWS[call][1]
    items = 65
    d = dict(inputs(call, n))
    d["pos"] = d["pos"].copy()
    out = {3: -1, 40: n + 1, 64: n + 1}
    for i, p in out.items():
        d["pos"][i, 0] = p
    how = {"x": "pad", "y": "pad"}
    run(L, call, items, n, how, PC.MEM_HOST, data=d, ret=-2)
    rows = run(L, call, items, n, how, PC.MEM_DEVICE, data=d)
    w = want(call, n, [])
    name = "z" if "z" in w else "y"
    ok = np.array([i not in out for i in range(items)])
    assert same_bits(rows[name][ok], w[name][:items][ok])
    for i in out:
        if name == "z":
            assert np.all(np.isnan(rows["z"][i]))
        else:
            assert rows["y"][i].tobytes() == d["y"][i].tobytes()
