"""The calling convention of the fourteen spangpu_*_batch() primitives, on the host.

spandsp_amd/csrc/prim_stage.hpp is the one place that says which strides such a call accepts and how many elements of an
array it touches (stride 0 only for a row that may be shared and is not written, otherwise stride >= row; extent
stride*(items - 1) + row); prim_api.hip and prim2_api.hip take every staging and copy-back count from it.  It makes no GPU
call, so tests/c_callers/prim_extents.cpp drives it alone -- the rule against the indices the kernels form, overflow, and the
table of arguments against what the prototypes promise (coeffs[len/2] among them) -- under -fsanitize=address,undefined (host
code only, a program of its own).  Bytes staged past a caller's array and copied back unchanged leave no trace a GPU test
could see: this is where they are excluded.

The refusals need no GPU either: every argument check of these calls comes before the device check."""
import os
import subprocess

import numpy as np
import pytest

import prim_calls as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_staging_rule_and_the_table_of_arguments(tmp_path):
    exe = os.path.join(str(tmp_path), "prim_extents")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           "-I" + os.path.join(ROOT, "spandsp_amd", "csrc"), os.path.join(ROOT, "tests", "c_callers", "prim_extents.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    p = subprocess.run([exe], capture_output=True, text=True)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "cases: ok" in out and "Sanitizer" not in out and "runtime error" not in out, out


def test_the_entry_points_count_with_the_rule_alone():
    """prim_api.hip and prim2_api.hip hold no staging or copy-back count of their own: no copy, allocation or size arithmetic
    outside the shared helper (prim_stage_hip.hpp), and every array goes through stage() with a constant of the table."""
    import re
    table = open(os.path.join(ROOT, "spandsp_amd", "csrc", "prim_stage.hpp")).read()
    consts = set(re.findall(r"X\((k\w+),", table))
    assert len(consts) == 46
    staged = set()
    for unit in ("prim_api.hip", "prim2_api.hip"):
        text = open(os.path.join(ROOT, "spandsp_amd", "csrc", unit)).read()
        api = text[text.index('extern "C" {'):]
        for word in ("hipMemcpy", "hipMalloc", "sizeof", "size_t)", "*items", "items*", "stride*", "stride *"):
            assert word not in api, (unit, word)
        staged |= set(re.findall(r"call\.stage\((k\w+),", api))
        assert set(re.findall(r"call\.arg\((k\w+),", api)) == set(re.findall(r"call\.stage\((k\w+),", api)), unit
    assert staged == consts


# ---- refusals: SPANGPU_ERR_BAD_ARG (-2) with or without a GPU ------------------------------------------------------------

ITEMS, N = 3, 4


def well_formed(call):
    """small host arrays, every stride the row itself"""
    arrays, _ = PC.CALLS[call]
    bufs, ptrs, strides = {}, {}, {}
    for a in arrays:
        stride = a.row_len(N)
        rows = np.ones((ITEMS, stride*a.width), a.dtype)
        bufs[a.name] = PC.lay_out(a, rows, stride, ITEMS, N, guard=4)
        ptrs[a.name] = bufs[a.name].ctypes.data
        strides[a.name] = stride
    if "phase_offset" in PC.CALLS[call][1]:
        bufs["phase_offset"] = np.array([1.0, 0.0], np.float32)
        ptrs["phase_offset"] = bufs["phase_offset"].ctypes.data
    return bufs, ptrs, strides


@pytest.fixture(scope="module")
def L(built):
    from spandsp_amd import engine
    return PC.bind(engine.lib())


@pytest.mark.parametrize("call", sorted(PC.CALLS))
def test_bad_strides_and_memory_kinds_are_refused_before_any_device_work(L, call):
    bufs, ptrs, strides = well_formed(call)
    assert PC.invoke(L, call, ptrs, strides, ITEMS, N, 7) == -2                         # neither host nor device memory
    assert PC.invoke(L, call, ptrs, strides, ITEMS, N, -1) == -2
    assert PC.invoke(L, call, ptrs, strides, 0, N, PC.MEM_HOST) == -2
    tried = 0
    for a in PC.CALLS[call][0]:
        if not a.strided:
            continue
        row = a.row_len(N)
        assert row >= 2
        for bad in [-1, -row, row - 1, 1] + ([0] if a.written else []):
            for items in (ITEMS, 1):
                for mem in (PC.MEM_HOST, PC.MEM_DEVICE):                                # (refused before anybody looks at a pointer)
                    s = dict(strides)
                    s[a.name] = bad
                    assert PC.invoke(L, call, ptrs, s, items, N, mem) == -2, (a.name, bad, items, mem)
                    tried += 1
    assert tried == 16*sum(a.strided for a in PC.CALLS[call][0]) + 4*sum(a.strided and a.written for a in PC.CALLS[call][0])
    for p in list(ptrs):
        q = dict(ptrs)
        q[p] = 0
        assert PC.invoke(L, call, q, strides, ITEMS, N, PC.MEM_HOST) == -2, p          # a NULL array
    if "pos" in ptrs:
        for bad in (-1, N + 1):
            bufs["pos"][1] = bad
            assert PC.invoke(L, call, ptrs, strides, ITEMS, N, PC.MEM_HOST) == -2       # a position outside its row, host memory
        bufs["pos"][1] = 1
    if call in ("periodogram_prepare", "periodogram_apply"):
        assert PC.invoke(L, call, ptrs, dict(strides, amp=1, coeffs=0), ITEMS, 1, PC.MEM_HOST) == -2        # no half to write or read


@pytest.mark.parametrize("call", sorted(PC.CALLS))
def test_a_well_formed_call_finds_no_device(L, call):
    """... and says so (-1): the arguments above were refused for what they were, not because nothing runs here"""
    from spandsp_amd import engine
    if engine.device_count() > 0:
        pytest.skip("a GPU is visible")
    bufs, ptrs, strides = well_formed(call)
    assert PC.invoke(L, call, ptrs, strides, ITEMS, N, PC.MEM_HOST) == -1
    assert PC.invoke(L, call, ptrs, strides, ITEMS, N, PC.MEM_DEVICE) == -1
    shared = {a.name: (0 if a.share else strides[a.name]) for a in PC.CALLS[call][0]}
    assert PC.invoke(L, call, ptrs, shared, ITEMS, N, PC.MEM_HOST) == -1
    if call == "periodogram":
        assert PC.invoke(L, call, ptrs, dict(strides, coeffs=0, amp=1), ITEMS, 1, PC.MEM_HOST) == -1        # len 1 stays accepted
