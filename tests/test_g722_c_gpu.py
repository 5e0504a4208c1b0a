"""A C caller of the reference's G.722 names on the GPU (tests/c_callers/g722_caller.c): a caller-supplied encoder state and an
allocated decoder, a 16 kHz line -> 56 kbit/s packed -> 16 kHz in calls of 160 samples, against the bytes and samples the
reference made (tests/golden/g722.npz), which this test writes out for it.  (The fixture's decoder took the same bytes on
another cut; the decoder's stream does not depend on the cut, which tests/c_callers/g722_host.cpp holds case by case.)"""
import os

import numpy as np
import pytest

import g722_lines as GL
from test_c_callers import build, run

pytestmark = pytest.mark.gpu


def test_c_caller_by_the_spandsp_names(built, tmp_path):
    cases = {(c.kind, c.rate, c.eight_k, c.packed, c.line): c for c in GL.cases(GL.load())}
    enc = cases[(GL.ENCODE, 56000, 0, 1, 0)]
    dec = cases[(GL.DECODE, 56000, 0, 1, 0)]
    assert np.array_equal(enc.want, dec.data)
    data = os.path.join(str(tmp_path), "g722_caller.txt")
    with open(data, "w") as f:
        for block in (enc.data, enc.want, dec.want):
            f.write("%d\n%s\n" % (len(block), " ".join(map(str, np.asarray(block).astype(np.int64).tolist()))))
    exe = build("g722_caller", str(tmp_path))
    out = run([exe, data])
    assert "ok %d samples, %d bytes" % (len(enc.data), len(enc.want)) in out, out
