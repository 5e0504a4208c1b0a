"""A C caller of the reference's G.726 names on the GPU (tests/c_callers/g726_transcode.c): a caller-supplied encoder state and
an allocated decoder, A-law -> 32 kbit/s right-packed -> A-law on the fixture's call schedule, against the bytes the
reference made (tests/golden/g726.npz), which this test writes out for it."""
import os

import numpy as np
import pytest

import g726_lines as GL
from test_c_callers import build, run

pytestmark = pytest.mark.gpu


def test_c_caller_by_the_spandsp_names(built, tmp_path):
    cases = {(c.kind, c.rate, c.coding, c.packing, c.line): c for c in GL.cases(GL.load())}
    enc = cases[(GL.ENCODE, 32000, GL.ALAW, GL.PACK_RIGHT, 0)]
    dec = cases[(GL.DECODE, 32000, GL.ALAW, GL.PACK_RIGHT, 0)]
    assert np.array_equal(enc.want, dec.data)
    data = os.path.join(str(tmp_path), "g726_transcode.txt")
    with open(data, "w") as f:
        for block in (enc.data, enc.want, dec.want):
            f.write("%d\n%s\n" % (len(block), " ".join(map(str, np.asarray(block).astype(np.int64).tolist()))))
    exe = build("g726_transcode", str(tmp_path))
    out = run([exe, data])
    assert "ok %d samples, %d bytes" % (len(enc.data), len(enc.want)) in out, out
