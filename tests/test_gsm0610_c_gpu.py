"""A C caller of the reference's twelve GSM 06.10 names on the GPU (tests/c_callers/gsm0610_caller.c): a caller-supplied encoder
state and an allocated decoder, the pulse-train line -> VoIP frames -> samples in calls of two frames, every frame through the
host packers and unpackers into the other two packings, and gsm0610_set_packing() in mid-stream, against the bytes and samples
the reference made (tests/golden/gsm0610.npz), which this test writes out for it.  (The fixture's codecs took the same stream
on another cut; the stream does not depend on the cut, which tests/c_callers/gsm0610_host.cpp holds case by case.)"""
import os

import numpy as np
import pytest

import gsm0610_lines as GL
from test_c_callers import build, run

pytestmark = pytest.mark.gpu


def test_c_caller_by_the_spandsp_names(built, tmp_path):
    cases = {(c.kind, c.packing, c.line): c for c in GL.cases(GL.load())}
    enc = {p: cases[(GL.ENCODE, p, 1)] for p in GL.PACKINGS}
    dec = cases[(GL.DECODE, GL.VOIP, 1)]
    assert np.array_equal(enc[GL.VOIP].want, dec.data)
    data = os.path.join(str(tmp_path), "gsm0610_caller.txt")
    with open(data, "w") as f:
        for block in (enc[GL.VOIP].data, enc[GL.VOIP].want, enc[GL.WAV49].want, enc[GL.NONE].want, dec.want):
            f.write("%d\n%s\n" % (len(block), " ".join(map(str, np.asarray(block).astype(np.int64).tolist()))))
    exe = build("gsm0610_caller", str(tmp_path))
    out = run([exe, data])
    assert "ok %d samples, %d bytes" % (len(enc[GL.VOIP].data), len(enc[GL.VOIP].want)) in out, out
