"""A C caller of the reference's five packet loss concealment names on the GPU (tests/c_callers/plc_caller.c): an allocated
concealer and one in the caller's own storage, the voiced line through plc_rx() and plc_fillin() on the fixture's schedule,
against the samples the reference made (tests/golden/plc.npz), which this test writes out for it."""
import os

import numpy as np
import pytest

import plc_lines as PL
from test_c_callers import build, run

pytestmark = pytest.mark.gpu


def test_c_caller_by_the_spandsp_names(built, tmp_path):
    case = PL.sched_cases(PL.load())[6]
    data = os.path.join(str(tmp_path), "plc_caller.txt")
    with open(data, "w") as f:
        f.write("%d\n" % len(case.calls))
        for lost, n, row, out, _ in case.calls:
            f.write("%d %d\n%s\n%s\n" % (lost, n, " ".join(map(str, row.astype(np.int64).tolist())), " ".join(map(str, out.astype(np.int64).tolist()))))
    exe = build("plc_caller", str(tmp_path))
    out = run([exe, data])
    assert "ok %d calls, %d samples" % (len(case.calls), sum(n for _, n in PL.SCHEDULE)) in out, out
