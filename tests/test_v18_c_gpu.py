"""tests/c_callers/v18_text.c: two v18 objects by their spandsp names converse in both directions; what the program prints --
every v18_tx() return value, every put_msg call -- equals a recording of the reference doing the same."""
import numpy as np
import pytest

import v18_ref
from test_c_callers import build, run

TICK, TICKS, ANSWER_AT = 160, 420, 200


def reference_recording(mode):
    lines = []
    a, b = v18_ref.RefV18(mode, True), v18_ref.RefV18(mode, False)
    lines.append("p A %d" % a.put(b"Hello B, 1 + 1?"))
    for t in range(TICKS):
        if t == ANSWER_AT:
            lines.append("p B %d" % b.put(b"Hi A: 2!"))
        outs = []
        for s in (a, b):
            row, got = s.tx(TICK)
            full = np.zeros(TICK, np.int16)
            full[:got] = row[:got]
            outs.append((full, got))
        if outs[0][1] or outs[1][1]:
            lines.append("t %d %d %d" % (t, outs[0][1], outs[1][1]))
        for who, s, heard in (("A", a, outs[1][0]), ("B", b, outs[0][0])):
            for ch in s.rx(heard):
                lines.append("m %s %d 1 %d 0" % (who, t, ch))
    return lines


def test_v18_text_compiles(built, tmp_path):
    build("v18_text", str(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", v18_ref.MODES, ids=["4545", "476", "50"])
def test_v18_text_runs(built, tmp_path, mode):
    want = reference_recording(mode)
    assert sum(w.startswith("m A") for w in want) >= 6 and sum(w.startswith("m B") for w in want) >= 10
    exe = build("v18_text", str(tmp_path))
    out = run([exe, str(mode)]).strip().splitlines()
    assert out[0].startswith("v18_text Weitbrecht TDD (") and out[0].endswith("/ Switched to EDT mode, mode %d" % mode)
    assert out[1:] == want
