"""tests/c_callers/hdlc_frames.c: the V.21 loop -- HDLC sender bank, FSK sender bank, FSK receiver bank, HDLC receiver bank --
from plain C99 against include/spangpu.h; what the program prints, every frame_handler and status_handler call with its
tick, equals the reference's loop as recorded in tests/golden/hdlc.npz."""
import numpy as np
import pytest

import hdlc_cases as HC
from test_c_callers import build, run


def test_hdlc_frames_compiles(built, tmp_path):
    build("hdlc_frames", str(tmp_path))


@pytest.mark.gpu
def test_hdlc_frames_runs(built, tmp_path):
    g = np.load(HC.GOLDEN)
    ticks, preamble, crc32, thr = (int(x) for x in g["loop_fsk_cfg"])
    assert crc32 == 0
    ends = np.cumsum([0] + [int(x) for x in g["loop_fsk_framelens"]])
    data = g["loop_fsk_frames"].tobytes()
    frames = [data[ends[i]:ends[i + 1]] for i in range(len(ends) - 1)]
    want, at, k = [], 0, 0
    by = g["loop_fsk_bytes"].tobytes()
    for t, n in enumerate(g["loop_fsk_nrecs"]):
        for r in g["loop_fsk_recs"][k:k + n]:
            r = int(r)
            if r < 0:
                want.append("s %d %d" % (t, r))
            else:
                want.append("f %d %d %d %s" % (t, r & 0xFFFF, (r >> 16) & 1, by[at:at + (r & 0xFFFF)].hex()))
                at += r & 0xFFFF
        k += n
    assert sum(w.startswith("f") for w in want) == len(frames)
    exe = build("hdlc_frames", str(tmp_path))
    out = run([exe, str(ticks), str(preamble), str(thr)] + [f.hex() for f in frames]).strip().splitlines()
    assert out == want
