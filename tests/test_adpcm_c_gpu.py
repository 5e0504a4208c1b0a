"""A C caller of the reference's IMA and OKI ADPCM names on the GPU (tests/c_callers/adpcm_caller.c, C99 -pedantic against
include/ alone): a VDVI encoder in caller storage and an allocated decoder, packet for packet, then OKI at 24 kbit/s, both in
pieces on the fixtures' schedule, against FNV-1a sums committed with the program.  This test writes the line out for it and
holds the committed sums against the fixtures (tests/golden/ima_adpcm.npz, oki_adpcm.npz)."""
import os
import re

import numpy as np
import pytest

import adpcm_lines as AL
from test_c_callers import SRC, build, run

pytestmark = pytest.mark.gpu


def fnv(data):
    h = 2166136261
    for b in np.asarray(data).tobytes():
        h = ((h ^ b)*16777619) & 0xFFFFFFFF
    return h


def test_c_caller_by_the_spandsp_names(built, tmp_path):
    ima = {(c.kind, c.a, c.b, c.tag): c for c in AL.cases(AL.load(AL.IMA))}
    oki = {(c.kind, c.a, c.b, c.tag): c for c in AL.cases(AL.load(AL.OKI))}
    want = {"SUM_VDVI_CODES": fnv(ima[(AL.ENCODE, AL.VDVI, 0, "line")].want.astype(np.uint8)),
            "SUM_VDVI_SAMPLES": fnv(ima[(AL.DECODE, AL.VDVI, 0, "line")].want.astype("<i2")),
            "SUM_OKI_CODES": fnv(oki[(AL.ENCODE, 24000, 0, "line")].want.astype(np.uint8)),
            "SUM_OKI_SAMPLES": fnv(oki[(AL.DECODE, 24000, 0, "line")].want.astype("<i2"))}
    text = open(os.path.join(SRC, "adpcm_caller.c")).read()
    for name, value in want.items():
        m = re.search(r"#define %s\s+0x([0-9a-fA-F]{8})u" % name, text)
        assert m and int(m.group(1), 16) == value, (name, "%08x" % value)
    assert tuple(int(x) for x in re.search(r"schedule\[10\] = \{([^}]*)\}", text).group(1).split(",")) == AL.SCHEDULE
    line = AL.line()
    data = os.path.join(str(tmp_path), "adpcm_line.txt")
    with open(data, "w") as f:
        f.write("%d\n%s\n" % (len(line), " ".join(map(str, line.astype(np.int64).tolist()))))
    exe = build("adpcm_caller", str(tmp_path))
    out = run([exe, data])
    assert out.splitlines()[-1] == "ok" and "DIFFERS" not in out, out
