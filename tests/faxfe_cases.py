"""tests/golden/faxfe.npz for the FAX front-end tests: the cases as dictionaries, per-tick slices of their back-to-back
lists, and the flat text form tests/c_callers/faxfe_host.cpp reads."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "faxfe.npz")
FIELDS = ("cfg", "lens", "ops", "path", "amp", "handler", "frx", "recs", "nrecs", "bytes", "nbytes", "put", "nput", "fast", "nfast",
          "v21", "nv21", "dc", "framer", "buffer")
SLOW, FAST = 1, 2
NONE, FAST_AND_V21, FAST_ONLY, V21_ONLY = 0, 1, 2, 3
TRAINING_SUCCEEDED = -4

_cases = []


def load():
    """[(name, {field: array, "at_<list>": start of every tick in that list})]; (.., case 11 present)"""
    if not _cases:
        g = np.load(GOLDEN)
        for k, name in enumerate(g["names"]):
            c = {f: g["c%d_%s" % (k, f)] for f in FIELDS}
            for lst, per in (("amp", "lens"), ("recs", "nrecs"), ("bytes", "nbytes"), ("put", "nput"), ("fast", "nfast"), ("v21", "nv21")):
                c["at_" + lst] = np.concatenate([[0], np.cumsum(c[per])]).astype(np.int64)
            _cases.append((str(name), c))
        _cases.append(int(g["case11"]))
    return _cases[:-1], _cases[-1]


def tick(c, lst, t):
    at = c["at_" + lst]
    return c[lst][at[t]:at[t + 1]]


def dump_text(path, cases):
    with open(path, "w") as f:
        put = lambda a: f.write(" ".join(str(int(x)) for x in a) + "\n")
        for _, c in cases:
            ticks = int(c["cfg"][1])
            f.write("C %d %d %d\n" % (c["cfg"][0], ticks, len(c["ops"])))
            for op in c["ops"]:
                put(op)
            for t in range(ticks):
                put([c["lens"][t]])
                put(tick(c, "amp", t))
                for lst in ("fast", "v21"):
                    row = tick(c, lst, t)
                    put([len(row)])
                    put(row)
                put([c["handler"][t], c["frx"][t]])
                for lst in ("recs", "bytes", "put"):
                    row = tick(c, lst, t)
                    put([len(row)])
                    put(row)
            put(c["dc"])
            put(c["framer"])
            put(c["buffer"])
        f.write("E\n")
    return len(cases)
