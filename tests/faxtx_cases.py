"""tests/golden/faxtx.npz for the FAX transmit front-end tests: the cases as dictionaries, per-tick slices of their back-to-back
lists, and the flat text form tests/c_callers/faxtx_host.cpp reads."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "faxtx.npz")
FIELDS = ("cfg", "ops", "path", "frames", "flens", "bits", "rows", "lens", "calls", "ncalls", "steps", "under", "handler", "transmit",
          "asked", "nasked", "end", "hdlc", "buffer")
RX_FIELDS = ("rx_ops", "rx_handler", "rx_frx", "rx_recs", "rx_nrecs", "rx_bytes", "rx_nbytes")
SET, RESTART, TEP, Q_FRAME, Q_FLAGS, Q_END, BITS, EOD = range(1, 9)
NONE, PAUSE, CED, CNG, V21, V27TER, V29, V17, V34HDX, DONE = range(10)
H_SILENCE, H_TONE, H_V21, H_FAST = range(4)

_cases = []
_flags = {}


def load():
    """([(name, {field: array, "at_<list>": start of every tick in that list, "frame_list": [bytes]})], {flag name: value})"""
    if not _cases:
        g = np.load(GOLDEN)
        for k, name in enumerate(g["names"]):
            c = {f: g["c%d_%s" % (k, f)] for f in FIELDS}
            for f in RX_FIELDS:
                if "c%d_%s" % (k, f) in g.files:
                    c[f] = g["c%d_%s" % (k, f)]
            lists = [("calls", "ncalls"), ("asked", "nasked")] + ([("rx_recs", "rx_nrecs"), ("rx_bytes", "rx_nbytes")] if "rx_recs" in c else [])
            for lst, per in lists:
                c["at_" + lst] = np.concatenate([[0], np.cumsum(c[per])]).astype(np.int64)
            at = np.concatenate([[0], np.cumsum(c["flens"])]).astype(np.int64)
            c["frame_list"] = [bytes(c["frames"][at[i]:at[i + 1]]) for i in range(len(c["flens"]))]
            _cases.append((str(name), c))
        _flags.update({str(n): int(v) for n, v in zip(g["flag_names"], g["flags"])})
    return _cases, _flags


def tick(c, lst, t):
    at = c["at_" + lst]
    return c[lst][at[t]:at[t + 1]]


def ops_of(c, t):
    return [[int(x) for x in op] for op in c["ops"] if op[0] == t]


def dump_text(path, cases):
    with open(path, "w") as f:
        put = lambda a: f.write(" ".join(str(int(x)) for x in a) + "\n")
        for _, c in cases:
            ticks = int(c["cfg"][1])
            f.write("C %d %d %d %d %d\n" % (c["cfg"][0], ticks, c["cfg"][2], len(c["frame_list"]), len(c["ops"])))
            for fr in c["frame_list"]:
                put([len(fr)] + list(fr))
            for op, path_ in zip(c["ops"], c["path"]):
                put(list(op) + [path_])
            for t in range(ticks):
                put([c["lens"][t], c["steps"][t], c["under"][t], c["handler"][t], c["transmit"][t]])
                calls = tick(c, "calls", t)
                put([len(calls)] + [x for call in calls for x in call])
                asked = tick(c, "asked", t)
                put([len(asked)] + list(asked))
            put(c["end"])
            put(c["hdlc"])
            put(c["buffer"])
        f.write("E\n")
    return len(cases)
