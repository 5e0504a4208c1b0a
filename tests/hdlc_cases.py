"""What the HDLC tests share: the cases of tests/golden/hdlc.npz (written by tests/golden/make_golden_hdlc.py from the
reference) unpacked into plain Python, and the text form tests/c_callers/hdlc_host.cpp reads."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hdlc.npz")
FRAME, FLAGS, ABORT, END = 1, 2, 3, 4
TX_REF_WORDS = 16       # the words of hdlc_tx_state_t; the queue's two follow
RX_WORDS = 18
END_OF_DATA = -7


class TxCase:
    def __init__(self, g, k):
        key = "tx_%d_" % k
        self.crc32, self.iff, self.depth, self.calls = (int(x) for x in g[key + "cfg"])
        self.schedule = [int(x) for x in g["schedule"]]
        opbytes = g[key + "opbytes"].tobytes()
        self.ops, at = [], 0
        for (call, kind, arg, corrupt), res in zip(g[key + "ops"], g[key + "results"]):
            data = b""
            if kind == FRAME:
                data = opbytes[at:at + arg]
                at += arg
            self.ops.append((int(call), int(kind), int(arg), int(corrupt), int(res), data))
        self.lens = [int(x) for x in g[key + "lens"]]
        self.under = [int(x) for x in g[key + "under"]]
        self.ended = [int(x) for x in g[key + "ended"]]
        self.words = g[key + "words"]
        ends = np.cumsum([0] + self.lens)
        bits = g[key + "bits"]
        self.bits = [bits[ends[i]:ends[i + 1]] for i in range(self.calls)]

    def want(self, call):
        return self.schedule[call % len(self.schedule)]


class RxCase:
    def __init__(self, g, k, octets=False):
        key = "rx_%d_" % k
        self.name = str(g["rx_names"][k])
        self.octets = octets
        self.crc32, self.bad, self.thr, self.max_len, self.interval = (int(x) for x in g[key + "cfg"])
        self.midops = [(int(a), int(b)) for a, b in g[key + "midops"]]
        events = g[key + "events"]
        per = "rxb_%d_" % k if octets else key
        if octets:
            entries = np.packbits(events.astype(np.uint8))
            lens = [int(x) for x in g[per + "lens"]]
        else:
            entries = events
            schedule = [int(x) for x in g["schedule"]]
            lens, at = [], 0
            while at < len(events):
                lens.append(min(schedule[len(lens) % len(schedule)], len(events) - at))
                at += lens[-1]
        ends = np.cumsum([0] + lens)
        self.calls = len(lens)
        self.entries = [entries[ends[i]:ends[i + 1]] for i in range(self.calls)]
        nrecs = np.cumsum([0] + [int(x) for x in g[per + "nrecs"]])
        assert len(nrecs) == self.calls + 1
        recs = g[key + "recs"]
        self.recs = [[int(r) for r in recs[nrecs[i]:nrecs[i + 1]]] for i in range(self.calls)]
        self.all_bytes = g[key + "bytes"].tobytes()
        self.words = g[per + "words"]
        self.buffer = g[per + "buffer"]
        # the records of each call in the form HdlcRxBank.records() gives them
        self.records, at = [], 0
        for rs in self.recs:
            out = []
            for r in rs:
                if r < 0:
                    out.append(r)
                else:
                    n = r & 0xFFFF
                    out.append((n, bool(r & 0x10000), self.all_bytes[at:at + n]))
                    at += n
            self.records.append(out)
        assert at == len(self.all_bytes)


class DeviceBytes:
    """n bytes in HBM, for the calls that take device pointers."""

    def __init__(self, n):
        import ctypes as C
        self.C = C
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.n = n
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), n) == 0

    def upload(self, host):
        host = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        assert len(host) <= self.n and self.hip.hipMemcpy(self.ptr, host.ctypes.data, len(host), 1) == 0

    def download(self, dtype=np.uint8):
        host = np.zeros(self.n, np.uint8)
        assert self.hip.hipMemcpy(host.ctypes.data, self.ptr, self.n, 2) == 0
        return host.view(dtype)

    def free(self):
        self.hip.hipFree(self.ptr)


def load():
    g = np.load(GOLDEN)
    tx = [TxCase(g, k) for k in range(int(g["tx_cases"]))]
    rx = [RxCase(g, k) for k in range(len(g["rx_names"]))]
    rxb = [RxCase(g, k, octets=True) for k in range(len(g["rx_names"])) if "rxb_%d_lens" % k in g.files]
    return g, tx, rx, rxb


def dump_text(path, tx, rx, rxb):
    """the cases as hdlc_host.cpp reads them"""
    out = []
    for c in tx:
        out.append("T %d %d %d %d %d" % (c.crc32, c.iff, c.depth, c.calls, len(c.ops)))
        for call, kind, arg, corrupt, res, data in c.ops:
            out.append(" ".join(str(x) for x in [call, kind, arg, corrupt, res] + list(data)))
        for k in range(c.calls):
            out.append(" ".join(str(int(x)) for x in [c.want(k), c.lens[k], c.under[k], c.ended[k]] + list(c.words[k]) + list(c.bits[k])))
    for c in rx + rxb:
        out.append("R %d %d %d %d %d %d %d %d" % (int(c.octets), c.crc32, c.bad, c.thr, c.max_len, c.interval, c.calls, len(c.midops)))
        for a, b in c.midops:
            out.append("%d %d" % (a, b))
        for k in range(c.calls):
            out.append(" ".join(str(int(x)) for x in [len(c.entries[k])] + list(c.entries[k]) + [len(c.recs[k])] + c.recs[k] + list(c.words[k])))
        out.append(" ".join(str(int(x)) for x in [len(c.all_bytes)] + list(c.all_bytes) + list(c.buffer)))
    out.append("E")
    open(path, "w").write("\n".join(out) + "\n")
    return len(tx), len(rx) + len(rxb)
