"""The generated lines, configurations and call schedules of the HDLC sweep (tests/test_hdlc_sweep.py on the CPU,
tests/test_hdlc_sweep_gpu.py on the GPU): thousands of receiver and sender lines for the HDLC framing banks, each compared
with the live reference (oracle/ref_hdlc.py).  32-bit linear congruential generators (codec_sweep.Lcg) and fixed seeds, integer
arithmetic only: what is generated here is the same everywhere, so none of it is committed.

  rx_lines(n, seed, form)       per line its events: int16, int8 or (form "octets") bits for whole octets; line i is of family
                                FAMILIES[i % DEAL], so every 64 consecutive lines hold all
  rx_configs(n, seed)           per line: crc32, report_bad_frames, threshold, max_frame_len argument (-1: none), interval
  rx_schedule(...)              per call, per line: lengths, never in step across a wave
  tx_lines(n, seed)             per line: configuration, the script of offers, the wants
  sweep_rx() / sweep_tx()       the above with what the reference makes of it
  coverage_rx() / coverage_tx() what the reference reached on these inputs, from its records and state words alone
  PINNED                        lines a sweep once failed on: (kind, seed, line), kept in the sweep by name
"""
import zlib

import numpy as np

from codec_sweep import Lcg, WAVE, cut, probes, seeds_of

SEED = 0x4D1C
N_GPU = 16*WAVE + 37                # 16 full waves and a partial one
FAMILIES = ("wire", "sent", "damaged", "noise", "ones_heavy", "abort_runs", "short_frames", "overlong", "statuses", "any_int16", "capacity")
DEAL = len(FAMILIES)                # 11: coprime to the 288 receiver configurations
EVENTS = 6144                       # a receiver line holds at least this many
RX_CALLS, TX_CALLS = 24, 40
PINNED = ()                         # (kind, seed, line): nothing has failed yet

OP_MAX_FRAME_LEN, OP_REPORT_INTERVAL, OP_RESTART = 1, 2, 3
FRAME, FLAGS, ABORT, END = 1, 2, 3, 4
FRAME_OK = 0x10000
# the banks' state words (csrc/hdlc_dev.hpp)
(HR_CRC_BYTES, HR_MAX_FRAME_LEN, HR_REPORT_BAD, HR_THRESHOLD, HR_ANNOUNCED, HR_FLAGS_SEEN, HR_RAW, HR_BYTE, HR_NUM_BITS, HR_COUNTING,
 HR_OCTET_COUNT, HR_INTERVAL, HR_LEN, HR_RX_BYTES, HR_RX_FRAMES, HR_CRC_ERRORS, HR_LENGTH_ERRORS, HR_ABORTS) = range(18)
(HT_CRC_BYTES, HT_IFF, HT_PROGRESSIVE, HT_MAX_FRAME_LEN, HT_OIP, HT_NUM_BITS, HT_IDLE_OCTET, HT_FLAG_OCTETS, HT_ABORT_OCTETS, HT_REPORT,
 HT_LEN, HT_POS, HT_CRC, HT_BYTE, HT_BITS, HT_TX_END) = range(16)
RX_WORDS, TX_WORDS = 18, 16

FLAG = np.array([0, 1, 1, 1, 1, 1, 1, 0], np.uint8)
SHARED = np.array([1, 1, 1, 1, 1, 1, 0], np.uint8)         # a flag on the zero of the one before
ABORT_OCTET = np.array([0, 1, 1, 1, 1, 1, 1, 1], np.uint8)  # 0x7F as hdlc_tx_get_bit() sends it
# octets that exercise the stuffing (tests/golden/make_golden_hdlc.py pattern())
SPECIAL = np.array([0xFF, 0x7E, 0x1F, 0xF8, 0xFF, 0xFF, 0x7E, 0x7E, 0x1F, 0x1F, 0xF8, 0xF8, 0x3E, 0x7C, 0xFB, 0xDF], np.uint8)

_CRC16 = []


def crc_of(data, crc32):
    """the CRC octets as they follow the frame (ITU CRC-32 is zlib's; ITU CRC-16 by table)"""
    if crc32:
        return np.frombuffer(int(zlib.crc32(bytes(data))).to_bytes(4, "little"), np.uint8)
    if not _CRC16:
        for b in range(256):
            c = b
            for _ in range(8):
                c = (c >> 1) ^ (0x8408 if c & 1 else 0)
            _CRC16.append(c)
    crc = 0xFFFF
    for b in bytes(data):
        crc = (crc >> 8) ^ _CRC16[(crc ^ b) & 0xFF]
    crc ^= 0xFFFF
    return np.array([crc & 0xFF, crc >> 8], np.uint8)


def stuffed(bits, mask):
    """bits with a zero behind every fifth one of a run of ones, where mask says the bits are a frame's (flags and aborts go
    as they are, and end a run)"""
    d = bits & mask
    idx = np.arange(len(d))
    last_zero = np.maximum.accumulate(np.where(d == 0, idx, -1))
    run = idx - last_zero
    return np.insert(bits, np.flatnonzero((d == 1) & (run % 5 == 0)) + 1, 0)


class Draws:
    """a line's scalar draws, in order"""

    def __init__(self, row):
        self.r, self.i = row, 0

    def __call__(self, m):
        v = self.r[self.i % len(self.r)]
        self.i += 1
        return v % m


def family_of(i):
    return np.asarray(i) % DEAL


# ---- receiver lines ------------------------------------------------------------------------------------------------------

def rx_configs(n, seed=SEED):
    """[n][5]: crc32, report_bad_frames, framing_ok_threshold, the set_max_frame_len argument behind the init (-1: none), the
    report interval.  The first three and the interval cycle with period 288; a third of the lines set a length.  The
    families that need a setting have it: overlong lines a small or no length in turn, capacity lines as their streams ask."""
    p = Lcg(seeds_of(n, seed, 11)).u16(2)
    cfg = np.zeros((n, 5), np.int32)
    for i in range(n):
        k = i % 288
        ml = -1
        if (k >> 4)//6 == 0:
            ml = int(3 + p[i, 0] % 18 if p[i, 1] % 2 else 21 + p[i, 0] % 430)
        cfg[i] = (k & 1, (k >> 1) & 1, 1 + (k >> 4) % 6, ml, (0, 1, 2, 20)[(k >> 2) & 3])
        fam = FAMILIES[i % DEAL]
        if fam == "overlong":
            cfg[i, 3] = int(3 + p[i, 0] % 18) if (i//DEAL) % 2 else -1
        elif fam == "capacity":
            which = (i//DEAL) % 3
            cfg[i] = ((i//(3*DEAL)) & 1 if which != 1 else 0, 1, 1, -1, 1)
    return cfg


class _Wire:
    """frames on the wire: segments of bits with a mask that says which are a frame's, stuffed in one pass at the end"""

    def __init__(self, d, pool, crc32):
        self.d, self.pool, self.crc32, self.at = d, pool, crc32, 0
        self.crc_bytes = 4 if crc32 else 2
        self.bits, self.mask, self.n = [], [], 0

    def raw(self, bits, data=0):
        self.bits.append(bits)
        self.mask.append(np.full(len(bits), data, np.uint8))
        self.n += len(bits)

    def flags(self, count, shared=False):
        self.raw(FLAG)
        for _ in range(count - 1):
            self.raw(SHARED if shared else FLAG)

    def body(self, n):
        if self.at + n > len(self.pool):
            self.at = 0
        self.at += n
        return self.pool[self.at - n:self.at]

    def frame(self, wire_len, good=True, cut_at=None):
        """wire_len octets between two flags: a body and its CRC, or below the CRC's size any octets"""
        if wire_len >= self.crc_bytes:
            b = self.body(wire_len - self.crc_bytes)
            crc = crc_of(b, self.crc32)
            octets = np.concatenate([b, crc if good else crc ^ 0x55])
        else:
            octets = self.body(wire_len)
        bits = np.unpackbits(octets, bitorder="little")
        self.raw(bits if cut_at is None else bits[:cut_at], 1)

    def done(self):
        bits, mask = np.concatenate(self.bits), np.concatenate(self.mask)
        return stuffed(bits, mask), bits, mask

    def length(self, d):
        cb = self.crc_bytes
        kind = d(8)
        if kind == 0:
            return (cb - 1, cb, cb + 1, 399, 400, 401, 402, 403, 404)[d(9)]
        if kind <= 4:
            return 1 + d(24)
        if kind <= 6:
            return 1 + d(120)
        return 1 + d(404)


def _wire_line(d, pool, cfg, need, aborts=False, overlong=False):
    crc32, _, thr, ml, _ = cfg
    w = _Wire(d, pool, crc32)
    w.flags(thr + 1 if d(4) else 1 + d(6))
    while w.n < need:
        if overlong:
            n = (405 + d(296) if d(3) == 0 else 1 + d(30)) if ml < 0 else (ml + w.crc_bytes + 1 + d(30) if d(2) else 1 + d(ml + w.crc_bytes))
        else:
            n = w.length(d)
        if aborts and d(3) == 0:
            # seven to twenty ones inside a frame
            w.frame(n, cut_at=1 + d(8*n))
            w.raw(np.ones(7 + d(14), np.uint8))
            w.raw(FLAG[:1])
        else:
            w.frame(n, good=d(16) != 0)
        w.flags(1 + d(6), shared=d(8) == 0)
        if aborts:
            k = d(4)
            if k == 0:
                w.raw(np.tile(ABORT_OCTET, 1 + d(30)))
                w.flags(1 + d(3))
            elif k == 1:
                w.raw(np.ones(7 + d(14), np.uint8))
                w.flags(1 + d(3))
    return w.done()[0]


def _capacity_line(d, pool, cfg, which):
    """(events, call lengths or None).  which 0: a run of 0x7F at report interval 1, a flag now and then; 1: frames of 404 and
    403 octets on the wire, the longest a receiver delivers, with calls of 1, 2, 7, 8 and 9 events whose first bit is the
    last of the closing flag (the 403 octets the capacity allows for would take len = 405 at a flag with the framing OK, a
    state the reference's own code never leaves: an over-long frame takes flags_seen below the threshold); 2: a bad frame
    of one octet every 16 bits."""
    crc32 = cfg[0]
    w = _Wire(d, pool, crc32)
    w.flags(2)
    if which == 0:
        w.frame(w.crc_bytes + 1 + d(5))
        w.flags(1)
        while w.n < EVENTS + 64:
            w.raw(np.tile(ABORT_OCTET, 5 + d(60)))
            if d(3) == 0:
                w.flags(1 + d(2))
        return w.done()[0], None
    if which == 2:
        while w.n < EVENTS + 64:
            o = SPECIAL[2 + d(2)] if d(4) == 0 else np.uint8(d(256) & 0x5F)           # no five ones: nothing is stuffed
            w.raw(np.unpackbits(np.array([o], np.uint8), bitorder="little"), 1)
            w.flags(1)
        return w.done()[0], None
    ends = []
    for n in (404, 403, 404):
        w.frame(n, good=d(4) != 0)
        w.flags(1)
        ends.append(w.n - 1)
        w.flags(d(2))
    w.frame(1 + d(20))
    w.flags(2)
    ev, bits, mask = w.done()
    # where the closing flags' last bits lie behind the stuffing
    added = np.cumsum((mask == 1) & (_run_of(bits & mask) % 5 == 0) & ((bits & mask) == 1))
    lens, at = [], 0
    for e in ends:
        e = int(e + added[e])
        span = e - at
        cuts = sorted({1 + d(span - 1) for _ in range(3)})
        lens += list(np.diff([0] + cuts + [span]))
        small = (1, 2, 7, 8, 9)[d(5)]
        lens.append(small)
        at = e + small
    lens.append(len(ev) - at)
    return ev, [int(x) for x in lens]


def _run_of(d):
    idx = np.arange(len(d))
    return idx - np.maximum.accumulate(np.where(d == 0, idx, -1))


def rx_lines(n, seed=SEED, form="int16", sent=None):
    """(events per line, schedules of their own {line: lens}).  form "int8": any_int16 lines hold any int8 values; "octets":
    bits only (statuses lines carry no codes, any_int16 lines bit 0 of their values).  sent(i): the bits the reference sender
    made of sender line i."""
    g = Lcg(seeds_of(n, seed, 12))
    u = g.u16(EVENTS + 64)
    rows = Lcg(seeds_of(n, seed, 13)).u16(2048)
    cfgs = rx_configs(n, seed)
    out, own = [], {}
    for i in range(n):
        fam = FAMILIES[i % DEAL]
        ui = u[i]
        d = Draws(rows[i].tolist())
        pool = np.where((ui >> 12) % 3 == 0, ui & 0xFF, SPECIAL[(ui >> 8) & 15]).astype(np.uint8)
        cfg = cfgs[i].tolist()
        if fam == "wire":
            ev = _wire_line(d, pool, cfg, EVENTS)
        elif fam == "sent":
            ev = sent(i)
            ev = np.tile(ev, -(-EVENTS//max(1, len(ev))))
        elif fam == "damaged":
            ev = _wire_line(d, pool, cfg, EVENTS + 64)
            for _ in range(1 + d(40)):
                at, how = d(EVENTS), d(3)
                if how == 0:
                    ev[at] ^= 1
                elif how == 1:
                    ev = np.delete(ev, at)
                else:
                    ev = np.insert(ev, at, d(2))
        elif fam == "noise":
            ev = (ui >> 7) & 1
        elif fam == "ones_heavy":
            ev = (ui % 6 != 0)
        elif fam == "abort_runs":
            ev = _wire_line(d, pool, cfg, EVENTS, aborts=True)
        elif fam == "short_frames":
            # a flag every 8 to 24 bits, any bits between
            period = 8 + (u[i, :EVENTS//8 + 8] >> 3) % 17
            start = np.concatenate([[0], np.cumsum(period)])
            seg = np.searchsorted(start, np.arange(EVENTS + 64), side="right") - 1
            pos = np.arange(EVENTS + 64) - start[seg]
            ev = np.where(pos < 8, FLAG[np.minimum(pos, 7)], (ui >> 9) & 1)
        elif fam == "overlong":
            ev = _wire_line(d, pool, cfg, EVENTS, overlong=True)
        elif fam == "statuses":
            ev = _wire_line(d, pool, cfg, EVENTS).astype(np.int16)
            if form != "octets":
                for _ in range(1 + d(30)):
                    ev = np.insert(ev, d(EVENTS), -1 - d(40))
        elif fam == "any_int16":
            ev = {"int16": ui - 32768, "int8": (ui & 0xFF) - 128, "octets": ui & 1}[form]
        else:
            ev, lens = _capacity_line(d, pool, cfg, (i//DEAL) % 3)
            if lens is not None:
                own[i] = lens
        ev = np.asarray(ev).astype(np.int16)
        assert len(ev) >= EVENTS, (fam, i, len(ev))
        out.append(ev if i in own else ev[:EVENTS])
    return out, own


def rx_schedule(n, calls, seed, avail, own=None, octets=False):
    """[calls][n] lengths: an eighth of the calls a line sits out (0), a quarter are 1 .. 16 events, the rest 1 .. 1 024; in
    octets 0, 1 .. 5 and up to 128.  Capacity lines without a schedule of their own take 1, 2, 7, 8 or 9 events in half of
    their calls.  Held to what a line has (codec_sweep.cut)."""
    r = Lcg(seeds_of(n, seed, 14)).u16(2*calls)
    kind, size = r[:, :calls] % 8, r[:, calls:]
    if octets:
        lens = np.where(kind == 0, 0, np.where(kind <= 2, 1 + size % 5, 1 + size % 128))
    else:
        lens = np.where(kind == 0, 0, np.where(kind <= 2, 1 + size % 16, 1 + size % 1024))
        cap = (np.arange(n) % DEAL == DEAL - 1)[:, None] & (kind >= 4)
        lens = np.where(cap, np.array([1, 2, 7, 8, 9])[size % 5], lens)
    lens = cut(avail, np.ascontiguousarray(lens.T.astype(np.int32)))
    for i, own_lens in (own or {}).items():
        assert len(own_lens) <= calls and sum(own_lens) <= avail[i]
        lens[:, i] = 0
        lens[:len(own_lens), i] = own_lens
    return lens


def rx_ops(cfgs, lens, seed):
    """per line [(call, operation, value)]: the settings behind the init (call -1), and on a sixth of the lines one or two
    operations ahead of calls with a length: max_frame_len taken down or up, a restart, another report interval"""
    calls, n = lens.shape
    r = Lcg(seeds_of(n, seed, 15)).u16(8)
    out = []
    for i in range(n):
        ops = []
        if cfgs[i, 3] >= 0:
            ops.append((-1, OP_MAX_FRAME_LEN, int(cfgs[i, 3])))
        if cfgs[i, 4]:
            ops.append((-1, OP_REPORT_INTERVAL, int(cfgs[i, 4])))
        live = np.flatnonzero(lens[:, i] > 0)
        if r[i, 0] % 6 == 0 and len(live) and i % DEAL != DEAL - 1:
            mid = []
            for j in range(1 + r[i, 1] % 2):
                k = int(live[r[i, 2 + 3*j] % len(live)])
                what = r[i, 3 + 3*j] % 4
                v = int(r[i, 4 + 3*j])
                mid.append({0: (k, OP_MAX_FRAME_LEN, v % 24), 1: (k, OP_MAX_FRAME_LEN, 20 + v % 420), 2: (k, OP_RESTART, 0),
                            3: (k, OP_REPORT_INTERVAL, (0, 1, 2, 20)[v % 4])}[int(what)])
            ops += sorted(mid, key=lambda o: o[0])
        out.append(ops)
    return out


# ---- sender lines --------------------------------------------------------------------------------------------------------

def tx_lines(n, seed=SEED, calls=TX_CALLS):
    """(cfgs [n][4]: crc32, inter_frame_flags, queue depth, max_frame_len or -1; ops per line [m][4]: call, command, argument,
    corrupt; opbytes per line; wants [calls][n])"""
    r = Lcg(seeds_of(n, seed, 21)).u16(2*calls)
    kind, size = r[:, :calls] % 8, r[:, calls:]
    wants = np.where(kind == 0, 0, np.where(kind <= 2, 1 + size % 16, 1 + size % 600))
    rows = Lcg(seeds_of(n, seed, 22)).u16(4096)
    cfgs = np.zeros((n, 4), np.int32)
    all_ops, all_bytes = [], []
    for i in range(n):
        d = Draws(rows[i].tolist())
        depth = 1 + (i//2) % 8
        cfgs[i] = (i % 2, 1 + i % 5, depth, 2 + d(399) if i % 7 == 0 else -1)
        ops, octets = [], []
        for k in range(calls):
            c = d(16)
            count = 0 if c < 9 else 1 if c < 13 else 2 if c < 15 else depth + 1 + d(4)
            for _ in range(count):
                what = d(16)
                if what < 9:
                    f = d(32)
                    n_oct = 1 + d(12) if f < 19 else 1 + d(60) if f < 28 else (1, 2, 3, 399, 400, 401, 402, 450)[d(8)] if f < 31 else 1 + d(400)
                    ops.append((k, FRAME, n_oct, int(d(8) == 0)))
                    at = d(4096 - n_oct)
                    o = np.asarray(rows[i, at:at + n_oct])
                    octets.append(np.where((o >> 12) % 3 == 0, o & 0xFF, SPECIAL[(o >> 8) & 15]).astype(np.uint8))
                elif what < 12:
                    ops.append((k, FLAGS, 0 if d(8) == 0 else d(46) - 5, 0))
                elif what < 14:
                    ops.append((k, ABORT, 0, 0))
                elif what < 15:
                    ops.append((k, END, 0, 0))
                else:
                    ops.append((k, FRAME, 0, 0))            # a frame of no octets: the end of the data
        all_ops.append(np.array(ops, np.int32).reshape(-1, 4))
        all_bytes.append(np.concatenate(octets) if octets else np.zeros(0, np.uint8))
    return cfgs, all_ops, all_bytes, np.ascontiguousarray(wants.T.astype(np.int32))


# ---- the sweeps: what goes in, and what the reference makes of it ----------------------------------------------------------

def _ref():
    from oracle import ref_hdlc
    return ref_hdlc


def wanted(lens, every_all=False):
    """[calls][n]: the calls after which a line's words are compared: every call of a probe line, the calls a line sits out,
    the last"""
    calls, n = lens.shape
    want = lens == 0
    want[-1] = True
    want[:, np.arange(n) if every_all else probes(n)] = True
    return want


def sweep_tx(n=N_GPU, seed=SEED, every_all=False, calls=TX_CALLS, ref=True):
    """"cfgs", "ops", "opbytes", "wants"; from the reference "bits" per line (one a byte, all calls), "lens", "under", "ended",
    "taken" [calls][n], "results" per line, "final" [n][16], "words" per line {call: words}"""
    cfgs, ops, opbytes, wants = tx_lines(n, seed, calls)
    r = {"cfgs": cfgs, "ops": ops, "opbytes": opbytes, "wants": wants, "family": "hdlc_tx", "seed": seed, "want": wanted(wants, every_all)}
    if ref:
        R = _ref()
        for key in ("bits", "results", "words", "final", "lens", "under", "ended", "taken"):
            r[key] = []
        for i in range(n):
            bits, lens, under, ended, taken, results, w = R.run_tx(*cfgs[i].tolist(), ops[i], opbytes[i], wants[:, i], want=r["want"][:, i])
            r["bits"].append(bits)
            r["results"].append(results)
            r["words"].append(dict(zip(np.flatnonzero(r["want"][:, i]).tolist(), w)))
            r["final"].append(w[-1])
            for key, v in (("lens", lens), ("under", under), ("ended", ended), ("taken", taken)):
                r[key].append(v)
        for key in ("lens", "under", "ended", "taken"):
            r[key] = np.ascontiguousarray(np.array(r[key], np.int32).T)
        r["final"] = np.array(r["final"], np.int32)
    return r


def _sent(n, seed):
    """the bits the reference sender makes of sender line i of this sweep"""
    cfgs, ops, opbytes, wants = tx_lines(n, seed, TX_CALLS)
    R = _ref()
    return lambda i: R.run_tx(*cfgs[i].tolist(), ops[i], opbytes[i], wants[:, i])[0]


def sweep_rx(n=N_GPU, seed=SEED, form="int16", every_all=False, calls=RX_CALLS, ref=True):
    """"cfgs", "fam", "ops" per line, "data" per line (int16 events, int8 events or octets), "lens" [calls][n], "full" [n]: the line takes whole
    rows (int8 form); from the reference "recs" and "bytes" per line (all calls back to back), "nrecs" and "nbytes" [calls][n], "final" [n][18], "words"
    per line {call: words}, "buffer" [n][404]"""
    cfgs = rx_configs(n, seed)
    data, own = rx_lines(n, seed, form, _sent(n, seed))
    octets = form == "octets"
    if octets:
        data = [np.packbits(d[:len(d) & ~7].astype(np.uint8)) for d in data]
        own = {}
    lens = rx_schedule(n, calls, seed, [len(d) for d in data], own, octets)
    full = np.zeros(n, bool)
    if form == "int8":
        # every fourth line takes whole rows (its count is given above the row, and the clamp makes it the row): the rows are
        # as wide as the other lines' longest call, rounded up to 16, and the line's events go round
        full = (np.arange(n) % 4 == 3) & np.array([i not in own for i in range(n)])
        lens[:, full] = ((lens[:, ~full].max(axis=1) + 15) & ~15)[:, None]
        data = [np.resize(d, int(lens[:, i].sum())) if full[i] else d for i, d in enumerate(data)]
    data = [d[:int(lens[:, i].sum())].astype({"int16": np.int16, "int8": np.int8, "octets": np.uint8}[form]) for i, d in enumerate(data)]
    ops = rx_ops(cfgs, lens, seed)
    r = {"cfgs": cfgs, "fam": family_of(np.arange(n)), "ops": ops, "data": data, "lens": lens, "family": "hdlc_rx", "form": form, "seed": seed,
         "want": wanted(lens, every_all), "full": full}
    if ref:
        R = _ref()
        for key in ("recs", "bytes", "nrecs", "nbytes", "final", "words", "buffer"):
            r[key] = []
        for i in range(n):
            recs, by, nrecs, nbytes, w, buf = R.run_rx(*cfgs[i, :3].tolist(), data[i], lens[:, i], ops[i], octets, want=r["want"][:, i])
            r["recs"].append(recs)
            r["bytes"].append(by)
            r["nrecs"].append(nrecs)
            r["nbytes"].append(nbytes)
            r["words"].append(dict(zip(np.flatnonzero(r["want"][:, i]).tolist(), w)))
            r["final"].append(w[-1])
            r["buffer"].append(buf)
        for key in ("nrecs", "nbytes"):
            r[key] = np.ascontiguousarray(np.array(r[key], np.int32).T)
        r["final"], r["buffer"] = np.array(r["final"], np.int32), np.array(r["buffer"], np.uint8)
    return r


def all_words(r):
    """[n][calls][W] of a sweep made with every_all"""
    return np.array([[w[k] for k in range(r["want"].shape[0])] for w in r["words"]], np.int32)


def records_of(r, i):
    """line i's calls: [[(len, ok, bytes) | code < 0]], as HdlcRxBank.records() has a channel's"""
    out, ra, ba = [], 0, 0
    by = r["bytes"][i].tobytes()
    for k in range(r["lens"].shape[0]):
        row = []
        for v in r["recs"][i][ra:ra + int(r["nrecs"][k, i])].tolist():
            if v < 0:
                row.append(v)
            else:
                row.append((v & 0xFFFF, bool(v & FRAME_OK), by[ba:ba + (v & 0xFFFF)]))
                ba += v & 0xFFFF
        ra += int(r["nrecs"][k, i])
        out.append(row)
    return out


def within_capacity(r):
    """every call of every line: the reference's records and octets within hdlc_rx_capacity() of the call's events"""
    R = _ref()
    rec_cap, byte_cap = R.rx_capacity(r["lens"].astype(np.int64)*(8 if r["form"] == "octets" else 1))
    live = r["lens"] > 0
    return bool(((r["nrecs"] <= rec_cap) & (r["nbytes"] <= byte_cap))[live].all()), float((r["nrecs"][live]/rec_cap[live]).max()), \
        float((r["nbytes"][live]/byte_cap[live]).max())


# ---- what the reference reached ------------------------------------------------------------------------------------------

def coverage_rx(r):
    """from the records and the words after every call (a sweep made with every_all) alone"""
    W = all_words(r)
    calls, n = r["lens"].shape
    c = {"statuses": set(), "good": {2: set(), 4: set()}, "bad_crc": 0, "bad_short": 0, "bad_long": 0, "bad_misaligned": 0, "len_0": 0,
         "len_405": int((W[:, :, HR_LEN] == 405).sum()), "counting_by_abort": 0, "counting_by_overlong": 0, "crc_error_lines": 0,
         "length_error_lines": 0, "frames": 0}
    zero = np.zeros(RX_WORDS, np.int32)
    for i in range(n):
        recs = r["recs"][i]
        cb = int(W[i, 0, HR_CRC_BYTES])
        c["statuses"] |= set(recs[recs < 0].tolist())
        fr = recs[recs >= 0]
        c["good"][cb] |= set((fr[fr >= FRAME_OK] & 0xFFFF).tolist())
        c["len_0"] += int(((fr & 0xFFFF) == 0).sum())
        c["frames"] += len(fr)
        c["crc_error_lines"] += bool(W[i, -1, HR_CRC_ERRORS])
        c["length_error_lines"] += bool(W[i, -1, HR_LENGTH_ERRORS])
        at = 0
        for k in range(calls):
            m = int(r["nrecs"][k, i])
            row = recs[at:at + m]
            at += m
            w0, w1 = (W[i, k - 1] if k else zero), W[i, k]
            if not w0[HR_COUNTING] and w1[HR_COUNTING] and r["lens"][k, i]:
                if w1[HR_LEN] == 405 and w1[HR_ABORTS] == w0[HR_ABORTS]:
                    c["counting_by_overlong"] += 1
                elif w1[HR_ABORTS] > w0[HR_ABORTS] and w1[HR_LEN] != 405:
                    c["counting_by_abort"] += 1
            bad = row[(row >= 0) & (row < FRAME_OK)]
            # a call with one frame, a bad one: which of the three kinds it was shows in the statistics and the length
            if len(bad) == 1 and (row >= 0).sum() == 1 and k:
                if w1[HR_CRC_ERRORS] == w0[HR_CRC_ERRORS] + 1:
                    c["bad_crc"] += 1
                elif w1[HR_LENGTH_ERRORS] == w0[HR_LENGTH_ERRORS] + 1:
                    if bad[0] == 0:
                        c["bad_short"] += 1
                    elif bad[0] + cb > w0[HR_MAX_FRAME_LEN]:
                        c["bad_long"] += 1
                    else:
                        c["bad_misaligned"] += 1
    return c


def coverage_tx(r):
    W = all_words(r)
    calls, n = r["wants"].shape
    idle = W[:, :, HT_LEN] == 0
    c = {"residues": set(W[:, :, HT_NUM_BITS][idle & (W[:, :, HT_POS] == 0)].tolist()), "idle_octets": set(W[:, :, HT_IDLE_OCTET].reshape(-1).tolist()),
         "corrupt_after_shorter": 0, "corrupt_after_longer": 0, "underflows_empty": int((r["under"] > 0).sum()),
         "taken_by_handler": {k: int(((r["taken"] >> k) & 1).sum()) for k in (FRAME, FLAGS, ABORT, END)},
         "taken_between_calls": {k: int(((r["taken"] >> (8 + k)) & 1).sum()) for k in (FRAME, FLAGS, ABORT, END)},
         "ended": int(r["ended"].sum()), "refused": 0, "refused_too_long": 0, "pos_400": int((W[:, :, HT_POS] >= 400).sum()),
         "flag_counts": set(), "frame_lens": set()}
    for i in range(n):
        prev = None
        for (k, kind, arg, corrupt), res in zip(r["ops"][i].tolist(), r["results"][i].tolist()):
            c["refused"] += res != 0
            if kind == FLAGS and res == 0:
                c["flag_counts"].add(arg)
            if kind != FRAME or arg == 0:
                continue
            limit = r["cfgs"][i, 3] if r["cfgs"][i, 3] >= 0 else 400
            c["refused_too_long"] += arg > limit
            if res == 0:
                c["frame_lens"].add(arg)
                if corrupt and prev is not None:
                    c["corrupt_after_shorter"] += prev < arg
                    c["corrupt_after_longer"] += prev > arg
                prev = arg
    return c


def left_out(lens):
    """the largest share of the lines any one call leaves out"""
    return float((lens == 0).mean(axis=1).max())


# ---- files for the stand-alone program (tests/c_callers/hdlc_sweep_host.cpp) -------------------------------------------------

def write_sweep(path, sweeps):
    """records written"""
    records = 0
    with open(path, "wb") as f:
        f.write(np.array([0x48444C43, sum(len(s["cfgs"]) for s in sweeps)], np.int32).tobytes())
        for s in sweeps:
            n = len(s["cfgs"])
            for i in range(n):
                if s["family"] == "hdlc_tx":
                    kind, lens, cfg, fam = 2, s["wants"][:, i], s["cfgs"][i].tolist() + [0], 0
                    ops, raw = s["ops"][i], s["opbytes"][i].tobytes()
                else:
                    kind, lens, cfg, fam = {"int16": 0, "octets": 1}[s["form"]], s["lens"][:, i], s["cfgs"][i].tolist(), int(s["fam"][i])
                    ops = np.array([o + (0,) for o in s["ops"][i]], np.int32).reshape(-1, 4)
                    raw = s["data"][i].tobytes()
                f.write(np.array([kind, i, fam] + cfg + [len(lens), len(ops), len(raw), s["seed"]], np.int32).tobytes())
                f.write(np.ascontiguousarray(lens, np.int32).tobytes())
                f.write(np.ascontiguousarray(ops, np.int32).tobytes())
                f.write(raw + b"\0"*(-len(raw) % 4))
                records += 1
    return records
