"""The lines of tests/loud_lines.py for the modem receivers (V.29, V.27ter, V.17), the runs on them, the "lost packet"
cases of xxx_rx_fillin(), and the fixture tests/golden/loud_modems.npz.

  RATES                      every (modem, bit rate)
  modem_lines(name, rate)    the 17 foreign lines() plus the modem's own transmission x8 and x40, clipped
  modem_rows(name, rate, n)  channel c of a bank: a foreign line as rows() gives it (line c mod L, rotated by 977 c); an own
                             line not rotated -- that would cut the transmission in two -- but started c mod 160 samples late
  run_modem()                one receiver (the reference's or the oracle's: same methods) over one line on the uneven call
                             schedule: the events of every call, the final words
  compact_modem()            the same cut down to what the fixture keeps
  fillin_points() / run_fillin()  a clean transmission on 160-sample calls, one of them (or its first 97 samples) replaced by
                             a fill-in

The own lines come from the oracle's restated senders (pinned to the reference's), so they can be made wherever the oracle
runs; the fixture stores a CRC of every line.
"""
import functools
import os

import numpy as np

import loud_lines as ll

RATES = (("v29", 9600), ("v29", 7200), ("v29", 4800), ("v27ter", 4800), ("v27ter", 2400),
         ("v17", 14400), ("v17", 12000), ("v17", 9600), ("v17", 7200), ("v17", 4800))
GOLDEN = os.path.join(ll.HERE, "golden", "loud_modems.npz")
OWN_SEED = 7
OWN_LEAD = 300                  # silent samples before the transmission
OWN_SAMPLES = 15000             # V.17's long train alone is some 11 150 samples; 1 500 and more of data after it
STAGE, SIGNAL_PRESENT = 6, 9    # int words of all three receivers ("State word map" of the kernels' headers)
PARKED = {"v29": 7, "v27ter": 6, "v17": 12}
STEADY = ("square6", "square2", "sine2280", "sine2600", "sine2400_2600", "sine1100", "noise", "fsk_v21", "fsk_bell202")
GATED = ("gated2280", "gated2600", "gated2400_2600")


def rate_id(r):
    return "%s_%d" % r


def use_tables():
    """the oracle's receivers and senders on the committed tables (the senders' pulse shapers: the library's host builder's,
    held to the committed copies of the reference's)"""
    from test_oracle_pin import use_v17_tx_tables
    use_v17_tx_tables(True)


def senders(side):
    if side == "ref":
        from oracle import ref as m
    else:
        from oracle import restated as m
    return {"v29": m.V29Tx, "v27ter": m.V27terTx, "v17": m.V17Tx}


def receivers(side):
    if side == "ref":
        from oracle import ref as m
        return {"v29": m.V29Rx, "v27ter": m.V27terRx, "v17": m.V17Rx}
    from oracle import restated as m
    return {"v29": m.V29, "v27ter": m.V27ter, "v17": m.V17}


@functools.lru_cache(maxsize=None)
def own_lines(name, bit_rate, side="orc"):
    """the modem's own transmission (scrambler seed 7, the sender's default level), 8 and 40 times too loud"""
    if side == "orc":
        use_tables()
    sig = senders(side)[name](bit_rate, False, OWN_SEED).tx(OWN_SAMPLES)
    assert len(sig) == OWN_SAMPLES
    x = np.zeros(ll.N)
    x[OWN_LEAD:OWN_LEAD + OWN_SAMPLES] = sig
    out = []
    for gain in (8, 40):
        y = ll._clip(x*gain)
        y.setflags(write=False)
        out.append(("own_x%d" % gain, y))
    return tuple(out)


def modem_lines(name, bit_rate):
    """[(name, int16[N])]: the 17 lines and own_x8, own_x40"""
    return ll.lines() + own_lines(name, bit_rate)


def delayed(x, d):
    return np.concatenate([np.zeros(d, np.int16), x])[:ll.N]


def modem_rows(name, bit_rate, n):
    named = modem_lines(name, bit_rate)
    foreign = len(ll.lines())
    out = []
    for c in range(n):
        k = c % len(named)
        x = named[k][1]
        out.append(np.roll(x, -ll.offset(c)) if k < foreign else delayed(x, c % 160))
    return np.stack(out)


def row_names(name, bit_rate, n):
    named = modem_lines(name, bit_rate)
    return [named[c % len(named)][0] for c in range(n)]


def line_crcs():
    out = [ll.crc(x) for _, x in ll.lines()]
    for r in RATES:
        out += [ll.crc(x) for _, x in own_lines(*r)]
    return np.array(out, np.uint32)


# ---- one receiver over one line ------------------------------------------------------------------------------------------
def run_modem(make, name, bit_rate, x, chunks=ll.CHUNKS):
    """the put_bit / status values of every call, the float (as bit patterns) and integer words at the end"""
    rx = make[name](bit_rate)
    per_call = []
    for pos, m in ll.calls(len(x), chunks):
        rx.sink.clear()
        rx.rx(x[pos:pos + m])
        per_call.append(rx.sink.events()["a"].astype(np.int8))
    f, w = rx.snapshot()
    return {"calls": per_call, "fwords": ll._bits(f).copy(), "iwords": np.asarray(w, np.int32).copy()}


def compact_modem(r):
    ev = np.concatenate(r["calls"])
    return {"call_crcs": np.array([ll.crc(e) if len(e) else 0 for e in r["calls"]], np.uint32),
            "status": ev[ev < 0].copy(), "sums": np.array([np.count_nonzero(ev >= 0), ll.crc(ev)], np.uint32),
            "fwords": r["fwords"], "iwords": r["iwords"]}


def same_run(a, b):
    """two run_modem() results: None, or where they part"""
    if len(a["calls"]) != len(b["calls"]):
        return "number of calls"
    for i, (x, y) in enumerate(zip(a["calls"], b["calls"])):
        if not np.array_equal(x, y):
            return "events of call %d" % i
    for k in ("iwords", "fwords"):
        bad = np.nonzero(a[k] != b[k])[0]
        if bad.size:
            return "%s %s" % (k, bad[:8])
    return None


def non_finite(fwords):
    return int(np.count_nonzero((np.asarray(fwords, np.uint32) & 0x7FFFFFFF) >= 0x7F800000))


def cycles(status, *codes):
    """how often the codes come in a row in a status list"""
    s = [int(v) for v in status]
    k = len(codes)
    return sum(1 for i in range(len(s) - k + 1) if tuple(s[i:i + k]) == codes)


# ---- lost packets ----------------------------------------------------------------------------------------------------------
# 160 samples are a whole number of bauds of every rate here and 36 turns of the nominal carrier: a receiver comes out of
# fillin(160) with its symbol phase where it was and its carrier phase moved by the loop's correction alone.  So the words
# right after the fill-in are kept as well, and two points lose 97 samples, which are neither.
FILLIN_POINTS = ("start", "training", "data", "parked", "training_97", "data_97")


def clean_input(name, bit_rate):
    return np.load(os.path.join(ll.HERE, "golden", "%s_%d.npz" % (name, bit_rate)))["amp"]


def run_fillin(make, name, bit_rate, x, at, fillin, lost=160, chunk=160):
    """x on calls of `chunk` samples, the first `lost` samples of call `at` replaced by fillin(rx, lost): all the events, the
    words right after the fill-in and at the end"""
    rx = make[name](bit_rate)
    after = None
    for i, k in enumerate(range(0, len(x), chunk)):
        if i == at:
            fillin(rx, lost)
            after = rx.snapshot()
            if lost < chunk:
                rx.rx(x[k + lost:k + chunk])
        else:
            rx.rx(x[k:k + chunk])
    f, w = rx.snapshot()
    return {"events": rx.sink.events()["a"].astype(np.int8), "fwords": ll._bits(f).copy(), "iwords": np.asarray(w, np.int32).copy(),
            "fwords_after": ll._bits(after[0]).copy(), "iwords_after": np.asarray(after[1], np.int32).copy()}


def calls_with(events_per_call, code):
    return [i for i, e in enumerate(events_per_call) if code in e]


def fillin_points(make, name, bit_rate):
    """{point: (line, call, samples lost)}: call 0 (no signal yet); the third call after TRAINING_IN_PROGRESS; the third after
    the last TRAINING_SUCCEEDED (V.17's clean line is a long-train burst that ends with its training and a short-train burst
    that carries the data); on sine2280 the third after TRAINING_FAILED (the receiver PARKED)"""
    x = clean_input(name, bit_rate)
    clean = run_modem(make, name, bit_rate, x, (160,))["calls"]
    tone = ll.line("sine2280")
    loud = run_modem(make, name, bit_rate, tone, (160,))["calls"]
    at_train = calls_with(clean, -3)[0] + 3
    at_data = calls_with(clean, -4)[-1] + 3
    assert at_train < calls_with(clean, -4)[0] and at_data + 5 < calls_with(clean, -1)[-1]
    return {"start": (x, 0, 160), "training": (x, at_train, 160), "data": (x, at_data, 160),
            "parked": (tone, calls_with(loud, -5)[0] + 3, 160), "training_97": (x, at_train + 1, 97), "data_97": (x, at_data + 1, 97)}


def ref_fillin(name):
    from oracle import ref
    fn = getattr(ref.lib(), name + "_rx_fillin")
    return lambda rx, n: fn(rx.p, n)


def all_cases(make, fillin_of=None):
    """{key: {field: array}} of every (modem, rate, line) run on `make`'s side, un-rotated; with fillin_of (the reference's
    xxx_rx_fillin), the lost-packet cases as well"""
    out = {}
    for name, rate in RATES:
        for lname, x in modem_lines(name, rate):
            out["rx/%s_%d/%s" % (name, rate, lname)] = compact_modem(run_modem(make, name, rate, x))
        if fillin_of is not None:
            for point, (x, at, lost) in fillin_points(make, name, rate).items():
                r = run_fillin(make, name, rate, x, at, fillin_of(name), lost)
                r["at"] = np.array([at, lost], np.int32)
                out["fillin/%s_%d/%s" % (name, rate, point)] = r
    return out


def pack(cases):
    out = ll.pack(cases)
    out["line_crcs"] = line_crcs()
    return out


def load(path=None):
    return np.load(path or GOLDEN)
