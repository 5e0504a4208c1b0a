"""Lines at and beyond full scale for the int16 receiver banks, the configurations run on them, and the runs themselves.

Deterministic: numpy's sine and the 32-bit linear congruential generator of tests/g726_lines.py; the tone senders' lines
come from the oracle's restated senders (integer DDS, pinned to the reference).  tests/golden/loud_lines.npz stores a CRC
of every line (line_crcs()), so a platform on which a sample rounds the other way shows as that, not as a kernel mismatch.

  lines()            the 17 lines every family runs on, 16 000 samples (2 s) each
  tone_lines(kind)   a sender's digits x8 and x40, clipped: "dtmf", "bell", "r2f", "r2b"
  echo_pairs()       the (tx, rx) scenarios of the echo canceller
  rows(lines, n)     channel c of a bank takes line c mod L, rotated by 977 c samples: no two lanes of a wave in step
  *_CONFIGS          what each family is configured as
  run_*()            one receiver (the reference's or the oracle's: same methods) over one line on the uneven call schedule,
                     everything it gave; compact_*() the same cut down to what the fixture keeps
"""
import functools
import io
import os
import zipfile
import zlib

import numpy as np

from g726_lines import Lcg

N = 16000
CHUNKS = (160, 1, 7, 333)
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "loud_lines.npz")


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def _clip(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def _sine(freq, peak, phase=0.0):
    t = np.arange(N, dtype=np.float64)
    return peak*np.sin(2.0*np.pi*freq*t/8000.0 + phase)


def _gate(on, off):
    return ((np.arange(N) % (on + off)) < on).astype(np.float64)


def _square(period):
    return np.where((np.arange(N) % period) < period//2, 32767.0, -32768.0)


def _ans(reversals):
    """2100 Hz at 32 767, the phase turned over every 450 ms as ANS/ does"""
    t = np.arange(N, dtype=np.float64)
    flips = (np.arange(N)//3600) if reversals else 0
    return 32767.0*np.sin(2.0*np.pi*2100.0*t/8000.0 + np.pi*flips)


def _fsk(freq_zero, freq_one, baud, seed, peak):
    bits = (Lcg(seed).int16(N*baud//8000 + 2) >> 7) & 1
    which = bits[(np.arange(N)*baud)//8000]
    freq = np.where(which == 0, float(freq_zero), float(freq_one))
    return peak*np.sin(np.cumsum(2.0*np.pi*freq/8000.0))


def _impulses():
    x = np.zeros(N)
    at = 37
    k = 0
    while at < N:
        x[at] = 32767.0 if k % 2 == 0 else -32768.0
        at += 101 + 53*(k % 7)
        k += 1
    return x


@functools.lru_cache(maxsize=None)
def lines():
    """[(name, int16[N])]; each array read-only"""
    out = [("square6", _square(6)),
           ("square2", _square(2)),
           ("sine2280", _sine(2280, 50000.0)),
           ("sine2600", _sine(2600, 60000.0)),
           ("sine2400_2600", _sine(2400, 30000.0) + _sine(2600, 30000.0)),
           ("sine1100", _sine(1100, 40000.0)),
           ("gated2280", _sine(2280, 45000.0)*_gate(400, 400)),
           ("gated2600", _sine(2600, 45000.0)*_gate(400, 400)),
           ("gated2400_2600", (_sine(2400, 22500.0) + _sine(2600, 22500.0))*_gate(400, 400)),
           ("gated1100", _sine(1100, 40000.0)*_gate(4000, 4000)),
           ("ans2100", _ans(False)),
           ("ans2100_reversals", _ans(True)),
           ("noise", Lcg(0x10D).int16(N).astype(np.float64)),
           ("minus_rail", np.full(N, -32768.0)),
           ("impulses", _impulses()),
           ("fsk_v21", _fsk(1850, 1650, 300, 0x21, 45000.0)),
           ("fsk_bell202", _fsk(2200, 1200, 1200, 0x202, 45000.0))]
    done = []
    for name, x in out:
        x = _clip(x)
        x.setflags(write=False)
        done.append((name, x))
    return tuple(done)


def line(name):
    return dict(lines())[name]


FOREIGN_TO_CONNECT_TONES = ("square6", "square2", "sine2280", "sine2600", "gated2600", "noise", "minus_rail", "impulses")
TONE_KINDS = ("dtmf", "bell", "r2f", "r2b")


def _keyed(tx, digits, on, off):
    parts = []
    for d in digits:
        tx.put(d)
        parts.append(tx.tx(on))
        tx.put("\0")
        parts.append(tx.tx(off))
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def tone_lines(kind):
    """a sender's own digits, 8 and 40 times too loud"""
    from oracle import restated as orc
    from test_oracle_pin import use_golden_modem_tables
    use_golden_modem_tables()               # the senders' DDS reads the sine table among them
    if kind == "dtmf":
        tx = orc.DtmfTx()
        tx.put("123A456B789C*0#D1470")
        x = tx.tx(N)
    elif kind == "bell":
        tx = orc.BellMfTx()
        tx.put("*1234567890#ABC*1234567890#ABC")
        x = tx.tx(N)
    else:
        x = _keyed(orc.R2MfTx(kind == "r2f"), "1234567890BCDEF", 800, 400)
    x = np.concatenate([x, np.zeros(N, np.int16)])[:N].astype(np.float64)
    out = []
    for gain in (8, 40):
        y = _clip(x*gain)
        y.setflags(write=False)
        out.append(("%s_x%d" % (kind, gain), y))
    return tuple(out)


def _echo(tx, gain):
    h = np.zeros(32)
    h[2], h[9], h[25] = 0.6, -0.35, 0.2
    return gain*np.convolve(tx.astype(np.float64), h)[:N]


@functools.lru_cache(maxsize=None)
def echo_pairs():
    """[(name, tx, rx)]"""
    noise = Lcg(0xEC0).int16(N)
    talk = np.zeros(N)
    burst = Lcg(0x7A1C).int16(2500).astype(np.float64)
    talk[3000:4500] = burst[:1500]
    talk[9000:10000] = burst[1500:]
    tone = _clip(_sine(1000, 60000.0)*(np.arange(N) >= 800))           # a silence first: the run ends on the third tap set
    sq = _clip(_square(6))
    rail = np.full(N, -32768, np.int16)
    out = [("noise_gain1", noise, _echo(noise, 1.0)),
           ("noise_gain0125", noise, _echo(noise, 0.125)),
           ("noise_gain1_talk", noise, _echo(noise, 1.0) + talk),
           ("noise_gain0125_talk", noise, _echo(noise, 0.125) + talk),
           ("square_both", sq, sq),
           ("tone1000", tone, _echo(tone, 0.5)),
           ("minus_rail_both", rail, rail)]
    done = []
    for name, tx, rx in out:
        tx, rx = _clip(tx), _clip(rx)
        tx.setflags(write=False)
        rx.setflags(write=False)
        done.append((name, tx, rx))
    return tuple(done)


def offset(c):
    return (977*c) % N


def rows(arrays, n):
    """[n, N]: channel c takes arrays[c mod L] rotated by offset(c)"""
    return np.stack([np.roll(arrays[c % len(arrays)], -offset(c)) for c in range(n)])


def family_lines(family):
    """the lines a family's banks run on: the 17, and for a tone bank its own sender's overdriven digits as well"""
    if family in TONE_KINDS:
        return lines() + tone_lines(family)
    return lines()


def pinned_rows(family):
    """[(name, row)]: every line of the family as the first channel that carries it sees it"""
    named = family_lines(family)
    r = rows([x for _, x in named], len(named))
    return [(name, r[c]) for c, (name, _) in enumerate(named)]


def pinned_echo_rows():
    p = echo_pairs()
    tx = rows([t for _, t, _ in p], len(p))
    rx = rows([r for _, _, r in p], len(p))
    return [(name, tx[c], rx[c]) for c, (name, _, _) in enumerate(p)]


def line_crcs():
    out = [crc(x) for _, x in lines()]
    for kind in TONE_KINDS:
        out += [crc(x) for _, x in tone_lines(kind)]
    for _, tx, rx in echo_pairs():
        out += [crc(tx), crc(rx)]
    return np.array(out, np.uint32)


# ---- configurations ------------------------------------------------------------------------------------------------------
SIGRX_CONFIGS = tuple((t, m) for t in (1, 2, 3) for m in (0x00, 0x40, 0xC0))
SIGTX_TYPES = (1, 2, 3)
MCT_CONFIGS = tuple((t, cb) for t in (1, 2, 3, 4, 7, 8, 9) for cb in (True, False))
# the presets and framing modes tests/test_fsk_gpu.py names (framed: the default 8N1)
FSK_CONFIGS = ((1, 1), (1, 0), (0, 1), (2, 0), (6, 1), (3, 0), (7, 0), (10, 1), (1, 2), (0, 2), (7, 2), (2, 2))
ECHO_CONFIGS = tuple((taps, mode, hpf) for taps in (32, 128, 512) for mode in (0x00, 0x01, 0x06, 0x67) for hpf in (False, True))
TONE_CONFIGS = (("dtmf", 0), ("dtmf", 1), ("bell", 0), ("r2f", 0), ("r2b", 0), ("st", 0))       # (kind, dial-tone filter)


def st_desc(D):
    """the super-tone descriptor: 1100 Hz (the gated line's own), a dial-tone pair, a busy cadence, 2100 Hz"""
    d = D()
    t = d.add_tone()
    d.add_element(t, 1100, 0, 400, 600)
    d.add_element(t, 0, 0, 400, 600)
    t = d.add_tone()
    d.add_element(t, 350, 440, 400, 0)
    t = d.add_tone()
    d.add_element(t, 480, 620, 450, 550)
    d.add_element(t, 0, 0, 450, 550)
    t = d.add_tone()
    d.add_element(t, 2100, 0, 300, 0)
    t = d.add_tone()
    d.add_element(t, 2280, 2600, 40, 60)
    return d


def sigtx_script(tone_type, k):
    """(mode, duration) pairs an update request is answered with: mostly the media passed through under the tone(s)"""
    g = Lcg(0x5160 + 16*tone_type + k)
    modes = (0x11, 0x15, 0x14, 0x10, 0x11, 0x15, 0x01, 0x05)
    durs = (37, 160, 161, 400, 801, 1, 333, 1200)
    v = g.int16(80) & 0x7FFF
    return [(modes[int(a) % 8], durs[int(b) % 8]) for a, b in zip(v[:40], v[40:])] + [(0x15 if tone_type == 3 else 0x11, 0)]


# ---- receivers of either side (oracle.ref / oracle.restated: the same methods) ---------------------------------------------
def makers(side):
    if side == "ref":
        from oracle import ref as m
        return {"sigrx": m.SigToneRx, "sigtx": m.SigToneTx, "mct": m.MctRx, "fsk": m.FskRx, "echo": m.EchoCan, "dtmf": m.DtmfRx,
                "bell": m.BellMfRx, "r2": m.R2MfRx, "st_desc": m.SuperToneDesc, "st": m.SuperToneRx}
    from oracle import restated as m
    return {"sigrx": m.SigToneRx, "sigtx": m.SigToneTx, "mct": m.Mct, "fsk": m.Fsk, "echo": m.EchoCan, "dtmf": m.Dtmf,
            "bell": m.BellMf, "r2": m.R2Mf, "st_desc": m.SuperToneDesc, "st": m.SuperTone}


def calls(total=N, chunks=CHUNKS):
    pos = 0
    k = 0
    while pos < total:
        m = min(chunks[k % len(chunks)], total - pos)
        yield pos, m
        pos += m
        k += 1


def on_rail(y, x):
    """samples of y on +32767 / -32768 where x is not that same sample"""
    y = np.asarray(y, np.int32)
    return int(np.count_nonzero(((y == 32767) | (y == -32768)) & (y != np.asarray(x, np.int32))))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_sigrx(make, cfg, x):
    from test_oracle_pin import sigtone_rx_run
    out, ev, snaps = sigtone_rx_run(make["sigrx"](cfg[0], cfg[1]), x, CHUNKS)
    return {"out": out, "reports": ev, "snaps": snaps}


def compact_sigrx(r, x):
    return {"reports": r["reports"], "snaps": r["snaps"],
            "sums": np.array([crc(r["out"]), len(r["out"]), on_rail(r["out"], x)], np.uint32)}


def run_sigtx(make, tone_type, k, x):
    """full-scale media under the tones: every update request answered from sigtx_script()"""
    tx = make["sigtx"](tone_type, sigtx_script(tone_type, k))
    tx.set_mode(0x15 if tone_type == 3 else 0x11, 120)
    out, snaps = [], []
    for i, (pos, m) in enumerate(calls()):
        out.append(tx.tx(x[pos:pos + m]))
        if i % 10 == 9:
            snaps.append(tx.snapshot())
    snaps.append(tx.snapshot())
    return {"out": np.concatenate(out), "snaps": np.stack(snaps), "requests": tx.requests()}


def compact_sigtx(r, x):
    return {"snaps": r["snaps"],
            "sums": np.array([crc(r["out"]), len(r["out"]), r["requests"], on_rail(r["out"], x)], np.uint32)}


def run_mct(make, cfg, x):
    """mct_run() of tests/test_oracle_pin.py on the uneven schedule"""
    tone_type, use_callback = cfg
    rx = make["mct"](tone_type, use_callback)
    snaps, hits = [], []
    for i, (pos, m) in enumerate(calls()):
        rx.rx(x[pos:pos + m])
        if i % 10 == 9:
            snaps.append(rx.snapshot())
            if not use_callback:
                hits.append(rx.get())
    snaps.append(rx.snapshot())
    ev = np.array([(e["a"], e["b"], e["c"]) for e in rx.sink.events() if e["kind"] == 1], np.int32).reshape(-1, 3)
    return {"reports": ev, "snaps": np.stack(snaps), "hits": np.array(hits, np.int32)}


def compact_mct(r, x):
    return {"reports": r["reports"], "hits": r["hits"], "snaps": r["snaps"]}


def run_fsk(make, cfg, x):
    from test_oracle_pin import fsk_run
    ev, snaps = fsk_run(make["fsk"](cfg[0], cfg[1]), x, CHUNKS)
    return {"events": ev, "snaps": snaps}


def compact_fsk(r, x):
    return {"head": r["events"][:64], "final": r["snaps"][-1][:28],
            "sums": np.array([len(r["events"]), crc(r["events"]), crc(r["snaps"]), len(r["snaps"])], np.uint32)}


def echo_snapshot_words(s, fields):
    return np.array([s[k] for k in fields], np.int64).astype(np.int32)


def run_echo(make, cfg, tx, rx):
    """every clean sample; the control words after every call; taps and history at the end"""
    from oracle import ref
    taps, mode, hpf = cfg
    ec = make["echo"](taps, mode)
    clean, words = [], []
    for pos, m in calls():
        clean.append(ec.run(tx[pos:pos + m], rx[pos:pos + m], hpf))
        words.append(echo_snapshot_words(ec.snapshot(), ref.ECHO_FIELDS))
    s = ec.snapshot()
    return {"clean": np.concatenate(clean), "words": np.stack(words), "taps32": s["taps32"].copy(), "taps16": s["taps16"].copy(),
            "history": s["history"].copy()}


def compact_echo(r, rx):
    t = r["taps32"].astype(np.int64)
    return {"final": r["words"][-1],
            "sums": np.array([crc(r["clean"]), crc(r["words"]), crc(r["taps32"]), crc(r["taps16"]), crc(r["history"]),
                              on_rail(r["clean"], rx), int(np.abs(t).max())], np.uint32)}


_TONE_INTS = {"dtmf": ("current_sample", "duration", "last_hit", "in_digit", "current_digits", "lost_digits"),
              "bell": ("current_sample", "current_digits", "lost_digits"), "r2f": ("current_sample", "current_digit"),
              "r2b": ("current_sample", "current_digit")}


def _tone_words(kind, s):
    w = [_bits(s["v2"]), _bits(s["v3"])]
    if kind == "dtmf":
        w.append(_bits([s["energy"]]))
    if kind == "bell":
        w.append(np.asarray(s["hits"], np.int32).view(np.uint32))
    w.append(np.array([s[k] for k in _TONE_INTS[kind]], np.int64).astype(np.uint32))
    return np.concatenate(w)


def make_tone(make, cfg):
    kind, filt = cfg
    if kind == "dtmf":
        d = make["dtmf"](0)
        if filt:
            d.parms(filter_dialtone=1)
        return d
    if kind == "bell":
        return make["bell"](0)
    if kind == "st":
        return make["st"](st_desc(make["st_desc"]), True)
    return make["r2"](kind == "r2f")


def run_tone(make, cfg, x):
    """the callbacks' events, the digits, the filter state and counters after every call (the super-tone receiver: events)"""
    kind = cfg[0]
    d = make_tone(make, cfg)
    words = []
    for pos, m in calls():
        if hasattr(d, "_rx"):
            d.rx(x[pos:pos + m], want_blocks=False)         # the oracle's detectors can trace their blocks: not wanted here
        else:
            d.rx(x[pos:pos + m])
        if kind != "st":
            words.append(_tone_words(kind, d.snapshot()))
    digits = d.get() if kind in ("dtmf", "bell") else ""
    ev = d.sink.events()
    return {"events": np.frombuffer(ev.tobytes(), np.uint8), "n_events": len(ev), "digits": np.frombuffer(digits.encode("latin1"), np.uint8),
            "words": np.stack(words) if words else np.zeros((0, 1), np.uint32)}


def compact_tone(r, x):
    return {"digits": r["digits"], "final": r["words"][-1] if len(r["words"]) else np.zeros(0, np.uint32),
            "sums": np.array([r["n_events"], crc(r["events"]), crc(r["words"])], np.uint32)}


def same(a, b):
    """two results, or two compact forms: the same keys and the same bytes"""
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            return k
    return None


def all_cases(make):
    """{key: compact form} of every (configuration, line) the GPU tests use, run on `make`'s side"""
    out = {}
    for cfg in SIGRX_CONFIGS:
        for name, x in pinned_rows("sigrx"):
            out["sigrx/%d_%02x/%s" % (cfg + (name,))] = compact_sigrx(run_sigrx(make, cfg, x), x)
    for t in SIGTX_TYPES:
        for k, (name, x) in enumerate(pinned_rows("sigtx")):
            out["sigtx/%d/%s" % (t, name)] = compact_sigtx(run_sigtx(make, t, k, x), x)
    for cfg in MCT_CONFIGS:
        for name, x in pinned_rows("mct"):
            out["mct/%d_%d/%s" % (cfg[0], int(cfg[1]), name)] = compact_mct(run_mct(make, cfg, x), x)
    for cfg in FSK_CONFIGS:
        for name, x in pinned_rows("fsk"):
            out["fsk/%d_%d/%s" % (cfg + (name,))] = compact_fsk(run_fsk(make, cfg, x), x)
    for cfg in ECHO_CONFIGS:
        for name, tx, rx in pinned_echo_rows():
            out["echo/%d_%02x_%d/%s" % (cfg[0], cfg[1], int(cfg[2]), name)] = compact_echo(run_echo(make, cfg, tx, rx), rx)
    for cfg in TONE_CONFIGS:
        for name, x in pinned_rows(cfg[0]):
            out["%s/%d/%s" % (cfg[0], cfg[1], name)] = compact_tone(run_tone(make, cfg, x), x)
    return out


# ---- the fixture: {case key: {field: array}} as one archive with a few long members ----------------------------------------
def pack(cases):
    """-> {member: array}: per field the values of all cases back to back, with the case keys and the lengths"""
    keys = sorted(cases)
    out = {"keys": np.array(keys), "line_crcs": line_crcs()}
    fields = sorted({(k.split("/")[0], f) for k in keys for f in cases[k]})
    for fam, f in fields:
        mine = [k for k in keys if k.split("/")[0] == fam]
        arrs = [np.ascontiguousarray(cases[k][f]) for k in mine]
        out["%s.%s.data" % (fam, f)] = np.concatenate([a.reshape(-1) for a in arrs])
        out["%s.%s.shape" % (fam, f)] = np.array([a.shape + (0,)*(2 - a.ndim) for a in arrs], np.int32)
    return out


def unpack(g):
    keys = [str(k) for k in g["keys"]]
    fams = {}
    for k in keys:
        fams.setdefault(k.split("/")[0], []).append(k)
    out = {k: {} for k in keys}
    for member in g.files:
        if not member.endswith(".data"):
            continue
        fam, f, _ = member.split(".")
        data, shapes = g[member], g["%s.%s.shape" % (fam, f)]
        at = 0
        for k, sh in zip(fams[fam], shapes):
            sh = tuple(int(v) for v in sh)
            shape = sh if sh[1] else sh[:1]
            n = int(np.prod(shape))
            out[k][f] = data[at:at + n].reshape(shape)
            at += n
    return out


def write_archive(path, members):
    """an .npz whose bytes depend on the arrays alone (fixed member order and time stamps)"""
    with zipfile.ZipFile(path, "w") as z:
        for name in sorted(members):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(members[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def load(path=None):
    return np.load(path or GOLDEN)
