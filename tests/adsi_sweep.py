"""The ADSI sweep: generated caller-ID lines, sender scripts and call schedules, and what the reference makes of them.

Everything comes from fixed seeds through codec_sweep.Lcg, in integers; nothing generated is committed.  The reference is the
live one behind oracle/ref_adsi.py (oracle/_ref/libspandsp_adsi_ref.so): its own sender renders the `sent` bursts, its dds the
lines of the run-length modulator, its AWGN the noise, and its adsi_rx / adsi_tx say what every line has to give.  Messages
are put together by the project's own host helpers (engine.adsi_add_field / adsi_pack_message); tests/adsi_lines.py frames
bytes into bits.

A bank is N_GPU = 16*WAVE + 37 lines, channel c in standard STANDARDS[c % 4].  The nine receiver families are dealt round
robin: 9 is coprime to 4, so any 36 consecutive lines hold every family in every standard.  tests/test_adsi_sweep.py runs
what needs no GPU, tests/test_adsi_sweep_gpu.py the banks; profiles/adsi_sweep.md has the figures."""
import numpy as np

import adsi_lines as AL
from codec_sweep import Lcg, seeds_of

WAVE = 64
SEED = 0xAD51
N_GPU = 16*WAVE + 37
STANDARDS = AL.STANDARDS
FAMILIES = ("sent", "levels", "framed", "back_to_back", "fast", "drift", "carrier_drop", "cross", "any_int16")
DEAL = len(FAMILIES)                # 9: coprime to the 4 standards
RX_CALLS = 64                       # calls of a receiver sweep with per-channel lengths
TICK = 160
RX_TICKS = 128                      # calls of the sweep on plain ticks
TX_CALLS = 60
PROBES = (0, 1, 2, 3, 63, 64, 65, 517, N_GPU - 2, N_GPU - 1)
PINNED = ()                         # (kind, seed, line): nothing has failed yet
LONGEST = {AL.CLASS: 255, AL.CLIP: 255, AL.ACLIP: 255, AL.JCLIP: 119}
OP_PUT, OP_PREAMBLE, OP_ALERT, OP_RESTART, OP_SHUT_DOWN = 1, 2, 3, 4, 5
FT_SHUTDOWN = 23                    # among a sender's 24 words
ADT_MSG_LEN, ADT_TX_SIGNAL_ON, ADT_TONE_SECTION = 8, 9, 10
ADR_ONES, ADR_MSG_LEN, ADR_FRAMING_ERRORS = 1, 4, 5
ALERT_SAMPLES = 880 + 480           # 110 ms of tone and 60 ms of silence
# round(1000*10^(-a/20)) for a = 10 .. 24 dB: the presets send at -14 dBm0 and hear from -30 dBm0
ATTENUATION = (316, 282, 251, 224, 200, 178, 158, 141, 126, 112, 100, 89, 79, 71, 63)
SNRS = (None, 30, 20, 14, 10, 6, 3)
FAST_TYPES = (0x55, 0xAA, 0x52, 0xD5, 0x25)
FAST_FIRST = (6, 7, 8, 9, 10)       # a transitional bit's length in half samples: 3 .. 5, where a sender's is 6.67


class Draws:
    """one line's stream of 16-bit draws"""

    def __init__(self, seed, count=8192):
        self.v = Lcg(np.array([seed], np.uint64)).u16(count)[0]
        self.i = 0

    def below(self, n):
        self.i += 1
        return int(self.v[self.i - 1]) % n

    def between(self, lo, hi):
        return lo + self.below(hi - lo + 1)

    def bytes(self, n, mask=0xFF):
        self.i += n
        return bytes((self.v[self.i - n:self.i] & mask).astype(np.uint8).tolist())


def _ref():
    from oracle import ref_adsi
    return ref_adsi


def _engine():
    from spandsp_amd import engine
    return engine


def family_of(i):
    return np.asarray(i) % DEAL


def standard_of(i):
    return STANDARDS[i % 4]


# ---- messages -------------------------------------------------------------------------------------------------------------

MESSAGE_KINDS = ("fields", "fields", "fields", "none", "empty", "sixteen", "dle", "longest", "over")


def message(d, standard, kind=None):
    """a message as adsi_tx_put_message() takes it, built field by field with the project's adsi_add_field()"""
    E = _engine()
    kind = kind or MESSAGE_KINDS[d.below(len(MESSAGE_KINDS))]
    mask = 0x7F if standard == AL.JCLIP else 0xFF
    msg = E.adsi_add_field(standard, b"", d.between(1, 0xFE) & mask | 1)
    if kind == "none":
        return msg
    if kind == "empty":
        return E.adsi_add_field(standard, msg, d.between(1, 0x7F), b"")
    if kind in ("longest", "over"):
        # one field whose body has no DLE and is not 0x10 long: the length lands where it is aimed
        size = LONGEST[standard] + (kind == "over") - len(msg) - 2
        body = bytes(b if b != AL.DLE else 0x11 for b in d.bytes(size, mask))
        msg = E.adsi_add_field(standard, msg, 0x02, body)
        assert len(msg) == LONGEST[standard] + (kind == "over")
        return msg
    for _ in range(d.between(1, 4)):
        n = 0x10 if kind == "sixteen" else d.below(21)
        body = bytearray(d.bytes(n, mask))
        if kind == "dle" and n:
            body[d.below(n)] = AL.DLE
            body[d.below(n)] = AL.DLE
        msg = E.adsi_add_field(standard, msg, AL.DLE if kind == "dle" and d.below(4) == 0 else d.between(1, 0x7F), bytes(body))
    return msg


def packed(standard, msg):
    """what the project's packing puts on the line, checked against tests/adsi_lines.py's restatement"""
    p = _engine().adsi_pack_message(standard, msg)
    assert p == AL.pack(standard, msg), (standard, msg)
    return p


# ---- receiver lines -----------------------------------------------------------------------------------------------------

def _edges(n_bits, per_mille=1000):
    """sample index at which bit k begins, k = 0 .. n_bits, for bits of 8000/1200 samples times per_mille/1000, rounded"""
    k = np.arange(n_bits + 1, dtype=np.int64)
    return (k*40*per_mille + 3000)//6000


def _nominal_runs(bits, per_mille=1000):
    e = _edges(len(bits), per_mille)
    return [(b, int(e[k + 1] - e[k])) for k, b in enumerate(bits)]


def _fast_runs(bits, first):
    """runs of k equal bits last round(first/2 + 6.667*(k - 1)) samples: only the bit behind a transition is shortened"""
    runs, k = [], 0
    while k < len(bits):
        j = k
        while j < len(bits) and bits[j] == bits[k]:
            j += 1
        runs.append((bits[k], (3*first + 40*(j - k - 1) + 3)//6))
        k = j
    return runs


def _bytes_bits(data, stop_bits=1):
    out = []
    for b in data:
        out += AL.byte_bits(b, stop_bits)
    return out


def _stops(standard):
    return 4 if standard == AL.JCLIP else 1


def _good(d, standard, marks=30):
    """(bits, packed) of a short good message behind `marks` marks"""
    p = packed(standard, message(d, standard, "fields"))
    return [1]*marks + _bytes_bits(p, _stops(standard)) + [1]*5, p


def _jclip_raw(msg_type, body, strip_len_parity=False, first=AL.DLE):
    """a J-CLIP message framed by hand: parity on every byte but, if asked, the length's; the CRC over what is sent"""
    out = [first, AL.SOH, 0x07, AL.DLE, AL.STX, msg_type, len(body)] + list(body) + [AL.DLE, AL.ETX]
    out = [(b & 0x7F) | ((bin(b & 0x7F).count("1") & 1) << 7) for b in out]
    if strip_len_parity:
        out[6] ^= 0x80
    crc = AL.crc16(out[2:])
    return bytes(out + [crc & 0xFF, crc >> 8])


_marks = {}                 # the marks of the `marks` line being built, by its draws
META = {}                   # (seed, line): (the framed case, its marks or 0), filled in as lines are built
FRAMED_KINDS = ("marks", "stop0", "check", "not_dle", "len_parity", "past_256", "marks", "check")


def _framed_bits(d, standard, kind):
    """the bits of one `framed` line: the case, then a good message right behind it"""
    sb = _stops(standard)
    jclip = standard == AL.JCLIP
    p = packed(standard, message(d, standard, "fields"))
    bits = [1]*40
    if kind == "marks":
        # 9, 10, 11 or 12 marks behind a stop bit in mid-message: 11 restart the message, 10 do not
        at = d.between(1, len(p) - 1)
        k = d.between(9, 12)
        _marks[id(d)] = k
        bits += _bytes_bits(p[:at], sb) + [1]*(k - (sb - 1)) + _bytes_bits(p[at:], sb)
    elif kind == "stop0":
        at = d.below(len(p))
        for i, b in enumerate(p):
            bits += AL.byte_bits(b, sb, stop=0 if i == at else 1)
    elif kind == "check":
        q = bytearray(p)
        q[len(q) - 1 - d.below(2 if jclip else 1)] ^= 1 << d.below(8)
        bits += _bytes_bits(q, sb)
    elif kind == "not_dle" and jclip:
        bits += _bytes_bits(_jclip_raw(0x40, d.bytes(d.below(12), 0x7F), first=(0x11, 0x90 ^ 0x80, 0x00)[d.below(3)]), sb)
    elif kind == "len_parity" and jclip:
        for strip in (False, True):
            bits += _bytes_bits(_jclip_raw(0x40, d.bytes(d.between(1, 7), 0x7F), strip_len_parity=strip), sb) + [1]*20
    elif kind == "past_256" and not jclip:
        # a length byte that points past 256: msg_len sticks at 256 through a message behind 5 marks, until 12 marks
        bits = [1]*20 + _bytes_bits(bytes([0x80, 0xFE]) + d.bytes(256), sb)
        g, _ = _good(d, standard, 5)
        bits += g + [1]*7
    else:
        # (the J-CLIP cases on the other standards and the other way round: a length byte one off either way)
        q = bytearray(p)
        q[6 if jclip else 1] += (1, -1)[d.below(2)]
        bits += _bytes_bits(q, sb)
    g, _ = _good(d, standard, d.between(11, 40))
    return bits + g


def rx_line(i, seed=SEED, family=None):
    """the samples of receiver line i (content only: rx_lines() pads it to what its schedule takes)"""
    R = _ref()
    standard = standard_of(i)
    fam = FAMILIES[int(family_of(i))] if family is None else family
    d = Draws(int(seeds_of(i + 1, seed, salt=1)[i]))
    z = lambda n: np.zeros(n, np.int16)
    if fam in ("sent", "levels", "cross"):
        parts = [z(d.below(700))]
        for _ in range(d.between(1, 3)):
            s = standard
            if fam == "cross":
                # a Bell 202 burst into a V.23 receiver and the other way round; a J-CLIP burst into a CLIP receiver
                s = {AL.CLASS: (AL.CLIP, AL.JCLIP), AL.CLIP: (AL.CLASS, AL.JCLIP), AL.ACLIP: (AL.CLASS, AL.JCLIP),
                     AL.JCLIP: (AL.CLASS, AL.CLIP)}[standard][d.below(2)]
            pre = None if d.below(2) else (d.below(120), d.between(12, 90), d.below(12), d.between(1, 5))
            msg = message(d, s, ("fields", "fields", "none", "empty", "sixteen", "dle", "longest")[d.below(7)])
            parts += [R.tx_burst(s, msg, alert=d.below(4) == 0, preamble=pre), z(d.between(1, 1500))]
        x = np.concatenate(parts)
        if fam == "levels":
            a = d.below(len(ATTENUATION))
            snr = SNRS[d.below(len(SNRS))]
            x = R.impair(x, ATTENUATION[a], 1000, seed=1 + d.below(30000), noise_dbm0=0 if snr is None else -14 - (10 + a) - snr)
        return x
    if fam == "framed":
        kind = FRAMED_KINDS[(i//DEAL//4 + d.below(2)*4) % len(FRAMED_KINDS)]
        bits = _framed_bits(d, standard, kind)
        META[(seed, i)] = (kind, _marks.pop(id(d), 0))
        return np.concatenate([z(d.below(300)), R.runs_line(standard, _nominal_runs(bits)), z(200)])
    if fam in ("back_to_back", "fast"):
        sb = _stops(standard)
        bits = [1]*60
        first = FAST_FIRST[d.below(len(FAST_FIRST))]
        for _ in range(40 if standard == AL.JCLIP else 110):
            t = FAST_TYPES[d.below(len(FAST_TYPES))] if fam == "fast" else d.between(1, 0xFE)
            body = b"" if fam == "fast" or d.below(2) else d.bytes(1)
            p = AL.pack(standard, bytes([t & (0x7F if standard == AL.JCLIP else 0xFF), len(body)]) + body)
            bits += _bytes_bits(p, 1 if fam == "fast" else sb)
        runs = _fast_runs(bits, first) if fam == "fast" else _nominal_runs(bits)
        return np.concatenate([R.runs_line(standard, runs), z(100)])
    if fam == "drift":
        # a sender whose baud is off by up to 4 % either way
        bits = []
        for _ in range(3):
            g, _p = _good(d, standard, d.between(20, 90))
            bits += g
        return np.concatenate([z(d.below(200)), R.runs_line(standard, _nominal_runs(bits, 1000 + d.between(-40, 40))), z(200)])
    if fam == "carrier_drop":
        g, p = _good(d, standard, 60)
        cut = d.between(60*20//3 + 30, len(g)*20//3 - 30)
        x = R.runs_line(standard, _nominal_runs(g))
        g2, _p = _good(d, standard, d.between(12, 80))
        return np.concatenate([x[:cut], z(d.between(40, 600)), R.runs_line(standard, _nominal_runs(g2 + g)), z(200)])
    assert fam == "any_int16"
    return (Lcg(seeds_of(i + 1, seed, salt=2)[i:i + 1]).u16(24576)[0] - 32768).astype(np.int16)


def rx_schedule(n, calls=RX_CALLS, seed=SEED):
    """lens[calls][n]: an eighth 0, a quarter 1 .. 16, the rest 1 .. 1 024, every line on draws of its own"""
    v = Lcg(seeds_of(n, seed, salt=3)).u16(2*calls).reshape(n, calls, 2)
    kind = v[:, :, 0] % 8
    lens = np.where(kind == 0, 0, np.where(kind <= 2, 1 + v[:, :, 1] % 16, 1 + v[:, :, 1] % 1024))
    return np.ascontiguousarray(lens.T.astype(np.int32))


_rx_cache = {}


def rx_lines(n=N_GPU, seed=SEED, ticks=False):
    """(rows [n][total] int16, lens [calls][n]): every line's content, padded with silence or cut to what its calls take"""
    key = (n, seed, ticks)
    if key not in _rx_cache:
        if len(_rx_cache) > 3:
            _rx_cache.clear()
        lens = np.full((RX_TICKS, n), TICK, np.int32) if ticks else rx_schedule(n, seed=seed)
        total = lens.sum(axis=0)
        rows = np.zeros((n, int(total.max())), np.int16)
        for i in range(n):
            x = rx_line(i, seed)[:total[i]]
            rows[i, :len(x)] = x
        _rx_cache[key] = (rows, lens)
    return _rx_cache[key]


def left_out(lens):
    """the largest share of lines that any call leaves out"""
    return float((np.asarray(lens) == 0).mean(axis=1).max())


def sweep_rx(n=N_GPU, seed=SEED, ticks=False, bits=False):
    """the receiver sweep and what the reference makes of it: per line run_rx()'s dict"""
    R = _ref()
    rows, lens = rx_lines(n, seed, ticks)
    return {"seed": seed, "rows": rows, "lens": lens, "ref": [R.run_rx(standard_of(i), rows[i], lens[:, i], bits=bits) for i in range(n)]}


def old_capacity(samples):
    """spangpu_adsi_rx_msg_capacity() as it was: a sender's bit length"""
    return np.asarray(samples)*1200//240000 + 1


def capacity(samples):
    """spangpu_adsi_rx_msg_capacity(): no two bits closer than the 4 samples from 50 % to 100 % of the bit clock"""
    return np.asarray(samples)//120 + 1


def coverage_rx(r):
    """what the receiver lines reach, from the reference's outputs alone"""
    n = len(r["ref"])
    lens = r["lens"]
    c = {"delivered": {s: 0 for s in STANDARDS}, "framing_error_lines": 0, "len_256_lines": 0, "multi_calls": 0, "over_old_capacity": 0,
         "fast_reach": {}, "most": 0, "marks": {}, "bad_check": {False: 0, True: 0}}
    fam = family_of(np.arange(n))
    for i, q in enumerate(r["ref"]):
        c["delivered"][standard_of(i)] += len(q["msgs"])
        c["framing_error_lines"] += int(q["words"][-1, ADR_FRAMING_ERRORS] > 0)
        c["len_256_lines"] += int((q["words"][:, ADR_MSG_LEN] == 256).any())
        c["multi_calls"] += int((q["counts"] >= 2).sum())
        c["most"] = max(c["most"], int(q["counts"].max()))
        over = q["counts"] > old_capacity(lens[:, i])
        c["over_old_capacity"] += int(over.sum())
        assert (q["counts"] <= capacity(lens[:, i])).all(), (i, "a call of the reference's above the derived capacity")
        kind, marks = META.get((r["seed"], i), ("", 0))
        if marks:
            # both messages arrive behind 9 or 10 marks in mid-message; 11 or 12 restart the first, and only the second does
            c["marks"].setdefault((marks, len(q["msgs"])), 0)
            c["marks"][(marks, len(q["msgs"]))] += 1
        if kind == "check":
            # a sum (CRC, on a J-CLIP line) one bit off: that message is not delivered, the good one behind it is
            c["bad_check"][standard_of(i) == AL.JCLIP] += int(len(q["msgs"]) == 1)
        if FAMILIES[fam[i]] == "fast":
            for k in np.nonzero(q["counts"])[0]:
                cap = int(capacity(lens[k, i]))
                c["fast_reach"][cap] = max(c["fast_reach"].get(cap, 0), int(q["counts"][k]))
    return c


# ---- sender lines ---------------------------------------------------------------------------------------------------------

def tx_schedule(calls=TX_CALLS, seed=SEED):
    """the call lengths, common to the bank: 1 .. 400, every residue modulo 8 among the running sums"""
    v = Lcg(seeds_of(1, seed, salt=4)).u16(calls)[0]
    return (1 + v % 400).astype(np.int32)


def tx_script(i, seed=SEED, calls=TX_CALLS):
    """(ops [(call, operation, a0 .. a3)], opbytes, messages): line i's script; a put's a0 / a1 are filled in here"""
    standard = standard_of(i)
    d = Draws(int(seeds_of(i + 1, seed, salt=5)[i]), 4096)
    events = []
    style = i//4 % 6
    # short preambles keep a message to a few calls, so that busy, refused and taken puts all come up in 60 calls
    if style != 0:
        events.append((0, OP_PREAMBLE, (d.below(30), d.between(0, 25), d.below(8), d.between(0, 3))))
    for _ in range(d.between(4, 9)):
        kind = ("fields", "fields", "none", "empty", "sixteen", "dle", "longest", "over", "over")[d.below(9)]
        if kind == "longest" and d.below(3):
            kind = "fields"
        events.append((d.below(calls), OP_PUT, message(d, standard, kind)))
    for _ in range(d.between(1, 3)):
        # negative, zero and positive in every place
        a = tuple((-1, 0, d.between(1, 40))[d.below(3)] for _ in range(4))
        events.append((d.below(calls), OP_PREAMBLE, (a[0], a[1], a[2] if a[2] < 13 else a[2] % 13, a[3] if a[3] < 6 else a[3] % 6)))
    k = d.below(calls)
    events.append((k, OP_ALERT, None))
    if style in (1, 4):
        events.append((min(k + d.below(3), calls - 1), OP_ALERT, None))         # twice in a row
    if style in (2, 4, 5):
        # in mid-message: a put and the tone two calls on
        k = d.below(calls - 4)
        events.append((k, OP_PUT, message(d, standard, "fields")))
        events.append((k + 2, OP_ALERT, None))
    if style == 3:
        events.append((d.below(calls), OP_RESTART, None))
    if style in (0, 2):
        # The modulator's shutdown flag set by hand while the signal may be on, which no call of the reference's leads to
        # and a bank's set_state allows: the only way to a call that gets nothing out of the modulator without the bit
        # source having turned the signal off itself (adsi.c:542-543).
        events.append((d.below(calls), OP_SHUT_DOWN, None))
    events.sort(key=lambda e: e[0])         # (stable: the order within a call stays as drawn)
    ops, blob, msgs = [], b"", []
    full = False
    for call, op, arg in events:
        # Behind a message that fills msg[] (255 bytes and the sum) byte_no is left at 256, and a preamble grown over bit_no
        # without a put in between makes the reference send msg[256], which is not there (profiles/adsi_sweep.md): the bank
        # sends msg[0].  No script changes the preamble behind such a put.
        full = full or (op == OP_PUT and len(arg) == 255)
        if full and op == OP_PREAMBLE:
            continue
        if op == OP_PUT:
            ops.append((call, op, len(blob), len(arg), 0, 0))
            blob += arg
            msgs.append(arg)
        elif op == OP_PREAMBLE:
            ops.append((call, op) + tuple(arg))
        else:
            ops.append((call, op, 0, 0, 0, 0))
    return ops, blob, msgs


def sweep_tx(n=N_GPU, seed=SEED, calls=TX_CALLS, ref=True):
    R = _ref()
    lens = tx_schedule(calls, seed)
    out = {"lens": lens, "scripts": [tx_script(i, seed, calls) for i in range(n)]}
    if ref:
        out["ref"] = [R.run_tx(standard_of(i), s[0], s[1], lens) for i, s in enumerate(out["scripts"])]
    return out


def coverage_tx(r):
    """what the sender lines reach, from the reference's outputs alone"""
    lens = r["lens"]
    c = {"put": {0: 0, -1: 0, 1: 0}, "refused_restarts": 0, "part_tone_part_modem": 0, "tone_ends_mod_8": set(), "tone_in_message": 0,
         "off_on_empty_call": 0, "off_by_the_rule_alone": 0, "restarts": 0, "preamble_signs": set()}
    for (ops, _, _), (pcm, out_lens, results, words, msg) in zip(r["scripts"], r["ref"]):
        for o, res in zip(ops, results):
            k = o[0]
            before = words[k - 1] if k else None
            if o[1] == OP_PUT:
                c["put"][int(np.sign(res))] += 1
                # a put that is refused after start_tx() has restarted the modulator: the signal was off, and is on behind it
                if res < 0 and before is not None and before[ADT_TX_SIGNAL_ON] == 0 and before[ADT_MSG_LEN] == 0:
                    c["refused_restarts"] += 1
            elif o[1] == OP_ALERT and before is not None and before[ADT_MSG_LEN] > 0 and before[ADT_TX_SIGNAL_ON]:
                c["tone_in_message"] += 1
            elif o[1] == OP_RESTART:
                c["restarts"] += 1
            elif o[1] == OP_SHUT_DOWN and before is not None and before[ADT_TX_SIGNAL_ON] and not words[k][ADT_TX_SIGNAL_ON]:
                # the signal was on, the modulator gave nothing, and nobody asked the bit source
                c["off_by_the_rule_alone"] += int((words[k][5:9] == before[5:9]).all())
            elif o[1] == OP_PREAMBLE:
                c["preamble_signs"] |= {(j, int(np.sign(a))) for j, a in enumerate(o[2:])}
        sec = words[:, ADT_TONE_SECTION]
        pos = words[:, ADT_TONE_SECTION + 1]
        for k in range(1, len(lens)):
            if sec[k - 1] >= 0 and sec[k] < 0:
                # the tone ended in call k, at this offset of its row
                at = (880 - int(pos[k - 1]) + 480) if sec[k - 1] == 0 else (480 - int(pos[k - 1]))
                c["tone_ends_mod_8"].add(at % 8)
                if 0 < at < lens[k] and out_lens[k] > at:
                    c["part_tone_part_modem"] += 1
            # the signal turned off by a call that got nothing out of the modulator
            if words[k - 1][ADT_TX_SIGNAL_ON] and not words[k][ADT_TX_SIGNAL_ON] and out_lens[k] == 0:
                c["off_on_empty_call"] += 1
    return c


# ---- the sweep as a file for tests/c_callers/adsi_frame_host.cpp ---------------------------------------------------------------

def write_sweep(path, rx=None, tx=None):
    """receiver lines (standard, calls, samples; lens; samples) and sender lines (standard, calls, ops, bytes; lens in bits; ops;
    the messages as put; per put the packed length or -1 and 256 packed bytes)"""
    E = _engine()
    with open(path, "wb") as f:
        n_rx = 0 if rx is None else rx[0].shape[0]
        n_tx = 0 if tx is None else len(tx["scripts"])
        np.array([0x41445349, n_rx, n_tx], np.int32).tofile(f)
        for i in range(n_rx):
            rows, lens = rx
            total = int(lens[:, i].sum())
            np.array([standard_of(i), lens.shape[0], total], np.int32).tofile(f)
            np.ascontiguousarray(lens[:, i], np.int32).tofile(f)
            np.ascontiguousarray(rows[i, :total], np.int16).tofile(f)
        for i in range(n_tx):
            ops, blob, msgs = tx["scripts"][i]
            np.array([standard_of(i), len(tx["lens"]), len(ops), len(blob), len(msgs)], np.int32).tofile(f)
            np.ascontiguousarray(tx["lens"], np.int32).tofile(f)
            np.array(ops, np.int32).reshape(-1, 6).tofile(f)
            np.frombuffer(blob + b"\0", np.uint8).tofile(f)
            for m in msgs:
                p = E.adsi_pack_message(standard_of(i), m)
                np.array([-1 if p == -1 else len(p)], np.int32).tofile(f)
                np.frombuffer((b"" if p == -1 else p).ljust(256, b"\0"), np.uint8).tofile(f)
    return n_rx + n_tx
