"""The lines of the caller-ID receiver tests, defined once: tests/golden/make_golden_adsi.py feeds them to the reference's
adsi_rx and keeps what it delivered; tests/test_adsi_gpu.py builds the same samples again at test time (the reference's
fsk_tx through fsktx_ref.RefFskTx with a Python get_bit, and the reference's awgn through oracle/ref.py) and feeds them to
the bank.  Nothing here comes from adsi.c: packing, framing and the CRC are restated in Python, and the generator asserts
that they agree with the reference before it relies on them."""
import numpy as np

import fsktx_ref

CLASS, CLIP, ACLIP, JCLIP = 1, 2, 3, 4
STANDARDS = (CLASS, CLIP, ACLIP, JCLIP)
NAMES = {CLASS: "class", CLIP: "clip", ACLIP: "aclip", JCLIP: "jclip"}
PRESET = {CLASS: 6, CLIP: 2, ACLIP: 2, JCLIP: 2}        # preset_fsk_specs[]: Bell 202, V.23 channel 1
DLE, SOH, STX, ETX = 0x10, 0x01, 0x02, 0x03
TICK = 160
ATTENUATIONS = (0, 10, 20, 30)          # dB below the presets' -14 dBm0
SNRS = (None, 30, 20, 14)               # dB; None = no noise
AUDIBLE = (0, 10)                       # the attenuations above the presets' -30 dBm0 carrier threshold


def crc16(data, crc=0):
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ 0x8408 if crc & 1 else crc >> 1
    return crc


def add_field(standard, msg, field_type, body=b""):
    """adsi_add_field() for the four FSK standards, on bytes"""
    if not msg:
        return bytes([field_type, 0])
    out = bytearray(msg)
    if standard == JCLIP:
        for b in (field_type, len(body)) + tuple(body):
            out.append(b)
            if b == DLE:
                out.append(b)
        return bytes(out)
    if field_type:
        out += bytes([field_type, len(body)])
        if len(body) == DLE:
            out.append(len(body))
    return bytes(out + body)


def pack(standard, msg):
    """What adsi_tx_put_message() leaves in msg[]"""
    n = len(msg)
    if standard == JCLIP:
        out = [DLE, SOH, 0x07, DLE, STX, msg[0], (n - 2) & 0xFF]
        if n - 2 == DLE:
            out.append(DLE)
        out += list(msg[2:]) + [DLE, ETX]
        out = [(b & 0x7F) | ((bin(b & 0x7F).count("1") & 1) << 7) for b in out]
        crc = crc16(out[2:])
        return bytes(out + [crc & 0xFF, crc >> 8])
    out = bytearray(msg)
    out[1] = (n - 2) & 0xFF
    out.append(-sum(out) & 0xFF)
    return bytes(out)


def defaults(standard):
    """preamble_len, preamble_ones_len, postamble_ones_len, stop_bits"""
    return (0, 75, 5, 4) if standard == JCLIP else (300, 80, 5, 1)


def byte_bits(b, stop_bits=1, stop=1):
    return [0] + [(b >> i) & 1 for i in range(8)] + [stop] + [1]*(stop_bits - 1)


def burst_bits(packed, preamble):
    """The bits adsi_tx_get_bit() hands out for one message, up to SIG_STATUS_END_OF_DATA"""
    pre, ones, post, stop_bits = preamble
    bits = [i & 1 for i in range(pre)] + [1]*ones
    for b in packed:
        bits += byte_bits(b, max(stop_bits, 1))
    return bits + [1]*post


def render(standard, bits, tail=0):
    """bits through the reference's fsk_tx, then end of data; `tail` samples of silence behind"""
    feed = fsktx_ref.BitFeed()
    feed.bits = list(bits)
    feed.end_of_data = True
    tx = fsktx_ref.RefFskTx(PRESET[standard], get_bit=feed)
    n = len(bits)*7 + 16
    row, got = tx.tx(n)
    assert got < n
    return np.concatenate([row[:got], np.zeros(tail, np.int16)])


def impair(samples, att_db, snr_db, seed):
    """attenuation, then the reference's AWGN at the attenuated signal's level less snr_db"""
    from oracle import ref
    x = np.round(samples.astype(np.float64)*10.0**(-att_db/20.0))
    if snr_db is not None:
        x = x + ref.awgn(seed, -14.0 - att_db - snr_db, len(samples)).astype(np.float64)
    return np.clip(x, -32768, 32767).astype(np.int16)


def number_message(standard, number, name=b""):
    """A multiple data message with a date, a number and, where given, a name"""
    mtype = {CLASS: 0x80, CLIP: 0x80, ACLIP: 0x80, JCLIP: 0x40}[standard]
    msg = add_field(standard, b"", mtype)
    if standard != JCLIP:
        msg = add_field(standard, msg, 0x01, b"10181530")
    msg = add_field(standard, msg, 0x02, number)
    if name:
        msg = add_field(standard, msg, 0x07 if standard != JCLIP else 0x09, name)
    return msg


# the messages of the sender and packing cases, per standard: (fields as (type, body)) -- built with the add_field under test
FIELD_CASES = {
    "cid": lambda s: [(0x40 if s == JCLIP else 0x80, b""), (0x02, b"0123456789"), (0x07 if s != JCLIP else 0x09, b"Caller ID")],
    "dle": lambda s: [(0x40 if s == JCLIP else 0x80, b""), (0x02, b"12345678901234")],          # J-CLIP: 2 + 14 = 16 = DLE body bytes
    "dle_body": lambda s: [(0x40 if s == JCLIP else 0x80, b""), (DLE, bytes([DLE, 0x31, DLE])), (0x02, b"5" * DLE)],
    "sdmf": lambda s: [(0x04, b""), (0x00, b"101815305551212")],
}


def build(standard, fields, add=add_field):
    msg = b""
    for t, body in fields:
        msg = add(standard, msg, t, body)
    return msg


def sweep_message(standard):
    return build(standard, FIELD_CASES["cid"](standard))


def sweep_lines():
    """(name, standard, samples): the (a) sweep, 4 standards x 4 attenuations x 4 SNRs"""
    out = []
    for s in STANDARDS:
        clean = render(s, burst_bits(pack(s, sweep_message(s)), defaults(s)), tail=3*TICK)
        clean = np.concatenate([np.zeros(TICK, np.int16), clean])
        for a, att in enumerate(ATTENUATIONS):
            for k, snr in enumerate(SNRS):
                out.append(("%s_a%d_s%s" % (NAMES[s], att, snr), s, impair(clean, att, snr, 1000 + 100*s + 10*a + k)))
    return _same_length(out)


def _same_length(lines, tick=TICK):
    """every line zero-filled to the longest, in whole calls: channels of one bank run the same number of calls"""
    n = max(len(ln[2]) for ln in lines if len(ln) < 4 or ln[3] == tick)
    n = -(-n//tick)*tick
    return [ln[:2] + (np.concatenate([ln[2], np.zeros(n - len(ln[2]), np.int16)]),) + ln[3:] if len(ln) < 4 or ln[3] == tick else ln for ln in lines]


def _framed(byte_list, lead=40, gap=None, tail=30):
    bits = [1]*lead
    for i, b in enumerate(byte_list):
        bits += byte_bits(b)
        if gap and i in gap:
            bits += [1]*gap[i]
    return bits + [1]*tail


def hand_lines():
    """(name, standard, samples, tick): the (b) lines, every one framed by hand"""
    out = []
    good = pack(CLASS, number_message(CLASS, b"5551212"))
    good2 = pack(CLIP, number_message(CLIP, b"0044123"))
    jgood = pack(JCLIP, number_message(JCLIP, b"0312345678"))

    def add(name, standard, bits, tick=TICK, tail=2*TICK, head=0):
        out.append((name, standard, np.concatenate([np.zeros(head, np.int16), render(standard, bits, tail=tail)]), tick))

    bad = bytearray(good)
    bad[-1] ^= 0x01
    add("bad_sum", CLASS, _framed(bad))
    bad = bytearray(jgood)
    bad[-1] ^= 0x40
    add("bad_crc", JCLIP, _framed(bad))
    add("jclip_not_dle_first", JCLIP, _framed(b"\x41" + jgood))
    bits = [1]*40
    for i, b in enumerate(good):
        bits += byte_bits(b, stop=0 if i == 4 else 1)
    add("stop_bit_0", CLASS, bits + [1]*30)
    add("marks_11_restart", CLIP, _framed(b"\x80\x05" + good2, gap={1: 11}))
    add("marks_10_no_restart", CLIP, _framed(b"\x80\x05" + good2, gap={1: 10}))
    add("length_0", CLASS, _framed(pack(CLASS, b"\x04\x00")))
    add("length_252", ACLIP, _framed(pack(ACLIP, bytes([0x80, 0]) + bytes((7*i + 1) & 0xFF for i in range(252)))))
    over = bytearray(bytes([0x80, 254]) + bytes((5*i + 3) & 0xFF for i in range(258)))
    add("length_past_256", CLIP, _framed(over))
    short_a = pack(CLASS, b"\x04\x00")
    short_b = pack(CLASS, b"\x06\x00\x42")
    # 1024 samples of marks, then both messages inside the second 1024-sample call
    add("two_in_one_call", CLASS, [1]*154 + _framed(short_a, lead=2, tail=2) + _framed(short_b, lead=0, tail=30), tick=1024, tail=1024)
    half = render(CLIP, _framed(good2[:6], tail=0))
    whole = render(CLIP, _framed(good2), tail=2*TICK)
    out.append(("carrier_drop", CLIP, np.concatenate([half, np.zeros(400, np.int16), whole]), TICK))
    return _same_length(out)


def calls_of(samples, tick):
    """the line cut into calls of `tick` samples, the last one zero-filled"""
    n = -(-len(samples)//tick)
    rows = np.zeros((n, tick), np.int16)
    rows.reshape(-1)[:len(samples)] = samples
    return rows
