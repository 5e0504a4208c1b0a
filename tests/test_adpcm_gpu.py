"""The IMA and OKI ADPCM codec banks on the GPU, for equality with what the reference's ima_adpcm.c and oki_adpcm.c produced
(tests/golden/ima_adpcm.npz, oki_adpcm.npz, written by tests/golden/make_golden_adpcm.py): outputs, counts and state words
call for call on the line and the random-code lines, per-channel lengths (0 among them), host and device rows, strides,
restart and state moved between channels; 1 024 generated lines a family through the bank and through the host-compiled
step functions (the same source: that proves the kernel's plumbing at mixed configurations; the algorithm is pinned by the
fixtures and by the CPU sweep); and a device-resident chain of 256 lines in front of a DTMF receiver bank.  Everything is
integer arithmetic, or binary32 sums in a fixed order: every comparison is equality.

The base shape is 136 channels: two full waves and a partial one; channel c runs configuration c mod K, so every wave holds
every variant and both chunk_size kinds, or both rates."""
import numpy as np
import pytest

import adpcm_lines as AL
from spandsp_amd import engine
from test_g726_gpu import DevBytes

pytestmark = pytest.mark.gpu

N = 136
PROBE = (0, 1, 63, 64, 135)         # the channels whose state words are read back after every call


@pytest.fixture(scope="module")
def cases():
    return {f: {(c.kind, c.a, c.b, c.tag): c for c in AL.cases(AL.load(f))} for f in (AL.IMA, AL.OKI)}


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    # (no sanitizer here: that build belongs to the CPU suite)
    return AL.build_host_program(str(tmp_path_factory.mktemp("adpcm_host")), sanitize=False)


def bank_of(family, configs, n=N):
    a, b = zip(*configs)
    return engine.ImaAdpcmBank(n, a, b) if family == AL.IMA else engine.OkiAdpcmBank(n, a)


def run_cases(bank, kind, chans, probe=PROBE, all_words_at_end=True):
    """Every channel of `bank` through its case (chans[c]), call for call with per-channel lengths (a channel past its last
    call brings 0); each call's outputs, counts and, on the probe channels, state words against the case."""
    n = bank.n
    lens_of = [[k[0] for k in chans[c].calls] for c in range(n)]
    at = [0]*n
    got = [0]*n
    ticks = max(len(x) for x in lens_of)
    most = max(max(x) for x in lens_of)
    saw_zero = False
    for k in range(ticks):
        lens = np.array([x[k] if k < len(x) else 0 for x in lens_of], np.int32)
        saw_zero |= bool((lens == 0).any())
        rows = np.zeros((n, most), np.int16 if kind == AL.ENCODE else np.uint8)
        for c in range(n):
            rows[c, :lens[c]] = chans[c].data[at[c]:at[c] + lens[c]]
        out, counts = bank.encode_host(rows, most, lens) if kind == AL.ENCODE else bank.decode_host(rows, most, lens)
        for c in range(n):
            case = chans[c]
            want_count = case.calls[k][1] if k < len(case.calls) else 0
            assert counts[c] == want_count, (case.name, c, k, counts[c], want_count)
            want = np.asarray(case.want)[got[c]:got[c] + want_count]
            assert np.array_equal(out[c, :want_count], want), (case.name, c, k, np.flatnonzero(out[c, :want_count] != want)[:4])
            at[c] += int(lens[c])
            got[c] += want_count
        for c in probe:
            if c < n:
                # (a channel past its last call sits the tick out: its words are still those of its last call)
                j = min(k, len(chans[c].calls) - 1)
                assert np.array_equal(bank.get_state(c), chans[c].calls[j][2]), (chans[c].name, c, k)
    for c in range(n):
        assert at[c] == len(chans[c].data) and got[c] == len(chans[c].want), (chans[c].name, c)
        if all_words_at_end:
            assert np.array_equal(bank.get_state(c), chans[c].calls[-1][2]), (chans[c].name, c)
    return saw_zero


@pytest.mark.parametrize("family,kind,tag", [(f, k, t) for f in (AL.IMA, AL.OKI) for k, t in ((AL.ENCODE, "line"), (AL.DECODE, "line"), (AL.DECODE, "rnd"))])
def test_fixture_parity(built, cases, family, kind, tag):
    configs = AL.CONFIGS[family]
    bank = bank_of(family, configs)
    chans = [cases[family][(kind,) + configs[c % len(configs)] + (tag,)] for c in range(N)]
    saw_zero = run_cases(bank, kind, chans)
    # the decoders' calls are the packets of their encoders, which differ in number: some channels sat calls out
    assert saw_zero or kind == AL.ENCODE or family == AL.OKI


def test_a_decoder_that_begins_at_phase_1(built, cases):
    """the entry phase no call leaves behind (tests/adpcm_lines.py coverage_oki()): put there by set_state"""
    case = cases[AL.OKI][(AL.DECODE, 24000, 0, "phase1")]
    bank = bank_of(AL.OKI, [(32000, 0), (24000, 0)], 66)
    for c in (1, 65):
        w = bank.get_state(c)
        w[AL.W_OKI["phase"]] = 1
        bank.set_state(c, w)
    rows = np.zeros((66, len(case.data)), np.uint8)
    lens = np.zeros(66, np.int32)
    for c in (1, 65):
        rows[c] = case.data
        lens[c] = len(case.data)
    out, counts = bank.decode_host(rows, len(case.data), lens)
    for c in (1, 65):
        assert counts[c] == len(case.want) and np.array_equal(out[c, :counts[c]], case.want)
        assert np.array_equal(bank.get_state(c), case.calls[-1][2])
    assert not counts[[0, 2, 64]].any()


@pytest.mark.parametrize("family", [AL.IMA, AL.OKI])
def test_strides_and_device_rows(built, family):
    configs = AL.CONFIGS[family]
    n = 160
    line = AL.line()
    rows = np.zeros((N, n), np.int16)
    for c in range(N):
        rows[c] = line[200 + c:200 + c + n]
    ref_codes, ref_counts = bank_of(family, configs).encode_host(rows, n)
    ref_pcm, ref_samples = bank_of(family, configs).decode_host(ref_codes, ref_codes.shape[1], ref_counts)
    assert ref_counts.min() > 0 and ref_samples.min() > 0 and len(set(ref_counts.tolist())) > 1
    # host rows wider than the call
    wide = np.full((N, n + 37), 0x5A5A, np.int16)
    wide[:, :n] = rows
    codes, counts = bank_of(family, configs).encode_host(wide, n)
    assert np.array_equal(counts, ref_counts)
    for c in range(N):
        assert np.array_equal(codes[c, :counts[c]], ref_codes[c, :counts[c]]), c
    # device rows wider than the call: strides of 512, 256 and 2048 bytes
    L = engine.lib()
    enc, dec = bank_of(family, configs), bank_of(family, configs)
    cap = enc.encode_capacity(n)
    assert dec.decode_capacity(cap)*2 <= 2048
    pcm, mid, back = DevBytes(N*512), DevBytes(N*256), DevBytes(N*2048)
    try:
        padded = np.zeros((N, 256), np.int16)
        padded[:, :n] = rows
        pcm.put(padded)
        counts = enc.encode_device(pcm.ptr, 512, n, mid.ptr, 256, counts=True)
        got = mid.get((N, 256))
        assert np.array_equal(counts, ref_counts)
        for c in range(N):
            assert np.array_equal(got[c, :counts[c]], ref_codes[c, :counts[c]]), c
            # nothing past the 16-byte boundary behind a row's count
            assert not got[c, (counts[c] + 15) & ~15:].any(), c
        samples = dec.decode_device(mid.ptr, 256, cap, back.ptr, 2048, lens=counts, counts=True)
        amp = back.get((N, 1024), np.int16)
        assert np.array_equal(samples, ref_samples)
        for c in range(N):
            assert np.array_equal(amp[c, :samples[c]], ref_pcm[c, :samples[c]]), c
            assert not amp[c, (samples[c] + 7) & ~7:].any(), c
        for c in PROBE:
            fresh_e, fresh_d = bank_of(family, configs, c + 1), bank_of(family, configs, c + 1)
            one, k1 = fresh_e.encode_host(rows[:c + 1], n)
            fresh_d.decode_host(one, one.shape[1], k1)
            assert np.array_equal(enc.get_state(c), fresh_e.get_state(c)) and np.array_equal(dec.get_state(c), fresh_d.get_state(c)), c
        words = enc.get_state(7)
        # refused: a stride that is no multiple of 16, a base that is not, a stride shorter than the row rounded up to 16
        BAD = -2
        f = getattr(L, "spangpu_%s_encode" % AL.NAMES[family])
        g = getattr(L, "spangpu_%s_decode" % AL.NAMES[family])
        args = (None, n, mid.ptr, engine.MEM_DEVICE, 256, None)
        assert f(enc.h, pcm.ptr, engine.MEM_DEVICE, 328, *args) == BAD
        assert f(enc.h, pcm.ptr.value + 8, engine.MEM_DEVICE, 512, *args) == BAD
        assert f(enc.h, pcm.ptr, engine.MEM_DEVICE, 304, *args) == BAD
        assert f(enc.h, pcm.ptr, engine.MEM_DEVICE, 512, None, n, mid.ptr, engine.MEM_DEVICE, 64, None) == BAD
        assert f(enc.h, pcm.ptr, engine.MEM_DEVICE, 512, None, n, mid.ptr.value + 4, engine.MEM_DEVICE, 256, None) == BAD
        assert g(dec.h, mid.ptr, engine.MEM_DEVICE, 250, None, cap, back.ptr, engine.MEM_DEVICE, 2048, None) == BAD
        assert g(dec.h, mid.ptr, engine.MEM_DEVICE, 256, None, cap, back.ptr, engine.MEM_DEVICE, 256, None) == BAD
        # a host stride shorter than the row, a bad memory kind, a length past 2^24
        spare = np.zeros((N, 256), np.uint8)
        assert f(enc.h, rows.ctypes.data, engine.MEM_HOST, 2*n - 1, None, n, spare.ctypes.data, engine.MEM_HOST, 256, None) == BAD
        assert f(enc.h, rows.ctypes.data, 7, 2*n, None, n, spare.ctypes.data, engine.MEM_HOST, 256, None) == BAD
        assert f(enc.h, rows.ctypes.data, engine.MEM_HOST, 2*n, None, n, spare.ctypes.data, engine.MEM_HOST, cap - 1, None) == BAD
        assert f(enc.h, rows.ctypes.data, engine.MEM_HOST, 2*n, None, (1 << 24) + 1, spare.ctypes.data, engine.MEM_HOST, 256, None) == BAD
        # a refused call changes nothing
        assert np.array_equal(enc.get_state(7), words)
    finally:
        for d in (pcm, mid, back):
            d.free()
    # the capacities: the worst channel of the bank, and of banks of one kind
    if family == AL.IMA:
        assert enc.encode_capacity(160) == 164 and enc.decode_capacity(84) == 4*84 and enc.encode_capacity(0) == 0
        assert bank_of(family, [(AL.DVI4, 0)], 8).encode_capacity(160) == 84 and bank_of(family, [(AL.DVI4, 0)], 8).decode_capacity(84) == 160
        assert bank_of(family, [(AL.IMA4, 0)], 8).encode_capacity(161) == 84 and bank_of(family, [(AL.IMA4, 0)], 8).decode_capacity(84) == 161
        assert bank_of(family, [(AL.IMA4, 5)], 8).encode_capacity(161) == 81 and bank_of(family, [(AL.VDVI, 9)], 8).decode_capacity(3) == 12
    else:
        assert enc.encode_capacity(160) == 80 and enc.decode_capacity(60) == 160 and enc.decode_capacity(0) == 0
        assert bank_of(family, [(24000, 0)], 8).encode_capacity(160) == 60 and bank_of(family, [(32000, 0)], 8).decode_capacity(80) == 160
        assert bank_of(family, [(24000, 0)], 8).decode_capacity(1) == 3 and bank_of(family, [(32000, 0)], 8).encode_capacity(161) == 81


@pytest.mark.parametrize("family,cfg", [(AL.IMA, (AL.DVI4, AL.CHUNK)), (AL.IMA, (AL.IMA4, AL.CHUNK)), (AL.OKI, (32000, 0)), (AL.OKI, (24000, 0))])
def test_restart_and_state_moved_between_channels(built, cases, family, cfg):
    """a stream that may be cut anywhere: 161 samples on channel 0 (an odd nibble stays behind), the rest of 248 on channel 5,
    which was another codec until then"""
    other = {(AL.DVI4, AL.CHUNK): (AL.VDVI, 0), (AL.IMA4, AL.CHUNK): (AL.DVI4, 0), (32000, 0): (24000, 0), (24000, 0): (32000, 0)}[cfg]
    case = cases[family][(AL.ENCODE,) + cfg + ("line",)]
    assert case.recut
    bank = bank_of(family, [cfg, other], 6)
    data = np.asarray(case.data, np.int16)[250:]            # (the loud part of the line)
    alone = np.zeros((1, 248), np.int16)
    alone[0] = data[:248]
    whole, total = bank_of(family, [cfg], 1).encode_host(alone, 248)
    whole = whole[0, :total[0]]

    def feed(start, n, chans):
        rows = np.zeros((6, n), np.int16)
        lens = np.zeros(6, np.int32)
        for c in chans:
            rows[c] = data[start:start + n]
            lens[c] = n
        return bank.encode_host(rows, n, lens)

    out, counts = feed(0, 161, (0, 2))
    first = int(counts[0])
    assert first > 0 and counts[2] == first and np.array_equal(out[0, :first], whole[:first]) and np.array_equal(out[2, :first], whole[:first])
    w = bank.get_state(0)
    parity = w[AL.W_IMA["bits"]] if family == AL.IMA else w[AL.W_OKI["mark"]]
    assert parity & 1
    bank.set_state(5, w)
    bank.restart(2, *cfg[:2 if family == AL.IMA else 1])
    assert np.array_equal(bank.get_state(2), bank.get_state(4))
    out, counts = feed(161, 87, (5,))
    assert first + counts[5] == len(whole) and np.array_equal(out[5, :counts[5]], whole[first:])
    assert not counts[[0, 1, 2, 3, 4]].any()
    out, counts = feed(0, 161, (2, 4))
    assert np.array_equal(out[2, :first], whole[:first]) and np.array_equal(out[4, :first], whole[:first])
    assert np.array_equal(bank.get_state(2), w) and np.array_equal(bank.get_state(4), w)
    # what set_state and restart refuse: words no call could have left
    names = AL.W_IMA if family == AL.IMA else AL.W_OKI
    for field, value in ((("step_index", 89), ("step_index", -1), ("last", 40000), ("variant", 3)) if family == AL.IMA else
                         (("step_index", 49), ("phase", 4), ("ptr", 32), ("bit_rate", 16000), ("last", 2048), ("history[31]", 70000))):
        bad = w.copy()
        bad[names[field]] = value
        with pytest.raises(engine.SpanGpuError):
            bank.set_state(1, bad)
    with pytest.raises(engine.SpanGpuError):
        if family == AL.IMA:
            bank.restart(1, 3, 0)
        else:
            bank.restart(1, 8000)
    assert np.array_equal(bank.get_state(4), w)


@pytest.mark.parametrize("family", [AL.IMA, AL.OKI])
def test_generated_lines_through_the_bank_and_the_host_functions(built, host_program, tmp_path, family):
    """1 024 lines, a configuration and a cut into calls of its own each: the bank against csrc/adpcm_dev.hpp compiled for the
    host, encoders and then the decoders of what they made."""
    n = 1024
    inputs = AL.generated_inputs(family, n, 0x6A00 + family, longest=300)
    enc_cases = AL.host_cases(host_program, str(tmp_path), [(family, AL.ENCODE, a, b, amp, lens) for a, b, amp, lens in inputs])
    dec_cases = AL.host_cases(host_program, str(tmp_path), [(family, AL.DECODE, c.a, c.b, c.want, [k[1] for k in c.calls]) for c in enc_cases])
    assert {(a, bool(b)) for a, b, _, _ in inputs} == {(a, bool(b)) for a, b in AL.CONFIGS[family]}
    configs = [(a, b) for a, b, _, _ in inputs]
    run_cases(bank_of(family, configs, n), AL.ENCODE, enc_cases, probe=())
    run_cases(bank_of(family, configs, n), AL.DECODE, dec_cases, probe=())


@pytest.mark.parametrize("family", [AL.IMA, AL.OKI])
def test_device_resident_chain(built, host_program, tmp_path, family):
    """DTMF sender bank -> encode -> decode -> DTMF receiver bank at 256 lines (DVI4 with a header per tick, as RTP carries it; OKI
    at 32 kbit/s), every hop in device memory.  The digits must equal those the same receiver configuration reports when fed,
    from host memory, the samples the host-compiled decoder makes of the same codes."""
    n, tick, ticks = 256, 160, 30
    cfg = (AL.DVI4, 0) if family == AL.IMA else (32000, 0)
    digs = ["159D", "2*80", "#A4C6", "7B3", "0000", "91", "D#*", "852"]
    mine = [digs[(c//3) % 8] for c in range(n)]
    L = engine.lib()
    tx = engine.TxBank(engine.TX_DTMF, n)
    rx = engine.ToneBank(engine.DTMF, n)
    enc, dec = bank_of(family, [cfg], n), bank_of(family, [cfg], n)
    stream = L.spangpu_bank_get_stream(rx.h)
    for b in (tx, enc, dec):
        b.set_stream(stream)
    assert not tx.put_each(mine).any()
    cap = enc.encode_capacity(tick)
    assert cap == (84 if family == AL.IMA else 80) and dec.decode_capacity(cap) == tick
    stride = (cap + 15) & ~15
    got = [""]*n
    sent = []
    a, codes, b = DevBytes(n*tick*2), DevBytes(n*stride), DevBytes(n*tick*2)
    try:
        for k in range(ticks):
            tx.tx_device(a.ptr, tick, tick)
            enc.encode_device(a.ptr, 2*tick, tick, codes.ptr, stride)
            dec.decode_device(codes.ptr, stride, cap, b.ptr, 2*tick)
            rx.rx_device(b.ptr.value, tick, tick)
            rx.sync()
            sent.append(codes.get((n, stride))[:, :cap].copy())
            for r in rx.blocks():
                if (r["flags"] & engine.BLK_CHANGE) and r["code"]:
                    got[r["channel"]] += chr(r["code"])
        last = b.get((n, tick), np.int16)
    finally:
        for d in (a, codes, b):
            d.free()
    # the same codes through the host-compiled decoder, one call a tick, into a receiver bank of the same configuration
    streams = np.concatenate(sent, axis=1)
    made = AL.host_cases(host_program, str(tmp_path), [(family, AL.DECODE, cfg[0], cfg[1], streams[c], [cap]*ticks) for c in range(n)])
    rx2 = engine.ToneBank(engine.DTMF, n)
    want = [""]*n
    for k in range(ticks):
        rows = np.stack([m.want[k*tick:(k + 1)*tick] for m in made]).astype(np.int16)
        assert rows.shape == (n, tick)
        rx2.rx_host(rows)
        for r in rx2.blocks():
            if (r["flags"] & engine.BLK_CHANGE) and r["code"]:
                want[r["channel"]] += chr(r["code"])
    assert np.array_equal(last, rows)
    assert got == want
    for c in (0, 1, 63, 64, n - 1):
        assert np.array_equal(dec.get_state(c), made[c].calls[-1][2]), c
    # the chain carries the signal: some line delivers the digits it was given
    assert any(g == m for g, m in zip(got, mine))
