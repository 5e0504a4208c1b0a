"""The caller-ID banks on the GPU, for equality with what the reference's adsi.c produced (tests/golden/adsi_fsk.npz, written
by tests/golden/make_golden_adsi.py): sender samples, lengths and state words call for call, receiver messages, arrival
calls, framing errors and state words on the lines of tests/adsi_lines.py, per-channel lengths, a device-resident loop of
4 096 lines, state moved between channels, and a C caller by the spandsp names.  Everything is integer arithmetic, or
tone_gen's binary32 restated exactly: no tolerance anywhere."""
import os

import numpy as np
import pytest

import adsi_lines as AL
import fsktx_ref
from spandsp_amd import engine
from test_c_callers import build, run

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adsi_fsk.npz")
SCHEDULE = fsktx_ref.SCHEDULE
N_TX = 70                       # a full wave of 64 and a partial one; every wave mixes the four standards
TX_WORDS = 24                   # ADT_* (16), then FT_BAUD_RATE .. FT_SHUTDOWN (8): what the fixture's words map to
ADT_MSG_LEN, ADT_TX_SIGNAL_ON, ADR_MSG_LEN, ADR_FRAMING_ERRORS = 8, 9, 4, 5


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def lines():
    """The receiver lines, rendered once: {name: (standard, samples)} for the 160-sample-call ones, and the 1 024 one"""
    sweep = AL.sweep_lines()
    hand = AL.hand_lines()
    return {"sweep": [(n, s, x) for n, s, x in sweep], "hand": [(n, s, x) for n, s, x, t in hand if t == AL.TICK],
            "wide": [(n, s, x, t) for n, s, x, t in hand if t != AL.TICK]}


def delivered_of(packed, standard):
    """what a receiver hands to put_msg for these bytes on the line"""
    return bytes(b & 0x7F for b in packed[:-2]) if standard == AL.JCLIP else bytes(packed[:-1])


def expect_tx(g, run_name, standard, call):
    """(samples, returned length, words) of call `call` of a fixture run; past its end the sender is idle"""
    lens = g["tx_%s_%d_len" % (run_name, standard)]
    words = g["tx_%s_%d_words" % (run_name, standard)]
    if call >= len(lens):
        return np.zeros(0, np.int16), 0, words[-1]
    at = int(np.sum(lens[:call]))
    return g["tx_%s_%d_pcm" % (run_name, standard)][at:at + lens[call]], int(lens[call]), words[call]


def check_tx_call(g, bank, run_of, call, n, first=0):
    """one call of every channel against the fixture; run_of(c) = (run name, call offset) of channel c"""
    pcm, lens = bank.tx_host(n)
    for c in range(bank.n):
        s = AL.STANDARDS[c % 4]
        name, off = run_of(c)
        want, wlen, words = expect_tx(g, name, s, call + off)
        assert lens[c] == wlen, (c, call, lens[c], wlen)
        assert np.array_equal(pcm[c, :wlen], want), (c, call)
        assert not pcm[c, wlen:].any(), (c, call)
        got = bank.get_state(c) if c in (0, 1, 2, 3, 63, 64, bank.n - 1) else None
        if got is not None:
            assert np.array_equal(got[:TX_WORDS], words), (c, call, got[:TX_WORDS], words)


@pytest.mark.parametrize("run_name", ["plain", "alert", "preamble"])
def test_sender_parity(built, golden, run_name):
    g = golden
    bank = engine.AdsiTxBank(AL.STANDARDS, N_TX)
    for c in range(4):
        assert np.array_equal(bank.get_state(c)[:TX_WORDS], g["tx_init_%d" % AL.STANDARDS[c]])
    for c in range(N_TX):
        if run_name == "alert":
            bank.send_alert_tone(c)
        if run_name == "preamble":
            bank.set_preamble(c, 40, 20, 7, 2)
    msgs = [AL.sweep_message(AL.STANDARDS[c % 4]) for c in range(N_TX)]
    assert np.array_equal(bank.put_message(msgs), [len(m) for m in msgs])
    calls = max(len(g["tx_%s_%d_len" % (run_name, s)]) for s in AL.STANDARDS) + 1
    for k in range(calls):
        check_tx_call(g, bank, lambda c: (run_name, 0), k, SCHEDULE[k % len(SCHEDULE)])


def test_sender_second_message_busy_put_and_too_long(built, golden):
    g = golden
    bank = engine.AdsiTxBank(AL.STANDARDS, N_TX)
    first = [AL.sweep_message(AL.STANDARDS[c % 4]) for c in range(N_TX)]
    other = [AL.number_message(AL.STANDARDS[c % 4], b"987", b"Zed") for c in range(N_TX)]
    assert np.array_equal(bank.put_message(first), [len(m) for m in first])
    # the fixture's run: 4 calls, a put while busy (0), on to the end, the second message, on to its end; each part starts
    # the schedule again, and the four standards' parts differ in length -- every channel follows its own standard's run
    splits = {s: g["tx_second_%d_split" % s] for s in AL.STANDARDS}
    total = {s: len(g["tx_second_%d_len" % s]) for s in AL.STANDARDS}
    assert all(splits[s][0] == 4 for s in AL.STANDARDS)
    for k in range(4):
        check_tx_call(g, bank, lambda c: ("second", 0), k, SCHEDULE[k])
    assert not bank.put_message(other).any()
    # the middle and last parts standard by standard: the other standards' channels run along and are checked in their turn
    for s in AL.STANDARDS:
        solo = engine.AdsiTxBank([s], 3)
        assert np.array_equal(solo.put_message([first[s - 1]]*3), [len(first[s - 1])]*3)
        pos = 0
        for part, end in enumerate((4, int(splits[s][1]), total[s])):
            if part == 1:
                assert not solo.put_message([other[s - 1]]*3).any()
            if part == 2:
                assert np.array_equal(solo.put_message([other[s - 1]]*3), [len(other[s - 1])]*3)
            for k in range(end - pos):
                n = SCHEDULE[k % len(SCHEDULE)]
                pcm, lens = solo.tx_host(n)
                want, wlen, words = expect_tx(g, "second", s, pos + k)
                for c in range(3):
                    assert lens[c] == wlen and np.array_equal(pcm[c, :wlen], want) and not pcm[c, wlen:].any(), (s, part, k)
                    assert np.array_equal(solo.get_state(c)[:TX_WORDS], words), (s, part, k)
            pos = end
        longest, over = g["tx_long_%d" % s][0]
        fresh = engine.AdsiTxBank([s], 2)
        body = bytes((i*3 + 1) & 0x7F for i in range(over))
        assert list(fresh.put_message([body[:longest], body])) == list(g["tx_long_%d" % s][1]) == [longest, -1]
        # a refused message leaves the sender free for the next one
        assert fresh.put_message([first[s - 1]], first=1)[0] == len(first[s - 1])


def test_set_preamble_on_one_channel_only(built, golden):
    g = golden
    bank = engine.AdsiTxBank(AL.STANDARDS, 8)
    bank.set_preamble(6, 40, 20, 7, 2)
    bank.put_message([AL.sweep_message(AL.STANDARDS[c % 4]) for c in range(8)])
    calls = max(len(g["tx_plain_%d_len" % s]) for s in AL.STANDARDS)
    for k in range(calls):
        check_tx_call(g, bank, lambda c: ("preamble" if c == 6 else "plain", 0), k, SCHEDULE[k % len(SCHEDULE)])


def run_lines(bank, rows_of, n_calls, tick):
    """every call of every channel; returns per channel [(call, message)]"""
    got = [[] for _ in range(bank.n)]
    for k in range(n_calls):
        bank.rx_host(np.stack([r[k*tick:(k + 1)*tick] for r in rows_of]))
        for c, msgs in enumerate(bank.messages()):
            got[c] += [(k, m) for m in msgs]
    return got


def fixture_messages(g, name):
    at, ln, by = g["rx_%s_at" % name], g["rx_%s_len" % name], g["rx_%s_bytes" % name].tobytes()
    ends = np.cumsum(ln)
    return [(int(at[i]), by[ends[i] - ln[i]:ends[i]]) for i in range(len(at))]


def test_receiver_parity_on_the_sweep(built, golden, lines):
    g = golden
    sweep = lines["sweep"]
    assert len(sweep) == 64
    chans = sweep + [sweep[i] for i in (0, 5, 17, 34, 49, 63)]
    bank = engine.AdsiRxBank([s for _, s, _ in chans], len(chans))
    n_calls = len(chans[0][2])//AL.TICK
    got = run_lines(bank, [x for _, _, x in chans], n_calls, AL.TICK)
    audible = 0
    for c, (name, s, _) in enumerate(chans):
        want = fixture_messages(g, name)
        assert got[c] == want, (name, got[c], want)
        words = bank.get_state(c)
        assert np.array_equal(words[:6], g["rx_%s_words" % name]), (name, words[:6])
        if c < 64 and int(name.split("_a")[1].split("_")[0]) in AL.AUDIBLE:
            assert [m for _, m in want] == [delivered_of(AL.pack(s, AL.sweep_message(s)), s)], name
            audible += 1
    assert audible == 32
    for c, i in enumerate((0, 5, 17, 34, 49, 63)):
        assert got[64 + c] == got[i]


def test_receiver_parity_on_the_hand_framed_lines(built, golden, lines):
    g = golden
    hand = lines["hand"]
    assert len(hand) == 10
    bank = engine.AdsiRxBank([s for _, s, _ in hand], len(hand))
    got = run_lines(bank, [x for _, _, x in hand], len(hand[0][2])//AL.TICK, AL.TICK)
    for c, (name, s, _) in enumerate(hand):
        want = fixture_messages(g, name)
        assert got[c] == want, (name, got[c], want)
        words = bank.get_state(c)
        assert np.array_equal(words[:6], g["rx_%s_words" % name]), (name, words[:6])
    by_name = {name: got[c] for c, (name, _, _) in enumerate(hand)}
    # what each line is there for
    for name in ("bad_sum", "bad_crc", "stop_bit_0", "marks_10_no_restart", "length_past_256"):
        assert by_name[name] == [], name
    for name in ("jclip_not_dle_first", "marks_11_restart", "carrier_drop"):
        assert len(by_name[name]) == 1, name
    assert [len(m) for _, m in by_name["length_0"]] == [2] and [len(m) for _, m in by_name["length_252"]] == [254]
    assert g["rx_stop_bit_0_words"][ADR_FRAMING_ERRORS] == 1
    # two deliveries in one record, and the bound on a record
    (name, s, x, tick), = lines["wide"]
    wide = engine.AdsiRxBank([s], 3)
    # (30 bits a message, and the receiver's bit clock reports no two bits closer than 4 samples: include/spangpu.h)
    assert wide.msg_capacity(tick) == tick//(30*4) + 1 == 9 and wide.msg_capacity(160) == 160//(30*4) + 1 == 2
    got = run_lines(wide, [AL.calls_of(x, tick).reshape(-1)]*3, -(-len(x)//tick), tick)
    want = fixture_messages(g, name)
    assert len(want) == 2 and want[0][0] == want[1][0] == 1
    for c in range(3):
        assert got[c] == want
        assert np.array_equal(wide.get_state(c)[:6], g["rx_%s_words" % name])


def test_receiver_with_per_channel_lengths(built, golden, lines):
    g = golden
    chans = lines["sweep"] + lines["hand"]
    n = len(chans)
    bank = engine.AdsiRxBank([s for _, s, _ in chans], n)
    total = np.array([len(x) for _, _, x in chans])
    pos = np.zeros(n, np.int64)
    rng = np.random.default_rng(2024)
    got = [[] for _ in range(n)]
    while (pos < total).any():
        lens = np.minimum(rng.choice([0, 1, 77, 160], n), total - pos).astype(np.int32)
        amp = np.zeros((n, 160), np.int16)
        for c in range(n):
            amp[c, :lens[c]] = chans[c][2][pos[c]:pos[c] + lens[c]]
        bank.rx_host_var(amp, lens)
        for c, msgs in enumerate(bank.messages()):
            assert not msgs or lens[c] > 0
            got[c] += [(int(pos[c]), int(pos[c] + lens[c]), m) for m in msgs]
        pos += lens
    some = 0
    for c, (name, _, _) in enumerate(chans):
        want = fixture_messages(g, name)
        assert [m for _, _, m in got[c]] == [m for _, m in want], name
        # the arrival call, recomputed from the cumulative samples: the message completed inside (lo, hi]
        for (lo, hi, _), (call, _) in zip(got[c], want):
            assert lo < (call + 1)*AL.TICK and hi > call*AL.TICK, (name, lo, hi, call)
        assert np.array_equal(bank.get_state(c)[:6], g["rx_%s_words" % name]), name
        some += len(want)
    assert some >= 32


def test_device_resident_loop(built):
    n = 4096
    tx = engine.AdsiTxBank(AL.STANDARDS, n)
    rx = engine.AdsiRxBank(AL.STANDARDS, n)
    rows = fsktx_ref.DeviceRows(n, AL.TICK)
    msgs = [AL.number_message(AL.STANDARDS[c % 4], b"555%04d" % c, b"Line %04d" % c) for c in range(n)]
    assert np.array_equal(tx.put_message(msgs), [len(m) for m in msgs])
    got = [[] for _ in range(n)]
    try:
        for k in range(40):
            tx.tx_device(rows.ptr, AL.TICK, AL.TICK, rows.lens)
            tx.sync()
            rx.rx_device(rows.ptr, AL.TICK, AL.TICK)
            for c, m in enumerate(rx.messages()):
                got[c] += [(k, x) for x in m]
        lens = rows.lengths()
    finally:
        rows.free()
    assert not lens.any()
    at = {s: set() for s in AL.STANDARDS}
    for c in range(n):
        s = AL.STANDARDS[c % 4]
        assert [m for _, m in got[c]] == [delivered_of(AL.pack(s, msgs[c]), s)], c
        at[s].add(got[c][0][0])
    # the messages are of one length per standard (the index has four digits): one arrival call each, J-CLIP's its own
    assert at[AL.CLASS] == at[AL.CLIP] == at[AL.ACLIP] and len(at[AL.CLASS]) == 1 and len(at[AL.JCLIP]) == 1 and at[AL.JCLIP] != at[AL.CLASS]
    for c in (0, 1, 2, 3, 63, 64, 2049, n - 1):
        w = tx.get_state(c)
        assert w[ADT_TX_SIGNAL_ON] == 0 and w[ADT_MSG_LEN] == 0, c
        assert rx.get_state(c)[ADR_MSG_LEN] == 0, c


def test_state_moves_between_channels(built, golden, lines):
    g = golden
    # sender: channel 1 (CLIP) and 3 (J-CLIP), mid-message, continue at indices 5 and 4
    tx = engine.AdsiTxBank(AL.STANDARDS, 6)
    tx.send_alert_tone(1)
    tx.put_message([AL.sweep_message(AL.STANDARDS[c % 4]) for c in range(4)])
    for k in range(6):
        tx.tx_host(SCHEDULE[k])
    for src, dst in ((1, 5), (3, 4)):
        w = tx.get_state(src)
        assert w[ADT_MSG_LEN] > 0
        tx.set_state(dst, w)
        tx.set_message(dst, tx.get_message(src))
        assert np.array_equal(tx.get_state(dst), w)
    for k in range(6, 34):
        pcm, lens = tx.tx_host(SCHEDULE[k % len(SCHEDULE)])
        for src, dst in ((1, 5), (3, 4)):
            assert lens[src] == lens[dst] and np.array_equal(pcm[src], pcm[dst]), (k, src)
            assert np.array_equal(tx.get_state(src), tx.get_state(dst))
        want, wlen, _ = expect_tx(g, "plain", AL.JCLIP, k)
        assert lens[4] == wlen and np.array_equal(pcm[4, :wlen], want)
    assert tx.get_state(5)[ADT_TX_SIGNAL_ON] == 0 and tx.get_state(4)[ADT_MSG_LEN] == 0
    # receiver: the long A-CLIP line and a J-CLIP line, moved in mid-message
    hand = {name: (s, x) for name, s, x in lines["hand"]}
    names = ("length_252", "jclip_not_dle_first")
    rx = engine.AdsiRxBank([hand[nm][0] for nm in names] + [AL.CLASS, AL.CLASS], 4)
    rows = [hand[nm][1] for nm in names]
    n_calls = len(rows[0])//AL.TICK
    got = [[] for _ in range(4)]
    for k in range(n_calls):
        if k == 9:
            for src, dst in ((0, 3), (1, 2)):
                w = rx.get_state(src)
                assert w[ADR_MSG_LEN] > 0
                rx.set_state(dst, w)
                rx.set_message(dst, rx.get_message(src))
        feed = [rows[0], rows[1], rows[1], rows[0]] if k >= 9 else [rows[0], rows[1], np.zeros_like(rows[1]), np.zeros_like(rows[0])]
        rx.rx_host(np.stack([r[k*AL.TICK:(k + 1)*AL.TICK] for r in feed]))
        for c, m in enumerate(rx.messages()):
            got[c] += [(k, x) for x in m]
    assert got[0] == got[3] == fixture_messages(g, names[0]) and got[1] == got[2] == fixture_messages(g, names[1])
    assert np.array_equal(rx.get_state(0), rx.get_state(3)) and np.array_equal(rx.get_state(1), rx.get_state(2))


def test_c_caller_by_the_spandsp_names(built, tmp_path):
    exe = build("adsi_callerid", str(tmp_path))
    out = run([exe]).strip().splitlines()
    assert out == ["CLASS 1 80:0 02:7:5551212", "CLIP 1 80:0 02:7:5551212", "A-CLIP 1 80:0 02:7:5551212", "J-CLIP 1 40:0 02:7:5551212",
                   "CLIP-DTMF NULL NULL", "TDD NULL NULL"]
