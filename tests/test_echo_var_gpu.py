"""spangpu_echo_update_var(): a tick in which every channel of an echo canceller bank has a length of its own -- late and
silent channels sit it out (length 0), the others are run by one launch per distinct (length, use_hpf_tx) over a slot ->
channel list (EchoLaunch::chan, csrc/echo_dev.hpp).  Every channel against its own oracle object, called with exactly
those lengths: every clean and tx_out sample, the complete state, bit-exact; under every lane mapping, from host rows
(compacted) and from device rows (addressed by channel)."""
import numpy as np
import pytest

from echo_lines import DeviceRows, compare_state, make_channels, same_state

pytestmark = pytest.mark.gpu

N_CH = 37                                   # ragged: the last wave of every mapping is partly filled
TICKS = 150
MAX_SAMPLES = 160
LENS = np.array([0, 1, 7, 31, 64, 77, 160])
LENS_P = np.array([0.25] + [0.125]*6)       # a quarter of the draws sit the tick out
CANARY = 0x5A5A
MIXED = [0x01, 0x03, 0x07, 0x67]


def scenario(taps, modes, seed=None):
    """(tx, rx, lens[tick][channel], flags[tick][channel], mode per channel); the lines are long enough for 160 samples a tick"""
    seed = 1000 + taps if seed is None else seed
    tx, rx = make_channels(N_CH, MAX_SAMPLES*TICKS, taps, seed)
    rng = np.random.default_rng(seed + 1)
    lens = rng.choice(LENS, size=(TICKS, N_CH), p=LENS_P).astype(np.int32)
    flags = rng.integers(0, 2, size=(TICKS, N_CH)).astype(np.uint8)
    if modes == "mixed":
        mode = [MIXED[i] for i in rng.integers(0, len(MIXED), N_CH)]
    else:
        mode = [modes]*N_CH
    return tx, rx, lens, flags, mode


def rare_paths_driven(snaps):
    # the scenario must really have driven the rare paths somewhere in the bank
    assert any(s["tap_set"] != 0 or s["tap_rotate_counter"] != 1600 for s in snaps)
    assert any(np.any(s["taps32"] != 0) for s in snaps)


def make_bank(taps, mode, lanes):
    from spandsp_amd import engine
    assert engine.lib().spangpu_tune_echo_lanes_per_channel(lanes) == 0
    try:
        bank = engine.EchoBank(N_CH, taps, mode[0])
    finally:
        engine.lib().spangpu_tune_echo_lanes_per_channel(0)
    if len(set(mode)) > 1:
        for c, m in enumerate(mode):
            bank.adaption_mode(m, channel=c)
    return bank


def oracle_tx_out(hp, tx, flag, mode=0x20):
    """What echo_can_hpf_tx() hands to the line (echo.c:663-669), from an oracle object kept for the transmit filter alone:
    its two filter words depend on nothing but the transmit samples it has seen."""
    import ctypes
    from oracle import restated as orc
    if not flag or not (mode & 0x20):       # (ECHO_CAN_USE_TX_HPF off: the filter hands tx on and keeps no state)
        return tx
    f = orc.lib().orc_echo_hpf_tx
    p = ctypes.c_void_p(hp.p)
    return np.array([f(p, ctypes.c_int16(int(x))) & 0xFFFF for x in tx], np.uint16).view(np.int16)


class Rows:
    """One tick's call on host rows or on device rows; the same results either way"""

    def __init__(self, bank, mem):
        self.bank = bank
        self.mem = mem
        if mem == "device":
            self.d = [DeviceRows(N_CH, MAX_SAMPLES) for _ in range(4)]

    def run(self, tx, rx, lens, flags):
        clean = np.full((N_CH, MAX_SAMPLES), CANARY, np.int16)
        tx_out = np.full((N_CH, MAX_SAMPLES), CANARY, np.int16)
        if self.mem == "host":
            _, n = self.bank.update_var_host(tx, rx, lens, flags, clean=clean, tx_out=tx_out)
            return clean, tx_out, n
        dtx, drx, dcl, dto = self.d
        dtx.put(tx)
        drx.put(rx)
        dcl.put(clean)
        dto.put(tx_out)
        n = self.bank.update_var_device(dtx.ptr, drx.ptr, dcl.ptr, dto.ptr, lens, flags, MAX_SAMPLES, MAX_SAMPLES)
        self.bank.sync()
        return dcl.get(), dto.get(), n

    def close(self):
        if self.mem == "device":
            for d in self.d:
                d.free()


def frame_rows(tx, rx, pos, lens):
    """the rows of a tick: channel c's next lens[c] samples, the rest of its row noise that must not matter"""
    a = np.full((N_CH, MAX_SAMPLES), 12345, np.int16)
    b = np.full((N_CH, MAX_SAMPLES), -4321, np.int16)
    for c in range(N_CH):
        a[c, :lens[c]] = tx[c, pos[c]:pos[c] + lens[c]]
        b[c, :lens[c]] = rx[c, pos[c]:pos[c] + lens[c]]
    return a, b


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("modes", [0x01, 0x07, "mixed"])
@pytest.mark.parametrize("lanes", [0, 2, 4, 8, 16])
@pytest.mark.parametrize("taps", [32, 128, 512])
def test_echo_update_var_parity(built, taps, lanes, modes, mem):
    from oracle import restated as orc
    from spandsp_amd import engine
    tx, rx, lens, flags, mode = scenario(taps, modes)
    bank = make_bank(taps, mode, lanes)
    rows = Rows(bank, mem)
    dets = [orc.EchoCan(taps, m) for m in mode]
    hps = [orc.EchoCan(taps, m) for m in mode]
    pos = np.zeros(N_CH, np.int64)
    for t in range(TICKS):
        a, b = frame_rows(tx, rx, pos, lens[t])
        idle = [c for c in range(N_CH) if lens[t, c] == 0]
        before = {c: bank.get_state(c) for c in idle}
        clean, tx_out, n = rows.run(a, b, lens[t], flags[t])
        assert n == int(np.count_nonzero(lens[t])), (t, n)
        for c, d in enumerate(dets):
            m = int(lens[t, c])
            if m:
                want = d.run(a[c, :m], b[c, :m], bool(flags[t, c]))
                assert np.array_equal(clean[c, :m], want), (t, c, m, np.nonzero(clean[c, :m] != want)[0][:5])
                assert np.array_equal(tx_out[c, :m], oracle_tx_out(hps[c], a[c, :m], flags[t, c], mode[c])), (t, c, m, "tx_out")
            assert np.all(clean[c, m:] == CANARY) and np.all(tx_out[c, m:] == CANARY), (t, c, m)
        for c in idle:
            after = bank.get_state(c)
            assert same_state(after, before[c], engine.ECHO_FIELDS) is None, (t, c)
        if t % 10 == 0:
            compare_state(bank, dets, (taps, lanes, modes, mem, t))
        pos += lens[t]
    compare_state(bank, dets, "final")
    rare_paths_driven([d.snapshot() for d in dets])
    rows.close()
    bank.close()


@pytest.mark.parametrize("mem", ["host", "device"])
def test_tx_out_is_the_filtered_transmit_signal(built, mem):
    """tx_out of a channel whose flag is set is what echo_can_hpf_tx() makes of tx, else tx: against a twin bank that runs
    the same lengths channel group by channel group through spangpu_echo_update_tx()."""
    from spandsp_amd import engine
    taps = 128
    tx, rx, lens, flags, mode = scenario(taps, 0x67, seed=77)
    bank = make_bank(taps, mode, 0)
    twin = [engine.EchoBank(1, taps, 0x67) for _ in range(N_CH)]
    rows = Rows(bank, mem)
    pos = np.zeros(N_CH, np.int64)
    for t in range(20):
        a, b = frame_rows(tx, rx, pos, lens[t])
        clean, tx_out, _ = rows.run(a, b, lens[t], flags[t])
        for c in range(N_CH):
            m = int(lens[t, c])
            if m == 0:
                continue
            wc = np.zeros((1, m), np.int16)
            wt = np.zeros((1, m), np.int16)
            ta = np.ascontiguousarray(a[c:c + 1, :m])
            tb = np.ascontiguousarray(b[c:c + 1, :m])
            assert engine.lib().spangpu_echo_update_tx(twin[c].h, ta.ctypes.data, tb.ctypes.data, wc.ctypes.data, wt.ctypes.data,
                                                       engine.MEM_HOST, m, m, int(flags[t, c])) == 0
            assert np.array_equal(clean[c, :m], wc[0]) and np.array_equal(tx_out[c, :m], wt[0]), (t, c)
        pos += lens[t]
    rows.close()


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("stats_mode", [1, 2])
def test_statistics_count_the_samples_that_ran(built, stats_mode, mem):
    """Statistics modes 1 (a pass of its own, with the CRC-32 of the clean stream) and 2 (sums by the update kernel): the
    oracle's sums over the samples each channel actually ran."""
    import zlib
    from oracle import restated as orc
    taps = 128
    tx, rx, lens, flags, mode = scenario(taps, 0x01, seed=4242)
    bank = make_bank(taps, mode, 0)
    bank.stats(stats_mode)
    rows = Rows(bank, mem)
    dets = [orc.EchoCan(taps, m) for m in mode]
    pos = np.zeros(N_CH, np.int64)
    sum_rx2 = np.zeros(N_CH, np.uint64)
    sum_clean2 = np.zeros(N_CH, np.uint64)
    crc = np.zeros(N_CH, np.uint32)
    for t in range(60):
        a, b = frame_rows(tx, rx, pos, lens[t])
        clean, _, _ = rows.run(a, b, lens[t], flags[t])
        for c, d in enumerate(dets):
            m = int(lens[t, c])
            if m == 0:
                continue
            want = d.run(a[c, :m], b[c, :m], bool(flags[t, c]))
            assert np.array_equal(clean[c, :m], want), (t, c)
            sum_rx2[c] += np.uint64((b[c, :m].astype(np.int64)**2).sum())
            sum_clean2[c] += np.uint64((want.astype(np.int64)**2).sum())
            crc[c] = zlib.crc32(want.astype("<i2").tobytes(), int(crc[c]))
        pos += lens[t]
    st = bank.stats_get()
    assert np.array_equal(st["samples"], lens[:60].sum(axis=0).astype(np.uint32))
    assert np.array_equal(st["sum_rx2"], sum_rx2) and np.array_equal(st["sum_clean2"], sum_clean2)
    if stats_mode == 1:
        assert np.array_equal(st["crc"], crc)
    rows.close()
    bank.close()


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("lanes", [0, 2])
def test_a_bank_in_step_is_the_plain_update(built, lanes, mem):
    """Every length 160 and one flag: the call is spangpu_echo_update_tx()'s, and output and state are a twin bank's that is
    driven through that entry point."""
    from spandsp_amd import engine
    taps = 128
    tx, rx, _, _, mode = scenario(taps, 0x01, seed=5)
    bank = make_bank(taps, mode, lanes)
    twin = make_bank(taps, mode, lanes)
    rows = Rows(bank, mem)
    lens = np.full(N_CH, 160, np.int32)
    flags = np.ones(N_CH, np.uint8)
    for t in range(40):
        a = np.ascontiguousarray(tx[:, 160*t:160*(t + 1)])
        b = np.ascontiguousarray(rx[:, 160*t:160*(t + 1)])
        clean, tx_out, n = rows.run(a, b, lens, flags)
        assert n == N_CH
        wc = np.zeros_like(a)
        wt = np.zeros_like(a)
        assert engine.lib().spangpu_echo_update_tx(twin.h, a.ctypes.data, b.ctypes.data, wc.ctypes.data, wt.ctypes.data,
                                                   engine.MEM_HOST, 160, 160, 1) == 0
        assert np.array_equal(clean, wc) and np.array_equal(tx_out, wt), t
    for c in range(N_CH):
        assert same_state(bank.get_state(c), twin.get_state(c), engine.ECHO_FIELDS) is None, c
    rows.close()


def test_bad_lengths_are_refused(built):
    from spandsp_amd import engine
    bank = engine.EchoBank(4, 128, 0x01)
    z = np.zeros((4, 160), np.int16)
    for lens in ([160, 161, 0, 0], [-1, 0, 0, 0]):
        with pytest.raises(engine.SpanGpuError) as ei:
            bank.update_var_host(z, z, lens)
        assert ei.value.code == -2
    _, n = bank.update_var_host(z, z, [0, 0, 0, 0])
    assert n == 0
