"""The FAX receive front-end banks on the GPU against tests/golden/faxfe.npz: what the reference's fax_modems delivered under
fax_rx()'s loop, tick by tick -- the hdlc_accept calls, the non-ECM put_bit calls, the handler installed afterwards and
rx_frame_received -- and, at the end of a channel's case, the dc_restore state, the framer's words and buffer, and the inner
receivers' state (against the oracle's receivers driven with the frames the reference's handlers handed on: a receiver that
sat out must be where it was when its handler left).  Everything is compared for equality."""
import numpy as np
import pytest

import faxfe_cases as FC
from hdlc_cases import DeviceBytes
from test_oracle_pin import bits, use_golden_modem_tables

pytestmark = pytest.mark.gpu

N = 70                      # two blocks of the route kernel; five waves of the four-lane receivers, the last one partial
V21_RX, V17_RX, V27TER_RX, V29_RX = 12, 13, 14, 15
V21_CUTOFF, V29_CUTOFF = -39.09, -45.5


def host_dc_restore(state, x):
    """dc_restore(), spandsp/dc_restore.h:73-77, over one frame"""
    out = np.zeros(len(x), np.int16)
    for i, s in enumerate(x.tolist()):
        state += ((s << 15) - state) >> 14
        out[i] = s - (state >> 15)
    return state, out


@pytest.fixture(scope="module")
def cases(built):
    return FC.load()[0]


@pytest.fixture(scope="module")
def ends(cases):
    """Per case: the oracle's receivers after the frames the reference's handlers handed them -- {"fast": {kind: (floats,
    ints)}, "v21": words}.  On the way the oracle's put_bit streams are held against the fixture's rows, so that the states
    compared at the end belong to receivers that said what the reference's said."""
    from oracle import restated as orc
    from spandsp_amd import engine
    use_golden_modem_tables()
    make = {V29_RX: (engine.V29, orc.V29), V17_RX: (engine.V17, orc.V17), V27TER_RX: (engine.V27TER, orc.V27ter)}
    out = {}
    for name, c in cases:
        v21 = orc.Fsk(engine.FSK_V21CH2, engine.FSK_FRAME_MODE_SYNC)
        v21.set_signal_cutoff(V21_CUTOFF)
        fast = {}
        which = 0
        handler = FC.NONE
        dc = 0
        for t in range(int(c["cfg"][1])):
            for op, path in zip(c["ops"], c["path"]):
                if op[0] != t:
                    continue
                if op[1] == FC.SLOW:
                    v21 = orc.Fsk(engine.FSK_V21CH2, engine.FSK_FRAME_MODE_SYNC)
                    v21.set_signal_cutoff(V21_CUTOFF)
                    handler = FC.V21_ONLY
                else:
                    which = int(op[2])
                    if path == 1:
                        fast[which] = make[which][1](int(op[3]))
                        if which == V29_RX:
                            fast[which].set_signal_cutoff(V29_CUTOFF)
                    else:
                        assert which == V17_RX, "the oracle restarts V.17 only"
                        fast[which].restart(int(op[3]), int(op[4]))
                    handler = FC.FAST_AND_V21
            x = FC.tick(c, "amp", t)
            if c["cfg"][0] and handler != FC.NONE:
                dc, x = host_dc_restore(dc, x)
            got_fast = np.zeros(0, np.int8)
            got_v21 = np.zeros(0, np.int16)
            if handler in (FC.FAST_AND_V21, FC.FAST_ONLY):
                fast[which].sink.clear()
                fast[which].rx(x)
                got_fast = fast[which].sink.events()["a"].astype(np.int8)
            if handler in (FC.FAST_AND_V21, FC.V21_ONLY):
                v21.sink.clear()
                v21.rx(x)
                got_v21 = v21.sink.events()["a"].astype(np.int16)
            assert np.array_equal(got_fast, FC.tick(c, "fast", t)), (name, t, "fast")
            assert np.array_equal(got_v21, FC.tick(c, "v21", t)), (name, t, "v21")
            handler = int(c["handler"][t])
        assert dc == int(c["dc"][0]), name
        out[name] = {"fast": {make[k][0]: o.snapshot() for k, o in fast.items()}, "v21": v21.snapshot()}
    return out


def run_plan(fe, plan, ends, lens, device_input=False, skip=(), after_tick=None):
    """plan[c] = (case, first tick) or None.  lens: the tick lengths.  Every tick's frames, non-ECM bits and handlers of every
    channel are held against the fixture (channels in `skip` against nothing), and the states at the end of a channel's case."""
    from spandsp_amd import engine
    dev = DeviceBytes(fe.n*max(lens)*2) if device_input else None
    checked = 0
    for t, n_samples in enumerate(lens):
        x = np.zeros((fe.n, n_samples), np.int16)
        local = {}
        for ch, p in enumerate(plan):
            if p is None:
                continue
            c, first = p
            lt = t - first
            if not 0 <= lt < int(c["cfg"][1]):
                continue
            assert c["lens"][lt] == n_samples
            local[ch] = lt
            x[ch] = FC.tick(c, "amp", lt)
            for op in c["ops"]:
                if op[0] == lt and op[1] == FC.SLOW:
                    fe.start_slow_modem(ch, int(op[2]))
                elif op[0] == lt:
                    fe.start_fast_modem(ch, int(op[2]), int(op[3]), int(op[4]), int(op[5]))
        if after_tick:
            after_tick(t)
        if device_input:
            dev.upload(x)
            fe.rx_device(dev.ptr, n_samples, n_samples)
        else:
            fe.rx_host(x)
        recs, nrecs, octets, noctets = fe.frames_raw()
        put = fe.put_bits()
        handler, frx = fe.handlers()
        for ch, p in enumerate(plan):
            if ch in skip:
                continue
            if ch not in local:
                # not started yet: nothing runs and nothing is said (after its case's end a channel is left to itself)
                if p is None or t < p[1]:
                    assert handler[ch] == FC.NONE and nrecs[ch] == 0 and noctets[ch] == 0 and len(put[ch]) == 0, (t, ch)
                continue
            c, lt = p[0], local[ch]
            assert np.array_equal(recs[ch, :nrecs[ch]], FC.tick(c, "recs", lt)), (t, ch, "records")
            assert np.array_equal(octets[ch, :noctets[ch]], FC.tick(c, "bytes", lt)), (t, ch, "octets")
            assert np.array_equal(put[ch], FC.tick(c, "put", lt)), (t, ch, "non-ECM bits")
            assert handler[ch] == c["handler"][lt] and frx[ch] == c["frx"][lt], (t, ch, handler[ch], frx[ch])
            checked += 1
        # the states, where a channel's case ends with this tick
        for ch, lt in local.items():
            c = plan[ch][0]
            if ch in skip or lt != int(c["cfg"][1]) - 1:
                continue
            w = fe.get_words(ch)
            assert w[engine.FAXFE_W_DC_STATE] == c["dc"][0], (ch, "dc_restore state")
            assert np.array_equal(fe.framer().get_state(ch), c["framer"]), (ch, "framer words")
            assert np.array_equal(fe.framer().get_buffer(ch), c["buffer"]), (ch, "framer buffer")
            end = ends[c["name"]]
            assert np.array_equal(fe.v21_bank().get_state(ch), end["v21"]), (ch, "V.21 state")
            assert end["fast"], ch
            for kind, (of, oi) in end["fast"].items():
                fw, iw = fe.fast_bank(kind).get_state(ch)
                assert np.array_equal(bits(fw), bits(of)) and np.array_equal(iw, oi), (ch, kind, "fast modem state")
    if dev:
        dev.free()
    return checked


def named(cases, without=()):
    out = []
    for name, c in cases:
        if name not in without:
            c["name"] = name
            out.append(c)
    return out


@pytest.mark.parametrize("mapping", [1, 4])
@pytest.mark.parametrize("device_input", [False, True])
def test_every_case_at_mixed_phases(cases, ends, mapping, device_input):
    """Channel c runs case c % K, its first control call (c // K) % 3 ticks late: neighbours in a wave are at different
    phases and under different handlers, and those that have not begun sit in NONE."""
    from spandsp_amd import engine
    use = named(cases, without=("v29_page_dc", "v17_ecm_odd_ticks"))
    k = len(use)
    plan = [(use[c % k], (c // k) % 3) for c in range(N)]
    ticks = max(int(c["cfg"][1]) for c in use) + 2
    engine.tune_modem_mapping(mapping)
    try:
        fe = engine.FaxFrontEnd(N, max_samples=160)
        checked = run_plan(fe, plan, ends, [160]*ticks, device_input=device_input)
        fe.close()
    finally:
        engine.tune_modem_mapping(0)
    assert checked == sum(int(p[0]["cfg"][1]) for p in plan)


def test_control_calls_leave_the_neighbours_alone(cases, ends):
    """One channel is started, restarted and re-initialised while its neighbours receive: their records and states stay the
    reference's."""
    from spandsp_amd import engine
    use = named(cases)
    c = [x for x in use if x["name"] == "v17_ecm"][0]
    victim = 33
    plan = [(c, ch % 2) for ch in range(N)]
    fe = engine.FaxFrontEnd(N, max_samples=160)
    seen = []

    def meddle(t):
        if t == 5:
            fe.start_slow_modem(victim)
        elif t == 30:
            fe.start_fast_modem(victim, V17_RX, 14400, True, True)          # the restart path
        elif t == 50:
            fe.start_fast_modem(victim, V29_RX, 9600, False, False)         # another kind: a fresh state in the V.29 bank
        elif t == 60:
            fe.start_fast_modem(victim, V17_RX, 12000, False, True)         # back: fresh again, in a bank made for the rate
        if t in (6, 31, 51, 61):
            seen.append((int(fe.handlers()[0][victim]), fe.get_words(victim).tolist()))

    checked = run_plan(fe, plan, ends, [160]*(int(c["cfg"][1]) + 1), skip=(victim,), after_tick=meddle)
    assert checked == (N - 1)*int(c["cfg"][1])
    assert seen[0][0] == FC.V21_ONLY
    assert seen[1][1][engine.FAXFE_W_SHORT_TRAIN] == 1 and seen[1][1][engine.FAXFE_W_FAST_MODEM] == V17_RX
    assert seen[2][1][engine.FAXFE_W_SHORT_TRAIN] == 0 and seen[2][1][engine.FAXFE_W_FAST_MODEM] == V29_RX
    assert seen[3][1][engine.FAXFE_W_BIT_RATE] == 12000 and fe.fast_bank(engine.V17, 12000) is not None
    # what is refused changes nothing
    before = fe.get_words(victim)
    for which, rate in ((V17_RX, 2400), (V29_RX, 14400), (V27TER_RX, 9600)):
        assert engine.lib().spangpu_faxfe_start_fast_modem(fe.h, victim, which, rate, 0, 0) == -2
    # the same kind at another rate would be a restart that moves the line to another bank: refused, V.29 apart
    assert engine.lib().spangpu_faxfe_start_fast_modem(fe.h, victim, V17_RX, 9600, 0, 1) == -6
    for which in (9, 10, 11, 16, 17):                                       # the senders, V.34
        assert engine.lib().spangpu_faxfe_start_fast_modem(fe.h, victim, which, 9600, 0, 0) == -6
    for which in (6, 7, 8):                                                 # CED / CNG receive, V.21 transmit
        assert engine.lib().spangpu_faxfe_start_slow_modem(fe.h, victim, which) == -6
    assert np.array_equal(fe.get_words(victim), before)
    fe.close()
    only29 = engine.FaxFrontEnd(4, kinds_mask=engine.FAXFE_V29)
    assert engine.lib().spangpu_faxfe_start_fast_modem(only29.h, 0, V17_RX, 14400, 0, 0) == -6
    assert only29.fast_bank(engine.V17) is None and only29.fast_bank(engine.V29) is not None
    only29.close()


@pytest.mark.parametrize("device_input", [False, True])
def test_ticks_shorter_and_longer_than_usual(cases, ends, device_input):
    """samples below max_samples, and the tick lengths 160, 7, 200, 40 in turn; half of the channels never begin."""
    from spandsp_amd import engine
    c = [x for x in named(cases) if x["name"] == "v17_ecm_odd_ticks"][0]
    plan = [(c, 0) if ch % 2 == 0 or ch > 60 else None for ch in range(N)]
    fe = engine.FaxFrontEnd(N, kinds_mask=engine.FAXFE_V17, max_samples=203)
    stream = None
    if device_input:
        # on a stream of the caller's: every inner bank follows
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        stream = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
        fe.set_stream(stream)
    checked = run_plan(fe, plan, ends, [int(x) for x in c["lens"]], device_input=device_input)
    assert checked == sum(p is not None for p in plan)*int(c["cfg"][1])
    assert engine.lib().spangpu_faxfe_rx(fe.h, np.zeros((N, 204), np.int16).ctypes.data, 0, 204, 204) == -2
    assert engine.lib().spangpu_faxfe_set_stream(fe.h, None) == -2
    fe.close()
    if stream is not None:
        hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
        assert hip.hipStreamDestroy(stream) == 0


def test_dc_restore_on_a_line_with_an_offset(cases, ends):
    from spandsp_amd import engine
    c = [x for x in named(cases) if x["name"] == "v29_page_dc"][0]
    plan = [(c, ch % 3) if ch % 5 else None for ch in range(N)]
    fe = engine.FaxFrontEnd(N, kinds_mask=engine.FAXFE_V29, max_samples=160, dc_restore=True)
    checked = run_plan(fe, plan, ends, [160]*(int(c["cfg"][1]) + 2))
    assert checked == sum(p is not None for p in plan)*int(c["cfg"][1])
    # a channel that never had a handler took no part: its dc_restore state is as it was made
    assert fe.get_words(0)[engine.FAXFE_W_DC_STATE] == 0
    fe.close()
