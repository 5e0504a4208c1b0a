"""Slot reuse on channel groups (include/spangpu_spandsp.h): a server frees a channel's object when a call ends and
attaches a new one to the same slot for the next call.  The new object must behave as a fresh xxx_rx_init() would --
whatever the previous object was doing when it was freed (mid-training, mid-data, mid-digit, mid-tone) and whatever
per-object settings it had changed (signal cutoff, dtmf_rx_parms(), status and QAM report handlers).

Every case compares the new object's callbacks with a fresh oracle that sees only the new call's samples, and checks in
the same test that an oracle which carried on from the previous call would have answered differently: a reuse that
leaked the old state would fail it.  Neighbouring slots (undisturbed, late and silent ones) run beside the churn and
must stay exact.  Where the library gives access to a bank, the reused channel's state words right after the attach must
equal those of a channel of a newly created group."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import synth
from test_oracle_pin import GOLDEN, use_golden_modem_tables

pytestmark = pytest.mark.gpu

PUT_BIT = C.CFUNCTYPE(None, C.c_void_p, C.c_int)
STATUS = C.CFUNCTYPE(None, C.c_void_p, C.c_int)
QAM = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)
DIGITS_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_int)
REPORT = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int)
FRAME = 160


class FskSpec(C.Structure):
    _fields_ = [("name", C.c_char_p), ("freq_zero", C.c_int), ("freq_one", C.c_int), ("tx_level", C.c_int),
                ("min_level", C.c_int), ("baud_rate", C.c_int)]


@pytest.fixture(scope="module")
def L(built):
    from spandsp_amd import engine
    lib = C.CDLL(engine.LIB_PATH)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    sig = {
        "spangpu_modem_group_create": (vp, [ci, ci, ci, ci, ci]),
        "spangpu_modem_group_destroy": (ci, [vp]),
        "spangpu_modem_group_flush": (ci, [vp]),
        "spangpu_modem_group_bank": (vp, [vp]),
        "spangpu_modem_state_words": (ci, [ci, vp, vp]),
        "spangpu_modem_get_state": (ci, [vp, ci, vp]),
        "spangpu_group_create": (vp, [ci, ci, ci, ci, vp]),
        "spangpu_group_destroy": (ci, [vp]),
        "spangpu_group_flush": (ci, [vp]),
        "spangpu_group_bank": (vp, [vp]),
        "spangpu_bank_get_state": (ci, [vp, ci, vp, ci, vp, ci]),
        "spangpu_dtmf_rx_attach": (vp, [vp, ci, DIGITS_CB, vp]),
        "dtmf_rx_init": (vp, [vp, DIGITS_CB, vp]),
        "dtmf_rx": (ci, [vp, vp, ci]),
        "dtmf_rx_parms": (None, [vp, ci, cf, cf, cf]),
        "dtmf_rx_free": (ci, [vp]),
        "spangpu_fsk_group_create": (vp, [ci, vp, ci, ci, ci]),
        "spangpu_modem_connect_tones_group_create": (vp, [ci, ci, ci, ci, ci]),
        "spangpu_line_group_destroy": (ci, [vp]),
        "spangpu_line_group_flush": (ci, [vp]),
        "fsk_rx_init": (vp, [vp, vp, ci, PUT_BIT, vp]),
        "spangpu_fsk_rx_attach": (vp, [vp, ci, PUT_BIT, vp]),
        "fsk_rx": (ci, [vp, vp, ci]),
        "fsk_rx_free": (ci, [vp]),
        "fsk_rx_set_signal_cutoff": (None, [vp, cf]),
        "fsk_rx_set_frame_parameters": (None, [vp, ci, ci, ci]),
        "fsk_rx_release": (ci, [vp]),
        "modem_connect_tones_rx_release": (ci, [vp]),
        "spangpu_bell_mf_rx_attach": (vp, [vp, ci, DIGITS_CB, vp]),
        "bell_mf_rx": (ci, [vp, vp, ci]),
        "bell_mf_rx_free": (ci, [vp]),
        "spangpu_r2_mf_rx_attach": (vp, [vp, ci, REPORT, vp]),
        "r2_mf_rx": (ci, [vp, vp, ci]),
        "r2_mf_rx_free": (ci, [vp]),
        "fsk_rx_set_modem_status_handler": (None, [vp, STATUS, vp]),
        "modem_connect_tones_rx_init": (vp, [vp, ci, REPORT, vp]),
        "spangpu_modem_connect_tones_rx_attach": (vp, [vp, ci, REPORT, vp]),
        "modem_connect_tones_rx": (ci, [vp, vp, ci]),
        "modem_connect_tones_rx_free": (ci, [vp]),
    }
    for pfx in ("v29_rx", "v27ter_rx", "v17_rx"):
        sig.update({
            pfx + "_init": (vp, [vp, ci, PUT_BIT, vp]),
            "spangpu_" + pfx + "_attach": (vp, [vp, ci, PUT_BIT, vp]),
            pfx: (ci, [vp, vp, ci]),
            pfx + "_free": (ci, [vp]),
            pfx + "_restart": (ci, [vp, ci, ci]),
            pfx + "_set_modem_status_handler": (None, [vp, STATUS, vp]),
            pfx + "_set_qam_report_handler": (None, [vp, QAM, vp]),
            pfx + "_set_signal_cutoff": (None, [vp, cf]),
            pfx + "_equalizer_state": (ci, [vp, C.POINTER(vp)]),
            pfx + "_carrier_frequency": (cf, [vp]),
            pfx + "_symbol_timing_correction": (cf, [vp]),
            pfx + "_signal_power": (cf, [vp]),
        })
    for name, (res, args) in sig.items():
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    return lib


def i16(a):
    return np.ascontiguousarray(a, np.int16)


class Call:
    """One call on one slot: attached at tick t0 (before that tick's frame), fed `sig` frame by frame (zeros once it has
    run out), freed at tick t1 (before that tick's frame; None = at the end).  `setup(obj)` runs right after the attach,
    `before_free(obj)` right before the free.  `fed` collects the samples the object was given, `ev` its callbacks."""

    def __init__(self, sig, t0=0, t1=None, setup=None, before_free=None):
        self.sig, self.t0, self.t1 = i16(sig), t0, t1
        self.setup, self.before_free = setup, before_free
        self.fed = []
        self.ev = []
        self.obj = None
        self.keep = []

    def frame(self, k):
        out = np.zeros(FRAME, np.int16)
        part = self.sig[(k - self.t0)*FRAME:(k - self.t0 + 1)*FRAME]
        out[:len(part)] = part
        return out

    def samples(self):
        return np.concatenate(self.fed) if self.fed else np.zeros(0, np.int16)


def drive(slots, ticks, attach, rx, free, flush, on_attach=None):
    """Run `ticks` ticks over slots (a list of Call lists, one per channel).  In each tick the channels go in order: a call
    ending there is freed, a call starting there is attached, then the live call stages its frame -- so frees and attaches
    happen while other channels of the same tick have staged and others have not.  flush() runs whatever did not run by
    itself (late, silent, or freed channels)."""
    for k in range(ticks):
        for c, calls in enumerate(slots):
            for call in calls:
                if call.obj is not None and call.t1 == k:
                    if call.before_free:
                        call.before_free(call.obj)
                    free(call.obj)
                    call.obj = None
            for call in calls:
                if call.t0 == k:
                    call.obj = attach(c, call)
                    assert call.obj, (c, k)
                    if on_attach:
                        on_attach(c, call)
                    if call.setup:
                        call.setup(call.obj)
            for call in calls:
                if call.obj is not None:
                    fr = call.frame(k)
                    call.fed.append(fr)
                    assert rx(call.obj, fr) == 0, (c, k)
        flush()
    for calls in slots:
        for call in calls:
            if call.obj is not None:
                free(call.obj)
                call.obj = None


# ---- modem receivers ----------------------------------------------------------------------------------------------
MODEMS = {
    # kind name: (prefix, oracle class, rate, golden, tick freed mid-training, tick freed mid-data)
    "v29_9600": ("v29_rx", "V29", 9600, "v29_9600", 6, 25),
    "v29_4800": ("v29_rx", "V29", 4800, "v29_4800", 6, 25),
    "v27ter_4800": ("v27ter_rx", "V27ter", 4800, "v27ter_4800", 12, 57),
    "v17_14400": ("v17_rx", "V17", 14400, "v17_14400", 25, 85),
}


def modem_kind(engine, pfx):
    return {"v29_rx": engine.V29, "v27ter_rx": engine.V27TER, "v17_rx": engine.V17}[pfx]


def modem_words(L, grp, kind, channel):
    n = L.spangpu_modem_state_words(kind, None, None)
    w = np.zeros(n, np.uint32)
    assert L.spangpu_modem_get_state(L.spangpu_modem_group_bank(grp), channel, w.ctypes.data) == n
    return w


def oracle_stream(cls, rate, parts, cutoffs=()):
    """Events of an oracle fed parts[0], parts[1], ...; cutoffs[i] (or None) is set after part i.  Returns the events
    of each part."""
    o = cls(rate)
    out = []
    n0 = 0
    for i, p in enumerate(parts):
        o.rx(p)
        ev = o.sink.events()["a"].astype(np.int32)
        out.append(ev[n0:])
        n0 = len(ev)
        if i < len(cutoffs) and cutoffs[i] is not None:
            o.set_signal_cutoff(cutoffs[i])
    return out


@pytest.mark.parametrize("name", list(MODEMS))
def test_modem_group_slot_reuse(L, name):
    """V.29 / V.27ter / V.17 group: objects freed mid-training and mid-data (after a cutoff change, with a status and a
    QAM report handler installed), a new object on the slot in the same tick or the next: the new object's put_bit stream
    is a fresh receiver's, the channel's words right after the attach are a new group's, the neighbours are untouched."""
    from oracle import restated as orc
    from spandsp_amd import engine
    use_golden_modem_tables()
    pfx, ocls, rate, gold, t_train, t_data = MODEMS[name]
    cls = getattr(orc, ocls)
    kind = modem_kind(engine, pfx)
    x = np.load(os.path.join(GOLDEN, gold + ".npz"))["amp"]
    nt = (len(x) + FRAME - 1)//FRAME
    has_cutoff = (pfx == "v29_rx")
    cutoff = -45.5

    fresh = L.spangpu_modem_group_create(0, kind, 1, rate, FRAME)
    assert fresh
    pristine = modem_words(L, fresh, kind, 0)
    L.spangpu_modem_group_destroy(fresh)

    qam_calls = [0]
    qam_cb = QAM(lambda u, a, b, s: qam_calls.__setitem__(0, qam_calls[0] + 1))

    def a_setup(obj, call):
        st = STATUS(lambda u, v: call.ev.append(v))
        call.keep.append(st)
        getattr(L, pfx + "_set_modem_status_handler")(obj, st, None)
        getattr(L, pfx + "_set_qam_report_handler")(obj, qam_cb, None)

    def a_free(obj):
        if has_cutoff:
            getattr(L, pfx + "_set_signal_cutoff")(obj, cutoff)

    def reuse(t_free, gap):
        a = Call(x, 0, t_free)
        a.setup = lambda o, a=a: a_setup(o, a)
        a.before_free = a_free
        b = Call(x, t_free + gap)
        return [a, b]

    ticks = nt + t_data + 2
    slots = [
        [Call(x)],                      # undisturbed
        reuse(t_train, 0),              # mid-training, new call in the same tick
        [Call(np.zeros(0))],            # silent
        reuse(t_data, 0),               # mid-data, same tick
        [Call(x, 5)],                   # late
        reuse(t_train, 1),              # mid-training, new call the next tick
        reuse(t_data, 1),               # mid-data, next tick
        [Call(x)],                      # undisturbed
    ]
    grp = L.spangpu_modem_group_create(0, kind, len(slots), rate, FRAME)
    assert grp
    attach_words = {}

    def attach(c, call):
        cb = PUT_BIT(lambda u, b: call.ev.append(b))
        call.keep.append(cb)
        return getattr(L, "spangpu_" + pfx + "_attach")(grp, c, cb, None)

    def on_attach(c, call):
        attach_words[(c, call.t0)] = modem_words(L, grp, kind, c)

    drive(slots, ticks, attach, lambda o, fr: getattr(L, pfx)(o, fr.ctypes.data, FRAME),
          getattr(L, pfx + "_free"), lambda: L.spangpu_modem_group_flush(grp), on_attach)
    L.spangpu_modem_group_destroy(grp)

    for (c, t0), w in attach_words.items():
        assert np.array_equal(w, pristine), (name, c, t0, np.nonzero(w != pristine)[0][:10])
    for c, calls in enumerate(slots):
        if len(calls) == 1:
            want, = oracle_stream(cls, rate, [calls[0].samples()])
            assert np.array_equal(np.array(calls[0].ev, np.int32), want), (name, c)
            continue
        a, b = calls
        want_a, = oracle_stream(cls, rate, [a.samples()])
        assert np.array_equal(np.array(a.ev, np.int32), want_a), (name, c)
        want_b, = oracle_stream(cls, rate, [b.samples()])
        assert np.array_equal(np.array(b.ev, np.int32), want_b), (name, c, len(b.ev), len(want_b))
        assert (want_b >= 0).sum() > 1000                           # call B trained and delivered data
        _, cont_b = oracle_stream(cls, rate, [a.samples(), b.samples()], [cutoff if has_cutoff else None])
        assert not np.array_equal(cont_b, want_b), (name, c)        # the case can tell a reset slot from a continued one
    # the slots freed mid-data really were in data; those freed mid-training had not trained
    assert (np.array(slots[3][0].ev) >= 0).sum() > 200 and (np.array(slots[1][0].ev) >= 0).sum() == 0
    assert qam_calls[0] > 0


@pytest.mark.parametrize("name", list(MODEMS))
def test_modem_private_reinit_in_place(L, name):
    """xxx_rx_init(s, ...) on a private object that has run (mid-data, with its own cutoff and handlers) is an init, not a
    restart: the callbacks after it are a fresh receiver's, and the getters read what a fresh object reads."""
    from oracle import restated as orc
    use_golden_modem_tables()
    pfx, ocls, rate, gold, _, t_data = MODEMS[name]
    cls = getattr(orc, ocls)
    x = np.load(os.path.join(GOLDEN, gold + ".npz"))["amp"]
    nt = (len(x) + FRAME - 1)//FRAME
    ev_a, ev_b, st_a = [], [], []
    cb_a = PUT_BIT(lambda u, b: ev_a.append(b))
    cb_b = PUT_BIT(lambda u, b: ev_b.append(b))
    st = STATUS(lambda u, v: st_a.append(v))
    n_qam = [0]
    qam = QAM(lambda u, a, b, s: n_qam.__setitem__(0, n_qam[0] + 1))
    s = getattr(L, pfx + "_init")(None, rate, cb_a, None)
    assert s
    getattr(L, pfx + "_set_modem_status_handler")(s, st, None)
    getattr(L, pfx + "_set_qam_report_handler")(s, qam, None)
    a = Call(x)
    for k in range(t_data):
        assert getattr(L, pfx)(s, a.frame(k).ctypes.data, FRAME) == 0
        a.fed.append(a.frame(k))
    if pfx == "v29_rx":
        getattr(L, pfx + "_set_signal_cutoff")(s, -45.5)
    assert getattr(L, pfx + "_init")(s, rate, cb_b, None) == s
    qam_at_init = n_qam[0]

    ref = getattr(L, pfx + "_init")(None, rate, cb_b, None)             # (never fed)
    for getter in ("_carrier_frequency", "_symbol_timing_correction", "_signal_power"):
        assert getattr(L, pfx + getter)(s) == getattr(L, pfx + getter)(ref), getter
    p1, p2 = C.c_void_p(), C.c_void_p()
    n1 = getattr(L, pfx + "_equalizer_state")(s, C.byref(p1))
    n2 = getattr(L, pfx + "_equalizer_state")(ref, C.byref(p2))
    assert n1 == n2 and C.string_at(p1.value, 8*n1) == C.string_at(p2.value, 8*n2)
    getattr(L, pfx + "_free")(ref)

    b = Call(x)
    for k in range(nt):
        assert getattr(L, pfx)(s, b.frame(k).ctypes.data, FRAME) == 0
        b.fed.append(b.frame(k))
    getattr(L, pfx + "_free")(s)
    want_b, = oracle_stream(cls, rate, [b.samples()])
    assert np.array_equal(np.array(ev_b, np.int32), want_b)      # status codes too: the handler went with the init
    assert st_a and not any(v >= 0 for v in st_a)
    assert qam_at_init > 0 and n_qam[0] == qam_at_init                 # the QAM report handler went too
    _, cont_b = oracle_stream(cls, rate, [a.samples(), b.samples()], [-45.5 if pfx == "v29_rx" else None])
    assert not np.array_equal(cont_b, want_b)


@pytest.mark.parametrize("pfx,ocls,rate,gold", [("v29_rx", "V29", 9600, "v29_9600"), ("v17_rx", "V17", 14400, "v17_14400")])
def test_modem_private_reinit_forgets_saved_training(L, pfx, ocls, rate, gold):
    """What tells an init from a restart: the training a receiver saves when it completes (equaliser, carrier, AGC) survives
    a restart, and a later v29_rx_restart(s, rate, old_train = 1) / v17_rx_restart(s, rate, short_train = 1) resumes from
    it.  After xxx_rx_init(s, ...) there is nothing saved: the receiver must behave as a fresh one does after the same
    restart."""
    from oracle import restated as orc
    from oracle.restated import lib as olib
    use_golden_modem_tables()
    x = i16(np.load(os.path.join(GOLDEN, gold + ".npz"))["amp"])
    ev = []
    cb = PUT_BIT(lambda u, b: ev.append(b))
    s = getattr(L, pfx + "_init")(None, rate, cb, None)
    for k in range(0, len(x), FRAME):
        assert getattr(L, pfx)(s, x[k:k + FRAME].ctypes.data, len(x[k:k + FRAME])) == 0
    assert len(ev) > 1000                                              # call A trained
    assert getattr(L, pfx + "_init")(s, rate, cb, None) == s
    assert getattr(L, pfx + "_restart")(s, rate, 1) == 0
    ev.clear()
    for k in range(0, len(x), FRAME):
        assert getattr(L, pfx)(s, x[k:k + FRAME].ctypes.data, len(x[k:k + FRAME])) == 0
    getattr(L, pfx + "_free")(s)

    def oracle(feed_a, restart_between):
        o = getattr(orc, ocls)(rate)
        if feed_a:
            o.rx(x)
        n0 = len(o.sink.events())
        if restart_between:
            (olib().orc_v29_restart(o.p, rate, 0) if pfx == "v29_rx" else o.restart(rate, 0))
        assert (olib().orc_v29_restart(o.p, rate, 1) if pfx == "v29_rx" else o.restart(rate, 1)) == 0
        o.rx(x)
        return o.sink.events()["a"].astype(np.int32)[n0:]
    want = oracle(False, False)
    assert np.array_equal(np.array(ev, np.int32), want)
    assert not np.array_equal(oracle(True, True), want)                # a restart in place of the init would answer otherwise


def test_v29_private_reinit_at_another_rate(L):
    """v29_rx_init(s, 4800, ...) on a 9600 object that has run: a fresh 4800 receiver."""
    from oracle import restated as orc
    use_golden_modem_tables()
    x96 = np.load(os.path.join(GOLDEN, "v29_9600.npz"))["amp"]
    x48 = np.load(os.path.join(GOLDEN, "v29_4800.npz"))
    ev = []
    cb = PUT_BIT(lambda u, b: ev.append(b))
    s = L.v29_rx_init(None, 9600, cb, None)
    for k in range(0, 4000, FRAME):
        L.v29_rx(s, i16(x96[k:k + FRAME]).ctypes.data, FRAME)
    L.v29_rx_set_signal_cutoff(s, -45.5)
    ev.clear()
    assert L.v29_rx_init(s, 4800, cb, None) == s
    y = i16(x48["amp"])
    for k in range(0, len(y), FRAME):
        assert L.v29_rx(s, y[k:k + FRAME].ctypes.data, len(y[k:k + FRAME])) == 0
    L.v29_rx_free(s)
    assert np.array_equal(np.array(ev, np.int32), x48["events"].astype(np.int32))


# ---- DTMF ---------------------------------------------------------------------------------------------------------
def dtmf_words(L, grp, channel):
    f = np.zeros(64, np.float32)
    w = np.zeros(4, np.int32)
    nf = L.spangpu_bank_get_state(L.spangpu_group_bank(grp), channel, f.ctypes.data, 64, w.ctypes.data, 4)
    assert nf > 0
    return np.concatenate([f[:nf].view(np.uint32), w.view(np.uint32)])


def test_dtmf_group_slot_reuse_restores_channel_parameters(L):
    """A DTMF object that set its own threshold, twists and dial-tone filter (dtmf_rx_parms()) is freed mid-digit; the
    object attached to its slot, and an attached object re-initialised with dtmf_rx_init(s, ...), detect with the group's
    parameters, as a fresh detector does."""
    from oracle import restated as orc
    from spandsp_amd import engine
    use_golden_modem_tables()           # (the oracle's tone generators)
    n_ch = 24
    ticks = 70
    sig, _ = synth.dtmf_channels(n_ch, FRAME*ticks, seed=71)
    # call B: quiet digits (-35 dBm0 a tone) that a detector left at a -20 dBm0 threshold would miss
    gen = orc.DtmfTx()
    gen.set_level(-35, 0)
    gen.put("1234567890*#ABCD")
    quiet = gen.tx(FRAME*ticks)
    assert np.abs(quiet).max() > 0
    parms = (1, 2.0, 2.0, -20.0)

    def a_free(obj):
        L.dtmf_rx_parms(obj, *parms)

    slots = []
    for c in range(n_ch):
        if c % 4 == 1:
            t_free = 9 + c % 7                      # call A is mid-digit (or between digits) when it is freed
            slots.append([Call(sig[c], 0, t_free, before_free=a_free), Call(quiet, t_free + (c % 8 == 5))])
        elif c % 8 == 2:
            slots.append([Call(np.zeros(0))])
        elif c % 8 == 6:
            slots.append([Call(sig[c], 7)])
        else:
            slots.append([Call(sig[c])])
    grp = L.spangpu_group_create(0, engine.DTMF, n_ch, FRAME, None)
    assert grp
    fresh = L.spangpu_group_create(0, engine.DTMF, 1, FRAME, None)
    pristine = dtmf_words(L, fresh, 0)
    L.spangpu_group_destroy(fresh)
    attach_words = {}

    def attach(c, call):
        cb = DIGITS_CB(lambda u, d, n: call.ev.append(d[:n].decode("latin1")))
        call.keep.append(cb)
        return L.spangpu_dtmf_rx_attach(grp, c, cb, None)

    def on_attach(c, call):
        attach_words[(c, call.t0)] = dtmf_words(L, grp, c)

    drive(slots, ticks, attach, lambda o, fr: L.dtmf_rx(o, fr.ctypes.data, FRAME), L.dtmf_rx_free,
          lambda: L.spangpu_group_flush(grp), on_attach)

    for key, w in attach_words.items():
        assert np.array_equal(w, pristine), key

    def oracle_digits(parts, set_parms_after_first=False):
        o = orc.Dtmf(1)
        out = []
        for i, p in enumerate(parts):
            o.rx(p)
            out.append(o.sink.text())
            if i == 0 and set_parms_after_first:
                o.parms(*parms)
        return out[0], out[-1][len(out[0]):]

    n_reused = 0
    for c, calls in enumerate(slots):
        if len(calls) == 1:
            assert "".join(calls[0].ev) == oracle_digits([calls[0].samples()])[0], c
            continue
        a, b = calls
        assert "".join(a.ev) == oracle_digits([a.samples()])[0], c
        want_b = oracle_digits([b.samples()])[0]
        assert "".join(b.ev) == want_b, (c, "".join(b.ev), want_b)
        assert len(want_b) >= 8
        _, cont_b = oracle_digits([a.samples(), b.samples()], True)
        assert cont_b != want_b, c
        n_reused += 1
    assert n_reused == n_ch//4

    # dtmf_rx_init(s, ...) on an attached object that set its own parameters: the group's parameters again
    g2 = L.spangpu_group_create(0, engine.DTMF, 2, FRAME, None)
    got = []
    cb = DIGITS_CB(lambda u, d, n: got.append(d[:n].decode("latin1")))
    cb_other = DIGITS_CB(lambda u, d, n: None)
    s0 = L.spangpu_dtmf_rx_attach(g2, 0, cb, None)
    s1 = L.spangpu_dtmf_rx_attach(g2, 1, cb_other, None)
    for k in range(10):
        for s, x in ((s0, sig[1]), (s1, sig[2])):
            assert L.dtmf_rx(s, i16(x[k*FRAME:(k + 1)*FRAME]).ctypes.data, FRAME) == 0
    L.dtmf_rx_parms(s0, *parms)
    assert L.dtmf_rx_init(s0, cb, None) == s0
    assert np.array_equal(dtmf_words(L, g2, 0), pristine)
    got.clear()
    for k in range(ticks):
        for s, x in ((s0, quiet), (s1, sig[2])):
            assert L.dtmf_rx(s, i16(x[k*FRAME:(k + 1)*FRAME]).ctypes.data, FRAME) == 0
    L.dtmf_rx_free(s0)
    L.dtmf_rx_free(s1)
    L.spangpu_group_destroy(g2)
    want = oracle_digits([quiet[:ticks*FRAME]])[0]
    assert "".join(got) == want and len(want) >= 8
    L.spangpu_group_destroy(grp)


TONE_CASES = {
    # name: (group kind attribute of engine, r2_fwd)
    "bell_mf": ("BELL_MF", None),
    "r2_fwd": ("R2_MF", True),
    "r2_back": ("R2_MF", False),
}


@pytest.mark.parametrize("name", list(TONE_CASES))
def test_mf_group_slot_reuse(L, name):
    """Bell MF and R2 MF (forward and backward) groups: detectors freed mid-digit, a new detector on the slot in the same
    tick or the next: a fresh detector's callbacks, and the channel's words right after the attach are a new group's."""
    import ctypes
    from oracle import restated as orc
    from spandsp_amd import engine
    kind_name, fwd = TONE_CASES[name]
    kind = getattr(engine, kind_name)
    n_ch, ticks = 18, 100
    if fwd is None:
        sig, _ = synth.bell_mf_channels(n_ch, FRAME*ticks, seed=61)
    else:
        sig, _ = synth.r2_mf_channels(n_ch, FRAME*ticks, seed=63, fwd=fwd)
    params = engine.ToneParams()
    params.r2_fwd = int(bool(fwd))
    pp = ctypes.addressof(params)

    def new_oracle():
        return orc.BellMf(1) if fwd is None else orc.R2Mf(fwd, True)

    def oracle(parts):
        o = new_oracle()
        out, n0 = [], 0
        for p in parts:
            for k in range(0, len(p), FRAME):
                o.rx(p[k:k + FRAME])
            ev = list(o.sink.text()) if fwd is None else [tuple(int(x) for x in e)[1:] for e in o.sink.events()]
            out.append(ev[n0:])
            n0 = len(ev)
        return out

    def pad(x, n):
        out = np.zeros(n, np.int16)
        out[:min(len(x), n)] = x[:n]
        return out

    slots = []
    for c in range(n_ch):
        if c % 3 == 1:
            # call B goes on with the line's signal where A stopped (a digit A has reported may still be on); the first
            # free tick at which a detector carried on from A would answer call B otherwise
            gap = c % 2
            for t_free in range(12, ticks//2):
                a = pad(sig[c], t_free*FRAME)
                b = pad(sig[c][(t_free + gap)*FRAME:], (ticks - t_free - gap)*FRAME)
                if oracle([a, b])[1] != oracle([b])[0]:
                    slots.append([Call(sig[c], 0, t_free), Call(sig[c][(t_free + gap)*FRAME:], t_free + gap)])
                    break
            else:
                slots.append([Call(sig[c])])        # (a line on which no timing tells the two apart)
        elif c % 6 == 3:
            slots.append([Call(np.zeros(0))])
        elif c % 6 == 5:
            slots.append([Call(sig[c], 8)])
        else:
            slots.append([Call(sig[c])])
    grp = L.spangpu_group_create(0, kind, n_ch, FRAME, pp)
    fresh = L.spangpu_group_create(0, kind, 1, FRAME, pp)
    assert grp and fresh
    pristine = dtmf_words(L, fresh, 0)
    L.spangpu_group_destroy(fresh)
    attach_words = {}

    def attach(c, call):
        if fwd is None:
            cb = DIGITS_CB(lambda u, d, n: call.ev.extend(d[:n].decode("latin1")))
            call.keep.append(cb)
            return L.spangpu_bell_mf_rx_attach(grp, c, cb, None)
        cb = REPORT(lambda u, code, lvl, delay: call.ev.append((code, lvl, delay)))
        call.keep.append(cb)
        return L.spangpu_r2_mf_rx_attach(grp, c, cb, None)

    def on_attach(c, call):
        attach_words[(c, call.t0)] = dtmf_words(L, grp, c)

    rx = L.bell_mf_rx if fwd is None else L.r2_mf_rx
    drive(slots, ticks, attach, lambda o, fr: rx(o, fr.ctypes.data, FRAME),
          L.bell_mf_rx_free if fwd is None else L.r2_mf_rx_free, lambda: L.spangpu_group_flush(grp), on_attach)
    L.spangpu_group_destroy(grp)
    for key, w in attach_words.items():
        assert np.array_equal(w, pristine), key
    n_reused = 0
    for c, calls in enumerate(slots):
        for call in calls:
            assert call.ev == oracle([call.samples()])[0], (name, c, call.t0)
        if len(calls) == 2:
            a, b = calls
            want_b = oracle([b.samples()])[0]
            assert oracle([a.samples(), b.samples()])[1] != want_b, (name, c)
            n_reused += 1
    assert n_reused >= 3


# ---- FSK and connect tones ----------------------------------------------------------------------------------------
def spec_ptr(L, which):
    arr = (FskSpec*11).in_dll(L, "preset_fsk_specs")
    return C.addressof(arr) + which*C.sizeof(FskSpec)


FSK_CASES = {
    # name: (preset, framing mode, signal parameters for synth.fsk_channels)
    "v21ch2_sync": (1, 1, (1850, 1650, 30000)),
    "v23ch1_async": (2, 0, (2100, 1300, 120000)),
    "v21ch2_framed": (1, 2, (1850, 1650, 30000)),
}


@pytest.mark.parametrize("name", list(FSK_CASES))
def test_fsk_group_slot_reuse(L, name):
    """FSK group: objects freed mid-signal after a cutoff change (framed mode: and new frame parameters) and with a status
    handler, a new object on the slot in the same tick or the next: a fresh receiver's bit stream, neighbours untouched."""
    from oracle import restated as orc
    which, mode, (f0, f1, baud) = FSK_CASES[name]
    framed = (mode == 2)
    n_ch, ticks = 16, 60
    sig = synth.fsk_channels(n_ch, FRAME*ticks, 931, f0, f1, baud, framed=framed)
    sig_b = synth.fsk_channels(n_ch, FRAME*ticks, 932, f0, f1, baud, framed=framed)
    cutoff = -20.0
    frame_parms = (7, 1, 2)

    def a_free(obj):
        L.fsk_rx_set_signal_cutoff(obj, cutoff)
        if framed:
            L.fsk_rx_set_frame_parameters(obj, *frame_parms)

    def a_setup(obj, call):
        st = STATUS(lambda u, v: call.ev.append(v))
        call.keep.append(st)
        L.fsk_rx_set_modem_status_handler(obj, st, None)

    slots = []
    for c in range(n_ch):
        if c % 3 == 1:
            t_free = 11 + 3*(c % 5)
            a = Call(sig[c], 0, t_free, before_free=a_free)
            a.setup = lambda o, a=a: a_setup(o, a)
            slots.append([a, Call(sig_b[c], t_free + (c % 2))])
        elif c % 8 == 3:
            slots.append([Call(np.zeros(0))])
        elif c % 8 == 5:
            slots.append([Call(sig[c], 6)])
        else:
            slots.append([Call(sig[c])])
    grp = L.spangpu_fsk_group_create(0, spec_ptr(L, which), mode, n_ch, FRAME)
    assert grp

    def attach(c, call):
        cb = PUT_BIT(lambda u, b: call.ev.append(b))
        call.keep.append(cb)
        return L.spangpu_fsk_rx_attach(grp, c, cb, None)

    drive(slots, ticks, attach, lambda o, fr: L.fsk_rx(o, fr.ctypes.data, FRAME), L.fsk_rx_free,
          lambda: L.spangpu_line_group_flush(grp))
    L.spangpu_line_group_destroy(grp)

    def oracle(parts, cut_after_first=False):
        o = orc.Fsk(which, mode)
        out, n0 = [], 0
        for i, p in enumerate(parts):
            o.rx(p)
            ev = [int(e["a"]) for e in o.sink.events()]
            out.append(ev[n0:])
            n0 = len(ev)
            if i == 0 and cut_after_first:
                o.set_signal_cutoff(cutoff)
                if framed:
                    o.set_frame_parameters(*frame_parms)
        return out

    n_diff = 0
    for c, calls in enumerate(slots):
        for call in calls:
            assert call.ev == oracle([call.samples()])[0], (name, c, call.t0)
        if len(calls) == 2:
            a, b = calls
            want_b = oracle([b.samples()])[0]
            assert len(want_b) > (10 if framed else 50)
            cont_b = oracle([a.samples(), b.samples()], True)[1]
            assert cont_b != want_b, (name, c)
            n_diff += 1
    assert n_diff > 0


MCT_CASES = {
    # name: (tone type, synth kind)
    "ans": (2, "ans"),
    "preamble": (6, "preamble"),
}


@pytest.mark.parametrize("name", list(MCT_CASES))
def test_connect_tones_group_slot_reuse(L, name):
    """Connect tone group: detectors freed mid-tone, a new detector on the slot: a fresh detector's reports."""
    from oracle import restated as orc
    tone_type, kind = MCT_CASES[name]
    n_ch, ticks = 16, 170
    sig = synth.connect_tone_channels(n_ch, FRAME*ticks, 941, kind)
    sig_b = synth.connect_tone_channels(n_ch, FRAME*ticks, 942, kind)
    slots = []
    for c in range(n_ch):
        if c % 3 == 1:
            t_free = 60 + 5*(c % 4)            # call A has reported its tone and it is still on
            slots.append([Call(sig[c], 0, t_free), Call(sig_b[c], t_free + (c % 2))])
        elif c % 8 == 3:
            slots.append([Call(np.zeros(0))])
        elif c % 8 == 5:
            slots.append([Call(sig[c], 9)])
        else:
            slots.append([Call(sig[c])])
    grp = L.spangpu_modem_connect_tones_group_create(0, tone_type, 1, n_ch, FRAME)
    assert grp

    def attach(c, call):
        cb = REPORT(lambda u, t, lvl, d: call.ev.append((t, lvl)))
        call.keep.append(cb)
        return L.spangpu_modem_connect_tones_rx_attach(grp, c, cb, None)

    drive(slots, ticks, attach, lambda o, fr: L.modem_connect_tones_rx(o, fr.ctypes.data, FRAME),
          L.modem_connect_tones_rx_free, lambda: L.spangpu_line_group_flush(grp))
    L.spangpu_line_group_destroy(grp)

    def oracle(parts):
        o = orc.Mct(tone_type)
        out, n0 = [], 0
        for p in parts:
            for k in range(0, len(p), FRAME):
                o.rx(p[k:k + FRAME])
            ev = [(int(e["a"]), int(e["b"])) for e in o.sink.events()]
            out.append(ev[n0:])
            n0 = len(ev)
        return out

    n_reused = 0
    for c, calls in enumerate(slots):
        for call in calls:
            assert call.ev == oracle([call.samples()])[0], (name, c, call.t0)
        if len(calls) == 2:
            a, b = calls
            want_b = oracle([b.samples()])[0]
            assert oracle([a.samples(), b.samples()])[1] != want_b, (name, c)
            n_reused += 1
    assert n_reused == len([c for c in range(n_ch) if c % 3 == 1])


@pytest.mark.parametrize("name", ["fsk", "mct"])
def test_line_private_reinit_in_place(L, name):
    """fsk_rx_init(s, ...) / modem_connect_tones_rx_init(s, ...) on caller storage whose previous object has run and been
    released (xxx_rx_release(): its private bank goes; the init then memset()s the storage, as the reference does): a fresh
    receiver."""
    from oracle import restated as orc
    ticks = 60
    if name == "fsk":
        x = synth.fsk_channels(2, FRAME*ticks, 951, 1850, 1650, 30000)
        init = lambda s, cb: L.fsk_rx_init(s, spec_ptr(L, 1), 1, cb, None)
        rx, free, release, mk = L.fsk_rx, L.fsk_rx_free, L.fsk_rx_release, PUT_BIT
        fresh = orc.Fsk(1, 1)
        size = 4096
    else:
        x = synth.connect_tone_channels(2, FRAME*ticks, 952, "ans")
        init = lambda s, cb: L.modem_connect_tones_rx_init(s, 2, cb, None)
        rx, free, release, mk = L.modem_connect_tones_rx, L.modem_connect_tones_rx_free, L.modem_connect_tones_rx_release, REPORT
        fresh = orc.Mct(2)
        size = 4096
    got = []
    cb = mk(lambda u, *a: got.append(a[:2] if name == "mct" else a[0]))
    storage = C.create_string_buffer(size)
    s = init(C.addressof(storage), cb)
    assert s
    a = i16(x[0][:FRAME*25])
    assert rx(s, a.ctypes.data, len(a)) == 0
    assert release(s) == 0
    s2 = init(C.addressof(storage), cb)
    assert s2 == s
    got.clear()
    b = i16(x[1])
    for k in range(0, len(b), FRAME):
        assert rx(s, b[k:k + FRAME].ctypes.data, FRAME) == 0
        fresh.rx(b[k:k + FRAME])
    want = [(int(e["a"]), int(e["b"])) if name == "mct" else int(e["a"]) for e in fresh.sink.events()]
    assert got == want and len(want) > 0
    free(s)


# ---- concurrent attach --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["modem", "fsk", "mct", "dtmf"])
def test_concurrent_attach_of_one_slot(L, family):
    """Two threads attach the same free slot at the same moment, on a fresh group each time: exactly one attach succeeds,
    and the group then runs its ticks by itself once every slot has staged (a second frame on a slot is accepted, which
    it would not be before the tick ran)."""
    from spandsp_amd import engine
    cb_bit = PUT_BIT(lambda u, b: None)
    cb_rep = REPORT(lambda u, t, lvl, d: None)
    cb_dig = DIGITS_CB(lambda u, d, n: None)
    if family == "modem":
        mk = lambda: L.spangpu_modem_group_create(0, engine.V29, 2, 9600, FRAME)
        att = lambda g, c: L.spangpu_v29_rx_attach(g, c, cb_bit, None)
        rx, free, destroy = L.v29_rx, L.v29_rx_free, L.spangpu_modem_group_destroy
    elif family == "fsk":
        mk = lambda: L.spangpu_fsk_group_create(0, spec_ptr(L, 1), 1, 2, FRAME)
        att = lambda g, c: L.spangpu_fsk_rx_attach(g, c, cb_bit, None)
        rx, free, destroy = L.fsk_rx, L.fsk_rx_free, L.spangpu_line_group_destroy
    elif family == "mct":
        mk = lambda: L.spangpu_modem_connect_tones_group_create(0, 2, 1, 2, FRAME)
        att = lambda g, c: L.spangpu_modem_connect_tones_rx_attach(g, c, cb_rep, None)
        rx, free, destroy = L.modem_connect_tones_rx, L.modem_connect_tones_rx_free, L.spangpu_line_group_destroy
    else:
        mk = lambda: L.spangpu_group_create(0, engine.DTMF, 2, FRAME, None)
        att = lambda g, c: L.spangpu_dtmf_rx_attach(g, c, cb_dig, None)
        rx, free, destroy = L.dtmf_rx, L.dtmf_rx_free, L.spangpu_group_destroy
    fr = np.zeros(FRAME, np.int16)
    for _ in range(40):
        g = mk()
        assert g
        other = att(g, 1)
        assert other
        res = [None, None]
        bar = threading.Barrier(2)

        def go(i):
            bar.wait()
            res[i] = att(g, 0)
        ts = [threading.Thread(target=go, args=(i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        won = [r for r in res if r]
        assert len(won) == 1, res
        for _tick in range(2):
            assert rx(won[0], fr.ctypes.data, FRAME) == 0
            assert rx(other, fr.ctypes.data, FRAME) == 0    # the last one of the tick runs it
        free(won[0])
        free(other)
        destroy(g)
