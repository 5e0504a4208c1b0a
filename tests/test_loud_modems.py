"""The oracle's V.29, V.27ter and V.17 receivers on lines at and beyond full scale (tests/loud_modem_lines.py: the 17 lines of
tests/loud_lines.py and the modem's own transmission x8 and x40), at every bit rate, pinned as everything else is: live against
the reference build where it is present, and against tests/golden/loud_modems.npz (written from that build by
tests/golden/make_golden_loud_modems.py) everywhere.  tests/test_loud_modems_gpu.py takes its expectations from the oracle on
these lines.

A cold receiver on a foreign or railed line is what no modulator's own signal gives it: the carrier detector flapping (a
restart inside the receiver at every carrier down), training failed and the receiver PARKED, training that succeeds on a pure
tone.  The reach conditions at the end look at what the reference made of the lines (the fixture), never at the code under
test.  Seen there, at every rate of a modem alike unless said:

  minus_rail        V.29 191 carrier ups and 190 downs in 2 s; V.27ter and V.17 131 and 130
  impulses          V.29 63 and 62; V.27ter and V.17 54 and 53
  gated 2280, 2600, 2400+2600 Hz   20 cycles of carrier up, TRAINING_FAILED, carrier down; V.27ter 2400 on 2400+2600 Hz 20 of
                    up, TRAINING_IN_PROGRESS, down
  gated1100         2 cycles
  steady lines      one carrier up and one TRAINING_FAILED, PARKED at the end (V.29 on sine1100 and noise, V.27ter 2400 on
                    sine2400_2600 and fsk_bell202 by way of TRAINING_IN_PROGRESS); V.27ter 2400 trains on both 2100 Hz lines
                    and delivers 2 548 bits of them
  own_x8            trains everywhere; bits: V.29 15 644 / 11 736 / 7 824, V.27ter 5 538 / 2 180, V.17 6 966 / 5 805 / 4 644 /
                    3 483 / 2 350
  own_x40           fails everywhere but at V.27ter 4800, which trains and delivers 5 538 bits
  no state word is non-finite anywhere

No line had to be changed to meet a condition at any rate; the own lines carry 15 000 samples of transmission (V.17's long
train alone is some 11 150).

The lost-packet cases (xxx_rx_fillin) are the reference's alone -- the oracle has no fill-in -- so they are held live to the
fixture, and the oracle only where a fill-in must change nothing.
"""
import os

import numpy as np
import pytest

import loud_lines as ll
import loud_modem_lines as lm
from test_oracle_pin import needs_ref

RATE_IDS = [lm.rate_id(r) for r in lm.RATES]
# own_x8, 12 000 samples of transmission, through the reference: the bits it delivered
BITS_SEEN = {("v29", 9600): 12048, ("v29", 7200): 9036, ("v29", 4800): 6024, ("v27ter", 4800): 3738, ("v27ter", 2400): 1280,
             ("v17", 14400): 1566, ("v17", 7200): 783}


@pytest.fixture(scope="module")
def golden(built):
    lm.use_tables()
    g = lm.load()
    assert np.array_equal(lm.line_crcs(), g["line_crcs"]), "the lines generated here are not the fixture's"
    return ll.unpack(g)


def rx_case(golden, name, rate, line):
    return golden["rx/%s_%d/%s" % (name, rate, line)]


def test_the_modem_lines(built):
    lm.use_tables()
    for name, rate in lm.RATES:
        named = lm.modem_lines(name, rate)
        assert [n for n, _ in named] == [n for n, _ in ll.lines()] + ["own_x8", "own_x40"]
        for lname, x in named[17:]:
            assert x.dtype == np.int16 and x.shape == (ll.N,) and not x[:lm.OWN_LEAD].any(), lname
            assert np.count_nonzero(np.abs(x.astype(np.int32)) >= 32767) >= 100, (name, rate, lname)
        r = lm.modem_rows(name, rate, 70)
        assert np.array_equal(r[20], np.roll(named[1][1], -ll.offset(20)))             # a foreign line: rotated
        assert np.array_equal(r[36][36:], named[17][1][:-36]) and not r[36][:36].any()  # an own line: late by c mod 160
        assert np.array_equal(r[18][18:], named[18][1][:-18]) and lm.row_names(name, rate, 70)[36] == "own_x8"


# ---- live pins -----------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("name,rate", lm.RATES, ids=RATE_IDS)
def test_modem_rx_live(built, name, rate):
    """reference == oracle on every line: the events of every call, the float and integer words at the end"""
    lm.use_tables()
    for (lname, x), (_, y) in zip(lm.own_lines(name, rate), lm.own_lines(name, rate, "ref")):
        assert np.array_equal(x, y), lname              # the oracle's sender made the reference's transmission
    for lname, x in lm.modem_lines(name, rate):
        a = lm.run_modem(lm.receivers("ref"), name, rate, x)
        b = lm.run_modem(lm.receivers("orc"), name, rate, x)
        assert lm.same_run(a, b) is None, (lname, lm.same_run(a, b))


@needs_ref
def test_fixture_is_what_the_reference_gives_now(built, tmp_path):
    """the recipe, run again (the lost-packet cases with it): the same members with the same bytes in them"""
    lm.use_tables()
    path = str(tmp_path/"loud_modems.npz")
    ll.write_archive(path, lm.pack(lm.all_cases(lm.receivers("ref"), lm.ref_fillin)))
    a, b = np.load(path), lm.load()
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


# ---- the frozen pin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rate", lm.RATES, ids=RATE_IDS)
def test_golden_loud_modems(built, golden, name, rate):
    for lname, x in lm.modem_lines(name, rate):
        got = lm.compact_modem(lm.run_modem(lm.receivers("orc"), name, rate, x))
        want = rx_case(golden, name, rate, lname)
        assert ll.same(got, want) is None, (lname, ll.same(got, want))


@pytest.mark.parametrize("name,rate", lm.RATES, ids=RATE_IDS)
def test_golden_fillin_where_it_changes_nothing(built, golden, name, rate):
    """call 0 lost before any signal, and a call lost by a PARKED receiver: the reference's fill-in does nothing there, so
    the oracle with that call left out must give the reference's events and words"""
    pts = lm.fillin_points(lm.receivers("orc"), name, rate)
    for point in lm.FILLIN_POINTS:
        x, at, lost = pts[point]
        want = golden["fillin/%s_%d/%s" % (name, rate, point)]
        assert [at, lost] == [int(v) for v in want["at"]], point
        got = lm.run_fillin(lm.receivers("orc"), name, rate, x, at, lambda rx, n: None, lost)
        differ = [k for k in got if not np.array_equal(got[k], want[k])]
        if point in ("start", "parked"):
            assert not differ, (point, differ)
        else:
            # where it does something, it shows: the phases right after it are not those of the samples merely left out
            assert "iwords_after" in differ and "fwords_after" not in differ, (point, differ)


# ---- reach conditions: what the reference made of the lines ----------------------------------------------------------------
@pytest.mark.parametrize("name,rate", lm.RATES, ids=RATE_IDS)
def test_reach(golden, name, rate):
    def status(line):
        return [int(v) for v in rx_case(golden, name, rate, line)["status"]]

    def bits(line):
        return int(rx_case(golden, name, rate, line)["sums"][0])

    ups = status("minus_rail").count(-2), status("impulses").count(-2)
    assert ups[0] >= 100 and ups[1] >= 40, ups
    assert lm.cycles(status("minus_rail"), -2, -1) >= 100 and -5 not in status("minus_rail")
    gated = {g: max(lm.cycles(status(g), -2, -5, -1), lm.cycles(status(g), -2, -3, -1)) for g in lm.GATED}
    assert min(gated.values()) >= 15, gated
    assert status("own_x8")[:3] == [-2, -3, -4], status("own_x8")
    assert bits("own_x8") >= max(BITS_SEEN.get((name, rate), 0)//2, rate*1500//8000), bits("own_x8")
    if (name, rate) == ("v27ter", 2400):
        assert status("ans2100") == [-2, -3, -4] and bits("ans2100") >= 1000
    if (name, rate) == ("v27ter", 4800):
        assert status("own_x40")[:3] == [-2, -3, -4] and bits("own_x40") >= BITS_SEEN[(name, rate)]//2
    else:
        assert -5 in status("own_x40") and -4 not in status("own_x40")
    parked = []
    for line in lm.STEADY + ("ans2100", "ans2100_reversals"):
        if (name, rate) == ("v27ter", 2400) and line.startswith("ans2100"):
            continue
        s = status(line)
        assert s in ([-2, -5], [-2, -3, -5]), (line, s)
        assert int(rx_case(golden, name, rate, line)["iwords"][lm.STAGE]) == lm.PARKED[name], line
        parked.append(line)
    for lname, _ in lm.modem_lines(name, rate):
        assert lm.non_finite(rx_case(golden, name, rate, lname)["fwords"]) == 0, lname
    print("%s %d: carrier ups on minus_rail %d, impulses %d; gated cycles %s; %d lines PARKED; own_x8 %d bits, own_x40 %s"
          % (name, rate, ups[0], ups[1], sorted(gated.values()), len(parked), bits("own_x8"), status("own_x40")))


def test_reach_fillin(golden):
    """the lost packets fall where they are meant to: before the carrier, between TRAINING_IN_PROGRESS and
    TRAINING_SUCCEEDED, in the data, and behind a TRAINING_FAILED; a fill-in of 97 samples leaves the symbol phase elsewhere"""
    for name, rate in lm.RATES:
        clean = np.load(os.path.join(ll.HERE, "golden", "%s_%d.npz" % (name, rate)))["events"].astype(np.int8)
        case = {p: golden["fillin/%s_%d/%s" % (name, rate, p)] for p in lm.FILLIN_POINTS}
        at = {p: int(case[p]["at"][0]) for p in case}
        assert at["start"] == 0 < at["training"] < at["training_97"] < at["data"] < at["data_97"]
        for p in ("training", "data", "training_97", "data_97"):
            w = case[p]["iwords_after"]
            assert int(w[lm.SIGNAL_PRESENT]) > 0 and int(w[lm.STAGE]) != lm.PARKED[name], (name, rate, p)
            assert (int(w[lm.STAGE]) == 0) == p.startswith("data"), (name, rate, p, int(w[lm.STAGE]))
            assert not np.array_equal(case[p]["events"], clean), (name, rate, p)
        assert int(case["start"]["iwords_after"][lm.SIGNAL_PRESENT]) <= 0
        neg = case["parked"]["events"]
        assert [int(v) for v in neg[neg < 0]] == [-2, -5] and int(case["parked"]["iwords_after"][lm.STAGE]) == lm.PARKED[name]
