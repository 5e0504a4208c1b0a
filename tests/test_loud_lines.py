"""The oracle on lines at and beyond full scale (tests/loud_lines.py), pinned as everything else is: live against the
reference build where it is present, and against tests/golden/loud_lines.npz (written from that build by
tests/golden/make_golden_loud.py) everywhere.  The GPU parity tests of tests/test_loud_lines_gpu.py take their
expectations from the oracle on exactly these lines and configurations.

The reach conditions at the end keep those tests from passing on lines that have gone tame: they look at what the
reference made of the lines (the fixture), never at a bank.
"""
import numpy as np
import pytest

import loud_lines as ll
from test_oracle_pin import needs_ref


@pytest.fixture(scope="module")
def golden(built):
    g = ll.load()
    assert np.array_equal(ll.line_crcs(), g["line_crcs"]), "the lines generated here are not the fixture's"
    return ll.unpack(g)


def family(cases, name):
    return {k: v for k, v in cases.items() if k.startswith(name + "/")}


def test_the_lines_are_loud_and_deterministic(built):
    named = list(ll.lines()) + [x for k in ll.TONE_KINDS for x in ll.tone_lines(k)]
    assert len(ll.lines()) == 17 and len({n for n, _ in named}) == len(named)
    for name, x in named:
        assert x.dtype == np.int16 and x.shape == (ll.N,), name
        assert np.abs(x.astype(np.int32)).max() >= 32767, name
    for name, tx, rx in ll.echo_pairs():
        assert tx.shape == rx.shape == (ll.N,) and np.abs(tx.astype(np.int32)).max() >= 32767, name
    ll.lines.cache_clear()
    ll.echo_pairs.cache_clear()
    again = list(ll.lines())
    assert all(np.array_equal(a, b) for (_, a), (_, b) in zip(named, again))
    # no two channels of a bank in step: the rotations of the channels that share a line differ
    r = ll.rows([x for _, x in ll.lines()], 70)
    assert len({ll.offset(c) for c in range(70)}) == 70
    assert np.array_equal(r[17], np.roll(ll.lines()[0][1], -ll.offset(17)))


# ---- live pins -----------------------------------------------------------------------------------------------------------
def both(run, *args):
    a = run(ll.makers("ref"), *args)
    b = run(ll.makers("orc"), *args)
    return ll.same(a, b)


@needs_ref
@pytest.mark.parametrize("cfg", ll.SIGRX_CONFIGS, ids=lambda c: "%d_%02x" % c)
def test_sigtone_rx_live(built, cfg):
    for name, x in ll.pinned_rows("sigrx"):
        assert both(ll.run_sigrx, cfg, x) is None, name


@needs_ref
@pytest.mark.parametrize("tone_type", ll.SIGTX_TYPES)
def test_sigtone_tx_live(built, tone_type):
    for k, (name, x) in enumerate(ll.pinned_rows("sigtx")):
        assert both(ll.run_sigtx, tone_type, k, x) is None, name


@needs_ref
@pytest.mark.parametrize("cfg", ll.MCT_CONFIGS, ids=lambda c: "%d_%s" % (c[0], "callback" if c[1] else "latch"))
def test_mct_live(built, cfg):
    for name, x in ll.pinned_rows("mct"):
        assert both(ll.run_mct, cfg, x) is None, name


@needs_ref
@pytest.mark.parametrize("cfg", ll.FSK_CONFIGS, ids=lambda c: "%d_%d" % c)
def test_fsk_live(built, cfg):
    for name, x in ll.pinned_rows("fsk"):
        assert both(ll.run_fsk, cfg, x) is None, name


@needs_ref
@pytest.mark.parametrize("cfg", ll.ECHO_CONFIGS, ids=lambda c: "%d_%02x_%d" % (c[0], c[1], int(c[2])))
def test_echo_live(built, cfg):
    for name, tx, rx in ll.pinned_echo_rows():
        assert both(ll.run_echo, cfg, tx, rx) is None, name


@needs_ref
@pytest.mark.parametrize("cfg", ll.TONE_CONFIGS, ids=lambda c: "%s_%d" % c)
def test_tone_live(built, cfg):
    for name, x in ll.pinned_rows(cfg[0]):
        assert both(ll.run_tone, cfg, x) is None, name


@needs_ref
def test_fixture_is_what_the_reference_gives_now(built, tmp_path):
    """the recipe, run again: the same members with the same bytes in them (and, the compression library being the same,
    the same file)"""
    path = str(tmp_path/"loud_lines.npz")
    ll.write_archive(path, ll.pack(ll.all_cases(ll.makers("ref"))))
    a, b = np.load(path), ll.load()
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


# ---- the frozen pin ------------------------------------------------------------------------------------------------------
def test_golden_loud_lines(built, golden):
    got = ll.all_cases(ll.makers("orc"))
    assert sorted(got) == sorted(golden)
    for k in sorted(got):
        assert ll.same(got[k], golden[k]) is None, (k, ll.same(got[k], golden[k]))


# ---- reach conditions: what the reference made of the lines ----------------------------------------------------------------
def test_reach_sigtone_rx(golden):
    cases = family(golden, "sigrx")
    for t in (1, 2, 3):
        rails = {k: int(v["sums"][2]) for k, v in cases.items() if k.startswith("sigrx/%d_c0/" % t)}
        assert max(rails.values()) >= 100, (t, rails)
        reports = {k: len(v["reports"]) for k, v in cases.items() if k.startswith("sigrx/%d_" % t) and "/gated" in k}
        assert max(reports.values()) >= 4, (t, reports)
        print("sig-tone rx type %d: most samples left on a rail %d, most reports on a gated line %d"
              % (t, max(rails.values()), max(reports.values())))
    for k, v in cases.items():
        assert int(v["sums"][1]) == ll.N, k
        if "_00/" in k:
            assert int(v["sums"][2]) == 0, k              # the muted media path leaves zeros


def test_reach_sigtone_tx(golden):
    for t in ll.SIGTX_TYPES:
        rails = [int(v["sums"][3]) for k, v in family(golden, "sigtx").items() if k.startswith("sigtx/%d/" % t)]
        requests = [int(v["sums"][2]) for k, v in family(golden, "sigtx").items() if k.startswith("sigtx/%d/" % t)]
        assert max(rails) > 0 and min(requests) >= 10, (t, rails, requests)
        print("sig-tone tx type %d: most samples driven onto a rail %d" % (t, max(rails)))


def test_reach_connect_tones(golden):
    cases = family(golden, "mct")
    for t in (1, 2, 3, 4, 7):
        told = [k for k, v in cases.items() if k.startswith("mct/%d_1/" % t) and np.any(v["reports"][:, 0] != 0)]
        latched = [k for k, v in cases.items() if k.startswith("mct/%d_0/" % t) and v["hits"].any()]
        assert told and latched, (t, told, latched)
        print("connect tones type %d: reports on %s" % (t, [k.split("/")[2] for k in told]))
    for k, v in cases.items():
        if k.split("/")[2] in ll.FOREIGN_TO_CONNECT_TONES:
            assert len(v["reports"]) == 0 and not v["hits"].any(), k
    gated = cases["mct/1_1/gated1100"]["reports"]
    assert len(gated) >= 2 and gated[-1][0] == 0          # declared and withdrawn as the tone comes and goes


def test_reach_fsk(golden):
    from oracle import restated as orc
    cases = family(golden, "fsk")
    for which, mode in ll.FSK_CONFIGS:
        if mode == 2:
            # a framed receiver delivers characters, and noise frames none: some line must
            most = max(int(v["sums"][0]) for k, v in cases.items() if k.startswith("fsk/%d_2/" % which))
            assert most >= 10, (which, most)
            continue
        # 100 events on the noise line, or half the bits two seconds hold at the preset's rate where that is fewer
        # (75 and 45.45 baud: 150 and 90 bits)
        bits = ll.N*int(orc.fsk_preset(which)[4])//(100*8000)
        n = int(cases["fsk/%d_%d/noise" % (which, mode)]["sums"][0])
        assert n >= min(100, bits//2), (which, mode, n, bits)
        print("fsk preset %d mode %d: %d events on the noise line" % (which, mode, n))


def test_reach_echo(golden):
    from oracle import ref
    cases = family(golden, "echo")
    field = {k: i for i, k in enumerate(ref.ECHO_FIELDS)}
    rails = {k: int(v["sums"][5]) for k, v in cases.items() if "_67_" in k}
    assert max(rails.values()) >= 50, rails
    big = {k: int(v["sums"][6]) for k, v in cases.items()}
    assert max(big.values()) > 100000000, max(big.values())
    third = [k for k, v in cases.items() if int(v["final"][field["tap_set"]]) == 2]
    assert any("/tone1000" in k for k in third), third
    for k, v in cases.items():
        taps, mode, _ = k.split("/")[1].split("_")
        if mode in ("00", "06"):
            assert int(v["sums"][6]) == 0, k
    print("echo: most clean samples on a rail in mode 0x67 %d, largest |tap| %d, %d cases end on the third tap set"
          % (max(rails.values()), max(big.values()), len(third)))


def test_reach_tone_banks(golden):
    for kind in ("dtmf", "bell"):
        assert any(len(v["digits"]) >= 4 for k, v in family(golden, kind).items() if "_x8" in k), kind
    for kind in ("r2f", "r2b", "st"):
        assert max(int(v["sums"][0]) for v in family(golden, kind).values()) >= 4, kind
