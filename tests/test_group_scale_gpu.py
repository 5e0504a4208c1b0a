"""Slot churn on a shared group at bank scale: tests/c_callers/group_churn.c drives 65 536 DTMF or 16 384 V.29 9600
receivers of one group from 16 threads, with objects freed and new ones attached (new calls) while other threads stage,
per-object settings changed, ticks sat out, short frames, and refused second frames.  Channel c plays base signal c % R on
schedule c % R (R = 97, coprime to 64: the replicas of a class fall on different lanes and workgroups), so

  * every channel's (event count, hash of (call, event)) must equal that of every other channel of its class;
  * a sample of channels (every 128th, and every churned one among the first 2048) is replayed on the oracle, one fresh
    oracle per call;
  * no xxx_rx() result is unexpected (0, or -1 for the scheduled second frame of a tick that has not run).

The driver prints the wall time per tick (reported, not judged).  A separate mode races four threads attaching the same
free slot of a fresh modem / FSK / connect-tone group, many times over: exactly one must win, and the group must then
run its ticks by itself."""
import os
import subprocess

import numpy as np
import pytest

import synth
from test_oracle_pin import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_callers", "group_churn.c")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "spandsp_amd")
FRAME, SHORT = 160, 80
STAGE, SHORT_FRAME, SKIP, SETTING, NEW_CALL, SECOND = range(6)
R = 97
THREADS = 16


def build(out_dir):
    obj = os.path.join(out_dir, "group_churn.o")
    exe = os.path.join(out_dir, "group_churn")
    for cmd in (["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + INC, "-c", SRC, "-o", obj],
                ["gcc", "-o", exe, obj, "-L" + LIBDIR, "-lspangpu", "-pthread", "-Wl,-rpath," + LIBDIR]):
        p = subprocess.run(cmd, capture_output=True, text=True)
        assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    return exe


def test_group_churn_builds_as_c99(built, tmp_path):
    build(str(tmp_path))


def schedule(ticks, seed):
    """One byte per class and tick.  Every third tick is a churn tick: some classes sit it out (so it is run by the owner's
    flush, and a second frame staged in it is refused for sure), about 1 % of the slots start a new call, some stage a
    second frame.  The other ticks have every channel stage (a full or a short frame, some after a setting change), and
    run from inside the last xxx_rx()."""
    rng = np.random.default_rng(seed)
    s = np.zeros((R, ticks), np.uint8)
    for k in range(1, ticks):
        if k % 3 == 2:
            col = rng.choice([STAGE, SKIP, SECOND, SETTING], R, p=[0.75, 0.1, 0.1, 0.05]).astype(np.uint8)
            col[rng.integers(R)] = SKIP
            for c in rng.choice(R, 1 + (k % 2), replace=False):
                col[c] = NEW_CALL
        else:
            col = rng.choice([STAGE, SHORT_FRAME, SETTING], R, p=[0.85, 0.1, 0.05]).astype(np.uint8)
        s[:, k] = col
    return s


def calls_of(sched_row, base):
    """The calls one channel of this class makes: a list of lists of ('rx', samples) / ('set',)."""
    calls = [[]]
    pos = 0
    for code in sched_row:
        if code == SKIP:
            continue
        if code == NEW_CALL:
            calls.append([])
        if code == SETTING:
            calls[-1].append(("set",))
        n = SHORT if code == SHORT_FRAME else FRAME
        calls[-1].append(("rx", base[pos:pos + n]))
        pos += n
    return calls


def run_churn(tmp_path, kind, n_ch, ticks, bases, sched, timeout):
    churned = {c for c in range(R) if (sched[c] == NEW_CALL).any()}
    logged = sorted(set(range(0, n_ch, 128)) | {c for c in range(min(n_ch, 2048)) if c % R in churned})
    inp = os.path.join(str(tmp_path), "in.bin")
    out = os.path.join(str(tmp_path), "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([kind, n_ch, ticks, R, THREADS, len(logged)], np.int32).tobytes())
        f.write(np.ascontiguousarray(sched, np.uint8).tobytes())
        f.write(np.ascontiguousarray(bases, np.int16).tobytes())
        f.write(np.array(logged, np.int32).tobytes())
    exe = build(str(tmp_path))
    p = subprocess.run([exe, "churn", inp, out], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    raw = open(out, "rb").read()
    stats = np.frombuffer(raw[:16*n_ch], np.dtype([("count", "<u4"), ("errors", "<u4"), ("hash", "<u8")]))
    tick_ms = np.frombuffer(raw[16*n_ch:16*n_ch + 8*ticks], np.float64)
    logs = {}
    off = 16*n_ch + 8*ticks
    for _ in logged:
        c, n = np.frombuffer(raw[off:off + 8], np.int32)
        off += 8
        logs[int(c)] = np.frombuffer(raw[off:off + 4*n], np.int32).reshape(-1, 2)
        off += 4*n
    print("%s; per-tick wall time: median %.3f ms, max %.3f ms (churn ticks: median %.3f ms)" % (
        p.stdout.strip(), np.median(tick_ms), tick_ms.max(), np.median(tick_ms[2::3])))
    assert (stats["errors"] == 0).all(), np.nonzero(stats["errors"])[0][:10]
    for cls in range(R):
        rep = stats[cls::R]
        assert (rep["count"] == rep["count"][0]).all() and (rep["hash"] == rep["hash"][0]).all(), cls
    assert len(churned) >= ticks//3
    return stats, logs


@pytest.mark.gpu
def test_dtmf_group_churn_at_bank_scale(built, tmp_path):
    from oracle import restated as orc
    n_ch, ticks = 65536, 60
    bases, _ = synth.dtmf_channels(R, FRAME*ticks, seed=171)
    sched = schedule(ticks, 172)
    stats, logs = run_churn(tmp_path, 0, n_ch, ticks, bases, sched, 600)
    n_digits = 0
    for c, log in logs.items():
        for call, ops in enumerate(calls_of(sched[c % R], bases[c % R])):
            o = orc.Dtmf(1)
            for op in ops:
                if op[0] == "set":
                    o.parms(-1, 6.0, 6.0, -36.0)
                else:
                    o.rx(op[1])
            got = "".join(chr(v) for v in log[log[:, 0] == call, 1])
            assert got == o.sink.text(), (c, call)
            n_digits += len(got)
    assert n_digits > len(logs)


@pytest.mark.gpu
def test_v29_group_churn_at_bank_scale(built, tmp_path):
    from oracle import restated as orc
    from test_oracle_pin import use_golden_modem_tables
    use_golden_modem_tables()
    n_ch, ticks = 16384, 40
    x = np.load(os.path.join(GOLDEN, "v29_9600.npz"))["amp"].astype(np.float64)
    rng = np.random.default_rng(181)
    bases = np.zeros((R, FRAME*ticks), np.int16)
    for c in range(R):
        lead = int(rng.integers(0, FRAME*ticks - len(x)))
        bases[c, lead:lead + len(x)] = np.round(x*rng.uniform(0.4, 1.0)).astype(np.int16)
    sched = schedule(ticks, 182)
    stats, logs = run_churn(tmp_path, 1, n_ch, ticks, bases, sched, 900)
    for c, log in logs.items():
        for call, ops in enumerate(calls_of(sched[c % R], bases[c % R])):
            o = orc.V29(9600)
            for op in ops:
                if op[0] == "set":
                    o.set_signal_cutoff(-40.0)
                else:
                    o.rx(op[1])
            got = log[log[:, 0] == call, 1]
            assert np.array_equal(got, o.sink.events()["a"].astype(np.int32)), (c, call, len(got))
    # the receivers trained: a class that never starts a new call delivers most of the page's 3900 bits
    calm = [c for c in range(R) if not (sched[c] == NEW_CALL).any()]
    assert calm and min(int(stats["count"][c]) for c in calm) > 2000


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["v29", "fsk", "mct"])
def test_concurrent_attach_race_in_c(built, tmp_path, what):
    exe = build(str(tmp_path))
    p = subprocess.run([exe, "race", what, "400"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and " 0 bad" in p.stdout, (p.returncode, p.stdout, p.stderr)
