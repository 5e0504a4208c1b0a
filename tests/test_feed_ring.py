"""The slot ring of the pipelined feeds and their one tick loop (spandsp_amd/csrc/feed_ring.hpp), on the host.

tests/c_callers/feed_ring.cpp includes that header alone and is built under -fsanitize=address,undefined (host code only, a
program of its own).  It runs ring_run() at every depth 1 .. 8 with every lag 1 .. depth - 1 and ticks in {1, depth - 1, depth,
3*depth + 1} over stand-in commit / collect callables that print their slot.  That transcript must be the one the loop written
out gives (written_out_loop() of test_feed_ticks_gpu.py: the form the tone and echo feeds had in C) and the one the modem feed's
former form gives -- both restated below over a ring of two counters: the header's claim that the forms are one sequence of calls,
checked.  Then the refusals: codes, texts, and a ring left as it was."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, STATE = -2, -5
RUN_TEXT = "bad arguments (lag in 1 .. depth - 1, nothing outstanding)"
FULL_TEXT = "every slot of the feed holds a tick: collect one first"


class Ring:
    """tick t lives in slot t % depth; every call is written down"""

    def __init__(self, depth):
        self.depth, self.n_commit, self.n_collect, self.said = depth, 0, 0, []

    def acquire(self):
        assert self.outstanding() < self.depth

    def commit(self, samples=None):
        self.said.append("commit %d" % (self.n_commit % self.depth))
        self.n_commit += 1

    def outstanding(self):
        return self.n_commit - self.n_collect

    def collect(self):
        self.said.append("collect %d" % (self.n_collect % self.depth))
        self.n_collect += 1


def written_out_loop(ops, samples, ticks, lag):
    got = []
    for _ in range(ticks):
        ops.acquire()                                           # the slot keeps what it holds
        ops.commit(samples)
        if ops.outstanding() > lag:
            got.append(ops.collect())
    while ops.outstanding():
        got.append(ops.collect())
    return got


def modem_form(ops, samples, ticks, lag):
    for i in range(ticks + 1):
        if i < ticks:
            ops.acquire(), ops.commit(samples)
        while ops.outstanding() > (lag if i < ticks else 0):
            ops.collect()


@pytest.fixture(scope="module")
def transcript(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("feed_ring")), "feed_ring")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
           "-I" + os.path.join(ROOT, "spandsp_amd", "csrc"), os.path.join(ROOT, "tests", "c_callers", "feed_ring.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr
    lines = p.stdout.splitlines()
    cut = lines.index("refusals")
    return lines[:cut], lines[cut + 1:]


def test_the_loop_is_both_former_forms(transcript):
    want = []
    cases = 0
    for depth in range(1, 9):
        for lag in range(1, depth):
            for ticks in (1, depth - 1, depth, 3*depth + 1):
                a, b = Ring(depth), Ring(depth)
                written_out_loop(a, None, ticks, lag)
                modem_form(b, None, ticks, lag)
                assert a.said == b.said, (depth, lag, ticks)
                assert len(a.said) == 2*ticks
                want += ["run depth %d lag %d ticks %d" % (depth, lag, ticks)] + a.said
                want += ["rc 0, outstanding 0, committed %d, elapsed written" % ticks]
                cases += 1
    assert cases == 4*sum(range(8))
    got = transcript[0]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d" % (i + 1)
    assert len(got) == len(want)


def test_refusals_leave_the_ring_as_it_was(transcript):
    want = ["depth %d ok: %d" % (d, 1 <= d <= 8) for d in range(10)]
    refused = 'refused run (%s): rc %d, "%s", calls 0, elapsed untouched, outstanding %d -> %d'
    for depth in range(1, 9):
        want.append("depth %d" % depth)
        want.append("collect on an empty ring: oldest -1, outstanding 0")
        for what in ("lag 0", "lag = depth", "no ticks"):
            want.append(refused % (what, BAD_ARG, RUN_TEXT, 0, 0))
        want.append(refused % ("a tick outstanding", BAD_ARG, RUN_TEXT, 1, 1))
        want.append("that tick: oldest 0, then oldest -1, outstanding 0")               # collectable, and exactly once
        want.append('every slot busy: next %d, "%s", commit %d, outstanding %d, oldest 0' % (STATE, FULL_TEXT, STATE, depth))
        for lag in range(1, depth):
            for k in range(depth + 1):
                out = min(k, lag)                               # what the rounds before tick k left outstanding
                want.append("lag %d, commit fails on tick %d: rc -77, outstanding %d -> %d, committed %d, elapsed untouched" % (lag, k, out, out, k))
    want.append(refused % ("no ring", BAD_ARG, RUN_TEXT, 0, 0))
    got = transcript[1]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d" % (i + 1)
    assert len(got) == len(want)
