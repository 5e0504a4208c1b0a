"""Echo canceller groups (include/spangpu_spandsp.h): N echo_can_state_t objects attached to one bank, frames staged by
spangpu_echo_can_update_block() and run in one tick.  Every object against its own oracle object -- every clean sample,
the complete state through spangpu_echo_group_bank() -- whatever the grouping into ticks was."""
import ctypes

import numpy as np
import pytest

from echo_lines import compare_state, make_channels, same_state, state_digest

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A
ERR_BAD_ARG, ERR_STATE = -2, -5
MODES = [0x01, 0x03, 0x07, 0x67]


def test_echo_group_of_300_objects(built):
    from oracle import ref, restated as orc
    from spandsp_amd import engine
    n_slots, n_obj, taps, max_samples, ticks = 310, 300, 128, 240, 64
    rng = np.random.default_rng(2024)
    # the objects sit on the slots that are not left out; ten slots stay unattached throughout
    spare = set(int(x) for x in rng.choice(n_slots, n_slots - n_obj, replace=False))
    slots = [c for c in range(n_slots) if c not in spare]
    mode = [MODES[i] for i in rng.integers(0, 4, n_obj)]
    tx, rx = make_channels(n_obj, max_samples*ticks + 64, taps, seed=300)
    grp = engine.EchoGroup(n_slots, taps, max_samples)
    bank = grp.bank
    initial = {c: bank.get_state(c) for c in spare}
    objs = [grp.attach(slots[k], mode[k]) for k in range(n_obj)]
    dets = [orc.EchoCan(taps, m) for m in mode]
    refs = [ref.EchoCan(taps, mode[k]) for k in range(8)] if ref.available() else []
    pos = np.zeros(n_obj, np.int64)
    assert grp.ticks() == 0
    with pytest.raises(engine.SpanGpuError):
        grp.attach(slots[0], 0x01)                          # the slot is taken

    def frame(k, n):
        a, b = tx[k, pos[k]:pos[k] + n], rx[k, pos[k]:pos[k] + n]
        pos[k] += n
        return a, b

    def check(k, a, b, hpf, clean, tx_out=None):
        want = dets[k].run(a, b, hpf)
        assert np.array_equal(clean[:len(a)], want), (k, np.nonzero(clean[:len(a)] != want)[0][:5])
        assert np.all(clean[len(a):] == CANARY), k
        if k < len(refs):
            assert np.array_equal(refs[k].run(a, b, hpf), want), ("reference", k)
        if tx_out is not None and not (hpf and mode_now[k] & 0x20):
            assert np.array_equal(tx_out[:len(a)], a), k

    mode_now = list(mode)
    for t in range(ticks):
        sizes = [160]*n_obj
        if t % 4 == 1:
            sizes = [(80, 160, 240)[(k + t) % 3] for k in range(n_obj)]        # mixed frame sizes in one tick
        sit_out = set(k for k in range(n_obj) if k % 3 == t % 3) if t % 5 == 2 else set()
        hpf = rng.integers(0, 2, n_obj).astype(bool)
        before = grp.ticks()
        staged = []
        order = [k for k in rng.permutation(n_obj) if k not in sit_out]
        for i, k in enumerate(order):
            a, b = frame(k, sizes[k])
            clean = np.full(max_samples, CANARY, np.int16)
            tx_out = np.full(max_samples, CANARY, np.int16) if k % 2 else None
            if t == 6 and i == 0:
                # an oversize frame is refused and nothing is staged
                big = np.zeros(max_samples + 1, np.int16)
                assert objs[k].update_block(big, big, np.zeros(max_samples + 1, np.int16)) == ERR_BAD_ARG
                assert objs[k].pending() == 0
                assert objs[k].update_block(big[:0], big[:0], clean) == 0 and objs[k].pending() == 0       # n = 0: nothing
            rc = objs[k].update_block(a, b, clean, tx_out, hpf[k])
            assert rc == 0, (t, k, rc)
            staged.append((k, a, b, clean, tx_out))
            last = (i == len(order) - 1) and not sit_out
            if not last:
                assert objs[k].pending() == 1 and grp.ticks() == before, (t, k)
            if t == 5 and i == 3:
                # a second frame before the tick ran: refused, the first one stays and runs
                junk = np.full(160, 999, np.int16)
                assert objs[k].update_block(junk, junk, np.zeros(160, np.int16)) == ERR_STATE
                assert objs[k].pending() == 1
        if sit_out:
            # a third of the objects are late: the owner of the tick runs it with what is there
            assert grp.ticks() == before
            assert grp.flush() == len(order)
        # (a full set: the last stager's call ran the tick)
        assert grp.ticks() == before + 1, t
        assert grp.flush() == 0 and grp.ticks() == before + 1
        for k, a, b, clean, tx_out in staged:
            assert objs[k].pending() == 0
            check(k, a, b, bool(hpf[k]), clean, tx_out)
        if t % 10 == 9:
            compare_state(bank, {slots[k]: dets[k] for k in range(n_obj)}, ("tick", t))
        # ---- between ticks ----
        if t == 20:
            # echo_can_flush() in mid-stream: one object idle, one with a frame pending (the tick runs first)
            objs[1].flush()
            dets[1].flush()
            a, b = frame(5, 160)
            clean = np.full(max_samples, CANARY, np.int16)
            assert objs[5].update_block(a, b, clean) == 0 and objs[5].pending() == 1
            objs[5].flush()
            assert objs[5].pending() == 0 and grp.ticks() == before + 2
            check(5, a, b, False, clean)
            dets[5].flush()
            for k in (1, 5):
                if k < len(refs):
                    refs[k].flush()
        if t == 30:
            # echo_can_adaption_mode() likewise
            for k, m in ((2, 0x67), (100, 0x01), (299, 0x03)):
                a, b = frame(k, 80)
                clean = np.full(max_samples, CANARY, np.int16)
                assert objs[k].update_block(a, b, clean, None, True) == 0
                objs[k].adaption_mode(m)
                assert objs[k].pending() == 0
                check(k, a, b, True, clean)
                dets[k].adaption_mode(m)
                mode_now[k] = m
                if k < len(refs):
                    refs[k].adaption_mode(m)
        if t == 35:
            # echo_can_snapshot(): tap set 0 as it is now; the object's bank is the group's
            got = objs[7].snapshot_taps()
            assert np.array_equal(got, dets[7].snapshot()["taps16"][0]) and np.any(got != 0)
            assert objs[7].bank_handle() == bank.h.value
        if t == 40:
            # the per-sample calls on an attached object: pending work runs, then one sample of one channel
            a, b = frame(3, 160)
            clean3 = np.full(max_samples, CANARY, np.int16)
            assert objs[3].update_block(a, b, clean3) == 0
            for i in range(3):
                x, y = frame(9, 1)
                want = dets[9].run(x, y, False)
                assert objs[9].update(x[0], y[0]) == int(want[0]), i
                if i == 0:
                    assert objs[3].pending() == 0
                    check(3, a, b, False, clean3)
            x, y = frame(2, 1)                              # (mode 0x67 since tick 30: the transmit filter is on)
            want = dets[2].run(x, y, True)
            assert objs[2].update(objs[2].hpf_tx(x[0]), y[0]) == int(want[0])
            if len(refs) > 2:
                refs[2].run(x, y, True)
        if t == 45:
            # detach with a frame pending: it is dropped, its buffers keep their canaries; the slot, attached again with
            # another mode, is a new canceller
            k = 11
            a, b = frame(k, 160)
            clean = np.full(max_samples, CANARY, np.int16)
            tx_out = np.full(max_samples, CANARY, np.int16)
            assert objs[k].update_block(a, b, clean, tx_out) == 0 and objs[k].pending() == 1
            objs[k].free()
            assert grp.flush() == 0
            assert np.all(clean == CANARY) and np.all(tx_out == CANARY)
            mode_now[k] = 0x07 if mode[k] != 0x07 else 0x03
            objs[k] = grp.attach(slots[k], mode_now[k])
            dets[k] = orc.EchoCan(taps, mode_now[k])
            compare_state(bank, {slots[k]: dets[k]}, "attached again")
    compare_state(bank, {slots[k]: dets[k] for k in range(n_obj)}, "final")
    snaps = [d.snapshot() for d in dets]
    assert any(s["tap_set"] != 0 or s["tap_rotate_counter"] != 1600 for s in snaps)
    assert any(np.any(s["taps32"] != 0) for s in snaps)
    if refs:
        for k in range(8):
            r = refs[k].snapshot()
            g = bank.get_state(slots[k])
            assert np.array_equal(g["taps32"], r["taps32"]) and np.array_equal(g["taps16"], r["taps16"]), k
            assert np.array_equal(g["history"], r["history"]), k
    for c in spare:
        assert same_state(bank.get_state(c), initial[c], engine.ECHO_FIELDS) is None, c
    for o in objs:
        o.free()
    grp.close()


def test_echo_group_at_bank_size(built):
    """16 384 attached objects x 128 taps, 160-sample frames, 100 ticks.  Objects c and c + 8192 have identical lines: their
    clean streams and their states must be identical (the replica property of test_full_size_gpu.py), the first 64 are
    the oracle's; in every fifth tick a random tenth of the objects -- replicas together -- sit out."""
    from oracle import restated as orc
    from spandsp_amd import engine
    n_obj, half, V, taps, n, ticks, span = 16384, 8192, 256, 128, 160, 100, 32
    base_tx, base_rx = make_channels(V, n*(ticks + span), taps, seed=16384)
    line = np.arange(half) % V                              # object c < 8192: line c mod 256, from frame (c div 256) on
    lead = (np.arange(half)//V) % span
    line[:64] = np.arange(64)
    base_tx = base_tx.reshape(V, ticks + span, n)
    base_rx = base_rx.reshape(V, ticks + span, n)
    grp = engine.EchoGroup(n_obj, taps, n)
    bank = grp.bank
    objs = [grp.attach(c, 0x01) for c in range(n_obj)]
    dets = [orc.EchoCan(taps, 0x01) for _ in range(64)]
    stage = engine.lib().spangpu_echo_can_update_block
    handles = [o.p for o in objs]
    took = np.zeros(half, np.int64)                         # frames each object has run
    rng = np.random.default_rng(7)
    clean = np.zeros((n_obj, n), np.int16)
    for t in range(ticks):
        out = rng.random(half) < 0.1 if t % 5 == 4 else np.zeros(half, bool)
        tx = np.ascontiguousarray(np.tile(base_tx[line, lead + took], (2, 1)))
        rx = np.ascontiguousarray(np.tile(base_rx[line, lead + took], (2, 1)))
        clean[:] = CANARY
        pt, pr, pc = tx.ctypes.data, rx.ctypes.data, clean.ctypes.data
        before = grp.ticks()
        for c in np.nonzero(~np.tile(out, 2))[0]:
            off = int(c)*n*2
            assert stage(handles[c], pt + off, pr + off, pc + off, None, n, 0) == 0, (t, c)
        if out.any():
            assert grp.ticks() == before
            assert grp.flush() == n_obj - 2*int(out.sum())
        assert grp.ticks() == before + 1
        assert np.array_equal(clean[:half], clean[half:]), t
        assert np.all(clean[:half][out] == CANARY), t
        for c in range(64):
            if not out[c]:
                want = dets[c].run(tx[c], rx[c], False)
                assert np.array_equal(clean[c], want), (t, c)
        took += ~out
    compare_state(bank, dets, "bank size")
    for c in range(half):
        assert state_digest(bank, c) == state_digest(bank, c + half), c
    for o in objs:
        o.free()
    grp.close()
