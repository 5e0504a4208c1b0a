"""Writes tests/golden/faxfe.npz from the live reference: the receive half of fax_modems_state_t, driven as fax_rx() drives it.

fax_modems.c, hdlc.c, crc.c and silence_gen.c are not among the modules of oracle/_ref/libspandsp_ref.so, so they are compiled
here, in a temporary directory, with the flags of oracle/Makefile (STRICT + DEFS), linked against that library, beside the few
lines of C below (DRIVER): fax_rx()'s loop -- the optional dc_restore(), s->rx_handler(s->rx_user_data, amp, len), a report of
which function is installed -- and senders that make the signals.  Nothing compiled is kept.  The fixture holds signals,
scripts and records only.

Where this driver is not fax_rx() to the letter:
  - dc_restore() is skipped while span_dummy_rx is installed (a channel whose handler is NONE takes no part in a tick of the
    bank at all);
  - the event rows are not those of twin receivers: the put_bit of the object's own fast modem and V.21 receiver is pointed at
    a recorder that notes the call and passes it on to where fax_modems had pointed it (the shared hdlc_rx, or the non-ECM
    put_bit).  The rows are what the object's own receivers said, in the order they said it.

Per case k (names in `names`):
  c<k>_cfg      dc_restore, ticks
  c<k>_lens     the tick lengths
  c<k>_ops      [tick, call, which, bit_rate, short_train, hdlc_mode]: the control calls ahead of that tick (call 1:
                start_slow_modem, 2: start_fast_modem), c<k>_path per op: 0 slow, 1 the init path, 2 the restart path
  c<k>_amp      the line, int16
  c<k>_handler  per tick, the handler installed afterwards (0 NONE, 1 FAST_AND_V21, 2 FAST_ONLY, 3 V21_ONLY); _frx
                rx_frame_received
  c<k>_recs     the hdlc_accept calls, all ticks back to back (>= 0: len | ok << 16, < 0: a status), _nrecs per tick, _bytes
                the frames' octets back to back, _nbytes per tick
  c<k>_put      the non-ECM put_bit calls back to back (int8), _nput per tick
  c<k>_fast     the fast modem's put_bit / status calls back to back (int8), _nfast per tick; _v21 / _nv21 (int16) the V.21
                receiver's
  c<k>_dc       the dc_restore state at the end
  c<k>_framer   the shared hdlc_rx at the end, as the HDLC bank's words (the offsets of tests/golden/hdlc.npz), _buffer its
                404 octets

The case "call" runs 215 ticks, more than the 130 or so of the others: it is one call from end to end, and a V.17 long
training alone is 70 ticks, each of its two V.21 frames 35.

Case 11 (training and a good frame from the fast modem inside one tick, so that the handler ends on V.21 although the fast
modem trained) is searched for over the start delay 0..159 of a V.17 signal; `case11` is 1 where a delay gave it and 0 where
none did.

Run from the repository root:  python tests/golden/make_golden_faxfe.py [reference source dir]"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_golden_hdlc import DEFS, RX_FIELDS, STRICT, pattern      # noqa: E402

GOLDEN = os.path.join(HERE, "faxfe.npz")
V21_RX, V17_RX, V27TER_RX, V29_RX = 12, 13, 14, 15      # FAX_MODEM_*, spandsp/fax_modems.h
SLOW, FAST = 1, 2
MAX_TICKS = 240

DRIVER = r"""
#include <inttypes.h>
#include <stdlib.h>
#include <stdio.h>
#include <stddef.h>
#include <string.h>
#include <math.h>
#include <stdbool.h>
#include "spandsp/telephony.h"
#include "spandsp/alloc.h"
#include "spandsp/logging.h"
#include "spandsp/bit_operations.h"
#include "spandsp/bitstream.h"
#include "spandsp/dc_restore.h"
#include "spandsp/queue.h"
#include "spandsp/power_meter.h"
#include "spandsp/complex.h"
#include "spandsp/modem_echo.h"
#include "spandsp/tone_detect.h"
#include "spandsp/tone_generate.h"
#include "spandsp/async.h"
#include "spandsp/crc.h"
#include "spandsp/hdlc.h"
#include "spandsp/silence_gen.h"
#include "spandsp/fsk.h"
#include "spandsp/godard.h"
#include "spandsp/v29tx.h"
#include "spandsp/v29rx.h"
#include "spandsp/v27ter_tx.h"
#include "spandsp/v27ter_rx.h"
#include "spandsp/v17tx.h"
#include "spandsp/v17rx.h"
#include "spandsp/super_tone_rx.h"
#include "spandsp/modem_connect_tones.h"
#include "spandsp/fax_modems.h"
#include "spandsp/private/logging.h"
#include "spandsp/private/bitstream.h"
#include "spandsp/private/silence_gen.h"
#include "spandsp/private/power_meter.h"
#include "spandsp/private/modem_echo.h"
#include "spandsp/private/fsk.h"
#include "spandsp/private/godard.h"
#include "spandsp/private/v17tx.h"
#include "spandsp/private/v17rx.h"
#include "spandsp/private/v27ter_tx.h"
#include "spandsp/private/v27ter_rx.h"
#include "spandsp/private/v29tx.h"
#include "spandsp/private/v29rx.h"
#include "spandsp/private/modem_connect_tones.h"
#include "spandsp/private/hdlc.h"
#include "spandsp/private/fax_modems.h"

/* ---- senders: hdlc_tx behind a modulator, or a seeded bit source ---- */
typedef struct
{
    hdlc_tx_state_t *h;
    const uint8_t *frames;
    const int *lens;
    const int *corrupt;
    int n;
    int at;
    int pos;
} feed_t;

static void underflow(void *user)
{
    feed_t *f = (feed_t *) user;
    if (f->at < f->n)
    {
        hdlc_tx_frame(f->h, f->frames + f->pos, f->lens[f->at]);
        if (f->corrupt[f->at])
            hdlc_tx_corrupt_frame(f->h);
        f->pos += f->lens[f->at];
    }
    else if (f->at == f->n)
        hdlc_tx_flags(f->h, 3);
    else
        hdlc_tx_frame(f->h, NULL, 0);
    f->at++;
}

static uint32_t lfsr;
static int prbs_left;
static int prbs_bit(void *user)
{
    if (prbs_left-- <= 0)
        return SIG_STATUS_END_OF_DATA;
    lfsr = lfsr*1103515245u + 12345u;
    return (lfsr >> 16) & 1;
}

/* which: a FAX_MODEM_*_RX (the signal that receiver takes).  n_frames < 0: -n_frames bits of the seeded source instead of
   frames.  Returns the samples made. */
int make_signal(int which, int bit_rate, int short_train, int preamble, const uint8_t *frames, const int *lens, const int *corrupt,
                int n_frames, int16_t *out, int max)
{
    feed_t f;
    span_get_bit_func_t get = (span_get_bit_func_t) hdlc_tx_get_bit;
    void *user;
    int n = 0;
    int got;
    memset(&f, 0, sizeof(f));
    f.frames = frames;
    f.lens = lens;
    f.corrupt = corrupt;
    f.n = n_frames;
    f.h = hdlc_tx_init(NULL, false, 2, false, underflow, &f);
    hdlc_tx_flags(f.h, preamble);
    user = f.h;
    if (n_frames < 0)
    {
        get = prbs_bit;
        lfsr = 12345u + (uint32_t) bit_rate;
        prbs_left = -n_frames;
        user = NULL;
    }
    if (which == FAX_MODEM_V21_RX)
    {
        fsk_tx_state_t *t = fsk_tx_init(NULL, &preset_fsk_specs[FSK_V21CH2], get, user);
        while (n < max  &&  (got = fsk_tx(t, out + n, (max - n < 160)  ?  (max - n)  :  160)) > 0)
            n += got;
        fsk_tx_free(t);
    }
    else if (which == FAX_MODEM_V29_RX)
    {
        v29_tx_state_t *t = v29_tx_init(NULL, bit_rate, false, get, user);
        while (n < max  &&  (got = v29_tx(t, out + n, (max - n < 160)  ?  (max - n)  :  160)) > 0)
            n += got;
        v29_tx_free(t);
    }
    else if (which == FAX_MODEM_V27TER_RX)
    {
        v27ter_tx_state_t *t = v27ter_tx_init(NULL, bit_rate, false, get, user);
        while (n < max  &&  (got = v27ter_tx(t, out + n, (max - n < 160)  ?  (max - n)  :  160)) > 0)
            n += got;
        v27ter_tx_free(t);
    }
    else
    {
        v17_tx_state_t *t = v17_tx_init(NULL, bit_rate, false, get, user);
        if (short_train)
            v17_tx_restart(t, bit_rate, false, true);
        while (n < max  &&  (got = v17_tx(t, out + n, (max - n < 160)  ?  (max - n)  :  160)) > 0)
            n += got;
        v17_tx_free(t);
    }
    hdlc_tx_free(f.h);
    return n;
}

/* ---- the object under fax_rx()'s loop ---- */
static fax_modems_state_t *m;
static int hdlc_mode_now;
static int32_t *o_recs; static int n_recs;
static uint8_t *o_bytes; static int n_bytes;
static int8_t *o_put; static int n_put;
static int8_t *o_fast; static int n_fast;
static int16_t *o_v21; static int n_v21;

static void accept(void *user, const uint8_t *msg, int len, int ok)
{
    if (len < 0)
    {
        o_recs[n_recs++] = len;
        return;
    }
    o_recs[n_recs++] = len | (ok  ?  0x10000  :  0);
    memcpy(o_bytes + n_bytes, msg, len);
    n_bytes += len;
}

static void non_ecm_put(void *user, int bit)
{
    o_put[n_put++] = (int8_t) bit;
}

static void fast_put(void *user, int bit)
{
    o_fast[n_fast++] = (int8_t) bit;
    if (hdlc_mode_now)
        hdlc_rx_put_bit(&m->hdlc_rx, bit);
    else
        non_ecm_put(NULL, bit);
}

static void v21_put(void *user, int bit)
{
    o_v21[n_v21++] = (int16_t) bit;
    hdlc_rx_put_bit(&m->hdlc_rx, bit);
}

static void point_at_recorders(void)
{
    fsk_rx_set_put_bit(&m->v21_rx, v21_put, NULL);
    if (m->fast_modem == FAX_MODEM_V29_RX)
        v29_rx_set_put_bit(&m->fast_modems.v29_rx, fast_put, NULL);
    else if (m->fast_modem == FAX_MODEM_V27TER_RX)
        v27ter_rx_set_put_bit(&m->fast_modems.v27ter_rx, fast_put, NULL);
    else if (m->fast_modem == FAX_MODEM_V17_RX)
        v17_rx_set_put_bit(&m->fast_modems.v17_rx, fast_put, NULL);
}

static int installed(void)
{
    if (m->rx_handler == (span_rx_handler_t) &span_dummy_rx)
        return 0;
    if (m->rx_handler == (span_rx_handler_t) &fax_modems_v29_v21_rx  ||  m->rx_handler == (span_rx_handler_t) &fax_modems_v17_v21_rx
        ||  m->rx_handler == (span_rx_handler_t) &fax_modems_v27ter_v21_rx)
        return 1;
    if (m->rx_handler == (span_rx_handler_t) &fsk_rx)
        return 3;
    if (m->rx_handler == (span_rx_handler_t) &v29_rx  ||  m->rx_handler == (span_rx_handler_t) &v17_rx
        ||  m->rx_handler == (span_rx_handler_t) &v27ter_rx)
        return 2;
    return -1;
}

/* ops: [n_ops][6] = tick, call, which, bit_rate, short_train, hdlc_mode.  per_tick: [ticks][7] = handler, rx_frame_received,
   and the running totals of records, octets, non-ECM bits, fast events, V.21 events.  path: per op, 0 / 1 init / 2 restart.
   tail: dc state, then 19 {offset, size} pairs' worth of hdlc_rx words are read by the caller from hdlc_at(). */
int run_case(int use_dc, const int32_t *ops, int n_ops, const int16_t *amp, const int32_t *lens, int ticks, int32_t *per_tick,
             int32_t *path, int32_t *recs, uint8_t *bytes, int8_t *put, int8_t *fast, int16_t *v21, int32_t *dc_state)
{
    int16_t buf[4096];
    int at = 0;
    o_recs = recs; o_bytes = bytes; o_put = put; o_fast = fast; o_v21 = v21;
    n_recs = n_bytes = n_put = n_fast = n_v21 = 0;
    hdlc_mode_now = 0;
    if (m)
        fax_modems_free(m);
    m = fax_modems_init(NULL, false, accept, NULL, non_ecm_put, NULL, NULL, NULL);
    point_at_recorders();
    for (int t = 0;  t < ticks;  t++)
    {
        for (int k = 0;  k < n_ops;  k++)
        {
            const int32_t *op = ops + 6*k;
            if (op[0] != t)
                continue;
            if (op[1] == 1)
            {
                fax_modems_start_slow_modem(m, op[2]);
                path[k] = 0;
            }
            else
            {
                path[k] = (m->fast_modem != op[2])  ?  1  :  2;
                fax_modems_start_fast_modem(m, op[2], op[3], op[4], op[5]);
                hdlc_mode_now = op[5];
            }
            point_at_recorders();
        }
        const int len = lens[t];
        memcpy(buf, amp + at, len*sizeof(int16_t));
        at += len;
        if (installed() != 0)
        {
            if (use_dc)
            {
                for (int i = 0;  i < len;  i++)
                    buf[i] = dc_restore(&m->dc_restore, buf[i]);
            }
            m->rx_handler(m->rx_user_data, buf, len);
        }
        int32_t *row = per_tick + 7*t;
        row[0] = installed();
        row[1] = m->rx_frame_received  ?  1  :  0;
        row[2] = n_recs; row[3] = n_bytes; row[4] = n_put; row[5] = n_fast; row[6] = n_v21;
        if (row[0] < 0)
            return -1;
    }
    *dc_state = m->dc_restore.state;
    return 0;
}

const void *hdlc_at(void)
{
    return &m->hdlc_rx;
}
"""

SRC = ("fax_modems.c", "hdlc.c", "crc.c", "silence_gen.c")


def build_reference(ref_src, d):
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    so = os.path.join(d, "libfaxfe_ref.so")
    drv = os.path.join(d, "driver.c")
    open(drv, "w").write(DRIVER)
    subprocess.run(["gcc"] + STRICT + DEFS + ["-I" + os.path.join(ref_dir, "gen"), "-I" + ref_src, "-shared", "-o", so, drv]
                   + [os.path.join(ref_src, f) for f in SRC] + ["-L" + ref_dir, "-lspandsp_ref", "-Wl,-rpath," + ref_dir, "-lm",
                                                                "-Wl,--no-undefined"], check=True)
    heads = ("telephony", "alloc", "async", "crc", "hdlc", "private/hdlc")
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>",
             "#include <stdbool.h>"] + ['#include "spandsp/%s.h"' % h for h in heads] + ["int main(void) {"]
    for f in RX_FIELDS:
        lines.append('printf("%%zu %%zu\\n", offsetof(hdlc_rx_state_t, %s), sizeof(((hdlc_rx_state_t *) 0)->%s));' % (f, f))
    lines.append("return 0; }")
    src = os.path.join(d, "off.c")
    open(src, "w").write("\n".join(lines) + "\n")
    exe = os.path.join(d, "off")
    subprocess.run(["gcc", "-std=gnu99"] + DEFS + ["-I" + ref_src, src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    offsets = [[int(x) for x in ln.split()] for ln in out.strip().splitlines()]
    C.CDLL(os.path.join(ref_dir, "libspandsp_ref.so"), mode=C.RTLD_GLOBAL)
    L = C.CDLL(so)
    L.hdlc_at.restype = C.c_void_p
    vp, ci = C.c_void_p, C.c_int
    L.make_signal.argtypes = [ci, ci, ci, ci, vp, vp, vp, ci, vp, ci]
    L.run_case.argtypes = [ci, vp, ci, vp, vp, ci] + [vp]*8
    return L, offsets


def signal(L, which, bit_rate=0, frames=(), corrupt=(), preamble=40, short_train=0, prbs_bits=0):
    out = np.zeros(MAX_TICKS*200, np.int16)
    data = np.frombuffer(b"".join(frames) or b"\0", np.uint8).copy()
    lens = np.array([len(f) for f in frames] or [0], np.int32)
    bad = np.array(list(corrupt) + [0]*(len(lens) - len(corrupt)), np.int32)
    n = L.make_signal(which, bit_rate, short_train, preamble, data.ctypes.data, lens.ctypes.data, bad.ctypes.data,
                      -prbs_bits if prbs_bits else len(frames), out.ctypes.data, len(out))
    assert 0 < n < len(out)
    return out[:n]


def line(parts, total, seed, dc=0):
    """parts: (start sample, signal); light seeded noise over all of it"""
    x = np.zeros(total, np.int32)
    for at, s in parts:
        k = min(len(s), total - at)
        x[at:at + k] += s[:k]
    rng = np.random.RandomState(seed)
    x = x + np.round(rng.normal(0.0, 3.0, total)).astype(np.int32) + dc
    return np.clip(x, -32768, 32767).astype(np.int16)


def run(L, offsets, use_dc, ops, amp, lens):
    ticks = len(lens)
    ops_a = np.array(ops, np.int32).reshape(-1, 6)
    lens_a = np.array(lens, np.int32)
    assert lens_a.sum() <= len(amp)
    per = np.zeros((ticks, 7), np.int32)
    path = np.zeros(len(ops_a), np.int32)
    room = int(lens_a.sum()) + 64*ticks
    recs = np.zeros(room, np.int32)
    octets = np.zeros(room, np.uint8)
    put = np.zeros(room, np.int8)
    fast = np.zeros(room, np.int8)
    v21 = np.zeros(room, np.int16)
    dc = np.zeros(1, np.int32)
    rc = L.run_case(use_dc, ops_a.ctypes.data, len(ops_a), amp.ctypes.data, lens_a.ctypes.data, ticks, per.ctypes.data, path.ctypes.data,
                    recs.ctypes.data, octets.ctypes.data, put.ctypes.data, fast.ctypes.data, v21.ctypes.data, dc.ctypes.data)
    assert rc == 0
    tot = per[-1, 2:]
    cum = np.concatenate([np.zeros((1, 5), np.int32), per[:, 2:]])
    each = np.diff(cum, axis=0).astype(np.int32)
    p = L.hdlc_at()
    words = np.array([int.from_bytes(C.string_at(p + off, size), "little") & 0xFFFFFFFF for off, size in offsets[:-1]], np.uint32).view(np.int32)
    buffer = np.frombuffer(C.string_at(p + offsets[-1][0], 404), np.uint8).copy()
    return {"cfg": np.array([use_dc, ticks], np.int32), "lens": lens_a, "ops": ops_a, "path": path, "amp": amp[:int(lens_a.sum())].copy(),
            "handler": per[:, 0].copy(), "frx": per[:, 1].copy(), "recs": recs[:tot[0]].copy(), "nrecs": each[:, 0].copy(),
            "bytes": octets[:tot[1]].copy(), "nbytes": each[:, 1].copy(), "put": put[:tot[2]].copy(), "nput": each[:, 2].copy(),
            "fast": fast[:tot[3]].copy(), "nfast": each[:, 3].copy(), "v21": v21[:tot[4]].copy(), "nv21": each[:, 4].copy(),
            "dc": dc, "framer": words, "buffer": buffer}


def good_frames(r):
    return [int(x) & 0xFFFF for x in r["recs"] if x >= 0x10000]


def cases(L, offsets):
    f12 = pattern(12, 201)
    f256 = pattern(256, 202)
    f30 = pattern(30, 203)
    out = []
    t160 = lambda n: [160]*n

    # 1: a V.29 9600 non-ECM page
    page = signal(L, V29_RX, 9600, prbs_bits=9600)
    r = run(L, offsets, 0, [[0, FAST, V29_RX, 9600, 0, 0]], line([(333, page)], 160*60, 1), t160(60))
    assert 2 in r["handler"] and len(r["put"]) > 5000 and not good_frames(r)
    out.append(("v29_page", r))
    # 2: V.17 14400, hdlc_mode, a 256-octet frame
    s17 = signal(L, V17_RX, 14400, [f256, f12])
    r = run(L, offsets, 0, [[0, FAST, V17_RX, 14400, 0, 1]], line([(500, s17)], 160*90, 2), t160(90))
    assert 2 in r["handler"] and good_frames(r) == [256, 12]
    out.append(("v17_ecm", r))
    # 3: V.27ter 4800, hdlc_mode
    s27 = signal(L, V27TER_RX, 4800, [f30, f12])
    r = run(L, offsets, 0, [[0, FAST, V27TER_RX, 4800, 0, 1]], line([(421, s27)], 160*110, 3), t160(110))
    assert 2 in r["handler"] and good_frames(r) == [30, 12]
    out.append(("v27ter_ecm", r))
    # 4: a V.21 frame while V.29 is expected
    s21 = signal(L, V21_RX, frames=[f12], preamble=32)
    r = run(L, offsets, 0, [[0, FAST, V29_RX, 9600, 0, 1]], line([(250, s21)], 160*85, 4), t160(85))
    assert r["handler"][-1] == 3 and 2 not in r["handler"] and good_frames(r) == [12]
    out.append(("v21_while_v29", r))
    # 5: an idle line stays on both
    r = run(L, offsets, 0, [[0, FAST, V29_RX, 9600, 0, 0]], line([], 160*30, 5), t160(30))
    assert (r["handler"] == 1).all()
    out.append(("idle", r))
    # 6: a V.21 frame with a bad CRC, then a good one: the switch comes on the good one
    s21b = signal(L, V21_RX, frames=[f12, f30], corrupt=[1, 0], preamble=10)
    r = run(L, offsets, 0, [[0, FAST, V17_RX, 14400, 0, 1]], line([(100, s21b)], 160*130, 6), t160(130))
    bad_at = [i for i, x in enumerate(r["recs"]) if 0 <= x < 0x10000]
    assert bad_at and r["handler"][-1] == 3 and good_frames(r) == [30]
    first_bad_tick = int(np.searchsorted(np.cumsum(r["nrecs"]), bad_at[0], side="right"))
    assert r["handler"][first_bad_tick] == 1
    out.append(("v21_bad_then_good", r))
    s21c = signal(L, V21_RX, frames=[f12], preamble=10)
    # 7: start_slow_modem alone, then start_fast_modem in mid-run
    r = run(L, offsets, 0, [[0, SLOW, V21_RX, 0, 0, 0], [70, FAST, V29_RX, 9600, 0, 0]],
            line([(200, s21c), (160*72 + 77, page)], 160*110, 7), t160(110))
    assert r["handler"][0] == 3 and 2 in r["handler"] and good_frames(r) == [12]
    out.append(("slow_then_fast", r))
    # 8: one call's sequence
    s21c = signal(L, V21_RX, frames=[f12], preamble=10)
    s17s = signal(L, V17_RX, 14400, [f30], short_train=1)
    s29 = signal(L, V29_RX, 9600, [f12])
    ops = [[0, SLOW, V21_RX, 0, 0, 0], [45, FAST, V17_RX, 14400, 0, 1], [125, SLOW, V21_RX, 0, 0, 0], [168, FAST, V17_RX, 14400, 1, 1],
           [188, FAST, V29_RX, 9600, 0, 1]]
    r = run(L, offsets, 0, ops, line([(100, s21c), (160*46, signal(L, V17_RX, 14400, [f30])), (160*126, s21c), (160*169 + 40, s17s),
                                      (160*189 + 9, s29)], 160*215, 8), t160(215))
    assert list(r["path"]) == [0, 1, 0, 2, 1], r["path"]
    assert good_frames(r) == [12, 30, 12, 30, 12], good_frames(r)
    out.append(("call", r))
    # 9: case 1 with dc_restore on and a DC offset on the line
    r = run(L, offsets, 1, [[0, FAST, V29_RX, 9600, 0, 0]], line([(333, page)], 160*60, 9, dc=700), t160(60))
    assert 2 in r["handler"] and len(r["put"]) > 5000 and r["dc"][0] != 0
    out.append(("v29_page_dc", r))
    # 10: case 2 on the tick lengths (160, 7, 200, 40), cycled
    lens = [(160, 7, 200, 40)[i % 4] for i in range(144)]
    r = run(L, offsets, 0, [[0, FAST, V17_RX, 14400, 0, 1]], line([(500, s17)], sum(lens), 10), lens)
    assert 2 in r["handler"] and good_frames(r) == [256, 12]
    out.append(("v17_ecm_odd_ticks", r))
    # 12: V.29 -> V.17 -> V.29 on one line: the second V.29 start is an init again, over what the first stay left in its bank
    r = run(L, offsets, 0, [[0, FAST, V29_RX, 9600, 0, 0], [30, FAST, V17_RX, 14400, 0, 0], [34, FAST, V29_RX, 7200, 0, 0]],
            line([(200, page[:3600]), (160*35 + 50, signal(L, V29_RX, 7200, prbs_bits=3600))], 160*70, 12), t160(70))
    assert list(r["path"]) == [1, 1, 1] and r["handler"][29] == 2 and r["handler"][33] == 1 and r["handler"][-1] == 2
    out.append(("v29_v17_v29", r))
    # 11: training succeeded and a good frame inside one tick
    found = 0
    s17q = signal(L, V17_RX, 14400, [b"\xff\x13"], preamble=6, short_train=1)
    for long_train in (1, 0):
        sig = signal(L, V17_RX, 14400, [b"\xff\x13"], preamble=6) if long_train else s17q
        for delay in range(160):
            # (the short train needs a trained receiver behind it: a long-trained page first, then the restart)
            if long_train:
                ops = [[0, FAST, V17_RX, 14400, 0, 1]]
                parts = [(delay, sig)]
                n = 76
            else:
                ops = [[0, FAST, V17_RX, 14400, 0, 1], [45, FAST, V17_RX, 14400, 1, 1]]
                parts = [(300, signal(L, V17_RX, 14400, [f12])), (160*46 + delay, sig)]
                n = 70
            r = run(L, offsets, 0, ops, line(parts, 160*n, 11), t160(n))
            h = r["handler"]
            for t in range(1, n):
                if h[t - 1] == 1 and h[t] == 3 and -4 in r["fast"][int(r["nfast"][:t].sum()):int(r["nfast"][:t + 1].sum())]:
                    found = 1
            if found:
                out.append(("same_tick", r))
                break
        if found:
            break
    return out, found


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    with tempfile.TemporaryDirectory() as d:
        L, offsets = build_reference(ref_src, d)
        got, found = cases(L, offsets)
    out = {"names": np.array([n for n, _ in got]), "case11": np.array(found, np.int32)}
    for k, (name, r) in enumerate(got):
        for f, v in r.items():
            out["c%d_%s" % (k, f)] = v
        print(k, name, "ticks", r["cfg"][1], "handlers", sorted(set(r["handler"].tolist())), "records", len(r["recs"]), "octets", len(r["bytes"]),
              "non-ECM bits", len(r["put"]), "paths", r["path"].tolist())
    print("case 11:", "found" if found else "no delay gives it")
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
