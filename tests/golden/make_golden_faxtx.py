"""Writes tests/golden/faxtx.npz from the live reference: the transmit half of fax_modems_state_t, driven as fax_tx() drives it.

fax_modems.c, hdlc.c, crc.c and silence_gen.c are compiled here, in a temporary directory, with the flags of oracle/Makefile
(STRICT + DEFS), linked against oracle/_ref/libspandsp_ref.so, beside the C below (DRIVER).  fax.c itself needs tiffio.h and is
not compiled; the driver makes, through the reference's public fax_modems_*, silence_gen_* and hdlc_tx_* functions, the calls of
  fax_set_tx_type()     src/fax.c:327-421   (ftx_set_tx_type)
  fax_tx()              src/fax.c:221-256   (ftx_tick: the loop, then the padding of transmit_on_idle)
and stands in for T.30 with
  a SEND_STEP_COMPLETE handler that only counts;
  an HDLC underflow handler (fax.c:161-167) that counts, then pops one command off a FIFO of frame / corrupt frame / flags / end;
  a non-ECM get_bit that reads a buffer, then answers 1 -- or, once the script has said so, SIG_STATUS_END_OF_DATA.
Nothing compiled is kept.  The fixture holds scripts, rows and records only.

Where the driver is not fax.c to the letter:
  - the row is cleared before a tick (FAX CNG leaves one sample unwritten where its cadence wraps inside a call; the banks
    write a zero there);
  - the hdlc_tx is offered its FIFO at the top of every handler call of a sender that takes its bits from it (commands until a
    frame is in or none is left): the convention of make_golden_hdlc.py's driver, where T.30 would have called from its handler;
  - the senders' get_bit is pointed at a recorder that notes the answer and passes it on;
  - what T.30 does inside the SEND_STEP_COMPLETE callback (a new set_tx_type in mid-row) is not done: the script's control
    calls come between ticks.

T30_MODEM_* (spandsp/t30.h:328-337): NONE 0, PAUSE 1, CED 2, CNG 3, V21 4, V27TER 5, V29 6, V17 7, V34HDX 8, DONE 9.
FAX_MODEM_*_TX (spandsp/fax_modems.h): V17 9, V27TER 10, V29 11.

Per case k (names in `names`):
  c<k>_cfg       use_tep, ticks, samples per tick
  c<k>_ops       [tick, op, a, b, c, d]: the calls ahead of that tick, in order.  op 1: set_tx_type(type a, bit_rate b, short_train
                 c, use_hdlc d); 2: restart; 3: set_tep_mode(a); 4: queue frame number a (b: corrupt); 5: queue flags(a); 6: queue
                 the end of the data; 7: non-ECM bits [a, a + b) of c<k>_bits; 8: the non-ECM end of data (the driver's flag stays
                 set once set; a bank's is cleared when its sender starts again, so the scripts say it again behind every start)
  c<k>_path      per op: for op 1, 0: nothing happened (the same type), 1: acted, 2: acted, a fast modem by the init path,
                 3: by the restart path
  c<k>_frames    the frames' octets back to back, _flens their lengths;  c<k>_bits: one bit per entry
  c<k>_rows      [ticks][samples] int16;  c<k>_lens: fax_tx()'s return without transmit_on_idle
  c<k>_calls     [n][3] the handler calls, all ticks back to back: which (0 silence, 1 tone, 2 V.21, 3 fast), offered, returned;
                 _ncalls per tick
  c<k>_steps     SEND_STEP_COMPLETE calls per tick;  _under: underflow handler calls that found the FIFO empty
  c<k>_handler   the handler installed after the tick;  _transmit
  c<k>_asked     what hdlc_tx_get_bit answered the senders, back to back (int8; -7: SIG_STATUS_END_OF_DATA), _nasked per tick
  c<k>_end       silence remaining_samples, total_samples, current_tx_type, fast_modem
  c<k>_hdlc      the hdlc_tx at the end as the HDLC bank's words (the offsets of tests/golden/hdlc.npz), _buffer its 404 octets
The case "loop" has beside these c<k>_rx_*: B's handler, rx_frame_received and hdlc_accept records per tick, in faxfe.npz's form.

`flags` / `flag_names`: one per situation the cases must have met; the generator asserts each.

Run from the repository root:  python tests/golden/make_golden_faxtx.py [reference source dir]"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_golden_hdlc import DEFS, STRICT, TX_FIELDS, pattern      # noqa: E402

GOLDEN = os.path.join(HERE, "faxtx.npz")
NONE, PAUSE, CED, CNG, V21, V27TER, V29, V17, V34HDX, DONE = range(10)
SET, RESTART, TEP, Q_FRAME, Q_FLAGS, Q_END, BITS, EOD = range(1, 9)
H_SILENCE, H_TONE, H_V21, H_FAST = range(4)
V17_TX, V27TER_TX, V29_TX = 9, 10, 11
V27TER_RX, V29_RX = 14, 15

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

enum { TY_NONE, TY_PAUSE, TY_CED, TY_CNG, TY_V21, TY_V27TER, TY_V29, TY_V17, TY_V34HDX, TY_DONE };
enum { CMD_FRAME = 1, CMD_FLAGS, CMD_END };
#define FIFO 64

typedef struct
{
    fax_modems_state_t *m;
    int hdlc_mode;
    int steps;
    int under;
    /* the FIFO the underflow handler pops */
    int cmd[FIFO];
    int arg[FIFO];
    int bad[FIFO];
    uint8_t data[FIFO][400];
    int head;
    int fill;
    /* the non-ECM source */
    uint8_t *bits;
    int n_bits;
    int bit_at;
    int eod;
    /* what the senders were answered */
    int8_t *asked;
    int n_asked;
    int max_asked;
} line_t;

static line_t A;

static int pop(line_t *s)
{
    const int k = s->head;
    if (s->fill == 0)
        return 0;
    s->head = (k + 1)%FIFO;
    s->fill--;
    if (s->cmd[k] == CMD_FRAME)
    {
        hdlc_tx_frame(&s->m->hdlc_tx, s->data[k], s->arg[k]);
        if (s->bad[k])
            hdlc_tx_corrupt_frame(&s->m->hdlc_tx);
    }
    else if (s->cmd[k] == CMD_FLAGS)
        hdlc_tx_flags(&s->m->hdlc_tx, s->arg[k]);
    else
        hdlc_tx_frame(&s->m->hdlc_tx, NULL, 0);
    return 1;
}

static void underflow(void *user)
{
    line_t *s = (line_t *) user;
    s->steps++;
    if (!pop(s))
        s->under++;
}

static void offer(line_t *s)
{
    while (s->m->hdlc_tx.len == 0  &&  pop(s))
        ;
}

static int framed_bit(void *user)
{
    line_t *s = (line_t *) user;
    const int bit = hdlc_tx_get_bit(&s->m->hdlc_tx);
    if (s->n_asked < s->max_asked)
        s->asked[s->n_asked] = (int8_t) bit;
    s->n_asked++;
    return bit;
}

static int plain_bit(void *user)
{
    line_t *s = (line_t *) user;
    if (s->bit_at < s->n_bits)
        return s->bits[s->bit_at++];
    return s->eod  ?  SIG_STATUS_END_OF_DATA  :  1;
}

static void point_at_recorders(line_t *s)
{
    fax_modems_state_t *m = s->m;
    fsk_tx_set_get_bit(&m->v21_tx, framed_bit, s);
    if (!s->hdlc_mode)
        return;
    if (m->fast_modem == FAX_MODEM_V29_TX)
        v29_tx_set_get_bit(&m->fast_modems.v29_tx, framed_bit, s);
    else if (m->fast_modem == FAX_MODEM_V27TER_TX)
        v27ter_tx_set_get_bit(&m->fast_modems.v27ter_tx, framed_bit, s);
    else if (m->fast_modem == FAX_MODEM_V17_TX)
        v17_tx_set_get_bit(&m->fast_modems.v17_tx, framed_bit, s);
}

static int installed(const fax_modems_state_t *m)
{
    if (m->tx_handler == (span_tx_handler_t) &silence_gen)
        return 0;
    if (m->tx_handler == (span_tx_handler_t) &modem_connect_tones_tx)
        return 1;
    if (m->tx_handler == (span_tx_handler_t) &fsk_tx)
        return 2;
    if (m->tx_handler == (span_tx_handler_t) &v29_tx  ||  m->tx_handler == (span_tx_handler_t) &v17_tx
        ||  m->tx_handler == (span_tx_handler_t) &v27ter_tx)
        return 3;
    return -1;
}

static void new_line(line_t *s, int use_tep, int8_t *asked, int max_asked)
{
    if (s->m)
        fax_modems_free(s->m);
    free(s->bits);
    memset(s, 0, sizeof(*s));
    s->asked = asked;
    s->max_asked = max_asked;
    s->m = fax_modems_init(NULL, use_tep, NULL, underflow, NULL, plain_bit, NULL, s);
}

/* what a channel is silent for and switches to: fax_set_tx_type().  Returns 0: the same type, nothing done; 1: done; 2, 3: done,
   and the fast modem went through its init (2) or restart (3) path */
static int set_tx_type(line_t *s, int type, int bit_rate, int short_train, int use_hdlc)
{
    fax_modems_state_t *m = s->m;
    int which = -1;
    int path = 1;
    if (m->current_tx_type == type)
        return 0;
    if (type == TY_PAUSE)
    {
        silence_gen_alter(&m->silence_gen, milliseconds_to_samples(short_train));
        fax_modems_set_tx_handler(m, (span_tx_handler_t) &silence_gen, &m->silence_gen);
        fax_modems_set_next_tx_handler(m, NULL, NULL);
        m->transmit = true;
    }
    else if (type == TY_CED  ||  type == TY_CNG)
    {
        fax_modems_start_slow_modem(m, (type == TY_CED)  ?  FAX_MODEM_CED_TONE_TX  :  FAX_MODEM_CNG_TONE_TX);
        fax_modems_set_next_tx_handler(m, NULL, NULL);
        m->transmit = true;
    }
    else if (type == TY_V21)
    {
        fax_modems_start_slow_modem(m, FAX_MODEM_V21_TX);
        fax_modems_hdlc_tx_flags(m, 32);
        silence_gen_alter(&m->silence_gen, milliseconds_to_samples(75));
        fax_modems_set_tx_handler(m, (span_tx_handler_t) &silence_gen, &m->silence_gen);
        fax_modems_set_next_tx_handler(m, (span_tx_handler_t) &fsk_tx, &m->v21_tx);
        m->transmit = true;
    }
    else if (type == TY_V17  ||  type == TY_V27TER  ||  type == TY_V29)
    {
        which = (type == TY_V17)  ?  FAX_MODEM_V17_TX  :  (type == TY_V29)  ?  FAX_MODEM_V29_TX  :  FAX_MODEM_V27TER_TX;
        path = (m->fast_modem != which)  ?  2  :  3;
        silence_gen_alter(&m->silence_gen, milliseconds_to_samples(75));
        fax_modems_hdlc_tx_flags(m, bit_rate/40);
        fax_modems_start_fast_modem(m, which, bit_rate, short_train, use_hdlc);
        fax_modems_set_tx_handler(m, (span_tx_handler_t) &silence_gen, &m->silence_gen);
        if (type == TY_V17)
            fax_modems_set_next_tx_handler(m, (span_tx_handler_t) &v17_tx, &m->fast_modems.v17_tx);
        else if (type == TY_V29)
            fax_modems_set_next_tx_handler(m, (span_tx_handler_t) &v29_tx, &m->fast_modems.v29_tx);
        else
            fax_modems_set_next_tx_handler(m, (span_tx_handler_t) &v27ter_tx, &m->fast_modems.v27ter_tx);
        m->transmit = true;
        s->hdlc_mode = use_hdlc;
    }
    else
    {
        silence_gen_alter(&m->silence_gen, 0);
        fax_modems_set_tx_handler(m, (span_tx_handler_t) &silence_gen, &m->silence_gen);
        fax_modems_set_next_tx_handler(m, NULL, NULL);
        m->transmit = false;
    }
    m->tx_bit_rate = bit_rate;
    m->current_tx_type = type;
    point_at_recorders(s);
    return path;
}

static void apply(line_t *s, const int32_t *op, int32_t *path, const uint8_t *frames, const int32_t *fstart, const int32_t *flens,
                  const uint8_t *bits)
{
    int k;
    *path = 0;
    switch (op[1])
    {
    case 1:
        *path = set_tx_type(s, op[2], op[3], op[4], op[5]);
        break;
    case 2:
        fax_modems_restart(s->m);
        break;
    case 3:
        fax_modems_set_tep_mode(s->m, op[2]);
        break;
    case 4:
    case 5:
    case 6:
        if (s->fill >= FIFO)
            abort();
        k = (s->head + s->fill)%FIFO;
        s->fill++;
        s->cmd[k] = (op[1] == 4)  ?  CMD_FRAME  :  (op[1] == 5)  ?  CMD_FLAGS  :  CMD_END;
        s->arg[k] = (op[1] == 4)  ?  flens[op[2]]  :  op[2];
        s->bad[k] = (op[1] == 4)  ?  op[3]  :  0;
        if (op[1] == 4)
            memcpy(s->data[k], frames + fstart[op[2]], flens[op[2]]);
        break;
    case 7:
        s->bits = (uint8_t *) realloc(s->bits, s->n_bits + op[3] + 1);
        memcpy(s->bits + s->n_bits, bits + op[2], op[3]);
        s->n_bits += op[3];
        break;
    case 8:
        s->eod = 1;
        break;
    }
}

/* fax_tx()'s loop; calls: [..][3] which, offered, returned.  Returns the length without transmit_on_idle. */
static int tick(line_t *s, int16_t *row, int samples, int32_t *calls, int *n_calls)
{
    fax_modems_state_t *m = s->m;
    int len = 0;
    memset(row, 0, samples*sizeof(int16_t));
    while (m->transmit)
    {
        const int which = installed(m);
        const int offered = samples - len;
        if (which == 2  ||  (which == 3  &&  s->hdlc_mode))
            offer(s);
        const int got = m->tx_handler(m->tx_user_data, row + len, offered);
        calls[3*(*n_calls)] = which;
        calls[3*(*n_calls) + 1] = offered;
        calls[3*(*n_calls) + 2] = got;
        (*n_calls)++;
        if ((len += got) >= samples)
            break;
        if (fax_modems_set_next_tx_type(m)  &&  m->current_tx_type != TY_NONE  &&  m->current_tx_type != TY_DONE)
            s->steps++;
    }
    return len;
}

/* per_tick: [ticks][8] = len, calls so far, steps, underflows, handler, transmit, asked so far, 0 */
int run_case(int use_tep, const int32_t *ops, int n_ops, int32_t *path, const uint8_t *frames, const int32_t *fstart, const int32_t *flens,
             const uint8_t *bits, int ticks, int samples, int16_t *rows, int32_t *per_tick, int32_t *calls, int8_t *asked, int max_asked,
             int32_t *end)
{
    int n_calls = 0;
    new_line(&A, use_tep, asked, max_asked);
    for (int t = 0;  t < ticks;  t++)
    {
        for (int k = 0;  k < n_ops;  k++)
        {
            if (ops[6*k] == t)
                apply(&A, ops + 6*k, path + k, frames, fstart, flens, bits);
        }
        A.steps = A.under = 0;
        int32_t *row = per_tick + 8*t;
        row[0] = tick(&A, rows + (size_t) t*samples, samples, calls, &n_calls);
        row[1] = n_calls;
        row[2] = A.steps;
        row[3] = A.under;
        row[4] = installed(A.m);
        row[5] = A.m->transmit  ?  1  :  0;
        row[6] = A.n_asked;
        if (row[4] < 0  ||  A.n_asked > max_asked)
            return -1;
    }
    end[0] = A.m->silence_gen.remaining_samples;
    end[1] = A.m->silence_gen.total_samples;
    end[2] = A.m->current_tx_type;
    end[3] = A.m->fast_modem;
    return 0;
}

const void *hdlc_at(void)
{
    return &A.m->hdlc_tx;
}

/* ---- the loop: A's rows into a receiving object B under fax_rx()'s loop, B started as make_golden_faxfe.py starts it ---- */
static fax_modems_state_t *B;
static int32_t *o_recs; static int n_recs;
static uint8_t *o_bytes; static int n_bytes;

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

static int rx_installed(void)
{
    if (B->rx_handler == (span_rx_handler_t) &span_dummy_rx)
        return 0;
    if (B->rx_handler == (span_rx_handler_t) &fax_modems_v29_v21_rx  ||  B->rx_handler == (span_rx_handler_t) &fax_modems_v17_v21_rx
        ||  B->rx_handler == (span_rx_handler_t) &fax_modems_v27ter_v21_rx)
        return 1;
    if (B->rx_handler == (span_rx_handler_t) &fsk_rx)
        return 3;
    return 2;
}

/* rx_ops: [n][6] = tick, call (1 start_slow_modem, 2 start_fast_modem), which, bit_rate, short_train, hdlc_mode;
   rx_tick: [ticks][4] = handler, rx_frame_received, records so far, octets so far */
int run_rx(const int32_t *rx_ops, int n_ops, const int16_t *rows, int ticks, int samples, int32_t *rx_tick, int32_t *recs, uint8_t *bytes)
{
    int16_t buf[4096];
    o_recs = recs; o_bytes = bytes;
    n_recs = n_bytes = 0;
    if (B)
        fax_modems_free(B);
    B = fax_modems_init(NULL, false, accept, NULL, NULL, NULL, NULL, NULL);
    for (int t = 0;  t < ticks;  t++)
    {
        for (int k = 0;  k < n_ops;  k++)
        {
            const int32_t *op = rx_ops + 6*k;
            if (op[0] != t)
                continue;
            if (op[1] == 1)
                fax_modems_start_slow_modem(B, op[2]);
            else
                fax_modems_start_fast_modem(B, op[2], op[3], op[4], op[5]);
        }
        memcpy(buf, rows + (size_t) t*samples, samples*sizeof(int16_t));
        if (rx_installed() != 0)
            B->rx_handler(B->rx_user_data, buf, samples);
        rx_tick[4*t] = rx_installed();
        rx_tick[4*t + 1] = B->rx_frame_received  ?  1  :  0;
        rx_tick[4*t + 2] = n_recs;
        rx_tick[4*t + 3] = n_bytes;
    }
    return 0;
}
"""

SRC = ("fax_modems.c", "hdlc.c", "crc.c", "silence_gen.c")


def build_reference(ref_src, d):
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    so = os.path.join(d, "libfaxtx_ref.so")
    drv = os.path.join(d, "driver.c")
    open(drv, "w").write(DRIVER)
    subprocess.run(["gcc"] + STRICT + DEFS + ["-I" + os.path.join(ref_dir, "gen"), "-I" + ref_src, "-shared", "-o", so, drv]
                   + [os.path.join(ref_src, f) for f in SRC] + ["-L" + ref_dir, "-lspandsp_ref", "-Wl,-rpath," + ref_dir, "-lm",
                                                                "-Wl,--no-undefined"], check=True)
    heads = ("telephony", "alloc", "async", "crc", "hdlc", "private/hdlc")
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <stdlib.h>", "#include <inttypes.h>", "#include <string.h>",
             "#include <stdbool.h>"] + ['#include "spandsp/%s.h"' % h for h in heads] + ["int main(void) {"]
    for f in TX_FIELDS:
        lines.append('printf("%%zu %%zu\\n", offsetof(hdlc_tx_state_t, %s), sizeof(((hdlc_tx_state_t *) 0)->%s));' % (f, f))
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
    L.run_case.argtypes = [ci, vp, ci, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, ci, vp]
    L.run_rx.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp]
    return L, offsets


def run(L, offsets, ops, ticks, samples=160, use_tep=0, frames=(), bits=()):
    ops_a = np.array(sorted(ops, key=lambda o: o[0]), np.int32).reshape(-1, 6)       # (a stable sort: the order inside a tick stays)
    data = np.frombuffer(b"".join(frames) or b"\0", np.uint8).copy()
    flens = np.array([len(f) for f in frames] or [0], np.int32)
    fstart = np.concatenate([[0], np.cumsum(flens)[:-1]]).astype(np.int32)
    bits_a = np.array(list(bits) or [0], np.uint8)
    path = np.zeros(len(ops_a), np.int32)
    rows = np.zeros((ticks, samples), np.int16)
    per = np.zeros((ticks, 8), np.int32)
    calls = np.zeros((ticks*8, 3), np.int32)
    max_asked = ticks*samples*2
    asked = np.zeros(max_asked, np.int8)
    end = np.zeros(4, np.int32)
    rc = L.run_case(use_tep, ops_a.ctypes.data, len(ops_a), path.ctypes.data, data.ctypes.data, fstart.ctypes.data, flens.ctypes.data,
                    bits_a.ctypes.data, ticks, samples, rows.ctypes.data, per.ctypes.data, calls.ctypes.data, asked.ctypes.data, max_asked,
                    end.ctypes.data)
    assert rc == 0
    each = lambda col: np.diff(np.concatenate([[0], per[:, col]])).astype(np.int32)
    p = L.hdlc_at()
    words = np.array([int.from_bytes(C.string_at(p + off, size), "little") & 0xFFFFFFFF for off, size in offsets[:-1]], np.uint32).view(np.int32)
    buffer = np.frombuffer(C.string_at(p + offsets[-1][0], 404), np.uint8).copy()
    return {"cfg": np.array([use_tep, ticks, samples], np.int32), "ops": ops_a, "path": path, "frames": data[:int(flens.sum())].copy(),
            "flens": flens if frames else np.zeros(0, np.int32), "bits": bits_a if len(bits) else np.zeros(0, np.uint8), "rows": rows,
            "lens": per[:, 0].copy(), "calls": calls[:per[-1, 1]].copy(), "ncalls": each(1), "steps": per[:, 2].copy(),
            "under": per[:, 3].copy(), "handler": per[:, 4].copy(), "transmit": per[:, 5].copy(), "asked": asked[:per[-1, 6]].copy(),
            "nasked": each(6), "end": end, "hdlc": words, "buffer": buffer}


def calls_of(r, t):
    at = int(r["ncalls"][:t].sum())
    return [tuple(int(x) for x in c) for c in r["calls"][at:at + int(r["ncalls"][t])]]


def v21_case(L, offsets, samples, ticks, frames):
    """set_tx_type(V21) ahead of tick 0; a preamble, a good and a corrupt frame through the FIFO; the underflow behind the second
    finds the FIFO empty, the sender idles on flags, and the end is queued after that"""
    ops = [[0, SET, V21, 300, 0, 1], [0, Q_FRAME, 0, 0, 0, 0], [0, Q_FRAME, 1, 1, 0, 0], [13000//samples, Q_END, 0, 0, 0, 0]]
    return run(L, offsets, ops, ticks, samples, frames=frames)


def cases(L, offsets):
    out = []
    flags = {}
    f5 = pattern(5, 301)
    f7 = pattern(7, 302)
    f40 = pattern(40, 303)
    rng = np.random.RandomState(77)

    # 1: PAUSE of 53 ms = 424 samples = 2 ticks and 104 samples
    r = run(L, offsets, [[0, SET, PAUSE, 0, 53, 0]], 5)
    assert calls_of(r, 2) == [(H_SILENCE, 160, 104)] and r["lens"][2] == 104 and r["steps"][2] == 1 and r["steps"].sum() == 1
    assert r["transmit"][2] == 0 and r["lens"][3] == 0
    flags["pause_short_return"] = 1
    out.append(("pause", r))

    # 2: CED from its start to its own end in mid-tick: (200 + 2600) ms = 22400 samples, which is 140 ticks of 160 to the sample,
    # so this one runs on ticks of 163
    r = run(L, offsets, [[0, SET, CED, 0, 0, 0]], 140, samples=163)
    short = [t for t in range(140) if any(c[0] == H_TONE and 0 < c[2] < c[1] for c in calls_of(r, t))]
    assert len(short) == 1 and r["steps"][short[0]] == 1 and r["transmit"][short[0]] == 0 and r["handler"][short[0]] == H_SILENCE
    assert r["lens"][short[0]] == 22400 - 163*short[0]
    flags["ced_ends_in_mid_tick"] = 1
    out.append(("ced", r))

    # 2b: restart() while CED runs: current_tx_type is -1 and the tone goes on; the same type again then acts (the tone from
    # the 200 ms of silence it starts with)
    r = run(L, offsets, [[0, SET, CED, 0, 0, 0], [12, RESTART, 0, 0, 0, 0], [15, SET, CED, 0, 0, 0],
                         [17, SET, DONE, 0, 0, 0]], 18)
    assert (r["handler"][:17] == H_TONE).all() and (r["lens"][:17] == 160).all() and r["steps"].sum() == 0 and list(r["path"]) == [1, 0, 1, 1]
    assert np.abs(r["rows"][13]).max() > 1000 and not r["rows"][15].any() and r["end"][2] == DONE and r["transmit"][-1] == 0
    flags["restart_while_tone_runs"] = 1
    out.append(("ced_restart", r))

    # 3: CNG running, then V21 in its place
    ops = [[0, SET, CNG, 0, 0, 0], [6, SET, V21, 300, 0, 1], [6, Q_FRAME, 0, 0, 0, 0], [6, Q_END, 0, 0, 0, 0]]
    r = run(L, offsets, ops, 110, frames=[f5])
    assert r["handler"][5] == H_TONE and r["handler"][6] == H_SILENCE and H_V21 in r["handler"] and list(r["path"][:2]) == [1, 1]
    assert r["transmit"][-1] == 0
    flags["cng_replaced_by_v21"] = 1
    out.append(("cng_then_v21", r))

    # 4, 5: V21 on ticks of 160 (the sender starts at sample 120 of the fourth tick), 200 (the silence ends on a row's end) and 163
    for samples, name in ((160, "v21_160"), (200, "v21_200"), (163, "v21_163")):
        ticks = 14500//samples
        r = v21_case(L, offsets, samples, ticks, [f5, f7])
        first = next(t for t in range(ticks) if any(c[0] == H_V21 for c in calls_of(r, t)))
        if samples == 160:
            assert first == 3 and calls_of(r, 3) == [(H_SILENCE, 160, 120), (H_V21, 40, 40)]
            flags["v21_starts_at_120_of_tick_4"] = 1
        elif samples == 200:
            assert calls_of(r, 2) == [(H_SILENCE, 200, 200)] and r["handler"][2] == H_SILENCE
            assert calls_of(r, 3) == [(H_SILENCE, 200, 0), (H_V21, 200, 200)]
            flags["silence_ends_on_a_rows_end"] = 1
        else:
            assert calls_of(r, first)[0] == (H_SILENCE, 163, 111)
            flags["odd_start_111"] = 1
        short = [t for t in range(ticks) if any(c[0] == H_V21 and c[2] < c[1] for c in calls_of(r, t))]
        assert len(short) == 1 and 0 < r["lens"][short[0]] < samples and r["transmit"][-1] == 0
        assert r["under"].sum() == 1 and r["steps"].sum() == 3, (r["under"].sum(), r["steps"].sum())
        assert -7 in r["asked"]
        flags["v21_end_in_mid_tick_" + str(samples)] = 1
        out.append((name, r))

    # 6: V.29 9600 with use_hdlc: 240 flags, two frames, the end, the shutdown; the tick after returns 0 and reports
    ops = [[0, SET, V29, 9600, 0, 1], [0, Q_FRAME, 0, 0, 0, 0], [0, Q_FRAME, 1, 0, 0, 0], [0, Q_END, 0, 0, 0, 0]]
    r = run(L, offsets, ops, 50, frames=[f40, f7])
    zero = [t for t in range(50) if (H_FAST, 160, 0) in calls_of(r, t)]
    assert len(zero) == 1 and r["lens"][zero[0]] == 0 and r["steps"][zero[0]] == 1 and r["transmit"][zero[0]] == 0
    assert r["handler"][zero[0] - 1] == H_FAST and r["path"][0] == 2 and r["end"][3] == V29_TX
    flags["v29_hdlc_shutdown_then_zero"] = 1
    out.append(("v29_9600_hdlc", r))

    # 7: non-ECM from the ring with the end of the data
    for type_, rate, name, ticks in ((V29, 7200, "v29_7200", 40), (V27TER, 4800, "v27ter_4800", 70), (V27TER, 2400, "v27ter_2400", 90)):
        n = rate//8
        bits = rng.randint(0, 2, n).astype(np.uint8)
        ops = [[0, SET, type_, rate, 0, 0], [0, BITS, 0, n, 0, 0], [0, EOD, 0, 0, 0, 0]]
        r = run(L, offsets, ops, ticks, bits=bits)
        zero = [t for t in range(ticks) if (H_FAST, 160, 0) in calls_of(r, t)]
        assert len(zero) == 1 and r["steps"].sum() == 1 and len(r["asked"]) == 0 and r["path"][0] == 2
        flags["non_ecm_" + name] = 1
        out.append((name, r))

    # 8: V.17 14400 from init (long training), V17 again after restart() with short_train (the restart path), then V.17 7200
    n = 900
    bits = rng.randint(0, 2, 3*n).astype(np.uint8)
    ops = [[0, SET, V17, 14400, 0, 0], [0, BITS, 0, n, 0, 0], [0, EOD, 0, 0, 0, 0],
           [84, RESTART, 0, 0, 0, 0], [84, SET, V17, 14400, 1, 0], [84, BITS, n, n, 0, 0], [84, EOD, 0, 0, 0, 0],
           [104, RESTART, 0, 0, 0, 0], [104, SET, V17, 7200, 1, 0], [104, BITS, 2*n, n, 0, 0], [104, EOD, 0, 0, 0, 0]]
    r = run(L, offsets, ops, 128, bits=bits)
    sets = [int(p) for p, o in zip(r["path"], r["ops"]) if o[1] == SET]
    assert sets == [2, 3, 3] and r["steps"].sum() == 3 and r["transmit"][83] == 0 and r["transmit"][103] == 0 and r["transmit"][-1] == 0
    flags["v17_init_restart_short_train"] = 1
    out.append(("v17", r))

    # 9: V.29, V.17 and V.29 on one line: the init path each time (each replaced while it trains)
    ops = [[0, SET, V29, 9600, 0, 0], [8, SET, V17, 12000, 0, 0], [16, SET, V29, 4800, 0, 0], [16, BITS, 0, 200, 0, 0], [16, EOD, 0, 0, 0, 0]]
    r = run(L, offsets, ops, 50, bits=bits[:200])
    assert [int(p) for p in r["path"][:3]] == [2, 2, 2] and r["transmit"][-1] == 0
    flags["v29_v17_v29_init_each_time"] = 1
    out.append(("v29_v17_v29", r))

    # 10: TEP on
    ops = [[0, SET, V27TER, 4800, 0, 1], [0, Q_FRAME, 0, 0, 0, 0], [0, Q_END, 0, 0, 0, 0]]
    r = run(L, offsets, ops, 75, use_tep=1, frames=[f7])
    assert r["transmit"][-1] == 0 and np.abs(r["rows"][4]).max() > 1000        # the carrier of the TEP, right behind the silence
    flags["tep"] = 1
    out.append(("v27ter_tep", r))

    # 11: the same type twice: nothing; after restart() it acts
    ops = [[0, SET, PAUSE, 0, 30, 0], [1, SET, PAUSE, 0, 30, 0], [3, RESTART, 0, 0, 0, 0], [3, SET, PAUSE, 0, 30, 0]]
    r = run(L, offsets, ops, 6)
    sets = [int(p) for p, o in zip(r["path"], r["ops"]) if o[1] == SET]
    assert sets == [1, 0, 1] and list(r["lens"]) == [160, 80, 0, 160, 80, 0] and r["steps"].sum() == 2
    flags["same_type_twice"] = 1
    out.append(("same_type", r))

    # 12: DONE
    r = run(L, offsets, [[0, SET, PAUSE, 0, 100, 0], [2, SET, DONE, 0, 0, 0]], 5)
    assert list(r["lens"]) == [160, 160, 0, 0, 0] and list(r["transmit"]) == [1, 1, 0, 0, 0] and not r["rows"].any() and r["steps"].sum() == 0
    # (silence_gen_alter(0): what was left of the pause stays in the generator)
    assert r["end"][0] == 800 - 320
    flags["done"] = 1
    out.append(("done", r))

    # 13: loop.  A: V21 frames, then a V.29 9600 HDLC burst; B: start_slow_modem(V21_RX) ahead of tick 0, start_fast_modem(V29_RX)
    # ahead of the tick A changes in
    t2 = 150
    ops = [[0, SET, V21, 300, 0, 1], [0, Q_FRAME, 0, 0, 0, 0], [0, Q_FRAME, 1, 0, 0, 0], [0, Q_END, 0, 0, 0, 0],
           [t2, SET, V29, 9600, 0, 1], [t2, Q_FRAME, 2, 0, 0, 0], [t2, Q_FRAME, 0, 0, 0, 0], [t2, Q_END, 0, 0, 0, 0]]
    ticks = t2 + 50
    r = run(L, offsets, ops, ticks, frames=[f5, f7, f40])
    assert r["transmit"][t2 - 1] == 0 and r["transmit"][-1] == 0
    rx_ops = np.array([[0, 1, 12, 0, 0, 0], [t2, 2, V29_RX, 9600, 0, 1]], np.int32)
    rx_tick = np.zeros((ticks, 4), np.int32)
    recs = np.zeros(4096, np.int32)
    octets = np.zeros(4096, np.uint8)
    L.run_rx(rx_ops.ctypes.data, len(rx_ops), r["rows"].ctypes.data, ticks, 160, rx_tick.ctypes.data, recs.ctypes.data, octets.ctypes.data)
    each = lambda col: np.diff(np.concatenate([[0], rx_tick[:, col]])).astype(np.int32)
    r.update({"rx_ops": rx_ops, "rx_handler": rx_tick[:, 0].copy(), "rx_frx": rx_tick[:, 1].copy(), "rx_recs": recs[:rx_tick[-1, 2]].copy(),
              "rx_nrecs": each(2), "rx_bytes": octets[:rx_tick[-1, 3]].copy(), "rx_nbytes": each(3)})
    good = [int(x) & 0xFFFF for x in r["rx_recs"] if x >= 0x10000]
    assert good == [5, 7, 40, 5], good
    flags["loop"] = 1
    out.append(("loop", r))
    return out, flags


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    with tempfile.TemporaryDirectory() as d:
        L, offsets = build_reference(ref_src, d)
        got, flags = cases(L, offsets)
    out = {"names": np.array([n for n, _ in got]), "flag_names": np.array(sorted(flags)),
           "flags": np.array([flags[k] for k in sorted(flags)], np.int32)}
    for k, (name, r) in enumerate(got):
        for f, v in r.items():
            out["c%d_%s" % (k, f)] = v
        print(k, name, "ticks", r["cfg"][1], "x", r["cfg"][2], "calls", len(r["calls"]), "steps", int(r["steps"].sum()), "underflows",
              int(r["under"].sum()), "asked", len(r["asked"]), "paths", r["path"].tolist())
    for k in sorted(flags):
        print("flag", k, flags[k])
    np.savez_compressed(GOLDEN, **out)
    size = os.path.getsize(GOLDEN)
    print("wrote", GOLDEN, size, "bytes")
    assert size <= 478071, "larger than the largest fixture committed (v17tx.npz)"


if __name__ == "__main__":
    main()
