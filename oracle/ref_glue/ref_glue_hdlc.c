/*
 * ref_glue_hdlc.c -- TEST INFRASTRUCTURE ONLY.  OUR drivers over the reference's HDLC framer (src/hdlc.c, src/crc.c): two
 * accessors that hand out a receiver's and a sender's state as the banks' state words, in the banks' word order
 * (hdlc_dev.hpp HR_*, HT_*), read out of the reference's private structs field by field, and two batch drivers that take one
 * line through a whole schedule of calls, so that a sweep of thousands of lines pays one foreign call a line.  Compiled only
 * into oracle/_ref/libspandsp_hdlc_ref.so; #includes reference headers at build time.
 *
 * State words after the calls asked for lie one set behind the other in `words`: call k where want[k] != 0, or the last call
 * alone where want is NULL.
 */
#include <stdlib.h>
#include <stddef.h>
#include <inttypes.h>
#include <string.h>
#include <stdio.h>
#include <stdbool.h>

#include "spandsp/telephony.h"
#include "spandsp/alloc.h"
#include "spandsp/async.h"
#include "spandsp/crc.h"
#include "spandsp/hdlc.h"
#include "spandsp/private/hdlc.h"

#define GLUE __attribute__((visibility("default")))

#define HDLC_RX_WORDS   18
#define HDLC_TX_WORDS   16
#define HDLC_BUF        (HDLC_MAXFRAME_LEN + 4)

/* control operations ahead of a receiver's call */
#define OP_MAX_FRAME_LEN    1
#define OP_REPORT_INTERVAL  2
#define OP_RESTART          3

/* a sender's commands (hdlc_dev.hpp kHdlcCmd*) */
#define CMD_FRAME   1
#define CMD_FLAGS   2
#define CMD_ABORT   3
#define CMD_END     4

#define MAX_DEPTH   64

static bool wanted(const int32_t want[], int k, int n_calls)
{
    return (want)  ?  (want[k] != 0)  :  (k == n_calls - 1);
}

GLUE int glue_hdlc_state_words(int sender)
{
    return (sender)  ?  HDLC_TX_WORDS  :  HDLC_RX_WORDS;
}

/* the order of HR_* */
GLUE int glue_hdlc_rx_words(const hdlc_rx_state_t *s, int32_t w[HDLC_RX_WORDS])
{
    int at = 0;

    w[at++] = (int32_t) s->crc_bytes;
    w[at++] = (int32_t) s->max_frame_len;
    w[at++] = (int32_t) s->report_bad_frames;
    w[at++] = (int32_t) s->framing_ok_threshold;
    w[at++] = (int32_t) s->framing_ok_announced;
    w[at++] = (int32_t) s->flags_seen;
    w[at++] = (int32_t) s->raw_bit_stream;
    w[at++] = (int32_t) s->byte_in_progress;
    w[at++] = (int32_t) s->num_bits;
    w[at++] = (int32_t) s->octet_counting_mode;
    w[at++] = (int32_t) s->octet_count;
    w[at++] = (int32_t) s->octet_count_report_interval;
    w[at++] = (int32_t) s->len;
    w[at++] = (int32_t) s->rx_bytes;
    w[at++] = (int32_t) s->rx_frames;
    w[at++] = (int32_t) s->rx_crc_errors;
    w[at++] = (int32_t) s->rx_length_errors;
    w[at++] = (int32_t) s->rx_aborts;
    return at;
}

/* the order of HT_*, up to the reference's last field */
GLUE int glue_hdlc_tx_words(const hdlc_tx_state_t *s, int32_t w[HDLC_TX_WORDS])
{
    int at = 0;

    w[at++] = (int32_t) s->crc_bytes;
    w[at++] = (int32_t) s->inter_frame_flags;
    w[at++] = (int32_t) s->progressive;
    w[at++] = (int32_t) s->max_frame_len;
    w[at++] = (int32_t) s->octets_in_progress;
    w[at++] = (int32_t) s->num_bits;
    w[at++] = (int32_t) s->idle_octet;
    w[at++] = (int32_t) s->flag_octets;
    w[at++] = (int32_t) s->abort_octets;
    w[at++] = (int32_t) s->report_flag_underflow;
    w[at++] = (int32_t) s->len;
    w[at++] = (int32_t) s->pos;
    w[at++] = (int32_t) s->crc;
    w[at++] = (int32_t) s->byte;
    w[at++] = (int32_t) s->bits;
    w[at++] = (int32_t) s->tx_end;
    return at;
}

GLUE void glue_hdlc_rx_buffer(const hdlc_rx_state_t *s, uint8_t out[HDLC_BUF])
{
    memcpy(out, s->buffer, HDLC_BUF);
}

GLUE void glue_hdlc_tx_buffer(const hdlc_tx_state_t *s, uint8_t out[HDLC_BUF])
{
    memcpy(out, s->buffer, HDLC_BUF);
}

/* ---- receiver ----------------------------------------------------------------------------------------------------------- */

typedef struct
{
    int32_t *recs;
    uint8_t *bytes;
    int rec_room;
    int byte_room;
    int n_recs;
    int n_bytes;
} rx_sink_t;

/* the bank's encoding of a handler call: a status code, or len | ok << 16 with the frame's octets behind the others */
static void rx_status(void *user_data, int status)
{
    rx_sink_t *k = (rx_sink_t *) user_data;

    if (k->n_recs < k->rec_room)
        k->recs[k->n_recs] = status;
    k->n_recs++;
}

static void rx_frame(void *user_data, const uint8_t *pkt, int len, int ok)
{
    rx_sink_t *k = (rx_sink_t *) user_data;

    if (k->n_recs < k->rec_room)
        k->recs[k->n_recs] = len | ((ok)  ?  0x10000  :  0);
    k->n_recs++;
    if (len > 0  &&  k->n_bytes + len <= k->byte_room)
        memcpy(k->bytes + k->n_bytes, pkt, len);
    k->n_bytes += len;
}

static void rx_control(hdlc_rx_state_t *s, int op, int value)
{
    switch (op)
    {
    case OP_MAX_FRAME_LEN:
        hdlc_rx_set_max_frame_len(s, (size_t) value);
        break;
    case OP_REPORT_INTERVAL:
        hdlc_rx_set_octet_counting_report_interval(s, value);
        break;
    case OP_RESTART:
        hdlc_rx_restart(s);
        break;
    }
}

/* One receiver through n_calls calls.  events: int16_t entries for hdlc_rx_put_bit(), or where `octets` is set uint8_t for
   hdlc_rx_put(); lens[k] of them go into call k.  ops: [n_ops][3] = call, operation, value, applied in their order ahead of
   that call (a call below zero: behind the init); a call of length 0 is not made and its operations are not either.
   n_recs[k], n_bytes[k]: what the handlers were handed in call k; recs and bytes: all calls back to back.  buffer: the 404
   octets at the end.  Returns the records of all calls, -1 where the init fails, -2 where recs or bytes has no room. */
GLUE int glue_hdlc_rx_run(int crc32, int report_bad_frames, int framing_ok_threshold, const void *events, int octets,
                          const int32_t lens[], int n_calls, const int32_t ops[], int n_ops, int32_t recs[], int rec_room,
                          uint8_t bytes[], int byte_room, int32_t n_recs[], int32_t n_bytes[], int32_t words[],
                          const int32_t want[], uint8_t buffer[HDLC_BUF])
{
    rx_sink_t sink = {recs, bytes, rec_room, byte_room, 0, 0};
    hdlc_rx_state_t *s;
    const int16_t *ev = (const int16_t *) events;
    const uint8_t *oct = (const uint8_t *) events;
    size_t at = 0;
    int k;
    int i;

    if ((s = hdlc_rx_init(NULL, crc32 != 0, report_bad_frames != 0, framing_ok_threshold, rx_frame, &sink)) == NULL)
        return -1;
    hdlc_rx_set_status_handler(s, rx_status, &sink);
    for (i = 0;  i < n_ops;  i++)
    {
        if (ops[3*i] < 0)
            rx_control(s, ops[3*i + 1], ops[3*i + 2]);
    }
    for (k = 0;  k < n_calls;  k++)
    {
        const int before_recs = sink.n_recs;
        const int before_bytes = sink.n_bytes;

        if (lens[k] > 0)
        {
            for (i = 0;  i < n_ops;  i++)
            {
                if (ops[3*i] == k)
                    rx_control(s, ops[3*i + 1], ops[3*i + 2]);
            }
            if (octets)
            {
                hdlc_rx_put(s, oct + at, lens[k]);
            }
            else
            {
                for (i = 0;  i < lens[k];  i++)
                    hdlc_rx_put_bit(s, ev[at + i]);
            }
            at += lens[k];
        }
        n_recs[k] = sink.n_recs - before_recs;
        n_bytes[k] = sink.n_bytes - before_bytes;
        if (wanted(want, k, n_calls))
            words += glue_hdlc_rx_words(s, words);
    }
    if (buffer)
        memcpy(buffer, s->buffer, HDLC_BUF);
    hdlc_rx_free(s);
    return (sink.n_recs > rec_room  ||  sink.n_bytes > byte_room)  ?  -2  :  sink.n_recs;
}

/* ---- sender ------------------------------------------------------------------------------------------------------------- */

typedef struct
{
    int kind;
    int arg;
    int corrupt;
    const uint8_t *bytes;
} tx_cmd_t;

/* the reference's sender with a FIFO of commands behind its underflow handler: what a bank's queue stands for */
typedef struct
{
    hdlc_tx_state_t *s;
    tx_cmd_t fifo[MAX_DEPTH];
    int head;
    int count;
    int depth;
    int under;
    int taken;          /* the kinds of command taken in this call: 1 << kind by the handler, 0x100 << kind between calls */
} tx_driver_t;

static void tx_take(tx_driver_t *d, int by_handler)
{
    const tx_cmd_t c = d->fifo[d->head];

    d->head = (d->head + 1) % d->depth;
    d->count--;
    d->taken |= ((by_handler)  ?  1  :  0x100) << c.kind;
    switch (c.kind)
    {
    case CMD_FRAME:
        /* (a frame of no octets is the end of the data) */
        if (hdlc_tx_frame(d->s, c.bytes, (size_t) c.arg) == 0  &&  c.arg > 0  &&  c.corrupt)
            hdlc_tx_corrupt_frame(d->s);
        break;
    case CMD_FLAGS:
        hdlc_tx_flags(d->s, c.arg);
        break;
    case CMD_ABORT:
        hdlc_tx_abort(d->s);
        break;
    case CMD_END:
        hdlc_tx_frame(d->s, NULL, 0);
        break;
    }
}

static void tx_underflow(void *user_data)
{
    tx_driver_t *d = (tx_driver_t *) user_data;

    if (d->count > 0)
        tx_take(d, 1);
    else
        d->under++;
}

static int tx_offer(tx_driver_t *d, tx_cmd_t c)
{
    if (d->count >= d->depth  ||  (c.kind == CMD_FRAME  &&  c.arg > (int) d->s->max_frame_len))
        return -1;
    d->fifo[(d->head + d->count) % d->depth] = c;
    d->count++;
    return 0;
}

/* One sender through n_calls calls of wants[k] bits.  ops: [n_ops][4] = call, command, argument (a frame's length, a flag
   count), corrupt, offered in their order ahead of that call; opbytes: the octets of the FRAME commands back to back.
   A call that wants no bits is sat out whole: its offers still reach the FIFO, nothing is taken from it.
   bits: one bit a byte, all calls back to back; lens[k]: the bits of call k; under[k]: the handler calls of call k that
   found the FIFO empty; ended[k]: the call stopped on SIG_STATUS_END_OF_DATA; taken[k]: the kinds of command call k took,
   1 << kind by the handler and 0x100 << kind between calls; results[i]: what offer i returned.
   max_frame_len below zero: not set.  buffer: the 404 octets at the end.  Returns the bits of all calls, or -1. */
GLUE int glue_hdlc_tx_run(int crc32, int inter_frame_flags, int depth, int max_frame_len, const int32_t ops[],
                          const uint8_t opbytes[], int n_ops, const int32_t wants[], int n_calls, uint8_t bits[],
                          int32_t lens[], int32_t under[], int32_t ended[], int32_t taken[], int32_t results[],
                          int32_t words[], const int32_t want[], uint8_t buffer[HDLC_BUF])
{
    tx_driver_t d;
    size_t byte_at = 0;
    int total = 0;
    int next_op = 0;
    int k;
    int i;

    if (depth < 1  ||  depth > MAX_DEPTH)
        return -1;
    memset(&d, 0, sizeof(d));
    d.depth = depth;
    if ((d.s = hdlc_tx_init(NULL, crc32 != 0, inter_frame_flags, false, tx_underflow, &d)) == NULL)
        return -1;
    if (max_frame_len >= 0)
        hdlc_tx_set_max_frame_len(d.s, (size_t) max_frame_len);
    for (k = 0;  k < n_calls;  k++)
    {
        /* (the operations are sorted by call) */
        for (  ;  next_op < n_ops  &&  ops[4*next_op] <= k;  next_op++)
        {
            tx_cmd_t c = {ops[4*next_op + 1], ops[4*next_op + 2], ops[4*next_op + 3], NULL};

            if (c.kind == CMD_FRAME)
            {
                c.bytes = opbytes + byte_at;
                byte_at += (size_t) c.arg;
            }
            results[next_op] = tx_offer(&d, c);
        }
        lens[k] = 0;
        under[k] = 0;
        ended[k] = 0;
        taken[k] = 0;
        if (wants[k] > 0)
        {
            /* between calls an idle sender is offered the FIFO: commands until a frame is in or nothing is left */
            d.taken = 0;
            while (d.s->len == 0  &&  d.count > 0)
                tx_take(&d, 0);
            d.under = 0;
            for (i = 0;  i < wants[k];  i++)
            {
                const int bit = hdlc_tx_get_bit(d.s);

                if (bit < 0)
                {
                    ended[k] = 1;
                    break;
                }
                bits[total + i] = (uint8_t) bit;
            }
            lens[k] = i;
            total += i;
            under[k] = d.under;
            taken[k] = d.taken;
        }
        if (wanted(want, k, n_calls))
            words += glue_hdlc_tx_words(d.s, words);
    }
    for (  ;  next_op < n_ops;  next_op++)
        results[next_op] = 0;
    if (buffer)
        memcpy(buffer, d.s->buffer, HDLC_BUF);
    hdlc_tx_free(d.s);
    return total;
}
