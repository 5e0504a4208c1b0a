/*
 * ref_glue_adsi.c -- TEST INFRASTRUCTURE ONLY.  OUR batch drivers over the reference build's caller-ID sender and receiver
 * (src/adsi.c with src/crc.c, src/fsk.c, src/tone_generate.c and what they call), for the ADSI sweep (tests/adsi_sweep.py):
 * one line through a whole schedule of calls inside C, with the state words in the order of the banks
 * (spandsp_amd/csrc/adsi_dev.hpp: ADT_*, then FT_BAUD_RATE .. FT_SHUTDOWN; ADR_*).  Compiled only into
 * oracle/_ref/libspandsp_adsi_ref.so; #includes reference headers from the reference tree at build time.
 */
#include <stdlib.h>
#include <inttypes.h>
#include <string.h>
#include <stdio.h>
#include <stdbool.h>
#include <math.h>

#include "spandsp/telephony.h"
#include "spandsp/alloc.h"
#include "spandsp/fast_convert.h"
#include "spandsp/logging.h"
#include "spandsp/queue.h"
#include "spandsp/complex.h"
#include "spandsp/dds.h"
#include "spandsp/power_meter.h"
#include "spandsp/async.h"
#include "spandsp/crc.h"
#include "spandsp/fsk.h"
#include "spandsp/tone_detect.h"
#include "spandsp/tone_generate.h"
#include "spandsp/super_tone_rx.h"
#include "spandsp/dtmf.h"
#include "spandsp/adsi.h"
#include "spandsp/awgn.h"
#include "spandsp/private/logging.h"
#include "spandsp/private/queue.h"
#include "spandsp/private/tone_generate.h"
#include "spandsp/private/async.h"
#include "spandsp/private/power_meter.h"
#include "spandsp/private/fsk.h"
#include "spandsp/private/dtmf.h"
#include "spandsp/private/adsi.h"

#define GLUE __attribute__((visibility("default")))

int glue_fsk_rx_snapshot(const fsk_rx_state_t *s, int32_t *out);        /* ref_glue_fsk.c */

enum
{
    GLUE_ADSI_TX_WORDS = 24,
    GLUE_ADSI_RX_WORDS = 6,
    GLUE_ADSI_FSK_WORDS = 28,
    GLUE_ADSI_MSG = 256
};

/* a sender's operations, each ahead of the call it is tagged with */
enum
{
    OP_PUT = 1,             /* a0: offset into the operations' bytes, a1: length */
    OP_PREAMBLE = 2,        /* a0 .. a3 */
    OP_ALERT = 3,
    OP_RESTART = 4,         /* adsi_tx_init() on the object, as the bank's restart */
    OP_SHUT_DOWN = 5        /* the modulator's shutdown flag set by hand, as a bank's set_state can: no call leads there */
};

GLUE int glue_adsi_words(int which)
{
    static const int n[4] = {GLUE_ADSI_TX_WORDS, GLUE_ADSI_RX_WORDS, GLUE_ADSI_FSK_WORDS, GLUE_ADSI_MSG};

    return (which >= 0  &&  which < 4)  ?  n[which]  :  -1;
}

static int preset_of(int standard)
{
    return (standard == ADSI_STANDARD_CLASS)  ?  FSK_BELL202  :  FSK_V23CH1;
}

static void tx_words(const adsi_tx_state_t *s, int32_t *w)
{
    int n = 0;

    w[n++] = s->standard;
    w[n++] = s->preamble_len;
    w[n++] = s->preamble_ones_len;
    w[n++] = s->postamble_ones_len;
    w[n++] = s->stop_bits;
    w[n++] = s->byte_no;
    w[n++] = s->bit_pos;
    w[n++] = s->bit_no;
    w[n++] = s->msg_len;
    w[n++] = s->tx_signal_on;
    w[n++] = s->alert_tone_gen.current_section;
    w[n++] = s->alert_tone_gen.current_position;
    w[n++] = (int32_t) s->alert_tone_gen.phase[0];
    w[n++] = (int32_t) s->alert_tone_gen.phase[1];
    w[n++] = s->alert_tone_gen.duration[0];
    w[n++] = s->alert_tone_gen.duration[1];
    w[n++] = s->fsk_tx.baud_rate;
    w[n++] = s->fsk_tx.phase_rates[0];
    w[n++] = s->fsk_tx.phase_rates[1];
    w[n++] = s->fsk_tx.scaling;
    w[n++] = s->fsk_tx.current_phase_rate;
    w[n++] = (int32_t) s->fsk_tx.phase_acc;
    w[n++] = s->fsk_tx.baud_frac;
    w[n++] = s->fsk_tx.shutdown;
}

/* One sender line.  ops[n_ops][6]: call, operation, a0 .. a3, sorted by call; lens[n_calls].  Call k's samples go to
   pcm + (lens[0] + .. + lens[k - 1]), which the caller zeroed: what lies behind a call's returned length stays zero.
   results[n_ops]: what a put returned (0 for the other operations).  words[n_calls][24] after every call; msg[256] at the
   end.  Returns the sum of the returned lengths. */
GLUE int glue_adsi_tx_run(int standard, const int32_t *ops, int n_ops, const uint8_t *opbytes, const int32_t *lens, int n_calls,
                          int16_t *pcm, int32_t *out_lens, int32_t *results, int32_t *words, uint8_t *msg)
{
    adsi_tx_state_t *s;
    int k;
    int op = 0;
    int total = 0;
    int at = 0;

    if ((s = adsi_tx_init(NULL, standard)) == NULL)
        return -1;
    for (k = 0;  k < n_calls;  k++)
    {
        for (  ;  op < n_ops  &&  ops[op*6] <= k;  op++)
        {
            const int32_t *o = ops + op*6;

            results[op] = 0;
            switch (o[1])
            {
            case OP_PUT:
                results[op] = adsi_tx_put_message(s, opbytes + o[2], o[3]);
                break;
            case OP_PREAMBLE:
                adsi_tx_set_preamble(s, o[2], o[3], o[4], o[5]);
                break;
            case OP_ALERT:
                adsi_tx_send_alert_tone(s);
                break;
            case OP_RESTART:
                adsi_tx_init(s, standard);
                break;
            case OP_SHUT_DOWN:
                s->fsk_tx.shutdown = true;
                break;
            default:
                adsi_tx_free(s);
                return -2;
            }
        }
        out_lens[k] = (lens[k] > 0)  ?  adsi_tx(s, pcm + at, lens[k])  :  0;
        at += lens[k];
        total += out_lens[k];
        tx_words(s, words + k*GLUE_ADSI_TX_WORDS);
    }
    for (  ;  op < n_ops;  op++)
        results[op] = 0;
    memcpy(msg, s->msg, GLUE_ADSI_MSG);
    adsi_tx_free(s);
    return total;
}

struct rx_record
{
    uint8_t *msgs;
    int32_t *msg_lens;
    int32_t *msg_calls;
    int room;
    int n;
    int call;
};

static void put_msg(void *user_data, const uint8_t *msg, int len)
{
    struct rx_record *r = (struct rx_record *) user_data;

    if (r->n < r->room)
    {
        memcpy(r->msgs + (size_t) r->n*GLUE_ADSI_MSG, msg, len);
        r->msg_lens[r->n] = len;
        r->msg_calls[r->n] = r->call;
    }
    r->n++;
}

struct bit_record
{
    int8_t *bits;
    int room;
    int n;
};

static void record_bit(void *user_data, int bit)
{
    struct bit_record *r = (struct bit_record *) user_data;

    if (r->n < r->room)
        r->bits[r->n] = (int8_t) bit;
    r->n++;
}

/* One receiver line: lens[n_calls] samples of amp a call, zeros allowed.  msgs[room][256], msg_lens[room], msg_calls[room]:
   every delivered message with the call it arrived in; counts[n_calls]; words[n_calls][6] and fsk_words[n_calls][28] after
   every call; msg[256] at the end.  bits[bit_room] / bit_counts[n_calls] (or null): what a second fsk_rx of the same preset
   in asynchronous framing hands to a recording put_bit, bits and statuses, counted by call -- the stream the receiver's own
   demodulator hands to the framer.  Returns the number of messages (above room: the record is cut short). */
GLUE int glue_adsi_rx_run(int standard, const int16_t *amp, const int32_t *lens, int n_calls, uint8_t *msgs, int32_t *msg_lens,
                          int32_t *msg_calls, int room, int32_t *counts, int32_t *words, int32_t *fsk_words, uint8_t *msg,
                          int8_t *bits, int bit_room, int32_t *bit_counts)
{
    struct rx_record rec = {msgs, msg_lens, msg_calls, room, 0, 0};
    struct bit_record rb = {bits, bit_room, 0};
    adsi_rx_state_t *s;
    fsk_rx_state_t *f = NULL;
    int32_t snap[GLUE_ADSI_FSK_WORDS + 4*128];
    int k;
    int at = 0;

    if ((s = adsi_rx_init(NULL, standard, put_msg, &rec)) == NULL)
        return -1;
    if (bits  &&  (f = fsk_rx_init(NULL, &preset_fsk_specs[preset_of(standard)], FSK_FRAME_MODE_ASYNC, record_bit, &rb)) == NULL)
    {
        adsi_rx_free(s);
        return -1;
    }
    for (k = 0;  k < n_calls;  k++)
    {
        const int before = rec.n;
        const int bits_before = rb.n;
        int32_t *w = words + k*GLUE_ADSI_RX_WORDS;

        rec.call = k;
        if (lens[k] > 0)
        {
            adsi_rx(s, amp + at, lens[k]);
            if (f)
                fsk_rx(f, amp + at, lens[k]);
        }
        at += lens[k];
        counts[k] = rec.n - before;
        if (bit_counts)
            bit_counts[k] = rb.n - bits_before;
        w[0] = s->standard;
        w[1] = s->consecutive_ones;
        w[2] = s->bit_pos;
        w[3] = s->in_progress;
        w[4] = s->msg_len;
        w[5] = s->framing_errors;
        if (fsk_words)
        {
            glue_fsk_rx_snapshot(&s->fsk_rx, snap);
            memcpy(fsk_words + k*GLUE_ADSI_FSK_WORDS, snap, GLUE_ADSI_FSK_WORDS*sizeof(int32_t));
        }
    }
    memcpy(msg, s->msg, GLUE_ADSI_MSG);
    adsi_rx_free(s);
    if (f)
        fsk_rx_free(f);
    return (rb.n > bit_room  &&  bits)  ?  -3  :  rec.n;
}

/* The run-length modulator: runs[n_runs][2] of (bit, samples) as one continuous-phase line at the two frequencies and the
   level of the FSK preset of `standard`, on the reference's dds as fsk_tx() uses it (fsk.c:168-170, 203), scaled by
   num/den (den 0: as the preset has it).  It renders what fsk_tx() cannot: bits of any length.  Returns the samples. */
GLUE int glue_adsi_runs_line(int standard, const int32_t *runs, int n_runs, int num, int den, int16_t *amp, int room)
{
    const fsk_spec_t *spec = &preset_fsk_specs[preset_of(standard)];
    int32_t rates[2];
    int16_t scaling;
    uint32_t phase_acc = 0;
    int i;
    int j;
    int n = 0;

    rates[0] = dds_phase_rate((float) spec->freq_zero);
    rates[1] = dds_phase_rate((float) spec->freq_one);
    scaling = dds_scaling_dbm0((float) spec->tx_level);
    for (i = 0;  i < n_runs;  i++)
    {
        for (j = 0;  j < runs[2*i + 1];  j++)
        {
            int32_t v = dds_mod(&phase_acc, rates[runs[2*i] & 1], scaling, 0);

            if (n >= room)
                return -1;
            if (den > 0)
                v = v*num/den;
            amp[n++] = (int16_t) ((v > 32767)  ?  32767  :  ((v < -32768)  ?  -32768  :  v));
        }
    }
    return n;
}

/* A burst of the reference's own sender: the message as adsi_tx_put_message() takes it, an alert tone in front and a
   preamble of the caller's if asked (preamble[4], or null), run in calls of 160 samples to its end.  Returns the samples. */
GLUE int glue_adsi_tx_burst(int standard, const uint8_t *m, int len, int alert, const int32_t *preamble, int16_t *amp, int room)
{
    adsi_tx_state_t *s;
    int n = 0;
    int got;

    if ((s = adsi_tx_init(NULL, standard)) == NULL)
        return -1;
    if (preamble)
        adsi_tx_set_preamble(s, preamble[0], preamble[1], preamble[2], preamble[3]);
    if (alert)
        adsi_tx_send_alert_tone(s);
    if (adsi_tx_put_message(s, m, len) <= 0)
    {
        adsi_tx_free(s);
        return -2;
    }
    while (n + 160 <= room  &&  (got = adsi_tx(s, amp + n, 160)) > 0)
        n += got;
    adsi_tx_free(s);
    return n;
}

/* A line attenuated to num/den with the reference's AWGN at `noise_dbm0` on top (seed: awgn_init_dbm0()'s idum); a level
   of 0 or above adds no noise.  In place, saturating. */
GLUE int glue_adsi_impair(int16_t *amp, int n, int num, int den, int seed, int noise_dbm0)
{
    awgn_state_t *noise = NULL;
    int i;

    if (den <= 0  ||  (noise_dbm0 < 0  &&  (noise = awgn_init_dbm0(NULL, seed, (float) noise_dbm0)) == NULL))
        return -1;
    for (i = 0;  i < n;  i++)
    {
        int32_t v = amp[i]*num/den + (noise  ?  awgn(noise)  :  0);

        amp[i] = (int16_t) ((v > 32767)  ?  32767  :  ((v < -32768)  ?  -32768  :  v));
    }
    if (noise)
        awgn_free(noise);
    return n;
}

/* One sender line asked for bits: the script of glue_adsi_tx_run(), but call k takes lens[k] bits straight from the
   sender's get_bit (the one start_tx() gave its modulator), with no modulator and no alert tone in between.  bits: 0, 1 or
   a status; words[n_calls][10]: the message layer's (ADT_STANDARD .. ADT_TX_SIGNAL_ON) after every call. */
GLUE int glue_adsi_tx_bits(int standard, const int32_t *ops, int n_ops, const uint8_t *opbytes, const int32_t *lens, int n_calls,
                           int8_t *bits, int32_t *results, int32_t *words)
{
    adsi_tx_state_t *s;
    int32_t w[GLUE_ADSI_TX_WORDS];
    int k;
    int i;
    int op = 0;
    int n = 0;

    if ((s = adsi_tx_init(NULL, standard)) == NULL)
        return -1;
    for (k = 0;  k < n_calls;  k++)
    {
        for (  ;  op < n_ops  &&  ops[op*6] <= k;  op++)
        {
            const int32_t *o = ops + op*6;

            results[op] = 0;
            if (o[1] == OP_PUT)
                results[op] = adsi_tx_put_message(s, opbytes + o[2], o[3]);
            else if (o[1] == OP_PREAMBLE)
                adsi_tx_set_preamble(s, o[2], o[3], o[4], o[5]);
            else if (o[1] == OP_RESTART)
                adsi_tx_init(s, standard);
        }
        for (i = 0;  i < lens[k];  i++)
            bits[n++] = (int8_t) s->fsk_tx.get_bit(s->fsk_tx.get_bit_user_data);
        tx_words(s, w);
        memcpy(words + k*10, w, 10*sizeof(int32_t));
    }
    for (  ;  op < n_ops;  op++)
        results[op] = 0;
    adsi_tx_free(s);
    return n;
}
