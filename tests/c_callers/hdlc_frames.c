/* hdlc_frames.c -- the V.21 control channel of a fax front end from plain C against include/spangpu.h: an HDLC sender bank
 * feeds an FSK sender bank's bit rings (V.21 channel 2), an FSK receiver bank demodulates what was sent, synchronously, and an
 * HDLC receiver bank frames its events.  Host memory throughout, one call per bank and tick of 160 samples.
 *
 *   hdlc_frames <ticks> <preamble flags> <framing_ok_threshold> <frame as hex> ...
 *
 * prints a line per handler call of line 0 -- "s <tick> <status>" or "f <tick> <len> <ok> <hex>" -- and fails where another
 * line saw anything else.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu.h"

#define LINES 130
#define TICK 160
#define STRIDE 8            /* octets of bits per line and tick: 6 bits are due at 300 baud */
#define MAX_FRAMES 8

#define TRY(call) do { int rc_ = (call); if (rc_ < 0) { fprintf(stderr, "%s: %d %s\n", #call, rc_, spangpu_last_error()); return 1; } } while (0)

static uint8_t bits[LINES*STRIDE];
static int32_t lens[LINES];
static int16_t pcm[LINES*TICK];
static uint8_t frames[LINES*SPANGPU_HDLC_BUFFER_BYTES];

static int from_hex(const char *hex, uint8_t *out, int max)
{
    int n = (int) strlen(hex)/2;
    int i;
    unsigned int v;

    if (n > max)
        return -1;
    for (i = 0;  i < n;  i++)
    {
        if (sscanf(hex + 2*i, "%2x", &v) != 1)
            return -1;
        out[i] = (uint8_t) v;
    }
    return n;
}

int main(int argc, char **argv)
{
    spangpu_hdlc_tx_t *htx;
    spangpu_hdlc_rx_t *hrx;
    spangpu_fsktx_t *ftx;
    spangpu_fsk_t *frx;
    spangpu_fsk_spec_t spec;
    int32_t flens[LINES];
    int32_t results[LINES];
    int ticks;
    int t;
    int i;
    int c;
    int baud_frac = 0;

    if (argc < 5  ||  argc > 4 + MAX_FRAMES)
    {
        fprintf(stderr, "usage: hdlc_frames <ticks> <preamble flags> <framing_ok_threshold> <frame as hex> ...\n");
        return 2;
    }
    ticks = atoi(argv[1]);
    TRY(spangpu_fsk_preset(SPANGPU_FSK_V21CH2, &spec));
    TRY(spangpu_hdlc_tx_create(&htx, 0, LINES, 0, 1, 0, MAX_FRAMES + 1));
    TRY(spangpu_hdlc_rx_create(&hrx, 0, LINES, 0, 0, atoi(argv[3])));
    TRY(spangpu_fsktx_create(&ftx, 0, LINES, &spec, SPANGPU_FSKTX_QUEUE, NULL, 256));
    TRY(spangpu_fsk_create(&frx, 0, LINES, &spec, SPANGPU_FSK_FRAME_MODE_SYNC));
    /* the preamble, then the frames: queued ahead, taken where hdlc_tx_get_byte() would call the underflow handler */
    TRY(spangpu_hdlc_tx_flags(htx, 0, LINES, atoi(argv[2]), results));
    for (i = 4;  i < argc;  i++)
    {
        int n = from_hex(argv[i], frames, SPANGPU_HDLC_BUFFER_BYTES);

        if (n <= 0)
            return 2;
        for (c = 0;  c < LINES;  c++)
        {
            memcpy(frames + c*SPANGPU_HDLC_BUFFER_BYTES, frames, (size_t) n);
            flens[c] = n;
        }
        TRY(spangpu_hdlc_tx_frames(htx, 0, LINES, frames, SPANGPU_HDLC_BUFFER_BYTES, flens, NULL, results));
        for (c = 0;  c < LINES;  c++)
        {
            if (results[c] != 0)
            {
                fprintf(stderr, "line %d refused frame %d\n", c, i - 4);
                return 1;
            }
        }
    }
    for (t = 0;  t < ticks;  t++)
    {
        const int16_t *events;
        const int32_t *counts;
        const int32_t *recs;
        const int32_t *rec_counts;
        const uint8_t *bytes;
        int cap;
        int rec_cap;
        int byte_cap;
        int at = 0;
        int due = (int) spangpu_fsktx_bits_due(spec.baud_rate, baud_frac, TICK);

        baud_frac = (int) (((long long) baud_frac + (long long) TICK*spec.baud_rate) % 800000);
        TRY(spangpu_hdlc_tx_get_bits(htx, SPANGPU_MEM_HOST, bits, STRIDE, NULL, due, lens));
        TRY(spangpu_fsktx_put_bits(ftx, 0, LINES, bits, STRIDE, lens, NULL));
        TRY(spangpu_fsktx_tx(ftx, SPANGPU_MEM_HOST, pcm, TICK, TICK, NULL));
        TRY(spangpu_fsk_rx(frx, pcm, SPANGPU_MEM_HOST, TICK, TICK));
        TRY(cap = spangpu_fsk_events(frx, &events, &counts));
        TRY(spangpu_hdlc_rx_put_events(hrx, SPANGPU_MEM_HOST, events, 2, cap, counts));
        TRY(rec_cap = spangpu_hdlc_rx_records(hrx, &recs, &rec_counts, &bytes));
        TRY(spangpu_hdlc_rx_capacity(cap, &i, &byte_cap));
        for (c = 1;  c < LINES;  c++)
        {
            if (rec_counts[c] != rec_counts[0]  ||  rec_counts[LINES + c] != rec_counts[LINES]
                ||  memcmp(recs + (size_t) c*rec_cap, recs, (size_t) rec_counts[0]*sizeof(int32_t)) != 0
                ||  memcmp(bytes + (size_t) c*byte_cap, bytes, (size_t) rec_counts[LINES]) != 0)
            {
                fprintf(stderr, "tick %d: line %d differs from line 0\n", t, c);
                return 1;
            }
        }
        for (i = 0;  i < rec_counts[0];  i++)
        {
            if (recs[i] < 0)
                printf("s %d %d\n", t, (int) recs[i]);
            else
            {
                int n = recs[i] & 0xFFFF;
                int k;

                printf("f %d %d %d ", t, n, (int) (recs[i] >> 16) & 1);
                for (k = 0;  k < n;  k++)
                    printf("%02x", bytes[at + k]);
                printf("\n");
                at += n;
            }
        }
    }
    spangpu_hdlc_tx_destroy(htx);
    spangpu_hdlc_rx_destroy(hrx);
    spangpu_fsktx_destroy(ftx);
    spangpu_fsk_destroy(frx);
    return 0;
}
