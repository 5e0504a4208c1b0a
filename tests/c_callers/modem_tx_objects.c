/* A C caller: a payload from a v29_tx object (get_bit callback, end of data, status handler) in 160-sample frames into a
 * v29_rx object (put_bit callback) -- the receiver trains, delivers the payload bit for bit, and sees the carrier drop after
 * the sender's shutdown.  Own code; exits 0 on success. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu_spandsp.h"

#define PAYLOAD_BITS    1000
#define MAX_BITS        4000

typedef struct
{
    unsigned char bits[PAYLOAD_BITS];
    int next;
    int calls;
    int end_of_data;
    int shutdown_complete;
} source_t;

typedef struct
{
    int n_bits;
    int trained_at;
    int failed;
    int carrier_down;
    unsigned char bits[MAX_BITS];
} sink_t;

static int get_bit(void *user_data)
{
    source_t *s = (source_t *) user_data;

    s->calls++;
    if (s->next >= PAYLOAD_BITS)
        return SIG_STATUS_END_OF_DATA;
    return s->bits[s->next++];
}

static void tx_status(void *user_data, int status)
{
    source_t *s = (source_t *) user_data;

    if (status == SIG_STATUS_END_OF_DATA)
        s->end_of_data++;
    else if (status == SIG_STATUS_SHUTDOWN_COMPLETE)
        s->shutdown_complete++;
}

static void put_bit(void *user_data, int bit)
{
    sink_t *p = (sink_t *) user_data;

    if (bit < 0)
    {
        if (bit == SIG_STATUS_TRAINING_SUCCEEDED)
            p->trained_at = p->n_bits;
        else if (bit == SIG_STATUS_TRAINING_FAILED)
            p->failed = 1;
        else if (bit == SIG_STATUS_CARRIER_DOWN)
            p->carrier_down = 1;
        return;
    }
    if (!p->carrier_down  &&  p->n_bits < MAX_BITS)
        p->bits[p->n_bits++] = (unsigned char) bit;
}

int main(void)
{
    static source_t source;
    static sink_t sink;
    v29_tx_state_t *tx;
    v29_rx_state_t *rx;
    int16_t amp[160];
    unsigned st = 0x2A5;
    int frame;
    int quiet = 0;
    int at;
    int i;

    for (i = 0;  i < PAYLOAD_BITS;  i++)
    {
        st = st*1103515245u + 12345u;
        source.bits[i] = (unsigned char) ((st >> 16) & 1);
    }
    sink.trained_at = -1;
    if ((tx = v29_tx_init(NULL, 9600, false, get_bit, &source)) == NULL
        ||  (rx = v29_rx_init(NULL, 9600, put_bit, &sink)) == NULL)
    {
        fprintf(stderr, "init failed: %s\n", spangpu_last_error());
        return 2;
    }
    if (v29_tx_init(NULL, 1200, false, get_bit, &source) != NULL  ||  v29_tx_get_logging_state(tx) == NULL)
        return 3;
    v29_tx_set_modem_status_handler(tx, tx_status, &source);
    v29_tx_power(tx, -12.0f);
    for (frame = 0;  frame < 60  &&  quiet < 3;  frame++)
    {
        const int got = v29_tx(tx, amp, 160);

        if (got == 0)
            quiet++;
        /* past its shutdown the sender writes nothing: the line is silent */
        memset(amp + got, 0, (size_t) (160 - got)*sizeof(int16_t));
        if (v29_rx(rx, amp, 160) != 0)
            return 4;
    }
    printf("modem_tx_objects: %d get_bit calls, trained after %d bits, %d bits received\n", source.calls, sink.trained_at, sink.n_bits);
    if (quiet < 3  ||  source.calls != PAYLOAD_BITS + 1  ||  source.end_of_data != 1  ||  source.shutdown_complete != 1)
        return 5;
    if (sink.failed  ||  sink.trained_at < 0  ||  !sink.carrier_down)
        return 6;
    /* the payload, behind nothing but the ones that end the training */
    for (at = sink.trained_at;  at + PAYLOAD_BITS <= sink.n_bits;  at++)
    {
        if (memcmp(sink.bits + at, source.bits, PAYLOAD_BITS) == 0)
            break;
        if (sink.bits[at] != 1)
            return 7;
    }
    if (at + PAYLOAD_BITS > sink.n_bits)
        return 8;
    /* and the same sender again after v29_tx_restart() */
    source.next = 0;
    source.calls = 0;
    if (v29_tx_restart(tx, 7200, true) != 0  ||  v29_tx(tx, amp, 160) != 160  ||  source.calls != 0)
        return 9;
    v29_tx_free(tx);
    v29_rx_free(rx);
    printf("modem_tx_objects: ok, payload at bit %d\n", at);
    return 0;
}
