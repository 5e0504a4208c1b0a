/*
 * shim_adsi.c -- host side (plain C) of the spandsp-named entry points for caller ID in the four FSK standards, declared in
 * include/spangpu_spandsp.h: adsi_*.  An object is a one-channel caller-ID bank of include/spangpu.h ("Caller-ID banks").
 * Without a GPU the two inits return NULL: there is no CPU implementation.  The field helpers are host code (adsi_host.c).
 */
#include "shim_object.h"

#define PIECE       4096        /* samples per launch of one object */

OBJ_SENDER_LOOP(tx_pieces, spangpu_adsi_tx_t, spangpu_adsi_tx)

static int fsk_standard(int standard)
{
    return standard >= ADSI_STANDARD_CLASS  &&  standard <= ADSI_STANDARD_JCLIP;
}

adsi_tx_state_t *adsi_tx_init(adsi_tx_state_t *s, int standard)
{
    int32_t std = standard;
    spangpu_adsi_tx_t *bank;

    if (!fsk_standard(standard)  ||  spangpu_adsi_tx_create(&bank, 0, 1, &std, 1) != SPANGPU_OK)
        return NULL;
    if ((s = OBJ_TAKE(s, adsi_tx_state_t)) == NULL)
    {
        spangpu_adsi_tx_destroy(bank);
        return NULL;
    }
    s->bank = bank;
    s->standard = standard;
    /* what memset() leaves of a logging_state_t, with the rate span_log would be given */
    s->logging.samples_per_second = 8000;
    return s;
}

int adsi_tx_release(adsi_tx_state_t *s)
{
    if (s)
    {
        if (s->bank)
            spangpu_adsi_tx_destroy(s->bank);
        s->bank = NULL;
        obj_drop(&s->obj, NULL);
    }
    return 0;
}

int adsi_tx_free(adsi_tx_state_t *s)
{
    if (s)
    {
        adsi_tx_release(s);
        obj_drop(&s->obj, s);
    }
    return 0;
}

int adsi_tx(adsi_tx_state_t *s, int16_t amp[], int max_len)
{
    if (s == NULL  ||  s->bank == NULL  ||  max_len <= 0)
        return 0;
    return tx_pieces(&s->obj, s->bank, amp, max_len, PIECE);
}

int adsi_tx_put_message(adsi_tx_state_t *s, const uint8_t *msg, int len)
{
    int32_t n = len;
    int32_t res = -1;

    if (s == NULL  ||  s->bank == NULL  ||  msg == NULL  ||  len < 2)
        return -1;
    if (spangpu_adsi_tx_put_message(s->bank, 0, 1, msg, len, &n, &res) != SPANGPU_OK)
        return -1;
    return res;
}

void adsi_tx_set_preamble(adsi_tx_state_t *s, int preamble_len, int preamble_ones_len, int postamble_ones_len, int stop_bits)
{
    if (s  &&  s->bank)
        spangpu_adsi_tx_set_preamble(s->bank, 0, preamble_len, preamble_ones_len, postamble_ones_len, stop_bits);
}

void adsi_tx_send_alert_tone(adsi_tx_state_t *s)
{
    if (s  &&  s->bank)
        spangpu_adsi_tx_send_alert_tone(s->bank, 0);
}

logging_state_t *adsi_tx_get_logging_state(adsi_tx_state_t *s)
{
    return &s->logging;
}

adsi_rx_state_t *adsi_rx_init(adsi_rx_state_t *s, int standard, span_put_msg_func_t put_msg, void *user_data)
{
    int32_t std = standard;
    spangpu_adsi_rx_t *bank;

    if (!fsk_standard(standard)  ||  spangpu_adsi_rx_create(&bank, 0, 1, &std, 1) != SPANGPU_OK)
        return NULL;
    if ((s = OBJ_TAKE(s, adsi_rx_state_t)) == NULL)
    {
        spangpu_adsi_rx_destroy(bank);
        return NULL;
    }
    s->bank = bank;
    s->standard = standard;
    s->put_msg = put_msg;
    s->user_data = user_data;
    s->logging.samples_per_second = 8000;
    return s;
}

int adsi_rx_release(adsi_rx_state_t *s)
{
    if (s)
    {
        if (s->bank)
            spangpu_adsi_rx_destroy(s->bank);
        s->bank = NULL;
    }
    return 0;
}

int adsi_rx_free(adsi_rx_state_t *s)
{
    if (s)
    {
        adsi_rx_release(s);
        obj_drop(&s->obj, s);
    }
    return 0;
}

int adsi_rx(adsi_rx_state_t *s, const int16_t amp[], int len)
{
    int done = 0;

    if (s == NULL  ||  s->bank == NULL)
        return 0;
    while (done < len)
    {
        const int piece = (len - done > PIECE)  ?  PIECE  :  (len - done);
        const uint8_t *bytes;
        const int32_t *lens;
        const int32_t *counts;
        int i;

        if (spangpu_adsi_rx(s->bank, amp + done, SPANGPU_MEM_HOST, piece, piece) != SPANGPU_OK
            ||  spangpu_adsi_rx_messages(s->bank, &bytes, &lens, &counts) < 0)
            break;
        for (i = 0;  i < counts[0];  i++)
        {
            if (s->put_msg)
                s->put_msg(s->user_data, bytes + (size_t) i*SPANGPU_ADSI_MSG_BYTES, lens[i]);
        }
        done += piece;
    }
    return 0;
}

logging_state_t *adsi_rx_get_logging_state(adsi_rx_state_t *s)
{
    return &s->logging;
}

int adsi_next_field(adsi_rx_state_t *s, const uint8_t *msg, int msg_len, int pos, uint8_t *field_type, uint8_t const **field_body, int *field_len)
{
    return spangpu_adsi_next_field(s->standard, msg, msg_len, pos, field_type, field_body, field_len);
}

int adsi_add_field(adsi_tx_state_t *s, uint8_t *msg, int len, uint8_t field_type, uint8_t const *field_body, int field_len)
{
    return spangpu_adsi_add_field(s->standard, &s->baudot_shift, msg, len, field_type, field_body, field_len);
}

const char *adsi_standard_to_str(int standard)
{
    return spangpu_adsi_standard_to_str(standard);
}
