/*
 * shim_v18.c -- host side (plain C) of the spandsp-named entry points for V.18 text telephones in the three Weitbrecht 5-bit
 * modes, declared in include/spangpu_spandsp.h: v18_*.  An object is a one-channel V.18 text bank of include/spangpu.h
 * ("V.18 text banks").  Without a GPU v18_init() returns NULL: there is no CPU implementation.
 */
#include "shim_object.h"

#define PIECE       4096        /* samples per launch of one object */

OBJ_SENDER_LOOP(tx_pieces, spangpu_v18_t, spangpu_v18_tx)

v18_state_t *v18_init(v18_state_t *s, bool calling_party, int mode, int nation, span_put_msg_func_t put_msg, void *put_msg_user_data,
                      span_modem_status_func_t status_handler, void *status_handler_user_data)
{
    int32_t bank_mode;
    spangpu_v18_t *bank;

    /* v18.c:2078: the option bit never reaches v18_set_modem() */
    mode &= ~V18_MODE_REPETITIVE_SHIFTS_OPTION;
    if (nation != V18_AUTOMODING_NONE
        ||  (mode != V18_MODE_WEITBRECHT_5BIT_4545  &&  mode != V18_MODE_WEITBRECHT_5BIT_476  &&  mode != V18_MODE_WEITBRECHT_5BIT_50))
        return NULL;
    bank_mode = mode;
    if (spangpu_v18_create(&bank, 0, 1, &bank_mode, 1, calling_party) != SPANGPU_OK)
        return NULL;
    if ((s = OBJ_TAKE(s, v18_state_t)) == NULL)
    {
        spangpu_v18_destroy(bank);
        return NULL;
    }
    s->bank = bank;
    s->current_mode = mode;
    s->put_msg = put_msg;
    s->put_msg_user_data = put_msg_user_data;
    s->status_handler = status_handler;
    s->status_handler_user_data = status_handler_user_data;
    strcpy(s->stored_message, "V.18 pls");
    /* what memset() leaves of a logging_state_t, with the rate span_log would be given */
    s->logging.samples_per_second = 8000;
    return s;
}

int v18_release(v18_state_t *s)
{
    if (s)
    {
        if (s->bank)
            spangpu_v18_destroy(s->bank);
        s->bank = NULL;
        obj_drop(&s->obj, NULL);
    }
    return 0;
}

int v18_free(v18_state_t *s)
{
    if (s)
    {
        v18_release(s);
        obj_drop(&s->obj, s);
    }
    return 0;
}

int v18_tx(v18_state_t *s, int16_t amp[], int max_len)
{
    if (s == NULL  ||  s->bank == NULL  ||  max_len <= 0)
        return 0;
    return tx_pieces(&s->obj, s->bank, amp, max_len, PIECE);
}

int v18_rx(v18_state_t *s, const int16_t amp[], int len)
{
    int done = 0;

    if (s == NULL  ||  s->bank == NULL)
        return 0;
    while (done < len)
    {
        const int piece = (len - done > PIECE)  ?  PIECE  :  (len - done);
        const uint8_t *chars;
        const int32_t *counts;
        int i;

        if (spangpu_v18_rx(s->bank, amp + done, SPANGPU_MEM_HOST, piece, piece) != SPANGPU_OK
            ||  spangpu_v18_text(s->bank, &chars, &counts) < 0)
            break;
        for (i = 0;  i < counts[0];  i++)
        {
            uint8_t msg[2];

            msg[0] = chars[i];
            msg[1] = '\0';
            if (s->put_msg)
                s->put_msg(s->put_msg_user_data, msg, 1);
        }
        done += piece;
    }
    return 0;
}

int v18_rx_fillin(v18_state_t *s, int len)
{
    if (s  &&  s->bank  &&  len > 0)
        spangpu_v18_fillin(s->bank, 0, len);
    return 0;
}

int v18_put(v18_state_t *s, const char msg[], int len)
{
    int32_t n;
    int32_t res = -1;

    if (s == NULL  ||  s->bank == NULL  ||  msg == NULL)
        return -1;
    if (len < 0)
    {
        if ((len = (int) strlen(msg)) == 0)
            return 0;
    }
    n = len;
    if (spangpu_v18_put(s->bank, 0, 1, (const uint8_t *) msg, (len > 0)  ?  len  :  1, &n, &res) != SPANGPU_OK)
        return -1;
    return res;
}

int v18_set_stored_message(v18_state_t *s, const char *msg)
{
    strncpy(s->stored_message, msg, 80);
    s->stored_message[80] = '\0';
    return 0;
}

int v18_get_current_mode(v18_state_t *s)
{
    return s->current_mode;
}

logging_state_t *v18_get_logging_state(v18_state_t *s)
{
    return &s->logging;
}

const char *v18_mode_to_str(int mode)
{
    switch (mode & 0xFFF)
    {
    case V18_MODE_NONE:
        return "None";
    case V18_MODE_WEITBRECHT_5BIT_4545:
        return "Weitbrecht TDD (45.45bps)";
    case V18_MODE_WEITBRECHT_5BIT_476:
        return "Weitbrecht TDD (47.6bps)";
    case V18_MODE_WEITBRECHT_5BIT_50:
        return "Weitbrecht TDD (50bps)";
    case V18_MODE_DTMF:
        return "DTMF";
    case V18_MODE_EDT:
        return "EDT";
    case V18_MODE_BELL103:
        return "Bell 103";
    case V18_MODE_V23VIDEOTEX:
        return "V.23 Videotex";
    case V18_MODE_V21TEXTPHONE:
        return "V.21";
    case V18_MODE_V18TEXTPHONE:
        return "V.18 text telephone";
    }
    return "???";
}

const char *v18_status_to_str(int status)
{
    static const char *const names[] =
    {
        "Switched to None mode",
        "Switched to Weitbrecht TDD (45.45bps) mode",
        "Switched to Weitbrecht TDD (47.6bps) mode",
        "Switched to Weitbrecht TDD (50bps) mode",
        "Switched to DTMF mode",
        "Switched to EDT mode",
        "Switched to Bell 103 mode",
        "Switched to V.23 Videotex mode",
        "Switched to V.21 mode",
        "Switched to V.18 text telephone mode"
    };

    if (status < 0  ||  status > V18_STATUS_SWITCH_TO_V18TEXTPHONE)
        return "???";
    return names[status];
}
