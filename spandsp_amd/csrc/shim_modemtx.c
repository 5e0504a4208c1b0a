/*
 * shim_modemtx.c -- host side (plain C) of the spandsp-named entry points for the V.29, V.27ter and V.17 senders, declared
 * in include/spangpu_spandsp.h: v29_tx*, v27ter_tx*, v17_tx*.  A sender object is a one-channel bank of include/spangpu.h
 * ("modem transmitter banks") with the bit queue as its source: xxx_tx() asks the caller's get_bit for exactly the bits the
 * call needs, in order, queues them and launches.  Without a GPU the _init() functions return NULL: there is no CPU
 * implementation.
 */
#include "shim_object.h"

#define PIECE       4096        /* samples per launch of one object */
#define RING        8192        /* bits its ring takes: 14400 bps makes 1.8 bits a sample */

typedef spangpu_modemtx_object_t obj_t;

static obj_t *obj_init(obj_t *o, size_t size, int modem, const char *protocol, int bit_rate, int tep, span_get_bit_func_t get_bit,
                       void *user_data)
{
    spangpu_modemtx_cursor_t cursor;
    spangpu_modemtx_t *bank;

    /* as the reference: a bad bit rate returns NULL and leaves the caller's storage alone; so does a bank that cannot be made */
    if (spangpu_modemtx_cursor_init(&cursor, modem, bit_rate, tep, 0) != SPANGPU_OK
        ||  spangpu_modemtx_create_ex(&bank, 0, modem, 1, bit_rate, tep, SPANGPU_MODEMTX_QUEUE, NULL, RING) != SPANGPU_OK)
        return NULL;
    if ((o = (obj_t *) obj_take(o, size, offsetof(obj_t, obj))) == NULL)
    {
        spangpu_modemtx_destroy(bank);
        return NULL;
    }
    o->bank = bank;
    o->cursor = cursor;
    o->get_bit = get_bit;
    o->get_bit_user_data = user_data;
    /* what span_log_init(.., SPAN_LOG_NONE, NULL) + span_log_set_protocol() leave behind (v29tx.c:423-424 and twins) */
    o->logging.samples_per_second = 8000;
    o->logging.protocol = protocol;
    return o;
}

static int obj_restart(obj_t *o, int bit_rate, int tep, int short_train)
{
    spangpu_modemtx_cursor_t cursor;

    if (o == NULL  ||  o->bank == NULL  ||  spangpu_modemtx_cursor_init(&cursor, o->cursor.modem, bit_rate, tep, short_train) != SPANGPU_OK
        ||  spangpu_modemtx_restart_ex(o->bank, 0, bit_rate, tep, short_train) != SPANGPU_OK)
        return -1;
    o->cursor = cursor;
    return 0;
}

static int obj_release(obj_t *o)
{
    if (o)
    {
        if (o->bank)
            spangpu_modemtx_destroy(o->bank);
        o->bank = NULL;
        obj_drop(&o->obj, NULL);
    }
    return 0;
}

static int obj_free(obj_t *o)
{
    if (o)
    {
        obj_release(o);
        obj_drop(&o->obj, o);
    }
    return 0;
}

static int obj_tx(obj_t *o, int16_t amp[], int len)
{
    uint8_t bits[RING/8];
    int done = 0;

    if (o == NULL  ||  o->bank == NULL  ||  len <= 0)
        return 0;
    while (done < len)
    {
        const int piece = (len - done > PIECE)  ?  PIECE  :  (len - done);
        spangpu_modemtx_cursor_t ahead = o->cursor;
        const long long due = spangpu_modemtx_cursor_advance(&ahead, piece, -1);
        const int32_t *channels;
        const int32_t *kinds;
        int32_t n_bits;
        int32_t got = 0;
        int16_t *row;
        int ended;
        int events;
        int i;

        /* exactly the calls xxx_tx() makes, in order, up to SIG_STATUS_END_OF_DATA (v29tx.c:108-118) */
        if (due < 0  ||  due > RING)
            return done;
        n_bits = obj_pull_bits(o->get_bit, o->get_bit_user_data, due, bits, sizeof(bits), &ended);
        if (ended  &&  o->status_handler)
            o->status_handler(o->status_user_data, SIG_STATUS_END_OF_DATA);
        if ((row = (int16_t *) obj_room(&o->obj, (size_t) piece*sizeof(int16_t))) == NULL)
            return done;
        if ((n_bits > 0  &&  spangpu_modemtx_put_bits(o->bank, 0, 1, bits, RING/8, &n_bits, NULL) != SPANGPU_OK)
            ||  (ended  &&  spangpu_modemtx_end_of_data(o->bank, 0, 1) != SPANGPU_OK)
            ||  ((done == 0)  ?  spangpu_modemtx_tx_lens(o->bank, SPANGPU_MEM_HOST, row, piece, piece, &got)
                              :  spangpu_modemtx_tx_continue(o->bank, SPANGPU_MEM_HOST, row, piece, piece, &got)) < 0)
            return done;
        if (done > 0  ||  got > 0)
            spangpu_modemtx_cursor_advance(&o->cursor, piece, ended  ?  n_bits  :  -1);
        memcpy(amp + done, row, (size_t) got*sizeof(int16_t));
        done += got;
        events = spangpu_modemtx_events(o->bank, &channels, &kinds);
        for (i = 0;  i < events;  i++)
        {
            if (kinds[i] == SPANGPU_MODEMTX_SHUTDOWN_COMPLETE  &&  o->status_handler)
                o->status_handler(o->status_user_data, SIG_STATUS_SHUTDOWN_COMPLETE);
        }
        if (got < piece)
            break;      /* the shutdown was over when the call began (v29tx.c:241-245) */
    }
    return done;
}

/* xxx_tx_set_get_bit(), v29tx.c:340-347: the new function is current at once unless fake_get_bit() is -- which it is exactly
   while in_training is set, when obj_tx() asks nobody; so the caller's function is simply the one asked from now on. */
#define SENDER(pfx, T, MODEM, PROTOCOL)                                                                                 \
T *pfx##_init(T *s, int bit_rate, bool tep, span_get_bit_func_t get_bit, void *user_data)                               \
{                                                                                                                       \
    return (T *) obj_init(s  ?  &s->o  :  NULL, sizeof(T), MODEM, PROTOCOL, bit_rate, tep, get_bit, user_data);         \
}                                                                                                                       \
int pfx##_release(T *s)                                                                                                 \
{                                                                                                                       \
    return obj_release(s  ?  &s->o  :  NULL);                                                                           \
}                                                                                                                       \
int pfx##_free(T *s)                                                                                                    \
{                                                                                                                       \
    return obj_free(s  ?  &s->o  :  NULL);                                                                              \
}                                                                                                                       \
void pfx##_power(T *s, float power)                                                                                     \
{                                                                                                                       \
    spangpu_modemtx_power(s->o.bank, 0, power);                                                                         \
}                                                                                                                       \
void pfx##_set_get_bit(T *s, span_get_bit_func_t get_bit, void *user_data)                                              \
{                                                                                                                       \
    s->o.get_bit = get_bit;                                                                                             \
    s->o.get_bit_user_data = user_data;                                                                                 \
}                                                                                                                       \
void pfx##_set_modem_status_handler(T *s, span_modem_status_func_t handler, void *user_data)                            \
{                                                                                                                       \
    s->o.status_handler = handler;                                                                                      \
    s->o.status_user_data = user_data;                                                                                  \
}                                                                                                                       \
logging_state_t *pfx##_get_logging_state(T *s)                                                                          \
{                                                                                                                       \
    return &s->o.logging;                                                                                               \
}                                                                                                                       \
int pfx(T *s, int16_t amp[], int len)                                                                                   \
{                                                                                                                       \
    return obj_tx(s  ?  &s->o  :  NULL, amp, len);                                                                      \
}

SENDER(v29_tx, v29_tx_state_t, SPANGPU_V29, "V.29 TX")
SENDER(v27ter_tx, v27ter_tx_state_t, SPANGPU_V27TER, "V.27ter TX")
SENDER(v17_tx, v17_tx_state_t, SPANGPU_V17, "V.17 TX")

int v29_tx_restart(v29_tx_state_t *s, int bit_rate, bool tep)
{
    return obj_restart(s  ?  &s->o  :  NULL, bit_rate, tep, 0);
}

int v27ter_tx_restart(v27ter_tx_state_t *s, int bit_rate, bool tep)
{
    return obj_restart(s  ?  &s->o  :  NULL, bit_rate, tep, 0);
}

int v17_tx_restart(v17_tx_state_t *s, int bit_rate, bool tep, bool short_train)
{
    return obj_restart(s  ?  &s->o  :  NULL, bit_rate, tep, short_train);
}
