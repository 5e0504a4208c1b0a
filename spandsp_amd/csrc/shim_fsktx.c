/*
 * shim_fsktx.c -- host side (plain C) of the spandsp-named entry points for the FSK sender, the modem connect tone
 * generator and the async character framer, declared in include/spangpu_spandsp.h: fsk_tx*, modem_connect_tones_tx*,
 * async_tx*.  A sender object is a one-channel bank of include/spangpu.h ("FSK and connect tone transmitter banks"):
 * fsk_tx() asks the caller's get_bit for exactly the bits the call needs, in order, queues them and launches.
 * async_tx* is host code as it is in the reference (src/async.c:277-393).
 * Without a GPU fsk_tx_init() and modem_connect_tones_tx_init() return NULL: there is no CPU implementation.
 */
#include "shim_object.h"

#define PIECE       8192        /* samples per launch of one object: at most as many bits, which is what its ring takes */

/* ---- fsk_tx ---------------------------------------------------------------------------------------------- */
static void spec_of(spangpu_fsk_spec_t *sp, const fsk_spec_t *spec)
{
    sp->freq_zero = spec->freq_zero;
    sp->freq_one = spec->freq_one;
    sp->tx_level = spec->tx_level;
    sp->min_level = spec->min_level;
    sp->baud_rate = spec->baud_rate;
}

fsk_tx_state_t *fsk_tx_init(fsk_tx_state_t *s, const fsk_spec_t *spec, span_get_bit_func_t get_bit, void *user_data)
{
    spangpu_fsk_spec_t sp;
    spangpu_fsktx_t *bank;

    if (spec == NULL)
        return NULL;
    spec_of(&sp, spec);
    if (spangpu_fsktx_create(&bank, 0, 1, &sp, SPANGPU_FSKTX_QUEUE, NULL, PIECE) != SPANGPU_OK)
        return NULL;
    if ((s = OBJ_TAKE(s, fsk_tx_state_t)) == NULL)
    {
        spangpu_fsktx_destroy(bank);
        return NULL;
    }
    s->bank = bank;
    s->get_bit = get_bit;
    s->get_bit_user_data = user_data;
    s->baud_rate = spec->baud_rate;
    return s;
}

int fsk_tx_restart(fsk_tx_state_t *s, const fsk_spec_t *spec)
{
    spangpu_fsk_spec_t sp;

    if (s == NULL  ||  s->bank == NULL  ||  spec == NULL)
        return -1;
    spec_of(&sp, spec);
    if (spangpu_fsktx_restart(s->bank, 0, &sp) != SPANGPU_OK  ||  spangpu_fsktx_end_of_data(s->bank, 0, 0) != SPANGPU_OK)
        return -1;
    s->baud_rate = spec->baud_rate;
    s->baud_frac = 0;
    s->shutdown = 0;
    return 0;
}

int fsk_tx_release(fsk_tx_state_t *s)
{
    if (s)
    {
        if (s->bank)
            spangpu_fsktx_destroy(s->bank);
        s->bank = NULL;
        obj_drop(&s->obj, NULL);
    }
    return 0;
}

int fsk_tx_free(fsk_tx_state_t *s)
{
    if (s)
    {
        fsk_tx_release(s);
        obj_drop(&s->obj, s);
    }
    return 0;
}

void fsk_tx_power(fsk_tx_state_t *s, float power)
{
    spangpu_fsktx_power(s->bank, 0, power);
}

void fsk_tx_set_get_bit(fsk_tx_state_t *s, span_get_bit_func_t get_bit, void *user_data)
{
    s->get_bit = get_bit;
    s->get_bit_user_data = user_data;
}

void fsk_tx_set_modem_status_handler(fsk_tx_state_t *s, span_modem_status_func_t handler, void *user_data)
{
    s->status_handler = handler;
    s->status_user_data = user_data;
}

int fsk_tx(fsk_tx_state_t *s, int16_t amp[], int len)
{
    uint8_t bits[PIECE/8];
    int done = 0;

    if (s == NULL  ||  s->bank == NULL  ||  s->shutdown  ||  len <= 0)
        return 0;
    while (done < len)
    {
        const int piece = (len - done > PIECE)  ?  PIECE  :  (len - done);
        const int due = (int) spangpu_fsktx_bits_due(s->baud_rate, s->baud_frac, piece);
        int32_t n_bits;
        int32_t got = 0;
        int ended;
        int16_t *row;

        /* exactly the calls fsk_tx() makes, in order, up to SIG_STATUS_END_OF_DATA (fsk.c:176-189) */
        n_bits = obj_pull_bits(s->get_bit, s->get_bit_user_data, due, bits, sizeof(bits), &ended);
        if ((row = (int16_t *) obj_room(&s->obj, (size_t) piece*sizeof(int16_t))) == NULL)
            return done;
        if ((n_bits > 0  &&  spangpu_fsktx_put_bits(s->bank, 0, 1, bits, PIECE/8, &n_bits, NULL) != SPANGPU_OK)
            ||  (ended  &&  spangpu_fsktx_end_of_data(s->bank, 0, 1) != SPANGPU_OK)
            ||  spangpu_fsktx_tx(s->bank, SPANGPU_MEM_HOST, row, piece, piece, &got) != SPANGPU_OK)
            return done;
        /* the samples past the returned count stay as the caller had them */
        memcpy(amp + done, row, (size_t) got*sizeof(int16_t));
        done += got;
        if (ended)
        {
            if (s->status_handler)
                s->status_handler(s->status_user_data, SIG_STATUS_END_OF_DATA);
            if (s->status_handler)
                s->status_handler(s->status_user_data, SIG_STATUS_SHUTDOWN_COMPLETE);
            s->shutdown = 1;
            break;
        }
        s->baud_frac = (int) (((long long) s->baud_frac + (long long) piece*s->baud_rate)%(8000*100));
    }
    return done;
}

/* ---- modem_connect_tones_tx -------------------------------------------------------------------------------- */
modem_connect_tones_tx_state_t *modem_connect_tones_tx_init(modem_connect_tones_tx_state_t *s, int tone_type)
{
    spangpu_mcttx_t *bank;

    if (spangpu_mcttx_create(&bank, 0, tone_type, 1) != SPANGPU_OK)
        return NULL;
    if ((s = OBJ_TAKE(s, modem_connect_tones_tx_state_t)) == NULL)
    {
        spangpu_mcttx_destroy(bank);
        return NULL;
    }
    s->bank = bank;
    s->tone_type = tone_type;
    return s;
}

int modem_connect_tones_tx_release(modem_connect_tones_tx_state_t *s)
{
    if (s)
    {
        if (s->bank)
            spangpu_mcttx_destroy(s->bank);
        s->bank = NULL;
        obj_drop(&s->obj, NULL);
    }
    return 0;
}

int modem_connect_tones_tx_free(modem_connect_tones_tx_state_t *s)
{
    if (s)
    {
        modem_connect_tones_tx_release(s);
        obj_drop(&s->obj, s);
    }
    return 0;
}

int modem_connect_tones_tx(modem_connect_tones_tx_state_t *s, int16_t amp[], int len)
{
    int32_t got = 0;
    int16_t *row;

    if (s == NULL  ||  s->bank == NULL  ||  len <= 0)
        return 0;
    if ((row = (int16_t *) obj_room(&s->obj, (size_t) len*sizeof(int16_t))) == NULL
        ||  spangpu_mcttx_tx(s->bank, SPANGPU_MEM_HOST, row, len, len, &got) != SPANGPU_OK)
        return 0;
    memcpy(amp, row, (size_t) got*sizeof(int16_t));
    return got;
}

/* ---- async_tx, src/async.c:277-393 ---------------------------------------------------------------------------- */
int async_tx_get_bit(void *user_data)
{
    async_tx_state_t *s = (async_tx_state_t *) user_data;
    uint8_t one[16];
    uint8_t byte;
    int next_byte;
    int n;
    int i;

    if (s->bitpos == 0)
    {
        if (s->presend_bits > 0)
        {
            s->presend_bits--;
            return 1;
        }
        if ((next_byte = s->get_byte(s->user_data)) < 0)
            return (next_byte != SIG_STATUS_LINK_IDLE)  ?  next_byte  :  1;
        byte = (uint8_t) next_byte;
        if ((n = spangpu_async_frame_bits(s->data_bits, s->parity, s->stop_bits, &byte, 1, one, 16)) <= 0)
            return 1;
        s->frame_in_progress = 0;
        for (i = 1;  i < n;  i++)
            s->frame_in_progress |= (uint16_t) (one[i] << (i - 1));
        s->total_bits = n - 1;
        s->bitpos = 1;
        return 0;
    }
    i = s->frame_in_progress & 1;
    s->frame_in_progress >>= 1;
    if (++s->bitpos > s->total_bits)
        s->bitpos = 0;
    return i;
}

void async_tx_presend_bits(async_tx_state_t *s, int bits)
{
    s->presend_bits = bits;
}

async_tx_state_t *async_tx_init(async_tx_state_t *s, int data_bits, int parity, int stop_bits, bool use_v14,
                                span_get_byte_func_t get_byte, void *user_data)
{
    (void) use_v14;
    if ((s = OBJ_TAKE(s, async_tx_state_t)) == NULL)
        return NULL;
    s->data_bits = data_bits;
    s->parity = parity;
    s->stop_bits = stop_bits;
    s->get_byte = get_byte;
    s->user_data = user_data;
    return s;
}

int async_tx_release(async_tx_state_t *s)
{
    (void) s;
    return 0;
}

int async_tx_free(async_tx_state_t *s)
{
    if (s)
        obj_drop(&s->obj, s);
    return 0;
}
