/*
 * shim_g722.c -- host side (plain C) of the spandsp-named entry points for G.722, declared in include/spangpu_spandsp.h:
 * g722_encode_* and g722_decode_*.  An object is a one-channel codec bank of include/spangpu.h ("G.722 codec banks").
 * Without a GPU the init calls return NULL: there is no CPU implementation.
 */
#include "shim_object.h"

#define PIECE       4096        /* samples (encode) or bytes (decode) per launch of one object */

OBJ_CODEC_LOOP(encode_pieces, spangpu_g722_t, spangpu_g722_encode_capacity, spangpu_g722_encode)
OBJ_CODEC_LOOP(decode_pieces, spangpu_g722_t, spangpu_g722_decode_capacity, spangpu_g722_decode)

/* every rate but 48000 and 56000 is 64000, g722.c:423-428 and 631-636; the option bits the reference does not look at are dropped */
static spangpu_g722_t *bank_of(int direction, int rate, int options, int *bits)
{
    const int32_t r = (rate == 48000  ||  rate == 56000)  ?  rate  :  64000;
    const int32_t o = options & (G722_SAMPLE_RATE_8000 | G722_PACKED);
    spangpu_g722_t *bank;

    *bits = r/8000;
    if (spangpu_g722_create(&bank, 0, 1, direction, &r, &o, 1) != SPANGPU_OK)
        return NULL;
    return bank;
}

g722_encode_state_t *g722_encode_init(g722_encode_state_t *s, int rate, int options)
{
    int bits;
    spangpu_g722_t *bank = bank_of(SPANGPU_G722_ENCODER, rate, options, &bits);

    if (bank == NULL)
        return NULL;
    if ((s = OBJ_TAKE(s, g722_encode_state_t)) == NULL)
    {
        spangpu_g722_destroy(bank);
        return NULL;
    }
    s->bank = bank;
    s->bits_per_sample = bits;
    s->eight_k = (options & G722_SAMPLE_RATE_8000) != 0;
    s->packed = (options & G722_PACKED) != 0  &&  bits != 8;
    return s;
}

int g722_encode_release(g722_encode_state_t *s)
{
    if (s)
    {
        if (s->bank)
            spangpu_g722_destroy(s->bank);
        s->bank = NULL;
        obj_drop(&s->obj, NULL);
    }
    return 0;
}

int g722_encode_free(g722_encode_state_t *s)
{
    if (s)
    {
        g722_encode_release(s);
        obj_drop(&s->obj, s);
    }
    return 0;
}

int g722_encode(g722_encode_state_t *s, uint8_t g722_data[], const int16_t amp[], int len)
{
    if (s == NULL  ||  s->bank == NULL  ||  g722_data == NULL  ||  amp == NULL)
        return 0;
    /* a 16 kHz encoder takes pairs: the odd sample at the end is left out (the reference reads amp[len] there) */
    if (!s->eight_k)
        len &= ~1;
    return encode_pieces(&s->obj, s->bank, amp, 2, g722_data, 1, len, PIECE);
}

g722_decode_state_t *g722_decode_init(g722_decode_state_t *s, int rate, int options)
{
    int bits;
    spangpu_g722_t *bank = bank_of(SPANGPU_G722_DECODER, rate, options, &bits);

    if (bank == NULL)
        return NULL;
    if ((s = OBJ_TAKE(s, g722_decode_state_t)) == NULL)
    {
        spangpu_g722_destroy(bank);
        return NULL;
    }
    s->bank = bank;
    s->bits_per_sample = bits;
    s->eight_k = (options & G722_SAMPLE_RATE_8000) != 0;
    s->packed = (options & G722_PACKED) != 0  &&  bits != 8;
    return s;
}

int g722_decode_release(g722_decode_state_t *s)
{
    if (s)
    {
        if (s->bank)
            spangpu_g722_destroy(s->bank);
        s->bank = NULL;
        obj_drop(&s->obj, NULL);
    }
    return 0;
}

int g722_decode_free(g722_decode_state_t *s)
{
    if (s)
    {
        g722_decode_release(s);
        obj_drop(&s->obj, s);
    }
    return 0;
}

int g722_decode(g722_decode_state_t *s, int16_t amp[], const uint8_t g722_data[], int len)
{
    if (s == NULL  ||  s->bank == NULL  ||  g722_data == NULL  ||  amp == NULL)
        return 0;
    return decode_pieces(&s->obj, s->bank, g722_data, 1, amp, 2, len, PIECE);
}
