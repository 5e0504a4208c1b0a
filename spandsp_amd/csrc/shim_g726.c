/*
 * shim_g726.c -- host side (plain C) of the spandsp-named entry points for G.726, declared in include/spangpu_spandsp.h:
 * g726_*.  An object is a one-channel codec bank of include/spangpu.h ("G.726 codec banks").  Without a GPU g726_init()
 * returns NULL: there is no CPU implementation.
 */
#include "shim_object.h"

#define PIECE       4096        /* samples (encode) or bytes (decode) per launch of one object */

OBJ_CODEC_LOOP(encode_pieces, spangpu_g726_t, spangpu_g726_encode_capacity, spangpu_g726_encode)
OBJ_CODEC_LOOP(decode_pieces, spangpu_g726_t, spangpu_g726_decode_capacity, spangpu_g726_decode)

g726_state_t *g726_init(g726_state_t *s, int bit_rate, int ext_coding, int packing)
{
    const int32_t rate = bit_rate;
    const int32_t coding = ext_coding;
    const int32_t pack = packing;
    spangpu_g726_t *bank;

    /* (the bank refuses the rates g726_init() refuses, g726.c:1179-1180) */
    if (spangpu_g726_create(&bank, 0, 1, &rate, &coding, &pack, 1) != SPANGPU_OK)
        return NULL;
    if ((s = OBJ_TAKE(s, g726_state_t)) == NULL)
    {
        spangpu_g726_destroy(bank);
        return NULL;
    }
    s->bank = bank;
    s->rate = bit_rate;
    s->ext_coding = ext_coding;
    s->bits_per_sample = bit_rate/8000;
    s->packing = packing;
    return s;
}

int g726_release(g726_state_t *s)
{
    if (s)
    {
        if (s->bank)
            spangpu_g726_destroy(s->bank);
        s->bank = NULL;
        obj_drop(&s->obj, NULL);
    }
    return 0;
}

int g726_free(g726_state_t *s)
{
    if (s)
    {
        g726_release(s);
        obj_drop(&s->obj, s);
    }
    return 0;
}

/* a sample is 2 bytes in the linear coding and 1 in the G.711 ones */
int g726_encode(g726_state_t *s, uint8_t g726_data[], const int16_t amp[], int len)
{
    if (s == NULL  ||  s->bank == NULL  ||  g726_data == NULL  ||  amp == NULL)
        return 0;
    return encode_pieces(&s->obj, s->bank, amp, (s->ext_coding == G726_ENCODING_LINEAR)  ?  2  :  1, g726_data, 1, len, PIECE);
}

int g726_decode(g726_state_t *s, int16_t amp[], const uint8_t g726_data[], int g726_bytes)
{
    if (s == NULL  ||  s->bank == NULL  ||  g726_data == NULL  ||  amp == NULL)
        return 0;
    return decode_pieces(&s->obj, s->bank, g726_data, 1, amp, (s->ext_coding == G726_ENCODING_LINEAR)  ?  2  :  1, g726_bytes, PIECE);
}
