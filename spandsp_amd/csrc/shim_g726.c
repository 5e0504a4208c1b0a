/*
 * shim_g726.c -- host side (plain C) of the spandsp-named entry points for G.726, declared in include/spangpu_spandsp.h:
 * g726_*.  An object is a one-channel codec bank of include/spangpu.h ("G.726 codec banks").  Without a GPU g726_init()
 * returns NULL: there is no CPU implementation.
 */
#include <stdlib.h>
#include <string.h>

#include "spangpu_spandsp.h"

#define PIECE       4096        /* samples (encode) or bytes (decode) per launch of one object */

g726_state_t *g726_init(g726_state_t *s, int bit_rate, int ext_coding, int packing)
{
    const int mine = (s != NULL);
    const int32_t rate = bit_rate;
    const int32_t coding = ext_coding;
    const int32_t pack = packing;
    spangpu_g726_t *bank;

    /* (the bank refuses the rates g726_init() refuses, g726.c:1179-1180) */
    if (spangpu_g726_create(&bank, 0, 1, &rate, &coding, &pack, 1) != SPANGPU_OK)
        return NULL;
    if (mine)
    {
        memset(s, 0, sizeof(*s));
    }
    else if ((s = (g726_state_t *) calloc(1, sizeof(*s))) == NULL)
    {
        spangpu_g726_destroy(bank);
        return NULL;
    }
    s->caller_storage = mine;
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
        free(s->row);
        s->row = NULL;
        s->row_cap = 0;
    }
    return 0;
}

int g726_free(g726_state_t *s)
{
    if (s)
    {
        g726_release(s);
        if (!s->caller_storage)
            free(s);
    }
    return 0;
}

static int room(g726_state_t *s, size_t bytes)
{
    if (s->row_cap < bytes)
    {
        uint8_t *r = (uint8_t *) realloc(s->row, bytes);

        if (r == NULL)
            return 0;
        s->row = r;
        s->row_cap = bytes;
    }
    return 1;
}

int g726_encode(g726_state_t *s, uint8_t g726_data[], const int16_t amp[], int len)
{
    const size_t el = (s  &&  s->ext_coding == G726_ENCODING_LINEAR)  ?  2  :  1;
    const uint8_t *in = (const uint8_t *) amp;
    int done = 0;
    int bytes = 0;

    if (s == NULL  ||  s->bank == NULL  ||  g726_data == NULL  ||  amp == NULL)
        return 0;
    while (done < len)
    {
        const int piece = (len - done > PIECE)  ?  PIECE  :  (len - done);
        const long long cap = spangpu_g726_encode_capacity(s->bank, piece);
        int32_t got = 0;

        /* the bank writes a row of its capacity; the caller's buffer holds what the reference would write */
        if (cap <= 0  ||  !room(s, (size_t) cap))
            break;
        if (spangpu_g726_encode(s->bank, in + (size_t) done*el, SPANGPU_MEM_HOST, (long long) (piece*el), NULL, piece, s->row, SPANGPU_MEM_HOST,
                                cap, &got) != SPANGPU_OK)
            break;
        memcpy(g726_data + bytes, s->row, (size_t) got);
        bytes += got;
        done += piece;
    }
    return bytes;
}

int g726_decode(g726_state_t *s, int16_t amp[], const uint8_t g726_data[], int g726_bytes)
{
    const size_t el = (s  &&  s->ext_coding == G726_ENCODING_LINEAR)  ?  2  :  1;
    uint8_t *out = (uint8_t *) amp;
    int done = 0;
    int samples = 0;

    if (s == NULL  ||  s->bank == NULL  ||  g726_data == NULL  ||  amp == NULL)
        return 0;
    while (done < g726_bytes)
    {
        const int piece = (g726_bytes - done > PIECE)  ?  PIECE  :  (g726_bytes - done);
        const long long cap = spangpu_g726_decode_capacity(s->bank, piece);
        int32_t got = 0;

        if (cap <= 0  ||  !room(s, (size_t) cap*el))
            break;
        if (spangpu_g726_decode(s->bank, g726_data + done, SPANGPU_MEM_HOST, piece, NULL, piece, s->row, SPANGPU_MEM_HOST,
                                (long long) (cap*el), &got) != SPANGPU_OK)
            break;
        memcpy(out + (size_t) samples*el, s->row, (size_t) got*el);
        samples += got;
        done += piece;
    }
    return samples;
}
