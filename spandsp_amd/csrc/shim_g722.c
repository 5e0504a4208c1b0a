/*
 * shim_g722.c -- host side (plain C) of the spandsp-named entry points for G.722, declared in include/spangpu_spandsp.h:
 * g722_encode_* and g722_decode_*.  An object is a one-channel codec bank of include/spangpu.h ("G.722 codec banks").
 * Without a GPU the init calls return NULL: there is no CPU implementation.
 */
#include <stdlib.h>
#include <string.h>

#include "spangpu_spandsp.h"

#define PIECE       4096        /* samples (encode) or bytes (decode) per launch of one object */

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

static int room(uint8_t **row, size_t *cap, size_t bytes)
{
    if (*cap < bytes)
    {
        uint8_t *r = (uint8_t *) realloc(*row, bytes);

        if (r == NULL)
            return 0;
        *row = r;
        *cap = bytes;
    }
    return 1;
}

g722_encode_state_t *g722_encode_init(g722_encode_state_t *s, int rate, int options)
{
    const int mine = (s != NULL);
    int bits;
    spangpu_g722_t *bank = bank_of(SPANGPU_G722_ENCODER, rate, options, &bits);

    if (bank == NULL)
        return NULL;
    if (mine)
    {
        memset(s, 0, sizeof(*s));
    }
    else if ((s = (g722_encode_state_t *) calloc(1, sizeof(*s))) == NULL)
    {
        spangpu_g722_destroy(bank);
        return NULL;
    }
    s->caller_storage = mine;
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
        free(s->row);
        s->row = NULL;
        s->row_cap = 0;
    }
    return 0;
}

int g722_encode_free(g722_encode_state_t *s)
{
    if (s)
    {
        g722_encode_release(s);
        if (!s->caller_storage)
            free(s);
    }
    return 0;
}

int g722_encode(g722_encode_state_t *s, uint8_t g722_data[], const int16_t amp[], int len)
{
    int done = 0;
    int bytes = 0;

    if (s == NULL  ||  s->bank == NULL  ||  g722_data == NULL  ||  amp == NULL)
        return 0;
    /* a 16 kHz encoder takes pairs: the odd sample at the end is left out (the reference reads amp[len] there) */
    if (!s->eight_k)
        len &= ~1;
    while (done < len)
    {
        const int piece = (len - done > PIECE)  ?  PIECE  :  (len - done);
        const long long cap = spangpu_g722_encode_capacity(s->bank, piece);
        int32_t got = 0;

        /* the bank writes a row of its capacity; the caller's buffer holds what the reference would write */
        if (cap <= 0  ||  !room(&s->row, &s->row_cap, (size_t) cap))
            break;
        if (spangpu_g722_encode(s->bank, amp + done, SPANGPU_MEM_HOST, (long long) piece*2, NULL, piece, s->row, SPANGPU_MEM_HOST,
                                cap, &got) != SPANGPU_OK)
            break;
        memcpy(g722_data + bytes, s->row, (size_t) got);
        bytes += got;
        done += piece;
    }
    return bytes;
}

g722_decode_state_t *g722_decode_init(g722_decode_state_t *s, int rate, int options)
{
    const int mine = (s != NULL);
    int bits;
    spangpu_g722_t *bank = bank_of(SPANGPU_G722_DECODER, rate, options, &bits);

    if (bank == NULL)
        return NULL;
    if (mine)
    {
        memset(s, 0, sizeof(*s));
    }
    else if ((s = (g722_decode_state_t *) calloc(1, sizeof(*s))) == NULL)
    {
        spangpu_g722_destroy(bank);
        return NULL;
    }
    s->caller_storage = mine;
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
        free(s->row);
        s->row = NULL;
        s->row_cap = 0;
    }
    return 0;
}

int g722_decode_free(g722_decode_state_t *s)
{
    if (s)
    {
        g722_decode_release(s);
        if (!s->caller_storage)
            free(s);
    }
    return 0;
}

int g722_decode(g722_decode_state_t *s, int16_t amp[], const uint8_t g722_data[], int len)
{
    int done = 0;
    int samples = 0;

    if (s == NULL  ||  s->bank == NULL  ||  g722_data == NULL  ||  amp == NULL)
        return 0;
    while (done < len)
    {
        const int piece = (len - done > PIECE)  ?  PIECE  :  (len - done);
        const long long cap = spangpu_g722_decode_capacity(s->bank, piece);
        int32_t got = 0;

        if (cap <= 0  ||  !room(&s->row, &s->row_cap, (size_t) cap*2))
            break;
        if (spangpu_g722_decode(s->bank, g722_data + done, SPANGPU_MEM_HOST, piece, NULL, piece, s->row, SPANGPU_MEM_HOST,
                                (long long) (cap*2), &got) != SPANGPU_OK)
            break;
        memcpy(amp + samples, s->row, (size_t) got*2);
        samples += got;
        done += piece;
    }
    return samples;
}
