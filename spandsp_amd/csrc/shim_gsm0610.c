/*
 * shim_gsm0610.c -- host side (plain C) of the spandsp-named entry points for GSM 06.10, declared in
 * include/spangpu_spandsp.h: gsm0610_init, _release, _free, _set_packing, _encode and _decode (the packers and unpackers are in
 * gsm0610_host.c).  An object is a pair of one-channel codec banks of include/spangpu.h ("GSM 06.10 codec banks"), as the
 * reference's one state type serves both directions.  Without a GPU gsm0610_init() returns NULL: there is no CPU
 * implementation.
 */
#include <stdlib.h>
#include <string.h>

#include "spangpu_spandsp.h"

#define PIECE_FRAMES    32          /* units (a frame, or a WAV49 pair) per launch of one object */

/* a packing the reference's switch statements do not name is GSM0610_PACKING_NONE to them */
static int known(int packing)
{
    return (packing == GSM0610_PACKING_WAV49  ||  packing == GSM0610_PACKING_VOIP)  ?  packing  :  GSM0610_PACKING_NONE;
}

static int unit_samples(int packing)
{
    return (packing == GSM0610_PACKING_WAV49)  ?  320  :  160;
}

static int unit_bytes(int packing)
{
    return (packing == GSM0610_PACKING_WAV49)  ?  65  :  ((packing == GSM0610_PACKING_VOIP)  ?  33  :  76);
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

gsm0610_state_t *gsm0610_init(gsm0610_state_t *s, int packing)
{
    const int mine = (s != NULL);
    const int32_t p = known(packing);
    spangpu_gsm0610_t *enc;
    spangpu_gsm0610_t *dec;

    if (spangpu_gsm0610_create(&enc, 0, 1, SPANGPU_GSM0610_ENCODER, &p, 1) != SPANGPU_OK)
        return NULL;
    if (spangpu_gsm0610_create(&dec, 0, 1, SPANGPU_GSM0610_DECODER, &p, 1) != SPANGPU_OK)
    {
        spangpu_gsm0610_destroy(enc);
        return NULL;
    }
    if (mine)
    {
        memset(s, 0, sizeof(*s));
    }
    else if ((s = (gsm0610_state_t *) calloc(1, sizeof(*s))) == NULL)
    {
        spangpu_gsm0610_destroy(enc);
        spangpu_gsm0610_destroy(dec);
        return NULL;
    }
    s->caller_storage = mine;
    s->encoder = enc;
    s->decoder = dec;
    s->packing = p;
    return s;
}

int gsm0610_release(gsm0610_state_t *s)
{
    if (s)
    {
        if (s->encoder)
            spangpu_gsm0610_destroy(s->encoder);
        if (s->decoder)
            spangpu_gsm0610_destroy(s->decoder);
        s->encoder = NULL;
        s->decoder = NULL;
        free(s->row);
        s->row = NULL;
        s->row_cap = 0;
    }
    return 0;
}

int gsm0610_free(gsm0610_state_t *s)
{
    if (s)
    {
        gsm0610_release(s);
        if (!s->caller_storage)
            free(s);
    }
    return 0;
}

int gsm0610_set_packing(gsm0610_state_t *s, int packing)
{
    const int p = known(packing);

    if (s == NULL  ||  s->encoder == NULL  ||  s->decoder == NULL)
        return -1;
    if (spangpu_gsm0610_set_packing(s->encoder, 0, p) != SPANGPU_OK  ||  spangpu_gsm0610_set_packing(s->decoder, 0, p) != SPANGPU_OK)
        return -1;
    s->packing = p;
    return 0;
}

int gsm0610_encode(gsm0610_state_t *s, uint8_t code[], const int16_t amp[], int len)
{
    int done = 0;
    int bytes = 0;

    if (s == NULL  ||  s->encoder == NULL  ||  code == NULL  ||  amp == NULL)
        return 0;
    /* whole frames: the reference reads past amp[len] at a partial one */
    len -= len%unit_samples(s->packing);
    while (done < len)
    {
        const int most = PIECE_FRAMES*unit_samples(s->packing);
        const int piece = (len - done > most)  ?  most  :  (len - done);
        const long long cap = spangpu_gsm0610_encode_capacity(s->encoder, piece);
        int32_t got = 0;

        if (cap <= 0  ||  !room(&s->row, &s->row_cap, (size_t) cap))
            break;
        if (spangpu_gsm0610_encode(s->encoder, amp + done, SPANGPU_MEM_HOST, (long long) piece*2, NULL, piece, s->row, SPANGPU_MEM_HOST,
                                   cap, &got) != SPANGPU_OK)
            break;
        memcpy(code + bytes, s->row, (size_t) got);
        bytes += got;
        done += piece;
    }
    return bytes;
}

int gsm0610_decode(gsm0610_state_t *s, int16_t amp[], const uint8_t code[], int len)
{
    int done = 0;
    int samples = 0;

    if (s == NULL  ||  s->decoder == NULL  ||  code == NULL  ||  amp == NULL)
        return 0;
    len -= len%unit_bytes(s->packing);
    while (done < len)
    {
        const int most = PIECE_FRAMES*unit_bytes(s->packing);
        const int piece = (len - done > most)  ?  most  :  (len - done);
        const long long cap = spangpu_gsm0610_decode_capacity(s->decoder, piece);
        int32_t got = 0;

        if (cap <= 0  ||  !room(&s->row, &s->row_cap, (size_t) cap*2))
            break;
        if (spangpu_gsm0610_decode(s->decoder, code + done, SPANGPU_MEM_HOST, piece, NULL, piece, s->row, SPANGPU_MEM_HOST,
                                   (long long) (cap*2), &got) != SPANGPU_OK)
            break;
        memcpy(amp + samples, s->row, (size_t) got*2);
        samples += got;
        done += piece;
    }
    return samples;
}
