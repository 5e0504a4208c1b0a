/*
 * shim_gsm0610.c -- host side (plain C) of the spandsp-named entry points for GSM 06.10, declared in
 * include/spangpu_spandsp.h: gsm0610_init, _release, _free, _set_packing, _encode and _decode (the packers and unpackers are in
 * gsm0610_host.c).  An object is a pair of one-channel codec banks of include/spangpu.h ("GSM 06.10 codec banks"), as the
 * reference's one state type serves both directions.  Without a GPU gsm0610_init() returns NULL: there is no CPU
 * implementation.
 */
#include "shim_object.h"

#define PIECE_FRAMES    32          /* units (a frame, or a WAV49 pair) per launch of one object */

OBJ_CODEC_LOOP(encode_pieces, spangpu_gsm0610_t, spangpu_gsm0610_encode_capacity, spangpu_gsm0610_encode)
OBJ_CODEC_LOOP(decode_pieces, spangpu_gsm0610_t, spangpu_gsm0610_decode_capacity, spangpu_gsm0610_decode)

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

gsm0610_state_t *gsm0610_init(gsm0610_state_t *s, int packing)
{
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
    if ((s = OBJ_TAKE(s, gsm0610_state_t)) == NULL)
    {
        spangpu_gsm0610_destroy(enc);
        spangpu_gsm0610_destroy(dec);
        return NULL;
    }
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
        obj_drop(&s->obj, NULL);
    }
    return 0;
}

int gsm0610_free(gsm0610_state_t *s)
{
    if (s)
    {
        gsm0610_release(s);
        obj_drop(&s->obj, s);
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
    if (s == NULL  ||  s->encoder == NULL  ||  code == NULL  ||  amp == NULL)
        return 0;
    /* whole frames: the reference reads past amp[len] at a partial one */
    len -= len%unit_samples(s->packing);
    return encode_pieces(&s->obj, s->encoder, amp, 2, code, 1, len, PIECE_FRAMES*unit_samples(s->packing));
}

int gsm0610_decode(gsm0610_state_t *s, int16_t amp[], const uint8_t code[], int len)
{
    if (s == NULL  ||  s->decoder == NULL  ||  code == NULL  ||  amp == NULL)
        return 0;
    len -= len%unit_bytes(s->packing);
    return decode_pieces(&s->obj, s->decoder, code, 1, amp, 2, len, PIECE_FRAMES*unit_bytes(s->packing));
}
