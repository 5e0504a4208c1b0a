/*
 * shim_adpcm.c -- host side (plain C) of the spandsp-named entry points for IMA and OKI ADPCM, declared in
 * include/spangpu_spandsp.h: ima_adpcm_* and oki_adpcm_*.  An object is a one-channel codec bank of include/spangpu.h
 * ("IMA ADPCM codec banks", "OKI ADPCM codec banks").  Without a GPU the init calls return NULL: there is no CPU
 * implementation.
 */
#include "shim_object.h"

/* samples (encode) or bytes (decode) per launch of one object: kMaxSamples, bank_host.hpp (tests/test_adpcm.py builds this file
   with a smaller one to walk the piece loop) */
#ifndef ADPCM_PIECE
#define ADPCM_PIECE (1 << 24)
#endif
#define PIECE       ADPCM_PIECE

OBJ_CODEC_LOOP(ima_encode_pieces, spangpu_ima_adpcm_t, spangpu_ima_adpcm_encode_capacity, spangpu_ima_adpcm_encode)
OBJ_CODEC_LOOP(ima_decode_pieces, spangpu_ima_adpcm_t, spangpu_ima_adpcm_decode_capacity, spangpu_ima_adpcm_decode)
OBJ_CODEC_LOOP(oki_encode_pieces, spangpu_oki_adpcm_t, spangpu_oki_adpcm_encode_capacity, spangpu_oki_adpcm_encode)
OBJ_CODEC_LOOP(oki_decode_pieces, spangpu_oki_adpcm_t, spangpu_oki_adpcm_decode_capacity, spangpu_oki_adpcm_decode)

ima_adpcm_state_t *ima_adpcm_init(ima_adpcm_state_t *s, int variant, int chunk_size)
{
    const int32_t v = variant;
    const int32_t chunk = chunk_size;
    spangpu_ima_adpcm_t *bank;

    if (spangpu_ima_adpcm_create(&bank, 0, 1, &v, &chunk, 1) != SPANGPU_OK)
        return NULL;
    if ((s = OBJ_TAKE(s, ima_adpcm_state_t)) == NULL)
    {
        spangpu_ima_adpcm_destroy(bank);
        return NULL;
    }
    s->bank = bank;
    s->variant = variant;
    s->chunk_size = chunk_size;
    return s;
}

int ima_adpcm_release(ima_adpcm_state_t *s)
{
    if (s)
    {
        if (s->bank)
            spangpu_ima_adpcm_destroy(s->bank);
        s->bank = NULL;
        obj_drop(&s->obj, NULL);
    }
    return 0;
}

int ima_adpcm_free(ima_adpcm_state_t *s)
{
    if (s)
    {
        ima_adpcm_release(s);
        obj_drop(&s->obj, s);
    }
    return 0;
}

/* a call whose pieces would not add up to it: every call has a header (chunk_size == 0), or resets and pads its bits (VDVI) */
static int ima_one_piece_only(const ima_adpcm_state_t *s, int len)
{
    return len > PIECE  &&  (s->chunk_size == 0  ||  s->variant == IMA_ADPCM_VDVI);
}

int ima_adpcm_encode(ima_adpcm_state_t *s, uint8_t ima_data[], const int16_t amp[], int len)
{
    if (s == NULL  ||  s->bank == NULL  ||  ima_data == NULL  ||  amp == NULL  ||  ima_one_piece_only(s, len))
        return 0;
    return ima_encode_pieces(&s->obj, s->bank, amp, 2, ima_data, 1, len, PIECE);
}

int ima_adpcm_decode(ima_adpcm_state_t *s, int16_t amp[], const uint8_t ima_data[], int ima_bytes)
{
    if (s == NULL  ||  s->bank == NULL  ||  ima_data == NULL  ||  amp == NULL  ||  ima_one_piece_only(s, ima_bytes))
        return 0;
    return ima_decode_pieces(&s->obj, s->bank, ima_data, 1, amp, 2, ima_bytes, PIECE);
}

oki_adpcm_state_t *oki_adpcm_init(oki_adpcm_state_t *s, int bit_rate)
{
    const int32_t rate = bit_rate;
    spangpu_oki_adpcm_t *bank;

    /* (the bank refuses the rates oki_adpcm_init() refuses, oki_adpcm.c:246-247) */
    if (spangpu_oki_adpcm_create(&bank, 0, 1, &rate, 1) != SPANGPU_OK)
        return NULL;
    if ((s = OBJ_TAKE(s, oki_adpcm_state_t)) == NULL)
    {
        spangpu_oki_adpcm_destroy(bank);
        return NULL;
    }
    s->bank = bank;
    s->bit_rate = bit_rate;
    return s;
}

int oki_adpcm_release(oki_adpcm_state_t *s)
{
    if (s)
    {
        if (s->bank)
            spangpu_oki_adpcm_destroy(s->bank);
        s->bank = NULL;
        obj_drop(&s->obj, NULL);
    }
    return 0;
}

int oki_adpcm_free(oki_adpcm_state_t *s)
{
    if (s)
    {
        oki_adpcm_release(s);
        obj_drop(&s->obj, s);
    }
    return 0;
}

/* (the 24 kbit/s decoder's nibble counter restarts with each piece as with each call; a piece is a whole number of bytes) */
int oki_adpcm_encode(oki_adpcm_state_t *s, uint8_t oki_data[], const int16_t amp[], int len)
{
    if (s == NULL  ||  s->bank == NULL  ||  oki_data == NULL  ||  amp == NULL)
        return 0;
    return oki_encode_pieces(&s->obj, s->bank, amp, 2, oki_data, 1, len, PIECE);
}

int oki_adpcm_decode(oki_adpcm_state_t *s, int16_t amp[], const uint8_t oki_data[], int oki_bytes)
{
    if (s == NULL  ||  s->bank == NULL  ||  oki_data == NULL  ||  amp == NULL)
        return 0;
    return oki_decode_pieces(&s->obj, s->bank, oki_data, 1, amp, 2, oki_bytes, PIECE);
}
