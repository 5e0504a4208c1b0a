/*
 * gsm0610_host.c -- the host-only parts of the GSM 06.10 codec: the three packers and the three unpackers of a frame's 76
 * parameters under their spandsp names (include/spangpu_spandsp.h), plain C with no HIP in it, so they need no GPU and a
 * stand-alone program can link this file alone.  The kernels pack and unpack on the device (csrc/gsm0610_dev.hpp).
 *
 * Written from the layouts, not from the reference's shift registers (src/gsm0610_encode.c:115-280, src/gsm0610_decode.c:
 * 103-310).  All three carry the parameters in one order: LARc[8] in 6,6,5,5,4,4,3,3 bits, then per subframe Nc (7), bc (2),
 * Mc (2), xmaxc (6) and xMc[13] (3 each): 260 bits.
 *   none    a byte a parameter, 76 bytes
 *   voip    the nibble 0xD, then the 260 bits, the first bit in the top bit of the first byte: 33 bytes
 *   wav49   the 260 bits of two frames, the first bit in the bottom bit of the first byte: 65 bytes
 * A packer keeps the low bits of a parameter (eight of them where a byte holds it), as the reference's do.
 */
#include <stddef.h>
#include <string.h>

#include "spangpu_spandsp.h"

#define PARAMS      76

static const uint8_t lar_bits[8] = {6, 6, 5, 5, 4, 4, 3, 3};

/* parameter k of a frame, in stream order, and its width */
static int16_t *param(gsm0610_frame_t *f, int k, int *bits)
{
    int sub;
    int i;

    if (k < 8)
    {
        *bits = lar_bits[k];
        return &f->LARc[k];
    }
    sub = (k - 8)/17;
    i = (k - 8)%17;
    switch (i)
    {
    case 0:
        *bits = 7;
        return &f->Nc[sub];
    case 1:
        *bits = 2;
        return &f->bc[sub];
    case 2:
        *bits = 2;
        return &f->Mc[sub];
    case 3:
        *bits = 6;
        return &f->xmaxc[sub];
    }
    *bits = 3;
    return &f->xMc[sub][i - 4];
}

/* `bits` of v at bit `at` of the stream in c[], the stream's first bit on top of a byte or at its bottom */
static void put_bits(uint8_t *c, int at, int bits, unsigned int v, int top_first)
{
    int i;

    for (i = 0;  i < bits;  i++, at++)
    {
        const unsigned int bit = top_first  ?  ((v >> (bits - 1 - i)) & 1)  :  ((v >> i) & 1);

        if (bit)
            c[at >> 3] |= (uint8_t) (top_first  ?  (0x80 >> (at & 7))  :  (1 << (at & 7)));
    }
}

static unsigned int get_bits(const uint8_t *c, int at, int bits, int top_first)
{
    unsigned int v = 0;
    int i;

    for (i = 0;  i < bits;  i++, at++)
    {
        const unsigned int bit = top_first  ?  ((c[at >> 3] >> (7 - (at & 7))) & 1)  :  ((c[at >> 3] >> (at & 7)) & 1);

        v |= top_first  ?  (bit << (bits - 1 - i))  :  (bit << i);
    }
    return v;
}

static int pack_stream(uint8_t *c, int at, const gsm0610_frame_t *f, int top_first)
{
    int k;
    int bits;

    for (k = 0;  k < PARAMS;  k++)
    {
        const int16_t *p = param((gsm0610_frame_t *) f, k, &bits);

        put_bits(c, at, bits, (unsigned int) *p & ((1u << bits) - 1u), top_first);
        at += bits;
    }
    return at;
}

static int unpack_stream(gsm0610_frame_t *f, const uint8_t *c, int at, int top_first)
{
    int k;
    int bits;

    for (k = 0;  k < PARAMS;  k++)
    {
        int16_t *p = param(f, k, &bits);

        *p = (int16_t) get_bits(c, at, bits, top_first);
        at += bits;
    }
    return at;
}

int gsm0610_pack_none(uint8_t c[76], const gsm0610_frame_t *s)
{
    int k;
    int bits;

    for (k = 0;  k < PARAMS;  k++)
        c[k] = (uint8_t) *param((gsm0610_frame_t *) s, k, &bits);
    return 76;
}

int gsm0610_pack_wav49(uint8_t c[65], const gsm0610_frame_t *s)
{
    memset(c, 0, 65);
    (void) pack_stream(c, pack_stream(c, 0, &s[0], 0), &s[1], 0);
    return 65;
}

int gsm0610_pack_voip(uint8_t c[33], const gsm0610_frame_t *s)
{
    memset(c, 0, 33);
    put_bits(c, 0, 4, 0xD, 1);
    (void) pack_stream(c, 4, s, 1);
    return 33;
}

int gsm0610_unpack_none(gsm0610_frame_t *s, const uint8_t c[76])
{
    int k;
    int bits;

    for (k = 0;  k < PARAMS;  k++)
        *param(s, k, &bits) = c[k];
    return 76;
}

int gsm0610_unpack_wav49(gsm0610_frame_t *s, const uint8_t c[65])
{
    (void) unpack_stream(&s[1], c, unpack_stream(&s[0], c, 0, 0), 0);
    return 65;
}

int gsm0610_unpack_voip(gsm0610_frame_t *s, const uint8_t c[33])
{
    (void) unpack_stream(s, c, 4, 1);
    return 33;
}
