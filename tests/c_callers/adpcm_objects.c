/* The IMA and OKI ADPCM objects (csrc/shim_adpcm.c, built with a piece of 4096) over the stand-in bank of
 * tests/adpcm_bank_stub.c: life in caller storage and on the heap, failed init, calls of 0, 1, 4095, 4096, 4097 and 8195
 * items, and NULL.  It prints every return value, a checksum of what the caller's buffer got and whether the bytes behind it
 * were left alone; tests/test_adpcm.py holds the transcript against tests/golden/adpcm_objects.txt. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu_spandsp.h"

extern int stub_fail_create;
extern int stub_live;

#define OUT_BYTES   (64*1024)
#define FILL        0xEE

static uint8_t *out;

static unsigned fnv(const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *) p;
    unsigned h = 2166136261u;
    size_t i;

    for (i = 0;  i < n;  i++)
        h = (h ^ b[i])*16777619u;
    return h;
}

static int all_of(const void *p, size_t n, int byte)
{
    const uint8_t *b = (const uint8_t *) p;
    size_t i;

    for (i = 0;  i < n;  i++)
    {
        if (b[i] != (uint8_t) byte)
            return 0;
    }
    return 1;
}

/* an input of exactly `bytes` bytes on the heap, so that a read past it is seen */
static void *input(size_t bytes)
{
    uint8_t *p = (uint8_t *) malloc(bytes  ?  bytes  :  1);
    size_t i;

    if (p == NULL)
        abort();
    for (i = 0;  i < bytes;  i++)
        p[i] = (uint8_t) (i*13 + 5);
    return p;
}

static void report(const char *what, int len, int ret, size_t el)
{
    const size_t got = (ret > 0)  ?  (size_t) ret*el  :  0;

    printf("%s(%d) -> %d, sum %08x, behind it %s\n", what, len, ret, fnv(out, got), all_of(out + got, OUT_BYTES - got, FILL)  ?  "untouched"  :  "WRITTEN");
}

#define LIFE(T, pfx, INIT)                                                                                              \
do                                                                                                                      \
{                                                                                                                       \
    T st;                                                                                                               \
    T *s;                                                                                                               \
                                                                                                                        \
    printf("== " #pfx ": life\n");                                                                                      \
    s = INIT(NULL);                                                                                                     \
    printf("init(NULL) -> %s\n", s  ?  "an object"  :  "NULL");                                                         \
    printf("release -> %d\n", pfx##_release(s));                                                                        \
    printf("release -> %d\n", pfx##_release(s));                                                                        \
    printf("free -> %d\n", pfx##_free(s));                                                                              \
    s = INIT(&st);                                                                                                      \
    printf("init(&st) -> %s\n", (s == &st)  ?  "&st"  :  (s  ?  "another object"  :  "NULL"));                          \
    printf("release -> %d\n", pfx##_release(s));                                                                        \
    printf("release -> %d\n", pfx##_release(s));                                                                        \
    printf("free -> %d\n", pfx##_free(s));                                                                              \
    printf("free(NULL) -> %d\n", pfx##_free(NULL));                                                                     \
    printf("release(NULL) -> %d\n", pfx##_release(NULL));                                                               \
    memset(&st, 0xA5, sizeof(st));                                                                                      \
    stub_fail_create = 1;                                                                                               \
    s = INIT(&st);                                                                                                      \
    printf("failed init(&st) -> %s\n", s  ?  "an object"  :  "NULL");                                                   \
    printf(#pfx ": storage %s after failed init\n", all_of(&st, sizeof(st), 0xA5)  ?  "unchanged"  :  "changed");       \
    stub_fail_create = 1;                                                                                               \
    s = INIT(NULL);                                                                                                     \
    printf("failed init(NULL) -> %s\n", s  ?  "an object"  :  "NULL");                                                  \
    stub_fail_create = 0;                                                                                               \
    printf("live banks: %d\n", stub_live);                                                                              \
}                                                                                                                       \
while (0)

#define ENCODE(what, call, s, len)                                                                                      \
do                                                                                                                      \
{                                                                                                                       \
    void *in = input((size_t) (len)*2);                                                                                 \
                                                                                                                        \
    memset(out, FILL, OUT_BYTES);                                                                                       \
    report(what, len, call(s, out, (const int16_t *) in, len), 1);                                                      \
    free(in);                                                                                                           \
}                                                                                                                       \
while (0)

#define DECODE(what, call, s, len)                                                                                      \
do                                                                                                                      \
{                                                                                                                       \
    void *in = input((size_t) (len));                                                                                   \
                                                                                                                        \
    memset(out, FILL, OUT_BYTES);                                                                                       \
    report(what, len, call(s, (int16_t *) out, (const uint8_t *) in, len), 2);                                          \
    free(in);                                                                                                           \
}                                                                                                                       \
while (0)

static const int lengths[6] = { 0, 1, 4095, 4096, 4097, 8195 };

#define IMA_INIT(s)     ima_adpcm_init(s, IMA_ADPCM_DVI4, 64)
#define OKI_INIT(s)     oki_adpcm_init(s, 24000)

int main(void)
{
    static const int ima[4][2] = { {IMA_ADPCM_IMA4, 64}, {IMA_ADPCM_DVI4, 0}, {IMA_ADPCM_VDVI, 64}, {IMA_ADPCM_VDVI, 0} };
    static const int oki[2] = { 32000, 24000 };
    ima_adpcm_state_t *a;
    oki_adpcm_state_t *o;
    int c;
    int i;

    if ((out = (uint8_t *) malloc(OUT_BYTES)) == NULL)
        abort();
    LIFE(ima_adpcm_state_t, ima_adpcm, IMA_INIT);
    for (c = 0;  c < 4;  c++)
    {
        /* (a call with a header, or of VDVI, is one launch or none: its pieces would not add up to it) */
        printf("== ima_adpcm: pieces, variant %d, chunk %d\n", ima[c][0], ima[c][1]);
        a = ima_adpcm_init(NULL, ima[c][0], ima[c][1]);
        for (i = 0;  i < 6;  i++)
            ENCODE("ima_adpcm_encode", ima_adpcm_encode, a, lengths[i]);
        for (i = 0;  i < 6;  i++)
            DECODE("ima_adpcm_decode", ima_adpcm_decode, a, lengths[i]);
        ima_adpcm_free(a);
    }
    a = ima_adpcm_init(NULL, IMA_ADPCM_DVI4, 0);
    printf("ima_adpcm_encode(NULL) -> %d\n", ima_adpcm_encode(NULL, out, (const int16_t *) out, 8));
    printf("ima_adpcm_decode(NULL) -> %d\n", ima_adpcm_decode(NULL, (int16_t *) out, out, 8));
    printf("ima_adpcm_encode(no data) -> %d\n", ima_adpcm_encode(a, NULL, (const int16_t *) out, 8));
    printf("ima_adpcm_encode(no amp) -> %d\n", ima_adpcm_encode(a, out, NULL, 8));
    printf("ima_adpcm_decode(no amp) -> %d\n", ima_adpcm_decode(a, NULL, out, 8));
    printf("ima_adpcm_decode(no data) -> %d\n", ima_adpcm_decode(a, (int16_t *) out, NULL, 8));
    ima_adpcm_free(a);

    LIFE(oki_adpcm_state_t, oki_adpcm, OKI_INIT);
    for (c = 0;  c < 2;  c++)
    {
        printf("== oki_adpcm: pieces, rate %d\n", oki[c]);
        o = oki_adpcm_init(NULL, oki[c]);
        for (i = 0;  i < 6;  i++)
            ENCODE("oki_adpcm_encode", oki_adpcm_encode, o, lengths[i]);
        for (i = 0;  i < 6;  i++)
            DECODE("oki_adpcm_decode", oki_adpcm_decode, o, lengths[i]);
        oki_adpcm_free(o);
    }
    o = oki_adpcm_init(NULL, 32000);
    printf("oki_adpcm_encode(NULL) -> %d\n", oki_adpcm_encode(NULL, out, (const int16_t *) out, 8));
    printf("oki_adpcm_decode(NULL) -> %d\n", oki_adpcm_decode(NULL, (int16_t *) out, out, 8));
    printf("oki_adpcm_encode(no data) -> %d\n", oki_adpcm_encode(o, NULL, (const int16_t *) out, 8));
    printf("oki_adpcm_encode(no amp) -> %d\n", oki_adpcm_encode(o, out, NULL, 8));
    printf("oki_adpcm_decode(no amp) -> %d\n", oki_adpcm_decode(o, NULL, out, 8));
    printf("oki_adpcm_decode(no data) -> %d\n", oki_adpcm_decode(o, (int16_t *) out, NULL, 8));
    oki_adpcm_free(o);
    printf("live banks at the end: %d\n", stub_live);
    free(out);
    return 0;
}
