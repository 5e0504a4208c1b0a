/*
 * g722_caller.c -- a caller of the reference's G.722 names, unchanged but for the header: a line through g722_encode() at
 * 56 kbit/s, packed, and back through g722_decode(), in calls of 160 samples and of the bytes each of them made, the encoder
 * in the caller's own storage and the decoder allocated by g722_decode_init().  tests/test_g722_c_gpu.py writes the
 * fixture's line, codes and samples out and holds the result against them.
 *
 *   g722_caller <file: n_in, the samples, n_codes, the packed bytes, n_out, the samples the decoder makes>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu_spandsp.h"

static int16_t *read_block(FILE *f, int *n)
{
    int16_t *p;
    int i;
    int v;

    if (fscanf(f, "%d", n) != 1  ||  *n <= 0  ||  (p = (int16_t *) malloc(((size_t) *n + 8)*sizeof(int16_t))) == NULL)
        exit(2);
    for (i = 0;  i < *n;  i++)
    {
        if (fscanf(f, "%d", &v) != 1)
            exit(2);
        p[i] = (int16_t) v;
    }
    return p;
}

int main(int argc, char **argv)
{
    g722_encode_state_t enc;
    g722_encode_state_t *odd;
    g722_decode_state_t *dec;
    int16_t *in;
    int16_t *codes;
    int16_t *want;
    int16_t *out;
    uint8_t *packed;
    FILE *f;
    int n_in;
    int n_codes;
    int n_out;
    int at;
    int made;
    int got;
    int bytes;
    int i;

    if (argc != 2  ||  (f = fopen(argv[1], "r")) == NULL)
        return 2;
    in = read_block(f, &n_in);
    codes = read_block(f, &n_codes);
    want = read_block(f, &n_out);
    fclose(f);
    packed = (uint8_t *) malloc((size_t) n_in + 8);
    out = (int16_t *) malloc(((size_t) n_in + 8)*sizeof(int16_t));
    if (packed == NULL  ||  out == NULL)
        return 2;
    if (g722_encode_init(&enc, 56000, G722_PACKED) != &enc  ||  (dec = g722_decode_init(NULL, 56000, G722_PACKED)) == NULL)
    {
        printf("FAIL: init\n");
        return 1;
    }
    for (at = 0, made = 0, got = 0;  at < n_in;  )
    {
        const int n = (160 < n_in - at)  ?  160  :  (n_in - at);

        bytes = g722_encode(&enc, packed + made, in + at, n);
        got += g722_decode(dec, out + got, packed + made, bytes);
        made += bytes;
        at += n;
    }
    if (made != n_codes)
    {
        printf("FAIL: %d bytes of codes, the reference made %d\n", made, n_codes);
        return 1;
    }
    for (i = 0;  i < made;  i++)
    {
        if (packed[i] != (uint8_t) codes[i])
        {
            printf("FAIL: byte %d is %d, the reference made %d\n", i, packed[i], codes[i]);
            return 1;
        }
    }
    if (got != n_out  ||  memcmp(out, want, (size_t) got*sizeof(int16_t)) != 0)
    {
        printf("FAIL: %d samples decoded, the reference made %d, or they differ\n", got, n_out);
        return 1;
    }
    /* every rate but 48000 and 56000 is 64000, as in the reference; an odd len on a 16 kHz encoder leaves the last sample out */
    if ((odd = g722_encode_init(NULL, 8000, 0)) == NULL  ||  odd->bits_per_sample != 8  ||  g722_encode(odd, packed, in, 7) != 3)
    {
        printf("FAIL: an unknown rate, or an odd len\n");
        return 1;
    }
    if (g722_encode_release(&enc) != 0  ||  g722_encode_free(&enc) != 0  ||  g722_encode_free(odd) != 0  ||  g722_decode_release(dec) != 0
        ||  g722_decode_free(dec) != 0)
    {
        printf("FAIL: release / free\n");
        return 1;
    }
    free(in);
    free(codes);
    free(want);
    free(packed);
    free(out);
    printf("ok %d samples, %d bytes\n", n_in, n_codes);
    return 0;
}
