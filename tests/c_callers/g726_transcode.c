/*
 * g726_transcode.c -- a caller of the reference's G.726 names, unchanged but for the header: A-law in, 32 kbit/s ADPCM
 * right-packed, A-law out, the encoder in the caller's own storage and the decoder allocated by g726_init(), on calls of
 * 160, 1, 7, 80 and 333.  tests/test_g726_c_gpu.py writes the fixture's bytes out and holds the result against them.
 *
 *   g726_transcode <file: n_in, the A-law bytes, n_codes, the packed bytes, n_out, the A-law bytes the decoder makes>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu_spandsp.h"

static uint8_t *read_block(FILE *f, int *n)
{
    uint8_t *p;
    int i;
    int v;

    if (fscanf(f, "%d", n) != 1  ||  *n <= 0  ||  (p = (uint8_t *) malloc((size_t) *n + 8)) == NULL)
        exit(2);
    for (i = 0;  i < *n;  i++)
    {
        if (fscanf(f, "%d", &v) != 1)
            exit(2);
        p[i] = (uint8_t) v;
    }
    return p;
}

int main(int argc, char **argv)
{
    static const int schedule[5] = {160, 1, 7, 80, 333};
    g726_state_t enc;
    g726_state_t *dec;
    uint8_t *in;
    uint8_t *codes;
    uint8_t *want;
    uint8_t *packed;
    uint8_t *out;
    FILE *f;
    int n_in;
    int n_codes;
    int n_out;
    int at;
    int made;
    int k;

    if (argc != 2  ||  (f = fopen(argv[1], "r")) == NULL)
        return 2;
    in = read_block(f, &n_in);
    codes = read_block(f, &n_codes);
    want = read_block(f, &n_out);
    fclose(f);
    packed = (uint8_t *) malloc((size_t) n_in + 8);
    out = (uint8_t *) malloc((size_t) n_in + 8);
    if (packed == NULL  ||  out == NULL)
        return 2;
    /* the rates g726_init() refuses */
    if (g726_init(NULL, 8000, G726_ENCODING_ALAW, G726_PACKING_RIGHT) != NULL  ||  g726_init(&enc, 48000, G726_ENCODING_LINEAR, G726_PACKING_NONE) != NULL)
    {
        printf("FAIL: g726_init() took a rate it refuses\n");
        return 1;
    }
    if (g726_init(&enc, 32000, G726_ENCODING_ALAW, G726_PACKING_RIGHT) != &enc
        ||  (dec = g726_init(NULL, 32000, G726_ENCODING_ALAW, G726_PACKING_RIGHT)) == NULL)
    {
        printf("FAIL: g726_init()\n");
        return 1;
    }
    for (at = 0, made = 0, k = 0;  at < n_in;  k++)
    {
        const int n = (schedule[k % 5] < n_in - at)  ?  schedule[k % 5]  :  (n_in - at);

        /* (G.711 bytes through the int16_t pointer, as the reference's callers pass them) */
        made += g726_encode(&enc, packed + made, (const int16_t *) (const void *) (in + at), n);
        at += n;
    }
    if (made != n_codes  ||  memcmp(packed, codes, (size_t) made) != 0)
    {
        printf("FAIL: %d bytes of codes, the reference made %d, or they differ\n", made, n_codes);
        return 1;
    }
    for (at = 0, made = 0, k = 0;  at < n_codes;  k++)
    {
        const int n = (schedule[k % 5] < n_codes - at)  ?  schedule[k % 5]  :  (n_codes - at);

        made += g726_decode(dec, (int16_t *) (void *) (out + made), packed + at, n);
        at += n;
    }
    if (made != n_out  ||  memcmp(out, want, (size_t) made) != 0)
    {
        printf("FAIL: %d samples decoded, the reference made %d, or they differ\n", made, n_out);
        return 1;
    }
    if (g726_release(&enc) != 0  ||  g726_free(&enc) != 0  ||  g726_free(dec) != 0)
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
