/*
 * adpcm_caller.c -- a caller of the reference's IMA and OKI ADPCM names, unchanged but for the header: a line of int16_t
 * samples through a VDVI encoder with chunk_size 0 (every call a packet with its header) in the caller's own storage and an
 * allocated decoder that takes the packets one for one; then through a 24 kbit/s OKI encoder and decoder, the bytes cut on
 * the same schedule.  The calls are of 1, 2, 3, 7, 15, 16, 17, 33, 160 and 161.  What comes out is held against the FNV-1a
 * sums below, taken from the fixture lines (tests/golden/ima_adpcm.npz, oki_adpcm.npz); tests/test_adpcm_c_gpu.py writes
 * the line out for it and checks that the sums here are the fixtures'.
 *
 *   adpcm_caller <file: n, the samples>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu_spandsp.h"

#define SUM_VDVI_CODES      0x44925653u
#define SUM_VDVI_SAMPLES    0x8fa26182u
#define SUM_OKI_CODES       0x5fc24dd8u
#define SUM_OKI_SAMPLES     0x0901edfeu

static const int schedule[10] = {1, 2, 3, 7, 15, 16, 17, 33, 160, 161};

static unsigned fnv(unsigned h, const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *) p;
    size_t i;

    for (i = 0;  i < n;  i++)
        h = (h ^ b[i])*16777619u;
    return h;
}

static int check(const char *what, unsigned got, unsigned want)
{
    printf("%s %08x%s\n", what, got, (got == want)  ?  ""  :  " DIFFERS");
    return got != want;
}

int main(int argc, char **argv)
{
    ima_adpcm_state_t enc;
    ima_adpcm_state_t *dec;
    oki_adpcm_state_t *oenc;
    oki_adpcm_state_t odec;
    FILE *f;
    int16_t *amp;
    int16_t *back;
    uint8_t *codes;
    unsigned h_codes = 2166136261u;
    unsigned h_samples = 2166136261u;
    int n;
    int i;
    int k;
    int v;
    int at;
    int bytes;
    int total;
    int samples;
    int bad = 0;

    if (argc != 2  ||  (f = fopen(argv[1], "r")) == NULL  ||  fscanf(f, "%d", &n) != 1  ||  n <= 0)
        return 2;
    amp = (int16_t *) malloc(sizeof(int16_t)*(size_t) n);
    back = (int16_t *) malloc(sizeof(int16_t)*(size_t) (4*n + 16));
    codes = (uint8_t *) malloc((size_t) n + 16);
    if (amp == NULL  ||  back == NULL  ||  codes == NULL)
        return 2;
    for (i = 0;  i < n;  i++)
    {
        if (fscanf(f, "%d", &v) != 1)
            return 2;
        amp[i] = (int16_t) v;
    }
    fclose(f);

    /* VDVI, a packet a call */
    if (ima_adpcm_init(&enc, IMA_ADPCM_VDVI, 0) != &enc  ||  (dec = ima_adpcm_init(NULL, IMA_ADPCM_VDVI, 0)) == NULL)
    {
        printf("no device\n");
        return 3;
    }
    total = 0;
    samples = 0;
    for (at = 0, k = 0;  at < n;  k++)
    {
        const int len = (n - at < schedule[k % 10])  ?  (n - at)  :  schedule[k % 10];

        bytes = ima_adpcm_encode(&enc, codes, amp + at, len);
        h_codes = fnv(h_codes, codes, (size_t) bytes);
        v = ima_adpcm_decode(dec, back, codes, bytes);
        h_samples = fnv(h_samples, back, sizeof(int16_t)*(size_t) v);
        at += len;
        total += bytes;
        samples += v;
    }
    printf("vdvi: %d samples, %d bytes, %d samples back\n", n, total, samples);
    bad += check("vdvi codes", h_codes, SUM_VDVI_CODES);
    bad += check("vdvi samples", h_samples, SUM_VDVI_SAMPLES);
    ima_adpcm_release(&enc);
    ima_adpcm_free(&enc);
    ima_adpcm_free(dec);

    /* OKI at 24 kbit/s: the whole stream first, then its bytes on the schedule */
    if ((oenc = oki_adpcm_init(NULL, 24000)) == NULL  ||  oki_adpcm_init(&odec, 24000) != &odec  ||  oki_adpcm_init(NULL, 16000) != NULL)
        return 3;
    total = 0;
    for (at = 0, k = 0;  at < n;  k++)
    {
        const int len = (n - at < schedule[k % 10])  ?  (n - at)  :  schedule[k % 10];

        total += oki_adpcm_encode(oenc, codes + total, amp + at, len);
        at += len;
    }
    h_codes = fnv(2166136261u, codes, (size_t) total);
    h_samples = 2166136261u;
    samples = 0;
    for (at = 0, k = 0;  at < total;  k++)
    {
        const int len = (total - at < schedule[k % 10])  ?  (total - at)  :  schedule[k % 10];

        v = oki_adpcm_decode(&odec, back, codes + at, len);
        h_samples = fnv(h_samples, back, sizeof(int16_t)*(size_t) v);
        at += len;
        samples += v;
    }
    printf("oki: %d samples, %d bytes, %d samples back\n", n, total, samples);
    bad += check("oki codes", h_codes, SUM_OKI_CODES);
    bad += check("oki samples", h_samples, SUM_OKI_SAMPLES);
    oki_adpcm_free(oenc);
    oki_adpcm_release(&odec);
    free(amp);
    free(back);
    free(codes);
    if (bad)
        return 1;
    printf("ok\n");
    return 0;
}
