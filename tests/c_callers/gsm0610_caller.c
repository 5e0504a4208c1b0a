/*
 * gsm0610_caller.c -- a caller of the reference's GSM 06.10 names, unchanged but for the header: a line through
 * gsm0610_encode() in the VoIP packing and back through gsm0610_decode(), in calls of two frames, the encoder in the caller's
 * own storage and the decoder allocated by gsm0610_init(); every frame unpacked, packed as WAV49 and as unpacked bytes and
 * held against what the reference's encoders made in those packings; then gsm0610_set_packing() in mid-stream.
 * tests/test_gsm0610_c_gpu.py writes the fixture's line, codes and samples out and holds the result against them.
 *
 *   gsm0610_caller <file: n_in, the samples, n_voip, the VoIP bytes, n_wav49, the WAV49 bytes, n_none, the unpacked bytes,
 *                   n_out, the samples the decoder makes>
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

static int same(const uint8_t *got, const int16_t *want, int n)
{
    int i;

    for (i = 0;  i < n;  i++)
    {
        if (got[i] != (uint8_t) want[i])
            return 0;
    }
    return 1;
}

int main(int argc, char **argv)
{
    gsm0610_state_t enc;
    gsm0610_state_t *dec;
    gsm0610_state_t *turn;
    gsm0610_frame_t pair[2];
    gsm0610_frame_t again[2];
    int16_t *in;
    int16_t *voip;
    int16_t *wav49;
    int16_t *none;
    int16_t *want;
    int16_t *out;
    uint8_t *codes;
    uint8_t buf[76];
    FILE *f;
    int n_in;
    int n_voip;
    int n_wav49;
    int n_none;
    int n_out;
    int at;
    int made;
    int got;
    int bytes;
    int k;

    if (argc != 2  ||  (f = fopen(argv[1], "r")) == NULL)
        return 2;
    in = read_block(f, &n_in);
    voip = read_block(f, &n_voip);
    wav49 = read_block(f, &n_wav49);
    none = read_block(f, &n_none);
    want = read_block(f, &n_out);
    fclose(f);
    codes = (uint8_t *) malloc((size_t) n_in + 8);
    out = (int16_t *) malloc(((size_t) n_in + 8)*sizeof(int16_t));
    if (codes == NULL  ||  out == NULL)
        return 2;
    if (gsm0610_init(&enc, GSM0610_PACKING_VOIP) != &enc  ||  (dec = gsm0610_init(NULL, GSM0610_PACKING_VOIP)) == NULL)
    {
        printf("FAIL: init\n");
        return 1;
    }
    for (at = 0, made = 0, got = 0;  at < n_in;  )
    {
        /* (a partial frame at the end would be left out: the line is whole frames) */
        const int n = (320 < n_in - at)  ?  320  :  (n_in - at);

        bytes = gsm0610_encode(&enc, codes + made, in + at, n);
        got += gsm0610_decode(dec, out + got, codes + made, bytes);
        made += bytes;
        at += n;
    }
    if (made != n_voip  ||  !same(codes, voip, made))
    {
        printf("FAIL: %d bytes of codes, the reference made %d, or they differ\n", made, n_voip);
        return 1;
    }
    if (got != n_out  ||  memcmp(out, want, (size_t) got*sizeof(int16_t)) != 0)
    {
        printf("FAIL: %d samples decoded, the reference made %d, or they differ\n", got, n_out);
        return 1;
    }
    /* the six host calls: every pair of VoIP frames as the WAV49 and the unpacked bytes the reference made */
    for (k = 0;  k + 1 < made/33;  k += 2)
    {
        if (gsm0610_unpack_voip(&pair[0], codes + 33*k) != 33  ||  gsm0610_unpack_voip(&pair[1], codes + 33*(k + 1)) != 33
            ||  gsm0610_pack_wav49(buf, pair) != 65  ||  !same(buf, wav49 + 65*(k/2), 65)
            ||  gsm0610_unpack_wav49(again, buf) != 65  ||  memcmp(again, pair, sizeof(pair)) != 0
            ||  gsm0610_pack_none(buf, &pair[1]) != 76  ||  !same(buf, none + 76*(k + 1), 76)
            ||  gsm0610_unpack_none(&again[0], buf) != 76  ||  memcmp(&again[0], &pair[1], sizeof(pair[1])) != 0
            ||  gsm0610_pack_voip(buf, &again[0]) != 33  ||  memcmp(buf, codes + 33*(k + 1), 33) != 0)
        {
            printf("FAIL: pack / unpack at frame %d\n", k);
            return 1;
        }
    }
    /* an encoder that turns to WAV49 after two VoIP frames: the parameters do not depend on the packing; a length that is no
       whole number of frames leaves the rest out, and a packing the reference does not name is the unpacked one */
    if ((turn = gsm0610_init(NULL, GSM0610_PACKING_VOIP)) == NULL  ||  gsm0610_encode(turn, codes, in, 320 + 159) != 66  ||  !same(codes, voip, 66)
        ||  gsm0610_set_packing(turn, GSM0610_PACKING_WAV49) != 0  ||  gsm0610_encode(turn, codes, in + 320, 320) != 65  ||  !same(codes, wav49 + 65, 65)
        ||  gsm0610_set_packing(turn, 7) != 0  ||  turn->packing != GSM0610_PACKING_NONE
        ||  gsm0610_encode(turn, codes, in + 640, 160) != 76  ||  !same(codes, none + 4*76, 76))
    {
        printf("FAIL: set_packing in mid-stream\n");
        return 1;
    }
    if (gsm0610_release(&enc) != 0  ||  gsm0610_free(&enc) != 0  ||  gsm0610_free(turn) != 0  ||  gsm0610_release(dec) != 0  ||  gsm0610_free(dec) != 0)
    {
        printf("FAIL: release / free\n");
        return 1;
    }
    free(in);
    free(voip);
    free(wav49);
    free(none);
    free(want);
    free(codes);
    free(out);
    printf("ok %d samples, %d bytes\n", n_in, n_voip);
    return 0;
}
