/*
 * plc_caller.c -- a caller of the reference's packet loss concealment names, unchanged but for the header: one line through
 * plc_rx() where a packet came and plc_fillin() where none did, once with a concealer allocated by plc_init(NULL) and once with
 * one in the caller's own storage, each call's samples held against what the reference made of them.
 * tests/test_plc_c_gpu.py writes a case of the fixture out.
 *
 *   plc_caller <file: n_calls, then per call: lost, len, the samples going in, the samples coming out>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu_spandsp.h"

static int next_int(FILE *f)
{
    int v;

    if (fscanf(f, "%d", &v) != 1)
        exit(2);
    return v;
}

int main(int argc, char **argv)
{
    plc_state_t mine;
    plc_state_t *s[2];
    FILE *f;
    int16_t *in;
    int16_t *want;
    int16_t *amp;
    int n_calls;
    int k;
    int i;
    int which;
    int total = 0;

    if (argc != 2  ||  (f = fopen(argv[1], "r")) == NULL)
        return 2;
    if ((s[0] = plc_init(NULL)) == NULL  ||  (s[1] = plc_init(&mine)) != &mine)
    {
        fprintf(stderr, "plc_init failed\n");
        return 1;
    }
    /* nothing to work on: nothing done */
    if (plc_rx(NULL, NULL, 160) != 0  ||  plc_fillin(NULL, NULL, 160) != 0  ||  plc_rx(s[0], NULL, 160) != 0)
        return 1;
    n_calls = next_int(f);
    for (k = 0;  k < n_calls;  k++)
    {
        const int lost = next_int(f);
        const int len = next_int(f);

        in = (int16_t *) malloc((size_t) len*sizeof(int16_t));
        want = (int16_t *) malloc((size_t) len*sizeof(int16_t));
        amp = (int16_t *) malloc((size_t) len*sizeof(int16_t));
        if (in == NULL  ||  want == NULL  ||  amp == NULL)
            return 2;
        for (i = 0;  i < len;  i++)
            in[i] = (int16_t) next_int(f);
        for (i = 0;  i < len;  i++)
            want[i] = (int16_t) next_int(f);
        for (which = 0;  which < 2;  which++)
        {
            memcpy(amp, in, (size_t) len*sizeof(int16_t));
            if ((lost  ?  plc_fillin(s[which], amp, len)  :  plc_rx(s[which], amp, len)) != len)
            {
                fprintf(stderr, "call %d: not %d samples\n", k, len);
                return 1;
            }
            for (i = 0;  i < len;  i++)
            {
                if (amp[i] != want[i])
                {
                    fprintf(stderr, "call %d object %d sample %d: got %d, reference %d\n", k, which, i, amp[i], want[i]);
                    return 1;
                }
            }
        }
        total += len;
        free(in);
        free(want);
        free(amp);
    }
    fclose(f);
    if (plc_release(s[1]) != 0  ||  plc_free(s[1]) != 0  ||  plc_free(s[0]) != 0)
        return 1;
    printf("ok %d calls, %d samples\n", n_calls, total);
    return 0;
}
