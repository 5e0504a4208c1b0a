/* The host-only caller-ID helpers (csrc/adsi_host.c, linked alone: no HIP, no library) over the cases tests/test_adsi.py dumps
 * from the committed fixture.  Built with -fsanitize=address,undefined: every buffer here is allocated at exactly the size the
 * expected result needs, so a byte too many is a finding.  The program checks itself and exits non-zero on a miss.
 *
 * File: u32 count, then per case u32 kind, u32 standard and
 *   kind 0 (pack)   u32 len, msg; i32 expected return; the expected bytes when that is > 0
 *   kind 1 (add)    u32 fields, each u32 type, u32 len, body; u32 expected len, expected bytes
 *   kind 2 (walk)   u32 len, msg; u32 rows, each i32 pos, type, len, body offset (-1: NULL); the last row is the end
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu.h"

static FILE *in;

static unsigned u32(void)
{
    unsigned v = 0;

    if (fread(&v, 4, 1, in) != 1)
    {
        fprintf(stderr, "short file\n");
        exit(2);
    }
    return v;
}

static uint8_t *bytes(unsigned n)
{
    uint8_t *p = (uint8_t *) malloc(n ? n : 1);

    if (p == NULL  ||  (n  &&  fread(p, 1, n, in) != n))
    {
        fprintf(stderr, "short file\n");
        exit(2);
    }
    return p;
}

static int miss(const char *what, unsigned k)
{
    fprintf(stderr, "case %u: %s\n", k, what);
    return 1;
}

int main(int argc, char **argv)
{
    unsigned count;
    unsigned k;

    if (argc < 2  ||  (in = fopen(argv[1], "rb")) == NULL)
        return 2;
    count = u32();
    for (k = 0;  k < count;  k++)
    {
        const unsigned kind = u32();
        const int standard = (int) u32();

        if (kind == 0)
        {
            const unsigned len = u32();
            uint8_t *msg = bytes(len);
            const int want = (int) u32();
            uint8_t *exp = bytes((want > 0)  ?  (unsigned) want  :  0);
            uint8_t *out = (uint8_t *) malloc(SPANGPU_ADSI_MSG_BYTES);
            const int got = spangpu_adsi_pack_message(standard, msg, (int) len, out, SPANGPU_ADSI_MSG_BYTES);

            if (got != want  ||  (want > 0  &&  memcmp(out, exp, (size_t) want) != 0))
                return miss("pack_message", k);
            free(msg);
            free(exp);
            free(out);
        }
        else if (kind == 1)
        {
            const unsigned fields = u32();
            uint8_t **body = (uint8_t **) malloc(fields*sizeof(*body));
            unsigned *type = (unsigned *) malloc(fields*sizeof(*type));
            unsigned *blen = (unsigned *) malloc(fields*sizeof(*blen));
            unsigned f;
            unsigned explen;
            uint8_t *exp;
            uint8_t *msg;
            int shift = (standard == SPANGPU_ADSI_STANDARD_TDD)  ?  2  :  0;    /* how a TDD sender starts */
            int len = -1;

            for (f = 0;  f < fields;  f++)
            {
                type[f] = u32();
                blen[f] = u32();
                body[f] = bytes(blen[f]);
            }
            explen = u32();
            exp = bytes(explen);
            msg = (uint8_t *) malloc(explen ? explen : 1);
            for (f = 0;  f < fields;  f++)
                len = spangpu_adsi_add_field(standard, &shift, msg, len, (uint8_t) type[f], body[f], (int) blen[f]);
            if (len != (int) explen  ||  memcmp(msg, exp, explen) != 0)
                return miss("add_field", k);
            for (f = 0;  f < fields;  f++)
                free(body[f]);
            free(body);
            free(type);
            free(blen);
            free(exp);
            free(msg);
        }
        else
        {
            const unsigned len = u32();
            uint8_t *msg = bytes(len);
            const unsigned rows = u32();
            unsigned r;
            int pos = -1;

            for (r = 0;  r < rows;  r++)
            {
                const int wpos = (int) u32();
                const int wtype = (int) u32();
                const int wlen = (int) u32();
                const int woff = (int) u32();
                uint8_t t = 0;
                const uint8_t *b = NULL;
                int n = 0;

                pos = spangpu_adsi_next_field(standard, msg, (int) len, pos, &t, &b, &n);
                if (pos != wpos)
                    return miss("next_field position", k);
                if (pos >= 0  &&  (t != wtype  ||  n != wlen  ||  (woff < 0  ?  b != NULL  :  b != msg + woff)))
                    return miss("next_field field", k);
            }
            if (pos >= 0)
                return miss("next_field did not end", k);
            free(msg);
        }
    }
    if (strcmp(spangpu_adsi_standard_to_str(SPANGPU_ADSI_STANDARD_JCLIP), "J-CLIP") != 0  ||  strcmp(spangpu_adsi_standard_to_str(9), "???") != 0)
        return miss("standard_to_str", count);
    fclose(in);
    printf("%u cases: ok\n", count);
    return 0;
}
