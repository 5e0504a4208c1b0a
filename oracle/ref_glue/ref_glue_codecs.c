/*
 * ref_glue_codecs.c -- TEST INFRASTRUCTURE ONLY.  OUR drivers over the reference's speech codecs and its packet loss
 * concealer (src/g726.c, src/g722.c, src/gsm0610_*.c, src/plc.c): for each family one accessor that hands out the state as
 * the banks' state words, in the banks' word order (g726_dev.hpp G7_*, g722_dev.hpp G2_*, gsm0610_dev.hpp, plc_dev.hpp), read
 * out of the reference's private structs by offsetof, and one batch driver that takes a line through a schedule of calls, so
 * that a sweep of thousands of lines pays one foreign call a line.  Compiled only into oracle/_ref/libspandsp_codecs_ref.so;
 * #includes reference headers at build time.
 *
 * Every driver: `lens[k]` items go into call k (a call of length 0 is not made: the line sits it out), the outputs lie one
 * behind the other in `out`, `counts[k]` is what call k returned, and `words` receives the state words after the calls asked
 * for, one set behind the other in the order of the calls: call k where want[k] != 0, or the last call alone where want is
 * NULL.  The return value is the number of output items, or -1 where the reference's init refused the configuration.
 */
#include <stdlib.h>
#include <stddef.h>
#include <inttypes.h>
#include <string.h>
#include <stdio.h>
#include <stdbool.h>

#include "spandsp/telephony.h"
#include "spandsp/alloc.h"
#include "spandsp/bitstream.h"
#include "spandsp/g726.h"
#include "spandsp/g722.h"
#include "spandsp/gsm0610.h"
#include "spandsp/plc.h"
#include "spandsp/private/bitstream.h"
#include "spandsp/private/g726.h"
#include "spandsp/private/g722.h"
#include "spandsp/private/gsm0610.h"
#include "spandsp/private/plc.h"

#define GLUE __attribute__((visibility("default")))

#define G726_WORDS      30
#define G722_WORDS      74
#define GSM0610_WORDS   160
#define PLC_WORDS       404
#define GSM_FRAME       160         /* samples in a GSM 06.10 frame */

typedef struct
{
    int32_t off;
    int32_t size;
} field_t;

#define FIELD(type, member)  {(int32_t) offsetof(type, member), (int32_t) sizeof(((type *) 0)->member)}

/* a field's bytes as a signed integer (a float's bit pattern and a sign-extended int16_t alike) */
static int32_t field_word(const void *s, field_t f)
{
    const uint8_t *p = (const uint8_t *) s + f.off;
    int8_t b;
    int16_t h;
    int32_t w;

    switch (f.size)
    {
    case 1:
        memcpy(&b, p, 1);
        return b;
    case 2:
        memcpy(&h, p, 2);
        return h;
    default:
        memcpy(&w, p, 4);
        return w;
    }
}

static void fields_words(const void *s, const field_t f[], int n, int32_t w[])
{
    int i;

    for (i = 0;  i < n;  i++)
        w[i] = field_word(s, f[i]);
}

/* a run of n array elements from `first` on */
static int field_run(field_t f[], int at, field_t first, int n)
{
    int i;

    for (i = 0;  i < n;  i++)
    {
        f[at].off = first.off + i*first.size;
        f[at++].size = first.size;
    }
    return at;
}

/* are the words after call k of n_calls asked for? */
static bool wanted(const int32_t want[], int k, int n_calls)
{
    return (want)  ?  (want[k] != 0)  :  (k == n_calls - 1);
}

/* ---- G.726 -------------------------------------------------------------------------------------------------------------- */

static int g726_fields(field_t f[G726_WORDS])
{
    int at = 0;

    f[at++] = (field_t) FIELD(g726_state_t, yl);
    f[at++] = (field_t) FIELD(g726_state_t, yu);
    f[at++] = (field_t) FIELD(g726_state_t, dms);
    f[at++] = (field_t) FIELD(g726_state_t, dml);
    f[at++] = (field_t) FIELD(g726_state_t, ap);
    at = field_run(f, at, (field_t) FIELD(g726_state_t, a[0]), 2);
    at = field_run(f, at, (field_t) FIELD(g726_state_t, b[0]), 6);
    at = field_run(f, at, (field_t) FIELD(g726_state_t, pk[0]), 2);
    at = field_run(f, at, (field_t) FIELD(g726_state_t, dq[0]), 6);
    at = field_run(f, at, (field_t) FIELD(g726_state_t, sr[0]), 2);
    f[at++] = (field_t) FIELD(g726_state_t, td);
    f[at++] = (field_t) FIELD(g726_state_t, bs.bitstream);
    f[at++] = (field_t) FIELD(g726_state_t, bs.residue);
    f[at++] = (field_t) FIELD(g726_state_t, rate);
    f[at++] = (field_t) FIELD(g726_state_t, ext_coding);
    f[at++] = (field_t) FIELD(g726_state_t, bits_per_sample);
    f[at++] = (field_t) FIELD(g726_state_t, packing);
    return at;
}

GLUE int glue_g726_words(const void *s, int32_t w[G726_WORDS])
{
    field_t f[G726_WORDS];
    const int n = g726_fields(f);

    fields_words(s, f, n, w);
    return n;
}

/* kind 0: encode (`in` is int16_t samples where coding is linear, G.711 bytes where it is not; `out` is bytes), kind 1:
   decode (`in` is bytes; `out` is int16_t samples or G.711 bytes) */
GLUE int glue_g726_run(int kind, int rate, int coding, int packing, const void *in, const int32_t lens[], int n_calls,
                       void *out, int32_t counts[], int32_t words[], const int32_t want[])
{
    g726_state_t *s;
    const int el = (coding == G726_ENCODING_LINEAR)  ?  2  :  1;
    const uint8_t *src = (const uint8_t *) in;
    uint8_t *dst = (uint8_t *) out;
    int total = 0;
    int k;
    int n;

    if ((s = g726_init(NULL, rate, coding, packing)) == NULL)
        return -1;
    for (k = 0;  k < n_calls;  k++)
    {
        n = 0;
        if (lens[k] > 0)
        {
            if (kind == 0)
            {
                n = g726_encode(s, dst + total, (const int16_t *) src, lens[k]);
                src += (size_t) lens[k]*el;
            }
            else
            {
                n = g726_decode(s, (int16_t *) (dst + (size_t) total*el), src, lens[k]);
                src += lens[k];
            }
        }
        counts[k] = n;
        total += n;
        if (wanted(want, k, n_calls))
        {
            glue_g726_words(s, words);
            words += G726_WORDS;
        }
    }
    g726_free(s);
    return total;
}

/* ---- G.722 -------------------------------------------------------------------------------------------------------------- */

#define G722_FIELDS(type, io_buffer, io_bits)                                                           \
    do                                                                                                  \
    {                                                                                                   \
        int b_;                                                                                         \
        f[at++] = (field_t) FIELD(type, packed);                                                        \
        f[at++] = (field_t) FIELD(type, eight_k);                                                       \
        f[at++] = (field_t) FIELD(type, bits_per_sample);                                               \
        at = field_run(f, at, (field_t) FIELD(type, x[0]), 12);                                         \
        at = field_run(f, at, (field_t) FIELD(type, y[0]), 12);                                         \
        f[at++] = (field_t) FIELD(type, ptr);                                                           \
        for (b_ = 0;  b_ < 2;  b_++)                                                                    \
        {                                                                                               \
            const int32_t base_ = (int32_t) (offsetof(type, band) + b_*sizeof(g722_band_t));            \
            const int from_ = at;                                                                       \
            f[at++] = (field_t) FIELD(g722_band_t, nb);                                                 \
            f[at++] = (field_t) FIELD(g722_band_t, det);                                                \
            f[at++] = (field_t) FIELD(g722_band_t, s);                                                  \
            f[at++] = (field_t) FIELD(g722_band_t, sz);                                                 \
            f[at++] = (field_t) FIELD(g722_band_t, r);                                                  \
            at = field_run(f, at, (field_t) FIELD(g722_band_t, p[0]), 2);                               \
            at = field_run(f, at, (field_t) FIELD(g722_band_t, a[0]), 2);                               \
            at = field_run(f, at, (field_t) FIELD(g722_band_t, b[0]), 6);                               \
            at = field_run(f, at, (field_t) FIELD(g722_band_t, d[0]), 7);                               \
            for (int i_ = from_;  i_ < at;  i_++)                                                       \
                f[i_].off += base_;                                                                     \
        }                                                                                               \
        f[at++] = (field_t) FIELD(type, io_buffer);                                                     \
        f[at++] = (field_t) FIELD(type, io_bits);                                                       \
    }                                                                                                   \
    while (0)

/* kind 0: a g722_encode_state_t, kind 1: a g722_decode_state_t */
GLUE int glue_g722_words(int kind, const void *s, int32_t w[G722_WORDS])
{
    field_t f[G722_WORDS];
    int at = 0;

    if (kind == 0)
        G722_FIELDS(g722_encode_state_t, out_buffer, out_bits);
    else
        G722_FIELDS(g722_decode_state_t, in_buffer, in_bits);
    fields_words(s, f, at, w);
    return at;
}

/* kind 0: encode (int16_t samples in, bytes out), kind 1: decode (bytes in, int16_t samples out) */
GLUE int glue_g722_run(int kind, int rate, int options, const void *in, const int32_t lens[], int n_calls,
                       void *out, int32_t counts[], int32_t words[], const int32_t want[])
{
    g722_encode_state_t *e = NULL;
    g722_decode_state_t *d = NULL;
    const int16_t *amp = (const int16_t *) in;
    const uint8_t *codes = (const uint8_t *) in;
    int total = 0;
    int k;
    int n;

    if (kind == 0)
        e = g722_encode_init(NULL, rate, options);
    else
        d = g722_decode_init(NULL, rate, options);
    if (e == NULL  &&  d == NULL)
        return -1;
    for (k = 0;  k < n_calls;  k++)
    {
        n = 0;
        if (lens[k] > 0)
        {
            if (kind == 0)
            {
                n = g722_encode(e, (uint8_t *) out + total, amp, lens[k]);
                amp += lens[k];
            }
            else
            {
                n = g722_decode(d, (int16_t *) out + total, codes, lens[k]);
                codes += lens[k];
            }
        }
        counts[k] = n;
        total += n;
        if (wanted(want, k, n_calls))
        {
            glue_g722_words(kind, (kind == 0)  ?  (const void *) e  :  (const void *) d, words);
            words += G722_WORDS;
        }
    }
    if (kind == 0)
        g722_encode_free(e);
    else
        g722_decode_free(d);
    return total;
}

/* ---- GSM 06.10 ---------------------------------------------------------------------------------------------------------- */

GLUE int glue_gsm0610_words(const void *s, int32_t w[GSM0610_WORDS])
{
    field_t f[GSM0610_WORDS];
    int at = 0;

    f[at++] = (field_t) FIELD(gsm0610_state_t, packing);
    at = field_run(f, at, (field_t) FIELD(gsm0610_state_t, dp0[0]), 120);
    f[at++] = (field_t) FIELD(gsm0610_state_t, z1);
    f[at++] = (field_t) FIELD(gsm0610_state_t, L_z2);
    f[at++] = (field_t) FIELD(gsm0610_state_t, mp);
    at = field_run(f, at, (field_t) FIELD(gsm0610_state_t, u[0]), 8);
    at = field_run(f, at, (field_t) FIELD(gsm0610_state_t, LARpp[0][0]), 16);
    f[at++] = (field_t) FIELD(gsm0610_state_t, j);
    f[at++] = (field_t) FIELD(gsm0610_state_t, nrp);
    at = field_run(f, at, (field_t) FIELD(gsm0610_state_t, v[0]), 9);
    f[at++] = (field_t) FIELD(gsm0610_state_t, msr);
    fields_words(s, f, at, w);
    return at;
}

/* kind 0: encode (int16_t samples in, whole frames; bytes out), kind 1: decode (bytes in, whole units; samples out) */
GLUE int glue_gsm0610_run(int kind, int packing, const void *in, const int32_t lens[], int n_calls,
                          void *out, int32_t counts[], int32_t words[], const int32_t want[])
{
    gsm0610_state_t *s;
    const int16_t *amp = (const int16_t *) in;
    const uint8_t *codes = (const uint8_t *) in;
    int total = 0;
    int k;
    int n;

    if ((s = gsm0610_init(NULL, packing)) == NULL)
        return -1;
    for (k = 0;  k < n_calls;  k++)
    {
        n = 0;
        if (lens[k] > 0)
        {
            if (kind == 0)
            {
                n = gsm0610_encode(s, (uint8_t *) out + total, amp, lens[k]);
                amp += lens[k];
            }
            else
            {
                n = gsm0610_decode(s, (int16_t *) out + total, codes, lens[k]);
                codes += lens[k];
            }
        }
        counts[k] = n;
        total += n;
        if (wanted(want, k, n_calls))
        {
            glue_gsm0610_words(s, words);
            words += GSM0610_WORDS;
        }
    }
    gsm0610_free(s);
    return total;
}

/* ---- packet loss concealment -------------------------------------------------------------------------------------------- */

GLUE int glue_plc_words(const void *s, int32_t w[PLC_WORDS])
{
    field_t f[PLC_WORDS];
    int at = 0;

    f[at++] = (field_t) FIELD(plc_state_t, missing_samples);
    f[at++] = (field_t) FIELD(plc_state_t, pitch_offset);
    f[at++] = (field_t) FIELD(plc_state_t, pitch);
    at = field_run(f, at, (field_t) FIELD(plc_state_t, pitchbuf[0]), PLC_PITCH_MIN);
    at = field_run(f, at, (field_t) FIELD(plc_state_t, history[0]), PLC_HISTORY_LEN);
    f[at++] = (field_t) FIELD(plc_state_t, buf_ptr);
    fields_words(s, f, at, w);
    return at;
}

/* The rows of the calls lie one behind the other in `amp` and are worked on in place: call k is plc_fillin() where lost[k],
   plc_rx() where not.  Returns the samples gone through. */
GLUE int glue_plc_run(int16_t amp[], const int32_t lens[], const int32_t lost[], int n_calls, int32_t words[], const int32_t want[])
{
    plc_state_t *s;
    int total = 0;
    int k;

    if ((s = plc_init(NULL)) == NULL)
        return -1;
    for (k = 0;  k < n_calls;  k++)
    {
        if (lens[k] > 0)
        {
            if (lost[k])
                plc_fillin(s, amp + total, lens[k]);
            else
                plc_rx(s, amp + total, lens[k]);
            total += lens[k];
        }
        if (wanted(want, k, n_calls))
        {
            glue_plc_words(s, words);
            words += PLC_WORDS;
        }
    }
    plc_free(s);
    return total;
}

/* A VoIP decoder in front of a concealer, tick by tick: a tick that is not lost decodes the next 33 bytes of `codes` into the
   tick's 160 samples of `amp` and hears them (plc_rx); a lost one fills them in (plc_fillin).  Returns the frames decoded. */
GLUE int glue_gsm_plc_run(const uint8_t codes[], const int32_t lost[], int n_ticks, int16_t amp[],
                          int32_t dec_words[], int32_t plc_words[], const int32_t want[])
{
    gsm0610_state_t *d;
    plc_state_t *s;
    int frames = 0;
    int k;

    if ((d = gsm0610_init(NULL, GSM0610_PACKING_VOIP)) == NULL)
        return -1;
    if ((s = plc_init(NULL)) == NULL)
    {
        gsm0610_free(d);
        return -1;
    }
    for (k = 0;  k < n_ticks;  k++)
    {
        int16_t *row = amp + (size_t) k*GSM_FRAME;

        if (lost[k])
        {
            plc_fillin(s, row, GSM_FRAME);
        }
        else
        {
            gsm0610_decode(d, row, codes + (size_t) 33*frames++, 33);
            plc_rx(s, row, GSM_FRAME);
        }
        if (wanted(want, k, n_ticks))
        {
            glue_gsm0610_words(d, dec_words);
            glue_plc_words(s, plc_words);
            dec_words += GSM0610_WORDS;
            plc_words += PLC_WORDS;
        }
    }
    plc_free(s);
    gsm0610_free(d);
    return frames;
}

/* ---- the objects themselves, for a caller that steps them (the stand-alone sweep program) -------------------------------- */

GLUE int glue_codecs_state_words(int family)
{
    static const int n[4] = {G726_WORDS, G722_WORDS, GSM0610_WORDS, PLC_WORDS};

    return (family >= 0  &&  family < 4)  ?  n[family]  :  -1;
}
