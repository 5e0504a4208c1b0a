/* The lone spandsp-named objects over a stand-in bank (tests/lone_bank_stub.c): every object's life, a failed init into the
 * caller's storage, the piece boundaries of every call that cuts its work into launches, the senders falling short, and the
 * bit pullers at SIG_STATUS_END_OF_DATA.  The stub prints each bank call, this program prints each return value with a
 * checksum of what the caller's buffer got and whether the bytes behind that are as the caller had them; the transcript is
 * compared with tests/golden/lone_objects.txt (tests/test_lone_objects.py).  No struct field is touched here. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu_spandsp.h"

extern int stub_fail_create;
extern int stub_short_tx;
extern int stub_short_got;
extern int stub_live;

#define OUT_BYTES   (256*1024)
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

/* ---- an object's life ---------------------------------------------------------------------------------------- */
#define LIFE(T, pfx, INIT, can_fail)                                                                                    \
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
    if (can_fail)                                                                                                       \
    {                                                                                                                   \
        memset(&st, 0xA5, sizeof(st));                                                                                  \
        stub_fail_create = 1;                                                                                           \
        s = INIT(&st);                                                                                                  \
        printf("failed init(&st) -> %s\n", s  ?  "an object"  :  "NULL");                                               \
        printf(#pfx ": storage %s after failed init\n", all_of(&st, sizeof(st), 0xA5)  ?  "unchanged"  :  "changed");   \
        stub_fail_create = 1;                                                                                           \
        s = INIT(NULL);                                                                                                 \
        printf("failed init(NULL) -> %s\n", s  ?  "an object"  :  "NULL");                                              \
    }                                                                                                                   \
    stub_fail_create = 0;                                                                                               \
    printf("live banks: %d\n", stub_live);                                                                              \
}                                                                                                                       \
while (0)

/* ---- callbacks ------------------------------------------------------------------------------------------------- */
static int bits_asked;
static int bits_before_end;     /* < 0: the data never ends */
static int loud;

static int get_bit(void *user_data)
{
    const int k = bits_asked++;

    (void) user_data;
    if (bits_before_end >= 0  &&  k >= bits_before_end)
    {
        if (loud)
            printf("  get_bit -> end of data\n");
        return SIG_STATUS_END_OF_DATA;
    }
    if (loud)
        printf("  get_bit -> %d\n", (k*5 >> 2) & 1);
    return (k*5 >> 2) & 1;
}

static void status(void *user_data, int status)
{
    (void) user_data;
    printf("  status %d\n", status);
}

static void put_msg(void *user_data, const uint8_t *msg, int len)
{
    (void) user_data;
    printf("  put_msg(len %d, sum %08x)\n", len, fnv(msg, (size_t) len));
}

static int get_byte(void *user_data)
{
    (void) user_data;
    return 0x55;
}

static const int pieces[6][2] = { {0, 0}, {0, 1}, {1, -1}, {1, 0}, {1, 1}, {2, 3} };   /* k*PIECE + d */

/* ---- the codecs ------------------------------------------------------------------------------------------------ */
#define ENCODE(what, call, s, len, in_el)                                                                               \
do                                                                                                                      \
{                                                                                                                       \
    void *in = input((size_t) (len)*(in_el));                                                                           \
                                                                                                                        \
    memset(out, FILL, OUT_BYTES);                                                                                       \
    report(what, len, call(s, out, (const int16_t *) in, len), 1);                                                      \
    free(in);                                                                                                           \
}                                                                                                                       \
while (0)

#define DECODE(what, call, s, len, out_el)                                                                              \
do                                                                                                                      \
{                                                                                                                       \
    void *in = input((size_t) (len));                                                                                   \
                                                                                                                        \
    memset(out, FILL, OUT_BYTES);                                                                                       \
    report(what, len, call(s, (int16_t *) out, (const uint8_t *) in, len), out_el);                                     \
    free(in);                                                                                                           \
}                                                                                                                       \
while (0)

#define G726_INIT(s)        g726_init(s, 32000, G726_ENCODING_LINEAR, G726_PACKING_LEFT)
#define G722_ENC_INIT(s)    g722_encode_init(s, 64000, 0)
#define G722_DEC_INIT(s)    g722_decode_init(s, 64000, 0)
#define GSM_INIT(s)         gsm0610_init(s, GSM0610_PACKING_NONE)

static void g726(void)
{
    static const int codings[2] = { G726_ENCODING_LINEAR, G726_ENCODING_ULAW };
    g726_state_t *s;
    int c;
    int i;

    LIFE(g726_state_t, g726, G726_INIT, 1);
    for (c = 0;  c < 2;  c++)
    {
        printf("== g726: pieces, coding %d\n", codings[c]);
        s = g726_init(NULL, 32000, codings[c], G726_PACKING_LEFT);
        for (i = 0;  i < 6;  i++)
            ENCODE("g726_encode", g726_encode, s, pieces[i][0]*4096 + pieces[i][1], (c == 0)  ?  2  :  1);
        for (i = 0;  i < 6;  i++)
            DECODE("g726_decode", g726_decode, s, pieces[i][0]*4096 + pieces[i][1], (c == 0)  ?  2  :  1);
        g726_free(s);
    }
    printf("g726_encode(NULL) -> %d\n", g726_encode(NULL, out, (const int16_t *) out, 8));
    printf("g726_decode(NULL) -> %d\n", g726_decode(NULL, (int16_t *) out, out, 8));
}

static void g722(void)
{
    g722_encode_state_t *e;
    g722_decode_state_t *d;
    int i;

    LIFE(g722_encode_state_t, g722_encode, G722_ENC_INIT, 1);
    LIFE(g722_decode_state_t, g722_decode, G722_DEC_INIT, 1);
    printf("== g722: pieces, 16 kHz\n");
    e = g722_encode_init(NULL, 64000, 0);
    d = g722_decode_init(NULL, 64000, 0);
    for (i = 0;  i < 6;  i++)
        ENCODE("g722_encode", g722_encode, e, pieces[i][0]*4096 + pieces[i][1], 2);
    ENCODE("g722_encode", g722_encode, e, 7, 2);
    for (i = 0;  i < 6;  i++)
        DECODE("g722_decode", g722_decode, d, pieces[i][0]*4096 + pieces[i][1], 2);
    g722_encode_free(e);
    g722_decode_free(d);
    printf("== g722: 8 kHz, 56000\n");
    e = g722_encode_init(NULL, 56000, G722_SAMPLE_RATE_8000 | G722_PACKED);
    d = g722_decode_init(NULL, 56000, G722_SAMPLE_RATE_8000 | G722_PACKED);
    ENCODE("g722_encode", g722_encode, e, 7, 2);
    ENCODE("g722_encode", g722_encode, e, 4097, 2);
    DECODE("g722_decode", g722_decode, d, 4097, 2);
    g722_encode_free(e);
    g722_decode_free(d);
    printf("g722_encode(NULL) -> %d\n", g722_encode(NULL, out, (const int16_t *) out, 8));
    printf("g722_decode(NULL) -> %d\n", g722_decode(NULL, (int16_t *) out, out, 8));
}

static void gsm0610(void)
{
    static const int packings[3] = { GSM0610_PACKING_NONE, GSM0610_PACKING_WAV49, GSM0610_PACKING_VOIP };
    static const int unit_samples[3] = { 160, 320, 160 };
    static const int unit_bytes[3] = { 76, 65, 33 };
    gsm0610_state_t st;
    gsm0610_state_t *s;
    int i;

    LIFE(gsm0610_state_t, gsm0610, GSM_INIT, 1);
    printf("== gsm0610: the second bank fails\n");
    memset(&st, 0xA5, sizeof(st));
    stub_fail_create = 2;
    s = gsm0610_init(&st, GSM0610_PACKING_VOIP);
    printf("failed init(&st) -> %s\n", s  ?  "an object"  :  "NULL");
    printf("gsm0610: storage %s after failed second create\n", all_of(&st, sizeof(st), 0xA5)  ?  "unchanged"  :  "changed");
    stub_fail_create = 2;
    s = gsm0610_init(NULL, GSM0610_PACKING_VOIP);
    printf("failed init(NULL) -> %s\n", s  ?  "an object"  :  "NULL");
    stub_fail_create = 0;
    printf("live banks: %d\n", stub_live);

    printf("== gsm0610: pieces, unpacked\n");
    s = gsm0610_init(NULL, GSM0610_PACKING_NONE);
    for (i = 0;  i < 6;  i++)
        ENCODE("gsm0610_encode", gsm0610_encode, s, (pieces[i][0]*32 + pieces[i][1])*160, 2);
    for (i = 0;  i < 6;  i++)
        DECODE("gsm0610_decode", gsm0610_decode, s, (pieces[i][0]*32 + pieces[i][1])*76, 2);
    for (i = 0;  i < 3;  i++)
    {
        printf("== gsm0610: packing %d, 32 units + 1 unit + a partial unit\n", packings[i]);
        printf("set_packing -> %d\n", gsm0610_set_packing(s, packings[i]));
        ENCODE("gsm0610_encode", gsm0610_encode, s, 33*unit_samples[i] + unit_samples[i]/2, 2);
        DECODE("gsm0610_decode", gsm0610_decode, s, 33*unit_bytes[i] + unit_bytes[i]/2, 2);
        ENCODE("gsm0610_encode", gsm0610_encode, s, unit_samples[i] - 1, 2);
        DECODE("gsm0610_decode", gsm0610_decode, s, unit_bytes[i] - 1, 2);
    }
    printf("set_packing(99) -> %d\n", gsm0610_set_packing(s, 99));
    gsm0610_free(s);
    printf("gsm0610_encode(NULL) -> %d\n", gsm0610_encode(NULL, out, (const int16_t *) out, 160));
    printf("gsm0610_decode(NULL) -> %d\n", gsm0610_decode(NULL, (int16_t *) out, out, 76));
    printf("set_packing(NULL) -> %d\n", gsm0610_set_packing(NULL, GSM0610_PACKING_NONE));
}

/* ---- the senders ----------------------------------------------------------------------------------------------- */
/* amp[] has exactly `len` samples, on the heap */
#define SEND(what, call, s, len)                                                                                        \
do                                                                                                                      \
{                                                                                                                       \
    const size_t bytes = (size_t) (((len) > 0)  ?  (len)  :  0)*2;                                                      \
    uint8_t *amp = (uint8_t *) input(bytes);                                                                            \
    int ret;                                                                                                            \
                                                                                                                        \
    memset(amp, FILL, bytes);                                                                                           \
    bits_asked = 0;                                                                                                     \
    ret = call(s, (int16_t *) amp, len);                                                                                \
    printf("%s(%d) -> %d, sum %08x, behind it %s, get_bit x %d\n", what, len, ret, fnv(amp, (ret > 0)  ?  (size_t) ret*2  :  0),   \
           all_of(amp + ((ret > 0)  ?  ret*2  :  0), bytes - ((ret > 0)  ?  (size_t) ret*2  :  0), FILL)  ?  "untouched"  :  "WRITTEN", bits_asked);   \
    free(amp);                                                                                                          \
}                                                                                                                       \
while (0)

#define V18_INIT(s)         v18_init(s, true, V18_MODE_WEITBRECHT_5BIT_4545, V18_AUTOMODING_NONE, put_msg, NULL, status, NULL)
#define ADSI_TX_INIT(s)     adsi_tx_init(s, ADSI_STANDARD_CLASS)
#define ADSI_RX_INIT(s)     adsi_rx_init(s, ADSI_STANDARD_CLASS, put_msg, NULL)

static void v18(void)
{
    v18_state_t st;
    v18_state_t *s;
    int16_t *amp;
    int i;

    LIFE(v18_state_t, v18, V18_INIT, 1);
    memset(&st, 0xA5, sizeof(st));
    printf("init(&st, a mode with no bank) -> %s\n", v18_init(&st, true, V18_MODE_DTMF, V18_AUTOMODING_NONE, put_msg, NULL, status, NULL)  ?  "an object"  :  "NULL");
    printf("v18: storage %s after refused init\n", all_of(&st, sizeof(st), 0xA5)  ?  "unchanged"  :  "changed");
    printf("== v18: pieces\n");
    s = V18_INIT(NULL);
    for (i = 0;  i < 6;  i++)
        SEND("v18_tx", v18_tx, s, pieces[i][0]*4096 + pieces[i][1]);
    printf("== v18: the second piece falls short\n");
    stub_short_tx = 2;
    stub_short_got = 100;
    SEND("v18_tx", v18_tx, s, 3*4096);
    stub_short_tx = 1;
    stub_short_got = 0;
    SEND("v18_tx", v18_tx, s, 64);
    stub_short_tx = 0;
    printf("== v18: the rest\n");
    amp = (int16_t *) input(2*4100);
    printf("v18_rx -> %d\n", v18_rx(s, amp, 4100));
    free(amp);
    printf("v18_rx_fillin -> %d\n", v18_rx_fillin(s, 80));
    printf("v18_put -> %d\n", v18_put(s, "hello", -1));
    printf("v18_put -> %d\n", v18_put(s, "", -1));
    printf("mode %d\n", v18_get_current_mode(s));
    v18_free(s);
    SEND("v18_tx(NULL)", v18_tx, NULL, 64);
}

static void adsi(void)
{
    static const uint8_t msg[4] = { 0x80, 0x02, 0x01, 0x02 };
    adsi_tx_state_t *t;
    adsi_rx_state_t *r;
    int16_t *amp;
    int i;

    LIFE(adsi_tx_state_t, adsi_tx, ADSI_TX_INIT, 1);
    LIFE(adsi_rx_state_t, adsi_rx, ADSI_RX_INIT, 1);
    printf("== adsi_tx: pieces\n");
    t = ADSI_TX_INIT(NULL);
    printf("put_message -> %d\n", adsi_tx_put_message(t, msg, 4));
    adsi_tx_set_preamble(t, 10, -1, -1, 1);
    adsi_tx_send_alert_tone(t);
    for (i = 0;  i < 6;  i++)
        SEND("adsi_tx", adsi_tx, t, pieces[i][0]*4096 + pieces[i][1]);
    printf("== adsi_tx: the second piece falls short\n");
    stub_short_tx = 2;
    stub_short_got = 100;
    SEND("adsi_tx", adsi_tx, t, 3*4096);
    stub_short_tx = 0;
    adsi_tx_free(t);
    SEND("adsi_tx(NULL)", adsi_tx, NULL, 64);
    printf("== adsi_rx\n");
    r = ADSI_RX_INIT(NULL);
    amp = (int16_t *) input(2*4100);
    printf("adsi_rx -> %d\n", adsi_rx(r, amp, 4100));
    free(amp);
    adsi_rx_free(r);
    printf("init(a standard with no bank) -> %s\n", adsi_tx_init(NULL, ADSI_STANDARD_NONE)  ?  "an object"  :  "NULL");
}

#define FSK_TX_INIT(s)      fsk_tx_init(s, &preset_fsk_specs[FSK_V21CH1], get_bit, NULL)
#define MCT_TX_INIT(s)      modem_connect_tones_tx_init(s, MODEM_CONNECT_TONES_ANS)
#define ASYNC_TX_INIT(s)    async_tx_init(s, 8, 0, 1, false, get_byte, NULL)

static void fsk_senders(void)
{
    fsk_tx_state_t *s;
    modem_connect_tones_tx_state_t *m;
    async_tx_state_t *a;
    int i;

    bits_before_end = -1;
    loud = 0;
    LIFE(fsk_tx_state_t, fsk_tx, FSK_TX_INIT, 1);
    LIFE(modem_connect_tones_tx_state_t, modem_connect_tones_tx, MCT_TX_INIT, 1);
    LIFE(async_tx_state_t, async_tx, ASYNC_TX_INIT, 0);
    printf("fsk_tx_init(no spec) -> %s\n", fsk_tx_init(NULL, NULL, get_bit, NULL)  ?  "an object"  :  "NULL");
    printf("== fsk_tx: pieces\n");
    s = FSK_TX_INIT(NULL);
    fsk_tx_set_modem_status_handler(s, status, NULL);
    for (i = 0;  i < 6;  i++)
        SEND("fsk_tx", fsk_tx, s, pieces[i][0]*8192 + pieces[i][1]);
    printf("== fsk_tx: the data ends after 5 bits\n");
    loud = 1;
    bits_before_end = 5;
    SEND("fsk_tx", fsk_tx, s, 400);
    SEND("fsk_tx", fsk_tx, s, 400);
    printf("restart -> %d\n", fsk_tx_restart(s, &preset_fsk_specs[FSK_V21CH2]));
    bits_before_end = 0;
    SEND("fsk_tx", fsk_tx, s, 8192 + 400);
    loud = 0;
    bits_before_end = -1;
    fsk_tx_free(s);
    SEND("fsk_tx(NULL)", fsk_tx, NULL, 64);
    printf("== fsk_tx: fed by async_tx\n");
    a = ASYNC_TX_INIT(NULL);
    async_tx_presend_bits(a, 3);
    s = fsk_tx_init(NULL, &preset_fsk_specs[FSK_V21CH1], async_tx_get_bit, a);
    SEND("fsk_tx", fsk_tx, s, 800);
    fsk_tx_free(s);
    async_tx_free(a);
    printf("== modem_connect_tones_tx\n");
    m = MCT_TX_INIT(NULL);
    SEND("modem_connect_tones_tx", modem_connect_tones_tx, m, 0);
    SEND("modem_connect_tones_tx", modem_connect_tones_tx, m, 10000);
    stub_short_tx = 1;
    stub_short_got = 17;
    SEND("modem_connect_tones_tx", modem_connect_tones_tx, m, 500);
    stub_short_tx = 0;
    modem_connect_tones_tx_free(m);
}

#define V29_INIT(s)         v29_tx_init(s, 9600, false, get_bit, NULL)
#define V27TER_INIT(s)      v27ter_tx_init(s, 4800, true, get_bit, NULL)
#define V17_INIT(s)         v17_tx_init(s, 14400, false, get_bit, NULL)

static void modem_senders(void)
{
    v29_tx_state_t st;
    v29_tx_state_t *s;
    v27ter_tx_state_t *s27;
    v17_tx_state_t *s17;
    int i;

    bits_before_end = -1;
    loud = 0;
    LIFE(v29_tx_state_t, v29_tx, V29_INIT, 1);
    LIFE(v27ter_tx_state_t, v27ter_tx, V27TER_INIT, 1);
    LIFE(v17_tx_state_t, v17_tx, V17_INIT, 1);
    memset(&st, 0xA5, sizeof(st));
    printf("init(&st, a bad bit rate) -> %s\n", v29_tx_init(&st, 1234, false, get_bit, NULL)  ?  "an object"  :  "NULL");
    printf("v29_tx: storage %s after refused init\n", all_of(&st, sizeof(st), 0xA5)  ?  "unchanged"  :  "changed");
    printf("== v29_tx: pieces\n");
    s = V29_INIT(NULL);
    v29_tx_set_modem_status_handler(s, status, NULL);
    v29_tx_power(s, -12.0f);
    for (i = 0;  i < 6;  i++)
        SEND("v29_tx", v29_tx, s, pieces[i][0]*4096 + pieces[i][1]);
    printf("== v29_tx: the second piece falls short\n");
    stub_short_tx = 2;
    stub_short_got = 100;
    SEND("v29_tx", v29_tx, s, 3*4096);
    stub_short_tx = 0;
    printf("== v29_tx: the data ends after 7 bits\n");
    loud = 1;
    bits_before_end = 7;
    SEND("v29_tx", v29_tx, s, 50);
    bits_before_end = 0;
    SEND("v29_tx", v29_tx, s, 50);
    printf("restart -> %d\n", v29_tx_restart(s, 7200, false));
    printf("restart(a bad bit rate) -> %d\n", v29_tx_restart(s, 1234, false));
    bits_before_end = 3;
    SEND("v29_tx", v29_tx, s, 4096 + 50);
    loud = 0;
    bits_before_end = -1;
    v29_tx_free(s);
    SEND("v29_tx(NULL)", v29_tx, NULL, 64);
    printf("== v27ter_tx, v17_tx\n");
    s27 = V27TER_INIT(NULL);
    SEND("v27ter_tx", v27ter_tx, s27, 4097);
    v27ter_tx_free(s27);
    s17 = V17_INIT(NULL);
    SEND("v17_tx", v17_tx, s17, 4097);
    printf("restart -> %d\n", v17_tx_restart(s17, 9600, true, true));
    v17_tx_free(s17);
}

#define DTMF_INIT(s)        dtmf_tx_init(s, NULL, NULL)
#define BELL_MF_INIT(s)     bell_mf_tx_init(s)
#define R2_MF_INIT(s)       r2_mf_tx_init(s, true)

static void digit_senders(void)
{
    dtmf_tx_state_t *d;
    bell_mf_tx_state_t *b;
    r2_mf_tx_state_t *r;

    LIFE(dtmf_tx_state_t, dtmf_tx, DTMF_INIT, 1);
    LIFE(bell_mf_tx_state_t, bell_mf_tx, BELL_MF_INIT, 1);
    LIFE(r2_mf_tx_state_t, r2_mf_tx, R2_MF_INIT, 1);
    printf("== digit senders\n");
    d = DTMF_INIT(NULL);
    printf("dtmf_tx_put -> %d\n", dtmf_tx_put(d, "123", -1));
    SEND("dtmf_tx", dtmf_tx, d, 1000);
    dtmf_tx_free(d);
    b = BELL_MF_INIT(NULL);
    printf("bell_mf_tx_put -> %d\n", bell_mf_tx_put(b, "123", -1));
    SEND("bell_mf_tx", bell_mf_tx, b, 1000);
    bell_mf_tx_free(b);
    r = R2_MF_INIT(NULL);
    printf("r2_mf_tx_put -> %d\n", r2_mf_tx_put(r, '5'));
    SEND("r2_mf_tx", r2_mf_tx, r, 1000);
    r2_mf_tx_free(r);
}

int main(void)
{
    if ((out = (uint8_t *) malloc(OUT_BYTES)) == NULL)
        return 1;
    g726();
    g722();
    gsm0610();
    v18();
    adsi();
    fsk_senders();
    modem_senders();
    digit_senders();
    free(out);
    printf("live banks at the end: %d\n", stub_live);
    return 0;
}
