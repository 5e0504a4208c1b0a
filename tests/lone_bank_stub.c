/* A stand-in for the one-channel banks behind the lone spandsp-named objects (csrc/shim_g726.c, shim_g722.c, shim_gsm0610.c,
 * shim_v18.c, shim_adsi.c, shim_fsktx.c, shim_modemtx.c and the digit senders of shim_fsk.c), for the host-side transcript test
 * tests/test_lone_objects.py: the shims + this file + tests/c_callers/lone_objects.c under -fsanitize=address,undefined; no GPU.
 * It keeps no signal state.  Every call prints itself with its scalar arguments, touches exactly the memory the real bank
 * touches (a whole row of the stride it is given), and answers with something trivial and deterministic: a codec counts what
 * the real rule would and fills its row from a sum of its input, a sender makes a ramp with zeros behind it.  The driver
 * sets stub_fail_create to make the k-th create from now fail, and stub_short_tx / stub_short_got to make the k-th sender
 * launch from now fall short.  The group receivers of shim_fsk.c are never reached: their banks abort().  Test code only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu.h"

int stub_fail_create = 0;
int stub_short_tx = 0;
int stub_short_got = 0;
int stub_live = 0;              /* banks created and not yet destroyed */

typedef struct
{
    int id;
    int a;                      /* g726: bits; g722: direction; gsm0610: packing */
    int b;                      /* g726: coding; g722: 8 kHz samples */
    int c;                      /* g726: packing */
    int ended;
    int shutdown;
    int sent;                   /* where a sender's ramp is */
    int32_t ev_channel;
    int32_t ev_kind;
    int n_ev;
} bank_t;

struct spangpu_g726_s { bank_t k; };
struct spangpu_g722_s { bank_t k; };
struct spangpu_gsm0610_s { bank_t k; };
struct spangpu_v18_s { bank_t k; };
struct spangpu_adsi_tx_s { bank_t k; };
struct spangpu_adsi_rx_s { bank_t k; };
struct spangpu_fsktx_s { bank_t k; };
struct spangpu_mcttx_s { bank_t k; };
struct spangpu_modemtx_s { bank_t k; };
struct spangpu_txbank_s { bank_t k; };

static int next_id = 0;

static void *make(const char *what)
{
    bank_t *k;

    if (stub_fail_create > 0  &&  --stub_fail_create == 0)
    {
        printf("  bank: %s fails\n", what);
        return NULL;
    }
    if ((k = (bank_t *) calloc(1, sizeof(*k))) == NULL)
        abort();
    k->id = ++next_id;
    stub_live++;
    printf("  bank: %s -> #%d\n", what, k->id);
    return k;
}

static void unmake(const char *what, void *bank)
{
    printf("  bank: %s(#%d)\n", what, ((bank_t *) bank)->id);
    stub_live--;
    free(bank);
}

static unsigned sum_of(const void *p, long long bytes)
{
    const uint8_t *b = (const uint8_t *) p;
    unsigned s = 0;
    long long i;

    for (i = 0;  i < bytes;  i++)
        s = s*31 + b[i];
    return s;
}

/* a codec's row: the whole stride, from a sum of the whole input row */
static void code_row(void *out, long long out_bytes, const void *in, long long in_bytes)
{
    const unsigned s = sum_of(in, in_bytes);
    long long i;

    for (i = 0;  i < out_bytes;  i++)
        ((uint8_t *) out)[i] = (uint8_t) (s + 7*i + 1);
}

/* a sender's row: a ramp, zeros behind what it made */
static int send_row(const char *what, bank_t *k, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    int got = samples;
    int i;

    if (k->shutdown)
        got = 0;
    else if (k->ended)
        got = samples/2;
    if (stub_short_tx > 0  &&  --stub_short_tx == 0)
        got = stub_short_got;
    for (i = 0;  i < samples;  i++)
        pcm[i] = (i < got)  ?  (int16_t) (k->sent + i + 1)  :  0;
    k->sent += got;
    k->n_ev = 0;
    if (k->ended  &&  !k->shutdown)
    {
        k->shutdown = 1;
        k->n_ev = 1;
    }
    if (lens)
        lens[0] = got;
    printf("  bank: %s(#%d, stride %lld, samples %d) -> %d\n", what, k->id, stride, samples, got);
    return SPANGPU_OK;
}

const char *spangpu_last_error(void) { return "stub bank"; }

/* ---- G.726 ------------------------------------------------------------------------------------------------- */
int spangpu_g726_create(spangpu_g726_t **bank, int device, int n_channels, const int32_t *rates, const int32_t *codings,
                        const int32_t *packings, int n)
{
    char what[96];

    sprintf(what, "g726_create(dev %d, ch %d, rate %d, coding %d, packing %d, n %d)", device, n_channels, (int) rates[0], (int) codings[0],
            (int) packings[0], n);
    if ((*bank = (spangpu_g726_t *) make(what)) == NULL)
        return SPANGPU_ERR_NO_DEVICE;
    (*bank)->k.a = rates[0]/8000;
    (*bank)->k.b = codings[0];
    (*bank)->k.c = packings[0];
    return SPANGPU_OK;
}

void spangpu_g726_destroy(spangpu_g726_t *bank) { unmake("g726_destroy", bank); }

long long spangpu_g726_encode_capacity(const spangpu_g726_t *bank, int samples)
{
    printf("  bank: g726_encode_capacity(#%d, %d)\n", bank->k.id, samples);
    return samples + 16;
}

long long spangpu_g726_decode_capacity(const spangpu_g726_t *bank, int bytes)
{
    printf("  bank: g726_decode_capacity(#%d, %d)\n", bank->k.id, bytes);
    return 4*(long long) bytes + 16;
}

int spangpu_g726_encode(spangpu_g726_t *bank, const void *amp, int amp_mem_kind, long long amp_stride_bytes, const int32_t *lens,
                        int max_samples, uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, int32_t *bytes_out)
{
    code_row(codes, codes_stride_bytes, amp, amp_stride_bytes);
    bytes_out[0] = (bank->k.c == SPANGPU_G726_PACKING_NONE)  ?  max_samples  :  max_samples*bank->k.a/8;
    printf("  bank: g726_encode(#%d, mem %d, in stride %lld, lens %s, samples %d, mem %d, out stride %lld) -> %d\n", bank->k.id, amp_mem_kind,
           amp_stride_bytes, lens  ?  "given"  :  "NULL", max_samples, codes_mem_kind, codes_stride_bytes, (int) bytes_out[0]);
    return SPANGPU_OK;
}

int spangpu_g726_decode(spangpu_g726_t *bank, const uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, const int32_t *lens,
                        int max_bytes, void *amp, int amp_mem_kind, long long amp_stride_bytes, int32_t *samples_out)
{
    code_row(amp, amp_stride_bytes, codes, codes_stride_bytes);
    samples_out[0] = (bank->k.c == SPANGPU_G726_PACKING_NONE)  ?  max_bytes  :  max_bytes*8/bank->k.a;
    printf("  bank: g726_decode(#%d, mem %d, in stride %lld, lens %s, bytes %d, mem %d, out stride %lld) -> %d\n", bank->k.id, codes_mem_kind,
           codes_stride_bytes, lens  ?  "given"  :  "NULL", max_bytes, amp_mem_kind, amp_stride_bytes, (int) samples_out[0]);
    return SPANGPU_OK;
}

/* ---- G.722 ------------------------------------------------------------------------------------------------- */
int spangpu_g722_create(spangpu_g722_t **bank, int device, int n_channels, int direction, const int32_t *rates, const int32_t *options, int n)
{
    char what[96];

    sprintf(what, "g722_create(dev %d, ch %d, direction %d, rate %d, options %d, n %d)", device, n_channels, direction, (int) rates[0],
            (int) options[0], n);
    if ((*bank = (spangpu_g722_t *) make(what)) == NULL)
        return SPANGPU_ERR_NO_DEVICE;
    (*bank)->k.a = direction;
    (*bank)->k.b = (options[0] & SPANGPU_G722_SAMPLE_RATE_8000) != 0;
    return SPANGPU_OK;
}

void spangpu_g722_destroy(spangpu_g722_t *bank) { unmake("g722_destroy", bank); }

long long spangpu_g722_encode_capacity(const spangpu_g722_t *bank, int samples)
{
    printf("  bank: g722_encode_capacity(#%d, %d)\n", bank->k.id, samples);
    return samples + 16;
}

long long spangpu_g722_decode_capacity(const spangpu_g722_t *bank, int bytes)
{
    printf("  bank: g722_decode_capacity(#%d, %d)\n", bank->k.id, bytes);
    return 2*(long long) bytes + 16;
}

int spangpu_g722_encode(spangpu_g722_t *bank, const void *amp, int amp_mem_kind, long long amp_stride_bytes, const int32_t *lens,
                        int max_samples, uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, int32_t *bytes_out)
{
    code_row(codes, codes_stride_bytes, amp, amp_stride_bytes);
    bytes_out[0] = bank->k.b  ?  max_samples  :  max_samples/2;
    printf("  bank: g722_encode(#%d, mem %d, in stride %lld, lens %s, samples %d, mem %d, out stride %lld) -> %d\n", bank->k.id, amp_mem_kind,
           amp_stride_bytes, lens  ?  "given"  :  "NULL", max_samples, codes_mem_kind, codes_stride_bytes, (int) bytes_out[0]);
    return SPANGPU_OK;
}

int spangpu_g722_decode(spangpu_g722_t *bank, const uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, const int32_t *lens,
                        int max_bytes, void *amp, int amp_mem_kind, long long amp_stride_bytes, int32_t *samples_out)
{
    code_row(amp, amp_stride_bytes, codes, codes_stride_bytes);
    samples_out[0] = bank->k.b  ?  max_bytes  :  2*max_bytes;
    printf("  bank: g722_decode(#%d, mem %d, in stride %lld, lens %s, bytes %d, mem %d, out stride %lld) -> %d\n", bank->k.id, codes_mem_kind,
           codes_stride_bytes, lens  ?  "given"  :  "NULL", max_bytes, amp_mem_kind, amp_stride_bytes, (int) samples_out[0]);
    return SPANGPU_OK;
}

/* ---- GSM 06.10 --------------------------------------------------------------------------------------------- */
static int gsm_unit_samples(int packing)
{
    return (packing == SPANGPU_GSM0610_PACKING_WAV49)  ?  320  :  160;
}

static int gsm_unit_bytes(int packing)
{
    return (packing == SPANGPU_GSM0610_PACKING_WAV49)  ?  65  :  ((packing == SPANGPU_GSM0610_PACKING_VOIP)  ?  33  :  76);
}

int spangpu_gsm0610_create(spangpu_gsm0610_t **bank, int device, int n_channels, int direction, const int32_t *packings, int n)
{
    char what[96];

    sprintf(what, "gsm0610_create(dev %d, ch %d, direction %d, packing %d, n %d)", device, n_channels, direction, (int) packings[0], n);
    if ((*bank = (spangpu_gsm0610_t *) make(what)) == NULL)
        return SPANGPU_ERR_NO_DEVICE;
    (*bank)->k.a = packings[0];
    return SPANGPU_OK;
}

void spangpu_gsm0610_destroy(spangpu_gsm0610_t *bank) { unmake("gsm0610_destroy", bank); }

int spangpu_gsm0610_set_packing(spangpu_gsm0610_t *bank, int channel, int packing)
{
    printf("  bank: gsm0610_set_packing(#%d, ch %d, %d)\n", bank->k.id, channel, packing);
    bank->k.a = packing;
    return SPANGPU_OK;
}

long long spangpu_gsm0610_encode_capacity(const spangpu_gsm0610_t *bank, int samples)
{
    printf("  bank: gsm0610_encode_capacity(#%d, %d)\n", bank->k.id, samples);
    return (long long) (samples/gsm_unit_samples(bank->k.a))*gsm_unit_bytes(bank->k.a) + 16;
}

long long spangpu_gsm0610_decode_capacity(const spangpu_gsm0610_t *bank, int bytes)
{
    printf("  bank: gsm0610_decode_capacity(#%d, %d)\n", bank->k.id, bytes);
    return (long long) (bytes/gsm_unit_bytes(bank->k.a))*gsm_unit_samples(bank->k.a) + 16;
}

int spangpu_gsm0610_encode(spangpu_gsm0610_t *bank, const void *amp, int amp_mem_kind, long long amp_stride_bytes, const int32_t *lens,
                           int max_samples, uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, int32_t *bytes_out)
{
    code_row(codes, codes_stride_bytes, amp, amp_stride_bytes);
    bytes_out[0] = (max_samples/gsm_unit_samples(bank->k.a))*gsm_unit_bytes(bank->k.a);
    printf("  bank: gsm0610_encode(#%d, mem %d, in stride %lld, lens %s, samples %d, mem %d, out stride %lld) -> %d\n", bank->k.id, amp_mem_kind,
           amp_stride_bytes, lens  ?  "given"  :  "NULL", max_samples, codes_mem_kind, codes_stride_bytes, (int) bytes_out[0]);
    return SPANGPU_OK;
}

int spangpu_gsm0610_decode(spangpu_gsm0610_t *bank, const uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, const int32_t *lens,
                           int max_bytes, void *amp, int amp_mem_kind, long long amp_stride_bytes, int32_t *samples_out)
{
    code_row(amp, amp_stride_bytes, codes, codes_stride_bytes);
    samples_out[0] = (max_bytes/gsm_unit_bytes(bank->k.a))*gsm_unit_samples(bank->k.a);
    printf("  bank: gsm0610_decode(#%d, mem %d, in stride %lld, lens %s, bytes %d, mem %d, out stride %lld) -> %d\n", bank->k.id, codes_mem_kind,
           codes_stride_bytes, lens  ?  "given"  :  "NULL", max_bytes, amp_mem_kind, amp_stride_bytes, (int) samples_out[0]);
    return SPANGPU_OK;
}

/* ---- V.18 -------------------------------------------------------------------------------------------------- */
int spangpu_v18_create(spangpu_v18_t **bank, int device, int n_channels, const int32_t *modes, int n_modes, int calling_party)
{
    char what[96];

    sprintf(what, "v18_create(dev %d, ch %d, mode %d, n %d, calling %d)", device, n_channels, (int) modes[0], n_modes, calling_party);
    return ((*bank = (spangpu_v18_t *) make(what)) == NULL)  ?  SPANGPU_ERR_NO_DEVICE  :  SPANGPU_OK;
}

void spangpu_v18_destroy(spangpu_v18_t *bank) { unmake("v18_destroy", bank); }

int spangpu_v18_tx(spangpu_v18_t *bank, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    (void) mem_kind;
    return send_row("v18_tx", &bank->k, pcm, stride, samples, lens);
}

int spangpu_v18_rx(spangpu_v18_t *bank, const int16_t *amp, int mem_kind, int samples, long long stride)
{
    printf("  bank: v18_rx(#%d, mem %d, samples %d, stride %lld, sum %u)\n", bank->k.id, mem_kind, samples, stride, sum_of(amp, 2LL*samples));
    return SPANGPU_OK;
}

int spangpu_v18_text(spangpu_v18_t *bank, const uint8_t **chars, const int32_t **counts)
{
    static const uint8_t text[2] = { 'o', 'k' };
    static const int32_t n = 2;

    printf("  bank: v18_text(#%d)\n", bank->k.id);
    *chars = text;
    *counts = &n;
    return 2;
}

int spangpu_v18_fillin(spangpu_v18_t *bank, int channel, int len)
{
    printf("  bank: v18_fillin(#%d, ch %d, %d)\n", bank->k.id, channel, len);
    return SPANGPU_OK;
}

int spangpu_v18_put(spangpu_v18_t *bank, int first, int n, const uint8_t *text, int stride, const int32_t *lens, int32_t *results)
{
    printf("  bank: v18_put(#%d, first %d, n %d, stride %d, len %d, sum %u)\n", bank->k.id, first, n, stride, (int) lens[0], sum_of(text, lens[0]));
    results[0] = lens[0];
    return SPANGPU_OK;
}

/* ---- caller ID --------------------------------------------------------------------------------------------- */
int spangpu_adsi_tx_create(spangpu_adsi_tx_t **bank, int device, int n_channels, const int32_t *standards, int n_standards)
{
    char what[96];

    sprintf(what, "adsi_tx_create(dev %d, ch %d, standard %d, n %d)", device, n_channels, (int) standards[0], n_standards);
    return ((*bank = (spangpu_adsi_tx_t *) make(what)) == NULL)  ?  SPANGPU_ERR_NO_DEVICE  :  SPANGPU_OK;
}

void spangpu_adsi_tx_destroy(spangpu_adsi_tx_t *bank) { unmake("adsi_tx_destroy", bank); }

int spangpu_adsi_tx(spangpu_adsi_tx_t *bank, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    (void) mem_kind;
    return send_row("adsi_tx", &bank->k, pcm, stride, samples, lens);
}

int spangpu_adsi_tx_put_message(spangpu_adsi_tx_t *bank, int first, int n, const uint8_t *msgs, int stride, const int32_t *lens, int32_t *results)
{
    printf("  bank: adsi_tx_put_message(#%d, first %d, n %d, stride %d, len %d, sum %u)\n", bank->k.id, first, n, stride, (int) lens[0],
           sum_of(msgs, lens[0]));
    results[0] = lens[0];
    return SPANGPU_OK;
}

int spangpu_adsi_tx_set_preamble(spangpu_adsi_tx_t *bank, int channel, int preamble_len, int preamble_ones_len, int postamble_ones_len, int stop_bits)
{
    printf("  bank: adsi_tx_set_preamble(#%d, ch %d, %d, %d, %d, %d)\n", bank->k.id, channel, preamble_len, preamble_ones_len, postamble_ones_len,
           stop_bits);
    return SPANGPU_OK;
}

int spangpu_adsi_tx_send_alert_tone(spangpu_adsi_tx_t *bank, int channel)
{
    printf("  bank: adsi_tx_send_alert_tone(#%d, ch %d)\n", bank->k.id, channel);
    return SPANGPU_OK;
}

int spangpu_adsi_rx_create(spangpu_adsi_rx_t **bank, int device, int n_channels, const int32_t *standards, int n_standards)
{
    char what[96];

    sprintf(what, "adsi_rx_create(dev %d, ch %d, standard %d, n %d)", device, n_channels, (int) standards[0], n_standards);
    return ((*bank = (spangpu_adsi_rx_t *) make(what)) == NULL)  ?  SPANGPU_ERR_NO_DEVICE  :  SPANGPU_OK;
}

void spangpu_adsi_rx_destroy(spangpu_adsi_rx_t *bank) { unmake("adsi_rx_destroy", bank); }

int spangpu_adsi_rx(spangpu_adsi_rx_t *bank, const int16_t *amp, int mem_kind, int samples, long long stride)
{
    printf("  bank: adsi_rx(#%d, mem %d, samples %d, stride %lld, sum %u)\n", bank->k.id, mem_kind, samples, stride, sum_of(amp, 2LL*samples));
    return SPANGPU_OK;
}

int spangpu_adsi_rx_messages(spangpu_adsi_rx_t *bank, const uint8_t **bytes, const int32_t **lens, const int32_t **counts)
{
    static const uint8_t msg[SPANGPU_ADSI_MSG_BYTES] = { 0x80, 0x02, 0x01, 0x02 };
    static const int32_t len = 4;
    static const int32_t n = 1;

    printf("  bank: adsi_rx_messages(#%d)\n", bank->k.id);
    *bytes = msg;
    *lens = &len;
    *counts = &n;
    return 1;
}

/* ---- FSK sender and connect tones -------------------------------------------------------------------------- */
int spangpu_fsktx_create(spangpu_fsktx_t **tx, int device, int n_channels, const spangpu_fsk_spec_t *spec, int bit_source, const uint32_t *seeds,
                         int queue_bits)
{
    char what[128];

    sprintf(what, "fsktx_create(dev %d, ch %d, %d/%d Hz, baud %d, source %d, seeds %s, queue %d)", device, n_channels, spec->freq_zero,
            spec->freq_one, spec->baud_rate, bit_source, seeds  ?  "given"  :  "NULL", queue_bits);
    return ((*tx = (spangpu_fsktx_t *) make(what)) == NULL)  ?  SPANGPU_ERR_NO_DEVICE  :  SPANGPU_OK;
}

void spangpu_fsktx_destroy(spangpu_fsktx_t *tx) { unmake("fsktx_destroy", tx); }

int spangpu_fsktx_tx(spangpu_fsktx_t *tx, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    (void) mem_kind;
    return send_row("fsktx_tx", &tx->k, pcm, stride, samples, lens);
}

int spangpu_fsktx_power(spangpu_fsktx_t *tx, int channel, float power_dbm0)
{
    printf("  bank: fsktx_power(#%d, ch %d, %.1f)\n", tx->k.id, channel, power_dbm0);
    return SPANGPU_OK;
}

int spangpu_fsktx_restart(spangpu_fsktx_t *tx, int channel, const spangpu_fsk_spec_t *spec)
{
    printf("  bank: fsktx_restart(#%d, ch %d, baud %d)\n", tx->k.id, channel, spec->baud_rate);
    tx->k.shutdown = 0;
    return SPANGPU_OK;
}

int spangpu_fsktx_put_bits(spangpu_fsktx_t *tx, int first, int n, const uint8_t *bits, int stride, const int32_t *lens, int32_t *accepted)
{
    printf("  bank: fsktx_put_bits(#%d, first %d, n %d, stride %d, bits %d, sum %u, accepted %s)\n", tx->k.id, first, n, stride, (int) lens[0],
           sum_of(bits, stride), accepted  ?  "given"  :  "NULL");
    return SPANGPU_OK;
}

int spangpu_fsktx_end_of_data(spangpu_fsktx_t *tx, int channel, int on)
{
    printf("  bank: fsktx_end_of_data(#%d, ch %d, %d)\n", tx->k.id, channel, on);
    tx->k.ended = on;
    return SPANGPU_OK;
}

int spangpu_async_frame_bits(int data_bits, int parity, int stop_bits, const uint8_t *bytes, int n, uint8_t *bits_out, int max)
{
    int i;

    (void) parity;
    (void) n;
    if (1 + data_bits + stop_bits > max)
        return -1;
    bits_out[0] = 0;
    for (i = 0;  i < data_bits;  i++)
        bits_out[1 + i] = (bytes[0] >> i) & 1;
    for (i = 0;  i < stop_bits;  i++)
        bits_out[1 + data_bits + i] = 1;
    return 1 + data_bits + stop_bits;
}

long long spangpu_fsktx_bits_due(int baud_rate, int baud_frac, int samples)
{
    return ((long long) baud_frac + (long long) samples*baud_rate)/(8000*100);
}

int spangpu_mcttx_create(spangpu_mcttx_t **tx, int device, int tone_type, int n_channels)
{
    char what[96];

    sprintf(what, "mcttx_create(dev %d, tone %d, ch %d)", device, tone_type, n_channels);
    return ((*tx = (spangpu_mcttx_t *) make(what)) == NULL)  ?  SPANGPU_ERR_NO_DEVICE  :  SPANGPU_OK;
}

void spangpu_mcttx_destroy(spangpu_mcttx_t *tx) { unmake("mcttx_destroy", tx); }

int spangpu_mcttx_tx(spangpu_mcttx_t *tx, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    (void) mem_kind;
    return send_row("mcttx_tx", &tx->k, pcm, stride, samples, lens);
}

/* ---- modem senders ------------------------------------------------------------------------------------------ */
int spangpu_modemtx_cursor_init(spangpu_modemtx_cursor_t *cur, int modem, int bit_rate, int tep, int short_train)
{
    printf("  bank: modemtx_cursor_init(modem %d, rate %d, tep %d, short %d)\n", modem, bit_rate, tep, short_train);
    if (bit_rate <= 0  ||  bit_rate%2400)
        return SPANGPU_ERR_BAD_ARG;
    memset(cur, 0, sizeof(*cur));
    cur->modem = modem;
    cur->bit_rate = bit_rate;
    cur->short_train = short_train;
    return SPANGPU_OK;
}

long long spangpu_modemtx_cursor_advance(spangpu_modemtx_cursor_t *cur, int samples, long long bits_before_end)
{
    const long long due = (long long) samples*cur->bit_rate/8000;

    printf("  bank: modemtx_cursor_advance(phase %d, samples %d, end %lld) -> %lld\n", cur->baud_phase, samples, bits_before_end, due);
    cur->baud_phase += samples;
    return due;
}

int spangpu_modemtx_create_ex(spangpu_modemtx_t **tx, int device, int modem, int n_channels, int bit_rate, int tep, int bit_source,
                              const uint32_t *seeds, int queue_bits)
{
    char what[128];

    sprintf(what, "modemtx_create_ex(dev %d, modem %d, ch %d, rate %d, tep %d, source %d, seeds %s, queue %d)", device, modem, n_channels,
            bit_rate, tep, bit_source, seeds  ?  "given"  :  "NULL", queue_bits);
    return ((*tx = (spangpu_modemtx_t *) make(what)) == NULL)  ?  SPANGPU_ERR_NO_DEVICE  :  SPANGPU_OK;
}

void spangpu_modemtx_destroy(spangpu_modemtx_t *tx) { unmake("modemtx_destroy", tx); }

int spangpu_modemtx_power(spangpu_modemtx_t *tx, int channel, float power_dbm0)
{
    printf("  bank: modemtx_power(#%d, ch %d, %.1f)\n", tx->k.id, channel, power_dbm0);
    return SPANGPU_OK;
}

int spangpu_modemtx_restart_ex(spangpu_modemtx_t *tx, int channel, int bit_rate, int tep, int short_train)
{
    printf("  bank: modemtx_restart_ex(#%d, ch %d, rate %d, tep %d, short %d)\n", tx->k.id, channel, bit_rate, tep, short_train);
    tx->k.ended = 0;
    tx->k.shutdown = 0;
    return SPANGPU_OK;
}

int spangpu_modemtx_tx_lens(spangpu_modemtx_t *tx, int mem, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    (void) mem;
    send_row("modemtx_tx_lens", &tx->k, pcm, stride, samples, lens);
    return samples;
}

int spangpu_modemtx_tx_continue(spangpu_modemtx_t *tx, int mem, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    (void) mem;
    send_row("modemtx_tx_continue", &tx->k, pcm, stride, samples, lens);
    return samples;
}

int spangpu_modemtx_put_bits(spangpu_modemtx_t *tx, int first, int n, const uint8_t *bits, int stride, const int32_t *lens, int32_t *accepted)
{
    printf("  bank: modemtx_put_bits(#%d, first %d, n %d, stride %d, bits %d, sum %u, accepted %s)\n", tx->k.id, first, n, stride, (int) lens[0],
           sum_of(bits, stride), accepted  ?  "given"  :  "NULL");
    return SPANGPU_OK;
}

int spangpu_modemtx_end_of_data(spangpu_modemtx_t *tx, int channel, int on)
{
    printf("  bank: modemtx_end_of_data(#%d, ch %d, %d)\n", tx->k.id, channel, on);
    tx->k.ended = on;
    return SPANGPU_OK;
}

int spangpu_modemtx_events(spangpu_modemtx_t *tx, const int32_t **channels, const int32_t **kinds)
{
    printf("  bank: modemtx_events(#%d) -> %d\n", tx->k.id, tx->k.n_ev);
    tx->k.ev_channel = 0;
    tx->k.ev_kind = SPANGPU_MODEMTX_SHUTDOWN_COMPLETE;
    *channels = &tx->k.ev_channel;
    *kinds = &tx->k.ev_kind;
    return tx->k.n_ev;
}

/* ---- digit senders ------------------------------------------------------------------------------------------ */
int spangpu_txbank_create(spangpu_txbank_t **bank, int device, int kind, int n_channels)
{
    char what[96];

    sprintf(what, "txbank_create(dev %d, kind %d, ch %d)", device, kind, n_channels);
    return ((*bank = (spangpu_txbank_t *) make(what)) == NULL)  ?  SPANGPU_ERR_NO_DEVICE  :  SPANGPU_OK;
}

void spangpu_txbank_destroy(spangpu_txbank_t *bank) { unmake("txbank_destroy", bank); }

int spangpu_txbank_set_level(spangpu_txbank_t *bank, int first, int n, int level, int twist)
{
    printf("  bank: txbank_set_level(#%d, first %d, n %d, %d, %d)\n", bank->k.id, first, n, level, twist);
    return SPANGPU_OK;
}

int spangpu_txbank_set_timing(spangpu_txbank_t *bank, int first, int n, int on_time, int off_time)
{
    printf("  bank: txbank_set_timing(#%d, first %d, n %d, %d, %d)\n", bank->k.id, first, n, on_time, off_time);
    return SPANGPU_OK;
}

int spangpu_txbank_put(spangpu_txbank_t *bank, int first, int n, const char *digits, int len)
{
    printf("  bank: txbank_put(#%d, first %d, n %d, len %d)\n", bank->k.id, first, n, len);
    (void) digits;
    return 0;
}

int spangpu_txbank_tx(spangpu_txbank_t *bank, int mem_kind, int16_t *pcm, long long stride, int samples, int *lens)
{
    int32_t got = 0;

    (void) mem_kind;
    send_row("txbank_tx", &bank->k, pcm, stride, samples, &got);
    *lens = got;
    return SPANGPU_OK;
}

/* ---- the group receivers of shim_fsk.c: linked, never reached ------------------------------------------------ */
int spangpu_fsk_create(spangpu_fsk_t **fsk, int device, int n_channels, const spangpu_fsk_spec_t *spec, int framing_mode)
{
    (void) fsk, (void) device, (void) n_channels, (void) spec, (void) framing_mode;
    abort();
}
void spangpu_fsk_destroy(spangpu_fsk_t *fsk) { (void) fsk; abort(); }
int spangpu_fsk_rx_var(spangpu_fsk_t *fsk, const int16_t *amp, int mem, const int32_t *lens, int max_samples, long long stride)
{
    (void) fsk, (void) amp, (void) mem, (void) lens, (void) max_samples, (void) stride;
    abort();
}
int spangpu_fsk_events(spangpu_fsk_t *fsk, const int16_t **events, const int32_t **counts) { (void) fsk, (void) events, (void) counts; abort(); }
int spangpu_fsk_state_words(const spangpu_fsk_t *fsk) { (void) fsk; abort(); }
int spangpu_fsk_get_state(spangpu_fsk_t *fsk, int channel, int32_t *words) { (void) fsk, (void) channel, (void) words; abort(); }
int spangpu_fsk_set_state(spangpu_fsk_t *fsk, int channel, const int32_t *words) { (void) fsk, (void) channel, (void) words; abort(); }
int spangpu_fsk_restart(spangpu_fsk_t *fsk, int channel, int framing_mode) { (void) fsk, (void) channel, (void) framing_mode; abort(); }
int spangpu_fsk_set_signal_cutoff(spangpu_fsk_t *fsk, int channel, float cutoff_dbm0) { (void) fsk, (void) channel, (void) cutoff_dbm0; abort(); }
int spangpu_fsk_set_frame_parameters(spangpu_fsk_t *fsk, int channel, int data_bits, int parity, int stop_bits)
{
    (void) fsk, (void) channel, (void) data_bits, (void) parity, (void) stop_bits;
    abort();
}
int spangpu_fsk_fillin(spangpu_fsk_t *fsk, int channel, int len) { (void) fsk, (void) channel, (void) len; abort(); }
int spangpu_mct_create(spangpu_mct_t **mct, int device, int tone_type, int n_channels, int use_callback)
{
    (void) mct, (void) device, (void) tone_type, (void) n_channels, (void) use_callback;
    abort();
}
void spangpu_mct_destroy(spangpu_mct_t *mct) { (void) mct; abort(); }
int spangpu_mct_rx_var(spangpu_mct_t *mct, const int16_t *amp, int mem, const int32_t *lens, int max_samples, long long stride)
{
    (void) mct, (void) amp, (void) mem, (void) lens, (void) max_samples, (void) stride;
    abort();
}
int spangpu_mct_events(spangpu_mct_t *mct, const int32_t **events, const int32_t **counts) { (void) mct, (void) events, (void) counts; abort(); }
int spangpu_mct_get(spangpu_mct_t *mct, int channel) { (void) mct, (void) channel; abort(); }
int spangpu_mct_state_words(const spangpu_mct_t *mct) { (void) mct; abort(); }
int spangpu_mct_get_state(spangpu_mct_t *mct, int channel, int32_t *words) { (void) mct, (void) channel, (void) words; abort(); }
int spangpu_mct_set_state(spangpu_mct_t *mct, int channel, const int32_t *words) { (void) mct, (void) channel, (void) words; abort(); }
