// adsi_api.hip -- C ABI of the caller-ID (ADSI) banks (include/spangpu.h, "Caller-ID banks"): batched adsi_tx_put_message()
// / adsi_tx() and adsi_rx() in the four FSK standards.  Device code: adsi_dev.hpp.  No CPU implementation of the signal path
// exists behind these entry points; message packing and the field helpers are plain host C (adsi_host.c), and the
// control-plane calls (preamble, alert tone, restart, state) edit one channel's words on the host, as the reference's own
// functions edit one object.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#define SPG_HDLC_STEP_FUNCTIONS_ONLY        // the HDLC banks' own kernels belong to hdlc_api.hip
#include "adsi_dev.hpp"
#include "bank_host.hpp"
#include "modem_tables.h"

using namespace spg;

extern "C" void spangpu_fsk_words_init(int32_t *w, const spangpu_fsk_spec_t *spec, int framing_mode, int data_bits, int parity, int stop_bits);
extern "C" void spangpu_fsktx_words_restart(int32_t *w, const spangpu_fsk_spec_t *spec);

struct spangpu_adsi_tx_s
{
    BankCore c;
    PcmStage pcm;               // frames of a host caller; d_lens: the lengths returned to one
    int16_t *quarter;
    float *sine;
    uint8_t *msgs;              // [n_ch][kAdsiMsg]
    int32_t tone[13];           // the alert tone's descriptor: rates, gains, durations, repeat
    uint8_t *d_packed;
    size_t packed_cap;
    int32_t *d_plens;
    int32_t *d_res;
};

struct spangpu_adsi_rx_s
{
    BankCore c;
    PcmStage pcm;
    int span;
    int16_t *quarter;
    uint8_t *msgs;
    VarLens rxlens;             // per-channel lengths of an rx_var call
    uint8_t *rec_bytes;         // [n_ch][last_cap][kAdsiMsg]
    uint8_t *h_bytes;
    int32_t *rec_lens;          // [n_ch][last_cap]
    int32_t *h_lens;
    CountRows counts;
    int cap;
    int lens_cap;
    int last_cap;
};

static int standard_ok(int standard)
{
    return standard >= SPANGPU_ADSI_STANDARD_CLASS  &&  standard <= SPANGPU_ADSI_STANDARD_JCLIP;
}

static void spec_of(int standard, spangpu_fsk_spec_t *spec)
{
    spangpu_fsk_preset((standard == SPANGPU_ADSI_STANDARD_CLASS)  ?  SPANGPU_FSK_BELL202  :  SPANGPU_FSK_V23CH1, spec);
}

// adsi_tx_set_preamble(), adsi.c:563-623: negative values take the standard's defaults
static void preamble_words(int32_t *w, int preamble_len, int preamble_ones_len, int postamble_ones_len, int stop_bits)
{
    const bool jclip = (w[ADT_STANDARD] == SPANGPU_ADSI_STANDARD_JCLIP);
    w[ADT_PREAMBLE_LEN] = (preamble_len < 0)  ?  (jclip  ?  0  :  300)  :  preamble_len;
    w[ADT_PREAMBLE_ONES_LEN] = (preamble_ones_len < 0)  ?  (jclip  ?  75  :  80)  :  preamble_ones_len;
    w[ADT_POSTAMBLE_ONES_LEN] = (postamble_ones_len < 0)  ?  5  :  postamble_ones_len;
    w[ADT_STOP_BITS] = (stop_bits < 0)  ?  (jclip  ?  4  :  1)  :  stop_bits;
}

// adsi_tx_init(), adsi.c:732-757: memset, the default preamble, start_tx().  The zeroed tone generator sits in section 0
// with no durations: the first call ends it.
static void tx_words(int32_t *w, int standard)
{
    spangpu_fsk_spec_t spec;
    spec_of(standard, &spec);
    memset(w, 0, (size_t) (kAdsiTxWords + kFskTxWords)*sizeof(int32_t));
    w[ADT_STANDARD] = standard;
    preamble_words(w, -1, -1, -1, -1);
    spangpu_fsktx_words_restart(w + kAdsiTxWords, &spec);
    w[ADT_TX_SIGNAL_ON] = 1;
}

// adsi_rx_init(), adsi.c:463-509: memset, fsk_rx_init(.., FSK_FRAME_MODE_ASYNC, ..)
static void rx_words(int32_t *w, int words, int standard)
{
    spangpu_fsk_spec_t spec;
    spec_of(standard, &spec);
    memset(w, 0, (size_t) words*sizeof(int32_t));
    w[ADR_STANDARD] = standard;
    spangpu_fsk_words_init(w + kAdsiRxWords, &spec, SPANGPU_FSK_FRAME_MODE_ASYNC, 8, SPANGPU_ASYNC_PARITY_NONE, 1);
}

static int standards_ok(const int32_t *standards, int n_standards)
{
    if (standards == NULL  ||  n_standards <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (at least one standard)");
    for (int i = 0;  i < n_standards;  i++)
    {
        if (!standard_ok(standards[i]))
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a caller-ID bank runs CLASS, CLIP, A-CLIP and J-CLIP only (not CLIP-DTMF, not TDD)");
    }
    return SPANGPU_OK;
}

extern "C" {

/*
 * Entry point                          stands for (paths relative to the reference tree)
 *   spangpu_adsi_tx_create()           adsi_tx_init(NULL, standard) x N                          src/adsi.c:732-757
 *   spangpu_adsi_tx_put_message()      adsi_tx_put_message(s, msg, len)                          src/adsi.c:626-723
 *   spangpu_adsi_tx_set_preamble()     adsi_tx_set_preamble(s, ..)                               src/adsi.c:563-623
 *   spangpu_adsi_tx_send_alert_tone()  adsi_tx_send_alert_tone(s)                                src/adsi.c:557-560
 *   spangpu_adsi_tx()                  adsi_tx(s, amp, max_len) x N                              src/adsi.c:525-555
 *   spangpu_adsi_tx_restart()          adsi_tx_init(s, standard) on one channel
 *   spangpu_adsi_rx_create()           adsi_rx_init(NULL, standard, put_msg, user_data) x N      src/adsi.c:463-509
 *   spangpu_adsi_rx() / _rx_var()      adsi_rx(s, amp, len) x N                                  src/adsi.c:436-454
 *   spangpu_adsi_rx_messages()         the put_msg calls of the last rx call                     src/adsi.c:285, 307
 *   spangpu_adsi_rx_restart()          adsi_rx_init(s, standard, ..) on one channel
 */

void spangpu_adsi_tx_destroy(spangpu_adsi_tx_t *b)
{
    if (b == NULL)
        return;
    core_destroy(&b->c);
    stage_free(&b->pcm);
    (void) hipFree(b->quarter);
    (void) hipFree(b->sine);
    (void) hipFree(b->msgs);
    (void) hipFree(b->d_packed);
    (void) hipFree(b->d_plens);
    (void) hipFree(b->d_res);
    free(b);
}

int spangpu_adsi_tx_create(spangpu_adsi_tx_t **out, int device, int n_channels, const int32_t *standards, int n_standards)
{
    if (out == NULL  ||  n_channels <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    *out = NULL;
    int rc = standards_ok(standards, n_standards);
    if (rc != SPANGPU_OK  ||  (rc = device_ok(device)) != SPANGPU_OK)
        return rc;
    spangpu_adsi_tx_s *b = (spangpu_adsi_tx_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    const int n_words = kAdsiTxWords + kFskTxWords;
    if ((rc = core_create(&b->c, device, n_channels, n_words)) != SPANGPU_OK  ||  (rc = quarter_sine_upload(&b->quarter)) != SPANGPU_OK
        ||  (rc = stage_lens(&b->c, &b->pcm)) != SPANGPU_OK)
    {
        spangpu_adsi_tx_destroy(b);
        return rc;
    }
    // adsi.c:742-751: 2130 Hz + 2750 Hz at -13 dBm0 each, 110 ms on, 60 ms off, once
    spg_make_tone_descriptor(b->tone, 2130, -13, 2750, -13, 110, 60, 0, 0, 0);
    const size_t n = (size_t) n_channels;
    int32_t *host = (int32_t *) calloc((size_t) n_words*n, sizeof(int32_t));
    float *sine = (float *) malloc(2048*sizeof(float));
    if (host == NULL  ||  sine == NULL  ||  hipMalloc(&b->msgs, n*kAdsiMsg) != hipSuccess  ||  hipMalloc(&b->sine, 2048*sizeof(float)) != hipSuccess)
    {
        free(host);
        free(sine);
        spangpu_adsi_tx_destroy(b);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the caller-ID sender bank failed");
    }
    spg_make_sine_table(sine);
    int32_t one[kAdsiTxWords + kFskTxWords];
    for (int c = 0;  c < n_channels;  c++)
    {
        tx_words(one, standards[c % n_standards]);
        for (int w = 0;  w < n_words;  w++)
            host[(size_t) w*n + c] = one[w];
    }
    rc = core_upload(&b->c, host);
    if (rc == SPANGPU_OK
        &&  (hipMemcpy(b->sine, sine, 2048*sizeof(float), hipMemcpyHostToDevice) != hipSuccess  ||  hipMemset(b->msgs, 0, n*kAdsiMsg) != hipSuccess))
        rc = spangpu_set_error(SPANGPU_ERR_HIP, "state upload failed");
    free(host);
    free(sine);
    if (rc != SPANGPU_OK)
    {
        spangpu_adsi_tx_destroy(b);
        return rc;
    }
    *out = b;
    return SPANGPU_OK;
}

int spangpu_adsi_tx_channels(const spangpu_adsi_tx_t *b) { return b  ?  b->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_adsi_tx_state_words(const spangpu_adsi_tx_t *b) { return b  ?  b->c.words  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_adsi_tx_set_stream(spangpu_adsi_tx_t *b, void *stream)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&b->c, stream);
}

int spangpu_adsi_tx_sync(spangpu_adsi_tx_t *b)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&b->c);
}

int spangpu_adsi_tx_put_message(spangpu_adsi_tx_t *b, int first, int n, const uint8_t *msgs, int stride, const int32_t *lens, int32_t *results)
{
    if (b == NULL  ||  !range_ok(&b->c, first, n)  ||  msgs == NULL  ||  lens == NULL  ||  stride <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    for (int i = 0;  i < n;  i++)
    {
        // (a message is its type, its length byte and the fields)
        if (lens[i] < 2  ||  lens[i] > stride)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a channel's message is shorter than 2 bytes or does not fit its row");
    }
    SPG_TRY(hipSetDevice(b->c.device));
    // the packing needs each channel's standard: the one word row is read back
    int32_t *stds = (int32_t *) malloc((size_t) n*3*sizeof(int32_t));
    uint8_t *packed = (uint8_t *) calloc((size_t) n, kAdsiMsg);
    if (stds == NULL  ||  packed == NULL)
    {
        free(stds);
        free(packed);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "malloc");
    }
    int32_t *plens = stds + n;
    int32_t *res = plens + n;
    int rc = SPANGPU_OK;
    if (hipMemcpyAsync(stds, b->c.st + (size_t) ADT_STANDARD*b->c.n_ch + first, (size_t) n*sizeof(int32_t), hipMemcpyDeviceToHost, b->c.stream) != hipSuccess
        ||  hipStreamSynchronize(b->c.stream) != hipSuccess)
        rc = spangpu_set_error(SPANGPU_ERR_HIP, "reading the standards back failed");
    for (int i = 0;  rc == SPANGPU_OK  &&  i < n;  i++)
    {
        plens[i] = spangpu_adsi_pack_message(stds[i], msgs + (size_t) i*stride, lens[i], packed + (size_t) i*kAdsiMsg, kAdsiMsg);
        if (plens[i] < -1)
            rc = spangpu_set_error(SPANGPU_ERR_STATE, "a channel's standard word is not one of the four");
    }
    if (rc == SPANGPU_OK)
        rc = grow(&b->d_packed, &b->packed_cap, (size_t) n*kAdsiMsg, 1, b->c.stream);
    if (rc == SPANGPU_OK
        &&  ((b->d_plens == NULL  &&  hipMalloc(&b->d_plens, (size_t) b->c.n_ch*sizeof(int32_t)) != hipSuccess)
             ||  (b->d_res == NULL  &&  hipMalloc(&b->d_res, (size_t) b->c.n_ch*sizeof(int32_t)) != hipSuccess)))
        rc = spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "message staging");
    if (rc == SPANGPU_OK)
    {
        hipError_t e = hipMemcpyAsync(b->d_packed, packed, (size_t) n*kAdsiMsg, hipMemcpyHostToDevice, b->c.stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(b->d_plens, plens, (size_t) n*sizeof(int32_t), hipMemcpyHostToDevice, b->c.stream);
        if (e == hipSuccess)
        {
            hipLaunchKernelGGL(adsi_put_kernel, dim3((n + 63)/64), dim3(64), 0, b->c.stream, b->c.st, b->msgs, b->c.n_ch, first, first + n,
                               b->d_packed, b->d_plens, b->d_res);
            e = hipGetLastError();
        }
        if (e == hipSuccess)
            e = hipMemcpyAsync(res, b->d_res, (size_t) n*sizeof(int32_t), hipMemcpyDeviceToHost, b->c.stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(b->c.stream);
        if (e != hipSuccess)
            rc = spangpu_set_error(SPANGPU_ERR_HIP, hipGetErrorString(e));
    }
    if (rc == SPANGPU_OK  &&  results)
    {
        for (int i = 0;  i < n;  i++)
            results[i] = (res[i] > 0)  ?  lens[i]  :  res[i];
    }
    free(stds);
    free(packed);
    return rc;
}

static int tx_edit(spangpu_adsi_tx_s *b, int channel, int what, const int *a)
{
    int32_t w[kAdsiTxWords + kFskTxWords];
    int rc = core_rw_words(&b->c, channel, 0, b->c.words, w, false);
    if (rc != SPANGPU_OK)
        return rc;
    switch (what)
    {
    case 0:
        tx_words(w, a[0]);
        break;
    case 1:
        preamble_words(w, a[0], a[1], a[2], a[3]);
        break;
    case 2:
        // tone_gen_init(&s->alert_tone_gen, &s->alert_tone_desc)
        w[ADT_TONE_SECTION] = 0;
        w[ADT_TONE_POS] = 0;
        w[ADT_TONE_PHASE0] = 0;
        w[ADT_TONE_PHASE1] = 0;
        w[ADT_TONE_DUR0] = b->tone[8];
        w[ADT_TONE_DUR1] = b->tone[9];
        break;
    }
    return core_rw_words(&b->c, channel, 0, b->c.words, w, true);
}

int spangpu_adsi_tx_set_preamble(spangpu_adsi_tx_t *b, int channel, int preamble_len, int preamble_ones_len, int postamble_ones_len, int stop_bits)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int a[4] = {preamble_len, preamble_ones_len, postamble_ones_len, stop_bits};
    return tx_edit(b, channel, 1, a);
}

int spangpu_adsi_tx_send_alert_tone(spangpu_adsi_tx_t *b, int channel)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return tx_edit(b, channel, 2, NULL);
}

int spangpu_adsi_tx_restart(spangpu_adsi_tx_t *b, int channel, int standard)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel)  ||  !standard_ok(standard))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (CLASS, CLIP, A-CLIP or J-CLIP)");
    // adsi_tx_init() clears the whole object, msg[] with it: a sender that is restarted and then runs without a put sends
    // msg[0] behind its preamble (adsi.c:129 with msg_len 0), and that byte is 0, not the first of the message before
    const int rc = tx_edit(b, channel, 0, &standard);
    if (rc != SPANGPU_OK)
        return rc;
    SPG_TRY(hipMemsetAsync(b->msgs + (size_t) channel*kAdsiMsg, 0, kAdsiMsg, b->c.stream));
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    return SPANGPU_OK;
}

int spangpu_adsi_tx(spangpu_adsi_tx_t *b, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    int rc = tx_args_ok(b, mem_kind, pcm, stride, samples);
    if (rc != SPANGPU_OK)
        return rc;
    if (samples == 0)
    {
        if (lens  &&  mem_kind == SPANGPU_MEM_HOST)
            memset(lens, 0, (size_t) b->c.n_ch*sizeof(int32_t));
        return SPANGPU_OK;
    }
    SPG_TRY(hipSetDevice(b->c.device));
    AdsiTxLaunch L;
    memset(&L, 0, sizeof(L));
    if ((rc = stage_out_target(&b->c, &b->pcm, mem_kind, pcm, stride, samples, lens, &L.pcm, &L.stride, &L.lens, &L.vec)) != SPANGPU_OK)
        return rc;
    L.st = b->c.st;
    L.quarter = b->quarter;
    L.sine = b->sine;
    L.msgs = b->msgs;
    L.n_ch = b->c.n_ch;
    L.samples = samples;
    L.tone_rate[0] = b->tone[0];
    L.tone_rate[1] = b->tone[1];
    memcpy(L.tone_gain, &b->tone[4], 2*sizeof(float));
    hipLaunchKernelGGL(adsi_tx_kernel, dim3((b->c.n_ch + kFtxCpw*kFtxWaves - 1)/(kFtxCpw*kFtxWaves)), dim3(64*kFtxWaves), 0, b->c.stream, L);
    SPG_TRY(hipGetLastError());
    return stage_out_back(&b->c, &b->pcm, mem_kind, pcm, stride, samples, lens);
}

int spangpu_adsi_tx_get_state(spangpu_adsi_tx_t *b, int channel, int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, 0, b->c.words, words, false);
}

int spangpu_adsi_tx_set_state(spangpu_adsi_tx_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int sec = words[ADT_TONE_SECTION];
    const int dur = (sec == 0)  ?  words[ADT_TONE_DUR0]  :  ((sec == 1)  ?  words[ADT_TONE_DUR1]  :  0);
    if (!standard_ok(words[ADT_STANDARD])  ||  words[ADT_MSG_LEN] < 0  ||  words[ADT_MSG_LEN] > kAdsiMsg
        ||  words[ADT_BYTE_NO] < 0  ||  words[ADT_BYTE_NO] >= kAdsiMsg  ||  words[ADT_BIT_POS] < 0  ||  words[ADT_BIT_NO] < 0
        ||  sec < -1  ||  sec > 3  ||  words[ADT_TONE_POS] < 0  ||  words[ADT_TONE_POS] > dur
        ||  words[ADT_TONE_DUR0] < 0  ||  words[ADT_TONE_DUR1] < 0
        ||  words[kAdsiTxWords + FT_BAUD_RATE] <= 0  ||  words[kAdsiTxWords + FT_BAUD_RATE] > kFtxBaudUnit
        ||  words[kAdsiTxWords + FT_BAUD_FRAC] < 0  ||  words[kAdsiTxWords + FT_BAUD_FRAC] >= kFtxBaudUnit)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "not the words of a channel of this bank");
    return core_rw_words(&b->c, channel, 0, b->c.words, const_cast<int32_t *>(words), true);
}

// The message bytes travel with the words when a channel is moved: msg[kAdsiMsg], host memory
int spangpu_adsi_tx_get_message(spangpu_adsi_tx_t *b, int channel, uint8_t *msg)
{
    if (b == NULL  ||  msg == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipMemcpyAsync(msg, b->msgs + (size_t) channel*kAdsiMsg, kAdsiMsg, hipMemcpyDeviceToHost, b->c.stream));
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    return SPANGPU_OK;
}

int spangpu_adsi_tx_set_message(spangpu_adsi_tx_t *b, int channel, const uint8_t *msg)
{
    if (b == NULL  ||  msg == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipMemcpyAsync(b->msgs + (size_t) channel*kAdsiMsg, msg, kAdsiMsg, hipMemcpyHostToDevice, b->c.stream));
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    return SPANGPU_OK;
}

// ---- receivers --------------------------------------------------------------------------------------------------------

void spangpu_adsi_rx_destroy(spangpu_adsi_rx_t *b)
{
    if (b == NULL)
        return;
    core_destroy(&b->c);
    stage_free(&b->pcm);
    (void) hipFree(b->quarter);
    (void) hipFree(b->msgs);
    lens_free(&b->rxlens);
    (void) hipFree(b->rec_bytes);
    (void) hipFree(b->rec_lens);
    if (b->h_bytes)
        (void) hipHostFree(b->h_bytes);
    if (b->h_lens)
        (void) hipHostFree(b->h_lens);
    counts_free(&b->counts);
    free(b);
}

int spangpu_adsi_rx_create(spangpu_adsi_rx_t **out, int device, int n_channels, const int32_t *standards, int n_standards)
{
    if (out == NULL  ||  n_channels <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    *out = NULL;
    int rc = standards_ok(standards, n_standards);
    if (rc != SPANGPU_OK  ||  (rc = device_ok(device)) != SPANGPU_OK)
        return rc;
    spangpu_adsi_rx_s *b = (spangpu_adsi_rx_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    b->span = kFskRateX100/(1200*100);      // both modems run at 1200 baud
    const int n_words = kAdsiRxWords + kFskScalars + 4*b->span;
    if ((rc = core_create(&b->c, device, n_channels, n_words)) != SPANGPU_OK  ||  (rc = quarter_sine_upload(&b->quarter)) != SPANGPU_OK)
    {
        spangpu_adsi_rx_destroy(b);
        return rc;
    }
    const size_t n = (size_t) n_channels;
    int32_t *one = (int32_t *) calloc(n_words, sizeof(int32_t));
    int32_t *host = (int32_t *) calloc((size_t) n_words*n, sizeof(int32_t));
    if (one == NULL  ||  host == NULL  ||  hipMalloc(&b->msgs, n*kAdsiMsg) != hipSuccess
        ||  counts_create(&b->c, &b->counts, 1, 1) != SPANGPU_OK)
    {
        free(one);
        free(host);
        spangpu_adsi_rx_destroy(b);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the caller-ID receiver bank failed");
    }
    for (int c = 0;  c < n_channels;  c++)
    {
        rx_words(one, n_words, standards[c % n_standards]);
        // (the correlation windows stay zero: only the scalars are written)
        for (int w = 0;  w < kAdsiRxWords + kFskScalars;  w++)
            host[(size_t) w*n + c] = one[w];
    }
    rc = core_upload(&b->c, host);
    free(one);
    free(host);
    if (rc == SPANGPU_OK  &&  hipMemset(b->msgs, 0, n*kAdsiMsg) != hipSuccess)
        rc = spangpu_set_error(SPANGPU_ERR_HIP, "state upload failed");
    if (rc != SPANGPU_OK)
    {
        spangpu_adsi_rx_destroy(b);
        return rc;
    }
    *out = b;
    return SPANGPU_OK;
}

int spangpu_adsi_rx_channels(const spangpu_adsi_rx_t *b) { return b  ?  b->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_adsi_rx_state_words(const spangpu_adsi_rx_t *b) { return b  ?  b->c.words  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_adsi_rx_set_stream(spangpu_adsi_rx_t *b, void *stream)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&b->c, stream);
}

int spangpu_adsi_rx_sync(spangpu_adsi_rx_t *b)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&b->c);
}

int spangpu_adsi_rx_msg_capacity(const spangpu_adsi_rx_t *b, int samples)
{
    if (b == NULL  ||  samples < 0)
        return SPANGPU_ERR_BAD_ARG;
    // The asynchronous bit clock (fsk.c:514-537, fsk_dev.hpp) is put to 50 % by every transition of the demodulator's output
    // and reports a bit when it reaches 100 %: after a report it stands below one sample's step, so no two bits are closer
    // than the samples from 50 % to 100 %, ceil(8000*50/1200) = 4 at 1200 baud, not the 6.67 of a sender.  The shortest
    // message is 3 bytes of 10 bits, so deliveries are at least 30*4 samples apart; and one for the message under way when
    // the call starts.
    const int bit_gap = (kFskRateX100/2 + 1200*100 - 1)/(1200*100);
    return samples/(30*bit_gap) + 1;
}

static int rx_launch(spangpu_adsi_rx_s *b, const int16_t *amp, int mem_kind, int samples, long long stride)
{
    SPG_TRY(hipSetDevice(b->c.device));
    const int cap = spangpu_adsi_rx_msg_capacity(b, samples);
    int rc = grow_pair(&b->rec_bytes, &b->h_bytes, &b->cap, cap, (size_t) b->c.n_ch*kAdsiMsg, b->c.stream);
    if (rc != SPANGPU_OK  ||  (rc = grow_pair(&b->rec_lens, &b->h_lens, &b->lens_cap, cap, (size_t) b->c.n_ch, b->c.stream)) != SPANGPU_OK)
        return rc;
    AdsiRxLaunch V;
    memset(&V, 0, sizeof(V));
    FskLaunch &L = V.f;
    L.st = b->c.st + (size_t) kAdsiRxWords*b->c.n_ch;
    L.quarter = b->quarter;
    L.n_ch = b->c.n_ch;
    L.samples = samples;
    L.lens = b->rxlens.next;
    L.span = b->span;
    // the caller's buffer is only borrowed for the call: the copy in is waited for
    if ((rc = stage_in(&b->c, &b->pcm, mem_kind, amp, stride, samples, true, &L.pcm, &L.stride, &L.vec)) != SPANGPU_OK)
        return rc;
    V.sv = b->c.st;
    V.msgs = b->msgs;
    V.rec_bytes = b->rec_bytes;
    V.rec_lens = b->rec_lens;
    V.counts = b->counts.dev;
    V.cap = cap;
    const size_t lds = (size_t) (4*b->span*64 + 2*kFskMsgWords*64)*sizeof(int32_t);
    hipLaunchKernelGGL(adsi_rx_kernel, dim3((b->c.n_ch + 63)/64), dim3(128), lds, b->c.stream, V);
    SPG_TRY(hipGetLastError());
    b->last_cap = cap;
    return SPANGPU_OK;
}

int spangpu_adsi_rx(spangpu_adsi_rx_t *b, const int16_t *amp, int mem_kind, int samples, long long stride)
{
    if (samples > kMaxSamples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int rc = rx_args_ok(b, mem_kind, amp, samples, &stride);
    if (rc != SPANGPU_OK)
        return rc;
    return rx_launch(b, amp, mem_kind, samples, stride);
}

// spangpu_adsi_rx() for a tick in which not every channel has a frame, or frames differ in length: channel c takes lens[c]
// samples of its row (0: it sits the call out: its state as it was, an empty record).
int spangpu_adsi_rx_var(spangpu_adsi_rx_t *b, const int16_t *amp, int mem_kind, const int32_t *lens, int max_samples, long long stride)
{
    if (b == NULL  ||  amp == NULL  ||  lens == NULL  ||  max_samples <= 0  ||  max_samples > kMaxSamples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (mem_kind_ok(mem_kind) != SPANGPU_OK)
        return SPANGPU_ERR_BAD_ARG;
    int longest;
    bool all;
    int rc = lens_check(lens, b->c.n_ch, max_samples, &longest, &all);
    if (rc != SPANGPU_OK)
        return rc;
    if (stride <= 0)
        stride = max_samples;
    if (stride < max_samples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "stride < max_samples");
    // always a launch of max_samples with the lengths: a call nobody takes part in leaves an empty record
    if ((rc = lens_upload(&b->c, &b->rxlens, lens)) != SPANGPU_OK)
        return rc;
    rc = rx_launch(b, amp, mem_kind, max_samples, stride);
    b->rxlens.next = NULL;
    return rc;
}

int spangpu_adsi_rx_messages(spangpu_adsi_rx_t *b, const uint8_t **bytes, const int32_t **lens, const int32_t **counts)
{
    if (b == NULL  ||  bytes == NULL  ||  lens == NULL  ||  counts == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (b->last_cap <= 0)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no spangpu_adsi_rx() yet");
    int rc = counts_fetch(&b->c, &b->counts, 1);
    if (rc != SPANGPU_OK)
        return rc;
    // the record is sized from the shortest message; a count above it would mean the sizing is wrong, and is not cut short quietly
    int most;
    if (!count_row_scan(b->counts.pinned, b->c.n_ch, b->last_cap, &most))
        return spangpu_set_error(SPANGPU_ERR_STATE, "a channel delivered more messages than a call of this length can carry");
    // (a message arrives once per call set-up: most calls have no column to bring back)
    if ((rc = rows_fetch(&b->c, b->h_bytes, b->rec_bytes, kAdsiMsg, b->last_cap, most)) != SPANGPU_OK
        ||  (rc = rows_fetch(&b->c, b->h_lens, b->rec_lens, sizeof(int32_t), b->last_cap, most)) != SPANGPU_OK)
        return rc;
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    *bytes = b->h_bytes;
    *lens = b->h_lens;
    *counts = b->counts.pinned;
    return b->last_cap;
}

int spangpu_adsi_rx_restart(spangpu_adsi_rx_t *b, int channel, int standard)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel)  ||  !standard_ok(standard))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (CLASS, CLIP, A-CLIP or J-CLIP)");
    int32_t *w = (int32_t *) malloc((size_t) b->c.words*sizeof(int32_t));
    if (w == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "malloc");
    rx_words(w, b->c.words, standard);
    const int rc = core_rw_words(&b->c, channel, 0, b->c.words, w, true);
    free(w);
    if (rc != SPANGPU_OK)
        return rc;
    // (adsi_rx_init() clears msg[] too; the framer never reads what it has not written, spangpu_adsi_rx_get_message() does)
    SPG_TRY(hipMemsetAsync(b->msgs + (size_t) channel*kAdsiMsg, 0, kAdsiMsg, b->c.stream));
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    return SPANGPU_OK;
}

int spangpu_adsi_rx_get_state(spangpu_adsi_rx_t *b, int channel, int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, 0, b->c.words, words, false);
}

int spangpu_adsi_rx_set_state(spangpu_adsi_rx_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (!standard_ok(words[ADR_STANDARD])  ||  words[ADR_MSG_LEN] < 0  ||  words[ADR_MSG_LEN] > kAdsiMsg  ||  words[ADR_BIT_POS] < 0
        ||  words[kAdsiRxWords + FS_SPAN] != b->span  ||  words[kAdsiRxWords + FS_BUF_PTR] < 0  ||  words[kAdsiRxWords + FS_BUF_PTR] >= b->span
        ||  words[kAdsiRxWords + FS_FRAMING] != SPANGPU_FSK_FRAME_MODE_ASYNC)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "not the words of a channel of this bank");
    return core_rw_words(&b->c, channel, 0, b->c.words, const_cast<int32_t *>(words), true);
}

int spangpu_adsi_rx_get_message(spangpu_adsi_rx_t *b, int channel, uint8_t *msg)
{
    if (b == NULL  ||  msg == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipMemcpyAsync(msg, b->msgs + (size_t) channel*kAdsiMsg, kAdsiMsg, hipMemcpyDeviceToHost, b->c.stream));
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    return SPANGPU_OK;
}

int spangpu_adsi_rx_set_message(spangpu_adsi_rx_t *b, int channel, const uint8_t *msg)
{
    if (b == NULL  ||  msg == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipMemcpyAsync(b->msgs + (size_t) channel*kAdsiMsg, msg, kAdsiMsg, hipMemcpyHostToDevice, b->c.stream));
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    return SPANGPU_OK;
}

}   // extern "C"
