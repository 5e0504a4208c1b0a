// faxtx_api.hip -- C ABI of the FAX transmit front-end banks (include/spangpu.h, "FAX transmit front-end banks"): the transmit
// half of N fax_modems_state_t objects under fax_tx(), every per-channel decision in device memory.  The bank owns the two
// connect tone sender banks (CED, CNG), a V.21 FSK sender bank, one modem sender bank per kind and an HDLC sender bank, all on
// its own stream, and runs them over per-channel spans of the row it plans on the device.  Device code: faxtx_dev.hpp.  No CPU
// implementation exists behind these entry points; the control-plane calls (set_tx_type, restart, set_tep_mode, the words) edit
// one channel on the host between ticks, as the reference's own functions edit one object.

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#define SPG_HDLC_STEP_FUNCTIONS_ONLY        // the HDLC banks' own kernels belong to hdlc_api.hip
#include "bank_host.hpp"
#include "faxtx_dev.hpp"

using namespace spg;

static constexpr int kRingBits = 1 << 14;           // the non-ECM bits a line holds ahead of its sender
static constexpr int kQueueDepth = 8;               // frames / flags / end commands a line holds ahead of its framer

struct spangpu_faxtx_s
{
    BankCore c;                         // st = fx[kFaxTxWords][n_ch]
    int kinds_mask;
    int max_samples;
    spangpu_mcttx_t *tone[2];           // CED, CNG
    spangpu_fsktx_t *v21;
    spangpu_modemtx_t *fast[3];         // V.27ter, V.29, V.17
    spangpu_hdlc_tx_t *framer;
    int assigned[kFaxTxSenders];        // channels whose handler or next handler lives in the sender's bank
    int32_t *h_sender;                  // [n_ch]: that bank, per channel, as the host set it
    int32_t *span;                      // [kSpanRows][n_ch]
    int32_t *ret;                       // [n_ch]
    int32_t *cnt;                       // [2][n_ch]
    CountRows out;                      // [kFaxTxOutRows][n_ch]
    int16_t *pcm;                       // [n_ch][pcm_stride]: the rows of a host caller
    long long pcm_stride;
    bool ran;
};

static int modem_of(int sender)
{
    return (sender == kFaxTxSendV17)  ?  SPANGPU_V17  :  (sender == kFaxTxSendV29)  ?  SPANGPU_V29  :  SPANGPU_V27TER;
}

static int mask_of(int sender)
{
    return (sender == kFaxTxSendV17)  ?  SPANGPU_FAXFE_V17  :  (sender == kFaxTxSendV29)  ?  SPANGPU_FAXFE_V29  :  SPANGPU_FAXFE_V27TER;
}

static bool rate_ok(int sender, int bit_rate)
{
    switch (sender)
    {
    case kFaxTxSendV27ter:
        return bit_rate == 4800  ||  bit_rate == 2400;
    case kFaxTxSendV29:
        return bit_rate == 9600  ||  bit_rate == 7200  ||  bit_rate == 4800;
    case kFaxTxSendV17:
        return bit_rate == 14400  ||  bit_rate == 12000  ||  bit_rate == 9600  ||  bit_rate == 7200  ||  bit_rate == 4800;
    }
    return false;
}

// the bank the channel's sender lives in, now or after its silence
static int sender_of_words(const int32_t *fx)
{
    int32_t w[kFaxTxWords];
    memcpy(w, fx, sizeof(w));
    if (w[FX_HANDLER] == kFaxTxSilence)
        w[FX_HANDLER] = w[FX_NEXT_HANDLER];
    return faxtx_sender(w);
}

static void assign(spangpu_faxtx_s *b, int channel, int sender)
{
    b->assigned[b->h_sender[channel]]--;
    b->h_sender[channel] = sender;
    b->assigned[sender]++;
}

extern "C" {

/*
 * Entry point                                  stands for (paths relative to the reference tree)
 *   spangpu_faxtx_create()                     the transmit half of fax_modems_init() x N                         src/fax_modems.c:618-677
 *   spangpu_faxtx_set_tx_type()                fax_set_tx_type()                                                  src/fax.c:327-421
 *                                              with fax_modems_start_slow_modem() / _start_fast_modem()           src/fax_modems.c:336-372, :375-513
 *   spangpu_faxtx_restart()                    fax_modems_restart()                                               src/fax_modems.c:611-615
 *   spangpu_faxtx_set_tep_mode()               fax_modems_set_tep_mode()                                          src/fax_modems.c:599-602
 *   spangpu_faxtx_tx()                         fax_tx() with transmit_on_idle, fax_modems_set_next_tx_type()      src/fax.c:221-256, src/fax_modems.c:581-596
 *   spangpu_faxtx_status()                     what fax_tx() returned, the t30_front_end_status() calls           src/fax.c:161-167, :234-235
 */

void spangpu_faxtx_destroy(spangpu_faxtx_t *b)
{
    if (b == NULL)
        return;
    // (the inner banks run on this bank's stream: they go first)
    spangpu_mcttx_destroy(b->tone[0]);
    spangpu_mcttx_destroy(b->tone[1]);
    spangpu_fsktx_destroy(b->v21);
    for (int i = 0;  i < 3;  i++)
        spangpu_modemtx_destroy(b->fast[i]);
    spangpu_hdlc_tx_destroy(b->framer);
    core_destroy(&b->c);
    free(b->h_sender);
    (void) hipFree(b->span);
    (void) hipFree(b->ret);
    (void) hipFree(b->cnt);
    (void) hipFree(b->pcm);
    counts_free(&b->out);
    free(b);
}

int spangpu_faxtx_create(spangpu_faxtx_t **out, int device, int n_channels, int kinds_mask, int max_samples, int use_tep)
{
    const int all = SPANGPU_FAXFE_V27TER | SPANGPU_FAXFE_V29 | SPANGPU_FAXFE_V17;
    if (out == NULL  ||  n_channels <= 0  ||  kinds_mask < 0  ||  (kinds_mask & ~all)  ||  max_samples <= 0  ||  max_samples > kMaxSamples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (kinds_mask: SPANGPU_FAXFE_V27TER | _V29 | _V17)");
    *out = NULL;
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_faxtx_s *b = (spangpu_faxtx_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    b->kinds_mask = kinds_mask;
    b->max_samples = max_samples;
    b->pcm_stride = ((long long) max_samples + 7) & ~7LL;
    if ((rc = core_create(&b->c, device, n_channels, kFaxTxWords)) != SPANGPU_OK)
    {
        spangpu_faxtx_destroy(b);
        return rc;
    }
    const size_t n = (size_t) n_channels;
    b->h_sender = (int32_t *) calloc(n, sizeof(int32_t));
    if (b->h_sender == NULL
        ||  hipMalloc(&b->span, kSpanRows*n*sizeof(int32_t)) != hipSuccess
        ||  hipMalloc(&b->ret, n*sizeof(int32_t)) != hipSuccess
        ||  hipMalloc(&b->cnt, 2*n*sizeof(int32_t)) != hipSuccess
        ||  counts_create(&b->c, &b->out, kFaxTxOutRows, kFaxTxOutRows) != SPANGPU_OK)
    {
        spangpu_faxtx_destroy(b);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the FAX transmit front-end bank failed");
    }
    b->assigned[kFaxTxSendNone] = n_channels;
    // fax_modems_init(): memset, silence_gen_init(0), silence_gen installed, transmit false
    int32_t one[kFaxTxWords];
    faxtx_words_init(one, use_tep);
    rc = core_fill(&b->c, one);
    // modem_connect_tones_tx_init(CNG) and fsk_tx_init(V.21 channel 2) as fax_modems_init() makes them, hdlc_tx_init(CRC-16, 2
    // flags between frames); the fast modems are made by the first set_tx_type that asks for them, so any rate will do here
    if (rc == SPANGPU_OK)
        rc = spangpu_mcttx_create(&b->tone[0], device, SPANGPU_MCT_ANS, n_channels);
    if (rc == SPANGPU_OK)
        rc = spangpu_mcttx_create(&b->tone[1], device, SPANGPU_MCT_FAX_CNG, n_channels);
    spangpu_fsk_spec_t spec;
    if (rc == SPANGPU_OK)
        rc = spangpu_fsk_preset(SPANGPU_FSK_V21CH2, &spec);
    if (rc == SPANGPU_OK)
        rc = spangpu_fsktx_create(&b->v21, device, n_channels, &spec, SPANGPU_FSKTX_LFSR, NULL, 0);
    if (rc == SPANGPU_OK)
        rc = spangpu_hdlc_tx_create(&b->framer, device, n_channels, 0, 2, 0, kQueueDepth);
    static const int senders[3] = {kFaxTxSendV27ter, kFaxTxSendV29, kFaxTxSendV17};
    static const int rates[3] = {4800, 9600, 14400};
    for (int i = 0;  i < 3  &&  rc == SPANGPU_OK;  i++)
    {
        if (kinds_mask & mask_of(senders[i]))
            rc = spangpu_modemtx_create_ex(&b->fast[i], device, modem_of(senders[i]), n_channels, rates[i], use_tep, SPANGPU_MODEMTX_QUEUE, NULL,
                                           kRingBits);
    }
    if (rc == SPANGPU_OK)
        rc = spangpu_faxtx_set_stream(b, (void *) b->c.stream);
    if (rc != SPANGPU_OK)
    {
        spangpu_faxtx_destroy(b);
        return rc;
    }
    *out = b;
    return SPANGPU_OK;
}

int spangpu_faxtx_channels(const spangpu_faxtx_t *b) { return b  ?  b->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_faxtx_state_words(const spangpu_faxtx_t *b) { return b  ?  b->c.words  :  SPANGPU_ERR_BAD_ARG; }

// Every inner bank follows: the tick is one sequence on one stream.
int spangpu_faxtx_set_stream(spangpu_faxtx_t *b, void *stream)
{
    if (b == NULL  ||  stream == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank, or the null stream");
    // the inner banks first: they wait on the stream they leave, which is this bank's until the last line here
    int rc = spangpu_mcttx_set_stream(b->tone[0], stream);
    if (rc == SPANGPU_OK)
        rc = spangpu_mcttx_set_stream(b->tone[1], stream);
    if (rc == SPANGPU_OK)
        rc = spangpu_fsktx_set_stream(b->v21, stream);
    for (int i = 0;  i < 3  &&  rc == SPANGPU_OK;  i++)
    {
        if (b->fast[i])
            rc = spangpu_modemtx_set_stream(b->fast[i], stream);
    }
    if (rc == SPANGPU_OK)
        rc = spangpu_hdlc_tx_set_stream(b->framer, stream);
    if (rc == SPANGPU_OK  &&  stream != (void *) b->c.stream)
        rc = core_set_stream(&b->c, stream);
    return rc;
}

int spangpu_faxtx_sync(spangpu_faxtx_t *b)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&b->c);
}

spangpu_hdlc_tx_t *spangpu_faxtx_framer(spangpu_faxtx_t *b) { return b  ?  b->framer  :  NULL; }
spangpu_fsktx_t *spangpu_faxtx_v21_bank(spangpu_faxtx_t *b) { return b  ?  b->v21  :  NULL; }

spangpu_modemtx_t *spangpu_faxtx_fast_bank(spangpu_faxtx_t *b, int kind)
{
    if (b == NULL)
        return NULL;
    return (kind == SPANGPU_V27TER)  ?  b->fast[0]  :  (kind == SPANGPU_V29)  ?  b->fast[1]  :  (kind == SPANGPU_V17)  ?  b->fast[2]  :  NULL;
}

spangpu_mcttx_t *spangpu_faxtx_tone_bank(spangpu_faxtx_t *b, int tone)
{
    if (b == NULL)
        return NULL;
    return (tone == SPANGPU_MCT_ANS)  ?  b->tone[0]  :  (tone == SPANGPU_MCT_FAX_CNG)  ?  b->tone[1]  :  NULL;
}

int spangpu_faxtx_get_words(spangpu_faxtx_t *b, int channel, int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, 0, kFaxTxWords, words, false);
}

int spangpu_faxtx_set_words(spangpu_faxtx_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    // a sender is reached from silence alone, and its bank exists: nothing else points a lane at a row
    const int handler = words[FX_HANDLER];
    const int next = words[FX_NEXT_HANDLER];
    const int sender = sender_of_words(words);
    const bool runs = (handler != kFaxTxSilence  ||  next != kFaxTxSilence);
    if (handler < kFaxTxSilence  ||  handler > kFaxTxFast  ||  next < kFaxTxSilence  ||  next > kFaxTxFast
        ||  (handler != kFaxTxSilence  &&  next != kFaxTxSilence)  ||  (runs  &&  sender == kFaxTxSendNone)
        ||  (sender >= kFaxTxSendV27ter  &&  (b->fast[sender - kFaxTxSendV27ter] == NULL  ||  !rate_ok(sender, words[FX_BIT_RATE])))
        ||  words[FX_SIL_REMAINING] < 0  ||  (words[FX_TONE] != 0  &&  words[FX_TONE] != kFaxTxSendCed  &&  words[FX_TONE] != kFaxTxSendCng))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "not the words of a channel of this bank");
    const int rc = core_rw_words(&b->c, channel, 0, kFaxTxWords, const_cast<int32_t *>(words), true);
    if (rc == SPANGPU_OK)
        assign(b, channel, sender);
    return rc;
}

int spangpu_faxtx_restart(spangpu_faxtx_t *b, int channel)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w = -1;
    return core_rw_words(&b->c, channel, FX_CURRENT_TX_TYPE, 1, &w, true);
}

int spangpu_faxtx_set_tep_mode(spangpu_faxtx_t *b, int channel, int on)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w = on  ?  1  :  0;
    return core_rw_words(&b->c, channel, FX_USE_TEP, 1, &w, true);
}

int spangpu_faxtx_set_tx_type(spangpu_faxtx_t *b, int channel, int type, int bit_rate, int short_train, int use_hdlc)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel)  ||  type < kT30None  ||  type > kT30Done)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (type: SPANGPU_T30_MODEM_*)");
    if (type == kT30V34hdx)
        return spangpu_set_error(SPANGPU_ERR_UNSUPPORTED, "a FAX transmit front-end bank has no V.34 sender");
    if (type == kT30Pause  &&  (short_train < 0  ||  short_train > (1 << 24)))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a pause of 0 .. 2^24 ms");
    if (type == kT30V27ter  ||  type == kT30V29  ||  type == kT30V17)
    {
        const int sender = (type == kT30V17)  ?  kFaxTxSendV17  :  (type == kT30V29)  ?  kFaxTxSendV29  :  kFaxTxSendV27ter;
        if (!(b->kinds_mask & mask_of(sender)))
            return spangpu_set_error(SPANGPU_ERR_UNSUPPORTED, "this bank was made without that kind of fast modem");
        if (!rate_ok(sender, bit_rate))
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bit rate not valid for this modem (V.29: 9600/7200/4800, V.27ter: 4800/2400, V.17: 14400/12000/9600/7200/4800)");
    }
    int32_t fx[kFaxTxWords];
    int rc = core_rw_words(&b->c, channel, 0, kFaxTxWords, fx, false);
    if (rc != SPANGPU_OK)
        return rc;
    FaxTxAct act;
    faxtx_set_tx_type(fx, type, bit_rate, short_train, use_hdlc, &act);
    if (!act.acted)
        return SPANGPU_OK;
    if (act.tone)
        rc = spangpu_mcttx_restart(b->tone[act.tone - kFaxTxSendCed], channel);
    if (act.v21)
    {
        spangpu_fsk_spec_t spec;
        (void) spangpu_fsk_preset(SPANGPU_FSK_V21CH2, &spec);
        rc = spangpu_fsktx_restart(b->v21, channel, &spec);
    }
    if (rc == SPANGPU_OK  &&  act.flags)
    {
        // hdlc_tx_flags() on the channel's own words, now; what is queued stays queued
        int32_t w[kHdlcTxWords];
        if ((rc = spangpu_hdlc_tx_get_state(b->framer, channel, w)) == SPANGPU_OK)
        {
            hdlc_tx_flags_now(w, act.flags);
            rc = spangpu_hdlc_tx_set_state(b->framer, channel, w);
        }
    }
    if (rc == SPANGPU_OK  &&  act.fast)
    {
        spangpu_modemtx_t *m = b->fast[act.fast - kFaxTxSendV27ter];
        if (act.fast_init)
            rc = spangpu_txline_modem_init(m, channel, bit_rate, fx[FX_USE_TEP]);
        else
            rc = spangpu_modemtx_restart_ex(m, channel, bit_rate, fx[FX_USE_TEP], (act.fast == kFaxTxSendV17)  ?  fx[FX_SHORT_TRAIN]  :  0);
    }
    if (rc < 0)
        return rc;
    if ((rc = core_rw_words(&b->c, channel, 0, kFaxTxWords, fx, true)) != SPANGPU_OK)
        return rc;
    assign(b, channel, sender_of_words(fx));
    return SPANGPU_OK;
}

int spangpu_faxtx_tx(spangpu_faxtx_t *b, int16_t *amp, int mem, int samples, long long stride)
{
    if (b == NULL  ||  amp == NULL  ||  samples <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (mem_kind_ok(mem) != SPANGPU_OK)
        return SPANGPU_ERR_BAD_ARG;
    if (stride <= 0)
        stride = samples;
    if (stride < samples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "stride < samples");
    if (samples > b->max_samples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "samples > max_samples");
    SPG_TRY(hipSetDevice(b->c.device));
    const size_t n = (size_t) b->c.n_ch;
    const bool host = (mem == SPANGPU_MEM_HOST);
    if (host  &&  b->pcm == NULL  &&  hipMalloc(&b->pcm, n*(size_t) b->pcm_stride*sizeof(int16_t)) != hipSuccess)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "row staging");
    FaxTxLaunch L;
    memset(&L, 0, sizeof(L));
    L.fx = b->c.st;
    L.n_ch = b->c.n_ch;
    L.samples = samples;
    L.span = b->span;
    L.ret = b->ret;
    L.cnt = b->cnt;
    L.out = b->out.dev;
    L.pcm = host  ?  b->pcm  :  amp;
    L.stride = host  ?  b->pcm_stride  :  stride;
    const dim3 grid((b->c.n_ch + 63)/64);
    // 1. the plan: the silence, and who is offered what is left of the row
    hipLaunchKernelGGL(faxtx_plan_kernel, grid, dim3(64), 0, b->c.stream, L);
    SPG_TRY(hipGetLastError());
    // 2. the senders that have a channel assigned, each over its channels' spans
    int rc;
    for (int i = 0;  i < 2;  i++)
    {
        if (b->assigned[kFaxTxSendCed + i] > 0
            &&  (rc = spangpu_txspans_mct(b->tone[i], L.pcm, L.stride, samples, b->span, kFaxTxSendCed + i, b->ret)) != SPANGPU_OK)
            return rc;
    }
    if (b->assigned[kFaxTxSendV21] > 0
        &&  (rc = spangpu_txspans_fsk(b->v21, L.pcm, L.stride, samples, b->span, kFaxTxSendV21, b->ret, b->framer, b->cnt)) != SPANGPU_OK)
        return rc;
    for (int i = 0;  i < 3;  i++)
    {
        if (b->fast[i]  &&  b->assigned[kFaxTxSendV27ter + i] > 0
            &&  (rc = spangpu_txspans_modem(b->fast[i], L.pcm, L.stride, samples, b->span, kFaxTxSendV27ter + i, b->ret, b->framer,
                                                   b->c.st + (size_t) FX_HDLC_MODE*n, b->cnt)) != SPANGPU_OK)
            return rc;
    }
    // 3. what they returned: the short return, the next handler, the reports, the zeros
    hipLaunchKernelGGL(faxtx_resolve_kernel, grid, dim3(64), 0, b->c.stream, L);
    SPG_TRY(hipGetLastError());
    b->ran = true;
    if (host)
    {
        SPG_TRY(hipMemcpy2DAsync(amp, (size_t) stride*sizeof(int16_t), b->pcm, (size_t) b->pcm_stride*sizeof(int16_t), (size_t) samples*sizeof(int16_t),
                                 n, hipMemcpyDeviceToHost, b->c.stream));
        SPG_TRY(hipStreamSynchronize(b->c.stream));
    }
    return SPANGPU_OK;
}

int spangpu_faxtx_status(spangpu_faxtx_t *b, int32_t *lens, int32_t *steps, int32_t *underflows, int32_t *handler, int32_t *transmit)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    if (!b->ran)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no spangpu_faxtx_tx() yet");
    const int rc = counts_fetch(&b->c, &b->out, kFaxTxOutRows);
    if (rc != SPANGPU_OK)
        return rc;
    const size_t n = (size_t) b->c.n_ch;
    int32_t *rows[kFaxTxOutRows] = {lens, steps, underflows, handler, transmit};
    for (int i = 0;  i < kFaxTxOutRows;  i++)
    {
        if (rows[i])
            memcpy(rows[i], b->out.pinned + (size_t) i*n, n*sizeof(int32_t));
    }
    return SPANGPU_OK;
}

}   // extern "C"
