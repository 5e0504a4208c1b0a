// modemtx_api.hip -- C ABI of the modem transmitter banks (include/spangpu.h, "modem transmitter banks"): batched
// v29_tx() / v27ter_tx() / v17_tx() as device-side signal sources, carrying an LFSR's bits or the caller's (a bit ring per
// channel, with the end-of-data shutdown).  Device code: modemtx_dev.hpp.  No CPU implementation of the modulators exists
// behind these entry points; the cursor at the end is plain host code.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#define SPG_HDLC_STEP_FUNCTIONS_ONLY        // the HDLC banks' own kernels belong to hdlc_api.hip
#include "modem_tables.h"
#include "modemtx_dev.hpp"
#include "bank_host.hpp"

using namespace spg;

struct spangpu_modemtx_s
{
    BankCore c;             // st[kV29TxWords][n_ch]
    PcmStage pcm;           // d_lens: only once a host caller of a queue-sourced bank asks for lengths
    int kind;               // kTxV29, kTxV27ter or kTxV17
    float *constel;         // V.17: the constellations of every rate + the ABCD training points
    float *sine;
    float *shaper;
    int source;             // kTxSrcLfsr or kTxSrcQueue
    int qcap;               // bits a channel's ring takes
    int qring;              // ring size in bits: qcap rounded up to whole words
    uint32_t *queue;
    int32_t *qst;           // [kVqWords][n_ch]
    int32_t *h_row;         // [5][n_ch] host scratch: the events as channels [2n], kinds [2n], and the flags read back [n]
    BitPut put;             // staging of spangpu_modemtx_put_bits()
};

static void put_f(int32_t *w, int idx, float v)
{
    memcpy(w + idx, &v, sizeof(float));
}

static float get_f(const int32_t *w, int idx)
{
    float v;
    memcpy(&v, w + idx, sizeof(float));
    return v;
}

static void gain_words(int32_t *w, int kind)
{
    if (kind != kTxV29)
        return;             // V.27ter keeps one gain per rate, V.17 one gain; both are set by xxx_tx_power()
    // set_working_gain(), v29tx.c:286-320
    const float base = get_f(w, VT_BASE_GAIN);
    switch (w[VT_BIT_RATE])
    {
    case 9600: put_f(w, VT_GAIN, 0.387f*base); break;
    case 7200: put_f(w, VT_GAIN, 0.605f*base); break;
    case 4800: put_f(w, VT_GAIN, 0.470f*base); break;
    }
}

static void power_words(int32_t *w, int kind, float power)
{
    if (kind == kTxV29)
    {
        // v29_tx_power(), v29tx.c:322-338; TX_PULSESHAPER_GAIN = 1.0f in the float build
        put_f(w, VT_BASE_GAIN, spg_db_to_amplitude_ratio(power - 3.14f)*32768.0f/1.000000f);
        gain_words(w, kind);
        return;
    }
    if (kind == kTxV17)
    {
        // v17_tx_power(), v17tx.c:371-383
        put_f(w, VT_BASE_GAIN, 0.223f*spg_db_to_amplitude_ratio(power - 3.14f)*32768.0f/1.000000f);
        return;
    }
    // v27ter_tx_power(), v27ter_tx.c:352-364: gain_2400 (word 1) and gain_4800 (word 2), both shaper gains 1.0f
    const float gain = spg_db_to_amplitude_ratio(power - 3.14f)*32768.0f;
    put_f(w, VT_BASE_GAIN, gain/1.000000f);
    put_f(w, VT_GAIN, gain/1.000000f);
}

static int restart_words(int32_t *w, int kind, int bit_rate, int tep, int short_train = 0)
{
    if (kind == kTxV17)
    {
        // v17_tx_restart(), v17tx.c:397-450
        if (bit_rate != 14400  &&  bit_rate != 12000  &&  bit_rate != 9600  &&  bit_rate != 7200  &&  bit_rate != 4800)
            return -1;
        w[VT_BIT_RATE] = bit_rate;
        w[VT_GAIN] = short_train  ?  0  :  1;          // diff
        for (int i = 0;  i < 18;  i++)
            w[VT_RRC_RE + i] = 0;
        w[VT_RRC_STEP] = 0;
        w[VT_TRAIN_SCRAMBLE] = 0;                       // convolution
        w[VT_SCRAMBLE] = 0x2ECDD5;
        w[VT_IN_TRAINING] = 1;
        w[VT_TRAINING_OFFSET] = short_train  ?  1  :  0;
        w[VT_TRAINING_STEP] = tep  ?  0  :  kV17Seg1;
        w[VT_CARRIER_PHASE] = 0;
        w[VT_BAUD_PHASE] = 0;
        w[VT_CONSTELLATION] = 0;
        return 0;
    }
    if (kind == kTxV27ter)
    {
        // v27ter_tx_restart(), v27ter_tx.c:384-409
        if (bit_rate != 4800  &&  bit_rate != 2400)
            return -1;
        w[VT_BIT_RATE] = bit_rate;
        for (int i = 0;  i < 18;  i++)
            w[VT_RRC_RE + i] = 0;
        w[VT_RRC_STEP] = 0;
        w[VT_SCRAMBLE] = 0x3C;
        w[VT_TRAIN_SCRAMBLE] = 0;               // scrambler_pattern_count
        w[VT_IN_TRAINING] = 1;
        w[VT_TRAINING_STEP] = tep  ?  0  :  kV27Seg2;
        w[VT_CARRIER_PHASE] = 0;
        w[VT_BAUD_PHASE] = 0;
        w[VT_CONSTELLATION] = 0;
        return 0;
    }
    // v29_tx_restart(), v29tx.c:365-404
    if (bit_rate != 9600  &&  bit_rate != 7200  &&  bit_rate != 4800)
        return -1;
    w[VT_BIT_RATE] = bit_rate;
    gain_words(w, kind);
    switch (bit_rate)
    {
    case 9600: w[VT_TRAINING_OFFSET] = 0; break;
    case 7200: w[VT_TRAINING_OFFSET] = 2; break;
    case 4800: w[VT_TRAINING_OFFSET] = 4; break;
    default: return -1;
    }
    for (int i = 0;  i < 18;  i++)
        w[VT_RRC_RE + i] = 0;
    w[VT_RRC_STEP] = 0;
    w[VT_SCRAMBLE] = 0;
    w[VT_TRAIN_SCRAMBLE] = 0x2A;
    w[VT_IN_TRAINING] = 1;
    w[VT_TRAINING_STEP] = tep  ?  0  :  kVtSeg1;
    w[VT_CARRIER_PHASE] = 0;
    w[VT_BAUD_PHASE] = 0;
    w[VT_CONSTELLATION] = 0;
    return 0;
}

template <int SRC>
static void launch_bank(spangpu_modemtx_s *t, const V29TxLaunch &L)
{
    if (t->kind == kTxV29)
        hipLaunchKernelGGL((modemtx_bank_kernel<kTxV29, SRC>), dim3((t->c.n_ch + 63)/64), dim3(64), 0, t->c.stream, L);
    else if (t->kind == kTxV17)
        hipLaunchKernelGGL((modemtx_bank_kernel<kTxV17, SRC>), dim3((t->c.n_ch + 63)/64), dim3(64), 0, t->c.stream, L);
    else
        hipLaunchKernelGGL((modemtx_bank_kernel<kTxV27ter, SRC>), dim3((t->c.n_ch + 63)/64), dim3(64), 0, t->c.stream, L);
}

extern "C" {

int spangpu_modemtx_create(spangpu_modemtx_t **out, int device, int modem, int n_channels, int bit_rate, int tep, const uint32_t *seeds)
{
    return spangpu_modemtx_create_ex(out, device, modem, n_channels, bit_rate, tep, SPANGPU_MODEMTX_LFSR, seeds, 0);
}

int spangpu_modemtx_create_ex(spangpu_modemtx_t **out, int device, int modem, int n_channels, int bit_rate, int tep, int bit_source,
                              const uint32_t *seeds, int queue_bits)
{
    if (out == NULL  ||  n_channels <= 0  ||  (modem != SPANGPU_V29  &&  modem != SPANGPU_V27TER  &&  modem != SPANGPU_V17))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (modem SPANGPU_V29, SPANGPU_V27TER or SPANGPU_V17)");
    if ((bit_source != SPANGPU_MODEMTX_LFSR  &&  bit_source != SPANGPU_MODEMTX_QUEUE)
        ||  (bit_source == SPANGPU_MODEMTX_QUEUE  &&  (queue_bits <= 0  ||  queue_bits > (1 << 24))))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bit source, queue_bits 1 .. 2^24)");
    const int kind = (modem == SPANGPU_V29)  ?  kTxV29  :  ((modem == SPANGPU_V27TER)  ?  kTxV27ter  :  kTxV17);
    int32_t probe[kV29TxWords];
    memset(probe, 0, sizeof(probe));
    if (restart_words(probe, kind, bit_rate, tep) != 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bit rate not valid for this modem (V.29: 9600/7200/4800, V.27ter: 4800/2400, V.17: 14400/12000/9600/7200/4800)");
    *out = NULL;
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_modemtx_s *t = (spangpu_modemtx_s *) calloc(1, sizeof(*t));
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    t->kind = kind;
    t->source = (bit_source == SPANGPU_MODEMTX_LFSR)  ?  kTxSrcLfsr  :  kTxSrcQueue;
    if ((rc = core_create(&t->c, device, n_channels, kV29TxWords)) != SPANGPU_OK)
    {
        spangpu_modemtx_destroy(t);
        return rc;
    }
    if (hipMalloc(&t->sine, 2048*sizeof(float)) != hipSuccess
        ||  hipMalloc(&t->shaper, 225*sizeof(float)) != hipSuccess
        ||  hipMalloc(&t->constel, 496*sizeof(float)) != hipSuccess)
    {
        spangpu_modemtx_destroy(t);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the V.29 transmitter bank failed");
    }
    if (t->source == kTxSrcQueue)
    {
        t->qcap = queue_bits;
        t->qring = (queue_bits + 31) & ~31;
        const size_t ring_bytes = (size_t) (t->qring/32)*n_channels*sizeof(uint32_t);
        const size_t q_bytes = (size_t) kVqWords*n_channels*sizeof(int32_t);
        t->h_row = (int32_t *) malloc((size_t) 5*n_channels*sizeof(int32_t));
        if (t->h_row == NULL
            ||  hipMalloc(&t->queue, ring_bytes) != hipSuccess  ||  hipMemset(t->queue, 0, ring_bytes) != hipSuccess
            ||  hipMalloc(&t->qst, q_bytes) != hipSuccess  ||  hipMemset(t->qst, 0, q_bytes) != hipSuccess)
        {
            spangpu_modemtx_destroy(t);
            return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the bit rings failed");
        }
    }
    float sine[2048];
    float shaper[225];
    memset(shaper, 0, sizeof(shaper));
    spg_make_sine_table(sine);
    // make_modem_filter -t: V.29 10 phases x 9 taps, excess bandwidth 0.25; V.27ter 4800 bps 5 x 9 and 2400 bps
    // 20 x 9, excess bandwidth 0.5 (make_modem_filter.c:375-412)
    // V.17 shapes with the V.29 parameters (make_modem_filter.c:319-331)
    if (((kind != kTxV27ter)  ?  spg_make_tx_pulseshaper(10, 9, 0.25, shaper)
                           :  (spg_make_tx_pulseshaper(5, 9, 0.5, shaper) | spg_make_tx_pulseshaper(20, 9, 0.5, shaper + 45))) != 0)
    {
        spangpu_modemtx_destroy(t);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "table scratch");
    }
    // v29_tx_init(), v29tx.c:406-434 / v27ter_tx_init(), v27ter_tx.c:411-437
    int32_t one[kV29TxWords];
    memset(one, 0, sizeof(one));
    one[VT_BIT_RATE] = bit_rate;
    one[VT_CARRIER_RATE] = spg_dds_phase_ratef((kind == kTxV29)  ?  1700.0f  :  1800.0f);
    // the V.17 constellations (v17_v32bis_tx_constellation_maps.h) and the ABCD training points (:314-323)
    float constel[496];
    memset(constel, 0, sizeof(constel));
    {
        static const int rates[5] = {14400, 12000, 9600, 7200, 4800};
        static const float abcd[8] = {-6.0f, -2.0f, 2.0f, -6.0f, 6.0f, 2.0f, -2.0f, 6.0f};
        int at = 0;
        for (int r = 0;  r < 5;  r++)
        {
            int8_t pts[128][2];
            const int np = spg_make_v17_constellation(rates[r], pts);
            for (int i = 0;  i < np;  i++)
            {
                constel[2*(at + i)] = (float) pts[i][0];
                constel[2*(at + i) + 1] = (float) pts[i][1];
            }
            at += np;
        }
        memcpy(constel + 2*at, abcd, sizeof(abcd));
    }
    power_words(one, kind, -14.0f);
    restart_words(one, kind, bit_rate, tep);
    // every channel starts from the same words, but for the seed of its LFSR
    int32_t *seed_row = (int32_t *) malloc((size_t) n_channels*sizeof(int32_t));
    if (seed_row == NULL)
    {
        spangpu_modemtx_destroy(t);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "malloc");
    }
    for (int c = 0;  c < n_channels;  c++)
        seed_row[c] = (int32_t) ((seeds  ?  seeds[c]  :  (uint32_t) (c*2654435761u + 1u)) & 0x7FFFu);
    rc = core_fill(&t->c, one);
    hipError_t e = hipSuccess;
    if (rc == SPANGPU_OK)
        e = hipMemcpy(t->c.st + (size_t) VT_PRBS*n_channels, seed_row, (size_t) n_channels*sizeof(int32_t), hipMemcpyHostToDevice);
    free(seed_row);
    if (e == hipSuccess)
        e = hipMemcpy(t->sine, sine, sizeof(sine), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(t->shaper, shaper, sizeof(shaper), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(t->constel, constel, sizeof(constel), hipMemcpyHostToDevice);
    if (rc == SPANGPU_OK  &&  e != hipSuccess)
        rc = spangpu_set_error(SPANGPU_ERR_HIP, "state upload failed");
    if (rc != SPANGPU_OK)
    {
        spangpu_modemtx_destroy(t);
        return rc;
    }
    *out = t;
    return SPANGPU_OK;
}

void spangpu_modemtx_destroy(spangpu_modemtx_t *t)
{
    if (t == NULL)
        return;
    core_destroy(&t->c);
    stage_free(&t->pcm);
    bitput_free(&t->put);
    (void) hipFree(t->sine);
    (void) hipFree(t->shaper);
    (void) hipFree(t->constel);
    (void) hipFree(t->queue);
    (void) hipFree(t->qst);
    free(t->h_row);
    free(t);
}

int spangpu_modemtx_channels(const spangpu_modemtx_t *t) { return t  ?  t->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_modemtx_state_words(void) { return kV29TxWords; }

int spangpu_modemtx_set_stream(spangpu_modemtx_t *t, void *stream)
{
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&t->c, stream);
}

int spangpu_modemtx_sync(spangpu_modemtx_t *t)
{
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&t->c);
}

int spangpu_modemtx_power(spangpu_modemtx_t *t, int channel, float power_dbm0)
{
    if (t == NULL  ||  !channel_ok(&t->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w[kV29TxWords];
    int rc = core_rw_words(&t->c, channel, 0, kV29TxWords, w, false);
    if (rc != SPANGPU_OK)
        return rc;
    power_words(w, t->kind, power_dbm0);
    return core_rw_words(&t->c, channel, 0, kV29TxWords, w, true);
}

// Every channel's level and carrier frequency in one pass over the state words: a population of lines for the receiver
// banks' workloads (carrier 1700 Hz +- 7 Hz, level -30 .. -10 dBm0).  The level is xxx_tx_power()'s; the
// carrier frequency is not something the reference's modulator lets a caller choose (v29tx.c:431 fixes it) -- it stands for the
// frequency shift of the line between the modems.
int spangpu_modemtx_line(spangpu_modemtx_t *t, const float *power_dbm0, const float *carrier_hz)
{
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    if (power_dbm0 == NULL  &&  carrier_hz == NULL)
        return SPANGPU_OK;
    for (int c = 0;  carrier_hz  &&  c < t->c.n_ch;  c++)
    {
        if (!(carrier_hz[c] > 0.0f  &&  carrier_hz[c] < 4000.0f))
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "carrier frequency out of range");
    }
    SPG_TRY(hipSetDevice(t->c.device));
    SPG_TRY(hipStreamSynchronize(t->c.stream));
    const size_t n = (size_t) t->c.n_ch;
    int32_t *host = (int32_t *) malloc((size_t) kV29TxWords*n*sizeof(int32_t));
    if (host == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "malloc");
    hipError_t e = hipMemcpy(host, t->c.st, (size_t) kV29TxWords*n*sizeof(int32_t), hipMemcpyDeviceToHost);
    for (int c = 0;  e == hipSuccess  &&  c < t->c.n_ch;  c++)
    {
        int32_t w[kV29TxWords];
        for (int k = 0;  k < kV29TxWords;  k++)
            w[k] = host[(size_t) k*n + c];
        if (power_dbm0)
            power_words(w, t->kind, power_dbm0[c]);
        if (carrier_hz)
            w[VT_CARRIER_RATE] = spg_dds_phase_ratef(carrier_hz[c]);
        for (int k = 0;  k < kV29TxWords;  k++)
            host[(size_t) k*n + c] = w[k];
    }
    if (e == hipSuccess)
        e = hipMemcpy(t->c.st, host, (size_t) kV29TxWords*n*sizeof(int32_t), hipMemcpyHostToDevice);
    free(host);
    if (e != hipSuccess)
        return spangpu_set_error(SPANGPU_ERR_HIP, "state transfer failed");
    return SPANGPU_OK;
}

int spangpu_modemtx_restart(spangpu_modemtx_t *t, int channel, int bit_rate, int tep)
{
    return spangpu_modemtx_restart_ex(t, channel, bit_rate, tep, 0);
}

int spangpu_modemtx_restart_ex(spangpu_modemtx_t *t, int channel, int bit_rate, int tep, int short_train)
{
    if (t == NULL  ||  !channel_ok(&t->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w[kV29TxWords];
    int rc = core_rw_words(&t->c, channel, 0, kV29TxWords, w, false);
    if (rc != SPANGPU_OK)
        return rc;
    if (restart_words(w, t->kind, bit_rate, tep, short_train) != 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bit rate not valid for this modem");
    if ((rc = core_rw_words(&t->c, channel, 0, kV29TxWords, w, true)) != SPANGPU_OK  ||  t->source != kTxSrcQueue)
        return rc;
    // a fresh sender has nothing queued and has not been told of the end of its data (as fsk_tx_restart() of the FSK objects)
    int32_t q[VQ_EOD + 1] = {0, 0, 0};
    return core_rw_at(&t->c, t->qst, channel, VQ_RD, VQ_EOD + 1, q, true);
}

int spangpu_modemtx_get_state(spangpu_modemtx_t *t, int channel, int32_t *words)
{
    if (t == NULL  ||  words == NULL  ||  !channel_ok(&t->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&t->c, channel, 0, kV29TxWords, words, false);
}

static int tx_call(spangpu_modemtx_t *t, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens, int more);

int spangpu_modemtx_tx(spangpu_modemtx_t *t, int mem_kind, int16_t *pcm, long long stride, int samples)
{
    return spangpu_modemtx_tx_lens(t, mem_kind, pcm, stride, samples, NULL);
}

int spangpu_modemtx_tx_lens(spangpu_modemtx_t *t, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    return tx_call(t, mem_kind, pcm, stride, samples, lens, 0);
}

int spangpu_modemtx_tx_continue(spangpu_modemtx_t *t, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    return tx_call(t, mem_kind, pcm, stride, samples, lens, 1);
}

static int tx_call(spangpu_modemtx_t *t, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens, int more)
{
    int rc = tx_args_ok(t, mem_kind, pcm, stride, samples);
    if (rc != SPANGPU_OK)
        return rc;
    SPG_TRY(hipSetDevice(t->c.device));
    const bool host = (mem_kind == SPANGPU_MEM_HOST);
    const bool queue = (t->source == kTxSrcQueue);
    if (samples == 0)
    {
        // xxx_tx(s, amp, 0) returns 0 and touches nothing; no channel has an event
        // (an empty call zeroes the lens of a device caller too and clears the event flags; the other senders do neither)
        if (queue)
            SPG_TRY(hipMemsetAsync(t->qst + (size_t) VQ_EVENT*t->c.n_ch, 0, (size_t) t->c.n_ch*sizeof(int32_t), t->c.stream));
        if (lens  &&  host)
            memset(lens, 0, (size_t) t->c.n_ch*sizeof(int32_t));
        else if (lens)
            SPG_TRY(hipMemsetAsync(lens, 0, (size_t) t->c.n_ch*sizeof(int32_t), t->c.stream));
        return 0;
    }
    // the kernel reports lengths only where they can differ: a queue-sourced bank whose caller asks for them
    int32_t *want = queue  ?  lens  :  NULL;
    if (want  &&  host  &&  (rc = stage_lens(&t->c, &t->pcm)) != SPANGPU_OK)
        return rc;
    V29TxLaunch L;
    memset(&L, 0, sizeof(L));
    L.st = t->c.st;
    L.sine = t->sine;
    L.shaper = t->shaper;
    L.constel = t->constel;
    L.n_ch = t->c.n_ch;
    L.samples = samples;
    if ((rc = stage_out_target(&t->c, &t->pcm, mem_kind, pcm, stride, samples, want, &L.pcm, &L.stride, &L.lens, &L.vec)) != SPANGPU_OK)
        return rc;
    if (queue)
    {
        L.qring = t->qring;
        L.more = more;
        L.queue = t->queue;
        L.qst = t->qst;
        L.lens = want  ?  L.lens  :  NULL;
        launch_bank<kTxSrcQueue>(t, L);
    }
    else
    {
        L.lens = NULL;
        launch_bank<kTxSrcLfsr>(t, L);
        // an LFSR never runs out of bits: no channel of such a bank shuts down
        if (lens  &&  !host)
            SPG_TRY(hipMemsetD32Async((hipDeviceptr_t) lens, samples, (size_t) t->c.n_ch, t->c.stream));
    }
    SPG_TRY(hipGetLastError());
    if ((rc = stage_out_back(&t->c, &t->pcm, mem_kind, pcm, stride, samples, want)) != SPANGPU_OK)
        return rc;
    for (int c = 0;  lens  &&  host  &&  !queue  &&  c < t->c.n_ch;  c++)
        lens[c] = samples;
    // (the modem senders return the length of the call, as xxx_tx() does; every other sender returns SPANGPU_OK)
    return samples;
}

// (what the HDLC sender bank's unit hands to the units whose kernels call hdlc_tx_get_bit() themselves; not part of the ABI)
extern "C" void spangpu_hdlc_tx_rows(spangpu_hdlc_tx_t *b, int32_t **st, uint32_t **buf, int32_t **q_hdr, uint32_t **q_data, int *depth);

// One xxx_tx() call per channel over its own span of the row (txspan_dev.hpp), everything in device memory, nothing waited for.
int spangpu_txspans_modem(spangpu_modemtx_t *t, int16_t *pcm, long long stride, int samples, const int32_t *spans, int sender,
                                 int32_t *ret, spangpu_hdlc_tx_t *framer, const int32_t *hdlc_mode, int32_t *counts)
{
    int rc = tx_args_ok(t, SPANGPU_MEM_DEVICE, pcm, stride, samples);
    if (rc != SPANGPU_OK)
        return rc;
    if (t->source != kTxSrcQueue  ||  spans == NULL  ||  ret == NULL  ||  framer == NULL  ||  hdlc_mode == NULL  ||  counts == NULL
        ||  spangpu_hdlc_tx_channels(framer) != t->c.n_ch)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source, a framer of as many channels)");
    if (samples == 0)
        return SPANGPU_OK;
    SPG_TRY(hipSetDevice(t->c.device));
    V29TxLaunch L;
    memset(&L, 0, sizeof(L));
    L.st = t->c.st;
    L.sine = t->sine;
    L.shaper = t->shaper;
    L.constel = t->constel;
    L.n_ch = t->c.n_ch;
    L.samples = samples;
    L.pcm = pcm;
    L.stride = stride;
    L.qring = t->qring;
    L.queue = t->queue;
    L.qst = t->qst;
    L.sp.span = spans;
    L.sp.id = sender;
    L.sp.ret = ret;
    uint32_t *q_data;
    spangpu_hdlc_tx_rows(framer, &L.sp.hst, &L.sp.hbuf, &L.sp.q_hdr, &q_data, &L.sp.depth);
    L.sp.q_data = q_data;
    L.sp.mode = hdlc_mode;
    L.sp.cnt = counts;
    launch_bank<kTxSrcFax>(t, L);
    SPG_TRY(hipGetLastError());
    return SPANGPU_OK;
}

// xxx_tx_init() of one channel: the words spangpu_modemtx_create_ex() would give it, and an empty ring
int spangpu_txline_modem_init(spangpu_modemtx_t *t, int channel, int bit_rate, int tep)
{
    if (t == NULL  ||  !channel_ok(&t->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w[kV29TxWords];
    memset(w, 0, sizeof(w));
    w[VT_BIT_RATE] = bit_rate;
    w[VT_CARRIER_RATE] = spg_dds_phase_ratef((t->kind == kTxV29)  ?  1700.0f  :  1800.0f);
    power_words(w, t->kind, -14.0f);
    if (restart_words(w, t->kind, bit_rate, tep) != 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bit rate not valid for this modem");
    int rc = core_rw_words(&t->c, channel, 0, kV29TxWords, w, true);
    if (rc != SPANGPU_OK  ||  t->source != kTxSrcQueue)
        return rc;
    int32_t q[VQ_EOD + 1] = {0, 0, 0};
    return core_rw_at(&t->c, t->qst, channel, VQ_RD, VQ_EOD + 1, q, true);
}

int spangpu_txline_modem_set_state(spangpu_modemtx_t *t, int channel, const int32_t *words)
{
    if (t == NULL  ||  words == NULL  ||  !channel_ok(&t->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    // (what indexes a table: the rate picks the constellation and the shaper, the ring position and the baud phase the coefficients)
    int32_t probe[kV29TxWords];
    memcpy(probe, words, sizeof(probe));
    const int period = (t->kind != kTxV27ter)  ?  10  :  (words[VT_BIT_RATE] == 4800)  ?  5  :  20;
    if (restart_words(probe, t->kind, words[VT_BIT_RATE], 0) != 0  ||  words[VT_RRC_STEP] < 0  ||  words[VT_RRC_STEP] >= 9
        ||  words[VT_BAUD_PHASE] < 0  ||  words[VT_BAUD_PHASE] >= period  ||  (t->kind == kTxV17  &&  (words[VT_GAIN] & ~3))
        ||  (t->kind == kTxV17  &&  (words[VT_TRAIN_SCRAMBLE] & ~7)))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "not the words of a channel of this bank");
    return core_rw_words(&t->c, channel, 0, kV29TxWords, const_cast<int32_t *>(words), true);
}

// the ring of one channel: VQ_RD, VQ_COUNT, VQ_EOD, then the ring's words (qring/32 of them); write: the same back
int spangpu_txline_modem_ring_words(const spangpu_modemtx_t *t)
{
    return (t == NULL  ||  t->source != kTxSrcQueue)  ?  SPANGPU_ERR_BAD_ARG  :  (3 + t->qring/32);
}

int spangpu_txline_modem_ring_rw(spangpu_modemtx_t *t, int channel, int32_t *words, int write)
{
    if (t == NULL  ||  words == NULL  ||  !channel_ok(&t->c, channel)  ||  t->source != kTxSrcQueue)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    if (write  &&  (words[0] < 0  ||  words[0] >= t->qring  ||  words[1] < 0  ||  words[1] > t->qcap))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "not the ring of a channel of this bank");
    int rc = core_rw_at(&t->c, t->qst, channel, VQ_RD, 3, words, write != 0);
    if (rc == SPANGPU_OK)
        rc = core_rw_at(&t->c, (int32_t *) t->queue, channel, 0, t->qring/32, words + 3, write != 0);
    return rc;
}

int spangpu_modemtx_put_bits(spangpu_modemtx_t *t, int first, int n, const uint8_t *bits, int stride, const int32_t *lens, int32_t *accepted)
{
    if (t == NULL  ||  t->source != kTxSrcQueue)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    return bitring_put(&t->c, &t->put, t->qst + (size_t) VQ_RD*t->c.n_ch, t->qst + (size_t) VQ_COUNT*t->c.n_ch, t->queue, t->qring,
                       t->qcap, first, n, bits, stride, lens, accepted);
}

// spangpu_modemtx_put_bits() from rows and lengths in device memory (another bank's output): no copy, no wait
int spangpu_bits_to_modemtx(spangpu_modemtx_t *t, int first, int n, const uint8_t *dev_bits, int stride, const int32_t *dev_lens,
                                    int32_t *dev_accepted)
{
    if (t == NULL  ||  t->source != kTxSrcQueue)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    return bitring_put_device(&t->c, &t->put, t->qst + (size_t) VQ_RD*t->c.n_ch, t->qst + (size_t) VQ_COUNT*t->c.n_ch, t->queue, t->qring,
                              t->qcap, first, n, dev_bits, stride, dev_lens, dev_accepted);
}

int spangpu_modemtx_queued(spangpu_modemtx_t *t, int channel)
{
    if (t == NULL  ||  !channel_ok(&t->c, channel)  ||  t->source != kTxSrcQueue)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    int32_t w = 0;
    const int rc = core_rw_at(&t->c, t->qst, channel, VQ_COUNT, 1, &w, false);
    return (rc != SPANGPU_OK)  ?  rc  :  w;
}

int spangpu_modemtx_end_of_data(spangpu_modemtx_t *t, int channel, int on)
{
    if (t == NULL  ||  !channel_ok(&t->c, channel)  ||  t->source != kTxSrcQueue)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    int32_t w = on  ?  1  :  0;
    return core_rw_at(&t->c, t->qst, channel, VQ_EOD, 1, &w, true);
}

int spangpu_modemtx_events(spangpu_modemtx_t *t, const int32_t **channels, const int32_t **kinds)
{
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    if (channels)
        *channels = NULL;
    if (kinds)
        *kinds = NULL;
    if (t->source != kTxSrcQueue)
        return 0;
    const int n = t->c.n_ch;
    int32_t *chans = t->h_row;                      // a channel has at most two events in a call
    int32_t *kind = t->h_row + (size_t) 2*n;
    int32_t *flags = t->h_row + (size_t) 4*n;
    SPG_TRY(hipSetDevice(t->c.device));
    SPG_TRY(hipMemcpyAsync(flags, t->qst + (size_t) VQ_EVENT*n, (size_t) n*sizeof(int32_t), hipMemcpyDeviceToHost, t->c.stream));
    SPG_TRY(hipStreamSynchronize(t->c.stream));
    int count = 0;
    for (int c = 0;  c < n;  c++)
    {
        // the reference's order: the end of the data, then (in a long call) the end of the shutdown it starts
        if (flags[c] & kVqEndOfData)
        {
            chans[count] = c;
            kind[count++] = SPANGPU_MODEMTX_END_OF_DATA;
        }
        if (flags[c] & kVqShutdownComplete)
        {
            chans[count] = c;
            kind[count++] = SPANGPU_MODEMTX_SHUTDOWN_COMPLETE;
        }
    }
    if (channels)
        *channels = chans;
    if (kinds)
        *kinds = kind;
    return count;
}

// ---- host code: the cursor.  The bookkeeping of getbaud() without the signal: which bauds ask the caller for bits ----

int spangpu_modemtx_cursor_init(spangpu_modemtx_cursor_t *cur, int modem, int bit_rate, int tep, int short_train)
{
    if (cur == NULL  ||  (modem != SPANGPU_V29  &&  modem != SPANGPU_V27TER  &&  modem != SPANGPU_V17))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (modem SPANGPU_V29, SPANGPU_V27TER or SPANGPU_V17)");
    const int kind = (modem == SPANGPU_V29)  ?  kTxV29  :  ((modem == SPANGPU_V27TER)  ?  kTxV27ter  :  kTxV17);
    int32_t w[kV29TxWords];
    memset(w, 0, sizeof(w));
    if (restart_words(w, kind, bit_rate, tep, short_train) != 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bit rate not valid for this modem");
    cur->modem = modem;
    cur->bit_rate = bit_rate;
    cur->short_train = (kind == kTxV17  &&  short_train)  ?  1  :  0;
    cur->baud_phase = w[VT_BAUD_PHASE];
    cur->training_step = w[VT_TRAINING_STEP];
    cur->in_training = w[VT_IN_TRAINING];
    return SPANGPU_OK;
}

long long spangpu_modemtx_cursor_advance(spangpu_modemtx_cursor_t *cur, int samples, long long bits_before_end)
{
    if (cur == NULL  ||  samples < 0  ||  (cur->modem != SPANGPU_V29  &&  cur->modem != SPANGPU_V27TER  &&  cur->modem != SPANGPU_V17))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int modem = cur->modem;
    const int rate = cur->bit_rate;
    int step = 3;
    int period = 10;            // V.29, V.17: 2400 baud
    int bits_per_baud;
    int shutdown_end;
    if (modem == SPANGPU_V29)
    {
        bits_per_baud = (rate == 9600)  ?  4  :  ((rate == 7200)  ?  3  :  2);
        shutdown_end = kVtShutdownEnd;
    }
    else if (modem == SPANGPU_V27TER)
    {
        step = (rate == 4800)  ?  1  :  3;              // 1600 baud, 1200 baud
        period = (rate == 4800)  ?  5  :  20;
        bits_per_baud = (rate == 4800)  ?  3  :  2;
        shutdown_end = kV27ShutdownEnd;
    }
    else
    {
        bits_per_baud = rate/2400;
        shutdown_end = kV17ShutdownEnd;
    }
    // the test at the start of xxx_tx(), v29tx.c:241
    if (cur->training_step >= shutdown_end)
        return 0;
    long long calls = 0;
    for (int i = 0;  i < samples;  i++)
    {
        if ((cur->baud_phase += step) < period)
            continue;
        cur->baud_phase -= period;
        // getbaud()
        if (cur->in_training)
        {
            if (modem == SPANGPU_V17)
            {
                if (cur->training_step <= kV17End)
                {
                    if (cur->training_step < kV17Seg4)
                    {
                        // training_get(), v17tx.c:143-175
                        cur->training_step++;
                        if (cur->training_step > kV17Seg2  &&  cur->training_step <= kV17Seg3  &&  cur->short_train
                            &&  cur->training_step == kV17ShortSeg4)
                            cur->training_step = kV17Seg4;
                        continue;
                    }
                    if (++cur->training_step > kV17End)
                        cur->in_training = 0;
                }
                else
                {
                    cur->training_step++;
                }
            }
            else
            {
                const int last_seg = (modem == SPANGPU_V29)  ?  kVtSeg4  :  kV27Seg5;
                const int end = (modem == SPANGPU_V29)  ?  kVtEnd  :  kV27End;
                if (++cur->training_step <= last_seg)
                    continue;
                if (cur->training_step == end + 1)
                    cur->in_training = 0;
            }
        }
        for (int b = 0;  b < bits_per_baud  &&  !cur->in_training;  b++)
        {
            calls++;
            if (bits_before_end >= 0  &&  calls > bits_before_end)
                cur->in_training = 1;       // SIG_STATUS_END_OF_DATA: fake_get_bit() for the rest, and the shutdown
        }
    }
    return calls;
}

// The pulse shaper tables this library builds (for tests).  which: 0 V.29 [10][9], 1 V.27ter 4800 bps [5][9],
// 2 V.27ter 2400 bps [20][9].  Returns the number of floats.
int spangpu_modemtx_table(int which, float *out, int max)
{
    static const int sets[3] = {10, 5, 20};
    static const double excess[3] = {0.25, 0.5, 0.5};
    if (out == NULL  ||  which < 0  ||  which > 2  ||  max < sets[which]*9)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad table request");
    if (spg_make_tx_pulseshaper(sets[which], 9, excess[which], out) != 0)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "table scratch");
    return sets[which]*9;
}

}   // extern "C"
