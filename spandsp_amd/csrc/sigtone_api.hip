// sigtone_api.hip -- C ABI of the in-band signalling tone banks (include/spangpu.h, "signalling tone banks"):
// batched sig_tone_rx() and sig_tone_tx().  Device code: sigtone_dev.hpp.  No CPU implementation of either path
// exists behind these entry points.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#include "sigtone_dev.hpp"
#include "bank_host.hpp"

using namespace spg;

static const float kMaxPower = 3.14f + 3.02f;       // DBM0_MAX_POWER

static int32_t power_level_dbm0(float level)
{
    // power_meter_level_dbm0(), power_meter.c:82-92
    level -= kMaxPower;
    if (level > 0.0)
        level = 0.0;
    return (int32_t) (powf(10.0f, level/10.0f)*(32767.0f*32767.0f));
}

// the parts of the three descriptors the host needs (sig_tone.c:137-223)
struct SigDesc
{
    int freq[2];
    int amp[2][2];
    int high_low_timeout;
    int tones;
    float detection_ratio;
    float sharp_threshold;
    float flat_threshold;
};

static const SigDesc kDesc[3] =
{
    {{2280, 0},    {{-10, -20}, {0, 0}}, 400*8, 1, 13.0f, -30.0f, -30.0f},
    {{2600, 0},    {{-8, -8}, {0, 0}},   0,     1, 15.6f, -30.0f, -30.0f},
    {{2400, 2600}, {{-8, -8}, {-8, -8}}, 0,     2, 15.6f, -30.0f, -30.0f}
};

// ---- receiver banks ----------------------------------------------------------------------------------------------

struct spangpu_sigtone_rx_s
{
    BankCore c;
    PcmStage pcm;
    int tone_type;
    VarLens lens;               // per-channel lengths of an rx_var call
    int32_t *events;            // [n_ch][ev_cap][3]
    int32_t *h_events;
    CountRows count;
    int ev_cap;
    int last_cap;
    int32_t thresholds[3];
};

extern "C" {

int spangpu_sigtone_rx_create(spangpu_sigtone_rx_t **out, int device, int tone_type, int n_channels)
{
    if (out == NULL  ||  n_channels <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    *out = NULL;
    // sig_tone_rx_init() refuses other types (sig_tone.c:679-680)
    if (tone_type < SPANGPU_SIG_TONE_2280HZ  ||  tone_type > SPANGPU_SIG_TONE_2400HZ_2600HZ)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "not a signalling tone type");
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_sigtone_rx_s *b = (spangpu_sigtone_rx_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    b->tone_type = tone_type;
    // sig_tone.c:714-716
    const SigDesc &d = kDesc[tone_type - 1];
    b->thresholds[0] = power_level_dbm0(d.flat_threshold);
    b->thresholds[1] = power_level_dbm0(d.sharp_threshold);
    b->thresholds[2] = (int32_t) (powf(10.0f, d.detection_ratio/10.0f) + 1.0f);
    if ((rc = core_create(&b->c, device, n_channels, kSigRxWords)) != SPANGPU_OK)
    {
        spangpu_sigtone_rx_destroy(b);
        return rc;
    }
    if ((rc = counts_create(&b->c, &b->count, 1, 1)) != SPANGPU_OK)
    {
        spangpu_sigtone_rx_destroy(b);
        return rc;
    }
    // memset(s, 0, sizeof(*s)) and last_sample_tone_present = -1 (sig_tone.c:690-704)
    int32_t one[kSigRxWords];
    memset(one, 0, sizeof(one));
    one[SG_LAST_PRESENT] = -1;
    if ((rc = core_fill(&b->c, one)) != SPANGPU_OK)
    {
        spangpu_sigtone_rx_destroy(b);
        return rc;
    }
    *out = b;
    return SPANGPU_OK;
}

void spangpu_sigtone_rx_destroy(spangpu_sigtone_rx_t *b)
{
    if (b == NULL)
        return;
    core_destroy(&b->c);
    stage_free(&b->pcm);
    lens_free(&b->lens);
    (void) hipFree(b->events);
    if (b->h_events)
        (void) hipHostFree(b->h_events);
    counts_free(&b->count);
    free(b);
}

int spangpu_sigtone_rx_channels(const spangpu_sigtone_rx_t *b) { return b  ?  b->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_sigtone_rx_state_words(const spangpu_sigtone_rx_t *b) { return b  ?  kSigRxWords  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_sigtone_rx_set_stream(spangpu_sigtone_rx_t *b, void *stream)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&b->c, stream);
}

int spangpu_sigtone_rx_sync(spangpu_sigtone_rx_t *b)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&b->c);
}

// sig_tone_rx_set_mode(s, mode, duration), sig_tone.c:666-669, for one channel or (channel < 0) for all
int spangpu_sigtone_rx_set_mode(spangpu_sigtone_rx_t *b, int channel, int mode)
{
    if (b == NULL  ||  channel >= b->c.n_ch)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    SPG_TRY(hipSetDevice(b->c.device));
    int32_t *row = b->c.st + (size_t) SG_RX_TONE*b->c.n_ch;
    if (channel >= 0)
    {
        const int32_t v = mode;
        SPG_TRY(hipMemcpyAsync(row + channel, &v, sizeof(v), hipMemcpyHostToDevice, b->c.stream));
        SPG_TRY(hipStreamSynchronize(b->c.stream));
        return SPANGPU_OK;
    }
    int32_t *host = (int32_t *) malloc((size_t) b->c.n_ch*sizeof(int32_t));
    if (host == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "malloc");
    for (int c = 0;  c < b->c.n_ch;  c++)
        host[c] = mode;
    const hipError_t e = hipMemcpyAsync(row, host, (size_t) b->c.n_ch*sizeof(int32_t), hipMemcpyHostToDevice, b->c.stream);
    const hipError_t e2 = hipStreamSynchronize(b->c.stream);
    free(host);
    if (e != hipSuccess  ||  e2 != hipSuccess)
        return spangpu_set_error(SPANGPU_ERR_HIP, "mode upload failed");
    return SPANGPU_OK;
}

int spangpu_sigtone_rx(spangpu_sigtone_rx_t *b, int16_t *amp, int mem_kind, int samples, long long stride)
{
    int rc = rx_args_ok(b, mem_kind, amp, samples, &stride);
    if (rc != SPANGPU_OK)
        return rc;
    SPG_TRY(hipSetDevice(b->c.device));
    // a tone is declared after 3 ms of consistent detection and withdrawn after 8 ms (or at once in flat mode, which
    // takes 225 ms to enter): 24 samples between two reports at the very least
    if ((rc = grow_pair(&b->events, &b->h_events, &b->ev_cap, 4 + samples/16, (size_t) b->c.n_ch*3, b->c.stream)) != SPANGPU_OK)
        return rc;
    SigRxLaunch L;
    memset(&L, 0, sizeof(L));
    L.st = b->c.st;
    L.events = b->events;
    L.ev_count = b->count.dev;
    L.n_ch = b->c.n_ch;
    L.samples = samples;
    L.lens = b->lens.next;
    L.ev_cap = b->ev_cap;
    L.flat_threshold = b->thresholds[0];
    L.sharp_threshold = b->thresholds[1];
    L.detection_ratio = b->thresholds[2];
    // (no wait for the copy in: the frame goes back to the caller after the launch, and that copy is waited for)
    const int16_t *rows;
    if ((rc = stage_in(&b->c, &b->pcm, mem_kind, amp, stride, samples, false, &rows, &L.stride, &L.vec)) != SPANGPU_OK)
        return rc;
    L.pcm = const_cast<int16_t *>(rows);
    const dim3 grid((b->c.n_ch + 63)/64);
    switch (b->tone_type)
    {
    case SPANGPU_SIG_TONE_2280HZ:   hipLaunchKernelGGL(sigtone_rx_kernel<1>, grid, dim3(64), 0, b->c.stream, L); break;
    case SPANGPU_SIG_TONE_2600HZ:   hipLaunchKernelGGL(sigtone_rx_kernel<2>, grid, dim3(64), 0, b->c.stream, L); break;
    default:                        hipLaunchKernelGGL(sigtone_rx_kernel<3>, grid, dim3(64), 0, b->c.stream, L); break;
    }
    SPG_TRY(hipGetLastError());
    b->last_cap = b->ev_cap;
    // the frame goes back as the receiver left it; the caller's buffer is only borrowed for the call
    return stage_out_back(&b->c, &b->pcm, mem_kind, amp, stride, samples, NULL);
}

// spangpu_sigtone_rx() for a tick in which not every channel has a frame, or frames differ in length: channel c takes
// lens[c] samples of its row (0: it sits the call out, its state and its row as they were, no events).  lens[] is host memory.
int spangpu_sigtone_rx_var(spangpu_sigtone_rx_t *b, int16_t *amp, int mem_kind, const int32_t *lens, int max_samples, long long stride)
{
    if (b == NULL  ||  amp == NULL  ||  lens == NULL  ||  max_samples <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int longest;
    bool all;
    int rc = lens_check(lens, b->c.n_ch, max_samples, &longest, &all);
    // nobody brings a sample: no launch; everybody the same: the plain call
    if (rc != SPANGPU_OK  ||  longest == 0)
        return rc;
    if (stride <= 0)
        stride = max_samples;
    if (!all  &&  (rc = lens_upload(&b->c, &b->lens, lens)) != SPANGPU_OK)
        return rc;
    rc = spangpu_sigtone_rx(b, amp, mem_kind, longest, stride);
    b->lens.next = NULL;
    return rc;
}

int spangpu_sigtone_rx_events(spangpu_sigtone_rx_t *b, const int32_t **events, const int32_t **counts)
{
    if (b == NULL  ||  events == NULL  ||  counts == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (b->last_cap <= 0)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no spangpu_sigtone_rx() yet");
    int rc = counts_fetch(&b->c, &b->count, 1);
    if (rc != SPANGPU_OK)
        return rc;
    int most;
    if (!count_row_scan(b->count.pinned, b->c.n_ch, b->last_cap, &most))
        return spangpu_set_error(SPANGPU_ERR_STATE, "a channel reported more often than the event buffer holds");
    if ((rc = rows_fetch(&b->c, b->h_events, b->events, 3*sizeof(int32_t), b->last_cap, most)) != SPANGPU_OK)
        return rc;
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    *events = b->h_events;
    *counts = b->count.pinned;
    return b->last_cap;
}

int spangpu_sigtone_rx_get_state(spangpu_sigtone_rx_t *b, int channel, int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, 0, kSigRxWords, words, false);
}

// The reverse of spangpu_sigtone_rx_get_state(): a channel's 27 words as a caller holds them (a snapshot taken earlier).
int spangpu_sigtone_rx_set_state(spangpu_sigtone_rx_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, 0, kSigRxWords, const_cast<int32_t *>(words), true);
}

int spangpu_sigtone_rx_thresholds(const spangpu_sigtone_rx_t *b, int32_t out[3])
{
    if (b == NULL  ||  out == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    memcpy(out, b->thresholds, sizeof(b->thresholds));
    return SPANGPU_OK;
}

}   // extern "C"

// ---- sender banks --------------------------------------------------------------------------------------------------

struct spangpu_sigtone_tx_s
{
    BankCore c;
    PcmStage pcm;
    int tone_type;
    int16_t *quarter;
    int32_t *start;
    int32_t *request;
    int32_t *d_modes;           // [2][n_ch]: modes, durations
    int32_t *h_modes;           // pinned
    int32_t *h_request;
    int32_t *h_start;
    int samples;                // of the frame in progress (0: none)
    int32_t phase_rate[2];
    int32_t scaling[2][2];
};

static int tx_run(spangpu_sigtone_tx_s *b, int16_t *amp, int mem_kind, long long stride)
{
    SigTxLaunch L;
    memset(&L, 0, sizeof(L));
    L.st = b->c.st;
    L.quarter = b->quarter;
    L.start = b->start;
    L.request = b->request;
    L.n_ch = b->c.n_ch;
    L.samples = b->samples;
    L.tones = kDesc[b->tone_type - 1].tones;
    memcpy(L.phase_rate, b->phase_rate, sizeof(L.phase_rate));
    memcpy(L.scaling, b->scaling, sizeof(L.scaling));
    // (the frame may hold the caller's own signal, so it goes in; no wait: the way back is waited for)
    const int16_t *rows;
    int rc = stage_in(&b->c, &b->pcm, mem_kind, amp, stride, b->samples, false, &rows, &L.stride, NULL);
    if (rc != SPANGPU_OK)
        return rc;
    L.pcm = const_cast<int16_t *>(rows);
    hipLaunchKernelGGL(sigtone_tx_kernel, dim3((b->c.n_ch + 63)/64), dim3(64), 0, b->c.stream, L);
    SPG_TRY(hipGetLastError());
    SPG_TRY(hipMemcpyAsync(b->h_request, b->request, (size_t) b->c.n_ch*sizeof(int32_t), hipMemcpyDeviceToHost, b->c.stream));
    SPG_TRY(hipMemcpyAsync(b->h_start, b->start, (size_t) b->c.n_ch*sizeof(int32_t), hipMemcpyDeviceToHost, b->c.stream));
    if ((rc = stage_out_back(&b->c, &b->pcm, mem_kind, amp, stride, b->samples, NULL)) != SPANGPU_OK)
        return rc;
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    int pending = 0;
    for (int c = 0;  c < b->c.n_ch;  c++)
        pending += (b->h_request[c] != 0);
    return pending;
}

extern "C" {

int spangpu_sigtone_tx_create(spangpu_sigtone_tx_t **out, int device, int tone_type, int n_channels)
{
    if (out == NULL  ||  n_channels <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    *out = NULL;
    if (tone_type < SPANGPU_SIG_TONE_2280HZ  ||  tone_type > SPANGPU_SIG_TONE_2400HZ_2600HZ)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "not a signalling tone type");
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_sigtone_tx_s *b = (spangpu_sigtone_tx_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    b->tone_type = tone_type;
    // sig_tone_tx_init(), sig_tone.c:369-380: dds_phase_rate() and dds_scaling_dbm0() (dds_int.c:316-331)
    const SigDesc &d = kDesc[tone_type - 1];
    for (int i = 0;  i < 2;  i++)
    {
        b->phase_rate[i] = d.freq[i]  ?  (int32_t) ((float) d.freq[i]*65536.0f*65536.0f/8000)  :  0;
        for (int k = 0;  k < 2;  k++)
            b->scaling[i][k] = (int16_t) (powf(10.0f, ((float) d.amp[i][k] - 3.14f)/20.0f)*32767.0f);
    }
    if ((rc = core_create(&b->c, device, n_channels, kSigTxWords)) != SPANGPU_OK  ||  (rc = quarter_sine_upload(&b->quarter)) != SPANGPU_OK)
    {
        spangpu_sigtone_tx_destroy(b);
        return rc;
    }
    const size_t nb = (size_t) n_channels*sizeof(int32_t);
    if (hipMalloc(&b->start, nb) != hipSuccess
        ||  hipMalloc(&b->request, nb) != hipSuccess
        ||  hipMalloc(&b->d_modes, 2*nb) != hipSuccess
        ||  hipHostMalloc(&b->h_modes, 2*nb) != hipSuccess
        ||  (b->h_request = (int32_t *) malloc(nb)) == NULL
        ||  (b->h_start = (int32_t *) malloc(nb)) == NULL)
    {
        spangpu_sigtone_tx_destroy(b);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the signalling tone sender bank failed");
    }
    if (hipMemset(b->c.st, 0, kSigTxWords*nb) != hipSuccess
        ||  hipMemset(b->start, 0, nb) != hipSuccess
        ||  hipMemset(b->request, 0, nb) != hipSuccess)
    {
        spangpu_sigtone_tx_destroy(b);
        return spangpu_set_error(SPANGPU_ERR_HIP, "state upload failed");
    }
    *out = b;
    return SPANGPU_OK;
}

void spangpu_sigtone_tx_destroy(spangpu_sigtone_tx_t *b)
{
    if (b == NULL)
        return;
    core_destroy(&b->c);
    stage_free(&b->pcm);
    (void) hipFree(b->quarter);
    (void) hipFree(b->start);
    (void) hipFree(b->request);
    (void) hipFree(b->d_modes);
    if (b->h_modes) (void) hipHostFree(b->h_modes);
    free(b->h_request);
    free(b->h_start);
    free(b);
}

int spangpu_sigtone_tx_channels(const spangpu_sigtone_tx_t *b) { return b  ?  b->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_sigtone_tx_state_words(const spangpu_sigtone_tx_t *b) { return b  ?  kSigTxWords  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_sigtone_tx_set_stream(spangpu_sigtone_tx_t *b, void *stream)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&b->c, stream);
}

// sig_tone_tx_set_mode(s, mode, duration) on every channel whose modes[] entry is not negative (host arrays of
// n_channels entries)
int spangpu_sigtone_tx_set_modes(spangpu_sigtone_tx_t *b, const int32_t *modes, const int32_t *durations)
{
    if (b == NULL  ||  modes == NULL  ||  durations == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    const size_t nb = (size_t) b->c.n_ch*sizeof(int32_t);
    memcpy(b->h_modes, modes, nb);
    memcpy(b->h_modes + b->c.n_ch, durations, nb);
    SPG_TRY(hipMemcpyAsync(b->d_modes, b->h_modes, 2*nb, hipMemcpyHostToDevice, b->c.stream));
    hipLaunchKernelGGL(sigtone_tx_set_mode_kernel, dim3((b->c.n_ch + 255)/256), dim3(256), 0, b->c.stream,
                       b->c.st, b->c.n_ch, b->d_modes, b->d_modes + b->c.n_ch, kDesc[b->tone_type - 1].high_low_timeout);
    SPG_TRY(hipGetLastError());
    return SPANGPU_OK;
}

int spangpu_sigtone_tx_set_mode(spangpu_sigtone_tx_t *b, int channel, int mode, int duration)
{
    if (b == NULL  ||  channel >= b->c.n_ch  ||  mode < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    if (channel >= 0)
    {
        // one channel: its five words through the host (sig_tone_tx_set_mode(), sig_tone.c:326-345), not two arrays of
        // n_channels entries through a kernel
        int32_t w[kSigTxWords];
        int rc = core_rw_words(&b->c, channel, 0, kSigTxWords, w, false);
        if (rc != SPANGPU_OK)
            return rc;
        const int old_tones = w[SX_TONE] & (SIG_1_PRESENT | SIG_2_PRESENT);
        const int new_tones = mode & (SIG_1_PRESENT | SIG_2_PRESENT);
        if (new_tones  &&  old_tones != new_tones)
            w[SX_HIGH_LOW] = kDesc[b->tone_type - 1].high_low_timeout;
        if ((mode & SIG_1_PRESENT)  &&  !(w[SX_TONE] & SIG_1_PRESENT))
            w[SX_PHASE0] = 0;
        if ((mode & SIG_2_PRESENT)  &&  !(w[SX_TONE] & SIG_2_PRESENT))
            w[SX_PHASE1] = 0;
        w[SX_TONE] = mode;
        w[SX_TIMEOUT] = duration;
        return core_rw_words(&b->c, channel, 0, kSigTxWords, w, true);
    }
    for (int c = 0;  c < b->c.n_ch;  c++)
    {
        b->h_modes[c] = mode;
        b->h_modes[b->c.n_ch + c] = duration;
    }
    SPG_TRY(hipMemcpyAsync(b->d_modes, b->h_modes, 2*(size_t) b->c.n_ch*sizeof(int32_t), hipMemcpyHostToDevice, b->c.stream));
    hipLaunchKernelGGL(sigtone_tx_set_mode_kernel, dim3((b->c.n_ch + 255)/256), dim3(256), 0, b->c.stream,
                       b->c.st, b->c.n_ch, b->d_modes, b->d_modes + b->c.n_ch, kDesc[b->tone_type - 1].high_low_timeout);
    SPG_TRY(hipGetLastError());
    return SPANGPU_OK;
}

// A new frame for every channel.  Returns the number of channels that stopped for their update request (see
// spangpu_sigtone_tx_requests()), 0 when the whole frame is done, or a negative error.
int spangpu_sigtone_tx(spangpu_sigtone_tx_t *b, int16_t *amp, int mem_kind, int samples, long long stride)
{
    // (a sender, but with a receiver's arguments: it works on the caller's frame in place, and its stride may be left out)
    const int rc = rx_args_ok(b, mem_kind, amp, samples, &stride);
    if (rc != SPANGPU_OK)
        return rc;
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipMemsetAsync(b->start, 0, (size_t) b->c.n_ch*sizeof(int32_t), b->c.stream));
    b->samples = samples;
    return tx_run(b, amp, mem_kind, stride);
}

// The same frame again, for the channels that had stopped: each goes on from where it stopped, in whatever mode its
// callback has set meanwhile.  Same return value.
int spangpu_sigtone_tx_continue(spangpu_sigtone_tx_t *b, int16_t *amp, int mem_kind, long long stride)
{
    if (b == NULL  ||  amp == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (b->samples <= 0)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no frame in progress");
    if (stride <= 0)
        stride = b->samples;
    SPG_TRY(hipSetDevice(b->c.device));
    return tx_run(b, amp, mem_kind, stride);
}

// After spangpu_sigtone_tx() / _continue(): request[c] != 0 for the channels whose callback is due, stopped[c] = the
// sample of the frame they stopped at (= samples for the channels that are done).
int spangpu_sigtone_tx_requests(spangpu_sigtone_tx_t *b, const int32_t **request, const int32_t **stopped)
{
    if (b == NULL  ||  request == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (b->samples <= 0)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no frame in progress");
    *request = b->h_request;
    if (stopped)
        *stopped = b->h_start;
    return SPANGPU_OK;
}

int spangpu_sigtone_tx_get_state(spangpu_sigtone_tx_t *b, int channel, int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, 0, kSigTxWords, words, false);
}

}   // extern "C"
