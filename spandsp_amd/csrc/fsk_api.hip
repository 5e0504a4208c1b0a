// fsk_api.hip -- C ABI of the FSK receiver banks (include/spangpu.h, "FSK receiver banks"): batched
// fsk_rx().  Device code: fsk_dev.hpp.  No CPU implementation of the receive path exists behind these
// entry points; the control-plane calls (restart, cutoff, frame parameters, fill-in) edit one channel's
// state words on the host, as the reference's own functions edit one object.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#include "fsk_dev.hpp"
#include "bank_host.hpp"

using namespace spg;

namespace spg
{

__global__ __launch_bounds__(64) void fsk_bank_kernel(const FskLaunch L)
{
    extern __shared__ int32_t win[];        // [4*span][64]
    __shared__ uint32_t wave[kFskWave];     // a separate object, so that table reads can move across window writes
    const int lane = threadIdx.x;
    const int ch = blockIdx.x*64 + lane;
    const bool live = ch < L.n_ch;
    const size_t n = (size_t) L.n_ch;
    const int span = L.span;

    fsk_fill_wave(wave, L.quarter, lane, 64);
    // (a lane past the end of the bank reads channel 0's words and stops after the barrier)
    int32_t *st = L.st + (live  ?  ch  :  0);
    fsk_load_window(win, st + (size_t) kFskScalars*n, n, span, lane);
    __syncthreads();
    if (!live)
        return;

    FskRegs r;
    fsk_load_regs(r, st, n);
    int16_t *ev = L.events + (size_t) ch*L.ev_cap;
    const int ev_cap = L.ev_cap;
    auto emit = [&](int v) __attribute__((always_inline))
    {
        if (r.n_ev < ev_cap)
            ev[r.n_ev] = (int16_t) v;
        r.n_ev++;
    };
    const int mylen = L.lens  ?  min(max(L.lens[ch], 0), L.samples)  :  L.samples;
    auto frame = [&](auto aligned, auto framed) __attribute__((always_inline))
    {
        FskRow<decltype(aligned)::value> row;
        fsk_row_begin(row, L.pcm + (size_t) ch*L.stride, mylen);
        for (int base = 0;  base < L.samples;  base += 8)
        {
            const int todo = max(0, min(8, mylen - base));      // per lane when the call carries per-channel lengths
            int32_t a[8];
            int32_t c0[8];
            int32_t q0[8];
            int32_t c1[8];
            int32_t q1[8];
            fsk_row_block(row, base, todo, a);
            fsk_block_lookups(r, wave, todo, c0, q0, c1, q1);
            // (a whole block in every lane is the common case: no per-sample guard, whose bodies the compiler moves out of line)
            if (__builtin_expect(__all(todo == 8), 1))
            {
#pragma unroll
                for (int k = 0;  k < 8;  k++)
                    fsk_step<decltype(framed)::value>(r, win, lane, span, a[k], c0[k], q0[k], c1[k], q1[k], emit);
            }
            else
            {
#pragma unroll
                for (int k = 0;  k < 8;  k++)
                {
                    if (k < todo)
                        fsk_step<true>(r, win, lane, span, a[k], c0[k], q0[k], c1[k], q1[k], emit);
                }
            }
        }
    };
    // (unaligned rows are the rare case: one copy, the general one)
    if (!L.vec)
        frame(std::false_type{}, std::true_type{});
    else if (__any(r.framing == 2))
        frame(std::true_type{}, std::true_type{});
    else
        frame(std::true_type{}, std::false_type{});
    fsk_store_regs(r, st, n);
    fsk_store_window(win, st + (size_t) kFskScalars*n, n, span, lane);
    L.ev_count[ch] = r.n_ev;
}

// put_bit() of the plain receiver: one more entry of the channel's int16 event list
struct FskEventSink
{
    const FskLaunch &L;
    int16_t *ev;

    __device__ __forceinline__ void open(bool live, int ch, size_t n, int mylen)
    {
        ev = L.events + (size_t) ch*L.ev_cap;
    }

    __device__ __forceinline__ void put(FskBitSide &t, int v)
    {
        if (t.n_ev < L.ev_cap)
            ev[t.n_ev] = (int16_t) v;
        t.n_ev++;
    }

    __device__ __forceinline__ void close(FskBitSide &t, int ch, size_t n)
    {
        L.ev_count[ch] = t.n_ev;
    }
};

// The same receiver as two waves per 64 channels (fsk_pair_body(), fsk_dev.hpp): the framing is each channel's own
__global__ __launch_bounds__(128) void fsk_pair_kernel(const FskLaunch L)
{
    FskEventSink sink = {L, nullptr};
    fsk_pair_body<FSK_FRAMING_BY_STATE>(L, sink);
}

}   // namespace spg

// 0 = the library's choice (two waves per 64 channels), 1 = the whole receiver in one wave, 2 = two waves
static int g_fsk_waves = 0;

extern "C" int spangpu_tune_fsk_waves(int waves)
{
    if (waves < 0  ||  waves > 2)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "0 (the library's choice), 1 or 2 waves per 64 channels");
    g_fsk_waves = waves;
    return SPANGPU_OK;
}

// (for the other bank families the knob covers; not part of the ABI)
extern "C" __attribute__((visibility("hidden"))) int spangpu_fsk_waves_choice(void)
{
    return g_fsk_waves;
}

struct spangpu_fsk_s
{
    VarLens lens;               // per-channel lengths of the call being prepared
    BankCore c;
    PcmStage pcm;               // staging for host-resident frames
    int span;
    spangpu_fsk_spec_t spec;
    int16_t *quarter;
    int16_t *events;            // [n_ch][ev_cap]
    int16_t *h_events;
    CountRows count;
    int ev_cap;
    int last_cap;
};

// preset_fsk_specs[], src/fsk.c:60-155: freq_zero, freq_one, tx_level, min_level, baud_rate x 100
static const spangpu_fsk_spec_t k_presets[11] =
{
    {1080 + 100, 1080 - 100, -14, -30, 300*100},        // V21 ch 1
    {1750 + 100, 1750 - 100, -14, -30, 300*100},        // V21 ch 2
    {1700 + 400, 1700 - 400, -14, -30, 1200*100},       // V23 ch 1
    {420 + 30, 420 - 30, -14, -30, 75*100},             // V23 ch 2
    {1170 - 100, 1170 + 100, -14, -30, 300*100},        // Bell103 ch 1
    {2125 - 100, 2125 + 100, -14, -30, 300*100},        // Bell103 ch 2
    {1700 + 500, 1700 - 500, -14, -30, 1200*100},       // Bell202
    {1600 + 200, 1600 - 200, -14, -30, 4545},           // Weitbrecht 45.45
    {1600 + 200, 1600 - 200, -14, -30, 50*100},         // Weitbrecht 50
    {1600 + 200, 1600 - 200, -14, -30, 4760},           // Weitbrecht 47.6
    {1080 + 100, 1080 - 100, -14, -30, 110*100}         // V21 (110bps) ch 1
};

static int32_t power_level_dbm0(float level)
{
    // power_meter_level_dbm0(), power_meter.c:82-92 (DBM0_MAX_POWER = 3.14 + 3.02)
    level -= (3.14f + 3.02f);
    if (level > 0.0)
        level = 0.0;
    return (int32_t) (powf(10.0f, level/10.0f)*(32767.0f*32767.0f));
}

static void cutoff_words(int32_t *w, float cutoff)
{
    // fsk_rx_set_signal_cutoff(), fsk.c:270-276
    w[FS_ON_POWER] = power_level_dbm0(cutoff + 2.5f - 5.3f);
    w[FS_OFF_POWER] = power_level_dbm0(cutoff - 2.5f - 5.3f);
}

static void frame_words(int32_t *w, int data_bits, int parity, int stop_bits)
{
    // fsk_rx_set_frame_parameters(), fsk.c:300-316
    if (w[FS_FRAMING] != SPANGPU_FSK_FRAME_MODE_FRAMED)
        return;
    w[FS_DATA_BITS] = data_bits;
    w[FS_PARITY] = parity;
    w[FS_STOP_BITS] = stop_bits;
    w[FS_TOTAL_BITS] = data_bits + ((parity != 0)  ?  1  :  0);
}

static int span_of(const spangpu_fsk_spec_t *spec)
{
    int span = kFskRateX100/spec->baud_rate;
    return (span > kFskMaxWindow)  ?  kFskMaxWindow  :  span;
}

static void restart_words(int32_t *w, const spangpu_fsk_spec_t *spec, int framing_mode)
{
    // fsk_rx_restart(), fsk.c:660-720.  The window and the running dot products are left as they are,
    // as the reference leaves them.
    w[FS_BAUD_RATE] = spec->baud_rate;
    w[FS_FRAMING] = framing_mode;
    if (framing_mode == SPANGPU_FSK_FRAME_MODE_FRAMED)
        frame_words(w, 8, 0, 1);
    cutoff_words(w, (float) spec->min_level);
    w[FS_RATE0] = (int32_t) ((float) spec->freq_zero*65536.0f*65536.0f/8000);      // dds_phase_rate(), dds_int.c
    w[FS_RATE1] = (int32_t) ((float) spec->freq_one*65536.0f*65536.0f/8000);
    w[FS_ACC0] = 0;
    w[FS_ACC1] = 0;
    w[FS_LAST_SAMPLE] = 0;
    w[FS_SPAN] = span_of(spec);
    int shift = 0;
    for (int chop = w[FS_SPAN];  chop != 0;  chop >>= 1)
        shift++;
    w[FS_SHIFT] = shift;
    w[FS_BAUD_PHASE] = 0;
    w[FS_FRAME_POS] = -2;
    w[FS_FRAME] = 0;
    w[FS_LAST_BIT] = 0;
    w[FS_POWER] = 0;
    w[FS_SIGNAL_PRESENT] = 0;
}

// The control plane's edits of one channel's words, for the bank families that carry an FSK receiver inside them (v18_api.hip);
// not part of the ABI.
extern "C" __attribute__((visibility("hidden"))) void spangpu_fsk_words_init(int32_t *w, const spangpu_fsk_spec_t *spec, int framing_mode,
                                                                             int data_bits, int parity, int stop_bits)
{
    restart_words(w, spec, framing_mode);
    frame_words(w, data_bits, parity, stop_bits);
}

extern "C" __attribute__((visibility("hidden"))) void spangpu_fsk_words_fillin(int32_t *w, int len)
{
    if (len > 0)
    {
        int32_t *slot = w + kFskScalars + 4*w[FS_BUF_PTR];
        w[FS_DOT0RE] -= slot[0];
        w[FS_DOT0IM] -= slot[1];
        w[FS_DOT1RE] -= slot[2];
        w[FS_DOT1IM] -= slot[3];
        slot[0] = slot[1] = slot[2] = slot[3] = 0;
        w[FS_ACC0] = (int32_t) ((uint32_t) w[FS_ACC0] + (uint32_t) len*(uint32_t) w[FS_RATE0]);
        w[FS_ACC1] = (int32_t) ((uint32_t) w[FS_ACC1] + (uint32_t) len*(uint32_t) w[FS_RATE1]);
    }
}

// the event rows of the last spangpu_fsk_rx(), where they lie on the device (faxfe_api.hip); not part of the ABI
extern "C" __attribute__((visibility("hidden"))) void spangpu_fsk_event_rows(const spangpu_fsk_t *f, const int16_t **events, const int32_t **counts, int *cap)
{
    *events = f->events;
    *counts = f->count.dev;
    *cap = f->last_cap;
}

// fsk_rx_set_signal_cutoff() of every channel: two rows of the state (faxfe_api.hip); not part of the ABI
extern "C" __attribute__((visibility("hidden"))) int spangpu_fsk_cutoff_all(spangpu_fsk_t *f, float cutoff_dbm0)
{
    int32_t w[kFskScalars];
    cutoff_words(w, cutoff_dbm0);
    SPG_TRY(hipSetDevice(f->c.device));
    SPG_TRY(hipMemsetD32Async((hipDeviceptr_t) (f->c.st + (size_t) FS_ON_POWER*f->c.n_ch), w[FS_ON_POWER], (size_t) f->c.n_ch, f->c.stream));
    SPG_TRY(hipMemsetD32Async((hipDeviceptr_t) (f->c.st + (size_t) FS_OFF_POWER*f->c.n_ch), w[FS_OFF_POWER], (size_t) f->c.n_ch, f->c.stream));
    SPG_TRY(hipStreamSynchronize(f->c.stream));
    return SPANGPU_OK;
}

extern "C" {

int spangpu_fsk_preset(int which, spangpu_fsk_spec_t *spec)
{
    if (which < 0  ||  which > SPANGPU_FSK_V21CH1_110  ||  spec == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "no such FSK preset");
    *spec = k_presets[which];
    return SPANGPU_OK;
}

int spangpu_fsk_create(spangpu_fsk_t **out, int device, int n_channels, const spangpu_fsk_spec_t *spec, int framing_mode)
{
    if (out == NULL  ||  spec == NULL  ||  n_channels <= 0  ||  spec->baud_rate <= 0  ||  framing_mode < 0  ||  framing_mode > 2)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    *out = NULL;
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_fsk_s *f = (spangpu_fsk_s *) calloc(1, sizeof(*f));
    if (f == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    f->spec = *spec;
    f->span = span_of(spec);
    const int words = kFskScalars + 4*f->span;
    if ((rc = core_create(&f->c, device, n_channels, words)) != SPANGPU_OK  ||  (rc = quarter_sine_upload(&f->quarter)) != SPANGPU_OK)
    {
        spangpu_fsk_destroy(f);
        return rc;
    }
    int32_t *one = (int32_t *) calloc(words, sizeof(int32_t));
    if (counts_create(&f->c, &f->count, 1, 1) != SPANGPU_OK  ||  one == NULL)
    {
        free(one);
        spangpu_fsk_destroy(f);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the FSK bank failed");
    }
    // fsk_rx_init() = memset + fsk_rx_restart(), fsk.c:723-742; the correlation window stays zero
    restart_words(one, spec, framing_mode);
    rc = core_fill(&f->c, one, kFskScalars);
    free(one);
    if (rc != SPANGPU_OK)
    {
        spangpu_fsk_destroy(f);
        return rc;
    }
    *out = f;
    return SPANGPU_OK;
}

void spangpu_fsk_destroy(spangpu_fsk_t *f)
{
    if (f == NULL)
        return;
    core_destroy(&f->c);
    stage_free(&f->pcm);
    (void) hipFree(f->quarter);
    lens_free(&f->lens);
    (void) hipFree(f->events);
    if (f->h_events)
        (void) hipHostFree(f->h_events);
    counts_free(&f->count);
    free(f);
}

int spangpu_fsk_channels(const spangpu_fsk_t *f) { return f  ?  f->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_fsk_state_words(const spangpu_fsk_t *f) { return f  ?  f->c.words  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_fsk_set_stream(spangpu_fsk_t *f, void *stream)
{
    if (f == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&f->c, stream);
}

int spangpu_fsk_sync(spangpu_fsk_t *f)
{
    if (f == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&f->c);
}

int spangpu_fsk_rx(spangpu_fsk_t *f, const int16_t *amp, int mem_kind, int samples, long long stride)
{
    int rc = rx_args_ok(f, mem_kind, amp, samples, &stride);
    if (rc != SPANGPU_OK)
        return rc;
    SPG_TRY(hipSetDevice(f->c.device));
    // at most one event per sample (a status change and a bit can share one sample: + 2)
    if ((rc = grow_pair(&f->events, &f->h_events, &f->ev_cap, samples + 2, (size_t) f->c.n_ch, f->c.stream)) != SPANGPU_OK)
        return rc;
    FskLaunch L;
    memset(&L, 0, sizeof(L));
    L.st = f->c.st;
    L.quarter = f->quarter;
    L.events = f->events;
    L.ev_count = f->count.dev;
    L.n_ch = f->c.n_ch;
    L.samples = samples;
    L.lens = f->lens.next;
    L.span = f->span;
    L.ev_cap = f->ev_cap;
    // the caller's buffer is only borrowed for the call: the copy in is waited for
    if ((rc = stage_in(&f->c, &f->pcm, mem_kind, amp, stride, samples, true, &L.pcm, &L.stride, &L.vec)) != SPANGPU_OK)
        return rc;
    const size_t lds = (size_t) (4*f->span*64)*sizeof(int32_t);
    if (g_fsk_waves != 1)
        hipLaunchKernelGGL(fsk_pair_kernel, dim3((f->c.n_ch + 63)/64), dim3(128), lds + 2*kFskMsgWords*64*sizeof(int32_t), f->c.stream, L);
    else
        hipLaunchKernelGGL(fsk_bank_kernel, dim3((f->c.n_ch + 63)/64), dim3(64), lds, f->c.stream, L);
    SPG_TRY(hipGetLastError());
    f->last_cap = f->ev_cap;
    return SPANGPU_OK;
}

// spangpu_fsk_rx() for a tick in which not every channel has a frame, or frames differ in length: channel c takes lens[c] samples
// of its row (0: it sits the call out, its state as it was, no events).  lens[] is host memory.
int spangpu_fsk_rx_var(spangpu_fsk_t *f, const int16_t *amp, int mem_kind, const int32_t *lens, int max_samples, long long stride)
{
    if (f == NULL  ||  amp == NULL  ||  lens == NULL  ||  max_samples <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int longest;
    bool all;
    int rc = lens_check(lens, f->c.n_ch, max_samples, &longest, &all);
    // nobody brings a sample: no launch; everybody the same: the plain call
    if (rc != SPANGPU_OK  ||  longest == 0)
        return rc;
    if (stride <= 0)
        stride = max_samples;
    if (!all  &&  (rc = lens_upload(&f->c, &f->lens, lens)) != SPANGPU_OK)
        return rc;
    rc = spangpu_fsk_rx(f, amp, mem_kind, longest, stride);
    f->lens.next = NULL;
    return rc;
}

// spangpu_fsk_rx_var() with the lengths already in device memory, the twin of spangpu_modem_rx_lens_dev(): channel c takes
// min(max(lens_dev[c], 0), samples) samples of its row, a channel that takes none sits the call out with a zero event count.
int spangpu_fsk_rx_lens_dev(spangpu_fsk_t *f, const int16_t *amp, int mem_kind, int samples, long long stride, const int32_t *lens_dev)
{
    if (f == NULL  ||  lens_dev == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    f->lens.next = lens_dev;
    const int rc = spangpu_fsk_rx(f, amp, mem_kind, samples, stride);
    f->lens.next = NULL;
    return rc;
}

int spangpu_fsk_events(spangpu_fsk_t *f, const int16_t **events, const int32_t **counts)
{
    if (f == NULL  ||  events == NULL  ||  counts == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (f->last_cap <= 0)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no spangpu_fsk_rx() yet");
    int rc = counts_fetch(&f->c, &f->count, 1);
    if (rc != SPANGPU_OK)
        return rc;
    // (samples + 2 events a call at the very most: a count cannot exceed the capacity)
    int most;
    (void) count_row_scan(f->count.pinned, f->c.n_ch, f->last_cap, &most);
    if ((rc = rows_fetch(&f->c, f->h_events, f->events, sizeof(int16_t), f->last_cap, most)) != SPANGPU_OK)
        return rc;
    SPG_TRY(hipStreamSynchronize(f->c.stream));
    *events = f->h_events;
    *counts = f->count.pinned;
    return f->last_cap;
}

// The last call's events device to device, the twin of spangpu_modem_copy_events(): dst = int32 counts[n_ch], then int16
// events[n_ch][per_channel].  Asynchronous on the bank's stream; a channel that made more than per_channel events shows it
// by its count.
int spangpu_fsk_copy_events(spangpu_fsk_t *f, void *dev_dst, size_t dst_bytes, int per_channel)
{
    if (f == NULL  ||  dev_dst == NULL  ||  per_channel <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (f->last_cap <= 0)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no spangpu_fsk_rx() yet");
    const size_t need = (size_t) f->c.n_ch*(sizeof(int32_t) + (size_t) per_channel*sizeof(int16_t));
    if (dst_bytes < need)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "destination too small");
    SPG_TRY(hipSetDevice(f->c.device));
    SPG_TRY(hipMemcpyAsync(dev_dst, f->count.dev, (size_t) f->c.n_ch*sizeof(int32_t), hipMemcpyDeviceToDevice, f->c.stream));
    const int w = (per_channel < f->last_cap)  ?  per_channel  :  f->last_cap;
    SPG_TRY(hipMemcpy2DAsync((char *) dev_dst + (size_t) f->c.n_ch*sizeof(int32_t), (size_t) per_channel*sizeof(int16_t), f->events,
                             (size_t) f->last_cap*sizeof(int16_t), (size_t) w*sizeof(int16_t), (size_t) f->c.n_ch, hipMemcpyDeviceToDevice,
                             f->c.stream));
    return SPANGPU_OK;
}

int spangpu_fsk_get_state(spangpu_fsk_t *f, int channel, int32_t *words)
{
    if (f == NULL  ||  words == NULL  ||  !channel_ok(&f->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&f->c, channel, 0, f->c.words, words, false);
}

int spangpu_fsk_set_state(spangpu_fsk_t *f, int channel, const int32_t *words)
{
    if (f == NULL  ||  words == NULL  ||  !channel_ok(&f->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (words[FS_SPAN] != f->span)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "the correlation span of a channel is fixed by its bank's baud rate");
    return core_rw_words(&f->c, channel, 0, f->c.words, const_cast<int32_t *>(words), true);
}

static int edit(spangpu_fsk_s *f, int channel, int what, int a, int b, int c, float x)
{
    if (f == NULL  ||  !channel_ok(&f->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t *w = (int32_t *) malloc((size_t) f->c.words*sizeof(int32_t));
    if (w == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "malloc");
    int rc = core_rw_words(&f->c, channel, 0, f->c.words, w, false);
    if (rc == SPANGPU_OK)
    {
        switch (what)
        {
        case 0:
            restart_words(w, &f->spec, a);
            break;
        case 1:
            cutoff_words(w, x);
            break;
        case 2:
            frame_words(w, a, b, c);
            break;
        case 3:
            // fsk_rx_fillin(), fsk.c:625-657: the current window slot is cleared, the oscillators run on, and
            // the slot index does not move
            spangpu_fsk_words_fillin(w, a);
            break;
        }
        rc = core_rw_words(&f->c, channel, 0, f->c.words, w, true);
    }
    free(w);
    return rc;
}

int spangpu_fsk_restart(spangpu_fsk_t *f, int channel, int framing_mode)
{
    if (framing_mode < 0  ||  framing_mode > 2)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad framing mode");
    return edit(f, channel, 0, framing_mode, 0, 0, 0.0f);
}

int spangpu_fsk_set_signal_cutoff(spangpu_fsk_t *f, int channel, float cutoff_dbm0)
{
    return edit(f, channel, 1, 0, 0, 0, cutoff_dbm0);
}

int spangpu_fsk_set_frame_parameters(spangpu_fsk_t *f, int channel, int data_bits, int parity, int stop_bits)
{
    return edit(f, channel, 2, data_bits, parity, stop_bits, 0.0f);
}

int spangpu_fsk_fillin(spangpu_fsk_t *f, int channel, int len)
{
    return edit(f, channel, 3, len, 0, 0, 0.0f);
}

}   // extern "C"
