// tone_rx.hip -- the tone bank's launch path: which kernel serves a frame, the launch geometry, the rx entry points and the
// launch several banks share.  The one unit that includes tone_dev.hpp and tone_fast.hpp: their kernels are instantiated once.

#include <atomic>
#include <stdlib.h>
#include <string.h>

#include "tone_cadence.hpp"
#include "tone_dev.hpp"
#include "tone_fast.hpp"

using namespace spg;

static_assert(kToneMaxBins == kMaxBins  &&  kToneMaxMulti == kMaxMulti, "tone_bank.hpp restates these for the other units");

// Lanes per channel: 2 while the bank is too small to put >= 4 one-channel-per-lane waves
// on every SIMD (1024 SIMDs x 64 lanes x 4), else 1.  SPANGPU_LPC=1|2 overrides (tuning).
static std::atomic<int> g_forced_lpc{-1};     // (the tuning knobs are process-wide and may be turned from any thread: relaxed atomics, read once per use)

static int forced_lpc(void)
{
    int v = g_forced_lpc.load(std::memory_order_relaxed);
    if (v < 0)
    {
        const char *e = getenv("SPANGPU_LPC");
        v = (e  &&  (e[0] == '1'  ||  e[0] == '2'))  ?  (e[0] - '0')  :  0;
        g_forced_lpc.store(v, std::memory_order_relaxed);
    }
    return v;
}

// the general kernel's mapping
static int pick_lpc(int n_ch)
{
    const int f = forced_lpc();
    if (f)
        return f;
    return (n_ch < 262144)  ?  2  :  1;
}

// Which kernel family serves a launch: the streaming kernels (tone_fast.hpp) whenever the frame is channel-major with
// 16-byte aligned rows, else the general one (tone_dev.hpp: sample-major / unaligned frames, zero-length calls).  Of the
// streaming kernels, banks up to kLoaderMaxChannels take the one with a loader wave per workgroup (the consumer waves
// of a small bank are alone on their SIMDs: nothing covers a wave that stands in the memory pipeline's queue), larger
// banks the one in which every wave fetches for itself (there the other waves of the SIMD cover it, and a loader wave
// would only take a wave slot).  Crossover measured in profiles/r2_probe.log.  spangpu_tune_tone_kernel() forces one
// family (A-B measurements, parity tests of all of them).
static std::atomic<int> g_tone_variant{0};  // 0 auto, 1 general, 2 streaming with loader waves, 3 streaming without
constexpr int kLoaderMaxChannels = 393216;

static bool fast_eligible(const ToneLaunch &L)
{
    return g_tone_variant != 1  &&  L.layout == 0  &&  L.aligned16  &&  L.samples > 0  &&  !L.lens_ragged
           &&  (unsigned long long) L.stride*2ull*256ull < 0xFFFFFFFFull  &&  L.n_ch <= (1 << 29);
}

static bool use_loader(int n_ch)
{
    if (g_tone_variant == 2)
        return true;
    if (g_tone_variant == 3)
        return false;
    return n_ch <= kLoaderMaxChannels;
}

constexpr int kFastWPB = 4;
constexpr int kRingLoader = 2;          // segment slots per consumer wave, kernels with a loader wave
constexpr int kRingSelf = 2;            // ... kernels whose waves fetch for themselves (three slots measured slower: r2_probe.log)

template <class Det> struct is_super_tone { static constexpr bool value = false; };
template <int N> struct is_super_tone<MultiDet<N, true>> { static constexpr bool value = true; };
static thread_local bool g_cadence_fused = false;   // the launch this thread just made matched the cadences in its epilogue

template <class Det, int LPC, bool G711>
static void launch_fast(const ToneLaunch &L, hipStream_t st, bool loader)
{
    const int waves = (L.n_ch + kWave/LPC - 1)/(kWave/LPC);
    const int blocks = (L.wgn > 0)  ?  L.wgn  :  (waves + kFastWPB - 1)/kFastWPB;
    if constexpr (is_super_tone<Det>::value  &&  LPC == 1  &&  !G711)
    {
        if (L.cad.state)
        {
            if (loader)
                launch_tone_fast<Det, 1, kRingLoader, false, false, kFastWPB, kToneCadence, true>(L, blocks, st);
            else
                launch_tone_fast<Det, 1, kRingSelf, false, false, kFastWPB, kToneCadence, false>(L, blocks, st);
            g_cadence_fused = true;
            return;
        }
    }
    if constexpr (Det::kDigits)
    {
        // a launch that also reports one digit byte per block runs the variant with those stores compiled in
        if (L.digits)
        {
            if (loader  &&  LPC == 1)
                launch_tone_fast<Det, 1, kRingLoader, G711, false, kFastWPB, kToneDigits, true>(L, blocks, st);
            else
                launch_tone_fast<Det, LPC, kRingSelf, G711, false, kFastWPB, kToneDigits, false>(L, blocks, st);
            return;
        }
    }
    if (loader  &&  LPC == 1)
        launch_tone_fast<Det, 1, kRingLoader, G711, false, kFastWPB, 0, true>(L, blocks, st);
    else
        launch_tone_fast<Det, LPC, kRingSelf, G711, false, kFastWPB, 0, false>(L, blocks, st);
}

template <class Det, int LPC>
static void launch_general(const ToneLaunch &L, hipStream_t st)
{
    const int waves = (L.n_ch + kWave/LPC - 1)/(kWave/LPC);
    const int blocks = (waves + kWavesPerBlock - 1)/kWavesPerBlock;
    if constexpr (Det::kDigits)
    {
        if (L.digits)
        {
            hipLaunchKernelGGL((tone_bank_kernel<Det, LPC, kToneDigits>), dim3(blocks), dim3(kWave*kWavesPerBlock), 0, st, L);
            return;
        }
    }
    hipLaunchKernelGGL((tone_bank_kernel<Det, LPC>), dim3(blocks), dim3(kWave*kWavesPerBlock), 0, st, L);
}

template <class Det>
static void launch_tone(const ToneLaunch &L, hipStream_t st)
{
    // Lanes per channel: the streaming kernels run one channel per lane unless two are asked for (the split mapping
    // only ever paid on the general kernel, for banks too small to give every SIMD two waves).
    if (fast_eligible(L)  &&  !(L.fmt != 0  &&  forced_lpc() == 2))
    {
        const bool loader = use_loader(L.n_ch);
        if (L.fmt != 0)
            launch_fast<Det, 1, true>(L, st, loader);
        else if (g_forced_lpc == 2)
            launch_fast<Det, 2, false>(L, st, false);
        else
            launch_fast<Det, 1, false>(L, st, loader);
        return;
    }
    if (L.fmt != 0  ||  pick_lpc(L.n_ch) == 2)              // G.711 input: the LPC = 2 kernels hold the decode table
        launch_general<Det, 2>(L, st);
    else
        launch_general<Det, 1>(L, st);
}

// Banks of more than 16 bins per channel: always two lanes per channel (16 bins = 8 packed pairs per lane is what one
// lane's registers hold), linear PCM only; the streaming kernel without loader waves where the frame allows it.
template <class Det>
static void launch_tone_wide(const ToneLaunch &L, hipStream_t st)
{
    const int waves = (L.n_ch + 31)/32;
    const int blocks = (waves + kWavesPerBlock - 1)/kWavesPerBlock;
    if (fast_eligible(L)  &&  L.fmt == 0)
        launch_tone_fast<Det, 2, kRingSelf, false, false, kFastWPB, 0, false>(L, blocks, st);
    else
        hipLaunchKernelGGL((tone_bank_kernel<Det, 2>), dim3(blocks), dim3(kWave*kWavesPerBlock), 0, st, L);
}

// Banks of more than 32 bins per channel (a super-tone descriptor may name 64 pitches, private/super_tone_rx.h:44): four
// lanes per channel, 16 channels per wavefront, the general kernel.
template <class Det>
static void launch_tone_quad(const ToneLaunch &L, hipStream_t st)
{
    const int waves = (L.n_ch + 15)/16;
    const int blocks = (waves + kWavesPerBlock - 1)/kWavesPerBlock;
    hipLaunchKernelGGL((tone_bank_kernel<Det, 4>), dim3(blocks), dim3(kWave*kWavesPerBlock), 0, st, L);
}

// The digits of the last launch as a compact list, for reports that leave the GPU (an RCCL gather to another rank, a
// small D2H copy): out[0] = number of blocks in which the detector accepted a digit, out[1 + i] = channel | code << 20 |
// block << 28, in no particular order.  `accept` = the flag that marks such a block when its code is not zero:
// SPANGPU_BLK_CHANGE for DTMF (dtmf.c:318-340), SPANGPU_BLK_REPORT for Bell MF (bell_r2_mf.c:629-655) and R2 MF (:869-875;
// the end of a tone is reported with code 0 and is no digit) -- those two never set SPANGPU_BLK_CHANGE, and their lists were
// empty while this kernel asked for it.
// A 65536-channel DTMF tick has 131072 record words and, on live lines, a few thousand such blocks.
__global__ __launch_bounds__(256) void digit_events_kernel(const uint32_t *rec, int n_ch, int maxb, uint32_t *out, int cap, uint32_t accept)
{
    const int ch = (int) (blockIdx.x*256 + threadIdx.x);
    if (ch >= n_ch)
        return;
    for (int b = 0;  b < maxb;  b++)
    {
        const uint32_t w = rec[(size_t) b*n_ch + ch];
        const uint32_t flags = (w >> 16) & 0xFF;
        const uint32_t code = (w >> 8) & 0xFF;
        if ((flags & kBlkValid)  &&  (flags & accept)  &&  code)
        {
            const uint32_t at = atomicAdd(out, 1u);
            if (at < (uint32_t) cap)
                out[1 + at] = (uint32_t) ch | (code << 20) | ((uint32_t) b << 28);
        }
    }
}

static void fill_launch(ToneLaunch &L, spangpu_bank_t *b, const int16_t *d_amp, long long d_stride, int samples, int layout,
                        int maxb, int force_end)
{
    memset(&L, 0, sizeof(L));
    L.amp = d_amp;
    L.stride = d_stride;
    L.samples = samples;
    L.n_ch = b->c.n_ch;
    L.layout = layout;
    L.fmt = b->next_fmt;
    L.lens = b->lens.next;
    L.lens_ragged = (b->lens.next  &&  b->next_ragged)  ?  1  :  0;
    L.chan_parms = b->chan_parms;
    L.digits = nullptr;
    if (b->ext_digits  &&  (size_t) maxb*b->c.n_ch <= b->ext_digits_bytes)
    {
        L.digits = b->ext_digits + (size_t) b->ext_digits_next*b->ext_digits_bytes;
        b->ext_digits_next = (b->ext_digits_next + 1 < b->ext_digits_slices)  ?  (b->ext_digits_next + 1)  :  0;
    }
    L.functor = (b->kind == SPANGPU_GOERTZEL)  ?  b->tp.functor  :  0;
    L.functor_threshold = b->tp.functor_threshold;
    {
        const int spc = L.fmt  ?  16  :  8;                 // samples per 16 bytes
        L.aligned16 = (layout == SPANGPU_LAYOUT_CHANNEL_MAJOR
                       &&  (((uintptr_t) d_amp) & 15) == 0
                       &&  (d_stride & (spc - 1)) == 0
                       &&  d_stride >= ((samples + spc - 1) & ~(spc - 1)))  ?  1  :  0;
    }
    L.sf = b->sf;
    L.si = b->si;
    L.rec = b->ext_rec  ?  b->ext_rec  :  b->rec;
    b->cur_rec = L.rec;
    memset(&L.cad, 0, sizeof(L.cad));
    if (b->cad)
    {
        // the streaming kernel matches the cadences in its epilogue when the event buffers hold this launch's slots and
        // every channel takes part (launch_fast() decides; any other kernel leaves them to cadence_kernel)
        b->cad->fused = false;
        b->cad->list_due = false;
        if (kCadSlotsPerBlock*maxb <= b->cad->slots_cap  &&  maxb > 0  &&  b->lens.next == nullptr  &&  !force_end
            &&  b->cad->n_tones <= kCadLdsTones  &&  b->cad->n_elems <= kCadLdsElems)
            cadence_args(b, b->cad, L.cad, b->cad->which ^ 1);
    }
    L.rec_energy = b->rec_energy;
    L.rec_dur = b->rec_dur;
    L.trace = b->trace;
    L.maxb = maxb;
    L.nbins = (b->kind == SPANGPU_SUPER_TONE  ||  b->kind == SPANGPU_GOERTZEL)  ?  b->tp.n_bins  :  b->nb;
    L.block_len = b->block_len;
    L.force_end = force_end;
    L.realtime = (b->kind == SPANGPU_DTMF  &&  b->tp.report_mode == SPANGPU_REPORT_REALTIME)  ?  1  :  0;
    for (int i = 0;  i < kMaxBins;  i++)
        L.fac[i] = b->fac[i];
    L.threshold = b->threshold;
    L.normal_twist = b->normal_twist;
    L.reverse_twist = b->reverse_twist;
}

static int launch_bank(spangpu_bank_t *b, const int16_t *d_amp, long long d_stride, int samples, int layout, int maxb, int force_end)
{
    const int caught = cadence_catch_up(b);
    if (caught != SPANGPU_OK)
        return caught;
    ToneLaunch L;
    fill_launch(L, b, d_amp, d_stride, samples, layout, maxb, force_end);

    // Queue mode: a launch the one-lane streaming kernel serves, of a bank of at least two workgroups per half and without
    // cadences (their epilogue's list is made on the bank's stream), goes out as two launches on two streams; the second stream
    // first waits for what the bank's stream holds now (the caller's frame, an earlier launch of another kind).  Anything
    // else joins the second stream into the bank's stream and runs there as ever.
    const int total_wg = (b->c.n_ch + kWave*kFastWPB - 1)/(kWave*kFastWPB);
    const bool split = b->queues == 2  &&  b->stream2 != nullptr  &&  !b->timing  &&  b->cad == nullptr  &&  b->nb <= 16  &&  total_wg >= 4
                       &&  fast_eligible(L)  &&  forced_lpc() != 2;
    if (split  &&  b->main_touched)
    {
        // something else went onto the bank's stream since the last split launch (a state edit, a launch of the other kernel
        // family, work of the caller's behind spangpu_bank_get_stream() / _join()): the second half runs behind it
        SPG_TRY(hipEventRecord(b->ev_in, b->c.stream));
        SPG_TRY(hipStreamWaitEvent(b->stream2, b->ev_in, 0));
        b->main_touched = false;
    }
    for (int half = 0;  half < (split  ?  2  :  1);  half++)
    {
    hipStream_t st = split  ?  b->c.stream  :  joined(b);
    if (split)
    {
        L.wg0 = half  ?  total_wg/2  :  0;
        L.wgn = half  ?  (total_wg - total_wg/2)  :  total_wg/2;
        st = half  ?  b->stream2  :  b->c.stream;
    }
    if (b->timing)
        SPG_TRY(hipEventRecord(b->ev0, st));
    g_cadence_fused = false;
    switch (b->kind)
    {
    case SPANGPU_DTMF:
        if (b->chan_parms  ?  (b->n_filter_on > 0)  :  (b->tp.filter_dialtone != 0))
            launch_tone<DtmfDet<true>>(L, st);
        else
            launch_tone<DtmfDet<false>>(L, st);
        break;
    case SPANGPU_BELL_MF:
        launch_tone<BellMfDet>(L, st);
        break;
    case SPANGPU_R2_MF:
        launch_tone<R2MfDet>(L, st);
        break;
    case SPANGPU_SUPER_TONE:
        switch (b->nb)
        {
        case 4:  launch_tone<MultiDet<4, true>>(L, st);  break;
        case 8:  launch_tone<MultiDet<8, true>>(L, st);  break;
        case 12: launch_tone<MultiDet<12, true>>(L, st); break;
        case 16: launch_tone<MultiDet<16, true>>(L, st); break;
        case 24: launch_tone_wide<MultiDet<24, true>>(L, st); break;
        case 32: launch_tone_wide<MultiDet<32, true>>(L, st); break;
        default: launch_tone_quad<MultiDet<64, true>>(L, st); break;
        }
        break;
    case SPANGPU_GOERTZEL:
        switch (b->nb)
        {
        case 4:  launch_tone<MultiDet<4, false>>(L, st);  break;
        case 8:  launch_tone<MultiDet<8, false>>(L, st);  break;
        case 12: launch_tone<MultiDet<12, false>>(L, st); break;
        case 16: launch_tone<MultiDet<16, false>>(L, st); break;
        case 24: launch_tone_wide<MultiDet<24, false>>(L, st); break;
        case 32: launch_tone_wide<MultiDet<32, false>>(L, st); break;
        default: launch_tone_quad<MultiDet<64, false>>(L, st); break;
        }
        break;
    default:
        return failf(SPANGPU_ERR_UNSUPPORTED, "kind %d", b->kind);
    }
    SPG_TRY(hipGetLastError());
    }
    if (split)
        b->s2_busy = true;
    if (b->cad  &&  g_cadence_fused)
    {
        b->cad->fused = true;
        b->cad->list_due = true;
    }
    if (b->timing)
    {
        SPG_TRY(hipEventRecord(b->ev1, joined(b)));
        b->ev_valid = true;
    }
    return SPANGPU_OK;
}

// Before a receive path's launch: the blocks of the call, room for their outputs, a records buffer of the caller's checked ...
static int rx_prepare(spangpu_bank_t *b, int samples, int *maxb)
{
    *maxb = (samples + b->block_len - 1)/b->block_len;
    const int rc = (*maxb <= b->maxb_cap)  ?  SPANGPU_OK  :  ensure_outputs(b, (*maxb > 0)  ?  *maxb  :  1);      // (no call where there is room)
    if (rc != SPANGPU_OK)
        return rc;
    if (b->ext_rec  &&  (size_t) *maxb*b->c.n_ch*sizeof(uint32_t) > b->ext_rec_bytes)
        return failf(SPANGPU_ERR_BAD_ARG, "records buffer too small for %d blocks", *maxb);
    return SPANGPU_OK;
}

// ... and behind it: what the read-backs and the cadence matcher know the last call by
static void rx_done(spangpu_bank_t *b, int maxb, int samples)
{
    b->last_maxb = maxb;
    b->launch_serial++;
    b->last_samples = samples;
}

// A host caller's frame into the bank's one staging block (grow-only, in int16 units whatever the format, 16 bytes to spare): `rows`
// rows of `width` bytes, `pitch` bytes apart at the caller's, `d_pitch` in the block.  Waited for: the frame is only borrowed.
static int stage_frame(spangpu_bank_t *b, const void *src, size_t pitch, size_t d_pitch, size_t width, size_t rows)
{
    const hipStream_t st = joined(b);
    const int rc = grow(&b->d_amp, &b->d_amp_cap, (d_pitch*rows + 16 + 1)/2, 1, st);
    if (rc != SPANGPU_OK)
        return rc;
    SPG_TRY(hipMemcpy2DAsync(b->d_amp, d_pitch, src, pitch, width, rows, hipMemcpyHostToDevice, st));
    SPG_TRY(hipStreamSynchronize(st));
    return SPANGPU_OK;
}

extern "C" {

int spangpu_tune_lanes_per_channel(int lpc)
{
    if (lpc != 0  &&  lpc != 1  &&  lpc != 2)
        return failf(SPANGPU_ERR_BAD_ARG, "lanes per channel must be 0 (auto), 1 or 2");
    g_forced_lpc = lpc;
    return SPANGPU_OK;
}

int spangpu_tune_tone_kernel(int variant)
{
    if (variant < 0  ||  variant > 3)
        return failf(SPANGPU_ERR_BAD_ARG, "variant must be 0 (auto), 1 (general), 2 (streaming, loader waves) or 3 (streaming)");
    g_tone_variant = variant;
    return SPANGPU_OK;
}

int spangpu_bank_rx(spangpu_bank_t *b, const int16_t *amp, int mem, int layout, int samples, long long stride)
{
    if (b == nullptr  ||  amp == nullptr  ||  samples < 0)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (layout != SPANGPU_LAYOUT_CHANNEL_MAJOR  &&  layout != SPANGPU_LAYOUT_SAMPLE_MAJOR)
        return failf(SPANGPU_ERR_BAD_ARG, "bad layout");
    if (samples == 0)
        return 0;
    SPG_TRY(hipSetDevice(b->c.device));
    const bool chan_major = (layout == SPANGPU_LAYOUT_CHANNEL_MAJOR);
    if (stride <= 0)
        stride = chan_major  ?  samples  :  b->c.n_ch;
    if (mem_kind_ok(mem) != SPANGPU_OK)             // refused first, as ever: before the size of a caller's records buffer
        return SPANGPU_ERR_BAD_ARG;
    int maxb;
    int rc = rx_prepare(b, samples, &maxb);
    if (rc != SPANGPU_OK)
        return rc;

    const int16_t *d_amp = amp;
    long long d_stride = stride;
    if (mem == SPANGPU_MEM_HOST)
    {
        // staged rows are the call's samples rounded up to 8 apart, or, sample-major, one sample of every channel
        d_stride = chan_major  ?  ((samples + 7) & ~7LL)  :  b->c.n_ch;
        const size_t width = chan_major  ?  samples  :  b->c.n_ch;
        if ((rc = stage_frame(b, amp, stride*sizeof(int16_t), d_stride*sizeof(int16_t), width*sizeof(int16_t), chan_major  ?  b->c.n_ch  :  samples)) != SPANGPU_OK)
            return rc;
        d_amp = b->d_amp;
    }
    rc = launch_bank(b, d_amp, d_stride, samples, layout, maxb, 0);
    if (rc < 0)
        return rc;
    rx_done(b, maxb, samples);
    return 0;
}

// spangpu_bank_rx() for a tick in which not every channel has a frame, or not all frames are of one length: channel c
// takes part with lens[c] samples of its row (0: it sits the call out -- its filters, block phase and debounce state are
// exactly as they were, and it reports no block).  lens[] is host memory whatever `mem` says; frames are channel-major.
int spangpu_bank_rx_var(spangpu_bank_t *b, const int16_t *amp, int mem, const int32_t *lens, int max_samples, long long stride)
{
    if (b == nullptr  ||  amp == nullptr  ||  lens == nullptr  ||  max_samples < 0)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int longest = 0;
    bool all = true;
    int rc = lens_check(lens, b->c.n_ch, max_samples, &longest, &all);
    if (rc != SPANGPU_OK  ||  longest == 0)
        return rc;
    if (stride <= 0)
        stride = max_samples;
    if (all)
        return spangpu_bank_rx(b, amp, mem, SPANGPU_LAYOUT_CHANNEL_MAJOR, longest, stride);
    bool ragged = false;
    for (int c = 0;  c < b->c.n_ch;  c++)
        ragged |= (lens[c] != 0  &&  lens[c] != longest);
    (void) joined(b);
    if ((rc = lens_upload(&b->c, &b->lens, lens)) != SPANGPU_OK)
        return rc;
    b->next_ragged = ragged;
    rc = spangpu_bank_rx(b, amp, mem, SPANGPU_LAYOUT_CHANNEL_MAJOR, longest, stride);
    b->lens.next = nullptr;
    b->next_ragged = false;
    return rc;
}

// spangpu_bank_rx() for G.711 input: `codes` holds one A-law or u-law byte per sample, channel-major (the wire format
// of a trunk); the kernel decodes through a 256-entry table in LDS (alaw_to_linear / ulaw_to_linear,
// src/spandsp/g711.h:165-175,239-252), so the PCM read traffic of the detector is halved and no decode pass is needed.
int spangpu_bank_rx_g711(spangpu_bank_t *b, const uint8_t *codes, int mem, int law, int samples, long long stride)
{
    if (b == nullptr  ||  codes == nullptr  ||  samples < 0)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (law != SPANGPU_G711_ALAW  &&  law != SPANGPU_G711_ULAW)
        return failf(SPANGPU_ERR_BAD_ARG, "law must be SPANGPU_G711_ALAW or SPANGPU_G711_ULAW");
    if (samples == 0)
        return 0;
    SPG_TRY(hipSetDevice(b->c.device));
    if (stride <= 0)
        stride = samples;
    if (mem_kind_ok(mem) != SPANGPU_OK)             // refused first, as ever: before the size of a caller's records buffer
        return SPANGPU_ERR_BAD_ARG;
    int maxb;
    int rc = rx_prepare(b, samples, &maxb);
    if (rc != SPANGPU_OK)
        return rc;
    const uint8_t *d_codes = codes;
    long long d_stride = stride;
    if (mem == SPANGPU_MEM_HOST)
    {
        d_stride = (samples + 15) & ~15LL;              // staged rows are the call's samples rounded up to 16 apart, in bytes
        if ((rc = stage_frame(b, codes, stride, d_stride, samples, b->c.n_ch)) != SPANGPU_OK)
            return rc;
        d_codes = (const uint8_t *) b->d_amp;
    }
    b->next_fmt = law;
    rc = launch_bank(b, (const int16_t *) d_codes, d_stride, samples, SPANGPU_LAYOUT_CHANNEL_MAJOR, maxb, 0);
    b->next_fmt = 0;
    if (rc < 0)
        return rc;
    rx_done(b, maxb, samples);
    return 0;
}

// Several banks, one launch (tone_multi_kernel): banks[k] is advanced by `samples` samples of amps[k].  All banks must
// be on the same device and stream and hold device-resident, channel-major frames; kinds that can share a launch are
// DTMF (without the dial-tone filter), Bell MF, R2 MF and super-tone.  Results are read per bank as after
// spangpu_bank_rx().
int spangpu_banks_rx(spangpu_bank_t *const *banks, const int16_t *const *amps, int n_banks, int samples, const long long *strides)
{
    if (banks == nullptr  ||  amps == nullptr  ||  n_banks < 1  ||  n_banks > kMaxMulti  ||  samples < 0)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments (at most %d banks per launch)", kMaxMulti);
    if (samples == 0)
        return 0;
    ToneMultiLaunch M;
    memset(&M, 0, sizeof(M));
    int total_ch = 0;
    for (int k = 0;  k < n_banks;  k++)
    {
        spangpu_bank_t *b = banks[k];
        if (b == nullptr  ||  amps[k] == nullptr)
            return failf(SPANGPU_ERR_BAD_ARG, "null bank or frame");
        if (b->c.device != banks[0]->c.device)
            return failf(SPANGPU_ERR_BAD_ARG, "banks of one call must be on one device");
        total_ch += b->c.n_ch;
    }
    // Banks that were given streams of their own (spangpu_bank_set_stream) are advanced by a launch each, every one on its
    // bank's stream: free-running hardware queues put one bank's launch boundary, start burst and write-back under the other
    // banks' steady state (configs[2], 131 072 channels in three banks: 23.7 us a tick as one launch, 18.4 us as three
    // launches on three streams; three launches on ONE stream 32.3 -- profiles/r5_mixed_streams.log).
    // (Round 6: banks are grouped by stream -- those that share one share a launch on it, a bank alone on its stream gets its
    // own: configs[2] as Bell MF + R2 MF in one launch on one queue beside the super-tone bank with its cadence matcher on
    // another balances the two queues.)
    bool own_streams = false;
    for (int k = 1;  k < n_banks;  k++)
        own_streams = own_streams  ||  (banks[k]->c.stream != banks[0]->c.stream);
    if (own_streams)
    {
        bool done[kMaxMulti] = {false, false, false, false};
        for (int k = 0;  k < n_banks;  k++)
        {
            if (done[k])
                continue;
            spangpu_bank_t *grp[kMaxMulti];
            const int16_t *gamps[kMaxMulti];
            long long gstrides[kMaxMulti];
            int n = 0;
            for (int j = k;  j < n_banks;  j++)
            {
                if (!done[j]  &&  banks[j]->c.stream == banks[k]->c.stream)
                {
                    grp[n] = banks[j];
                    gamps[n] = amps[j];
                    gstrides[n] = strides  ?  strides[j]  :  0;
                    n++;
                    done[j] = true;
                }
            }
            const int rc = (n == 1)  ?  spangpu_bank_rx(grp[0], gamps[0], SPANGPU_MEM_DEVICE, SPANGPU_LAYOUT_CHANNEL_MAJOR, samples, gstrides[0])
                                     :  spangpu_banks_rx(grp, gamps, n, samples, strides  ?  gstrides  :  nullptr);
            if (rc < 0)
                return rc;
        }
        return 0;
    }
    for (int k = 0;  k < n_banks;  k++)
        (void) joined(banks[k]);
    SPG_TRY(hipSetDevice(banks[0]->c.device));
    bool all_fast = true;
    for (int k = 0;  k < n_banks;  k++)
    {
        spangpu_bank_t *b = banks[k];
        switch (b->kind)
        {
        case SPANGPU_DTMF:
            // the shared launch runs the unfiltered detector: what counts is whether any channel's filter is on (a bank
            // given per-channel parameters keeps the switch per channel; launch_bank() tests the same)
            if (b->chan_parms  ?  (b->n_filter_on > 0)  :  (b->tp.filter_dialtone != 0))
                return failf(SPANGPU_ERR_UNSUPPORTED, "a DTMF bank with a dial-tone filter switched on cannot share a launch");
            M.kind[k] = TONE_K_DTMF;
            break;
        case SPANGPU_BELL_MF: M.kind[k] = TONE_K_BELL; break;
        case SPANGPU_R2_MF: M.kind[k] = TONE_K_R2; break;
        case SPANGPU_SUPER_TONE:
            if (b->nb > 16)
                return failf(SPANGPU_ERR_UNSUPPORTED, "a super-tone bank of more than 16 bins cannot share a launch");
            M.kind[k] = (b->nb == 4)  ?  TONE_K_ST4  :  (b->nb == 8)  ?  TONE_K_ST8  :  (b->nb == 12)  ?  TONE_K_ST12  :  TONE_K_ST16;
            break;
        default:
            return failf(SPANGPU_ERR_UNSUPPORTED, "bank kind %d cannot share a launch", b->kind);
        }
        // the kernels of a shared launch write records, not digit bytes: a bank whose caller collects digit bytes
        // (spangpu_bank_set_digits_buffer / _ring) would hand on stale bytes and lose a slice of its ring
        if (b->ext_digits)
            return failf(SPANGPU_ERR_UNSUPPORTED, "a bank with a digits buffer cannot share a launch (it would get no digit bytes)");
        const long long stride = (strides  &&  strides[k] > 0)  ?  strides[k]  :  samples;
        int maxb;
        const int rc = rx_prepare(b, samples, &maxb);
        if (rc != SPANGPU_OK)
            return rc;
        const int caught = cadence_catch_up(b);
        if (caught != SPANGPU_OK)
            return caught;
        fill_launch(M.bank[k], b, amps[k], stride, samples, SPANGPU_LAYOUT_CHANNEL_MAJOR, maxb, 0);
        all_fast = all_fast  &&  fast_eligible(M.bank[k]);
        rx_done(b, maxb, samples);
    }
    // lanes per channel: the streaming kernels run one channel per lane unless two are asked for
    const int lpc = all_fast  ?  ((forced_lpc() == 2)  ?  2  :  1)  :  pick_lpc(total_ch);
    const int cpw = kWave/lpc;
    // Workgroups are dispatched in index order and a launch of this kind fills the chip more than once: the detectors with
    // the most work per channel go first, so that what runs last, when the chip drains, is the cheap kind (the super-tone
    // banks' workgroups at the end of the range left a tail of their own length; measured in tools/bench_paths.py mixed).
    auto cost = [](int kind) { return (kind == TONE_K_ST16)  ?  6  :  (kind == TONE_K_ST12)  ?  5  :  (kind == TONE_K_ST8)  ?  4
                                      :  (kind == TONE_K_DTMF)  ?  3  :  (kind == TONE_K_ST4)  ?  2  :  1; };
    for (int i = 1;  i < n_banks;  i++)
    {
        for (int k = i;  k > 0  &&  cost(M.kind[k]) > cost(M.kind[k - 1]);  k--)
        {
            const int kk = M.kind[k];
            M.kind[k] = M.kind[k - 1];
            M.kind[k - 1] = kk;
            const ToneLaunch tl = M.bank[k];
            M.bank[k] = M.bank[k - 1];
            M.bank[k - 1] = tl;
        }
    }
    int first = 0;
    for (int k = 0;  k < n_banks;  k++)
    {
        M.first[k] = first;
        const int waves = (M.bank[k].n_ch + cpw - 1)/cpw;
        first += (waves + kWavesPerBlock - 1)/kWavesPerBlock;
    }
    for (int k = n_banks;  k <= kMaxMulti;  k++)
        M.first[k] = first;
    M.n = n_banks;
    static_assert(kFastWPB == kWavesPerBlock, "the workgroup ranges above serve both kernel families");
    if (all_fast)
    {
        // the streaming kernels read their prologue's flags from the aligned16 slot (tone_fast.hpp: kFast...)
        for (int k = 0;  k < n_banks;  k++)
            M.bank[k].aligned16 = tone_fast_flags(M.bank[k]);
    }
    if (all_fast  &&  lpc == 1  &&  use_loader(total_ch))
        hipLaunchKernelGGL((tone_multi_fast_kernel<1, kRingLoader, true>), dim3(first), dim3(kWave*(kWavesPerBlock + 1)), 0, banks[0]->c.stream, M);
    else if (all_fast  &&  lpc == 1)
        hipLaunchKernelGGL((tone_multi_fast_kernel<1, kRingSelf, false>), dim3(first), dim3(kWave*kWavesPerBlock), 0, banks[0]->c.stream, M);
    else if (all_fast)
        hipLaunchKernelGGL((tone_multi_fast_kernel<2, kRingSelf, false>), dim3(first), dim3(kWave*kWavesPerBlock), 0, banks[0]->c.stream, M);
    else if (lpc == 2)
        hipLaunchKernelGGL(tone_multi_kernel<2>, dim3(first), dim3(kWave*kWavesPerBlock), 0, banks[0]->c.stream, M);
    else
        hipLaunchKernelGGL(tone_multi_kernel<1>, dim3(first), dim3(kWave*kWavesPerBlock), 0, banks[0]->c.stream, M);
    SPG_TRY(hipGetLastError());
    return 0;
}

int spangpu_bank_force_block(spangpu_bank_t *b)
{
    if (b == nullptr)
        return failf(SPANGPU_ERR_BAD_ARG, "null bank");
    SPG_TRY(hipSetDevice(b->c.device));
    int rc = ensure_outputs(b, 1);
    if (rc != SPANGPU_OK)
        return rc;
    rc = launch_bank(b, nullptr, 0, 0, SPANGPU_LAYOUT_CHANNEL_MAJOR, 1, 1);
    if (rc < 0)
        return rc;
    rx_done(b, 1, 0);
    return SPANGPU_OK;
}

int spangpu_bank_digit_events(spangpu_bank_t *b, uint32_t *dst_device, int cap_entries)
{
    if (b == nullptr  ||  dst_device == nullptr  ||  cap_entries < 0)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (b->c.n_ch > (1 << 20)  ||  b->last_maxb > 16)
        return failf(SPANGPU_ERR_UNSUPPORTED, "digit events pack the channel in 20 bits and the block in 4");
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipMemsetAsync(dst_device, 0, sizeof(uint32_t), joined(b)));
    if (b->last_maxb > 0)
    {
        hipLaunchKernelGGL(digit_events_kernel, dim3((b->c.n_ch + 255)/256), dim3(256), 0, joined(b),
                           (const uint32_t *) records_of(b), b->c.n_ch, b->last_maxb, dst_device, cap_entries,
                           (uint32_t) ((b->kind == SPANGPU_BELL_MF  ||  b->kind == SPANGPU_R2_MF)  ?  kBlkReport  :  kBlkChange));
        SPG_TRY(hipGetLastError());
    }
    return SPANGPU_OK;
}

}   // extern "C"

// ---- test hook: the two block-end decisions of a detector side by side -----------------------------------------------
// Det::decide() (the reference's scan, every option) and Det::decide_plain() (the production case of the streaming kernels)
// on caller-made energies and history words -- ties among the energies, zeros, values either side of every threshold: cases a
// synthesised signal reaches rarely or never (tests/test_tone_gpu.py: test_lean_block_end_*).  kind: SPANGPU_DTMF, _BELL_MF, _R2_MF.
// e: [n][8] floats (the MF detectors use the first six), energy / w0 / w1: [n]; out: [6][n] words: record, w0, w1 of decide(), then
// of decide_plain().  Host pointers.  Not part of the drop-in boundary.
template <class Det>
__global__ void debug_decide_kernel(const float *e8, const float *energy, const uint32_t *w0in, const int32_t *w1in, uint32_t *out, int n, const ToneLaunch L)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    float e[Det::NB];
#pragma unroll
    for (int k = 0;  k < Det::NB;  k++)
        e[k] = e8[(size_t) i*8 + k];
    Det det;
    det.load_extra(L, 0);
    float en = energy[i];
    uint32_t w0 = w0in[i] & 0xFFFF0000u;
    int32_t w1 = w1in[i];
    out[i] = det.decide(L, e, en, w0, w1, 0, 0, false);
    out[(size_t) n + i] = w0;
    out[(size_t) 2*n + i] = (uint32_t) w1;
    en = energy[i];
    w0 = w0in[i] & 0xFFFF0000u;
    w1 = w1in[i];
    if constexpr (Det::kLean)
        out[(size_t) 3*n + i] = det.decide_plain(L, e, en, w0, w1);
    out[(size_t) 4*n + i] = w0;
    out[(size_t) 5*n + i] = (uint32_t) w1;
}

extern "C" __attribute__((visibility("default")))
int spangpu_debug_decide(int kind, const float *e8, const float *energy, const uint32_t *w0, const int32_t *w1, uint32_t *out, int n)
{
    if (e8 == nullptr  ||  energy == nullptr  ||  w0 == nullptr  ||  w1 == nullptr  ||  out == nullptr  ||  n <= 0)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    ToneLaunch L;
    memset(&L, 0, sizeof(L));
    L.n_ch = 1;
    L.threshold = 171029200.0f;         // dtmf.c:104-110
    L.normal_twist = 6.309f;
    L.reverse_twist = 2.512f;
    float *d_e = nullptr, *d_en = nullptr;
    uint32_t *d_w0 = nullptr, *d_out = nullptr;
    int32_t *d_w1 = nullptr;
    SPG_TRY(hipMalloc(&d_e, (size_t) n*8*sizeof(float)));
    SPG_TRY(hipMalloc(&d_en, (size_t) n*sizeof(float)));
    SPG_TRY(hipMalloc(&d_w0, (size_t) n*4));
    SPG_TRY(hipMalloc(&d_w1, (size_t) n*4));
    SPG_TRY(hipMalloc(&d_out, (size_t) n*6*4));
    SPG_TRY(hipMemcpy(d_e, e8, (size_t) n*8*sizeof(float), hipMemcpyHostToDevice));
    SPG_TRY(hipMemcpy(d_en, energy, (size_t) n*sizeof(float), hipMemcpyHostToDevice));
    SPG_TRY(hipMemcpy(d_w0, w0, (size_t) n*4, hipMemcpyHostToDevice));
    SPG_TRY(hipMemcpy(d_w1, w1, (size_t) n*4, hipMemcpyHostToDevice));
    SPG_TRY(hipMemset(d_out, 0, (size_t) n*6*4));
    const dim3 grid((n + 255)/256), block(256);
    if (kind == SPANGPU_DTMF)
        hipLaunchKernelGGL(debug_decide_kernel<DtmfDet<false>>, grid, block, 0, 0, d_e, d_en, d_w0, d_w1, d_out, n, L);
    else if (kind == SPANGPU_BELL_MF)
        hipLaunchKernelGGL(debug_decide_kernel<BellMfDet>, grid, block, 0, 0, d_e, d_en, d_w0, d_w1, d_out, n, L);
    else if (kind == SPANGPU_R2_MF)
        hipLaunchKernelGGL(debug_decide_kernel<R2MfDet>, grid, block, 0, 0, d_e, d_en, d_w0, d_w1, d_out, n, L);
    else
        return failf(SPANGPU_ERR_UNSUPPORTED, "no lean block end for detector kind %d", kind);
    SPG_TRY(hipGetLastError());
    SPG_TRY(hipMemcpy(out, d_out, (size_t) n*6*4, hipMemcpyDeviceToHost));
    (void) hipFree(d_e); (void) hipFree(d_en); (void) hipFree(d_w0); (void) hipFree(d_w1); (void) hipFree(d_out);
    return SPANGPU_OK;
}
