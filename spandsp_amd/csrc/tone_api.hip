// tone_api.hip -- the tone bank's calls that launch no detector: bank lifetime, streams and queue mode, the per-call output
// blocks and their read-backs, the caller-owned record and digit buffers.  Owns the bank's HBM allocations (tone_bank.hpp).

#include <chrono>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "tone_cadence.hpp"

using namespace spg;

void free_outputs(spangpu_bank_t *b)
{
    if (b->cur_rec == b->rec)
        b->cur_rec = nullptr;           // (a records buffer of the caller's stays what it is)
    if (b->rec) (void) hipFree(b->rec);
    if (b->rec_energy) (void) hipFree(b->rec_energy);
    if (b->rec_dur) (void) hipFree(b->rec_dur);
    if (b->trace) (void) hipFree(b->trace);
    if (b->h_rec) (void) hipHostFree(b->h_rec);
    if (b->h_energy) (void) hipHostFree(b->h_energy);
    if (b->h_dur) (void) hipHostFree(b->h_dur);
    b->rec = nullptr;
    b->rec_energy = nullptr;
    b->rec_dur = nullptr;
    b->trace = nullptr;
    b->h_rec = nullptr;
    b->h_energy = nullptr;
    b->h_dur = nullptr;
    b->maxb_cap = 0;
}

int ensure_outputs(spangpu_bank_t *b, int maxb)
{
    if (maxb <= b->maxb_cap)
        return SPANGPU_OK;
    // The records of the launch before may still be owed to the cadence matcher (cadence_catch_up()): it reads them
    // from the buffer that is about to be freed, so it runs now, and has finished before the buffer goes.
    if (b->rec)
    {
        const int caught = cadence_catch_up(b);
        if (caught != SPANGPU_OK)
            return caught;
        SPG_TRY(hipStreamSynchronize(joined(b)));
    }
    free_outputs(b);
    const size_t n = (size_t) maxb*b->c.n_ch;
    SPG_TRY(hipMalloc(&b->rec, n*sizeof(uint32_t)));
    SPG_TRY(hipHostMalloc(&b->h_rec, n*sizeof(uint32_t)));
    const bool want_energy = (b->kind == SPANGPU_DTMF  &&  b->tp.report_mode == SPANGPU_REPORT_REALTIME)
                             ||  b->kind == SPANGPU_SUPER_TONE;
    if (want_energy)
    {
        SPG_TRY(hipMalloc(&b->rec_energy, n*sizeof(float)));
        SPG_TRY(hipHostMalloc(&b->h_energy, n*sizeof(float)));
        SPG_TRY(hipMemsetAsync(b->rec_energy, 0, n*sizeof(float), joined(b)));
    }
    if (b->kind == SPANGPU_DTMF  &&  b->tp.report_mode == SPANGPU_REPORT_REALTIME)
    {
        SPG_TRY(hipMalloc(&b->rec_dur, n*sizeof(int32_t)));
        SPG_TRY(hipHostMalloc(&b->h_dur, n*sizeof(int32_t)));
        SPG_TRY(hipMemsetAsync(b->rec_dur, 0, n*sizeof(int32_t), joined(b)));
    }
    if (b->tp.trace  ||  b->kind == SPANGPU_GOERTZEL)
    {
        SPG_TRY(hipMalloc(&b->trace, n*(b->nb + 1)*sizeof(float)));
        SPG_TRY(hipMemsetAsync(b->trace, 0, n*(b->nb + 1)*sizeof(float), joined(b)));
    }
    b->maxb_cap = maxb;
    return SPANGPU_OK;
}

extern "C" {

// make_goertzel_descriptor(), tone_detect.c:60-68: the argument is formed in double
// (M_PI is a double) and narrowed to float at the cosf() call.
float spangpu_goertzel_fac(float freq_hz)
{
    const double two_pi = 2.0f*3.14159265358979323846264338327;
    const float ratio = freq_hz/8000.0f;
    return 2.0f*cosf((float) (two_pi*ratio));
}

int spangpu_bank_create(spangpu_bank_t **bank, int device, int kind, int n_channels, const void *params, size_t params_size)
{
    if (bank == nullptr  ||  n_channels <= 0)
        return failf(SPANGPU_ERR_BAD_ARG, "bad bank/n_channels");
    *bank = nullptr;
    if (spangpu_device_count() <= 0)
        return failf(SPANGPU_ERR_NO_DEVICE, "no HIP device: libspangpu has no CPU fallback");
    if (device < 0  ||  device >= spangpu_device_count())
        return failf(SPANGPU_ERR_BAD_ARG, "device %d out of range", device);
    SPG_TRY(hipSetDevice(device));

    spangpu_bank_t *b = (spangpu_bank_t *) calloc(1, sizeof(*b));
    if (b == nullptr)
        return failf(SPANGPU_ERR_NO_MEMORY, "calloc");
    b->kind = kind;
    if (params)
        memcpy(&b->tp, params, (params_size < sizeof(b->tp))  ?  params_size  :  sizeof(b->tp));

    switch (kind)
    {
    case SPANGPU_DTMF:
    {
        // dtmf.c:104-119
        static const float freqs[8] = {697.0f, 770.0f, 852.0f, 941.0f, 1209.0f, 1336.0f, 1477.0f, 1633.0f};
        b->nb = 8;
        b->nsf = 21;     // v2[8] v3[8] energy z350[2] z440[2] (filter words unused when the notch is off)
        b->block_len = 102;
        for (int i = 0;  i < 8;  i++)
            b->fac[i] = spangpu_goertzel_fac(freqs[i]);
        dtmf_levels(b->tp, b->threshold, b->normal_twist, b->reverse_twist);
        break;
    }
    case SPANGPU_BELL_MF:
    {
        static const int freqs[6] = {700, 900, 1100, 1300, 1500, 1700};         // bell_r2_mf.c:251-254
        b->nb = 6;
        b->nsf = 12;
        b->block_len = 120;
        for (int i = 0;  i < 6;  i++)
            b->fac[i] = spangpu_goertzel_fac((float) freqs[i]);
        break;
    }
    case SPANGPU_R2_MF:
    {
        static const int fwd[6] = {1380, 1500, 1620, 1740, 1860, 1980};         // bell_r2_mf.c:264-267
        static const int back[6] = {1140, 1020, 900, 780, 660, 540};            // bell_r2_mf.c:269-272
        b->nb = 6;
        b->nsf = 12;
        b->block_len = 133;
        for (int i = 0;  i < 6;  i++)
            b->fac[i] = spangpu_goertzel_fac((float) ((b->tp.r2_fwd)  ?  fwd[i]  :  back[i]));
        break;
    }
    case SPANGPU_SUPER_TONE:
    case SPANGPU_GOERTZEL:
    {
        const int m = b->tp.n_bins;
        if (m < ((kind == SPANGPU_SUPER_TONE)  ?  2  :  1)  ||  m > SPANGPU_MAX_BINS)
        {
            free(b);
            return failf(SPANGPU_ERR_BAD_ARG, "n_bins %d out of range", m);
        }
        b->nb = (m <= 4)  ?  4  :  (m <= 8)  ?  8  :  (m <= 12)  ?  12  :  (m <= 16)  ?  16  :  (m <= 24)  ?  24  :  (m <= 32)  ?  32  :  64;
        b->nsf = 2*b->nb + 1;
        b->block_len = (kind == SPANGPU_SUPER_TONE)  ?  128  :  b->tp.block_len;
        if (b->block_len <= 0  ||  b->block_len > 65535)
        {
            free(b);
            return failf(SPANGPU_ERR_BAD_ARG, "block_len %d out of range", b->block_len);
        }
        if (kind == SPANGPU_GOERTZEL  &&  (b->tp.functor < 0  ||  b->tp.functor > SPANGPU_FUNCTOR_ADEMCO
                                           ||  (b->tp.functor == SPANGPU_FUNCTOR_ADEMCO  &&  m != 2)))
        {
            free(b);
            return failf(SPANGPU_ERR_BAD_ARG, "functor %d does not fit a bank of %d bins", b->tp.functor, m);
        }
        for (int i = 0;  i < m;  i++)
            b->fac[i] = b->tp.bin_fac[i];
        break;
    }
    default:
        free(b);
        return failf(SPANGPU_ERR_UNSUPPORTED, "bank kind %d not available from this entry point", kind);
    }

    const int rc = core_create(&b->c, device, n_channels, 0);       // (no words of the core's: sf and si are the state)
    if (rc != SPANGPU_OK)
    {
        spangpu_bank_destroy(b);
        return rc;
    }
    const size_t nf = (size_t) b->nsf*b->c.n_ch;
    if (hipMalloc(&b->sf, nf*sizeof(float)) != hipSuccess
        ||  hipMalloc(&b->si, (size_t) 2*b->c.n_ch*sizeof(int32_t)) != hipSuccess)
    {
        spangpu_bank_destroy(b);
        return failf(SPANGPU_ERR_NO_MEMORY, "hipMalloc of bank state failed");
    }
    (void) hipMemsetAsync(b->sf, 0, nf*sizeof(float), joined(b));
    (void) hipMemsetAsync(b->si, 0, (size_t) 2*b->c.n_ch*sizeof(int32_t), joined(b));
    (void) hipEventCreate(&b->ev0);
    (void) hipEventCreate(&b->ev1);
    (void) hipStreamSynchronize(joined(b));
    *bank = b;
    return SPANGPU_OK;
}

int spangpu_bank_destroy(spangpu_bank_t *b)
{
    if (b == nullptr)
        return SPANGPU_OK;
    (void) hipSetDevice(b->c.device);
    if (b->c.stream)
        (void) hipStreamSynchronize(joined(b));
    if (b->stream2)
    {
        (void) hipStreamSynchronize(b->stream2);
        (void) hipStreamDestroy(b->stream2);
    }
    if (b->ev_in) (void) hipEventDestroy(b->ev_in);
    if (b->ev_q) (void) hipEventDestroy(b->ev_q);
    free_outputs(b);
    cadence_free(b->cad);
    if (b->sf) (void) hipFree(b->sf);
    if (b->si) (void) hipFree(b->si);
    if (b->d_amp) (void) hipFree(b->d_amp);
    lens_free(&b->lens);
    if (b->chan_parms) (void) hipFree(b->chan_parms);
    free(b->h_chan_parms);
    if (b->ev0) (void) hipEventDestroy(b->ev0);
    if (b->ev1) (void) hipEventDestroy(b->ev1);
    core_destroy(&b->c);
    free(b);
    return SPANGPU_OK;
}

int spangpu_bank_kind(const spangpu_bank_t *b) { return b  ?  b->kind  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_bank_device(const spangpu_bank_t *b) { return b  ?  b->c.device  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_bank_channels(const spangpu_bank_t *b) { return b  ?  b->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_bank_set_stream(spangpu_bank_t *b, void *hip_stream)
{
    if (b == nullptr)
        return failf(SPANGPU_ERR_BAD_ARG, "null bank");
    (void) joined(b);
    return core_set_stream(&b->c, hip_stream, true);        // NULL: back to a stream of the bank's own
}

// Streams of their own for the banks of one tick, on hardware queues that are different ones.  A HIP stream is bound to one
// of a few hardware queues by the runtime, in an order a caller does not control: two of three freshly made streams can land
// on one queue, and the launches of those two banks then run one after the other (configs[2], round 6: Bell MF and super-tone
// on one queue, 30 us a tick instead of 17 -- profiles/r6_mixed_trace_overlap_collision.txt).  Stream priorities do give
// queues of their own, but the lower queues then wait for the higher ones (measured: 42.7 us a tick where three plain streams
// on three queues take 15.3; only the longest bank's stream at high priority: 25 - 26 us against 20).  So: candidates are made, and a pair is PROBED -- a spin kernel of 200 us on each, started
// together: they end together on two queues and one after the other on one -- until every bank has a stream that runs beside
// all the others' (a few milliseconds, once).  Returns the number of banks whose stream was proven to run beside every other
// bank's (n_banks unless the device ran out of queues: then the rest share).
__global__ void queue_probe_kernel(long long ticks)
{
    const long long t0 = wall_clock64();           // the 100 MHz constant clock
    while (wall_clock64() - t0 < ticks)
        __builtin_amdgcn_s_sleep(8);
}

static bool probe_streams_overlap(hipStream_t a, hipStream_t b)
{
    constexpr long long kTicks = 20000;             // 200 us
    for (int attempt = 0;  attempt < 3;  attempt++)
    {
        (void) hipStreamSynchronize(a);
        (void) hipStreamSynchronize(b);
        const auto t0 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(queue_probe_kernel, dim3(1), dim3(64), 0, a, kTicks);
        hipLaunchKernelGGL(queue_probe_kernel, dim3(1), dim3(64), 0, b, kTicks);
        (void) hipStreamSynchronize(a);
        (void) hipStreamSynchronize(b);
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        if (us < 290.0)
            return true;                            // both spun at once
        if (us > 390.0  &&  us < 600.0)
            return false;                           // one behind the other
        // (anything else: the host was held up; look again)
    }
    return false;
}

int spangpu_banks_own_queues(spangpu_bank_t *const *banks, int n_banks)
{
    if (banks == nullptr  ||  n_banks < 1  ||  n_banks > kToneMaxMulti)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments (at most %d banks)", kToneMaxMulti);
    for (int k = 0;  k < n_banks;  k++)
    {
        if (banks[k] == nullptr  ||  banks[k]->c.device != banks[0]->c.device)
            return failf(SPANGPU_ERR_BAD_ARG, "null bank, or banks on different devices");
        for (int j = 0;  j < k;  j++)
        {
            if (banks[j] == banks[k])
                return failf(SPANGPU_ERR_BAD_ARG, "bank %d is listed twice", k);
        }
    }
    SPG_TRY(hipSetDevice(banks[0]->c.device));
    // Every stream is made and probed first, and the banks' work so far waited for; only then do the banks change streams,
    // which cannot fail.  An error before that gives back every stream made here and leaves the banks as they were.
    constexpr int kCandidates = 12;
    hipStream_t made[kCandidates];      // [0, n_chosen): each proven to run beside all before it; behind them the other candidates
    int n_made = 0, n_chosen = 0;
    while (n_chosen < n_banks  &&  n_made < kCandidates  &&  hipStreamCreateWithFlags(&made[n_made], hipStreamNonBlocking) == hipSuccess)
    {
        const hipStream_t st = made[n_made++];
        bool beside_all = true;
        for (int j = 0;  j < n_chosen  &&  beside_all;  j++)
            beside_all = probe_streams_overlap(made[j], st);
        if (beside_all)
        {
            made[n_made - 1] = made[n_chosen];
            made[n_chosen++] = st;
        }
    }
    const int proven = n_chosen;
    // out of queues (or of candidates): the banks left over take candidates as they are, made[proven .. n_banks)
    int rc = (n_made >= n_banks)  ?  SPANGPU_OK  :  failf(SPANGPU_ERR_HIP, "hipStreamCreate failed");
    for (int k = 0;  k < n_banks  &&  rc == SPANGPU_OK;  k++)
    {
        (void) joined(banks[k]);
        rc = core_sync(&banks[k]->c);
    }
    for (int i = (rc == SPANGPU_OK)  ?  n_banks  :  0;  i < n_made;  i++)
        (void) hipStreamDestroy(made[i]);
    if (rc != SPANGPU_OK)
        return rc;
    for (int k = 0;  k < n_banks;  k++)
    {
        spangpu_bank_t *b = banks[k];
        if (b->c.own_stream)
            (void) hipStreamDestroy(b->c.stream);
        b->c.stream = made[k];
        b->c.own_stream = true;
    }
    return proven;
}

// The HIP stream the bank launches on (its own, unless spangpu_bank_set_stream() gave it another).
void *spangpu_bank_get_stream(spangpu_bank_t *b)
{
    return b  ?  (void *) joined(b)  :  nullptr;
}

// Queue mode.  queues = 2: launches the streaming kernel serves are cut in two workgroup ranges, the second on a stream
// (hardware queue) the bank owns; queues = 1: one launch on the bank's stream (the default); queues = 0: the library's
// choice -- two from 131 072 channels (measured, profiles/r5_probe_mq.log: 131 072 channels 18.3 -> 16.5 us a tick, 262 144
// 35.0 -> 29.5, 1 048 576 118 -> 109; 65 536 channels 11.15 -> 11.7: one).  Results are those of one launch, bit for bit.
// Ordering: the second stream starts a tick behind whatever the bank's stream held when the tick was queued, and every
// spangpu_bank_* call that reads results, edits state or waits joins it back first.  A caller that puts work of its own on
// the bank's stream behind a launch -- an event, a collective reading the records buffer -- calls spangpu_bank_join() first.
int spangpu_bank_set_queues(spangpu_bank_t *b, int queues)
{
    if (b == nullptr  ||  queues < 0  ||  queues > 2)
        return failf(SPANGPU_ERR_BAD_ARG, "queues must be 0 (the library's choice), 1 or 2");
    SPG_TRY(hipSetDevice(b->c.device));
    // The library's own choice is two queues only for a bank on its OWN stream: there every frame reaches the bank through this
    // library (the host copy, or a device frame that is complete when the call is made), and the second queue's ordering is the
    // library's business.  On a caller's stream (spangpu_bank_set_stream) frames may be produced by the caller's kernels on
    // that stream between two ticks, which the second queue would not wait for -- half the channels would read a frame still
    // being written.  A caller who asks for two queues explicitly takes the contract of include/spangpu.h (frames complete at
    // the call, or spangpu_bank_join() / _get_stream() behind whatever made them) with it.
    if (queues == 0)
        queues = (b->c.n_ch >= 131072  &&  b->c.own_stream)  ?  2  :  1;
    (void) joined(b);
    if (queues == 2  &&  b->stream2 == nullptr)
    {
        SPG_TRY(hipStreamCreateWithFlags(&b->stream2, hipStreamNonBlocking));
        SPG_TRY(hipEventCreateWithFlags(&b->ev_in, hipEventDisableTiming));
        SPG_TRY(hipEventCreateWithFlags(&b->ev_q, hipEventDisableTiming));
    }
    b->queues = queues;
    return queues;
}

int spangpu_bank_join(spangpu_bank_t *b)
{
    if (b == nullptr)
        return failf(SPANGPU_ERR_BAD_ARG, "null bank");
    (void) joined(b);
    return SPANGPU_OK;
}

int spangpu_bank_set_timing(spangpu_bank_t *b, int on)
{
    if (b == nullptr)
        return failf(SPANGPU_ERR_BAD_ARG, "null bank");
    b->timing = (on != 0);
    return SPANGPU_OK;
}

int spangpu_bank_sync(spangpu_bank_t *b)
{
    if (b == nullptr)
        return failf(SPANGPU_ERR_BAD_ARG, "null bank");
    (void) joined(b);
    return core_sync(&b->c);
}

float spangpu_bank_last_kernel_ms(spangpu_bank_t *b)
{
    float ms = -1.0f;
    if (b == nullptr  ||  !b->ev_valid)
        return -1.0f;
    if (hipEventSynchronize(b->ev1) != hipSuccess)
        return -1.0f;
    if (hipEventElapsedTime(&ms, b->ev0, b->ev1) != hipSuccess)
        return -1.0f;
    return ms;
}

int spangpu_bank_blocks(spangpu_bank_t *b, spangpu_block_t *out, int max)
{
    if (b == nullptr)
        return failf(SPANGPU_ERR_BAD_ARG, "null bank");
    if (b->last_maxb <= 0)
        return 0;
    SPG_TRY(hipSetDevice(b->c.device));
    const size_t n = (size_t) b->last_maxb*b->c.n_ch;
    SPG_TRY(hipMemcpyAsync(b->h_rec, records_of(b), n*sizeof(uint32_t), hipMemcpyDeviceToHost, joined(b)));
    if (b->rec_energy)
        SPG_TRY(hipMemcpyAsync(b->h_energy, b->rec_energy, n*sizeof(float), hipMemcpyDeviceToHost, joined(b)));
    if (b->rec_dur)
        SPG_TRY(hipMemcpyAsync(b->h_dur, b->rec_dur, n*sizeof(int32_t), hipMemcpyDeviceToHost, joined(b)));
    SPG_TRY(hipStreamSynchronize(joined(b)));
    int count = 0;
    const bool bias = (b->kind == SPANGPU_SUPER_TONE);
    for (int ch = 0;  ch < b->c.n_ch;  ch++)
    {
        for (int k = 0;  k < b->last_maxb;  k++)
        {
            const size_t idx = (size_t) k*b->c.n_ch + ch;
            const uint32_t r = b->h_rec[idx];
            const int flags = (int) (r >> 16);
            if (!(flags & SPANGPU_BLK_VALID))
                continue;
            if (out  &&  count < max)
            {
                spangpu_block_t *o = &out[count];
                o->channel = ch;
                o->block = k;
                o->hit = (int) (r & 0xFF) - (bias  ?  1  :  0);
                o->code = (int) ((r >> 8) & 0xFF) - (bias  ?  1  :  0);
                o->flags = flags;
                o->duration = (b->h_dur  &&  (flags & SPANGPU_BLK_REPORT))  ?  b->h_dur[idx]  :  0;
                o->energy = (b->h_energy)  ?  b->h_energy[idx]  :  0.0f;
            }
            count++;
        }
    }
    return count;
}

// Have the following launches write their block records straight into a caller-owned device buffer (for example the
// send buffer of an RCCL gather: no copy between the kernel and the collective).  The buffer must hold
// ceil(samples/block)*n_channels words for the frames to come (2*n_channels covers 160-sample frames of every
// detector); NULL goes back to the bank's own buffer.  spangpu_bank_blocks() reads whichever was written last.
int spangpu_bank_set_records_buffer(spangpu_bank_t *b, void *dev_ptr, size_t bytes)
{
    if (b == nullptr)
        return failf(SPANGPU_ERR_BAD_ARG, "null bank");
    b->ext_rec = (uint32_t *) dev_ptr;
    b->ext_rec_bytes = dev_ptr  ?  bytes  :  0;
    return SPANGPU_OK;
}

long long spangpu_bank_copy_records(spangpu_bank_t *b, void *dst_device, size_t dst_bytes)
{
    if (b == nullptr  ||  dst_device == nullptr)
        return failf(SPANGPU_ERR_BAD_ARG, "null argument");
    const size_t bytes = (size_t) b->last_maxb*b->c.n_ch*sizeof(uint32_t);
    if (bytes > dst_bytes)
        return failf(SPANGPU_ERR_BAD_ARG, "record buffer too small: need %zu bytes", bytes);
    if (bytes == 0)
        return 0;
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipMemcpyAsync(dst_device, records_of(b), bytes, hipMemcpyDeviceToDevice, joined(b)));
    return (long long) bytes;
}

// The launches from now on also write one byte per block and channel into a caller-owned device buffer (e.g. a slice of
// an RCCL send buffer): digits[block][channel] = the digit the block delivered, 0 = none (DTMF: the debouncer accepted a
// digit; Bell MF / R2 MF: the digit of a report), blocks a channel did not complete in the call = 0.  A quarter of the
// record words' bytes, no extra launch, no atomics.  A launch whose blocks do not fit `bytes` leaves the buffer alone.
// _ring: the buffer is n_slices slices of slice_bytes; successive launches fill successive slices, round and round (a
// reporting interval of n steps is then set up with one call instead of one per step).
int spangpu_bank_set_digits_ring(spangpu_bank_t *b, void *dev_ptr, size_t slice_bytes, int n_slices)
{
    if (b == nullptr  ||  (dev_ptr  &&  n_slices <= 0))
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (dev_ptr  &&  b->kind != SPANGPU_DTMF  &&  b->kind != SPANGPU_BELL_MF  &&  b->kind != SPANGPU_R2_MF)
        return failf(SPANGPU_ERR_UNSUPPORTED, "digit bytes exist for DTMF / Bell MF / R2 MF banks");
    b->ext_digits = (uint8_t *) dev_ptr;
    b->ext_digits_bytes = dev_ptr  ?  slice_bytes  :  0;
    b->ext_digits_slices = dev_ptr  ?  n_slices  :  0;
    b->ext_digits_next = 0;
    return SPANGPU_OK;
}

int spangpu_bank_set_digits_buffer(spangpu_bank_t *b, void *dev_ptr, size_t bytes)
{
    return spangpu_bank_set_digits_ring(b, dev_ptr, bytes, 1);
}

int spangpu_bank_trace(spangpu_bank_t *b, float *energies, size_t max_floats)
{
    if (b == nullptr  ||  energies == nullptr)
        return failf(SPANGPU_ERR_BAD_ARG, "null argument");
    if (b->trace == nullptr)
        return failf(SPANGPU_ERR_STATE, "bank was created without trace");
    const size_t n = (size_t) b->last_maxb*(b->nb + 1)*b->c.n_ch;
    if (n > max_floats)
        return failf(SPANGPU_ERR_BAD_ARG, "trace buffer too small: need %zu floats", n);
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipStreamSynchronize(joined(b)));
    SPG_TRY(hipMemcpy(energies, b->trace, n*sizeof(float), hipMemcpyDeviceToHost));
    return b->last_maxb;
}

int spangpu_bank_bins(const spangpu_bank_t *b)
{
    return b  ?  b->nb  :  SPANGPU_ERR_BAD_ARG;
}

}   // extern "C"
