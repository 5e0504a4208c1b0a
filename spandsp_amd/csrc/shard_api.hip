// shard_api.hip -- one logical bank over several devices, behind the C ABI (include/spangpu.h): tone banks (spangpu_shard_*),
// echo cancellers (spangpu_echo_shard_*) and modem receivers (spangpu_modem_shard_*).  The three sit on one shard core
// (shard_core.hpp: the struct and what needs no GPU; below: create, destroy, sync, post, wait) and keep only what is theirs.
// No kernel lives in this unit.
//
// channels are independent, so a bank of N channels shards as contiguous channel ranges, n/G per device; every
// device owns its channels' state for their lifetime; inputs are delivered per device; nothing is exchanged between compute
// steps.  The one exchange is the gather of the per-channel results of a reporting interval to one device: here the digit
// byte of every block and channel (what bench.py's multi-GPU runs gather through RCCL from Python, spandsp_amd/parallel.py),
// written by each shard's detector kernel itself into a buffer on its own device and brought to the collecting device with
// hipMemcpyPeerAsync behind the kernel, on the shard's own stream -- device-to-device over xGMI where the devices are
// peers, no host in the path.  A C caller needs no torch.distributed for it.
//
// One host thread drives all shards: every call below only queues work (a launch and a copy per shard) and returns; the
// devices run side by side because each shard has a stream of its own on its own device.
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/spangpu.h"
#include "bank_host.hpp"
#include "shard_core.hpp"

using namespace spg;

// How shard i's results reach the collecting device: SPANGPU_LINK_SAME (it is the collecting device), SPANGPU_LINK_PEER (peer
// access is on: hipMemcpyPeerAsync goes device to device over xGMI) or SPANGPU_LINK_STAGED (the devices cannot reach each
// other, or enabling failed: the runtime stages the copy through host memory -- correct, and slow; spangpu_*_shard_info() says so).
static int link_to(int from_device, int to_device)
{
    if (from_device == to_device)
        return SPANGPU_LINK_SAME;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, from_device, to_device) != hipSuccess  ||  !can)
    {
        (void) hipGetLastError();
        return SPANGPU_LINK_STAGED;
    }
    // (the current device is from_device: it is given access to to_device's memory)
    const hipError_t e = hipDeviceEnablePeerAccess(to_device, 0);
    (void) hipGetLastError();
    return (e == hipSuccess  ||  e == hipErrorPeerAccessAlreadyEnabled)  ?  SPANGPU_LINK_PEER  :  SPANGPU_LINK_STAGED;
}

// Debug knob (spangpu_tune_force_peer_copy): a shard on the collecting device itself sends its results with hipMemcpyPeerAsync
// too (source and destination device equal: HIP allows it), so that the multi-device code path runs on a one-GPU box.
static std::atomic<int> g_force_peer{0};

static hipError_t gather_copy(void *dst, int dst_device, const void *src, int src_device, size_t bytes, hipStream_t st)
{
    if (src_device == dst_device  &&  !g_force_peer.load())
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
    return hipMemcpyPeerAsync(dst, dst_device, src, src_device, bytes, st);
}

// ---- the shard core's calls that touch a device ---------------------------------------------------------------------------

template <typename B, int (*Sync)(B *), int (*Destroy)(B *), void *(*GetStream)(B *)>
static const ShardOps kOps = {[](void *b) { return Sync((B *) b); }, [](void *b) { return Destroy((B *) b); },
                              [](void *b) { return GetStream((B *) b); }};

static void shard_destroy(ShardCore *c)
{
    for (int i = 0;  i < c->n;  i++)
    {
        (void) hipSetDevice(c->device[i]);
        if (c->bank[i])
        {
            (void) c->ops->sync(c->bank[i]);
            (void) c->ops->destroy(c->bank[i]);
        }
        if (c->out[i]) (void) hipFree(c->out[i]);
        for (int k = 0;  k < 2;  k++)
        {
            if (c->done[k][i]) (void) hipEventDestroy(c->done[k][i]);
        }
    }
    (void) hipSetDevice(c->collect_device);
    for (int k = 0;  k < 2;  k++)
    {
        if (c->gathered[k]) (void) hipFree(c->gathered[k]);
    }
    if (c->h_gathered) (void) hipHostFree(c->h_gathered);
}

// Deals the channels, then per shard: its device, its bank (make_bank(i, device, channels, &bank): what it made is kept even
// where it fails, for the destroy that follows), its result buffer of out_per_channel bytes a channel, its two events, its
// link; then the two collecting slots, and the pinned copy of one where the family reorders on the host.  A failure leaves
// the core as far as it got: the caller's destroy unwinds it.
template <typename F>
static int shard_create(ShardCore *c, const ShardOps *ops, const int *devices, int n_devices, int n_channels, size_t out_per_channel,
                        bool pinned, const char *gathered_what, F make_bank)
{
    c->ops = ops;
    if (shard_deal(c, devices, n_devices, n_channels) != SPANGPU_OK)
    {
        c->n = 0;
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "channels do not deal out over the shards");
    }
    int rc = SPANGPU_OK;
    for (int i = 0;  i < n_devices  &&  rc == SPANGPU_OK;  i++)
    {
        const int mine = shard_channels(c, i);
        if (hipSetDevice(devices[i]) != hipSuccess)
            rc = spangpu_set_error(SPANGPU_ERR_HIP, "hipSetDevice failed");
        else if ((rc = make_bank(i, devices[i], mine, &c->bank[i])) == SPANGPU_OK)
        {
            if (hipMalloc(&c->out[i], out_per_channel*mine) != hipSuccess
                ||  hipEventCreateWithFlags(&c->done[0][i], hipEventDisableTiming) != hipSuccess
                ||  hipEventCreateWithFlags(&c->done[1][i], hipEventDisableTiming) != hipSuccess)
                rc = spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "out of device memory");
        }
        if (rc == SPANGPU_OK)
            c->link[i] = link_to(devices[i], c->collect_device);
    }
    if (rc == SPANGPU_OK)
    {
        if (hipSetDevice(c->collect_device) != hipSuccess
            ||  hipMalloc(&c->gathered[0], out_per_channel*n_channels) != hipSuccess
            ||  hipMalloc(&c->gathered[1], out_per_channel*n_channels) != hipSuccess
            ||  (pinned  &&  hipHostMalloc(&c->h_gathered, out_per_channel*n_channels) != hipSuccess))
            rc = spangpu_set_error(SPANGPU_ERR_NO_MEMORY, gathered_what);
    }
    return rc;
}

static int shard_sync(ShardCore *c)
{
    if (c == nullptr)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null shard");
    for (int i = 0;  i < c->n;  i++)
    {
        SPG_TRY(hipSetDevice(c->device[i]));
        const int rc = c->ops->sync(c->bank[i]);
        if (rc < 0)
            return rc;
    }
    return SPANGPU_OK;
}

// Behind what shard i's bank has queued on its stream: `bytes` of its result buffer go to byte `offset` of collecting slot
// `slot`, and the slot's event of the shard is recorded.  (The shard's device is current.)
static int shard_post(ShardCore *c, int i, int slot, size_t offset, size_t bytes)
{
    hipStream_t st = (hipStream_t) c->ops->get_stream(c->bank[i]);
    SPG_TRY(gather_copy((uint8_t *) c->gathered[slot] + offset, c->collect_device, c->out[i], c->device[i], bytes, st));
    SPG_TRY(hipEventRecord(c->done[slot][i], st));
    return SPANGPU_OK;
}

static int shard_last_slot(const ShardCore *c)
{
    return (int) ((c->steps - 1u) & 1u);
}

// `hip_stream` (a stream of the collecting device; NULL: the calling host thread) waits until every shard's bytes of the last
// step have arrived.
static int shard_wait(ShardCore *c, void *hip_stream)
{
    const int slot = shard_last_slot(c);
    for (int i = 0;  i < c->n;  i++)
    {
        if (hip_stream)
        {
            SPG_TRY(hipSetDevice(c->collect_device));
            SPG_TRY(hipStreamWaitEvent((hipStream_t) hip_stream, c->done[slot][i], 0));
        }
        else
        {
            SPG_TRY(hipSetDevice(c->device[i]));
            SPG_TRY(hipEventSynchronize(c->done[slot][i]));
        }
    }
    return SPANGPU_OK;
}

// the last step's slot in the pinned host copy
static int shard_fetch(ShardCore *c, size_t bytes)
{
    SPG_TRY(hipSetDevice(c->collect_device));
    SPG_TRY(hipMemcpy(c->h_gathered, c->gathered[shard_last_slot(c)], bytes, hipMemcpyDeviceToHost));
    return SPANGPU_OK;
}

template <typename S>
static ShardCore *core_of(S *s)
{
    return s  ?  (ShardCore *) &s->c  :  nullptr;
}

// ---- tone banks: the digit byte of every block and channel -----------------------------------------------------------------
struct spangpu_shard_s
{
    ShardCore c;                        // out[i] = digits [max_blocks][channels of the shard]; a slot is shard-major, shard i's
                                        // [max_blocks][n_i] at max_blocks*first[i]
    int kind;
    int max_blocks;
    int last_blocks;
};

extern "C" {

int spangpu_shard_destroy(spangpu_shard_t *s)
{
    if (s == nullptr)
        return SPANGPU_OK;
    shard_destroy(&s->c);
    free(s);
    return SPANGPU_OK;
}

// max_samples sizes the digit buffers.  (The dealing of the channels over devices[]: shard_deal(), shard_core.hpp.)
int spangpu_shard_create(spangpu_shard_t **out, const int *devices, int n_devices, int kind, int n_channels, int max_samples,
                         const void *params, size_t params_size)
{
    if (out == nullptr  ||  devices == nullptr  ||  n_devices < 1  ||  n_devices > kMaxShards  ||  n_channels < n_devices  ||  max_samples <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (1 .. 64 shards, at least a channel each)");
    if (kind != SPANGPU_DTMF  &&  kind != SPANGPU_BELL_MF  &&  kind != SPANGPU_R2_MF)
        return spangpu_set_error(SPANGPU_ERR_UNSUPPORTED, "sharded banks: DTMF, Bell MF, R2 MF (the kinds that report digit bytes)");
    *out = nullptr;
    spangpu_shard_t *s = (spangpu_shard_t *) calloc(1, sizeof(*s));
    if (s == nullptr)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "out of memory");
    s->kind = kind;
    // shortest block of the kinds above: DTMF 102 samples
    s->max_blocks = max_samples/102 + 2;
    int rc = shard_create(&s->c, &kOps<spangpu_bank_t, spangpu_bank_sync, spangpu_bank_destroy, spangpu_bank_get_stream>, devices, n_devices,
                          n_channels, (size_t) s->max_blocks, true, "out of memory for the gathered digits",
                          [&](int, int device, int mine, void **bank)
                          { return spangpu_bank_create((spangpu_bank_t **) bank, device, kind, mine, params, params_size); });
    for (int i = 0;  i < s->c.n  &&  rc == SPANGPU_OK;  i++)
        rc = spangpu_bank_set_digits_buffer((spangpu_bank_t *) s->c.bank[i], (uint8_t *) s->c.out[i], (size_t) s->max_blocks*shard_channels(&s->c, i));
    if (rc != SPANGPU_OK)
    {
        spangpu_shard_destroy(s);
        return rc;
    }
    *out = s;
    return SPANGPU_OK;
}

int spangpu_shard_count(const spangpu_shard_t *s) { return s  ?  s->c.n  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_shard_channels(const spangpu_shard_t *s) { return s  ?  s->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }

// Shard i: its device, its first channel and how many it has; its bank (for everything a bank can do: parameters, state,
// records, a stream of the caller's choice ...).
int spangpu_shard_range(const spangpu_shard_t *s, int i, int *device, int *first_channel, int *n_channels)
{
    return shard_range(core_of(s), i, device, first_channel, n_channels);
}

int spangpu_shard_info(const spangpu_shard_t *s, int i, spangpu_shard_info_t *info)
{
    return shard_info(core_of(s), i, g_force_peer.load(), info);
}

int spangpu_tune_force_peer_copy(int on)
{
    return g_force_peer.exchange(on  ?  1  :  0);
}

spangpu_bank_t *spangpu_shard_bank(spangpu_shard_t *s, int i)
{
    return (spangpu_bank_t *) shard_bank(core_of(s), i);
}

// One step of the whole bank: amp[i] = shard i's frame on ITS device (channel-major rows of `stride` samples, its own
// channels only), `samples` samples per channel.  Queues, per shard, the detector launch and the copy of its digit bytes to
// the collecting device behind it; returns without waiting.  Returns the blocks per channel the step can complete.
int spangpu_shard_rx(spangpu_shard_t *s, const int16_t *const *amp, int samples, long long stride)
{
    if (s == nullptr  ||  amp == nullptr  ||  samples <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int block = (s->kind == SPANGPU_DTMF)  ?  102  :  (s->kind == SPANGPU_BELL_MF)  ?  120  :  133;
    const int maxb = (samples + block - 1)/block;
    if (maxb > s->max_blocks)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "more samples than the shard was made for");
    const int slot = (int) (s->c.steps & 1u);
    for (int i = 0;  i < s->c.n;  i++)
    {
        SPG_TRY(hipSetDevice(s->c.device[i]));
        int rc = spangpu_bank_rx((spangpu_bank_t *) s->c.bank[i], amp[i], SPANGPU_MEM_DEVICE, SPANGPU_LAYOUT_CHANNEL_MAJOR, samples, stride);
        if (rc < 0  ||  (rc = shard_post(&s->c, i, slot, (size_t) s->max_blocks*s->c.first[i], (size_t) maxb*shard_channels(&s->c, i))) < 0)
            return rc;
    }
    s->c.steps++;
    s->last_blocks = maxb;
    return maxb;
}

// Makes `hip_stream` (a stream of the collecting device; NULL: the calling host thread) wait until every shard's digit bytes
// of the last spangpu_shard_rx() have arrived, and hands out where they are: on the collecting device (the first shard's),
// shard-major -- shard i's bytes as [blocks][its channels] at offset max_blocks*first_channel(i); 0 = no digit in that block.
int spangpu_shard_digits_device(spangpu_shard_t *s, void *hip_stream, const uint8_t **digits, int *collect_device, int *max_blocks)
{
    if (s == nullptr  ||  digits == nullptr)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (s->c.steps == 0)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no step has been queued yet");
    const int rc = shard_wait(&s->c, hip_stream);
    if (rc < 0)
        return rc;
    *digits = (const uint8_t *) s->c.gathered[shard_last_slot(&s->c)];
    if (collect_device) *collect_device = s->c.collect_device;
    if (max_blocks) *max_blocks = s->max_blocks;
    return s->last_blocks;
}

// The same on the host, in the whole bank's channel order: out[b*n_channels + c] = the digit block b of the last step
// delivered on channel c (0 = none), b < the return value.
int spangpu_shard_digits_host(spangpu_shard_t *s, uint8_t *out, size_t out_bytes)
{
    const uint8_t *dev;
    if (s == nullptr  ||  out == nullptr)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int nb = spangpu_shard_digits_device(s, nullptr, &dev, nullptr, nullptr);
    if (nb < 0)
        return nb;
    if (out_bytes < (size_t) nb*s->c.n_ch)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "destination too small");
    const int rc = shard_fetch(&s->c, (size_t) s->max_blocks*s->c.n_ch);
    if (rc < 0)
        return rc;
    shard_rows_to_channels(&s->c, (const uint8_t *) s->c.h_gathered, s->max_blocks, nb, out);
    return nb;
}

int spangpu_shard_sync(spangpu_shard_t *s)
{
    return shard_sync(core_of(s));
}

}   // extern "C"

// ---- BASELINE configs[4]'s own object: the echo cancellers of N lines over several devices --------------------------------
// Channels in contiguous ranges (multiples of 64), every device owning its lines' taps, history and control words for their
// lifetime; per step one update launch per device on the shard's own stream (tx / rx rows in, clean rows out, each on its
// device); per reporting interval every shard turns its lines' energy sums into ERLE on its own device (echo_erle_kernel)
// and the floats travel to the collecting device (the first shard's) behind that, on the shard's stream: hipMemcpyPeerAsync,
// xGMI where the devices are peers.  Two result slots used in turn, as above.  (Reference: echo.c:421-661 per line; the
// ERLE is tests/echo_tests.c:577-594's level measurement, 10 log10(sum rx^2 / sum clean^2).)
struct spangpu_echo_shard_s
{
    ShardCore c;                        // out[i] = float erle[channels of the shard]; a slot is float [n_ch], the whole bank's
                                        // channel order; steps counts the reports
};

extern "C" {

int spangpu_echo_shard_destroy(spangpu_echo_shard_t *s)
{
    if (s == nullptr)
        return SPANGPU_OK;
    shard_destroy(&s->c);
    free(s);
    return SPANGPU_OK;
}

int spangpu_echo_shard_create(spangpu_echo_shard_t **out, const int *devices, int n_devices, int n_channels, int taps, int adaption_mode)
{
    if (out == nullptr  ||  devices == nullptr  ||  n_devices < 1  ||  n_devices > kMaxShards  ||  n_channels < n_devices)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (1 .. 64 shards, at least a channel each)");
    *out = nullptr;
    spangpu_echo_shard_t *s = (spangpu_echo_shard_t *) calloc(1, sizeof(*s));
    if (s == nullptr)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "out of memory");
    const int rc = shard_create(&s->c, &kOps<spangpu_echo_t, spangpu_echo_sync, spangpu_echo_destroy, spangpu_echo_get_stream>, devices, n_devices,
                                n_channels, sizeof(float), false, "out of memory for the gathered ERLE",
                                [&](int, int device, int mine, void **bank)
                                {
                                    const int r = spangpu_echo_create((spangpu_echo_t **) bank, device, mine, taps, adaption_mode);
                                    // the update kernel itself keeps the energy sums
                                    return (r != SPANGPU_OK)  ?  r  :  spangpu_echo_stats((spangpu_echo_t *) *bank, 2);
                                });
    if (rc != SPANGPU_OK)
    {
        spangpu_echo_shard_destroy(s);
        return rc;
    }
    *out = s;
    return SPANGPU_OK;
}

int spangpu_echo_shard_count(const spangpu_echo_shard_t *s) { return s  ?  s->c.n  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_echo_shard_range(const spangpu_echo_shard_t *s, int i, int *device, int *first_channel, int *n_channels)
{
    return shard_range(core_of(s), i, device, first_channel, n_channels);
}

int spangpu_echo_shard_info(const spangpu_echo_shard_t *s, int i, spangpu_shard_info_t *info)
{
    return shard_info(core_of(s), i, g_force_peer.load(), info);
}

spangpu_echo_t *spangpu_echo_shard_bank(spangpu_echo_shard_t *s, int i)
{
    return (spangpu_echo_t *) shard_bank(core_of(s), i);
}

// One step: tx[i], rx[i], clean[i] = shard i's rows on ITS device (its own lines only), `samples` per line.  Queues one
// update launch per shard and returns.
int spangpu_echo_shard_update(spangpu_echo_shard_t *s, const int16_t *const *tx, const int16_t *const *rx, int16_t *const *clean,
                              int samples, long long stride)
{
    if (s == nullptr  ||  tx == nullptr  ||  rx == nullptr  ||  clean == nullptr  ||  samples <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    for (int i = 0;  i < s->c.n;  i++)
    {
        SPG_TRY(hipSetDevice(s->c.device[i]));
        const int rc = spangpu_echo_update((spangpu_echo_t *) s->c.bank[i], tx[i], rx[i], clean[i], SPANGPU_MEM_DEVICE, samples, stride, 0);
        if (rc < 0)
            return rc;
    }
    return SPANGPU_OK;
}

// A report: every shard's ERLE over the samples since its sums were last cleared, gathered to the collecting device (the
// whole bank's channel order); with `reset` the sums start again behind it.  Queues and returns.
int spangpu_echo_shard_report(spangpu_echo_shard_t *s, int reset)
{
    if (s == nullptr)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null shard");
    const int slot = (int) (s->c.steps & 1u);
    for (int i = 0;  i < s->c.n;  i++)
    {
        spangpu_echo_t *bank = (spangpu_echo_t *) s->c.bank[i];
        SPG_TRY(hipSetDevice(s->c.device[i]));
        int rc = spangpu_echo_erle(bank, (float *) s->c.out[i], SPANGPU_MEM_DEVICE);
        if (rc < 0  ||  (rc = shard_post(&s->c, i, slot, (size_t) s->c.first[i]*sizeof(float), (size_t) shard_channels(&s->c, i)*sizeof(float))) < 0)
            return rc;
        if (reset  &&  (rc = spangpu_echo_stats_reset(bank, SPANGPU_ECHO_STATS_SUMS)) < 0)
            return rc;
    }
    s->c.steps++;
    return SPANGPU_OK;
}

// The last report: `hip_stream` (of the collecting device; NULL: the calling thread) waits for every shard's floats.
int spangpu_echo_shard_erle_device(spangpu_echo_shard_t *s, void *hip_stream, const float **erle_db, int *collect_device)
{
    if (s == nullptr  ||  erle_db == nullptr)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (s->c.steps == 0)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no report has been queued yet");
    const int rc = shard_wait(&s->c, hip_stream);
    if (rc < 0)
        return rc;
    *erle_db = (const float *) s->c.gathered[shard_last_slot(&s->c)];
    if (collect_device) *collect_device = s->c.collect_device;
    return s->c.n_ch;
}

int spangpu_echo_shard_erle_host(spangpu_echo_shard_t *s, float *out, size_t out_floats)
{
    const float *dev;
    if (s == nullptr  ||  out == nullptr  ||  out_floats < (size_t) s->c.n_ch)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int n = spangpu_echo_shard_erle_device(s, nullptr, &dev, nullptr);
    if (n < 0)
        return n;
    SPG_TRY(hipSetDevice(s->c.collect_device));
    SPG_TRY(hipMemcpy(out, dev, (size_t) n*sizeof(float), hipMemcpyDeviceToHost));
    return n;
}

int spangpu_echo_shard_sync(spangpu_echo_shard_t *s)
{
    return shard_sync(core_of(s));
}

}   // extern "C"

// ---- modem receivers over several devices: the put_bit streams of a step gathered to one device ---------------------------
// What travels per shard and step is what spangpu_modem_copy_events() lays out: int32 counts[n_i], then int8 events[n_i][per]
// (24 bytes per channel and 160-sample frame for V.29 at 9600 bit/s); shard i's block sits at byte offset
// (4 + per)*first_channel(i) of the collecting buffer.
struct spangpu_modem_shard_s
{
    ShardCore c;                        // out[i] = the shard's block
    int per;
};

extern "C" {

int spangpu_modem_shard_destroy(spangpu_modem_shard_t *s)
{
    if (s == nullptr)
        return SPANGPU_OK;
    shard_destroy(&s->c);
    free(s);
    return SPANGPU_OK;
}

int spangpu_modem_shard_create(spangpu_modem_shard_t **out, const int *devices, int n_devices, int kind, int n_channels, int bit_rate,
                               int events_per_channel)
{
    if (out == nullptr  ||  devices == nullptr  ||  n_devices < 1  ||  n_devices > kMaxShards  ||  n_channels < n_devices
        ||  events_per_channel < 1  ||  events_per_channel > 4096)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (1 .. 64 shards, at least a channel each, 1 .. 4096 events a channel and step)");
    *out = nullptr;
    spangpu_modem_shard_t *s = (spangpu_modem_shard_t *) calloc(1, sizeof(*s));
    if (s == nullptr)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "out of memory");
    s->per = events_per_channel;
    const int rc = shard_create(&s->c, &kOps<spangpu_modem_t, spangpu_modem_sync, spangpu_modem_destroy, spangpu_modem_get_stream>, devices,
                                n_devices, n_channels, 4u + (size_t) events_per_channel, true, "out of memory for the gathered events",
                                [&](int, int device, int mine, void **bank)
                                { return spangpu_modem_create((spangpu_modem_t **) bank, device, kind, mine, bit_rate); });
    if (rc != SPANGPU_OK)
    {
        spangpu_modem_shard_destroy(s);
        return rc;
    }
    *out = s;
    return SPANGPU_OK;
}

int spangpu_modem_shard_range(const spangpu_modem_shard_t *s, int i, int *device, int *first_channel, int *n_channels)
{
    return shard_range(core_of(s), i, device, first_channel, n_channels);
}

int spangpu_modem_shard_info(const spangpu_modem_shard_t *s, int i, spangpu_shard_info_t *info)
{
    return shard_info(core_of(s), i, g_force_peer.load(), info);
}

spangpu_modem_t *spangpu_modem_shard_bank(spangpu_modem_shard_t *s, int i)
{
    return (spangpu_modem_t *) shard_bank(core_of(s), i);
}

// One step: amp[i] = shard i's rows on its device; queues per shard the receiver launch, the copy of its event block and
// the block's trip to the collecting device, and returns.
int spangpu_modem_shard_rx(spangpu_modem_shard_t *s, const int16_t *const *amp, int samples, long long stride)
{
    if (s == nullptr  ||  amp == nullptr  ||  samples <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int slot = (int) (s->c.steps & 1u);
    const size_t per_ch = 4u + (size_t) s->per;
    for (int i = 0;  i < s->c.n;  i++)
    {
        spangpu_modem_t *bank = (spangpu_modem_t *) s->c.bank[i];
        const size_t bytes = per_ch*shard_channels(&s->c, i);
        SPG_TRY(hipSetDevice(s->c.device[i]));
        int rc = spangpu_modem_rx(bank, amp[i], SPANGPU_MEM_DEVICE, samples, stride);
        if (rc < 0  ||  (rc = spangpu_modem_copy_events(bank, s->c.out[i], bytes, s->per)) < 0
            ||  (rc = shard_post(&s->c, i, slot, per_ch*s->c.first[i], bytes)) < 0)
            return rc;
    }
    s->c.steps++;
    return SPANGPU_OK;
}

// The last step's events on the host, in the whole bank's channel order: counts[c] = put_bit calls of channel c in the step
// (bits and negative SIG_STATUS_* codes), events[c*per + k] = the k-th of them (k < min(counts[c], per)).
int spangpu_modem_shard_events_host(spangpu_modem_shard_t *s, int32_t *counts, int8_t *events)
{
    if (s == nullptr  ||  counts == nullptr  ||  events == nullptr)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (s->c.steps == 0)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no step has been queued yet");
    int rc = shard_wait(&s->c, nullptr);
    if (rc < 0  ||  (rc = shard_fetch(&s->c, (4u + (size_t) s->per)*s->c.n_ch)) < 0)
        return rc;
    shard_blocks_to_channels(&s->c, (const uint8_t *) s->c.h_gathered, 4u, (size_t) s->per, (uint8_t *) counts, (uint8_t *) events);
    return s->c.n_ch;
}

int spangpu_modem_shard_sync(spangpu_modem_shard_t *s)
{
    return shard_sync(core_of(s));
}

}   // extern "C"
