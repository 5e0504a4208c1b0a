// feed_api.hip -- the pipelined host-buffer paths: of a tone bank (include/spangpu.h: spangpu_feed_*), and further down of the
// echo canceller and modem receiver banks (spangpu_echo_feed_*, spangpu_modem_feed_*).
//
// spangpu_bank_rx(.., SPANGPU_MEM_HOST, ..) is a synchronous convenience: copy the frame in, launch, and the caller then
// asks for records.  A caller that holds its frames in host memory tick after tick -- every caller that is not itself
// on the GPU -- wants the three legs to overlap: while tick t's kernel runs and its digits travel back, tick t + 1's
// frame is already crossing PCIe.  A feed owns, per slot of a small ring: a pinned host buffer the caller's receive
// path writes the frame into (no staging copy by the library), a device frame buffer, a device digit list and its
// pinned host copy.  commit() queues  H2D (copy stream) -> event -> kernel + digit list + D2H (bank stream) -> event;
// collect() waits for the oldest tick's last event and hands out its digits: channel | digit << 20 | block << 28, the
// entries of spangpu_bank_digit_events().  What crosses PCIe per tick is the frame down and four bytes per digit up,
// not the 32-bit record of every block of every channel.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#include "bank_host.hpp"
#include "feed_ring.hpp"

using namespace spg;

// =====================================================================================================================
// The feed core: what the three families' feeds are made of.  The ring (feed_ring.hpp), the stream the input travels down
// on, and per slot the pinned and device input blocks with the event behind the copy down and the event that says the tick
// is done; where the family asks for it an output pair per slot, and with an out-stream the event behind the bank's kernels
// that the way up waits for.  A family's struct embeds FeedCore and keeps what is its own; a commit is
//     slot = ring_next();  feed_send();  the family's launches, its way up and the record of ev_done;  ring_committed()
// so that a commit refused or failed anywhere leaves the ring as it was, and a collect is feed_wait_oldest() and the
// family's look at the slot.
// =====================================================================================================================
namespace {

struct FeedSlot
{
    void *h_in;                 // pinned: the caller writes the tick's input here
    void *d_in;
    void *h_out;                // pinned: the caller reads the tick's output here
    void *d_out;
    hipEvent_t ev_in;           // the copy down is done
    hipEvent_t ev_k;            // the bank's stream is done with the tick (out-stream only)
    hipEvent_t ev_done;         // the tick is done
};

struct FeedCore
{
    int device;
    FeedRing ring;
    size_t in_bytes;            // what travels down per tick
    size_t out_bytes;           // the output pair's size, whole 16 bytes
    hipStream_t in_stream;
    hipStream_t out_stream;
    FeedSlot slot[kFeedMaxDepth];
};

// what the three create calls refuse first (rest_ok: whatever else the family checks in the same breath), and the law
int feed_args_ok(const void *out, const void *bank, int max_samples, int depth, bool rest_ok = true)
{
    if (out == nullptr  ||  bank == nullptr  ||  max_samples <= 0  ||  !rest_ok  ||  !ring_depth_ok(depth))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (1 .. 8 slots)");
    return SPANGPU_OK;
}

int feed_law_ok(int law)
{
    if (law != 0  &&  law != SPANGPU_G711_ALAW  &&  law != SPANGPU_G711_ULAW)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "law must be 0 (16 bit linear), SPANGPU_G711_ALAW or SPANGPU_G711_ULAW");
    return SPANGPU_OK;
}

hipError_t feed_stream(hipStream_t *s, bool prio, int hi)
{
    return prio  ?  hipStreamCreateWithPriority(s, hipStreamNonBlocking, hi)  :  hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

// *c is zeroed.  in_bytes down and out_bytes up per slot (0: no output pair), device blocks with 64 bytes to spare, pinned
// blocks zeroed; an out-stream (and ev_k) for a family that sends its output up on a stream of its own; prio: the copy
// streams at the device's high priority.  After a failure the family still calls feed_destroy().
int feed_create(FeedCore *c, int device, int depth, size_t in_bytes, size_t out_bytes, bool out_stream, bool prio)
{
    c->device = device;
    c->ring.depth = depth;
    c->in_bytes = in_bytes;
    c->out_bytes = (out_bytes + 15)/16*16;
    int lo = 0;
    int hi = 0;
    bool ok = hipSetDevice(device) == hipSuccess;
    if (ok  &&  prio)
        (void) hipDeviceGetStreamPriorityRange(&lo, &hi);
    ok = ok  &&  feed_stream(&c->in_stream, prio, hi) == hipSuccess  &&  (!out_stream  ||  feed_stream(&c->out_stream, prio, hi) == hipSuccess);
    for (int k = 0;  ok  &&  k < depth;  k++)
    {
        FeedSlot *s = &c->slot[k];
        ok = hipHostMalloc(&s->h_in, c->in_bytes) == hipSuccess
             &&  hipMalloc(&s->d_in, c->in_bytes + 64) == hipSuccess
             &&  (c->out_bytes == 0  ||  (hipHostMalloc(&s->h_out, c->out_bytes) == hipSuccess  &&  hipMalloc(&s->d_out, c->out_bytes + 64) == hipSuccess))
             &&  hipEventCreateWithFlags(&s->ev_in, hipEventDisableTiming) == hipSuccess
             &&  (!out_stream  ||  hipEventCreateWithFlags(&s->ev_k, hipEventDisableTiming) == hipSuccess)
             &&  hipEventCreateWithFlags(&s->ev_done, hipEventDisableTiming) == hipSuccess;
        if (ok)
        {
            memset(s->h_in, 0, c->in_bytes);
            if (c->out_bytes)
                memset(s->h_out, 0, c->out_bytes);
        }
    }
    return ok  ?  SPANGPU_OK  :  spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "out of (pinned) memory for the feed");
}

// Nothing is freed under a tick: the way down, then the bank (sync_bank(), the family's), then the way up are waited for.
template <typename SyncBank>
void feed_destroy(FeedCore *c, SyncBank sync_bank)
{
    (void) hipSetDevice(c->device);
    if (c->in_stream) (void) hipStreamSynchronize(c->in_stream);
    sync_bank();
    if (c->out_stream) (void) hipStreamSynchronize(c->out_stream);
    if (c->in_stream) (void) hipStreamDestroy(c->in_stream);
    if (c->out_stream) (void) hipStreamDestroy(c->out_stream);
    for (int k = 0;  k < c->ring.depth;  k++)
    {
        FeedSlot *s = &c->slot[k];
        if (s->h_in) (void) hipHostFree(s->h_in);
        if (s->d_in) (void) hipFree(s->d_in);
        if (s->h_out) (void) hipHostFree(s->h_out);
        if (s->d_out) (void) hipFree(s->d_out);
        if (s->ev_in) (void) hipEventDestroy(s->ev_in);
        if (s->ev_k) (void) hipEventDestroy(s->ev_k);
        if (s->ev_done) (void) hipEventDestroy(s->ev_done);
    }
}

// Send the slot's input down and make the bank's stream wait for it.  *bs = bank_stream(), asked for with the feed's device
// current.  (The slot's device blocks are free: its last tick was collected, i.e. its kernels and copies are done.)
template <typename BankStream>
inline int feed_send(FeedCore *c, int slot, BankStream bank_stream, hipStream_t *bs)
{
    FeedSlot *s = &c->slot[slot];
    SPG_TRY(hipSetDevice(c->device));
    *bs = bank_stream();
    SPG_TRY(hipMemcpyAsync(s->d_in, s->h_in, c->in_bytes, hipMemcpyHostToDevice, c->in_stream));
    SPG_TRY(hipEventRecord(s->ev_in, c->in_stream));
    SPG_TRY(hipStreamWaitEvent(*bs, s->ev_in, 0));
    return SPANGPU_OK;
}

// Wait for the oldest tick: *slot is its slot, now free to be committed again, or -1 when no tick is outstanding.
inline int feed_wait_oldest(FeedCore *c, int *slot)
{
    if ((*slot = ring_oldest(&c->ring)) < 0)
        return SPANGPU_OK;
    SPG_TRY(hipSetDevice(c->device));
    SPG_TRY(hipEventSynchronize(c->slot[*slot].ev_done));
    ring_collected(&c->ring, *slot);
    return SPANGPU_OK;
}

}   // namespace

// ---- tone: input = the frame (slot.h_in / d_in), output pair = the digit list, which travels up on the bank's stream --------
struct spangpu_feed_s
{
    FeedCore core;
    spangpu_bank_t *bank;
    int n_ch;
    int max_samples;
    int law;                    // 0 = 16 bit linear, SPANGPU_G711_ALAW / _ULAW = one byte per sample
    int cap;                    // digit list entries per tick (no tick can make more: blocks per frame x channels)
    int quick;                  // entries that travel back with every tick; a livelier tick has the rest fetched when it is collected
    long long stride;           // samples per row of the staging buffers (rows 16-byte aligned)
};

extern "C" {

int spangpu_feed_destroy(spangpu_feed_t *f)
{
    if (f == nullptr)
        return SPANGPU_OK;
    feed_destroy(&f->core, [f] { (void) spangpu_bank_sync(f->bank); });
    free(f);
    return SPANGPU_OK;
}

int spangpu_feed_create(spangpu_feed_t **out, spangpu_bank_t *bank, int device, int max_samples, int law, int depth)
{
    if (feed_args_ok(out, bank, max_samples, depth) != SPANGPU_OK  ||  feed_law_ok(law) != SPANGPU_OK)
        return SPANGPU_ERR_BAD_ARG;
    *out = nullptr;
    const int n_ch = spangpu_bank_channels(bank);
    if (n_ch <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad bank");
    // the frame buffers and the copy stream live where the kernels read them: on the bank's device, no other
    if (device != spangpu_bank_device(bank))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "the feed's device must be the bank's");
    // spangpu_bank_digit_events() packs the block index in four bits: a tick of more than 16 blocks per channel (the shortest
    // block is 64 samples) could queue its copy and kernel and then fail to report -- refused here instead of half way
    if (max_samples > 16*64)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a feed's ticks hold at most 1024 samples per channel (16 blocks)");
    spangpu_feed_t *f = (spangpu_feed_t *) calloc(1, sizeof(*f));
    if (f == nullptr)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "out of memory");
    f->bank = bank;
    f->n_ch = n_ch;
    f->max_samples = max_samples;
    f->law = law;
    const int bps = law  ?  1  :  2;
    f->stride = ((long long) max_samples*bps + 15)/16*16/bps;
    // a block is at least 64 samples long on every detector kind: blocks per frame (+1 for one in progress)
    f->cap = n_ch*(max_samples/64 + 2);
    f->quick = (n_ch/8 > 4096)  ?  n_ch/8  :  4096;
    if (f->quick > f->cap)
        f->quick = f->cap;
    // a plain copy stream, and no out-stream: the list's quick part follows the kernel on the bank's stream
    const int rc = feed_create(&f->core, device, depth, (size_t) f->stride*bps*n_ch, (size_t) (1 + f->cap)*sizeof(uint32_t), false, false);
    if (rc != SPANGPU_OK)
    {
        spangpu_feed_destroy(f);
        return rc;
    }
    *out = f;
    return SPANGPU_OK;
}

// The layout of a staging buffer: channel c's samples start at c*stride samples (16 bit linear) or bytes (G.711).
long long spangpu_feed_stride(const spangpu_feed_t *f)
{
    return f  ?  f->stride  :  (long long) SPANGPU_ERR_BAD_ARG;
}

// The pinned host buffer of the next tick, for the caller to write the frame into; NULL while every slot holds a tick
// that has not been collected.
void *spangpu_feed_acquire(spangpu_feed_t *f)
{
    if (f == nullptr)
        return nullptr;
    const int slot = ring_next(&f->core.ring);
    return (slot < 0)  ?  nullptr  :  f->core.slot[slot].h_in;
}

// Queue the tick whose frame the caller has written into the acquired buffer.  Returns at once.
int spangpu_feed_commit(spangpu_feed_t *f, int samples)
{
    if (f == nullptr  ||  samples <= 0  ||  samples > f->max_samples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int slot = ring_next(&f->core.ring);
    if (slot < 0)
        return slot;
    FeedSlot *s = &f->core.slot[slot];
    hipStream_t bs;
    int rc = feed_send(&f->core, slot, [f] { return (hipStream_t) spangpu_bank_get_stream(f->bank); }, &bs);
    if (rc < 0)
        return rc;
    if (f->law)
        rc = spangpu_bank_rx_g711(f->bank, (const uint8_t *) s->d_in, SPANGPU_MEM_DEVICE, f->law, samples, f->stride);
    else
        rc = spangpu_bank_rx(f->bank, (const int16_t *) s->d_in, SPANGPU_MEM_DEVICE, SPANGPU_LAYOUT_CHANNEL_MAJOR, samples, f->stride);
    if (rc < 0)
        return rc;
    if ((rc = spangpu_bank_digit_events(f->bank, (uint32_t *) s->d_out, f->cap)) < 0)
        return rc;
    SPG_TRY(hipMemcpyAsync(s->h_out, s->d_out, (size_t) (1 + f->quick)*sizeof(uint32_t), hipMemcpyDeviceToHost, bs));
    SPG_TRY(hipEventRecord(s->ev_done, bs));
    ring_committed(&f->core.ring, slot);
    return SPANGPU_OK;
}

// The digits of the oldest tick not yet collected (waits for it): *entries points at `return value` words
// channel | digit << 20 | block << 28, good until the slot is committed again.  Returns 0 with *entries = NULL when no
// tick is outstanding.
int spangpu_feed_collect(spangpu_feed_t *f, const uint32_t **entries)
{
    if (f == nullptr  ||  entries == nullptr)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    *entries = nullptr;
    int slot;
    const int rc = feed_wait_oldest(&f->core, &slot);
    if (rc < 0  ||  slot < 0)
        return rc;
    uint32_t *h_list = (uint32_t *) f->core.slot[slot].h_out;
    const uint32_t n = h_list[0];
    if (n > (uint32_t) f->cap)
        return spangpu_set_error(SPANGPU_ERR_STATE, "digit list overflow");
    if (n > (uint32_t) f->quick)
    {
        // more digits than travel with every tick (an eighth of the channels delivering one in the same 20 ms): the rest now
        SPG_TRY(hipMemcpy(h_list + 1 + f->quick, (const uint32_t *) f->core.slot[slot].d_out + 1 + f->quick,
                          (size_t) (n - (uint32_t) f->quick)*sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    *entries = h_list + 1;
    return (int) n;
}

int spangpu_feed_outstanding(const spangpu_feed_t *f)
{
    return f  ?  ring_outstanding(&f->core.ring)  :  SPANGPU_ERR_BAD_ARG;
}

// A caller's tick loop in C, for measurements (bench.py's `e2e`): ring_run() over the frames the slots hold (the caller's
// receive path is not part of this path), with `lag` ticks between a commit and the collect of its digits (1 .. depth - 1).
// *elapsed_ms = wall time of the whole loop, *digits = the entries collected.
int spangpu_feed_run(spangpu_feed_t *f, int samples, int ticks, int lag, double *elapsed_ms, long long *digits)
{
    long long seen = 0;
    const uint32_t *entries;
    const int rc = ring_run(f  ?  &f->core.ring  :  nullptr, ticks, lag, elapsed_ms,
                            [=] { return spangpu_feed_commit(f, samples); },
                            [&]
                            {
                                const int n = spangpu_feed_collect(f, &entries);
                                seen += (n > 0)  ?  n  :  0;
                                return n;
                            });
    if (rc == SPANGPU_OK  &&  digits)
        *digits = seen;
    return rc;
}

}   // extern "C"

// =====================================================================================================================
// The pipelined host path of the echo canceller and modem receiver banks (round 4; include/spangpu.h: spangpu_echo_feed_*,
// spangpu_modem_feed_*).
//
// echo_can_update() hands the cleaned sample back to its caller (src/echo.c:421-661) and v29_rx() delivers bits through
// put_bit (src/v29rx.c:867-965): for these paths the way back over PCIe is as much the product as the way down.  A slot of
// these feeds therefore has a pinned buffer each way, and a tick's three legs run on three streams --
//     copy-in stream:   H2D of the tick's input                       -> event
//     the bank's stream: (waits) the kernel(s)                         -> event
//     copy-out stream:  (waits) D2H of the tick's output              -> event (the tick is done)
// so that tick t + 1's input crosses PCIe downwards while tick t's kernel runs and tick t - 1's output crosses it upwards:
// the link is full duplex, and a tick costs max(H2D, D2H, kernel), not their sum.
//
// Echo: input = tx rows then rx rows ([2][n_ch][stride] int16, or G.711 bytes decoded on the device), output = the clean
// rows ([n_ch][stride] int16, or G.711 bytes encoded on the device: linear_to_alaw / linear_to_ulaw, spandsp/g711.h).
// Modem: input = PCM rows, output = the put_bit stream packed by spangpu_modem_pack_events() (a header word and the data
// bits per channel, one sparse list of status reports per bank): 28 bytes per channel and tick for V.29 9600 instead of
// one byte per put_bit call.
// =====================================================================================================================
extern "C" {
void *spangpu_echo_get_stream(spangpu_echo_t *e);
int spangpu_echo_device(const spangpu_echo_t *e);
void *spangpu_modem_get_stream(spangpu_modem_t *m);
int spangpu_modem_device(const spangpu_modem_t *m);
}

namespace {

// spandsp/g711.h:165-175 (ulaw_to_linear) and :239-252 (alaw_to_linear)
__device__ __forceinline__ int g711_decode(int code, int law)
{
    if (law == SPANGPU_G711_ULAW)
    {
        const int u = ~code & 0xFF;
        const int t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4);
        return (u & 0x80)  ?  (0x84 - t)  :  (t - 0x84);
    }
    const int a = code ^ 0x55;
    int i = (a & 0x0F) << 4;
    const int sg = (a & 0x70) >> 4;
    i = sg  ?  ((i + 0x108) << (sg - 1))  :  (i + 8);
    return (a & 0x80)  ?  i  :  -i;
}

// spandsp/g711.h:128-163 (linear_to_ulaw) and :198-237 (linear_to_alaw); top_bit() = 31 - clz
__device__ __forceinline__ int g711_encode(int linear, int law)
{
    if (law == SPANGPU_G711_ULAW)
    {
        int mask;
        if (linear >= 0)
        {
            linear = 0x84 + linear;             // G711_ULAW_BIAS
            mask = 0xFF;
        }
        else
        {
            linear = 0x84 - linear;
            mask = 0x7F;
        }
        const int seg = (31 - __clz(linear | 0xFF)) - 7;
        if (seg >= 8)
            return 0x7F ^ mask;
        return ((seg << 4) | ((linear >> (seg + 3)) & 0xF)) ^ mask;
    }
    int mask;
    if (linear >= 0)
    {
        mask = 0x55 | 0x80;                     // G711_ALAW_AMI_MASK | 0x80
    }
    else
    {
        mask = 0x55;
        linear = -linear - 1;
    }
    const int seg = (31 - __clz(linear | 0xFF)) - 7;
    if (seg >= 8)
        return 0x7F ^ mask;
    return ((seg << 4) | ((linear >> (seg  ?  (seg + 3)  :  4)) & 0x0F)) ^ mask;
}

// rows of `n` samples: 16 codes per thread-step (one 16-byte load, two 16-byte stores)
__global__ void g711_to_linear_kernel(const uint8_t *src, int16_t *dst, long long total16, int law)
{
    const long long i = (long long) blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= total16)
        return;
    const uint4 c = ((const uint4 *) src)[i];
    const uint32_t w[4] = {c.x, c.y, c.z, c.w};
    uint32_t o[8];
#pragma unroll
    for (int k = 0;  k < 4;  k++)
    {
        const int a = g711_decode(w[k] & 0xFF, law);
        const int b = g711_decode((w[k] >> 8) & 0xFF, law);
        const int cc = g711_decode((w[k] >> 16) & 0xFF, law);
        const int d = g711_decode(w[k] >> 24, law);
        o[2*k] = ((uint32_t) a & 0xFFFFu) | ((uint32_t) b << 16);
        o[2*k + 1] = ((uint32_t) cc & 0xFFFFu) | ((uint32_t) d << 16);
    }
    ((uint4 *) dst)[2*i] = make_uint4(o[0], o[1], o[2], o[3]);
    ((uint4 *) dst)[2*i + 1] = make_uint4(o[4], o[5], o[6], o[7]);
}

__global__ void linear_to_g711_kernel(const int16_t *src, uint8_t *dst, long long total16, int law)
{
    const long long i = (long long) blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= total16)
        return;
    const uint4 a = ((const uint4 *) src)[2*i];
    const uint4 b = ((const uint4 *) src)[2*i + 1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t o[4];
#pragma unroll
    for (int k = 0;  k < 4;  k++)
    {
        const uint32_t c0 = (uint32_t) g711_encode((int) (int16_t) (w[2*k] & 0xFFFF), law) & 0xFF;
        const uint32_t c1 = (uint32_t) g711_encode((int) (int16_t) (w[2*k] >> 16), law) & 0xFF;
        const uint32_t c2 = (uint32_t) g711_encode((int) (int16_t) (w[2*k + 1] & 0xFFFF), law) & 0xFF;
        const uint32_t c3 = (uint32_t) g711_encode((int) (int16_t) (w[2*k + 1] >> 16), law) & 0xFF;
        o[k] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
    }
    ((uint4 *) dst)[i] = make_uint4(o[0], o[1], o[2], o[3]);
}

}   // namespace

// D2H by a kernel: rows read from HBM and stored into the slot's pinned buffer through its device mapping.  The runtime's
// two copy directions share what they share (measured: an H2D and a D2H hipMemcpyAsync on two streams take nearly the sum of
// their times); stores from a kernel run beside the H2D copy engine.
typedef uint32_t feed_u32x4 __attribute__((ext_vector_type(4)));

__global__ void copy_out_kernel(feed_u32x4 *dst, const feed_u32x4 *src, size_t n16)
{
    for (size_t i = (size_t) blockIdx.x*blockDim.x + threadIdx.x;  i < n16;  i += (size_t) gridDim.x*blockDim.x)
        __builtin_nontemporal_store(src[i], &dst[i]);
}

// Both families' handles are this struct (include/spangpu.h), so a feed carries its family, and every entry point refuses
// the other family's feed like a null one.
enum { kEchoFeed = 1, kModemFeed = 2 };

struct spangpu_xfeed_s
{
    FeedCore core;
    int what;                   // kEchoFeed / kModemFeed: which of the two below
    union
    {
        spangpu_echo_t *echo;
        spangpu_modem_t *modem;
    };
    int d2h_kernel;             // the way up by copy_out_kernel instead of hipMemcpyAsync
    void *h_out_dev[kFeedMaxDepth];
    int n_ch;
    int max_samples;
    int law;
    long long stride;           // samples per row (rows 16-byte aligned in either format)
    int wpc;                    // modem: packed words per channel
    int status_cap;             // modem: status list entries
    int use_hpf_tx;
    int16_t *d_pcm_in;          // echo, G.711: the decoded tx and rx rows (one buffer: a tick's kernel has read it before the next decode, both on the bank's stream)
    int16_t *d_pcm_out;         // echo, G.711: the clean rows before encoding
    int samples_of[kFeedMaxDepth];
};

typedef struct spangpu_xfeed_s spangpu_xfeed_t;

static inline bool is_feed_of(const spangpu_xfeed_t *f, int what)
{
    return f != nullptr  &&  f->what == what;
}

static int xfeed_destroy(spangpu_xfeed_t *f)
{
    if (f == nullptr)
        return SPANGPU_OK;
    feed_destroy(&f->core, [f] { (void) ((f->what == kEchoFeed)  ?  spangpu_echo_sync(f->echo)  :  spangpu_modem_sync(f->modem)); });
    if (f->d_pcm_in) (void) hipFree(f->d_pcm_in);
    if (f->d_pcm_out) (void) hipFree(f->d_pcm_out);
    free(f);
    return SPANGPU_OK;
}

static int xfeed_alloc(spangpu_xfeed_t *f, int device, int depth, size_t in_bytes, size_t out_bytes)
{
    // Measured (profiles/r4_feed_ab.log, 131 072 echo lines / 16 384 V.29 receivers per tick): the echo feed's 21 - 42 MB way
    // up is fastest as a DMA copy on a stream of its own priority (u-law 0.82 ms a tick against 1.08; int16 1.66 against 1.73),
    // the modem feed's 0.6 MB as a kernel's stores on a plain stream (0.20 ms against 0.35 - 0.49).
    const char *how = getenv("SPANGPU_FEED_D2H");           // "dma" / "kernel" for A-B runs
    f->d2h_kernel = (how == nullptr)  ?  (f->what == kModemFeed)  :  (strcmp(how, "kernel") == 0);
    // The copy streams get a priority of their own: the runtime deals streams of one priority round over a handful of
    // hardware queues (GPU_MAX_HW_QUEUES, 4 by default), and a copy stream that lands on the bank stream's queue runs in
    // turn with its kernels instead of beside them (measured: the way up of tick t then sits between the kernels of t and t + 1).
    const char *pr = getenv("SPANGPU_FEED_PRIORITY");       // "0": plain streams (A-B runs)
    const bool prio = (pr == nullptr)  ?  (f->what == kEchoFeed)  :  (strcmp(pr, "0") != 0);
    const int rc = feed_create(&f->core, device, depth, in_bytes, out_bytes, true, prio);
    if (rc != SPANGPU_OK)
        return rc;
    for (int k = 0;  f->d2h_kernel  &&  k < depth;  k++)
    {
        if (hipHostGetDevicePointer(&f->h_out_dev[k], f->core.slot[k].h_out, 0) != hipSuccess)
            f->d2h_kernel = 0;
    }
    if (f->what == kEchoFeed  &&  f->law)
    {
        const size_t rows = (size_t) f->stride*f->n_ch*sizeof(int16_t);
        if (hipMalloc((void **) &f->d_pcm_in, 2*rows + 64) != hipSuccess  ||  hipMalloc((void **) &f->d_pcm_out, rows + 64) != hipSuccess)
            return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "out of (pinned) memory for the feed");
    }
    return SPANGPU_OK;
}

// The way up, behind what the family has put on the bank's stream: the out-stream waits for it, takes the slot's output to
// its pinned block -- by DMA or by copy_out_kernel -- and says when the tick is done.  Then the tick counts as queued.
static int xfeed_send_up(spangpu_xfeed_t *f, int slot, hipStream_t bs, int samples)
{
    FeedCore *c = &f->core;
    FeedSlot *s = &c->slot[slot];
    SPG_TRY(hipEventRecord(s->ev_k, bs));
    SPG_TRY(hipStreamWaitEvent(c->out_stream, s->ev_k, 0));
    if (f->d2h_kernel)
    {
        const size_t n16 = (c->out_bytes + 15)/16;
        hipLaunchKernelGGL(copy_out_kernel, dim3(256), dim3(256), 0, c->out_stream, (feed_u32x4 *) f->h_out_dev[slot], (const feed_u32x4 *) s->d_out, n16);
        SPG_TRY(hipGetLastError());
    }
    else
        SPG_TRY(hipMemcpyAsync(s->h_out, s->d_out, c->out_bytes, hipMemcpyDeviceToHost, c->out_stream));
    SPG_TRY(hipEventRecord(s->ev_done, c->out_stream));
    f->samples_of[slot] = samples;
    ring_committed(&c->ring, slot);
    return SPANGPU_OK;
}

extern "C" {

// ---- echo ------------------------------------------------------------------------------------------------------------------
int spangpu_echo_feed_create(spangpu_echo_feed_t **out, spangpu_echo_t *ec, int max_samples, int law, int depth, int use_hpf_tx)
{
    if (feed_args_ok(out, ec, max_samples, depth) != SPANGPU_OK  ||  feed_law_ok(law) != SPANGPU_OK)
        return SPANGPU_ERR_BAD_ARG;
    *out = nullptr;
    spangpu_xfeed_t *f = (spangpu_xfeed_t *) calloc(1, sizeof(*f));
    if (f == nullptr)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "out of memory");
    f->what = kEchoFeed;
    f->echo = ec;
    f->n_ch = spangpu_echo_channels(ec);
    f->max_samples = max_samples;
    f->law = law;
    f->use_hpf_tx = use_hpf_tx;
    const int bps = law  ?  1  :  2;
    f->stride = ((long long) max_samples + 15)/16*16;            // rows of whole 16-sample groups in either format
    const size_t rows_bytes = (size_t) f->stride*bps*f->n_ch;
    const int rc = xfeed_alloc(f, spangpu_echo_device(ec), depth, 2*rows_bytes, rows_bytes);
    if (rc != SPANGPU_OK)
    {
        xfeed_destroy(f);
        return rc;
    }
    *out = f;
    return SPANGPU_OK;
}

int spangpu_echo_feed_destroy(spangpu_echo_feed_t *f) { return xfeed_destroy(f); }

long long spangpu_echo_feed_stride(const spangpu_echo_feed_t *f)
{
    return f  ?  f->stride  :  (long long) SPANGPU_ERR_BAD_ARG;
}

// The pinned buffers of the next tick: *tx and *rx for the caller to write (channel c's samples at c*stride samples -- int16,
// or bytes with a G.711 law); NULL / SPANGPU_ERR_STATE while every slot holds a tick that has not been collected.
int spangpu_echo_feed_acquire(spangpu_echo_feed_t *f, void **tx, void **rx)
{
    if (!is_feed_of(f, kEchoFeed)  ||  tx == nullptr  ||  rx == nullptr)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int slot = ring_next(&f->core.ring);
    if (slot < 0)
        return slot;
    *tx = f->core.slot[slot].h_in;
    *rx = (char *) f->core.slot[slot].h_in + f->core.in_bytes/2;
    return SPANGPU_OK;
}

int spangpu_echo_feed_commit(spangpu_echo_feed_t *f, int samples)
{
    if (!is_feed_of(f, kEchoFeed)  ||  samples <= 0  ||  samples > f->max_samples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int slot = ring_next(&f->core.ring);
    if (slot < 0)
        return slot;
    FeedSlot *s = &f->core.slot[slot];
    hipStream_t bs;
    int rc = feed_send(&f->core, slot, [f] { return (hipStream_t) spangpu_echo_get_stream(f->echo); }, &bs);
    if (rc < 0)
        return rc;
    const size_t rows = (size_t) f->stride*f->n_ch;
    if (f->law)
    {
        const long long n16 = (long long) (2*rows/16);
        hipLaunchKernelGGL(g711_to_linear_kernel, dim3((unsigned) ((n16 + 255)/256)), dim3(256), 0, bs, (const uint8_t *) s->d_in, f->d_pcm_in, n16, f->law);
        SPG_TRY(hipGetLastError());
        rc = spangpu_echo_update(f->echo, f->d_pcm_in, f->d_pcm_in + rows, f->d_pcm_out, SPANGPU_MEM_DEVICE, samples, f->stride, f->use_hpf_tx);
        if (rc < 0)
            return rc;
        const long long m16 = (long long) (rows/16);
        hipLaunchKernelGGL(linear_to_g711_kernel, dim3((unsigned) ((m16 + 255)/256)), dim3(256), 0, bs, (const int16_t *) f->d_pcm_out, (uint8_t *) s->d_out, m16, f->law);
        SPG_TRY(hipGetLastError());
    }
    else
    {
        rc = spangpu_echo_update(f->echo, (const int16_t *) s->d_in, (const int16_t *) s->d_in + rows, (int16_t *) s->d_out,
                                 SPANGPU_MEM_DEVICE, samples, f->stride, f->use_hpf_tx);
        if (rc < 0)
            return rc;
    }
    return xfeed_send_up(f, slot, bs, samples);
}

// The clean rows of the oldest tick not yet collected (waits for it): *clean is good until the slot is committed again.
// Returns the tick's samples per channel, 0 with *clean = NULL when no tick is outstanding.
int spangpu_echo_feed_collect(spangpu_echo_feed_t *f, const void **clean)
{
    if (!is_feed_of(f, kEchoFeed)  ||  clean == nullptr)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    *clean = nullptr;
    int slot;
    const int rc = feed_wait_oldest(&f->core, &slot);
    if (rc < 0  ||  slot < 0)
        return rc;
    *clean = f->core.slot[slot].h_out;
    return f->samples_of[slot];
}

int spangpu_echo_feed_outstanding(const spangpu_echo_feed_t *f)
{
    return f  ?  ring_outstanding(&f->core.ring)  :  SPANGPU_ERR_BAD_ARG;
}

// A caller's tick loop in C, for measurements: ring_run() over what the slots hold, with `lag` ticks between a commit and the
// collect of its clean rows.
int spangpu_echo_feed_run(spangpu_echo_feed_t *f, int samples, int ticks, int lag, double *elapsed_ms)
{
    const void *clean;
    return ring_run(f  ?  &f->core.ring  :  nullptr, ticks, lag, elapsed_ms,
                    [=] { return spangpu_echo_feed_commit(f, samples); },
                    [&] { return spangpu_echo_feed_collect(f, &clean); });
}

// ---- modem receivers ---------------------------------------------------------------------------------------------------------
int spangpu_modem_feed_create(spangpu_modem_feed_t **out, spangpu_modem_t *modem, int max_samples, int max_bit_rate, int depth)
{
    if (feed_args_ok(out, modem, max_samples, depth, max_bit_rate > 0) != SPANGPU_OK)
        return SPANGPU_ERR_BAD_ARG;
    *out = nullptr;
    spangpu_xfeed_t *f = (spangpu_xfeed_t *) calloc(1, sizeof(*f));
    if (f == nullptr)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "out of memory");
    f->what = kModemFeed;
    f->modem = modem;
    f->n_ch = spangpu_modem_channels(modem);
    f->max_samples = max_samples;
    f->stride = ((long long) max_samples + 7)/8*8;
    f->wpc = spangpu_modem_packed_words(max_bit_rate, max_samples);
    // What a tick can produce: a receiver reports at most a carrier drop and a new carrier with its training in progress in
    // 160 samples (SIG_STATUS_CARRIER_DOWN, _CARRIER_UP, _TRAINING_IN_PROGRESS; or _TRAINING_FAILED and _CARRIER_DOWN), and a bank
    // fed in step does so on every channel in the same tick -- two entries a channel, and one more for every further 160 samples
    // of the tick.  (One entry a channel, as this was, lost a tick's reports above 4 096 channels: the raw events of a tick are
    // gone once the next one runs.)
    const long long per_channel = 2 + (max_samples + 159)/160;
    const long long cap = (long long) f->n_ch*per_channel;
    f->status_cap = (int) ((cap > 4096)  ?  ((cap < 0x3FFFFFFF)  ?  cap  :  0x3FFFFFFF)  :  4096);
    const int rc = xfeed_alloc(f, spangpu_modem_device(modem), depth, (size_t) f->stride*sizeof(int16_t)*f->n_ch,
                               ((size_t) f->n_ch*f->wpc + 1 + 2*(size_t) f->status_cap)*sizeof(uint32_t));
    if (rc != SPANGPU_OK)
    {
        xfeed_destroy(f);
        return rc;
    }
    *out = f;
    return SPANGPU_OK;
}

int spangpu_modem_feed_destroy(spangpu_modem_feed_t *f) { return xfeed_destroy(f); }

long long spangpu_modem_feed_stride(const spangpu_modem_feed_t *f)
{
    return f  ?  f->stride  :  (long long) SPANGPU_ERR_BAD_ARG;
}

int spangpu_modem_feed_words_per_channel(const spangpu_modem_feed_t *f)
{
    return f  ?  f->wpc  :  SPANGPU_ERR_BAD_ARG;
}

int spangpu_modem_feed_status_cap(const spangpu_modem_feed_t *f)
{
    return f  ?  f->status_cap  :  SPANGPU_ERR_BAD_ARG;
}

void *spangpu_modem_feed_acquire(spangpu_modem_feed_t *f)
{
    if (!is_feed_of(f, kModemFeed))
        return nullptr;
    const int slot = ring_next(&f->core.ring);
    return (slot < 0)  ?  nullptr  :  f->core.slot[slot].h_in;
}

int spangpu_modem_feed_commit(spangpu_modem_feed_t *f, int samples)
{
    if (!is_feed_of(f, kModemFeed)  ||  samples <= 0  ||  samples > f->max_samples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int slot = ring_next(&f->core.ring);
    if (slot < 0)
        return slot;
    FeedSlot *s = &f->core.slot[slot];
    hipStream_t bs;
    int rc = feed_send(&f->core, slot, [f] { return (hipStream_t) spangpu_modem_get_stream(f->modem); }, &bs);
    if (rc < 0)
        return rc;
    if ((rc = spangpu_modem_rx(f->modem, (const int16_t *) s->d_in, SPANGPU_MEM_DEVICE, samples, f->stride)) < 0)
        return rc;
    uint32_t *packed = (uint32_t *) s->d_out;
    uint32_t *status = packed + (size_t) f->n_ch*f->wpc;
    if ((rc = spangpu_modem_pack_events(f->modem, packed, f->wpc, status, f->status_cap)) < 0)
        return rc;
    return xfeed_send_up(f, slot, bs, samples);
}

// The oldest tick's put_bit stream in packed form (waits for it): *packed = [n_ch][words_per_channel] rows, *status = the
// bank's status list (word 0 = entries), both good until the slot is committed again; spangpu_modem_unpack_events() turns
// them into the calls.  Returns the tick's samples per channel, 0 when no tick is outstanding.
int spangpu_modem_feed_collect(spangpu_modem_feed_t *f, const uint32_t **packed, const uint32_t **status)
{
    if (!is_feed_of(f, kModemFeed)  ||  packed == nullptr  ||  status == nullptr)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    *packed = nullptr;
    *status = nullptr;
    int slot;
    const int rc = feed_wait_oldest(&f->core, &slot);
    if (rc < 0  ||  slot < 0)
        return rc;
    *packed = (const uint32_t *) f->core.slot[slot].h_out;
    *status = *packed + (size_t) f->n_ch*f->wpc;
    return f->samples_of[slot];
}

int spangpu_modem_feed_outstanding(const spangpu_modem_feed_t *f)
{
    return f  ?  ring_outstanding(&f->core.ring)  :  SPANGPU_ERR_BAD_ARG;
}

// The same loop; *bits = the sum of what the header words of every 64th row say (a look at the rows: the data is there).
int spangpu_modem_feed_run(spangpu_modem_feed_t *f, int samples, int ticks, int lag, double *elapsed_ms, long long *bits)
{
    const uint32_t *packed;
    const uint32_t *status;
    long long seen = 0;
    const int rc = ring_run(f  ?  &f->core.ring  :  nullptr, ticks, lag, elapsed_ms,
                            [=] { return spangpu_modem_feed_commit(f, samples); },
                            [&]
                            {
                                const int n = spangpu_modem_feed_collect(f, &packed, &status);
                                for (int c = 0;  n > 0  &&  c < f->n_ch;  c += 64)
                                    seen += packed[(size_t) c*f->wpc] & 0x7FFFu;
                                return n;
                            });
    if (rc == SPANGPU_OK  &&  bits)
        *bits = seen;
    return rc;
}

}   // extern "C"
