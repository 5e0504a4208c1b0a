// bank_host.hpp -- the host plumbing the banks share: the HIP-call macro (every C ABI unit), the device check, a bank's stream
// and state words, the staging of a host caller's frames, grow-only device scratch, the quarter sine of dds_int.c and the put
// side of a bit ring.  Plain structs and free functions; a bank struct embeds BankCore (and PcmStage where it stages frames)
// and keeps only what is its own.  Nothing here is exported.
//
// Who uses what.  The sender and side-receiver banks (txgen, modemtx, fsktx, v18, fsk, mct, sigtone, awgn _api.hip) and the
// modem receiver bank (modem_api.hip) embed BankCore and PcmStage; the echo canceller bank (echo_api.hip) embeds BankCore for
// its device, channel count and stream alone (its four-row staging is its own).  The sets of banks over several devices
// (shard_api.hip) sit on shard_core.hpp, which holds banks of these kinds.  The tone bank (tone_bank.hpp; tone_api, tone_rx,
// tone_state, tone_cadence .hip) embeds BankCore for its device, channel count and stream, a VarLens, and stages host frames
// with grow(); its two float / int state arrays, its three frame formats and its two joined streams stay its own (every core
// call that uses c.stream comes behind its joined()).  The primitives take SPG_TRY only.  So do the three pipelined feeds
// (feed_api.hip) of this header: a ring of slots is another shape, and its core is theirs -- feed_ring.hpp (the ring and the tick
// loop of the _run calls, no HIP) and FeedCore in feed_api.hip (streams, per-slot blocks and events, create, destroy, the way down).
// The seven banks with an _rx_var entry point (tone, fsk, mct, sigtone, modem, v18, adsi) keep that call's per-channel lengths
// in a VarLens; the last six and the HDLC receiver and FAX front-end banks (hdlc_api.hip, faxfe_api.hip) hand a call's result
// rows to the host through CountRows, count_row_scan() and rows_fetch().
// The codec banks (g726_api.hip, g722_api.hip) embed codec_host.hpp's CodecBank, and through it BankCore, a VarLens and a
// CountRows; its one encode / decode call uses grow(), lens_check(), lens_upload() and counts_fetch().
//
// The behaviours this sharing makes uniform:
//  - every sender's tx refuses more than kMaxSamples samples a call (tx_args_ok); before, the tone and modem senders did not;
//  - set_stream and sync of the modem receiver and echo canceller banks make the bank's device current first, as the core's
//    always did; before, those two acted on whatever device the calling thread had current;
//  - spangpu_modem_rx() refuses a row stride shorter than the call (rx_args_ok), like the other receivers;
//  - every read-back of result rows hands out pinned host blocks, made in the rx call (grow_pair); before, fsk, mct, sigtone,
//    v18 and adsi grew pageable blocks inside the read-back;
//  - every read-back brings the counts first and then only the columns some channel filled (before, only hdlc and faxfe
//    did; adsi's "only if any count is non-zero" is the case of no column): two waits where small banks had one;
//  - so host entries past a channel's count may hold an earlier call's data.  spangpu.h promises entries below the count only.
//  - the tone bank: spangpu_bank_set_stream() and _sync() make the bank's device current first; a bad length in
//    spangpu_bank_rx_var() is refused with lens_check()'s text (same code, still before anything is queued);
//    spangpu_dtmf_import_state() writes its parameter row through the bank's stream, not with blocking copies;
//    spangpu_banks_own_queues() returns SPANGPU_ERR_BAD_ARG for a bank listed twice, makes at most 12 streams in all and
//    gives up with SPANGPU_ERR_HIP at the first stream that cannot be made; a records buffer too small for a call is refused
//    before a host frame is staged (behind a bad mem kind, as ever), in spangpu_banks_rx() with the other paths' text (no
//    bank index); a bank whose stream cannot be made reports core_create()'s text.
// Everything else a family does differently is a parameter or stays at its call site.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/spangpu.h"

extern "C" int spangpu_set_error(int code, const char *msg);

#define SPG_TRY(expr)                                                                       \
    do                                                                                      \
    {                                                                                       \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
        {                                                                                   \
            char m_[256];                                                                   \
            snprintf(m_, sizeof(m_), "%s failed: %s", #expr, hipGetErrorString(e_));        \
            return spangpu_set_error(SPANGPU_ERR_HIP, m_);                                  \
        }                                                                                   \
    }                                                                                       \
    while (0)

namespace spg __attribute__((visibility("hidden")))
{

constexpr int kMaxSamples = 1 << 24;        // per call: the chunk index of a wave's 16 rows stays inside 32 bits

// spangpu_set_error() with a formatted message (spangpu_api.hip); returns code
int failf(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// hipGetDeviceCount, the range check, hipSetDevice: SPANGPU_ERR_NO_DEVICE where there is no GPU, never a CPU path
int device_ok(int device);

// ---- a bank's stream and its state words st[words][n_ch] -------------------------------------------------------------

struct BankCore
{
    int device;
    int n_ch;
    int words;
    hipStream_t stream;
    bool own_stream;
    int32_t *st;
};

int core_create(BankCore *c, int device, int n_channels, int words);        // the stream and the (unwritten) state
int core_upload(BankCore *c, const int32_t *host);                          // all of st, as the caller prepared it
int core_fill(BankCore *c, const int32_t *one, int lead = -1);             // one[0 .. lead) in every channel, zero after (-1: all)
// Hands the bank to the caller's stream, after the work on the old one.  A NULL stream is stored as it is (the eight sender and
// side-receiver banks: the caller asked for the null stream) unless fresh_if_null, where the bank makes itself a new stream
// of its own (the modem receiver and echo canceller banks: their documented way back from a borrowed stream).
int core_set_stream(BankCore *c, void *stream, bool fresh_if_null = false);
int core_sync(BankCore *c);
void core_destroy(BankCore *c);                                             // syncs first; the stream goes only if the bank made it
// words [first, first + count) of one channel, of st or of another [..][n_ch] array of the bank's
int core_rw_at(BankCore *c, int32_t *base, int ch, int first, int count, int32_t *w, bool write);

static inline int core_rw_words(BankCore *c, int ch, int first, int count, int32_t *w, bool write)
{
    return core_rw_at(c, c->st, ch, first, count, w, write);
}

static inline bool channel_ok(const BankCore *c, int ch)
{
    return ch >= 0  &&  ch < c->n_ch;
}

static inline bool range_ok(const BankCore *c, int first, int n)
{
    return first >= 0  &&  n > 0  &&  first <= c->n_ch - n;
}

// ---- frames of a host caller -----------------------------------------------------------------------------------------

struct PcmStage
{
    int16_t *d_pcm;         // [n_ch][pcm_cap]
    size_t pcm_cap;         // samples per channel, a multiple of 8
    int32_t *d_lens;        // [n_ch]: the lengths a sender returns to a host caller (stage_lens())
};

int stage_lens(BankCore *c, PcmStage *s);

static inline void stage_free(PcmStage *s)
{
    (void) hipFree(s->d_pcm);
    (void) hipFree(s->d_lens);
}

static inline int mem_kind_ok(int mem_kind)
{
    if (mem_kind != SPANGPU_MEM_HOST  &&  mem_kind != SPANGPU_MEM_DEVICE)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad mem kind");
    return SPANGPU_OK;
}

// A sender's arguments: 0 <= samples <= kMaxSamples, stride >= samples.
static inline int tx_args_ok(const void *bank, int mem_kind, const int16_t *pcm, long long stride, int samples)
{
    if (bank == NULL  ||  pcm == NULL  ||  samples < 0  ||  samples > kMaxSamples  ||  stride < samples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return mem_kind_ok(mem_kind);
}

// A receiver's: samples > 0, and stride <= 0 stands for "rows are `samples` long".
static inline int rx_args_ok(const void *bank, int mem_kind, const int16_t *amp, int samples, long long *stride)
{
    if (bank == NULL  ||  amp == NULL  ||  samples <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (mem_kind_ok(mem_kind) != SPANGPU_OK)
        return SPANGPU_ERR_BAD_ARG;
    if (*stride <= 0)
        *stride = samples;
    if (*stride < samples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "stride < samples");
    return SPANGPU_OK;
}

// Senders.  Where the kernel writes: the caller's rows, or the staging copy of them; then the way back.  vec may be NULL.
int stage_out_target(BankCore *c, PcmStage *s, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens,
                     int16_t **k_pcm, long long *k_stride, int32_t **k_lens, int *vec);
int stage_out_back(BankCore *c, PcmStage *s, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens);
// Receivers.  What the kernel reads: a host caller's rows are copied in, and with `sync` the copy is waited for (the buffer
// is only borrowed for the call).
int stage_in(BankCore *c, PcmStage *s, int mem_kind, const int16_t *amp, long long stride, int samples, bool sync,
             const int16_t **k_pcm, long long *k_stride, int *vec);

// ---- grow-only device scratch: need*per elements once need > *cap; the stream is synchronised before the old block goes --

template <typename T, typename C>
static inline int grow(T **ptr, C *cap, C need, size_t per, hipStream_t stream)
{
    if (need <= *cap)
        return SPANGPU_OK;
    SPG_TRY(hipStreamSynchronize(stream));
    (void) hipFree(*ptr);
    *ptr = NULL;
    *cap = 0;
    if (hipMalloc(ptr, (size_t) need*per*sizeof(T)) != hipSuccess)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "device scratch");
    *cap = need;
    return SPANGPU_OK;
}

// the same for a device block and the pinned host block its contents are handed out of: one capacity, both or neither
template <typename T, typename C>
static inline int grow_pair(T **dev, T **pinned, C *cap, C need, size_t per, hipStream_t stream)
{
    if (need <= *cap)
        return SPANGPU_OK;
    const int rc = grow(dev, cap, need, per, stream);
    if (rc != SPANGPU_OK)
        return rc;
    if (*pinned)
        (void) hipHostFree(*pinned);
    *pinned = NULL;
    if (hipHostMalloc(pinned, (size_t) need*per*sizeof(T)) != hipSuccess)
    {
        *cap = 0;
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "pinned scratch");
    }
    return SPANGPU_OK;
}

// ---- the per-channel lengths of an _rx_var call ------------------------------------------------------------------------

struct VarLens
{
    const int32_t *next;    // what the launch being prepared reads (device memory: dev, or a caller's), or NULL
    int32_t *dev;           // [n_ch]
    int32_t *pinned;        // [n_ch]
};

// lens[0 .. n_ch) against 0..max_samples; the longest, and whether all are equal.  No HIP call.
static inline int lens_check(const int32_t *lens, int n_ch, int max_samples, int *longest, bool *all_equal)
{
    int lo = max_samples;
    int hi = 0;
    for (int c = 0;  c < n_ch;  c++)
    {
        if (lens[c] < 0  ||  lens[c] > max_samples)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a channel's length is outside 0..max_samples");
        lo = (lens[c] < lo)  ?  lens[c]  :  lo;
        hi = (lens[c] > hi)  ?  lens[c]  :  hi;
    }
    *longest = hi;
    *all_equal = (lo == hi);
    return SPANGPU_OK;
}

// Both blocks on first use; then the stream is waited for (the last copy out of the pinned block is done), the lengths go
// into the pinned block and their copy to the device is queued.  v->next = v->dev: the caller clears it after its launch.
int lens_upload(BankCore *c, VarLens *v, const int32_t *lens);

static inline void lens_free(VarLens *v)
{
    (void) hipFree(v->dev);
    if (v->pinned)
        (void) hipHostFree(v->pinned);
}

// ---- a call's result rows on their way to the host: counts[rows][n_ch] first, then of each block [n_ch][cap] the columns
// some channel filled (blocks and their pinned twins: grow_pair(), before the launch) ---------------------------------------

struct CountRows
{
    int32_t *dev;           // [rows][n_ch]
    int32_t *pinned;        // the same, and whatever rows more the bank asked for
};

int counts_create(BankCore *c, CountRows *k, int rows, int pinned_rows);
int counts_fetch(BankCore *c, CountRows *k, int rows);        // device current, one copy, one wait

static inline void counts_free(CountRows *k)
{
    (void) hipFree(k->dev);
    if (k->pinned)
        (void) hipHostFree(k->pinned);
}

// one row of counts: the largest (0 at least); false where a count is above cap.  No HIP call.
static inline bool count_row_scan(const int32_t *row, int n_ch, int cap, int *most)
{
    int hi = 0;
    for (int c = 0;  c < n_ch;  c++)
        hi = (row[c] > hi)  ?  row[c]  :  hi;
    *most = hi;
    return hi <= cap;
}

// queues the copy of the first `columns` (at most cap) elements, elem bytes each, of every channel's row of `cap`; none:
// nothing.  The caller waits once behind all its blocks.
int rows_fetch(BankCore *c, void *pinned, const void *dev, size_t elem, int cap, int columns);

// dds_int.c: one quadrant of a sine, 257 entries, in device memory (hipFree() it)
int quarter_sine_upload(int16_t **quarter);

// ---- the put side of a bit ring per channel (spangpu_fsktx_put_bits(), spangpu_modemtx_put_bits()) ----------------------

struct BitPut
{
    uint8_t *d_bits;
    size_t bits_cap;
    int32_t *d_blens;       // [n_ch]
    int32_t *d_acc;         // [n_ch]
};

// rd_row / count_row: the [n_ch] rows of the bank's words that hold each ring's read index and fill
int bitring_put(BankCore *c, BitPut *p, int32_t *rd_row, int32_t *count_row, uint32_t *queue, int qring, int qcap, int first, int n,
                const uint8_t *bits, int stride, const int32_t *lens, int32_t *accepted);

// the same from rows and lengths that are already in device memory, with no copy and no wait: asynchronous on the bank's
// stream.  Nobody checks a length against its row here: lens[i] <= 8*stride is the caller's to keep.  accepted (device
// memory) may be NULL.
int bitring_put_device(BankCore *c, BitPut *p, int32_t *rd_row, int32_t *count_row, uint32_t *queue, int qring, int qcap, int first, int n,
                       const uint8_t *bits, int stride, const int32_t *lens, int32_t *accepted);

static inline void bitput_free(BitPut *p)
{
    (void) hipFree(p->d_bits);
    (void) hipFree(p->d_blens);
    (void) hipFree(p->d_acc);
}

}   // namespace spg
