// codec_host.hpp -- the host side the codec banks share (g726_api.hip, g722_api.hip), on top of bank_host.hpp: a bank's rows
// in and out, its per-channel lengths and counts, the three configuration words the host mirrors, and one encode / decode
// call.  A family's bank embeds CodecBank and keeps its summary of the configurations, its capacity functions and its own
// checks; what differs between the families arrives here as a parameter or stays at the call site.  Nothing here is exported.

#pragma once

#include "bank_host.hpp"
#include "codec_rows.hpp"

namespace spg __attribute__((visibility("hidden")))
{

struct CodecBank
{
    BankCore c;
    uint8_t *d_in;              // a host caller's rows: [n_ch][in_cap] bytes
    size_t in_cap;
    uint8_t *d_out;
    size_t out_cap;
    VarLens lens;               // per-channel lengths of a call
    bool lens_kept;             // lens.dev holds what lens.pinned holds: a caller that brings the same lengths tick after tick
    CountRows count;            // counts of the last call: bytes (encode) or samples (decode)
    uint8_t *cfg;               // [n_ch][3]: the three configuration words of every channel, as the state has them
    int cfg_word[3];            // ... and which state words they are
};

// one channel's first words, c.words of them (the family's init-words call on its create arguments)
typedef void (*CodecInit)(const void *arg, int channel, int32_t *words);

// The stream, the state and the counts; then every channel's words from `init` into the state and into cfg, and counts of
// zero.  After a failure the bank is as codec_destroy() left it.
int codec_create(CodecBank *k, int device, int n_channels, int words, int cfg0, int cfg1, int cfg2, CodecInit init, const void *arg);
void codec_destroy(CodecBank *k);           // (a zeroed bank too)

// one encode or decode call: the rows, what a row must hold (from the family's capacity functions), the lengths
struct CodecCall
{
    const void *in;
    int in_kind;
    long long in_stride;
    long long in_need;          // bytes
    void *out;
    int out_kind;
    long long out_stride;
    long long out_need;
    const int32_t *lens;        // [n_ch], 0 .. max_len each, or NULL: max_len for all
    int max_len;
    int32_t *counts_out;        // host memory [n_ch], or NULL
    // codec_check() adds
    int longest;
    bool all;                   // every channel brings `longest`
};

static inline int codec_args_ok(const void *bank, int max_len)
{
    if (bank == NULL  ||  max_len < 0  ||  max_len > kMaxSamples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return SPANGPU_OK;
}

// both rows and the lengths.  No HIP call: a family's own checks follow, and nothing is queued before them.
int codec_check(const CodecBank *k, CodecCall *call);

typedef void (*CodecLaunchFn)(const CodecLaunch &L, dim3 grid, hipStream_t stream);

// A checked call.  A host caller's rows are copied in and out through the bank's own (pitch: the row rounded up to 16);
// unequal lengths go to the device unless they are the last upload's; a call nobody brings anything to launches nothing
// and zeroes the counts.  With counts_out the call waits once, behind the rows; without, only if a host buffer was lent.
int codec_run(CodecBank *k, const CodecCall *call, CodecLaunchFn launch);

// one channel's words into the state and into cfg (the family summarises again)
int codec_put_words(CodecBank *k, int channel, int32_t *w);

// the bodies of the small entry points: k is NULL where the caller's bank is
int codec_get_state(CodecBank *k, int channel, int32_t *words);
int codec_set_stream(CodecBank *k, void *stream);
int codec_sync(CodecBank *k);

}   // namespace spg
