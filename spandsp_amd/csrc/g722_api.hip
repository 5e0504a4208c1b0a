// g722_api.hip -- C ABI of the G.722 wideband codec banks (include/spangpu.h, "G.722 codec banks"): batched g722_encode() or
// g722_decode() at the three rates, at 16 kHz or 8 kHz, packed or not, per channel.  Device code: g722_dev.hpp.  No CPU
// implementation of either path exists behind these entry points; restart and the state calls edit one channel's words on
// the host, as the reference's own g722_*_init() edits one object.

#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#include "g722_dev.hpp"
#include "codec_host.hpp"

using namespace spg;

struct spangpu_g722_s
{
    CodecBank k;                // cfg: bits per sample, eight_k, packed
    int direction;              // SPANGPU_G722_ENCODER or SPANGPU_G722_DECODER
    int present[3][2][2];       // channels per configuration: what the capacity functions and the row checks need of cfg
};

static void summarise(spangpu_g722_s *b)
{
    memset(b->present, 0, sizeof(b->present));
    for (int c = 0;  c < b->k.c.n_ch;  c++)
        b->present[b->k.cfg[3*c] - 6][b->k.cfg[3*c + 1]][b->k.cfg[3*c + 2]]++;
}

// the worst channel's output for `items` samples (encode: bytes) or bytes (decode: samples)
static long long capacity(const spangpu_g722_s *b, bool encode, long long items)
{
    long long worst = 0;
    for (int bps = 6;  bps <= 8;  bps++)
    {
        for (int e = 0;  e < 2;  e++)
        {
            for (int p = 0;  p < 2;  p++)
            {
                if (b->present[bps - 6][e][p] == 0)
                    continue;
                const long long v = encode  ?  g722_encode_capacity(bps, p, e, items)  :  g722_decode_capacity(bps, p, e, items);
                worst = (v > worst)  ?  v  :  worst;
            }
        }
    }
    return worst;
}

template <bool ENCODE>
static void launch(const CodecLaunch &L, dim3 grid, hipStream_t stream)
{
    hipLaunchKernelGGL((codec_kernel<G722Codec, ENCODE>), grid, dim3(64), 0, stream, L);
}

static int run(spangpu_g722_s *b, bool encode, const void *in, int in_kind, long long in_stride, const int32_t *lens, int max_len,
               void *out, int out_kind, long long out_stride, int32_t *counts_out)
{
    int rc;
    if ((rc = codec_args_ok(b, max_len)) != SPANGPU_OK)
        return rc;
    if (b->direction != (encode  ?  SPANGPU_G722_ENCODER  :  SPANGPU_G722_DECODER))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "an encoder bank does not decode, and a decoder bank does not encode");
    const long long in_need = encode  ?  2*(long long) max_len  :  (long long) max_len;
    const long long out_need = encode  ?  capacity(b, true, max_len)  :  2*capacity(b, false, max_len);
    CodecCall call = {in, in_kind, in_stride, in_need, out, out_kind, out_stride, out_need, lens, max_len, counts_out, 0, false};
    if ((rc = codec_check(&b->k, &call)) != SPANGPU_OK)
        return rc;
    // a 16 kHz encoder takes pairs: the reference reads amp[len] at an odd len
    if (encode)
    {
        for (int c = 0;  c < b->k.c.n_ch;  c++)
        {
            if (!b->k.cfg[3*c + 1]  &&  ((lens  ?  lens[c]  :  max_len) & 1))
                return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "an odd number of samples for a 16 kHz encoder");
        }
    }
    return codec_run(&b->k, &call, encode  ?  launch<true>  :  launch<false>);
}

// create's arguments, for init_channel()
struct InitArgs
{
    const int32_t *rates;
    const int32_t *options;
    int n;
};

static void init_channel(const void *arg, int channel, int32_t *words)
{
    const InitArgs *a = (const InitArgs *) arg;
    (void) g722_init_words(words, a->rates[channel % a->n], a->options[channel % a->n]);
}

// words g722_*_init() and a codec's calls could have left: the configuration, a ring position inside the histories (a lane
// addresses its state with it) and a bit count a call can end with
static int words_ok(const int32_t *w)
{
    return (w[G2_PACKED] == 0  ||  w[G2_PACKED] == 1)  &&  (w[G2_EIGHT_K] == 0  ||  w[G2_EIGHT_K] == 1)  &&  w[G2_BPS] >= 6  &&  w[G2_BPS] <= 8
           &&  !(w[G2_PACKED]  &&  w[G2_BPS] == 8)  &&  w[G2_PTR] >= 0  &&  w[G2_PTR] < 12  &&  w[G2_BITS] >= 0  &&  w[G2_BITS] <= 7;
}

extern "C" {

/*
 * Entry point                          stands for (paths relative to the reference tree)
 *   spangpu_g722_create()              g722_encode_init(NULL, rate, options) x N                 src/g722.c:621-648
 *                                      or g722_decode_init(NULL, rate, options) x N              src/g722.c:413-441
 *   spangpu_g722_encode()              g722_encode(s, g722_data, amp, len) x N                   src/g722.c:457-618
 *   spangpu_g722_decode()              g722_decode(s, amp, g722_data, len) x N                   src/g722.c:261-410
 *                                        (both through block4(), 184-258)
 *   spangpu_g722_restart()             g722_encode_init(s, rate, options) / g722_decode_init(s, rate, options) on one channel
 *   spangpu_g722_destroy()             g722_encode_free(s) / g722_decode_free(s) x N             src/g722.c:450-454, 657-661
 */

void spangpu_g722_destroy(spangpu_g722_t *b)
{
    if (b == NULL)
        return;
    codec_destroy(&b->k);
    free(b);
}

int spangpu_g722_create(spangpu_g722_t **out, int device, int n_channels, int direction, const int32_t *rates, const int32_t *options, int n)
{
    if (out == NULL  ||  n_channels <= 0  ||  rates == NULL  ||  options == NULL  ||  n <= 0
        ||  (direction != SPANGPU_G722_ENCODER  &&  direction != SPANGPU_G722_DECODER))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a direction, at least one rate and one set of options)");
    *out = NULL;
    int32_t one[kG722Words];
    for (int i = 0;  i < n;  i++)
    {
        if (!g722_init_words(one, rates[i], options[i]))
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a rate other than 48000, 56000, 64000, or option bits outside 0x3");
    }
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_g722_s *b = (spangpu_g722_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    const InitArgs args = {rates, options, n};
    if ((rc = codec_create(&b->k, device, n_channels, kG722Words, G2_BPS, G2_EIGHT_K, G2_PACKED, init_channel, &args)) != SPANGPU_OK)
    {
        spangpu_g722_destroy(b);
        return rc;
    }
    b->direction = direction;
    summarise(b);
    *out = b;
    return SPANGPU_OK;
}

int spangpu_g722_channels(const spangpu_g722_t *b) { return b  ?  b->k.c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_g722_state_words(const spangpu_g722_t *b) { return b  ?  kG722Words  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_g722_set_stream(spangpu_g722_t *b, void *stream) { return codec_set_stream(b  ?  &b->k  :  NULL, stream); }
int spangpu_g722_sync(spangpu_g722_t *b) { return codec_sync(b  ?  &b->k  :  NULL); }

int spangpu_g722_encode(spangpu_g722_t *b, const void *amp, int amp_mem_kind, long long amp_stride_bytes, const int32_t *lens, int max_samples,
                        uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, int32_t *bytes_out)
{
    return run(b, true, amp, amp_mem_kind, amp_stride_bytes, lens, max_samples, codes, codes_mem_kind, codes_stride_bytes, bytes_out);
}

int spangpu_g722_decode(spangpu_g722_t *b, const uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, const int32_t *lens, int max_bytes,
                        void *amp, int amp_mem_kind, long long amp_stride_bytes, int32_t *samples_out)
{
    return run(b, false, codes, codes_mem_kind, codes_stride_bytes, lens, max_bytes, amp, amp_mem_kind, amp_stride_bytes, samples_out);
}

long long spangpu_g722_encode_capacity(const spangpu_g722_t *b, int samples)
{
    if (b == NULL  ||  samples < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return capacity(b, true, samples);
}

long long spangpu_g722_decode_capacity(const spangpu_g722_t *b, int bytes)
{
    if (b == NULL  ||  bytes < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return capacity(b, false, bytes);
}

const int32_t *spangpu_g722_counts_dev(const spangpu_g722_t *b)
{
    return b  ?  b->k.count.dev  :  NULL;
}

static int put_words(spangpu_g722_s *b, int channel, int32_t *w)
{
    const int rc = codec_put_words(&b->k, channel, w);
    if (rc == SPANGPU_OK)
        summarise(b);
    return rc;
}

int spangpu_g722_restart(spangpu_g722_t *b, int channel, int rate, int options)
{
    int32_t w[kG722Words];
    if (b == NULL  ||  !channel_ok(&b->k.c, channel)  ||  !g722_init_words(w, rate, options))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return put_words(b, channel, w);
}

int spangpu_g722_get_state(spangpu_g722_t *b, int channel, int32_t *words)
{
    return codec_get_state(b  ?  &b->k  :  NULL, channel, words);
}

// The channel takes the configuration words too (a stream moves with its rate, sample rate and packing, its histories and
// the bits that wait); words no codec could have left are refused.
int spangpu_g722_set_state(spangpu_g722_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->k.c, channel)  ||  !words_ok(words))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return put_words(b, channel, const_cast<int32_t *>(words));
}

}   // extern "C"
