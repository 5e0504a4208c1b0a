// g726_api.hip -- C ABI of the G.726 ADPCM codec banks (include/spangpu.h, "G.726 codec banks"): batched g726_encode() and
// g726_decode() at the four rates, in the three external codings and the three packings, per channel.  Device code:
// g726_dev.hpp.  No CPU implementation of either path exists behind these entry points; restart and the state calls edit
// one channel's words on the host, as the reference's own g726_init() edits one object.

#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "../../include/spangpu.h"
#include "g726_dev.hpp"
#include "codec_host.hpp"

using namespace spg;

struct spangpu_g726_s
{
    CodecBank k;                // cfg: bits per sample, coding, packing
    // what the capacity functions and the row checks need of cfg
    bool any_unpacked;
    bool any_linear;
    int max_bps;                // over the packed channels, 0: none
    int min_bps;
};

static void summarise(spangpu_g726_s *b)
{
    b->any_unpacked = false;
    b->any_linear = false;
    b->max_bps = 0;
    b->min_bps = 0;
    for (int c = 0;  c < b->k.c.n_ch;  c++)
    {
        const int bps = b->k.cfg[3*c];
        b->any_linear |= (b->k.cfg[3*c + 1] == kG726Linear);
        if (b->k.cfg[3*c + 2] == kG726PackNone)
        {
            b->any_unpacked = true;
            continue;
        }
        b->max_bps = (bps > b->max_bps)  ?  bps  :  b->max_bps;
        b->min_bps = (b->min_bps == 0  ||  bps < b->min_bps)  ?  bps  :  b->min_bps;
    }
}

static long long enc_capacity(const spangpu_g726_s *b, long long samples)
{
    const long long packed = b->max_bps  ?  g726_encode_capacity(b->max_bps, kG726PackRight, samples)  :  0;
    return (b->any_unpacked  &&  samples > packed)  ?  samples  :  packed;
}

static long long dec_capacity(const spangpu_g726_s *b, long long bytes)
{
    const long long packed = b->min_bps  ?  g726_decode_capacity(b->min_bps, kG726PackRight, bytes)  :  0;
    return (b->any_unpacked  &&  bytes > packed)  ?  bytes  :  packed;
}

// bytes of a row of `samples` elements in the bank's widest external coding
static long long pcm_bytes(const spangpu_g726_s *b, long long samples)
{
    return b->any_linear  ?  2*samples  :  samples;
}

template <bool ENCODE>
static void launch(const CodecLaunch &L, dim3 grid, hipStream_t stream)
{
    hipLaunchKernelGGL((codec_kernel<G726Codec, ENCODE>), grid, dim3(64), 0, stream, L);
}

static int run(spangpu_g726_s *b, bool encode, const void *in, int in_kind, long long in_stride, const int32_t *lens, int max_len,
               void *out, int out_kind, long long out_stride, int32_t *counts_out)
{
    int rc;
    if ((rc = codec_args_ok(b, max_len)) != SPANGPU_OK)
        return rc;
    const long long in_need = encode  ?  pcm_bytes(b, max_len)  :  (long long) max_len;
    const long long out_need = encode  ?  enc_capacity(b, max_len)  :  pcm_bytes(b, dec_capacity(b, max_len));
    CodecCall call = {in, in_kind, in_stride, in_need, out, out_kind, out_stride, out_need, lens, max_len, counts_out, 0, false};
    if ((rc = codec_check(&b->k, &call)) != SPANGPU_OK)
        return rc;
    return codec_run(&b->k, &call, encode  ?  launch<true>  :  launch<false>);
}

// create's arguments, for init_channel()
struct InitArgs
{
    const int32_t *rates;
    const int32_t *codings;
    const int32_t *packings;
    int n;
};

static void init_channel(const void *arg, int channel, int32_t *words)
{
    const InitArgs *a = (const InitArgs *) arg;
    const int i = channel % a->n;
    (void) g726_init_words(words, a->rates[i], a->codings[i], a->packings[i]);
}

static int config_ok(const int32_t *w)
{
    int32_t ref[kG726Words];
    return g726_init_words(ref, w[G7_RATE], w[G7_CODING], w[G7_PACKING])  &&  w[G7_BPS] == ref[G7_BPS];
}

extern "C" {

/*
 * Entry point                          stands for (paths relative to the reference tree)
 *   spangpu_g726_create()              g726_init(NULL, bit_rate, ext_coding, packing) x N        src/g726.c:1175-1238
 *   spangpu_g726_encode()              g726_encode(s, g726_data, amp, len) x N                   src/g726.c:1109-1172
 *                                        (the encoders: 730-761, 809-840, 888-919, 968-999)
 *   spangpu_g726_decode()              g726_decode(s, amp, g726_data, g726_bytes) x N            src/g726.c:1044-1106
 *                                        (the decoders: 767-803, 846-882, 925-961, 1005-1041; tandem adjustment 624-725)
 *   spangpu_g726_restart()             g726_init(s, bit_rate, ext_coding, packing) on one channel
 *   spangpu_g726_destroy()             g726_free(s) x N                                          src/g726.c:1247-1251
 */

void spangpu_g726_destroy(spangpu_g726_t *b)
{
    if (b == NULL)
        return;
    codec_destroy(&b->k);
    free(b);
}

int spangpu_g726_create(spangpu_g726_t **out, int device, int n_channels, const int32_t *rates, const int32_t *codings,
                        const int32_t *packings, int n)
{
    if (out == NULL  ||  n_channels <= 0  ||  rates == NULL  ||  codings == NULL  ||  packings == NULL  ||  n <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (at least one rate, coding and packing)");
    *out = NULL;
    int32_t one[kG726Words];
    for (int i = 0;  i < n;  i++)
    {
        if (!g726_init_words(one, rates[i], codings[i], packings[i]))
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a rate other than 16000, 24000, 32000, 40000, or a coding or packing out of range");
    }
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_g726_s *b = (spangpu_g726_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    const InitArgs args = {rates, codings, packings, n};
    if ((rc = codec_create(&b->k, device, n_channels, kG726Words, G7_BPS, G7_CODING, G7_PACKING, init_channel, &args)) != SPANGPU_OK)
    {
        spangpu_g726_destroy(b);
        return rc;
    }
    summarise(b);
    *out = b;
    return SPANGPU_OK;
}

int spangpu_g726_channels(const spangpu_g726_t *b) { return b  ?  b->k.c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_g726_state_words(const spangpu_g726_t *b) { return b  ?  kG726Words  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_g726_set_stream(spangpu_g726_t *b, void *stream) { return codec_set_stream(b  ?  &b->k  :  NULL, stream); }
int spangpu_g726_sync(spangpu_g726_t *b) { return codec_sync(b  ?  &b->k  :  NULL); }

int spangpu_g726_encode(spangpu_g726_t *b, const void *amp, int amp_mem_kind, long long amp_stride_bytes, const int32_t *lens, int max_samples,
                        uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, int32_t *bytes_out)
{
    return run(b, true, amp, amp_mem_kind, amp_stride_bytes, lens, max_samples, codes, codes_mem_kind, codes_stride_bytes, bytes_out);
}

int spangpu_g726_decode(spangpu_g726_t *b, const uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, const int32_t *lens, int max_bytes,
                        void *amp, int amp_mem_kind, long long amp_stride_bytes, int32_t *samples_out)
{
    return run(b, false, codes, codes_mem_kind, codes_stride_bytes, lens, max_bytes, amp, amp_mem_kind, amp_stride_bytes, samples_out);
}

long long spangpu_g726_encode_capacity(const spangpu_g726_t *b, int samples)
{
    if (b == NULL  ||  samples < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return enc_capacity(b, samples);
}

long long spangpu_g726_decode_capacity(const spangpu_g726_t *b, int bytes)
{
    if (b == NULL  ||  bytes < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return dec_capacity(b, bytes);
}

const int32_t *spangpu_g726_counts_dev(const spangpu_g726_t *b)
{
    return b  ?  b->k.count.dev  :  NULL;
}

static int put_words(spangpu_g726_s *b, int channel, int32_t *w)
{
    const int rc = codec_put_words(&b->k, channel, w);
    if (rc == SPANGPU_OK)
        summarise(b);
    return rc;
}

int spangpu_g726_restart(spangpu_g726_t *b, int channel, int rate, int coding, int packing)
{
    int32_t w[kG726Words];
    if (b == NULL  ||  !channel_ok(&b->k.c, channel)  ||  !g726_init_words(w, rate, coding, packing))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return put_words(b, channel, w);
}

int spangpu_g726_get_state(spangpu_g726_t *b, int channel, int32_t *words)
{
    return codec_get_state(b  ?  &b->k  :  NULL, channel, words);
}

// The channel takes the configuration words too (a stream moves with its rate, coding and packing); a set of them that
// g726_init() could not have made, or a bit residue outside 0..7, is refused.
int spangpu_g726_set_state(spangpu_g726_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->k.c, channel)  ||  !config_ok(words)  ||  words[G7_RESIDUE] < 0  ||  words[G7_RESIDUE] > 7)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return put_words(b, channel, const_cast<int32_t *>(words));
}

}   // extern "C"
