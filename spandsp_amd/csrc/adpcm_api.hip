// adpcm_api.hip -- C ABI of the IMA and OKI ADPCM codec banks (include/spangpu.h, "IMA ADPCM codec banks" and "OKI ADPCM codec
// banks"): batched ima_adpcm_encode() / ima_adpcm_decode() in the three variants and oki_adpcm_encode() / oki_adpcm_decode()
// at the two rates, per channel.  Device code: adpcm_dev.hpp.  No CPU implementation of either path exists behind these
// entry points; restart and the state calls edit one channel's words on the host, as the reference's init calls edit one
// object.

#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "../../include/spangpu.h"
#include "adpcm_dev.hpp"
#include "codec_host.hpp"

using namespace spg;

// What the capacity functions need of the channels: how many there are of each kind.  IMA: kind = 2*variant + (chunk_size
// == 0); OKI: kind = (bit_rate == 24000).  (CodecBank's own mirror keeps a byte of a word, too little for a chunk size.)
struct AdpcmKinds
{
    uint8_t *of;                // [n_ch]
    int count[6];
};

struct spangpu_ima_adpcm_s
{
    CodecBank k;
    AdpcmKinds kinds;
};

struct spangpu_oki_adpcm_s
{
    CodecBank k;
    AdpcmKinds kinds;
};

static int ima_kind(const int32_t *w)
{
    return 2*w[IM_VARIANT] + ((w[IM_CHUNK] == 0)  ?  1  :  0);
}

static int oki_kind(const int32_t *w)
{
    return (w[OK_RATE] == 24000)  ?  1  :  0;
}

static void kinds_set(AdpcmKinds *t, int channel, int kind, bool fresh)
{
    if (!fresh)
        t->count[t->of[channel]]--;
    t->of[channel] = (uint8_t) kind;
    t->count[kind]++;
}

// the worst channel's capacity: the largest over the kinds the bank holds
static long long ima_capacity(const spangpu_ima_adpcm_s *b, bool encode, long long len)
{
    long long most = 0;
    for (int kind = 0;  kind < 6;  kind++)
    {
        if (b->kinds.count[kind] == 0)
            continue;
        const long long c = encode  ?  ima_encode_capacity(kind >> 1, kind & 1, len)  :  ima_decode_capacity(kind >> 1, kind & 1, len);
        most = (c > most)  ?  c  :  most;
    }
    return most;
}

static long long oki_capacity(const spangpu_oki_adpcm_s *b, bool encode, long long len)
{
    long long most = 0;
    for (int kind = 0;  kind < 2;  kind++)
    {
        if (b->kinds.count[kind] == 0)
            continue;
        const int rate = kind  ?  24000  :  32000;
        const long long c = encode  ?  oki_encode_capacity(rate, len)  :  oki_decode_capacity(rate, len);
        most = (c > most)  ?  c  :  most;
    }
    return most;
}

template <bool ENCODE>
static void ima_launch(const CodecLaunch &L, dim3 grid, hipStream_t stream)
{
    hipLaunchKernelGGL((ima_adpcm_kernel<ENCODE>), grid, dim3(64), 0, stream, L);
}

template <bool ENCODE>
static void oki_launch(const CodecLaunch &L, dim3 grid, hipStream_t stream)
{
    hipLaunchKernelGGL((oki_adpcm_kernel<ENCODE>), grid, dim3(64), 0, stream, L);
}

// one encode or decode call of either family.  cap: what the bank's worst channel makes of max_len; PCM rows are int16_t.
static int run(CodecBank *k, bool encode, long long cap, const void *in, int in_kind, long long in_stride, const int32_t *lens, int max_len,
               void *out, int out_kind, long long out_stride, int32_t *counts_out, CodecLaunchFn launch)
{
    int rc;
    if ((rc = codec_args_ok(k, max_len)) != SPANGPU_OK)
        return rc;
    cap = (cap > 0)  ?  cap  :  1;
    const long long in_need = encode  ?  2*(long long) max_len  :  (long long) max_len;
    const long long out_need = encode  ?  cap  :  2*cap;
    CodecCall call = {in, in_kind, in_stride, in_need, out, out_kind, out_stride, out_need, lens, max_len, counts_out, 0, false};
    if ((rc = codec_check(k, &call)) != SPANGPU_OK)
        return rc;
    return codec_run(k, &call, launch);
}

struct ImaInit
{
    const int32_t *variants;
    const int32_t *chunk_sizes;
    int n;
};

static void ima_init_channel(const void *arg, int channel, int32_t *words)
{
    const ImaInit *a = (const ImaInit *) arg;
    const int i = channel % a->n;
    (void) ima_init_words(words, a->variants[i], a->chunk_sizes[i]);
}

struct OkiInit
{
    const int32_t *bit_rates;
    int n;
};

static void oki_init_channel(const void *arg, int channel, int32_t *words)
{
    const OkiInit *a = (const OkiInit *) arg;
    (void) oki_init_words(words, a->bit_rates[channel % a->n]);
}

extern "C" {

/*
 * Entry point                          stands for (paths relative to the reference tree)
 *   spangpu_ima_adpcm_create()         ima_adpcm_init(NULL, variant, chunk_size) x N             src/ima_adpcm.c:280-295
 *   spangpu_ima_adpcm_encode()         ima_adpcm_encode(s, ima_data, amp, len) x N               src/ima_adpcm.c:426-508
 *   spangpu_ima_adpcm_decode()         ima_adpcm_decode(s, amp, ima_data, ima_bytes) x N         src/ima_adpcm.c:310-424
 *   spangpu_ima_adpcm_restart()        ima_adpcm_init(s, variant, chunk_size) on one channel
 *   spangpu_ima_adpcm_destroy()        ima_adpcm_free(s) x N                                     src/ima_adpcm.c:303-307
 *   spangpu_oki_adpcm_create()         oki_adpcm_init(NULL, bit_rate) x N                        src/oki_adpcm.c:244-257
 *   spangpu_oki_adpcm_encode()         oki_adpcm_encode(s, oki_data, amp, len) x N               src/oki_adpcm.c:326-384
 *   spangpu_oki_adpcm_decode()         oki_adpcm_decode(s, amp, oki_data, oki_bytes) x N         src/oki_adpcm.c:273-323
 *   spangpu_oki_adpcm_restart()        oki_adpcm_init(s, bit_rate) on one channel
 *   spangpu_oki_adpcm_destroy()        oki_adpcm_free(s) x N                                     src/oki_adpcm.c:266-270
 */

// ---- IMA --------------------------------------------------------------------------------------------------------------

void spangpu_ima_adpcm_destroy(spangpu_ima_adpcm_t *b)
{
    if (b == NULL)
        return;
    codec_destroy(&b->k);
    free(b->kinds.of);
    free(b);
}

int spangpu_ima_adpcm_create(spangpu_ima_adpcm_t **out, int device, int n_channels, const int32_t *variants, const int32_t *chunk_sizes, int n)
{
    if (out == NULL  ||  n_channels <= 0  ||  variants == NULL  ||  chunk_sizes == NULL  ||  n <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (at least one variant and chunk size)");
    *out = NULL;
    int32_t one[kImaWords];
    for (int i = 0;  i < n;  i++)
    {
        if (!ima_init_words(one, variants[i], chunk_sizes[i]))
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a variant other than IMA4, DVI4 and VDVI");
    }
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_ima_adpcm_s *b = (spangpu_ima_adpcm_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    const ImaInit args = {variants, chunk_sizes, n};
    if ((b->kinds.of = (uint8_t *) calloc((size_t) n_channels, 1)) == NULL)
        rc = spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    else
        rc = codec_create(&b->k, device, n_channels, kImaWords, IM_VARIANT, IM_VARIANT, IM_VARIANT, ima_init_channel, &args);
    if (rc != SPANGPU_OK)
    {
        spangpu_ima_adpcm_destroy(b);
        return rc;
    }
    for (int c = 0;  c < n_channels;  c++)
    {
        ima_init_channel(&args, c, one);
        kinds_set(&b->kinds, c, ima_kind(one), true);
    }
    *out = b;
    return SPANGPU_OK;
}

int spangpu_ima_adpcm_channels(const spangpu_ima_adpcm_t *b) { return b  ?  b->k.c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_ima_adpcm_state_words(const spangpu_ima_adpcm_t *b) { return b  ?  kImaWords  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_ima_adpcm_set_stream(spangpu_ima_adpcm_t *b, void *stream) { return codec_set_stream(b  ?  &b->k  :  NULL, stream); }
int spangpu_ima_adpcm_sync(spangpu_ima_adpcm_t *b) { return codec_sync(b  ?  &b->k  :  NULL); }

int spangpu_ima_adpcm_encode(spangpu_ima_adpcm_t *b, const void *amp, int amp_mem_kind, long long amp_stride_bytes, const int32_t *lens,
                             int max_samples, uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, int32_t *bytes_out)
{
    return run(b  ?  &b->k  :  NULL, true, b  ?  ima_capacity(b, true, max_samples)  :  0, amp, amp_mem_kind, amp_stride_bytes, lens, max_samples,
               codes, codes_mem_kind, codes_stride_bytes, bytes_out, ima_launch<true>);
}

int spangpu_ima_adpcm_decode(spangpu_ima_adpcm_t *b, const uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, const int32_t *lens,
                             int max_bytes, void *amp, int amp_mem_kind, long long amp_stride_bytes, int32_t *samples_out)
{
    return run(b  ?  &b->k  :  NULL, false, b  ?  ima_capacity(b, false, max_bytes)  :  0, codes, codes_mem_kind, codes_stride_bytes, lens, max_bytes,
               amp, amp_mem_kind, amp_stride_bytes, samples_out, ima_launch<false>);
}

long long spangpu_ima_adpcm_encode_capacity(const spangpu_ima_adpcm_t *b, int samples)
{
    if (b == NULL  ||  samples < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return ima_capacity(b, true, samples);
}

long long spangpu_ima_adpcm_decode_capacity(const spangpu_ima_adpcm_t *b, int bytes)
{
    if (b == NULL  ||  bytes < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return ima_capacity(b, false, bytes);
}

const int32_t *spangpu_ima_adpcm_counts_dev(const spangpu_ima_adpcm_t *b)
{
    return b  ?  b->k.count.dev  :  NULL;
}

static int ima_put_words(spangpu_ima_adpcm_s *b, int channel, int32_t *w)
{
    const int rc = codec_put_words(&b->k, channel, w);
    if (rc == SPANGPU_OK)
        kinds_set(&b->kinds, channel, ima_kind(w), false);
    return rc;
}

int spangpu_ima_adpcm_restart(spangpu_ima_adpcm_t *b, int channel, int variant, int chunk_size)
{
    int32_t w[kImaWords];
    if (b == NULL  ||  !channel_ok(&b->k.c, channel)  ||  !ima_init_words(w, variant, chunk_size))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return ima_put_words(b, channel, w);
}

int spangpu_ima_adpcm_get_state(spangpu_ima_adpcm_t *b, int channel, int32_t *words)
{
    return codec_get_state(b  ?  &b->k  :  NULL, channel, words);
}

// The channel takes the configuration words too (a stream moves with its variant and chunk size); words no call could have
// left (ima_words_ok(), adpcm_dev.hpp) are refused.
int spangpu_ima_adpcm_set_state(spangpu_ima_adpcm_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->k.c, channel)  ||  !ima_words_ok(words))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return ima_put_words(b, channel, const_cast<int32_t *>(words));
}

// ---- OKI --------------------------------------------------------------------------------------------------------------

void spangpu_oki_adpcm_destroy(spangpu_oki_adpcm_t *b)
{
    if (b == NULL)
        return;
    codec_destroy(&b->k);
    free(b->kinds.of);
    free(b);
}

int spangpu_oki_adpcm_create(spangpu_oki_adpcm_t **out, int device, int n_channels, const int32_t *bit_rates, int n)
{
    if (out == NULL  ||  n_channels <= 0  ||  bit_rates == NULL  ||  n <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (at least one bit rate)");
    *out = NULL;
    int32_t one[kOkiWords];
    for (int i = 0;  i < n;  i++)
    {
        if (!oki_init_words(one, bit_rates[i]))
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a bit rate other than 24000 and 32000");
    }
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_oki_adpcm_s *b = (spangpu_oki_adpcm_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    const OkiInit args = {bit_rates, n};
    if ((b->kinds.of = (uint8_t *) calloc((size_t) n_channels, 1)) == NULL)
        rc = spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    else
        rc = codec_create(&b->k, device, n_channels, kOkiWords, OK_RATE, OK_RATE, OK_RATE, oki_init_channel, &args);
    if (rc != SPANGPU_OK)
    {
        spangpu_oki_adpcm_destroy(b);
        return rc;
    }
    for (int c = 0;  c < n_channels;  c++)
    {
        oki_init_channel(&args, c, one);
        kinds_set(&b->kinds, c, oki_kind(one), true);
    }
    *out = b;
    return SPANGPU_OK;
}

int spangpu_oki_adpcm_channels(const spangpu_oki_adpcm_t *b) { return b  ?  b->k.c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_oki_adpcm_state_words(const spangpu_oki_adpcm_t *b) { return b  ?  kOkiWords  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_oki_adpcm_set_stream(spangpu_oki_adpcm_t *b, void *stream) { return codec_set_stream(b  ?  &b->k  :  NULL, stream); }
int spangpu_oki_adpcm_sync(spangpu_oki_adpcm_t *b) { return codec_sync(b  ?  &b->k  :  NULL); }

int spangpu_oki_adpcm_encode(spangpu_oki_adpcm_t *b, const void *amp, int amp_mem_kind, long long amp_stride_bytes, const int32_t *lens,
                             int max_samples, uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, int32_t *bytes_out)
{
    return run(b  ?  &b->k  :  NULL, true, b  ?  oki_capacity(b, true, max_samples)  :  0, amp, amp_mem_kind, amp_stride_bytes, lens, max_samples,
               codes, codes_mem_kind, codes_stride_bytes, bytes_out, oki_launch<true>);
}

int spangpu_oki_adpcm_decode(spangpu_oki_adpcm_t *b, const uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, const int32_t *lens,
                             int max_bytes, void *amp, int amp_mem_kind, long long amp_stride_bytes, int32_t *samples_out)
{
    return run(b  ?  &b->k  :  NULL, false, b  ?  oki_capacity(b, false, max_bytes)  :  0, codes, codes_mem_kind, codes_stride_bytes, lens, max_bytes,
               amp, amp_mem_kind, amp_stride_bytes, samples_out, oki_launch<false>);
}

long long spangpu_oki_adpcm_encode_capacity(const spangpu_oki_adpcm_t *b, int samples)
{
    if (b == NULL  ||  samples < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return oki_capacity(b, true, samples);
}

long long spangpu_oki_adpcm_decode_capacity(const spangpu_oki_adpcm_t *b, int bytes)
{
    if (b == NULL  ||  bytes < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return oki_capacity(b, false, bytes);
}

const int32_t *spangpu_oki_adpcm_counts_dev(const spangpu_oki_adpcm_t *b)
{
    return b  ?  b->k.count.dev  :  NULL;
}

static int oki_put_words(spangpu_oki_adpcm_s *b, int channel, int32_t *w)
{
    const int rc = codec_put_words(&b->k, channel, w);
    if (rc == SPANGPU_OK)
        kinds_set(&b->kinds, channel, oki_kind(w), false);
    return rc;
}

int spangpu_oki_adpcm_restart(spangpu_oki_adpcm_t *b, int channel, int bit_rate)
{
    int32_t w[kOkiWords];
    if (b == NULL  ||  !channel_ok(&b->k.c, channel)  ||  !oki_init_words(w, bit_rate))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return oki_put_words(b, channel, w);
}

int spangpu_oki_adpcm_get_state(spangpu_oki_adpcm_t *b, int channel, int32_t *words)
{
    return codec_get_state(b  ?  &b->k  :  NULL, channel, words);
}

// The channel takes the rate too; words no call could have left (oki_words_ok(), adpcm_dev.hpp) are refused.
int spangpu_oki_adpcm_set_state(spangpu_oki_adpcm_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->k.c, channel)  ||  !oki_words_ok(words))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return oki_put_words(b, channel, const_cast<int32_t *>(words));
}

}   // extern "C"
