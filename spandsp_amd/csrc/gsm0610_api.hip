// gsm0610_api.hip -- C ABI of the GSM 06.10 full-rate codec banks (include/spangpu.h, "GSM 06.10 codec banks"): batched
// gsm0610_encode() or gsm0610_decode() in the three packings, per channel.  Device code: gsm0610_dev.hpp, two kernels of its
// own (a frame is the item, which the streaming kernel of codec_rows.hpp has no place for) behind the launch struct and the
// host core the other codec banks use.  No CPU implementation of either path exists behind these entry points; restart,
// set_packing and the state calls edit one channel's words on the host, as the reference's own calls edit one object.

#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#include "gsm0610_dev.hpp"
#include "codec_host.hpp"

using namespace spg;

struct spangpu_gsm0610_s
{
    CodecBank k;                // cfg: the packing (the core mirrors three words; all three are the packing here)
    int direction;              // SPANGPU_GSM0610_ENCODER or SPANGPU_GSM0610_DECODER
    int present[3];             // channels per packing: what the capacity functions need of cfg
};

static void summarise(spangpu_gsm0610_s *b)
{
    memset(b->present, 0, sizeof(b->present));
    for (int c = 0;  c < b->k.c.n_ch;  c++)
        b->present[b->k.cfg[3*c]]++;
}

// the worst channel's output for `items` samples (encode: bytes) or bytes (decode: samples)
static long long capacity(const spangpu_gsm0610_s *b, bool encode, int items)
{
    long long worst = 0;
    for (int p = 0;  p < 3;  p++)
    {
        if (b->present[p] == 0)
            continue;
        // (any int from a caller: 64-bit products here; the kernels' lengths are inside kMaxSamples)
        const long long v = encode  ?  (long long) (items/gsm0610_unit_samples(p))*gsm0610_unit_bytes(p)
                                    :  (long long) (items/gsm0610_unit_bytes(p))*gsm0610_unit_samples(p);
        worst = (v > worst)  ?  v  :  worst;
    }
    return worst;
}

static void launch_encode(const CodecLaunch &L, dim3 grid, hipStream_t stream)
{
    hipLaunchKernelGGL(gsm0610_encode_kernel, grid, dim3(64), 0, stream, L);
}

static void launch_decode(const CodecLaunch &L, dim3 grid, hipStream_t stream)
{
    hipLaunchKernelGGL(gsm0610_decode_kernel, grid, dim3(64), 0, stream, L);
}

static int run(spangpu_gsm0610_s *b, bool encode, const void *in, int in_kind, long long in_stride, const int32_t *lens, int max_len,
               void *out, int out_kind, long long out_stride, int32_t *counts_out)
{
    int rc;
    if ((rc = codec_args_ok(b, max_len)) != SPANGPU_OK)
        return rc;
    if (b->direction != (encode  ?  SPANGPU_GSM0610_ENCODER  :  SPANGPU_GSM0610_DECODER))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "an encoder bank does not decode, and a decoder bank does not encode");
    const long long in_need = encode  ?  2*(long long) max_len  :  (long long) max_len;
    const long long out_need = encode  ?  capacity(b, true, max_len)  :  2*capacity(b, false, max_len);
    CodecCall call = {in, in_kind, in_stride, in_need, out, out_kind, out_stride, out_need, lens, max_len, counts_out, 0, false};
    if ((rc = codec_check(&b->k, &call)) != SPANGPU_OK)
        return rc;
    // whole frames only: the reference reads past the end of a partial one
    for (int c = 0;  c < b->k.c.n_ch;  c++)
    {
        const int p = b->k.cfg[3*c];
        const int unit = encode  ?  gsm0610_unit_samples(p)  :  gsm0610_unit_bytes(p);
        if ((lens  ?  lens[c]  :  max_len) % unit != 0)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a length that is not a whole number of the channel's frames (160 samples, 320 under WAV49; 76, 33 or 65 bytes)");
    }
    return codec_run(&b->k, &call, encode  ?  launch_encode  :  launch_decode);
}

// create's arguments, for init_channel()
struct InitArgs
{
    const int32_t *packings;
    int n;
};

static void init_channel(const void *arg, int channel, int32_t *words)
{
    const InitArgs *a = (const InitArgs *) arg;
    (void) gsm0610_init_words(words, a->packings[channel % a->n]);
}

// words gsm0610_init() and a codec's calls could have left: a packing of the three, a set of ratios that exists, and a lag
// inside the history (a lane addresses its working memory with it)
static int words_ok(const int32_t *w)
{
    return gsm0610_packing_ok(w[GW_PACKING])  &&  (w[GW_J] == 0  ||  w[GW_J] == 1)  &&  w[GW_NRP] >= 40  &&  w[GW_NRP] <= 120;
}

extern "C" {

/*
 * Entry point                          stands for (paths relative to the reference tree)
 *   spangpu_gsm0610_create()           gsm0610_init(NULL, packing) x N                           src/gsm0610_encode.c:313-326
 *   spangpu_gsm0610_encode()           gsm0610_encode(s, code, amp, len) x N                     src/gsm0610_encode.c:282-310
 *   spangpu_gsm0610_decode()           gsm0610_decode(s, amp, code, len) x N                     src/gsm0610_decode.c:312-353
 *   spangpu_gsm0610_set_packing()      gsm0610_set_packing(s, packing) on one channel            src/gsm0610_encode.c:108-112
 *   spangpu_gsm0610_restart()          gsm0610_init(s, packing) on one channel
 *   spangpu_gsm0610_destroy()          gsm0610_free(s) x N                                       src/gsm0610_encode.c:335-341
 */

void spangpu_gsm0610_destroy(spangpu_gsm0610_t *b)
{
    if (b == NULL)
        return;
    codec_destroy(&b->k);
    free(b);
}

int spangpu_gsm0610_create(spangpu_gsm0610_t **out, int device, int n_channels, int direction, const int32_t *packings, int n)
{
    if (out == NULL  ||  n_channels <= 0  ||  packings == NULL  ||  n <= 0
        ||  (direction != SPANGPU_GSM0610_ENCODER  &&  direction != SPANGPU_GSM0610_DECODER))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a direction and at least one packing)");
    *out = NULL;
    for (int i = 0;  i < n;  i++)
    {
        if (!gsm0610_packing_ok(packings[i]))
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a packing other than NONE, WAV49, VOIP");
    }
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_gsm0610_s *b = (spangpu_gsm0610_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    const InitArgs args = {packings, n};
    if ((rc = codec_create(&b->k, device, n_channels, kGsmWords, GW_PACKING, GW_PACKING, GW_PACKING, init_channel, &args)) != SPANGPU_OK)
    {
        spangpu_gsm0610_destroy(b);
        return rc;
    }
    b->direction = direction;
    summarise(b);
    *out = b;
    return SPANGPU_OK;
}

int spangpu_gsm0610_channels(const spangpu_gsm0610_t *b) { return b  ?  b->k.c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_gsm0610_state_words(const spangpu_gsm0610_t *b) { return b  ?  kGsmWords  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_gsm0610_set_stream(spangpu_gsm0610_t *b, void *stream) { return codec_set_stream(b  ?  &b->k  :  NULL, stream); }
int spangpu_gsm0610_sync(spangpu_gsm0610_t *b) { return codec_sync(b  ?  &b->k  :  NULL); }

int spangpu_gsm0610_encode(spangpu_gsm0610_t *b, const void *amp, int amp_mem_kind, long long amp_stride_bytes, const int32_t *lens, int max_samples,
                           uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, int32_t *bytes_out)
{
    return run(b, true, amp, amp_mem_kind, amp_stride_bytes, lens, max_samples, codes, codes_mem_kind, codes_stride_bytes, bytes_out);
}

int spangpu_gsm0610_decode(spangpu_gsm0610_t *b, const uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes, const int32_t *lens, int max_bytes,
                           void *amp, int amp_mem_kind, long long amp_stride_bytes, int32_t *samples_out)
{
    return run(b, false, codes, codes_mem_kind, codes_stride_bytes, lens, max_bytes, amp, amp_mem_kind, amp_stride_bytes, samples_out);
}

long long spangpu_gsm0610_encode_capacity(const spangpu_gsm0610_t *b, int samples)
{
    if (b == NULL  ||  samples < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return capacity(b, true, samples);
}

long long spangpu_gsm0610_decode_capacity(const spangpu_gsm0610_t *b, int bytes)
{
    if (b == NULL  ||  bytes < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return capacity(b, false, bytes);
}

const int32_t *spangpu_gsm0610_counts_dev(const spangpu_gsm0610_t *b)
{
    return b  ?  b->k.count.dev  :  NULL;
}

static int put_words(spangpu_gsm0610_s *b, int channel, int32_t *w)
{
    const int rc = codec_put_words(&b->k, channel, w);
    if (rc == SPANGPU_OK)
        summarise(b);
    return rc;
}

// the one word, and the core's mirror of it
int spangpu_gsm0610_set_packing(spangpu_gsm0610_t *b, int channel, int packing)
{
    if (b == NULL  ||  !channel_ok(&b->k.c, channel)  ||  !gsm0610_packing_ok(packing))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w = packing;
    const int rc = core_rw_words(&b->k.c, channel, GW_PACKING, 1, &w, true);
    if (rc == SPANGPU_OK)
    {
        b->k.cfg[3*channel] = b->k.cfg[3*channel + 1] = b->k.cfg[3*channel + 2] = (uint8_t) packing;
        summarise(b);
    }
    return rc;
}

int spangpu_gsm0610_restart(spangpu_gsm0610_t *b, int channel, int packing)
{
    int32_t w[kGsmWords];
    if (b == NULL  ||  !channel_ok(&b->k.c, channel)  ||  !gsm0610_init_words(w, packing))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return put_words(b, channel, w);
}

int spangpu_gsm0610_get_state(spangpu_gsm0610_t *b, int channel, int32_t *words)
{
    return codec_get_state(b  ?  &b->k  :  NULL, channel, words);
}

// The channel takes the packing too (a stream moves with it); words no codec could have left are refused.
int spangpu_gsm0610_set_state(spangpu_gsm0610_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->k.c, channel)  ||  !words_ok(words))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w[kGsmWords];
    memcpy(w, words, sizeof(w));
    return put_words(b, channel, w);
}

}   // extern "C"
