// g726_api.hip -- C ABI of the G.726 ADPCM codec banks (include/spangpu.h, "G.726 codec banks"): batched g726_encode() and
// g726_decode() at the four rates, in the three external codings and the three packings, per channel.  Device code:
// g726_dev.hpp.  No CPU implementation of either path exists behind these entry points; restart and the state calls edit
// one channel's words on the host, as the reference's own g726_init() edits one object.

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#include "g726_dev.hpp"
#include "bank_host.hpp"

using namespace spg;

struct spangpu_g726_s
{
    BankCore c;
    uint8_t *d_in;              // a host caller's rows: [n_ch][in_cap] bytes
    size_t in_cap;
    uint8_t *d_out;
    size_t out_cap;
    VarLens lens;               // per-channel lengths of a call
    bool lens_kept;             // lens.dev holds what lens.pinned holds: a caller that brings the same lengths tick after tick
    CountRows count;            // counts of the last call: bytes (encode) or samples (decode)
    uint8_t *cfg;               // [n_ch][3]: bits per sample, coding, packing, as the state words have them
    // what the capacity functions and the row checks need of cfg
    bool any_unpacked;
    bool any_linear;
    int max_bps;                // over the packed channels, 0: none
    int min_bps;
};

static size_t round16(size_t v)
{
    return (v + 15) & ~(size_t) 15;
}

static void summarise(spangpu_g726_s *b)
{
    b->any_unpacked = false;
    b->any_linear = false;
    b->max_bps = 0;
    b->min_bps = 0;
    for (int c = 0;  c < b->c.n_ch;  c++)
    {
        const int bps = b->cfg[3*c];
        b->any_linear |= (b->cfg[3*c + 1] == kG726Linear);
        if (b->cfg[3*c + 2] == kG726PackNone)
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

// A row in device memory is read and written in aligned 16-byte chunks, its last one whole: the base and the stride are
// multiples of 16 and the stride holds the row rounded up to 16.  A host caller's rows are copied, so any stride that
// holds the row will do.
static int row_ok(const void *p, int mem_kind, long long stride, long long need)
{
    if (p == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null rows");
    if (mem_kind_ok(mem_kind) != SPANGPU_OK)
        return SPANGPU_ERR_BAD_ARG;
    if (mem_kind == SPANGPU_MEM_HOST)
        return (stride >= need)  ?  SPANGPU_OK  :  spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a row stride is shorter than the row");
    if ((stride & 15) != 0  ||  (reinterpret_cast<uintptr_t>(p) & 15) != 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "rows in device memory: base and stride are multiples of 16 bytes");
    if (stride < (long long) round16((size_t) need))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a row stride is shorter than the row rounded up to 16 bytes");
    return SPANGPU_OK;
}

static int run(spangpu_g726_s *b, bool encode, const void *in, int in_kind, long long in_stride, const int32_t *lens, int max_len,
               void *out, int out_kind, long long out_stride, int32_t *counts_out)
{
    if (b == NULL  ||  max_len < 0  ||  max_len > kMaxSamples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const long long in_need = encode  ?  pcm_bytes(b, max_len)  :  (long long) max_len;
    const long long out_need = encode  ?  enc_capacity(b, max_len)  :  pcm_bytes(b, dec_capacity(b, max_len));
    int rc;
    if ((rc = row_ok(in, in_kind, in_stride, in_need)) != SPANGPU_OK  ||  (rc = row_ok(out, out_kind, out_stride, out_need)) != SPANGPU_OK)
        return rc;
    bool all = true;
    int longest = max_len;
    if (lens  &&  (rc = lens_check(lens, b->c.n_ch, max_len, &longest, &all)) != SPANGPU_OK)
        return rc;
    SPG_TRY(hipSetDevice(b->c.device));
    if (longest == 0)
    {
        // nobody brings anything: no launch, and the counts of this call are zeros
        SPG_TRY(hipMemsetAsync(b->count.dev, 0, (size_t) b->c.n_ch*sizeof(int32_t), b->c.stream));
    }
    else
    {
        // (the same lengths as the last upload, the steady state of a gateway's ticks: no copy and no wait)
        if (!all  &&  !(b->lens_kept  &&  memcmp(b->lens.pinned, lens, (size_t) b->c.n_ch*sizeof(int32_t)) == 0))
        {
            b->lens_kept = false;
            if ((rc = lens_upload(&b->c, &b->lens, lens)) != SPANGPU_OK)
                return rc;
            b->lens_kept = true;
        }
        G726Launch L;
        memset(&L, 0, sizeof(L));
        L.st = b->c.st;
        L.lens = all  ?  NULL  :  b->lens.dev;
        L.counts = b->count.dev;
        L.n_ch = b->c.n_ch;
        L.len = longest;
        L.in = (const uint8_t *) in;
        L.in_stride = in_stride;
        if (in_kind == SPANGPU_MEM_HOST)
        {
            const size_t pitch = round16((size_t) in_need);
            if ((rc = grow(&b->d_in, &b->in_cap, pitch, (size_t) b->c.n_ch, b->c.stream)) != SPANGPU_OK)
                return rc;
            SPG_TRY(hipMemcpy2DAsync(b->d_in, b->in_cap, in, (size_t) in_stride, (size_t) in_need, (size_t) b->c.n_ch, hipMemcpyHostToDevice, b->c.stream));
            L.in = b->d_in;
            L.in_stride = (long long) b->in_cap;
        }
        L.out = (uint8_t *) out;
        L.out_stride = out_stride;
        if (out_kind == SPANGPU_MEM_HOST)
        {
            const size_t pitch = round16((size_t) out_need);
            if ((rc = grow(&b->d_out, &b->out_cap, pitch, (size_t) b->c.n_ch, b->c.stream)) != SPANGPU_OK)
                return rc;
            L.out = b->d_out;
            L.out_stride = (long long) b->out_cap;
        }
        const dim3 grid((b->c.n_ch + 63)/64);
        if (encode)
            hipLaunchKernelGGL(g726_kernel<true>, grid, dim3(64), 0, b->c.stream, L);
        else
            hipLaunchKernelGGL(g726_kernel<false>, grid, dim3(64), 0, b->c.stream, L);
        SPG_TRY(hipGetLastError());
        if (out_kind == SPANGPU_MEM_HOST  &&  out_need > 0)
            SPG_TRY(hipMemcpy2DAsync(out, (size_t) out_stride, b->d_out, b->out_cap, (size_t) out_need, (size_t) b->c.n_ch, hipMemcpyDeviceToHost, b->c.stream));
    }
    b->lens.next = NULL;
    if (counts_out)
    {
        // the one wait of the call, behind the rows
        if ((rc = counts_fetch(&b->c, &b->count, 1)) != SPANGPU_OK)
            return rc;
        memcpy(counts_out, b->count.pinned, (size_t) b->c.n_ch*sizeof(int32_t));
    }
    else if (in_kind == SPANGPU_MEM_HOST  ||  out_kind == SPANGPU_MEM_HOST)
        SPG_TRY(hipStreamSynchronize(b->c.stream));         // a host buffer is only borrowed for the call
    return SPANGPU_OK;
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
    core_destroy(&b->c);
    (void) hipFree(b->d_in);
    (void) hipFree(b->d_out);
    lens_free(&b->lens);
    counts_free(&b->count);
    free(b->cfg);
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
    if ((rc = core_create(&b->c, device, n_channels, kG726Words)) != SPANGPU_OK  ||  (rc = counts_create(&b->c, &b->count, 1, 1)) != SPANGPU_OK)
    {
        spangpu_g726_destroy(b);
        return rc;
    }
    const size_t nn = (size_t) n_channels;
    int32_t *host = (int32_t *) calloc((size_t) kG726Words*nn, sizeof(int32_t));
    b->cfg = (uint8_t *) malloc(3*nn);
    if (host == NULL  ||  b->cfg == NULL)
    {
        free(host);
        spangpu_g726_destroy(b);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the codec bank failed");
    }
    for (int c = 0;  c < n_channels;  c++)
    {
        (void) g726_init_words(one, rates[c % n], codings[c % n], packings[c % n]);
        for (int w = 0;  w < kG726Words;  w++)
            host[(size_t) w*nn + c] = one[w];
        b->cfg[3*c] = (uint8_t) one[G7_BPS];
        b->cfg[3*c + 1] = (uint8_t) one[G7_CODING];
        b->cfg[3*c + 2] = (uint8_t) one[G7_PACKING];
    }
    summarise(b);
    rc = core_upload(&b->c, host);
    free(host);
    if (rc == SPANGPU_OK  &&  hipMemset(b->count.dev, 0, nn*sizeof(int32_t)) != hipSuccess)
        rc = spangpu_set_error(SPANGPU_ERR_HIP, "state upload failed");
    if (rc != SPANGPU_OK)
    {
        spangpu_g726_destroy(b);
        return rc;
    }
    *out = b;
    return SPANGPU_OK;
}

int spangpu_g726_channels(const spangpu_g726_t *b) { return b  ?  b->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_g726_state_words(const spangpu_g726_t *b) { return b  ?  kG726Words  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_g726_set_stream(spangpu_g726_t *b, void *stream)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&b->c, stream);
}

int spangpu_g726_sync(spangpu_g726_t *b)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&b->c);
}

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
    return b  ?  b->count.dev  :  NULL;
}

static int put_words(spangpu_g726_s *b, int channel, int32_t *w)
{
    const int rc = core_rw_words(&b->c, channel, 0, kG726Words, w, true);
    if (rc != SPANGPU_OK)
        return rc;
    b->cfg[3*channel] = (uint8_t) w[G7_BPS];
    b->cfg[3*channel + 1] = (uint8_t) w[G7_CODING];
    b->cfg[3*channel + 2] = (uint8_t) w[G7_PACKING];
    summarise(b);
    return SPANGPU_OK;
}

int spangpu_g726_restart(spangpu_g726_t *b, int channel, int rate, int coding, int packing)
{
    int32_t w[kG726Words];
    if (b == NULL  ||  !channel_ok(&b->c, channel)  ||  !g726_init_words(w, rate, coding, packing))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return put_words(b, channel, w);
}

int spangpu_g726_get_state(spangpu_g726_t *b, int channel, int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, 0, kG726Words, words, false);
}

// The channel takes the configuration words too (a stream moves with its rate, coding and packing); a set of them that
// g726_init() could not have made, or a bit residue outside 0..7, is refused.
int spangpu_g726_set_state(spangpu_g726_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel)  ||  !config_ok(words)  ||  words[G7_RESIDUE] < 0  ||  words[G7_RESIDUE] > 7)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return put_words(b, channel, const_cast<int32_t *>(words));
}

}   // extern "C"
