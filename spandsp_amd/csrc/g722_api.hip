// g722_api.hip -- C ABI of the G.722 wideband codec banks (include/spangpu.h, "G.722 codec banks"): batched g722_encode() or
// g722_decode() at the three rates, at 16 kHz or 8 kHz, packed or not, per channel.  Device code: g722_dev.hpp.  No CPU
// implementation of either path exists behind these entry points; restart and the state calls edit one channel's words on
// the host, as the reference's own g722_*_init() edits one object.

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#include "g722_dev.hpp"
#include "bank_host.hpp"

using namespace spg;

struct spangpu_g722_s
{
    BankCore c;
    int direction;              // SPANGPU_G722_ENCODER or SPANGPU_G722_DECODER
    uint8_t *d_in;              // a host caller's rows: [n_ch][in_cap] bytes
    size_t in_cap;
    uint8_t *d_out;
    size_t out_cap;
    VarLens lens;               // per-channel lengths of a call
    bool lens_kept;             // lens.dev holds what lens.pinned holds: a caller that brings the same lengths tick after tick
    CountRows count;            // counts of the last call: bytes (encode) or samples (decode)
    uint8_t *cfg;               // [n_ch][3]: bits per sample, eight_k, packed, as the state words have them
    int present[3][2][2];       // channels per configuration: what the capacity functions and the row checks need of cfg
};

static size_t round16(size_t v)
{
    return (v + 15) & ~(size_t) 15;
}

static void summarise(spangpu_g722_s *b)
{
    memset(b->present, 0, sizeof(b->present));
    for (int c = 0;  c < b->c.n_ch;  c++)
        b->present[b->cfg[3*c] - 6][b->cfg[3*c + 1]][b->cfg[3*c + 2]]++;
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

static int run(spangpu_g722_s *b, bool encode, const void *in, int in_kind, long long in_stride, const int32_t *lens, int max_len,
               void *out, int out_kind, long long out_stride, int32_t *counts_out)
{
    if (b == NULL  ||  max_len < 0  ||  max_len > kMaxSamples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (b->direction != (encode  ?  SPANGPU_G722_ENCODER  :  SPANGPU_G722_DECODER))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "an encoder bank does not decode, and a decoder bank does not encode");
    const long long in_need = encode  ?  2*(long long) max_len  :  (long long) max_len;
    const long long out_need = encode  ?  capacity(b, true, max_len)  :  2*capacity(b, false, max_len);
    int rc;
    if ((rc = row_ok(in, in_kind, in_stride, in_need)) != SPANGPU_OK  ||  (rc = row_ok(out, out_kind, out_stride, out_need)) != SPANGPU_OK)
        return rc;
    bool all = true;
    int longest = max_len;
    if (lens  &&  (rc = lens_check(lens, b->c.n_ch, max_len, &longest, &all)) != SPANGPU_OK)
        return rc;
    // a 16 kHz encoder takes pairs: the reference reads amp[len] at an odd len
    if (encode)
    {
        for (int c = 0;  c < b->c.n_ch;  c++)
        {
            if (!b->cfg[3*c + 1]  &&  ((lens  ?  lens[c]  :  max_len) & 1))
                return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "an odd number of samples for a 16 kHz encoder");
        }
    }
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
        G722Launch L;
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
            hipLaunchKernelGGL(g722_kernel<true>, grid, dim3(64), 0, b->c.stream, L);
        else
            hipLaunchKernelGGL(g722_kernel<false>, grid, dim3(64), 0, b->c.stream, L);
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
    core_destroy(&b->c);
    (void) hipFree(b->d_in);
    (void) hipFree(b->d_out);
    lens_free(&b->lens);
    counts_free(&b->count);
    free(b->cfg);
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
    if ((rc = core_create(&b->c, device, n_channels, kG722Words)) != SPANGPU_OK  ||  (rc = counts_create(&b->c, &b->count, 1, 1)) != SPANGPU_OK)
    {
        spangpu_g722_destroy(b);
        return rc;
    }
    b->direction = direction;
    const size_t nn = (size_t) n_channels;
    int32_t *host = (int32_t *) calloc((size_t) kG722Words*nn, sizeof(int32_t));
    b->cfg = (uint8_t *) malloc(3*nn);
    if (host == NULL  ||  b->cfg == NULL)
    {
        free(host);
        spangpu_g722_destroy(b);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the codec bank failed");
    }
    for (int c = 0;  c < n_channels;  c++)
    {
        (void) g722_init_words(one, rates[c % n], options[c % n]);
        for (int w = 0;  w < kG722Words;  w++)
            host[(size_t) w*nn + c] = one[w];
        b->cfg[3*c] = (uint8_t) one[G2_BPS];
        b->cfg[3*c + 1] = (uint8_t) one[G2_EIGHT_K];
        b->cfg[3*c + 2] = (uint8_t) one[G2_PACKED];
    }
    summarise(b);
    rc = core_upload(&b->c, host);
    free(host);
    if (rc == SPANGPU_OK  &&  hipMemset(b->count.dev, 0, nn*sizeof(int32_t)) != hipSuccess)
        rc = spangpu_set_error(SPANGPU_ERR_HIP, "state upload failed");
    if (rc != SPANGPU_OK)
    {
        spangpu_g722_destroy(b);
        return rc;
    }
    *out = b;
    return SPANGPU_OK;
}

int spangpu_g722_channels(const spangpu_g722_t *b) { return b  ?  b->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_g722_state_words(const spangpu_g722_t *b) { return b  ?  kG722Words  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_g722_set_stream(spangpu_g722_t *b, void *stream)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&b->c, stream);
}

int spangpu_g722_sync(spangpu_g722_t *b)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&b->c);
}

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
    return b  ?  b->count.dev  :  NULL;
}

static int put_words(spangpu_g722_s *b, int channel, int32_t *w)
{
    const int rc = core_rw_words(&b->c, channel, 0, kG722Words, w, true);
    if (rc != SPANGPU_OK)
        return rc;
    b->cfg[3*channel] = (uint8_t) w[G2_BPS];
    b->cfg[3*channel + 1] = (uint8_t) w[G2_EIGHT_K];
    b->cfg[3*channel + 2] = (uint8_t) w[G2_PACKED];
    summarise(b);
    return SPANGPU_OK;
}

int spangpu_g722_restart(spangpu_g722_t *b, int channel, int rate, int options)
{
    int32_t w[kG722Words];
    if (b == NULL  ||  !channel_ok(&b->c, channel)  ||  !g722_init_words(w, rate, options))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return put_words(b, channel, w);
}

int spangpu_g722_get_state(spangpu_g722_t *b, int channel, int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, 0, kG722Words, words, false);
}

// The channel takes the configuration words too (a stream moves with its rate, sample rate and packing, its histories and
// the bits that wait); words no codec could have left are refused.
int spangpu_g722_set_state(spangpu_g722_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel)  ||  !words_ok(words))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return put_words(b, channel, const_cast<int32_t *>(words));
}

}   // extern "C"
