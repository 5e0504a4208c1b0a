// awgn_api.hip -- C ABI of the noise source banks (include/spangpu.h, "noise source banks"): batched
// awgn_init_dbm0() / awgn().  Device code: awgn_dev.hpp.  No CPU implementation of the generator exists behind
// these entry points; the host only seeds the per-channel state (integer LCG steps and pow(), as awgn.c:82-146).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#include "awgn_dev.hpp"
#include "bank_host.hpp"

using namespace spg;

struct spangpu_awgn_s
{
    BankCore c;
    int16_t *d_amp;         // staging for a host caller: whole rows at the caller's stride
    size_t amp_cap;         // samples
};

static void put_double(int32_t w[], double v)
{
    memcpy(w, &v, sizeof(v));           // little endian: low word first
}

// ran_init() + awgn_init_dbov(level - DBM0_MAX_POWER): awgn.c:82-105,127-152
static void seed_words(int32_t w[kAwgnWords], int idum, float level)
{
    if (idum < 0)
        idum = -idum;
    int ix1 = (54773 + idum)%259200;
    ix1 = (7141*ix1 + 54773)%259200;
    int ix2 = ix1%134456;
    ix1 = (7141*ix1 + 54773)%259200;
    const int ix3 = ix1%243000;
    for (int j = 0;  j < 97;  j++)
    {
        ix1 = (7141*ix1 + 54773)%259200;
        ix2 = (8121*ix2 + 28411)%134456;
        put_double(&w[AW_R + 2*j], ((double) ix1 + (double) ix2*(1.0/134456.0))*(1.0/259200.0));
    }
    level -= (3.14f + 3.02f);
    put_double(&w[AW_RMS], pow(10.0, level/20.0)*32768.0);
    put_double(&w[AW_AMP2], 0.0);
    w[AW_ODD] = 1;
    w[AW_IX1] = ix1;
    w[AW_IX2] = ix2;
    w[AW_IX3] = ix3;
}

extern "C" {

int spangpu_awgn_create(spangpu_awgn_t **out, int device, int n_channels, const int32_t seeds[], const float levels_dbm0[])
{
    if (out == NULL  ||  n_channels <= 0  ||  seeds == NULL  ||  levels_dbm0 == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    *out = NULL;
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_awgn_s *b = (spangpu_awgn_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    int32_t *host = (int32_t *) malloc((size_t) kAwgnWords*n_channels*sizeof(int32_t));
    if (host == NULL)
        rc = spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the noise source bank failed");
    else
        rc = core_create(&b->c, device, n_channels, kAwgnWords);
    int32_t one[kAwgnWords];
    for (int c = 0;  rc == SPANGPU_OK  &&  c < n_channels;  c++)
    {
        seed_words(one, seeds[c], levels_dbm0[c]);
        for (int k = 0;  k < kAwgnWords;  k++)
            host[(size_t) k*n_channels + c] = one[k];
    }
    if (rc == SPANGPU_OK)
        rc = core_upload(&b->c, host);
    free(host);
    if (rc != SPANGPU_OK)
    {
        spangpu_awgn_destroy(b);
        return rc;
    }
    *out = b;
    return SPANGPU_OK;
}

void spangpu_awgn_destroy(spangpu_awgn_t *b)
{
    if (b == NULL)
        return;
    core_destroy(&b->c);
    (void) hipFree(b->d_amp);
    free(b);
}

int spangpu_awgn_channels(const spangpu_awgn_t *b) { return b  ?  b->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_awgn_state_words(const spangpu_awgn_t *b) { return b  ?  kAwgnWords  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_awgn_set_stream(spangpu_awgn_t *b, void *stream)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&b->c, stream);
}

int spangpu_awgn_sync(spangpu_awgn_t *b)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&b->c);
}

int spangpu_awgn_reinit(spangpu_awgn_t *b, int channel, int seed, float level_dbm0)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t one[kAwgnWords];
    seed_words(one, seed, level_dbm0);
    return core_rw_words(&b->c, channel, 0, kAwgnWords, one, true);
}

int spangpu_awgn_tx(spangpu_awgn_t *b, int mem_kind, int16_t *amp, long long stride, int samples, int mix)
{
    int rc = rx_args_ok(b, mem_kind, amp, samples, &stride);
    if (rc != SPANGPU_OK)
        return rc;
    SPG_TRY(hipSetDevice(b->c.device));
    AwgnLaunch L;
    memset(&L, 0, sizeof(L));
    L.st = b->c.st;
    L.n_ch = b->c.n_ch;
    L.samples = samples;
    L.mix = mix  ?  1  :  0;
    // (not a PcmStage: the noise is mixed into whole rows at the caller's own stride, and the kernel has no vector path)
    const size_t count = (size_t) b->c.n_ch*(size_t) stride;
    const size_t bytes = count*sizeof(int16_t);
    if (mem_kind == SPANGPU_MEM_HOST)
    {
        if ((rc = grow(&b->d_amp, &b->amp_cap, count, 1, b->c.stream)) != SPANGPU_OK)
            return rc;
        if (mix)
            SPG_TRY(hipMemcpyAsync(b->d_amp, amp, bytes, hipMemcpyHostToDevice, b->c.stream));
        L.amp = b->d_amp;
    }
    else
    {
        L.amp = amp;
    }
    L.stride = stride;
    hipLaunchKernelGGL(awgn_bank_kernel, dim3((b->c.n_ch + 63)/64), dim3(64), (97*64 + 2*kLogTab)*sizeof(double), b->c.stream, L);
    SPG_TRY(hipGetLastError());
    if (mem_kind == SPANGPU_MEM_HOST)
    {
        // the caller's buffer is only borrowed for this call
        SPG_TRY(hipMemcpyAsync(amp, b->d_amp, bytes, hipMemcpyDeviceToHost, b->c.stream));
        SPG_TRY(hipStreamSynchronize(b->c.stream));
    }
    return samples;
}

int spangpu_awgn_get_state(spangpu_awgn_t *b, int channel, int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, 0, kAwgnWords, words, false);
}

}   // extern "C"
