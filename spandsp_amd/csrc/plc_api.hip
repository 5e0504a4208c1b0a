// plc_api.hip -- C ABI of the packet loss concealment banks (include/spangpu.h, "Packet loss concealment banks"): batched
// plc_rx() / plc_fillin() on rows in place, from a host caller's word of who was lost or from a decoder bank's counts in
// device memory.  Device code: plc_dev.hpp.  No CPU implementation exists behind these entry points; restart and the state
// calls edit one line's words on the host, as the reference's own calls edit one object.

#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#include "plc_dev.hpp"
#include "bank_host.hpp"

using namespace spg;

struct spangpu_plc_s
{
    BankCore c;
    uint8_t *d_rows;            // a host caller's rows: [n_ch][rows_cap] bytes
    size_t rows_cap;
    VarLens ctl;                // per line 2*len + lost of a call
    bool ctl_kept;              // ctl.dev holds what ctl.pinned holds: a caller that brings the same words tick after tick
    int32_t *scratch;           // [n_ch]: a call's words while they are put together
};

static size_t round16(size_t v)
{
    return (v + 15) & ~(size_t) 15;
}

// what a call's lines do, per line (lens and / or lost) or the same for all
struct PlcCall
{
    const int32_t *lens;
    const int32_t *lost;        // NULL with all_lost: everybody
    int all_len;
    int all_lost;
    int cap;                    // a length's upper bound
};

// The words of a call into scratch; false: a length outside 0..cap.  *uniform: every line has (*uniform) as its word.
static bool call_words(spangpu_plc_s *b, const PlcCall *call, bool *same, int *longest)
{
    *same = true;
    *longest = 0;
    for (int c = 0;  c < b->c.n_ch;  c++)
    {
        const int len = call->lens  ?  call->lens[c]  :  call->all_len;
        if (len < 0  ||  len > call->cap)
            return false;
        b->scratch[c] = 2*len + ((call->lost  ?  (call->lost[c] != 0)  :  call->all_lost)  ?  1  :  0);
        *same = *same  &&  b->scratch[c] == b->scratch[0];
        *longest = (len > *longest)  ?  len  :  *longest;
    }
    return true;
}

// the call's words where the kernel reads them: L->ctl (the last upload where it holds the same words: no copy, no wait)
static int words_to_device(spangpu_plc_s *b, bool same, PlcLaunch *L)
{
    L->ctl = NULL;
    L->ctl_all = b->scratch[0];
    if (same)
        return SPANGPU_OK;
    if (!(b->ctl_kept  &&  memcmp(b->ctl.pinned, b->scratch, (size_t) b->c.n_ch*sizeof(int32_t)) == 0))
    {
        b->ctl_kept = false;
        const int rc = lens_upload(&b->c, &b->ctl, b->scratch);
        if (rc != SPANGPU_OK)
            return rc;
        b->ctl_kept = true;
        b->ctl.next = NULL;
    }
    L->ctl = b->ctl.dev;
    return SPANGPU_OK;
}

static int launch(spangpu_plc_s *b, const PlcLaunch &L)
{
    hipLaunchKernelGGL(plc_kernel, dim3((b->c.n_ch + 63)/64), dim3(64), 0, b->c.stream, L);
    SPG_TRY(hipGetLastError());
    return SPANGPU_OK;
}

static void init_words(int32_t *w)
{
    memset(w, 0, kPlcWords*sizeof(int32_t));
}

extern "C" {

/*
 * Entry point                      stands for (paths relative to the reference tree)
 *   spangpu_plc_create()           plc_init(NULL) x N                                              src/plc.c:261-272
 *   spangpu_plc_run()              plc_rx(s, amp, len) or plc_fillin(s, amp, len), per line        src/plc.c:125-258
 *   spangpu_plc_conceal()          the same, chosen by a decoder bank's counts on the device
 *   spangpu_plc_restart()          plc_init(s) on one line
 *   spangpu_plc_destroy()          plc_free(s) x N                                                 src/plc.c:281-288
 */

void spangpu_plc_destroy(spangpu_plc_t *b)
{
    if (b == NULL)
        return;
    core_destroy(&b->c);
    (void) hipFree(b->d_rows);
    lens_free(&b->ctl);
    free(b->scratch);
    free(b);
}

int spangpu_plc_create(spangpu_plc_t **out, int device, int n_channels)
{
    if (out == NULL  ||  n_channels <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    *out = NULL;
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_plc_s *b = (spangpu_plc_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    b->scratch = (int32_t *) malloc((size_t) n_channels*sizeof(int32_t));
    int32_t w[kPlcWords];
    init_words(w);
    if (b->scratch == NULL)
        rc = spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "malloc");
    else if ((rc = core_create(&b->c, device, n_channels, kPlcWords)) == SPANGPU_OK)
        rc = core_fill(&b->c, w);
    if (rc != SPANGPU_OK)
    {
        spangpu_plc_destroy(b);
        return rc;
    }
    *out = b;
    return SPANGPU_OK;
}

int spangpu_plc_channels(const spangpu_plc_t *b) { return b  ?  b->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_plc_state_words(const spangpu_plc_t *b) { return b  ?  kPlcWords  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_plc_set_stream(spangpu_plc_t *b, void *stream)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&b->c, stream);
}

int spangpu_plc_sync(spangpu_plc_t *b)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&b->c);
}

int spangpu_plc_run(spangpu_plc_t *b, void *amp, int amp_mem_kind, long long amp_stride_bytes, const int32_t *lens, const int32_t *lost,
                    int max_samples)
{
    if (b == NULL  ||  amp == NULL  ||  max_samples < 0  ||  max_samples > kMaxSamples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (mem_kind_ok(amp_mem_kind) != SPANGPU_OK)
        return SPANGPU_ERR_BAD_ARG;
    const bool host = (amp_mem_kind == SPANGPU_MEM_HOST);
    const size_t need = 2*(size_t) max_samples;
    if (host)
    {
        if (amp_stride_bytes < (long long) need)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "the row stride is shorter than the row");
    }
    else
    {
        if ((amp_stride_bytes & 15) != 0  ||  (reinterpret_cast<uintptr_t>(amp) & 15) != 0)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "rows in device memory: base and stride are multiples of 16 bytes");
        if (amp_stride_bytes < (long long) round16(need))
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "the row stride is shorter than the row rounded up to 16 bytes");
    }
    const PlcCall call = {lens, lost, max_samples, 0, max_samples};
    bool same;
    int longest;
    if (!call_words(b, &call, &same, &longest))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a line's length is outside 0..max_samples");
    if (longest == 0)
        return SPANGPU_OK;          // every line sits out
    SPG_TRY(hipSetDevice(b->c.device));
    const size_t nn = (size_t) b->c.n_ch;
    PlcLaunch L;
    memset(&L, 0, sizeof(L));
    int rc;
    if ((rc = words_to_device(b, same, &L)) != SPANGPU_OK)
        return rc;
    L.st = b->c.st;
    L.n_ch = b->c.n_ch;
    L.max_len = max_samples;
    L.rows = (uint8_t *) amp;
    L.stride = amp_stride_bytes;
    if (host)
    {
        if ((rc = grow(&b->d_rows, &b->rows_cap, round16(need), nn, b->c.stream)) != SPANGPU_OK)
            return rc;
        SPG_TRY(hipMemcpy2DAsync(b->d_rows, b->rows_cap, amp, (size_t) amp_stride_bytes, need, nn, hipMemcpyHostToDevice, b->c.stream));
        L.rows = b->d_rows;
        L.stride = (long long) b->rows_cap;
    }
    if ((rc = launch(b, L)) != SPANGPU_OK)
        return rc;
    if (host)
    {
        // a host buffer is only borrowed for the call
        SPG_TRY(hipMemcpy2DAsync(amp, (size_t) amp_stride_bytes, b->d_rows, b->rows_cap, need, nn, hipMemcpyDeviceToHost, b->c.stream));
        SPG_TRY(hipStreamSynchronize(b->c.stream));
    }
    return SPANGPU_OK;
}

int spangpu_plc_conceal(spangpu_plc_t *b, void *amp_dev, long long amp_stride_bytes, const int32_t *counts_dev, const int32_t *fill_lens,
                        int fill_samples, int max_samples)
{
    if (b == NULL  ||  amp_dev == NULL  ||  counts_dev == NULL  ||  max_samples < 0  ||  max_samples > kMaxSamples
        ||  fill_samples < 0  ||  fill_samples > max_samples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if ((amp_stride_bytes & 15) != 0  ||  (reinterpret_cast<uintptr_t>(amp_dev) & 15) != 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "rows in device memory: base and stride are multiples of 16 bytes");
    if (amp_stride_bytes < (long long) round16(2*(size_t) max_samples))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "the row stride is shorter than the row rounded up to 16 bytes");
    const PlcCall call = {fill_lens, NULL, fill_samples, 1, max_samples};
    bool same;
    int longest;
    if (!call_words(b, &call, &same, &longest))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a line's fill length is outside 0..max_samples");
    if (max_samples == 0)
        return SPANGPU_OK;
    SPG_TRY(hipSetDevice(b->c.device));
    PlcLaunch L;
    memset(&L, 0, sizeof(L));
    int rc;
    if ((rc = words_to_device(b, same, &L)) != SPANGPU_OK)
        return rc;
    L.st = b->c.st;
    L.n_ch = b->c.n_ch;
    L.max_len = max_samples;
    L.rows = (uint8_t *) amp_dev;
    L.stride = amp_stride_bytes;
    L.counts = counts_dev;
    return launch(b, L);
}

int spangpu_plc_restart(spangpu_plc_t *b, int channel)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w[kPlcWords];
    init_words(w);
    return core_rw_words(&b->c, channel, 0, kPlcWords, w, true);
}

int spangpu_plc_get_state(spangpu_plc_t *b, int channel, int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, 0, kPlcWords, words, false);
}

// words no plc_state_t could hold, or a lane would index past its words with, are refused
int spangpu_plc_set_state(spangpu_plc_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel)  ||  !plc_words_ok(words))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w[kPlcWords];
    memcpy(w, words, sizeof(w));
    return core_rw_words(&b->c, channel, 0, kPlcWords, w, true);
}

}   // extern "C"
