// codec_host.hip -- what of codec_host.hpp is not inline: a codec bank's making and unmaking, one encode / decode call, and
// the state calls.

#include <stdlib.h>
#include <string.h>

#include "codec_host.hpp"

namespace spg
{

static size_t round16(size_t v)
{
    return (v + 15) & ~(size_t) 15;
}

static void cfg_take(CodecBank *k, int channel, const int32_t *w)
{
    for (int i = 0;  i < 3;  i++)
        k->cfg[3*channel + i] = (uint8_t) w[k->cfg_word[i]];
}

int codec_create(CodecBank *k, int device, int n_channels, int words, int cfg0, int cfg1, int cfg2, CodecInit init, const void *arg)
{
    int rc;
    if ((rc = core_create(&k->c, device, n_channels, words)) != SPANGPU_OK  ||  (rc = counts_create(&k->c, &k->count, 1, 1)) != SPANGPU_OK)
        return rc;
    k->cfg_word[0] = cfg0;
    k->cfg_word[1] = cfg1;
    k->cfg_word[2] = cfg2;
    const size_t nn = (size_t) n_channels;
    int32_t *host = (int32_t *) calloc((size_t) words*nn, sizeof(int32_t));
    int32_t *one = (int32_t *) calloc((size_t) words, sizeof(int32_t));
    k->cfg = (uint8_t *) malloc(3*nn);
    if (host == NULL  ||  one == NULL  ||  k->cfg == NULL)
    {
        free(host);
        free(one);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the codec bank failed");
    }
    for (int c = 0;  c < n_channels;  c++)
    {
        init(arg, c, one);
        for (int w = 0;  w < words;  w++)
            host[(size_t) w*nn + c] = one[w];
        cfg_take(k, c, one);
    }
    rc = core_upload(&k->c, host);
    free(host);
    free(one);
    if (rc == SPANGPU_OK  &&  hipMemset(k->count.dev, 0, nn*sizeof(int32_t)) != hipSuccess)
        rc = spangpu_set_error(SPANGPU_ERR_HIP, "state upload failed");
    return rc;
}

void codec_destroy(CodecBank *k)
{
    core_destroy(&k->c);
    (void) hipFree(k->d_in);
    (void) hipFree(k->d_out);
    lens_free(&k->lens);
    counts_free(&k->count);
    free(k->cfg);
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

int codec_check(const CodecBank *k, CodecCall *call)
{
    int rc;
    if ((rc = row_ok(call->in, call->in_kind, call->in_stride, call->in_need)) != SPANGPU_OK
        ||  (rc = row_ok(call->out, call->out_kind, call->out_stride, call->out_need)) != SPANGPU_OK)
        return rc;
    call->all = true;
    call->longest = call->max_len;
    return call->lens  ?  lens_check(call->lens, k->c.n_ch, call->max_len, &call->longest, &call->all)  :  SPANGPU_OK;
}

int codec_run(CodecBank *k, const CodecCall *call, CodecLaunchFn launch)
{
    const size_t nn = (size_t) k->c.n_ch;
    const bool in_host = (call->in_kind == SPANGPU_MEM_HOST);
    const bool out_host = (call->out_kind == SPANGPU_MEM_HOST);
    int rc;
    SPG_TRY(hipSetDevice(k->c.device));
    if (call->longest == 0)
    {
        // nobody brings anything: no launch, and the counts of this call are zeros
        SPG_TRY(hipMemsetAsync(k->count.dev, 0, nn*sizeof(int32_t), k->c.stream));
    }
    else
    {
        // (the same lengths as the last upload, the steady state of a gateway's ticks: no copy and no wait)
        if (!call->all  &&  !(k->lens_kept  &&  memcmp(k->lens.pinned, call->lens, nn*sizeof(int32_t)) == 0))
        {
            k->lens_kept = false;
            if ((rc = lens_upload(&k->c, &k->lens, call->lens)) != SPANGPU_OK)
                return rc;
            k->lens_kept = true;
        }
        CodecLaunch L;
        memset(&L, 0, sizeof(L));
        L.st = k->c.st;
        L.lens = call->all  ?  NULL  :  k->lens.dev;
        L.counts = k->count.dev;
        L.n_ch = k->c.n_ch;
        L.len = call->longest;
        L.in = (const uint8_t *) call->in;
        L.in_stride = call->in_stride;
        if (in_host)
        {
            if ((rc = grow(&k->d_in, &k->in_cap, round16((size_t) call->in_need), nn, k->c.stream)) != SPANGPU_OK)
                return rc;
            SPG_TRY(hipMemcpy2DAsync(k->d_in, k->in_cap, call->in, (size_t) call->in_stride, (size_t) call->in_need, nn, hipMemcpyHostToDevice, k->c.stream));
            L.in = k->d_in;
            L.in_stride = (long long) k->in_cap;
        }
        L.out = (uint8_t *) call->out;
        L.out_stride = call->out_stride;
        if (out_host)
        {
            if ((rc = grow(&k->d_out, &k->out_cap, round16((size_t) call->out_need), nn, k->c.stream)) != SPANGPU_OK)
                return rc;
            L.out = k->d_out;
            L.out_stride = (long long) k->out_cap;
        }
        launch(L, dim3((k->c.n_ch + 63)/64), k->c.stream);
        SPG_TRY(hipGetLastError());
        if (out_host  &&  call->out_need > 0)
            SPG_TRY(hipMemcpy2DAsync(call->out, (size_t) call->out_stride, k->d_out, k->out_cap, (size_t) call->out_need, nn, hipMemcpyDeviceToHost, k->c.stream));
    }
    k->lens.next = NULL;
    if (call->counts_out)
    {
        // the one wait of the call, behind the rows
        if ((rc = counts_fetch(&k->c, &k->count, 1)) != SPANGPU_OK)
            return rc;
        memcpy(call->counts_out, k->count.pinned, nn*sizeof(int32_t));
    }
    else if (in_host  ||  out_host)
        SPG_TRY(hipStreamSynchronize(k->c.stream));         // a host buffer is only borrowed for the call
    return SPANGPU_OK;
}

int codec_put_words(CodecBank *k, int channel, int32_t *w)
{
    const int rc = core_rw_words(&k->c, channel, 0, k->c.words, w, true);
    if (rc == SPANGPU_OK)
        cfg_take(k, channel, w);
    return rc;
}

int codec_get_state(CodecBank *k, int channel, int32_t *words)
{
    if (k == NULL  ||  words == NULL  ||  !channel_ok(&k->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&k->c, channel, 0, k->c.words, words, false);
}

int codec_set_stream(CodecBank *k, void *stream)
{
    if (k == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&k->c, stream);
}

int codec_sync(CodecBank *k)
{
    if (k == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&k->c);
}

}   // namespace spg
