// bank_host.hip -- the host plumbing the banks share; see bank_host.hpp.  Host code, apart from
// the put kernel of the bit rings.

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "bank_host.hpp"

namespace spg
{

int device_ok(int device)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess  ||  count <= 0)
        return spangpu_set_error(SPANGPU_ERR_NO_DEVICE, "no HIP device: libspangpu has no CPU fallback");
    if (device < 0  ||  device >= count)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "device out of range");
    SPG_TRY(hipSetDevice(device));
    return SPANGPU_OK;
}

int core_create(BankCore *c, int device, int n_channels, int words)
{
    c->device = device;
    c->n_ch = n_channels;
    c->words = words;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
        return spangpu_set_error(SPANGPU_ERR_HIP, "hipStreamCreate failed");
    c->own_stream = true;
    if (hipMalloc(&c->st, (size_t) words*n_channels*sizeof(int32_t)) != hipSuccess)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the bank's state failed");
    return SPANGPU_OK;
}

int core_upload(BankCore *c, const int32_t *host)
{
    if (hipMemcpy(c->st, host, (size_t) c->words*c->n_ch*sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
        return spangpu_set_error(SPANGPU_ERR_HIP, "state upload failed");
    return SPANGPU_OK;
}

int core_fill(BankCore *c, const int32_t *one, int lead)
{
    const size_t n = (size_t) c->n_ch;
    int32_t *host = (int32_t *) calloc((size_t) c->words*n, sizeof(int32_t));
    if (host == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    for (int k = 0;  k < ((lead < 0)  ?  c->words  :  lead);  k++)
    {
        for (size_t ch = 0;  ch < n;  ch++)
            host[(size_t) k*n + ch] = one[k];
    }
    const int rc = core_upload(c, host);
    free(host);
    return rc;
}

int core_set_stream(BankCore *c, void *stream, bool fresh_if_null)
{
    SPG_TRY(hipSetDevice(c->device));
    SPG_TRY(hipStreamSynchronize(c->stream));
    if (c->own_stream)
        (void) hipStreamDestroy(c->stream);
    c->stream = (hipStream_t) stream;
    c->own_stream = false;
    if (stream == NULL  &&  fresh_if_null)
    {
        SPG_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    return SPANGPU_OK;
}

int core_sync(BankCore *c)
{
    SPG_TRY(hipSetDevice(c->device));
    SPG_TRY(hipStreamSynchronize(c->stream));
    return SPANGPU_OK;
}

void core_destroy(BankCore *c)
{
    (void) hipSetDevice(c->device);
    if (c->stream)
        (void) hipStreamSynchronize(c->stream);
    (void) hipFree(c->st);
    if (c->own_stream  &&  c->stream)
        (void) hipStreamDestroy(c->stream);
}

int core_rw_at(BankCore *c, int32_t *base, int ch, int first, int count, int32_t *w, bool write)
{
    SPG_TRY(hipSetDevice(c->device));
    int32_t *at = base + (size_t) first*c->n_ch + ch;
    const size_t pitch = (size_t) c->n_ch*sizeof(int32_t);
    if (write)
        SPG_TRY(hipMemcpy2DAsync(at, pitch, w, sizeof(int32_t), sizeof(int32_t), count, hipMemcpyHostToDevice, c->stream));
    else
        SPG_TRY(hipMemcpy2DAsync(w, sizeof(int32_t), at, pitch, sizeof(int32_t), count, hipMemcpyDeviceToHost, c->stream));
    SPG_TRY(hipStreamSynchronize(c->stream));
    return SPANGPU_OK;
}

int stage_lens(BankCore *c, PcmStage *s)
{
    if (s->d_lens == NULL  &&  hipMalloc(&s->d_lens, (size_t) c->n_ch*sizeof(int32_t)) != hipSuccess)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "length staging");
    return SPANGPU_OK;
}

// the rows of a kernel are read and written 8 samples at a time where they allow it
static int vec_of(const int16_t *pcm, long long stride)
{
    return ((stride & 7) == 0  &&  (reinterpret_cast<uintptr_t>(pcm) & 15) == 0)  ?  1  :  0;
}

static int stage_room(BankCore *c, PcmStage *s, int samples)
{
    return grow(&s->d_pcm, &s->pcm_cap, (size_t) ((samples + 7) & ~7), (size_t) c->n_ch, c->stream);
}

int stage_out_target(BankCore *c, PcmStage *s, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens,
                     int16_t **k_pcm, long long *k_stride, int32_t **k_lens, int *vec)
{
    const bool host = (mem_kind == SPANGPU_MEM_HOST);
    int rc;
    if (host  &&  (rc = stage_room(c, s, samples)) != SPANGPU_OK)
        return rc;
    *k_pcm = host  ?  s->d_pcm  :  pcm;
    *k_stride = host  ?  (long long) s->pcm_cap  :  stride;
    *k_lens = host  ?  s->d_lens  :  lens;
    if (vec)
        *vec = vec_of(*k_pcm, *k_stride);
    return SPANGPU_OK;
}

int stage_out_back(BankCore *c, PcmStage *s, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    if (mem_kind != SPANGPU_MEM_HOST)
        return SPANGPU_OK;
    SPG_TRY(hipMemcpy2DAsync(pcm, (size_t) stride*sizeof(int16_t), s->d_pcm, s->pcm_cap*sizeof(int16_t),
                             (size_t) samples*sizeof(int16_t), c->n_ch, hipMemcpyDeviceToHost, c->stream));
    if (lens)
        SPG_TRY(hipMemcpyAsync(lens, s->d_lens, (size_t) c->n_ch*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SPG_TRY(hipStreamSynchronize(c->stream));
    return SPANGPU_OK;
}

int stage_in(BankCore *c, PcmStage *s, int mem_kind, const int16_t *amp, long long stride, int samples, bool sync,
             const int16_t **k_pcm, long long *k_stride, int *vec)
{
    const bool host = (mem_kind == SPANGPU_MEM_HOST);
    if (host)
    {
        const int rc = stage_room(c, s, samples);
        if (rc != SPANGPU_OK)
            return rc;
        SPG_TRY(hipMemcpy2DAsync(s->d_pcm, s->pcm_cap*sizeof(int16_t), amp, (size_t) stride*sizeof(int16_t),
                                 (size_t) samples*sizeof(int16_t), c->n_ch, hipMemcpyHostToDevice, c->stream));
        if (sync)
            SPG_TRY(hipStreamSynchronize(c->stream));
    }
    *k_pcm = host  ?  s->d_pcm  :  amp;
    *k_stride = host  ?  (long long) s->pcm_cap  :  stride;
    if (vec)
        *vec = vec_of(*k_pcm, *k_stride);
    return SPANGPU_OK;
}

int lens_upload(BankCore *c, VarLens *v, const int32_t *lens)
{
    const size_t bytes = (size_t) c->n_ch*sizeof(int32_t);
    SPG_TRY(hipSetDevice(c->device));
    if (v->dev == NULL)
    {
        SPG_TRY(hipMalloc(&v->dev, bytes));
        SPG_TRY(hipHostMalloc(&v->pinned, bytes));
    }
    SPG_TRY(hipStreamSynchronize(c->stream));
    memcpy(v->pinned, lens, bytes);
    SPG_TRY(hipMemcpyAsync(v->dev, v->pinned, bytes, hipMemcpyHostToDevice, c->stream));
    v->next = v->dev;
    return SPANGPU_OK;
}

int counts_create(BankCore *c, CountRows *k, int rows, int pinned_rows)
{
    const size_t row = (size_t) c->n_ch*sizeof(int32_t);
    if (hipMalloc(&k->dev, rows*row) != hipSuccess  ||  hipHostMalloc(&k->pinned, pinned_rows*row) != hipSuccess)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "result counts");
    return SPANGPU_OK;
}

int counts_fetch(BankCore *c, CountRows *k, int rows)
{
    SPG_TRY(hipSetDevice(c->device));
    SPG_TRY(hipMemcpyAsync(k->pinned, k->dev, (size_t) rows*c->n_ch*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SPG_TRY(hipStreamSynchronize(c->stream));
    return SPANGPU_OK;
}

int rows_fetch(BankCore *c, void *pinned, const void *dev, size_t elem, int cap, int columns)
{
    columns = (columns > cap)  ?  cap  :  columns;
    if (columns > 0)
        SPG_TRY(hipMemcpy2DAsync(pinned, (size_t) cap*elem, dev, (size_t) cap*elem, (size_t) columns*elem, (size_t) c->n_ch,
                                 hipMemcpyDeviceToHost, c->stream));
    return SPANGPU_OK;
}

int quarter_sine_upload(int16_t **quarter)
{
    int16_t q[257];
    for (int i = 0;  i <= 256;  i++)
        q[i] = (int16_t) lrint(32767.0*sin(i*3.14159265358979323846/512.0));
    if (hipMalloc(quarter, sizeof(q)) != hipSuccess)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "quarter sine");
    SPG_TRY(hipMemcpy(*quarter, q, sizeof(q), hipMemcpyHostToDevice));
    return SPANGPU_OK;
}

// Channels [lo, hi): the bits of channel c are packed LSB first at bits[(c - lo)*bstride ...], lens[c - lo] of them;
// accepted[c - lo] = how many had room.
__global__ void bitring_put_kernel(const int32_t *rd_row, int32_t *count_row, uint32_t *queue, int n_ch, int qring, int qcap, int lo,
                                   int hi, const uint8_t *bits, int bstride, const int32_t *lens, int32_t *accepted)
{
    const int ch = lo + blockIdx.x*blockDim.x + threadIdx.x;
    if (ch >= hi)
        return;
    const size_t n = (size_t) n_ch;
    const uint8_t *src = bits + (size_t) (ch - lo)*bstride;
    const int count = count_row[ch];
    int mine = lens[ch - lo];
    mine = (mine > qcap - count)  ?  (qcap - count)  :  mine;
    mine = (mine < 0)  ?  0  :  mine;
    int at = rd_row[ch] + count;
    at -= (at >= qring)  ?  qring  :  0;
    for (int i = 0;  i < mine;  i++)
    {
        const uint32_t bit = (src[i >> 3] >> (i & 7)) & 1u;
        uint32_t *w = queue + (size_t) (at >> 5)*n + ch;
        *w = (*w & ~(1u << (at & 31))) | (bit << (at & 31));
        at = (at + 1 == qring)  ?  0  :  (at + 1);
    }
    count_row[ch] = count + mine;
    accepted[ch - lo] = mine;
}

int bitring_put(BankCore *c, BitPut *p, int32_t *rd_row, int32_t *count_row, uint32_t *queue, int qring, int qcap, int first, int n,
                const uint8_t *bits, int stride, const int32_t *lens, int32_t *accepted)
{
    if (!range_ok(c, first, n)  ||  bits == NULL  ||  lens == NULL  ||  stride <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    for (int i = 0;  i < n;  i++)
    {
        if (lens[i] < 0  ||  (lens[i] + 7)/8 > stride)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a channel's bits do not fit its row");
    }
    SPG_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t) n*stride;
    const size_t row = (size_t) c->n_ch*sizeof(int32_t);
    const int rc = grow(&p->d_bits, &p->bits_cap, bytes, 1, c->stream);
    if (rc != SPANGPU_OK)
        return rc;
    if ((p->d_blens == NULL  &&  hipMalloc(&p->d_blens, row) != hipSuccess)
        ||  (p->d_acc == NULL  &&  hipMalloc(&p->d_acc, row) != hipSuccess))
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "bit staging");
    SPG_TRY(hipMemcpyAsync(p->d_bits, bits, bytes, hipMemcpyHostToDevice, c->stream));
    SPG_TRY(hipMemcpyAsync(p->d_blens, lens, (size_t) n*sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(bitring_put_kernel, dim3((n + 63)/64), dim3(64), 0, c->stream, rd_row, count_row, queue, c->n_ch, qring, qcap,
                       first, first + n, p->d_bits, stride, p->d_blens, p->d_acc);
    SPG_TRY(hipGetLastError());
    if (accepted)
        SPG_TRY(hipMemcpyAsync(accepted, p->d_acc, (size_t) n*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    // the caller's arrays are pageable: they must not change under the copies
    SPG_TRY(hipStreamSynchronize(c->stream));
    return SPANGPU_OK;
}

int bitring_put_device(BankCore *c, BitPut *p, int32_t *rd_row, int32_t *count_row, uint32_t *queue, int qring, int qcap, int first, int n,
                       const uint8_t *bits, int stride, const int32_t *lens, int32_t *accepted)
{
    if (!range_ok(c, first, n)  ||  bits == NULL  ||  lens == NULL  ||  stride <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    SPG_TRY(hipSetDevice(c->device));
    if (accepted == NULL)
    {
        if (p->d_acc == NULL  &&  hipMalloc(&p->d_acc, (size_t) c->n_ch*sizeof(int32_t)) != hipSuccess)
            return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "bit staging");
        accepted = p->d_acc;
    }
    hipLaunchKernelGGL(bitring_put_kernel, dim3((n + 63)/64), dim3(64), 0, c->stream, rd_row, count_row, queue, c->n_ch, qring, qcap,
                       first, first + n, bits, stride, lens, accepted);
    SPG_TRY(hipGetLastError());
    return SPANGPU_OK;
}

}   // namespace spg
