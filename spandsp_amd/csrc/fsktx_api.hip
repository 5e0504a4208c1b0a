// fsktx_api.hip -- C ABI of the FSK and modem connect tone transmitter banks (include/spangpu.h, "FSK and connect tone
// transmitter banks"): batched fsk_tx() / modem_connect_tones_tx() as device-side signal sources, and the async_tx
// character framing in front of the FSK modulator.  Device code: fsktx_dev.hpp.  No CPU implementation of the generators
// exists behind these entry points; the two framing helpers at the end are plain host code.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#include "modem_tables.h"
#include "fsktx_dev.hpp"

using namespace spg;

extern "C" int spangpu_set_error(int code, const char *msg);

#define FT_TRY(expr)                                                                        \
    do                                                                                      \
    {                                                                                       \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
        {                                                                                   \
            char m_[256];                                                                   \
            snprintf(m_, sizeof(m_), "%s failed: %s", #expr, hipGetErrorString(e_));        \
            return spangpu_set_error(SPANGPU_ERR_HIP, m_);                                  \
        }                                                                                   \
    }                                                                                       \
    while (0)

constexpr int kMaxSamples = 1 << 24;        // per call: the chunk index of a wave's 16 rows stays inside 32 bits

// What the two banks share: the stream, the state words, the quarter sine and the staging of a host caller's frame.
struct TxCommon
{
    int device;
    int n_ch;
    int words;
    hipStream_t stream;
    bool own_stream;
    int32_t *st;
    int16_t *quarter;
    int16_t *d_pcm;
    size_t pcm_cap;
    int32_t *d_lens;
};

struct spangpu_fsktx_s
{
    TxCommon c;
    int source;
    int qcap;               // bits a channel's ring takes
    int qring;              // ring size in bits: qcap rounded up to whole words
    uint32_t *queue;
    int32_t *h_row;         // [n_ch] host scratch: a row of state words, the list of events
    uint8_t *frame_par;     // [n_ch][3]: data bits, parity, stop bits of spangpu_fsktx_put_bytes()
    uint8_t *d_bits;
    int32_t *d_blens;
    int32_t *d_acc;
    size_t bits_cap;
    int put_cap;
};

struct spangpu_mcttx_s
{
    TxCommon c;
    int tone_type;
    MctTxLaunch proto;      // the tone type's constants
    int32_t init[kMctTxWords];
};

// dds_scaling_dbm0(), dds_int.c:328-331 (DBM0_MAX_SINE_POWER = 3.14f); dds_phase_rate(), dds_int.c:316-319
static int scaling_dbm0(float level)
{
    return (int16_t) (spg_db_to_amplitude_ratio(level - 3.14f)*32767.0f);
}

static int32_t phase_rate(float hz)
{
    return (int32_t) (hz*65536.0f*65536.0f/8000);
}

static int spec_ok(const spangpu_fsk_spec_t *spec)
{
    // a boundary at most once per sample keeps baud_frac below 800000, as every real modem does
    return spec != NULL  &&  spec->baud_rate > 0  &&  spec->baud_rate <= kFtxBaudUnit;
}

// fsk_tx_restart(), fsk.c:221-235
static void fsk_restart_words(int32_t *w, const spangpu_fsk_spec_t *spec)
{
    w[FT_BAUD_RATE] = spec->baud_rate;
    w[FT_RATE0] = phase_rate((float) spec->freq_zero);
    w[FT_RATE1] = phase_rate((float) spec->freq_one);
    w[FT_SCALING] = scaling_dbm0((float) spec->tx_level);
    w[FT_PHASE] = 0;
    w[FT_BAUD_FRAC] = 0;
    w[FT_CUR_RATE] = w[FT_RATE1];
    w[FT_SHUTDOWN] = 0;
}

// (for the bank families that carry an FSK sender inside them, v18_api.hip; not part of the ABI)
extern "C" __attribute__((visibility("hidden"))) void spangpu_fsktx_words_restart(int32_t *w, const spangpu_fsk_spec_t *spec)
{
    fsk_restart_words(w, spec);
}

static int common_create(TxCommon *c, int device, int n_channels, int words)
{
    c->device = device;
    c->n_ch = n_channels;
    c->words = words;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
        return spangpu_set_error(SPANGPU_ERR_HIP, "hipStreamCreate failed");
    c->own_stream = true;
    if (hipMalloc(&c->st, (size_t) words*n_channels*sizeof(int32_t)) != hipSuccess
        ||  hipMalloc(&c->quarter, 257*sizeof(int16_t)) != hipSuccess
        ||  hipMalloc(&c->d_lens, (size_t) n_channels*sizeof(int32_t)) != hipSuccess)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the transmitter bank failed");
    // dds_int.c: one quadrant of a sine, 257 entries
    int16_t quarter[257];
    for (int i = 0;  i <= 256;  i++)
        quarter[i] = (int16_t) lrint(32767.0*sin(i*3.14159265358979323846/512.0));
    if (hipMemcpy(c->quarter, quarter, sizeof(quarter), hipMemcpyHostToDevice) != hipSuccess)
        return spangpu_set_error(SPANGPU_ERR_HIP, "table upload failed");
    return SPANGPU_OK;
}

static void common_destroy(TxCommon *c)
{
    (void) hipSetDevice(c->device);
    if (c->stream)
        (void) hipStreamSynchronize(c->stream);
    (void) hipFree(c->st);
    (void) hipFree(c->quarter);
    (void) hipFree(c->d_pcm);
    (void) hipFree(c->d_lens);
    if (c->own_stream  &&  c->stream)
        (void) hipStreamDestroy(c->stream);
}

// every channel starts from the same words
static int common_fill(TxCommon *c, const int32_t *one)
{
    const size_t n = (size_t) c->n_ch;
    int32_t *host = (int32_t *) malloc((size_t) c->words*n*sizeof(int32_t));
    if (host == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "malloc");
    for (int k = 0;  k < c->words;  k++)
    {
        for (size_t ch = 0;  ch < n;  ch++)
            host[(size_t) k*n + ch] = one[k];
    }
    const hipError_t e = hipMemcpy(c->st, host, (size_t) c->words*n*sizeof(int32_t), hipMemcpyHostToDevice);
    free(host);
    if (e != hipSuccess)
        return spangpu_set_error(SPANGPU_ERR_HIP, "state upload failed");
    return SPANGPU_OK;
}

static int common_set_stream(TxCommon *c, void *stream)
{
    FT_TRY(hipSetDevice(c->device));
    FT_TRY(hipStreamSynchronize(c->stream));
    if (c->own_stream)
        (void) hipStreamDestroy(c->stream);
    c->stream = (hipStream_t) stream;
    c->own_stream = false;
    return SPANGPU_OK;
}

static int common_sync(TxCommon *c)
{
    FT_TRY(hipSetDevice(c->device));
    FT_TRY(hipStreamSynchronize(c->stream));
    return SPANGPU_OK;
}

// words [first, first + count) of one channel
static int rw_words(TxCommon *c, int ch, int first, int count, int32_t *w, bool write)
{
    FT_TRY(hipSetDevice(c->device));
    int32_t *at = c->st + (size_t) first*c->n_ch + ch;
    if (write)
        FT_TRY(hipMemcpy2DAsync(at, (size_t) c->n_ch*sizeof(int32_t), w, sizeof(int32_t), sizeof(int32_t), count,
                                hipMemcpyHostToDevice, c->stream));
    else
        FT_TRY(hipMemcpy2DAsync(w, sizeof(int32_t), at, (size_t) c->n_ch*sizeof(int32_t), sizeof(int32_t), count,
                                hipMemcpyDeviceToHost, c->stream));
    FT_TRY(hipStreamSynchronize(c->stream));
    return SPANGPU_OK;
}

// Where the kernel writes: the caller's rows, or a staging copy of them for a host caller.
static int frame_target(TxCommon *c, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens, int16_t **k_pcm,
                        long long *k_stride, int32_t **k_lens, int *vec)
{
    if (mem_kind == SPANGPU_MEM_HOST)
    {
        const size_t need = (size_t) ((samples + 7) & ~7);
        if (need > c->pcm_cap)
        {
            FT_TRY(hipStreamSynchronize(c->stream));
            (void) hipFree(c->d_pcm);
            c->d_pcm = NULL;
            c->pcm_cap = 0;
            if (hipMalloc(&c->d_pcm, need*c->n_ch*sizeof(int16_t)) != hipSuccess)
                return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "pcm staging");
            c->pcm_cap = need;
        }
        *k_pcm = c->d_pcm;
        *k_stride = (long long) c->pcm_cap;
        *k_lens = c->d_lens;
    }
    else
    {
        *k_pcm = pcm;
        *k_stride = stride;
        *k_lens = lens;
    }
    *vec = ((*k_stride & 7) == 0  &&  (reinterpret_cast<uintptr_t>(*k_pcm) & 15) == 0)  ?  1  :  0;
    return SPANGPU_OK;
}

static int frame_back(TxCommon *c, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    if (mem_kind != SPANGPU_MEM_HOST)
        return SPANGPU_OK;
    FT_TRY(hipMemcpy2DAsync(pcm, (size_t) stride*sizeof(int16_t), c->d_pcm, c->pcm_cap*sizeof(int16_t),
                            (size_t) samples*sizeof(int16_t), c->n_ch, hipMemcpyDeviceToHost, c->stream));
    if (lens)
        FT_TRY(hipMemcpyAsync(lens, c->d_lens, (size_t) c->n_ch*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    FT_TRY(hipStreamSynchronize(c->stream));
    return SPANGPU_OK;
}

static int tx_args_ok(const void *t, int mem_kind, const int16_t *pcm, long long stride, int samples)
{
    if (t == NULL  ||  pcm == NULL  ||  samples < 0  ||  samples > kMaxSamples  ||  stride < samples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (mem_kind != SPANGPU_MEM_HOST  &&  mem_kind != SPANGPU_MEM_DEVICE)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad mem kind");
    return SPANGPU_OK;
}

static int device_ok(int device)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess  ||  count <= 0)
        return spangpu_set_error(SPANGPU_ERR_NO_DEVICE, "no HIP device: libspangpu has no CPU fallback");
    if (device < 0  ||  device >= count)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "device out of range");
    FT_TRY(hipSetDevice(device));
    return SPANGPU_OK;
}

static int framing_ok(int data_bits, int parity, int stop_bits)
{
    return data_bits >= 5  &&  data_bits <= 8  &&  parity >= SPANGPU_ASYNC_PARITY_NONE  &&  parity <= SPANGPU_ASYNC_PARITY_SPACE
           &&  stop_bits >= 1  &&  stop_bits <= 2;
}

// async_tx_get_bit() of one character, async.c:303-335: start bit, data LSB first, parity, stop bits
static int frame_one(int data_bits, int parity, int stop_bits, int byte, uint8_t *out)
{
    int frame = byte & (0xFFFF >> (16 - data_bits));
    int total_data_bits = data_bits;
    if (parity != SPANGPU_ASYNC_PARITY_NONE)
    {
        int p = frame & 0xFF;
        p ^= p >> 4;
        p ^= p >> 2;
        p ^= p >> 1;
        p &= 1;
        if (parity == SPANGPU_ASYNC_PARITY_MARK)
            frame |= 1 << data_bits;
        else if (parity == SPANGPU_ASYNC_PARITY_EVEN)
            frame |= p << data_bits;
        else if (parity == SPANGPU_ASYNC_PARITY_ODD)
            frame |= (p ^ 1) << data_bits;
        total_data_bits++;
    }
    frame |= 0xFFFF << total_data_bits;
    int k = 0;
    out[k++] = 0;
    for (int i = 0;  i < total_data_bits + stop_bits;  i++)
        out[k++] = (uint8_t) ((frame >> i) & 1);
    return k;
}

extern "C" {

// ---- FSK transmitter banks ------------------------------------------------------------------------------------------------

void spangpu_fsktx_destroy(spangpu_fsktx_t *t)
{
    if (t == NULL)
        return;
    common_destroy(&t->c);
    (void) hipFree(t->queue);
    (void) hipFree(t->d_bits);
    (void) hipFree(t->d_blens);
    (void) hipFree(t->d_acc);
    free(t->h_row);
    free(t->frame_par);
    free(t);
}

int spangpu_fsktx_create(spangpu_fsktx_t **out, int device, int n_channels, const spangpu_fsk_spec_t *spec, int bit_source,
                         const uint32_t *seeds, int queue_bits)
{
    if (out == NULL  ||  n_channels <= 0  ||  !spec_ok(spec)
        ||  (bit_source != SPANGPU_FSKTX_LFSR  &&  bit_source != SPANGPU_FSKTX_QUEUE)
        ||  (bit_source == SPANGPU_FSKTX_QUEUE  &&  (queue_bits <= 0  ||  queue_bits > (1 << 24))))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (n_channels > 0, baud_rate 1..800000, a bit source, queue_bits > 0)");
    *out = NULL;
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_fsktx_s *t = (spangpu_fsktx_s *) calloc(1, sizeof(*t));
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    t->source = (bit_source == SPANGPU_FSKTX_LFSR)  ?  FTX_SRC_LFSR  :  FTX_SRC_QUEUE;
    if ((rc = common_create(&t->c, device, n_channels, kFskTxWords)) != SPANGPU_OK)
    {
        spangpu_fsktx_destroy(t);
        return rc;
    }
    t->h_row = (int32_t *) malloc((size_t) n_channels*sizeof(int32_t));
    t->frame_par = (uint8_t *) malloc((size_t) n_channels*3);
    if (t->h_row == NULL  ||  t->frame_par == NULL)
    {
        spangpu_fsktx_destroy(t);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "malloc");
    }
    for (int c = 0;  c < n_channels;  c++)
    {
        t->frame_par[3*c] = 8;
        t->frame_par[3*c + 1] = SPANGPU_ASYNC_PARITY_NONE;
        t->frame_par[3*c + 2] = 1;
    }
    if (t->source == FTX_SRC_QUEUE)
    {
        t->qcap = queue_bits;
        t->qring = (queue_bits + 31) & ~31;
        const size_t bytes = (size_t) (t->qring/32)*n_channels*sizeof(uint32_t);
        if (hipMalloc(&t->queue, bytes) != hipSuccess  ||  hipMemset(t->queue, 0, bytes) != hipSuccess)
        {
            spangpu_fsktx_destroy(t);
            return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the bit rings failed");
        }
    }
    // fsk_tx_init() = memset + fsk_tx_restart(), fsk.c:237-255
    int32_t one[kFskTxWords];
    memset(one, 0, sizeof(one));
    fsk_restart_words(one, spec);
    if ((rc = common_fill(&t->c, one)) != SPANGPU_OK)
    {
        spangpu_fsktx_destroy(t);
        return rc;
    }
    if (t->source == FTX_SRC_LFSR)
    {
        for (int c = 0;  c < n_channels;  c++)
            t->h_row[c] = (int32_t) ((seeds  ?  seeds[c]  :  (uint32_t) (c*2654435761u + 1u)) & 0x7FFFu);
        if (hipMemcpy(t->c.st + (size_t) FT_LFSR*n_channels, t->h_row, (size_t) n_channels*sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
        {
            spangpu_fsktx_destroy(t);
            return spangpu_set_error(SPANGPU_ERR_HIP, "seed upload failed");
        }
    }
    *out = t;
    return SPANGPU_OK;
}

int spangpu_fsktx_channels(const spangpu_fsktx_t *t) { return t  ?  t->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_fsktx_state_words(void) { return kFskTxWords; }

int spangpu_fsktx_set_stream(spangpu_fsktx_t *t, void *stream)
{
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return common_set_stream(&t->c, stream);
}

int spangpu_fsktx_sync(spangpu_fsktx_t *t)
{
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return common_sync(&t->c);
}

int spangpu_fsktx_get_state(spangpu_fsktx_t *t, int channel, int32_t *words)
{
    if (t == NULL  ||  words == NULL  ||  channel < 0  ||  channel >= t->c.n_ch)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return rw_words(&t->c, channel, 0, kFskTxWords, words, false);
}

// fsk_tx_power(), fsk.c:201-204
int spangpu_fsktx_power(spangpu_fsktx_t *t, int channel, float power_dbm0)
{
    if (t == NULL  ||  channel < 0  ||  channel >= t->c.n_ch)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w = scaling_dbm0(power_dbm0);
    return rw_words(&t->c, channel, FT_SCALING, 1, &w, true);
}

int spangpu_fsktx_restart(spangpu_fsktx_t *t, int channel, const spangpu_fsk_spec_t *spec)
{
    if (t == NULL  ||  channel < 0  ||  channel >= t->c.n_ch  ||  !spec_ok(spec))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w[FT_SHUTDOWN + 1];
    fsk_restart_words(w, spec);
    return rw_words(&t->c, channel, 0, FT_SHUTDOWN + 1, w, true);
}

int spangpu_fsktx_end_of_data(spangpu_fsktx_t *t, int channel, int on)
{
    if (t == NULL  ||  channel < 0  ||  channel >= t->c.n_ch  ||  t->source != FTX_SRC_QUEUE)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    int32_t w = on  ?  1  :  0;
    return rw_words(&t->c, channel, FT_EOD, 1, &w, true);
}

int spangpu_fsktx_queued(spangpu_fsktx_t *t, int channel)
{
    if (t == NULL  ||  channel < 0  ||  channel >= t->c.n_ch  ||  t->source != FTX_SRC_QUEUE)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    int32_t w = 0;
    const int rc = rw_words(&t->c, channel, FT_QCOUNT, 1, &w, false);
    return (rc != SPANGPU_OK)  ?  rc  :  w;
}

int spangpu_fsktx_put_bits(spangpu_fsktx_t *t, int first, int n, const uint8_t *bits, int stride, const int32_t *lens, int32_t *accepted)
{
    if (t == NULL  ||  t->source != FTX_SRC_QUEUE  ||  first < 0  ||  n <= 0  ||  first + n > t->c.n_ch  ||  bits == NULL
        ||  lens == NULL  ||  stride <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    for (int i = 0;  i < n;  i++)
    {
        if (lens[i] < 0  ||  (lens[i] + 7)/8 > stride)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a channel's bits do not fit its row");
    }
    FT_TRY(hipSetDevice(t->c.device));
    const size_t bytes = (size_t) n*stride;
    if (bytes > t->bits_cap  ||  n > t->put_cap)
    {
        FT_TRY(hipStreamSynchronize(t->c.stream));
        (void) hipFree(t->d_bits);
        (void) hipFree(t->d_blens);
        (void) hipFree(t->d_acc);
        t->d_bits = NULL;
        t->d_blens = NULL;
        t->d_acc = NULL;
        t->bits_cap = 0;
        t->put_cap = 0;
        const size_t want = (bytes > t->bits_cap)  ?  bytes  :  t->bits_cap;
        if (hipMalloc(&t->d_bits, want) != hipSuccess  ||  hipMalloc(&t->d_blens, (size_t) t->c.n_ch*sizeof(int32_t)) != hipSuccess
            ||  hipMalloc(&t->d_acc, (size_t) t->c.n_ch*sizeof(int32_t)) != hipSuccess)
            return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "bit staging");
        t->bits_cap = want;
        t->put_cap = t->c.n_ch;
    }
    FT_TRY(hipMemcpyAsync(t->d_bits, bits, bytes, hipMemcpyHostToDevice, t->c.stream));
    FT_TRY(hipMemcpyAsync(t->d_blens, lens, (size_t) n*sizeof(int32_t), hipMemcpyHostToDevice, t->c.stream));
    hipLaunchKernelGGL(fsktx_put_kernel, dim3((n + 63)/64), dim3(64), 0, t->c.stream, t->c.st, t->queue, t->c.n_ch, t->qring, t->qcap,
                       first, first + n, t->d_bits, stride, t->d_blens, t->d_acc);
    FT_TRY(hipGetLastError());
    if (accepted)
        FT_TRY(hipMemcpyAsync(accepted, t->d_acc, (size_t) n*sizeof(int32_t), hipMemcpyDeviceToHost, t->c.stream));
    // the caller's arrays are pageable: they must not change under the copies
    FT_TRY(hipStreamSynchronize(t->c.stream));
    return SPANGPU_OK;
}

int spangpu_fsktx_set_framing(spangpu_fsktx_t *t, int channel, int data_bits, int parity, int stop_bits)
{
    if (t == NULL  ||  channel < -1  ||  channel >= t->c.n_ch  ||  !framing_ok(data_bits, parity, stop_bits))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (data bits 5..8, parity SPANGPU_ASYNC_PARITY_*, stop bits 1..2)");
    for (int c = (channel < 0)  ?  0  :  channel;  c < ((channel < 0)  ?  t->c.n_ch  :  channel + 1);  c++)
    {
        t->frame_par[3*c] = (uint8_t) data_bits;
        t->frame_par[3*c + 1] = (uint8_t) parity;
        t->frame_par[3*c + 2] = (uint8_t) stop_bits;
    }
    return SPANGPU_OK;
}

int spangpu_fsktx_put_bytes(spangpu_fsktx_t *t, int first, int n, const uint8_t *bytes, int stride, const int32_t *lens,
                            int presend_bits, int32_t *accepted)
{
    if (t == NULL  ||  t->source != FTX_SRC_QUEUE  ||  first < 0  ||  n <= 0  ||  first + n > t->c.n_ch  ||  bytes == NULL
        ||  lens == NULL  ||  stride <= 0  ||  presend_bits < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    int most = 0;
    for (int i = 0;  i < n;  i++)
    {
        if (lens[i] < 0  ||  lens[i] > stride)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a channel's bytes do not fit its row");
        most = (lens[i] > most)  ?  lens[i]  :  most;
    }
    // how much room each ring has: whole characters only
    FT_TRY(hipSetDevice(t->c.device));
    FT_TRY(hipMemcpyAsync(t->h_row, t->c.st + (size_t) FT_QCOUNT*t->c.n_ch + first, (size_t) n*sizeof(int32_t), hipMemcpyDeviceToHost,
                          t->c.stream));
    FT_TRY(hipStreamSynchronize(t->c.stream));
    const int row = (presend_bits + most*12 + 7)/8 + 1;
    uint8_t *packed = (uint8_t *) calloc((size_t) n, (size_t) row);
    int32_t *blens = (int32_t *) malloc((size_t) n*sizeof(int32_t));
    if (packed == NULL  ||  blens == NULL)
    {
        free(packed);
        free(blens);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "malloc");
    }
    for (int i = 0;  i < n;  i++)
    {
        const uint8_t *par = t->frame_par + 3*(first + i);
        uint8_t *dst = packed + (size_t) i*row;
        int room = t->qcap - t->h_row[i];
        int at = (presend_bits < room)  ?  presend_bits  :  room;       // async_tx_presend_bits(): marks first
        for (int k = 0;  k < at;  k++)
            dst[k >> 3] |= (uint8_t) (1 << (k & 7));
        room -= at;
        int took = 0;
        const int per = 1 + par[0] + ((par[1] != SPANGPU_ASYNC_PARITY_NONE)  ?  1  :  0) + par[2];
        while (took < lens[i]  &&  room >= per)
        {
            uint8_t one[16];
            const int m = frame_one(par[0], par[1], par[2], bytes[(size_t) i*stride + took], one);
            for (int k = 0;  k < m;  k++)
                dst[(at + k) >> 3] |= (uint8_t) (one[k] << ((at + k) & 7));
            at += m;
            room -= m;
            took++;
        }
        blens[i] = at;
        if (accepted)
            accepted[i] = took;
    }
    const int rc = spangpu_fsktx_put_bits(t, first, n, packed, row, blens, NULL);
    free(packed);
    free(blens);
    return rc;
}

int spangpu_fsktx_tx(spangpu_fsktx_t *t, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    int rc = tx_args_ok(t, mem_kind, pcm, stride, samples);
    if (rc != SPANGPU_OK)
        return rc;
    if (samples == 0)
    {
        if (lens  &&  mem_kind == SPANGPU_MEM_HOST)
            memset(lens, 0, (size_t) t->c.n_ch*sizeof(int32_t));
        return SPANGPU_OK;
    }
    FT_TRY(hipSetDevice(t->c.device));
    FskTxLaunch L;
    memset(&L, 0, sizeof(L));
    if ((rc = frame_target(&t->c, mem_kind, pcm, stride, samples, lens, &L.pcm, &L.stride, &L.lens, &L.vec)) != SPANGPU_OK)
        return rc;
    L.st = t->c.st;
    L.quarter = t->c.quarter;
    L.queue = t->queue;
    L.n_ch = t->c.n_ch;
    L.samples = samples;
    L.source = t->source;
    L.qring = t->qring;
    // 16 channels per wave, four waves per workgroup, as the other sender banks (txgen_api.hip)
    hipLaunchKernelGGL(fsktx_bank_kernel, dim3((t->c.n_ch + kFtxCpw*kFtxWaves - 1)/(kFtxCpw*kFtxWaves)), dim3(64*kFtxWaves), 0,
                       t->c.stream, L);
    FT_TRY(hipGetLastError());
    return frame_back(&t->c, mem_kind, pcm, stride, samples, lens);
}

int spangpu_fsktx_events(spangpu_fsktx_t *t, const int32_t **channels)
{
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    FT_TRY(hipSetDevice(t->c.device));
    FT_TRY(hipMemcpyAsync(t->h_row, t->c.st + (size_t) FT_EVENT*t->c.n_ch, (size_t) t->c.n_ch*sizeof(int32_t), hipMemcpyDeviceToHost,
                          t->c.stream));
    FT_TRY(hipStreamSynchronize(t->c.stream));
    int count = 0;
    for (int c = 0;  c < t->c.n_ch;  c++)
    {
        if (t->h_row[c])
            t->h_row[count++] = c;
    }
    if (channels)
        *channels = t->h_row;
    return count;
}

// ---- modem connect tone transmitter banks ---------------------------------------------------------------------------------

void spangpu_mcttx_destroy(spangpu_mcttx_t *t)
{
    if (t == NULL)
        return;
    common_destroy(&t->c);
    free(t);
}

int spangpu_mcttx_create(spangpu_mcttx_t **out, int device, int tone_type, int n_channels)
{
    if (out == NULL  ||  n_channels <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    // modem_connect_tones_tx_init(), modem_connect_tones.c:302-403; milliseconds_to_samples(t) = t*8
    MctTxLaunch P;
    memset(&P, 0, sizeof(P));
    int32_t init[kMctTxWords] = {0, 0, 0, 0};
    switch (tone_type)
    {
    case SPANGPU_MCT_FAX_CNG:
        P.cadenced = 1;
        P.tone_rate = phase_rate(1100.0f);
        P.level = scaling_dbm0(-11);
        P.tone_len = 3000*8;
        P.period = (500 + 3000)*8;
        init[MTX_TIMER] = P.period;
        break;
    case SPANGPU_MCT_CALLING_TONE:
        P.cadenced = 1;
        P.tone_rate = phase_rate(1300.0f);
        P.level = scaling_dbm0(-11);
        P.tone_len = 2000*8;
        P.period = (600 + 2000)*8;
        init[MTX_TIMER] = P.period;
        break;
    case SPANGPU_MCT_ANS:
    case SPANGPU_MCT_BELL_ANS:
        P.tone_rate = phase_rate((tone_type == SPANGPU_MCT_ANS)  ?  2100.0f  :  2225.0f);
        P.level = scaling_dbm0(-11);
        P.tone_len = 2600*8;
        init[MTX_TIMER] = (200 + 2600)*8;
        break;
    case SPANGPU_MCT_ANSAM:
        P.am = 1;
        P.tone_rate = phase_rate(2100.0f);
        P.level = scaling_dbm0(-11);
        P.mod_rate = phase_rate(15.0f);
        P.mod_level = P.level/5;
        P.tone_len = 5000*8;
        init[MTX_TIMER] = (200 + 5000)*8;
        break;
    case SPANGPU_MCT_ANS_PR:
        P.hops = 1;
        P.tone_rate = phase_rate(2100.0f);
        P.level = scaling_dbm0(-12);
        P.tone_len = 3300*8;
        init[MTX_TIMER] = (200 + 3300)*8;
        init[MTX_HOP] = kMtxHop;
        break;
    case SPANGPU_MCT_ANSAM_PR:
        P.hops = 1;
        P.am = 1;
        P.tone_rate = phase_rate(2100.0f);
        P.level = scaling_dbm0(-12);
        P.mod_rate = phase_rate(15.0f);
        P.mod_level = P.level/5;
        P.tone_len = 5000*8;
        init[MTX_TIMER] = (200 + 5000)*8;
        init[MTX_HOP] = kMtxHop;
        break;
    default:
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "no sender for this tone type (FAX CNG, ANS, ANS/PR, ANSam, ANSam/PR, Bell ANS, calling tone)");
    }
    *out = NULL;
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_mcttx_s *t = (spangpu_mcttx_s *) calloc(1, sizeof(*t));
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    t->tone_type = tone_type;
    t->proto = P;
    memcpy(t->init, init, sizeof(init));
    if ((rc = common_create(&t->c, device, n_channels, kMctTxWords)) != SPANGPU_OK  ||  (rc = common_fill(&t->c, init)) != SPANGPU_OK)
    {
        spangpu_mcttx_destroy(t);
        return rc;
    }
    *out = t;
    return SPANGPU_OK;
}

int spangpu_mcttx_channels(const spangpu_mcttx_t *t) { return t  ?  t->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_mcttx_state_words(void) { return kMctTxWords; }

int spangpu_mcttx_set_stream(spangpu_mcttx_t *t, void *stream)
{
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return common_set_stream(&t->c, stream);
}

int spangpu_mcttx_sync(spangpu_mcttx_t *t)
{
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return common_sync(&t->c);
}

int spangpu_mcttx_get_state(spangpu_mcttx_t *t, int channel, int32_t *words)
{
    if (t == NULL  ||  words == NULL  ||  channel < 0  ||  channel >= t->c.n_ch)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return rw_words(&t->c, channel, 0, kMctTxWords, words, false);
}

int spangpu_mcttx_restart(spangpu_mcttx_t *t, int channel)
{
    if (t == NULL  ||  channel < 0  ||  channel >= t->c.n_ch)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return rw_words(&t->c, channel, 0, kMctTxWords, t->init, true);
}

int spangpu_mcttx_tx(spangpu_mcttx_t *t, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    int rc = tx_args_ok(t, mem_kind, pcm, stride, samples);
    if (rc != SPANGPU_OK)
        return rc;
    if (samples == 0)
    {
        if (lens  &&  mem_kind == SPANGPU_MEM_HOST)
            memset(lens, 0, (size_t) t->c.n_ch*sizeof(int32_t));
        return SPANGPU_OK;
    }
    FT_TRY(hipSetDevice(t->c.device));
    MctTxLaunch L = t->proto;
    if ((rc = frame_target(&t->c, mem_kind, pcm, stride, samples, lens, &L.pcm, &L.stride, &L.lens, &L.vec)) != SPANGPU_OK)
        return rc;
    L.st = t->c.st;
    L.quarter = t->c.quarter;
    L.n_ch = t->c.n_ch;
    L.samples = samples;
    hipLaunchKernelGGL(mcttx_bank_kernel, dim3((t->c.n_ch + kFtxCpw*kFtxWaves - 1)/(kFtxCpw*kFtxWaves)), dim3(64*kFtxWaves), 0,
                       t->c.stream, L);
    FT_TRY(hipGetLastError());
    return frame_back(&t->c, mem_kind, pcm, stride, samples, lens);
}

// ---- host helpers: async_tx framing and the bit clock, no device needed ---------------------------------------------------

// The bits async_tx_get_bit() (async.c:277-338) hands out for these bytes, one 0/1 per entry of bits_out.  Returns how
// many there are; at most `max` of them are written.
int spangpu_async_frame_bits(int data_bits, int parity, int stop_bits, const uint8_t *bytes, int n, uint8_t *bits_out, int max)
{
    if (!framing_ok(data_bits, parity, stop_bits)  ||  n < 0  ||  (n > 0  &&  bytes == NULL)  ||  (max > 0  &&  bits_out == NULL))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (data bits 5..8, parity SPANGPU_ASYNC_PARITY_*, stop bits 1..2)");
    int total = 0;
    for (int i = 0;  i < n;  i++)
    {
        uint8_t one[16];
        const int m = frame_one(data_bits, parity, stop_bits, bytes[i], one);
        for (int k = 0;  k < m;  k++, total++)
        {
            if (total < max)
                bits_out[total] = one[k];
        }
    }
    return total;
}

// How many get_bit calls fsk_tx() makes in a call of `samples` from this baud_frac: one for each time
// (baud_frac += baud_rate) >= 800000 (fsk.c:176).
long long spangpu_fsktx_bits_due(int baud_rate, int baud_frac, int samples)
{
    if (baud_rate <= 0  ||  baud_rate > kFtxBaudUnit  ||  baud_frac < 0  ||  baud_frac >= kFtxBaudUnit  ||  samples < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return ((long long) baud_frac + (long long) samples*baud_rate)/kFtxBaudUnit;
}

}   // extern "C"
