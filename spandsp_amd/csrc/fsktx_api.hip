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
#define SPG_HDLC_STEP_FUNCTIONS_ONLY        // the HDLC banks' own kernels belong to hdlc_api.hip
#include "modem_tables.h"
#include "fsktx_dev.hpp"
#include "bank_host.hpp"

using namespace spg;

struct spangpu_fsktx_s
{
    BankCore c;
    PcmStage pcm;
    int16_t *quarter;
    int source;
    int qcap;               // bits a channel's ring takes
    int qring;              // ring size in bits: qcap rounded up to whole words
    uint32_t *queue;
    int32_t *h_row;         // [n_ch] host scratch: a row of state words, the list of events
    uint8_t *frame_par;     // [n_ch][3]: data bits, parity, stop bits of spangpu_fsktx_put_bytes()
    BitPut put;
};

struct spangpu_mcttx_s
{
    BankCore c;
    PcmStage pcm;
    int16_t *quarter;
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

// the state, the quarter sine and the lengths of a host caller: the same in both banks
static int sender_create(BankCore *c, PcmStage *pcm, int16_t **quarter, int device, int n_channels, int words)
{
    int rc;
    if ((rc = core_create(c, device, n_channels, words)) != SPANGPU_OK  ||  (rc = quarter_sine_upload(quarter)) != SPANGPU_OK)
        return rc;
    return stage_lens(c, pcm);
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
    core_destroy(&t->c);
    stage_free(&t->pcm);
    bitput_free(&t->put);
    (void) hipFree(t->quarter);
    (void) hipFree(t->queue);
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
    if ((rc = sender_create(&t->c, &t->pcm, &t->quarter, device, n_channels, kFskTxWords)) != SPANGPU_OK)
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
    if ((rc = core_fill(&t->c, one)) != SPANGPU_OK)
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
    return core_set_stream(&t->c, stream);
}

int spangpu_fsktx_sync(spangpu_fsktx_t *t)
{
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&t->c);
}

int spangpu_fsktx_get_state(spangpu_fsktx_t *t, int channel, int32_t *words)
{
    if (t == NULL  ||  words == NULL  ||  !channel_ok(&t->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&t->c, channel, 0, kFskTxWords, words, false);
}

// fsk_tx_power(), fsk.c:201-204
int spangpu_fsktx_power(spangpu_fsktx_t *t, int channel, float power_dbm0)
{
    if (t == NULL  ||  !channel_ok(&t->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w = scaling_dbm0(power_dbm0);
    return core_rw_words(&t->c, channel, FT_SCALING, 1, &w, true);
}

int spangpu_fsktx_restart(spangpu_fsktx_t *t, int channel, const spangpu_fsk_spec_t *spec)
{
    if (t == NULL  ||  !channel_ok(&t->c, channel)  ||  !spec_ok(spec))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w[FT_SHUTDOWN + 1];
    fsk_restart_words(w, spec);
    return core_rw_words(&t->c, channel, 0, FT_SHUTDOWN + 1, w, true);
}

int spangpu_fsktx_end_of_data(spangpu_fsktx_t *t, int channel, int on)
{
    if (t == NULL  ||  !channel_ok(&t->c, channel)  ||  t->source != FTX_SRC_QUEUE)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    int32_t w = on  ?  1  :  0;
    return core_rw_words(&t->c, channel, FT_EOD, 1, &w, true);
}

int spangpu_fsktx_queued(spangpu_fsktx_t *t, int channel)
{
    if (t == NULL  ||  !channel_ok(&t->c, channel)  ||  t->source != FTX_SRC_QUEUE)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    int32_t w = 0;
    const int rc = core_rw_words(&t->c, channel, FT_QCOUNT, 1, &w, false);
    return (rc != SPANGPU_OK)  ?  rc  :  w;
}

int spangpu_fsktx_put_bits(spangpu_fsktx_t *t, int first, int n, const uint8_t *bits, int stride, const int32_t *lens, int32_t *accepted)
{
    if (t == NULL  ||  t->source != FTX_SRC_QUEUE)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    return bitring_put(&t->c, &t->put, t->c.st + (size_t) FT_QRD*t->c.n_ch, t->c.st + (size_t) FT_QCOUNT*t->c.n_ch, t->queue, t->qring,
                       t->qcap, first, n, bits, stride, lens, accepted);
}

// spangpu_fsktx_put_bits() from rows and lengths in device memory (another bank's output): no copy, no wait
int spangpu_bits_to_fsktx(spangpu_fsktx_t *t, int first, int n, const uint8_t *dev_bits, int stride, const int32_t *dev_lens,
                                  int32_t *dev_accepted)
{
    if (t == NULL  ||  t->source != FTX_SRC_QUEUE)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a bank with the bit queue as its source)");
    return bitring_put_device(&t->c, &t->put, t->c.st + (size_t) FT_QRD*t->c.n_ch, t->c.st + (size_t) FT_QCOUNT*t->c.n_ch, t->queue, t->qring,
                              t->qcap, first, n, dev_bits, stride, dev_lens, dev_accepted);
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
    SPG_TRY(hipSetDevice(t->c.device));
    SPG_TRY(hipMemcpyAsync(t->h_row, t->c.st + (size_t) FT_QCOUNT*t->c.n_ch + first, (size_t) n*sizeof(int32_t), hipMemcpyDeviceToHost,
                          t->c.stream));
    SPG_TRY(hipStreamSynchronize(t->c.stream));
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
        // (an empty call zeroes a host caller's lens; the tone sender leaves them)
        if (lens  &&  mem_kind == SPANGPU_MEM_HOST)
            memset(lens, 0, (size_t) t->c.n_ch*sizeof(int32_t));
        return SPANGPU_OK;
    }
    SPG_TRY(hipSetDevice(t->c.device));
    FskTxLaunch L;
    memset(&L, 0, sizeof(L));
    if ((rc = stage_out_target(&t->c, &t->pcm, mem_kind, pcm, stride, samples, lens, &L.pcm, &L.stride, &L.lens, &L.vec)) != SPANGPU_OK)
        return rc;
    L.st = t->c.st;
    L.quarter = t->quarter;
    L.queue = t->queue;
    L.n_ch = t->c.n_ch;
    L.samples = samples;
    L.source = t->source;
    L.qring = t->qring;
    // 16 channels per wave, four waves per workgroup, as the other sender banks (txgen_api.hip)
    hipLaunchKernelGGL(fsktx_bank_kernel, dim3((t->c.n_ch + kFtxCpw*kFtxWaves - 1)/(kFtxCpw*kFtxWaves)), dim3(64*kFtxWaves), 0,
                       t->c.stream, L);
    SPG_TRY(hipGetLastError());
    return stage_out_back(&t->c, &t->pcm, mem_kind, pcm, stride, samples, lens);
}

// (what the HDLC sender bank's unit hands to the units whose kernels call hdlc_tx_get_bit() themselves; not part of the ABI)
extern "C" void spangpu_hdlc_tx_rows(spangpu_hdlc_tx_t *b, int32_t **st, uint32_t **buf, int32_t **q_hdr, uint32_t **q_data, int *depth);

// One fsk_tx() call per channel over its own span of the row (txspan_dev.hpp), its get_bit the framer's hdlc_tx_get_bit();
// everything in device memory, nothing waited for.
int spangpu_txspans_fsk(spangpu_fsktx_t *t, int16_t *pcm, long long stride, int samples, const int32_t *spans, int sender,
                               int32_t *ret, spangpu_hdlc_tx_t *framer, int32_t *counts)
{
    int rc = tx_args_ok(t, SPANGPU_MEM_DEVICE, pcm, stride, samples);
    if (rc != SPANGPU_OK)
        return rc;
    if (spans == NULL  ||  ret == NULL  ||  framer == NULL  ||  counts == NULL  ||  spangpu_hdlc_tx_channels(framer) != t->c.n_ch)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a framer of as many channels)");
    if (samples == 0)
        return SPANGPU_OK;
    SPG_TRY(hipSetDevice(t->c.device));
    FskTxLaunch L;
    memset(&L, 0, sizeof(L));
    L.st = t->c.st;
    L.quarter = t->quarter;
    L.pcm = pcm;
    L.stride = stride;
    L.n_ch = t->c.n_ch;
    L.samples = samples;
    L.sp.span = spans;
    L.sp.id = sender;
    L.sp.ret = ret;
    uint32_t *q_data;
    spangpu_hdlc_tx_rows(framer, &L.sp.hst, &L.sp.hbuf, &L.sp.q_hdr, &q_data, &L.sp.depth);
    L.sp.q_data = q_data;
    L.sp.cnt = counts;
    hipLaunchKernelGGL(fsktx_span_kernel, dim3((t->c.n_ch + kFtxCpw*kFtxWaves - 1)/(kFtxCpw*kFtxWaves)), dim3(64*kFtxWaves), 0,
                       t->c.stream, L);
    SPG_TRY(hipGetLastError());
    return SPANGPU_OK;
}

int spangpu_txline_fsk_set_state(spangpu_fsktx_t *t, int channel, const int32_t *words)
{
    if (t == NULL  ||  words == NULL  ||  !channel_ok(&t->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    // (the walk divides by the baud rate and steps baud_frac up to 800000; the ring position indexes the ring)
    if (words[FT_BAUD_RATE] <= 0  ||  words[FT_BAUD_RATE] > kFtxBaudUnit  ||  words[FT_BAUD_FRAC] < 0  ||  words[FT_BAUD_FRAC] >= kFtxBaudUnit
        ||  words[FT_QRD] < 0  ||  words[FT_QRD] >= ((t->qring > 0)  ?  t->qring  :  1)  ||  words[FT_QCOUNT] < 0  ||  words[FT_QCOUNT] > t->qcap)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "not the words of a channel of this bank");
    return core_rw_words(&t->c, channel, 0, kFskTxWords, const_cast<int32_t *>(words), true);
}

int spangpu_fsktx_events(spangpu_fsktx_t *t, const int32_t **channels)
{
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    SPG_TRY(hipSetDevice(t->c.device));
    SPG_TRY(hipMemcpyAsync(t->h_row, t->c.st + (size_t) FT_EVENT*t->c.n_ch, (size_t) t->c.n_ch*sizeof(int32_t), hipMemcpyDeviceToHost,
                          t->c.stream));
    SPG_TRY(hipStreamSynchronize(t->c.stream));
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
    core_destroy(&t->c);
    stage_free(&t->pcm);
    (void) hipFree(t->quarter);
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
    if ((rc = sender_create(&t->c, &t->pcm, &t->quarter, device, n_channels, kMctTxWords)) != SPANGPU_OK
        ||  (rc = core_fill(&t->c, init)) != SPANGPU_OK)
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
    return core_set_stream(&t->c, stream);
}

int spangpu_mcttx_sync(spangpu_mcttx_t *t)
{
    if (t == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&t->c);
}

int spangpu_mcttx_get_state(spangpu_mcttx_t *t, int channel, int32_t *words)
{
    if (t == NULL  ||  words == NULL  ||  !channel_ok(&t->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&t->c, channel, 0, kMctTxWords, words, false);
}

int spangpu_mcttx_restart(spangpu_mcttx_t *t, int channel)
{
    if (t == NULL  ||  !channel_ok(&t->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&t->c, channel, 0, kMctTxWords, t->init, true);
}

int spangpu_mcttx_tx(spangpu_mcttx_t *t, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    int rc = tx_args_ok(t, mem_kind, pcm, stride, samples);
    if (rc != SPANGPU_OK)
        return rc;
    if (samples == 0)
    {
        // (an empty call zeroes a host caller's lens; the tone sender leaves them)
        if (lens  &&  mem_kind == SPANGPU_MEM_HOST)
            memset(lens, 0, (size_t) t->c.n_ch*sizeof(int32_t));
        return SPANGPU_OK;
    }
    SPG_TRY(hipSetDevice(t->c.device));
    MctTxLaunch L = t->proto;
    if ((rc = stage_out_target(&t->c, &t->pcm, mem_kind, pcm, stride, samples, lens, &L.pcm, &L.stride, &L.lens, &L.vec)) != SPANGPU_OK)
        return rc;
    L.st = t->c.st;
    L.quarter = t->quarter;
    L.n_ch = t->c.n_ch;
    L.samples = samples;
    hipLaunchKernelGGL(mcttx_bank_kernel, dim3((t->c.n_ch + kFtxCpw*kFtxWaves - 1)/(kFtxCpw*kFtxWaves)), dim3(64*kFtxWaves), 0,
                       t->c.stream, L);
    SPG_TRY(hipGetLastError());
    return stage_out_back(&t->c, &t->pcm, mem_kind, pcm, stride, samples, lens);
}

// modem_connect_tones_tx() once per channel over its own span of the row (txspan_dev.hpp)
int spangpu_txspans_mct(spangpu_mcttx_t *t, int16_t *pcm, long long stride, int samples, const int32_t *spans, int sender, int32_t *ret)
{
    int rc = tx_args_ok(t, SPANGPU_MEM_DEVICE, pcm, stride, samples);
    if (rc != SPANGPU_OK)
        return rc;
    if (spans == NULL  ||  ret == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (samples == 0)
        return SPANGPU_OK;
    SPG_TRY(hipSetDevice(t->c.device));
    MctTxLaunch L = t->proto;
    L.st = t->c.st;
    L.quarter = t->quarter;
    L.pcm = pcm;
    L.stride = stride;
    L.n_ch = t->c.n_ch;
    L.samples = samples;
    L.sp.span = spans;
    L.sp.id = sender;
    L.sp.ret = ret;
    hipLaunchKernelGGL(mcttx_span_kernel, dim3((t->c.n_ch + kFtxCpw*kFtxWaves - 1)/(kFtxCpw*kFtxWaves)), dim3(64*kFtxWaves), 0,
                       t->c.stream, L);
    SPG_TRY(hipGetLastError());
    return SPANGPU_OK;
}

int spangpu_txline_mct_set_state(spangpu_mcttx_t *t, int channel, const int32_t *words)
{
    if (t == NULL  ||  words == NULL  ||  !channel_ok(&t->c, channel)  ||  words[MTX_TIMER] < 0  ||  words[MTX_HOP] < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&t->c, channel, 0, kMctTxWords, const_cast<int32_t *>(words), true);
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
