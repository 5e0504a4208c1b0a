// hdlc_api.hip -- C ABI of the HDLC framing banks (include/spangpu.h, "HDLC framing banks"): batched hdlc_rx_put_bit() /
// hdlc_rx_put() over the event rows a receiver bank keeps on the device, and hdlc_tx_get_bit() into the bit rows a sender
// bank's ring takes.  Device code: hdlc_dev.hpp.  No CPU implementation exists behind these entry points; the control-plane
// calls (max frame length, report interval, restart, state, buffer) edit one channel's words on the host, as the reference's
// own functions edit one object.

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#include "bank_host.hpp"
#include "hdlc_dev.hpp"

using namespace spg;

struct spangpu_hdlc_rx_s
{
    BankCore c;
    uint32_t *buf;              // [101][n_ch]
    uint8_t *d_events;          // a host caller's rows
    size_t events_cap;
    int32_t *d_counts;          // [n_ch]: a host caller's counts
    int32_t *recs;              // [n_ch][rec_cap]
    int32_t *h_recs;            // pinned
    int rec_room;
    uint8_t *bytes;             // [n_ch][byte_cap]
    uint8_t *h_bytes;           // pinned
    int byte_room;
    CountRows counts;           // [2][n_ch]: records, then octets
    int rec_cap;                // of the last call; 0: none yet
    int byte_cap;
};

struct spangpu_hdlc_tx_s
{
    BankCore c;
    uint32_t *buf;              // [101][n_ch]
    int depth;
    int32_t *q_hdr;             // [n_ch][depth]
    uint32_t *q_data;           // [n_ch][depth][101]
    uint8_t *d_frames;          // commands of a host caller
    size_t frames_cap;
    int32_t *d_cmd;             // [3][n_ch]: lens, flags, results
    int32_t *h_cmd;             // pinned
    uint8_t *d_bits;            // a host caller's rows
    size_t bits_cap;
    int32_t *d_want;            // [n_ch]
    int32_t *out;               // [3][n_ch]: lens, ended, underflows
    int32_t *h_out;             // pinned
    int32_t *ev_channels;       // [2*n_ch]
    int32_t *ev_kinds;
    bool ran;
};

// one word of every channel, or of one
static int row_rw(BankCore *c, int word, int channel, int32_t *host, bool write)
{
    if (channel >= 0)
        return core_rw_words(c, channel, word, 1, host, write);
    SPG_TRY(hipSetDevice(c->device));
    int32_t *at = c->st + (size_t) word*c->n_ch;
    const size_t bytes = (size_t) c->n_ch*sizeof(int32_t);
    if (write)
        SPG_TRY(hipMemcpyAsync(at, host, bytes, hipMemcpyHostToDevice, c->stream));
    else
        SPG_TRY(hipMemcpyAsync(host, at, bytes, hipMemcpyDeviceToHost, c->stream));
    SPG_TRY(hipStreamSynchronize(c->stream));
    return SPANGPU_OK;
}

static int buffer_rw(BankCore *c, uint32_t *buf, int channel, uint8_t *bytes, bool write)
{
    int32_t w[kHdlcBufWords];
    if (write)
        memcpy(w, bytes, kHdlcBuf);
    const int rc = core_rw_at(c, reinterpret_cast<int32_t *>(buf), channel, 0, kHdlcBufWords, w, write);
    if (rc == SPANGPU_OK  &&  !write)
        memcpy(bytes, w, kHdlcBuf);
    return rc;
}

// a receiver bank's words and frame buffers, where they lie on the device, for a bank family that frames on the device inside
// a kernel of its own (faxfe_api.hip); not part of the ABI
extern "C" __attribute__((visibility("hidden"))) void spangpu_framer_rows(spangpu_hdlc_rx_t *b, int32_t **st, uint32_t **buf)
{
    *st = b->c.st;
    *buf = b->buf;
}

// the same of a sender bank, for the sender kernels that call hdlc_tx_get_bit() themselves (txspan_dev.hpp)
extern "C" __attribute__((visibility("hidden"))) void spangpu_hdlc_tx_rows(spangpu_hdlc_tx_t *b, int32_t **st, uint32_t **buf, int32_t **q_hdr,
                                                                           uint32_t **q_data, int *depth)
{
    *st = b->c.st;
    *buf = b->buf;
    *q_hdr = b->q_hdr;
    *q_data = b->q_data;
    *depth = b->depth;
}

extern "C" {

/*
 * Entry point                                  stands for (paths relative to the reference tree)
 *   spangpu_hdlc_rx_create()                   hdlc_rx_init(NULL, crc32, report_bad_frames, threshold, ..) x N   src/hdlc.c:373-396
 *   spangpu_hdlc_rx_put_events()               hdlc_rx_put_bit(s, event) over each channel's row                 src/hdlc.c:303-314
 *   spangpu_hdlc_rx_put()                      hdlc_rx_put(s, buf, len) x N                                      src/hdlc.c:316-344
 *   spangpu_hdlc_rx_records()                  the frame_handler / status_handler calls of the last put
 *   spangpu_hdlc_rx_set_max_frame_len()        hdlc_rx_set_max_frame_len()                                       src/hdlc.c:346-351
 *   spangpu_hdlc_rx_set_octet_counting_report_interval()   the call of that name                                 src/hdlc.c:353-357
 *   spangpu_hdlc_rx_restart()                  hdlc_rx_restart()                                                 src/hdlc.c:359-371
 *   spangpu_hdlc_rx_get_stats()                hdlc_rx_get_stats()                                               src/hdlc.c:425-435
 *   spangpu_hdlc_tx_create()                   hdlc_tx_init(NULL, crc32, inter_frame_flags, false, pop, fifo) x N  src/hdlc.c:704-738
 *   spangpu_hdlc_tx_frames() / _flags() / _abort() / _end()   hdlc_tx_frame() (+ hdlc_tx_corrupt_frame()), hdlc_tx_flags(),
 *                                              hdlc_tx_abort(), hdlc_tx_frame(s, NULL, 0), queued            src/hdlc.c:437-519
 *   spangpu_hdlc_tx_get_bits()                 hdlc_tx_get_bit(s) x want[c] x N                                  src/hdlc.c:521-657
 *   spangpu_hdlc_tx_set_max_frame_len() / _restart()   the calls of those names                                  src/hdlc.c:676-702
 */

// ---- receivers --------------------------------------------------------------------------------------------------------

void spangpu_hdlc_rx_destroy(spangpu_hdlc_rx_t *b)
{
    if (b == NULL)
        return;
    core_destroy(&b->c);
    (void) hipFree(b->buf);
    (void) hipFree(b->d_events);
    (void) hipFree(b->d_counts);
    (void) hipFree(b->recs);
    (void) hipFree(b->bytes);
    counts_free(&b->counts);
    if (b->h_recs)
        (void) hipHostFree(b->h_recs);
    if (b->h_bytes)
        (void) hipHostFree(b->h_bytes);
    free(b);
}

int spangpu_hdlc_rx_create(spangpu_hdlc_rx_t **out, int device, int n_channels, int crc32, int report_bad_frames, int framing_ok_threshold)
{
    if (out == NULL  ||  n_channels <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    *out = NULL;
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_hdlc_rx_s *b = (spangpu_hdlc_rx_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    if ((rc = core_create(&b->c, device, n_channels, kHdlcRxWords)) != SPANGPU_OK)
    {
        spangpu_hdlc_rx_destroy(b);
        return rc;
    }
    const size_t n = (size_t) n_channels;
    if (hipMalloc(&b->buf, n*kHdlcBufWords*sizeof(uint32_t)) != hipSuccess  ||  hipMalloc(&b->d_counts, n*sizeof(int32_t)) != hipSuccess
        ||  counts_create(&b->c, &b->counts, 2, 2) != SPANGPU_OK)
    {
        spangpu_hdlc_rx_destroy(b);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the HDLC receiver bank failed");
    }
    int32_t one[kHdlcRxWords];
    hdlc_rx_words_init(one, crc32, report_bad_frames, framing_ok_threshold);
    rc = core_fill(&b->c, one);
    if (rc == SPANGPU_OK  &&  hipMemset(b->buf, 0, n*kHdlcBufWords*sizeof(uint32_t)) != hipSuccess)
        rc = spangpu_set_error(SPANGPU_ERR_HIP, "state upload failed");
    if (rc != SPANGPU_OK)
    {
        spangpu_hdlc_rx_destroy(b);
        return rc;
    }
    *out = b;
    return SPANGPU_OK;
}

int spangpu_hdlc_rx_channels(const spangpu_hdlc_rx_t *b) { return b  ?  b->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_hdlc_rx_state_words(const spangpu_hdlc_rx_t *b) { return b  ?  b->c.words  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_hdlc_rx_set_stream(spangpu_hdlc_rx_t *b, void *stream)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&b->c, stream);
}

int spangpu_hdlc_rx_sync(spangpu_hdlc_rx_t *b)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&b->c);
}

// (the derivation is beside hdlc_rx_capacity(), hdlc_dev.hpp)
int spangpu_hdlc_rx_capacity(long long events, int *rec_cap, int *byte_cap)
{
    if (events < 0  ||  events > kMaxSamples  ||  rec_cap == NULL  ||  byte_cap == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    long long r;
    long long y;
    hdlc_rx_capacity(events, &r, &y);
    *rec_cap = (int) r;
    *byte_cap = (int) y;
    return SPANGPU_OK;
}

// elem_bytes 1 or 2: events; 0: octets (8 bit events each)
static int rx_launch(spangpu_hdlc_rx_s *b, int mem_kind, const void *rows, int elem_bytes, long long cap, const int32_t *counts)
{
    const int esz = elem_bytes  ?  elem_bytes  :  1;
    if (b == NULL  ||  rows == NULL  ||  cap <= 0  ||  cap*(elem_bytes  ?  1  :  8) > kMaxSamples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int rc = mem_kind_ok(mem_kind);
    if (rc != SPANGPU_OK)
        return rc;
    SPG_TRY(hipSetDevice(b->c.device));
    const size_t n = (size_t) b->c.n_ch;
    int rec_cap;
    int byte_cap;
    (void) spangpu_hdlc_rx_capacity(cap*(elem_bytes  ?  1  :  8), &rec_cap, &byte_cap);
    if ((rc = grow_pair(&b->recs, &b->h_recs, &b->rec_room, rec_cap, n, b->c.stream)) != SPANGPU_OK
        ||  (rc = grow_pair(&b->bytes, &b->h_bytes, &b->byte_room, byte_cap, n, b->c.stream)) != SPANGPU_OK)
        return rc;
    HdlcRxLaunch L;
    memset(&L, 0, sizeof(L));
    L.events = rows;
    L.counts = counts;
    if (mem_kind == SPANGPU_MEM_HOST)
    {
        const size_t bytes = n*(size_t) cap*esz;
        if ((rc = grow(&b->d_events, &b->events_cap, bytes, 1, b->c.stream)) != SPANGPU_OK)
            return rc;
        SPG_TRY(hipMemcpyAsync(b->d_events, rows, bytes, hipMemcpyHostToDevice, b->c.stream));
        if (counts)
            SPG_TRY(hipMemcpyAsync(b->d_counts, counts, n*sizeof(int32_t), hipMemcpyHostToDevice, b->c.stream));
        // the caller's arrays are only borrowed for the call
        SPG_TRY(hipStreamSynchronize(b->c.stream));
        L.events = b->d_events;
        L.counts = counts  ?  b->d_counts  :  NULL;
    }
    L.st = b->c.st;
    L.buf = b->buf;
    L.n_ch = b->c.n_ch;
    L.cap = cap;
    L.all = (int) cap;
    L.vec = (((size_t) cap*esz) % 16 == 0  &&  (reinterpret_cast<uintptr_t>(L.events) & 15) == 0)  ?  1  :  0;
    L.recs = b->recs;
    L.bytes = b->bytes;
    L.rec_counts = b->counts.dev;
    L.byte_counts = b->counts.dev + n;
    L.rec_cap = rec_cap;
    L.byte_cap = byte_cap;
    const dim3 grid((b->c.n_ch + 63)/64);
    if (elem_bytes == 2)
        hipLaunchKernelGGL(hdlc_rx_kernel<int16_t>, grid, dim3(64), 0, b->c.stream, L);
    else if (elem_bytes == 1)
        hipLaunchKernelGGL(hdlc_rx_kernel<int8_t>, grid, dim3(64), 0, b->c.stream, L);
    else
        hipLaunchKernelGGL(hdlc_rx_kernel<uint8_t>, grid, dim3(64), 0, b->c.stream, L);
    SPG_TRY(hipGetLastError());
    b->rec_cap = rec_cap;
    b->byte_cap = byte_cap;
    return SPANGPU_OK;
}

int spangpu_hdlc_rx_put_events(spangpu_hdlc_rx_t *b, int mem_kind, const void *events, int elem_bytes, long long cap, const int32_t *counts)
{
    if (elem_bytes != 1  &&  elem_bytes != 2)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "events are int8 or int16");
    return rx_launch(b, mem_kind, events, elem_bytes, cap, counts);
}

int spangpu_hdlc_rx_put_modem_events(spangpu_hdlc_rx_t *b, const void *dev_block, int per_channel)
{
    if (b == NULL  ||  dev_block == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int32_t *counts = (const int32_t *) dev_block;
    return rx_launch(b, SPANGPU_MEM_DEVICE, counts + b->c.n_ch, 1, per_channel, counts);
}

int spangpu_hdlc_rx_put(spangpu_hdlc_rx_t *b, int mem_kind, const uint8_t *bytes, long long stride, const int32_t *lens)
{
    return rx_launch(b, mem_kind, bytes, 0, stride, lens);
}

int spangpu_hdlc_rx_records(spangpu_hdlc_rx_t *b, const int32_t **recs, const int32_t **counts, const uint8_t **bytes)
{
    if (b == NULL  ||  recs == NULL  ||  counts == NULL  ||  bytes == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (b->rec_cap <= 0)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no put yet");
    int rc = counts_fetch(&b->c, &b->counts, 2);
    if (rc != SPANGPU_OK)
        return rc;
    // the lists are sized from what a call can deliver at most: a count above that means the sizing is wrong, and is not
    // cut short quietly
    const int32_t *h = b->counts.pinned;
    int most_recs;
    int most_bytes;
    if (!count_row_scan(h, b->c.n_ch, b->rec_cap, &most_recs)  ||  !count_row_scan(h + b->c.n_ch, b->c.n_ch, b->byte_cap, &most_bytes))
        return spangpu_set_error(SPANGPU_ERR_STATE, "a channel delivered more than a call of this length can carry");
    if ((rc = rows_fetch(&b->c, b->h_recs, b->recs, sizeof(int32_t), b->rec_cap, most_recs)) != SPANGPU_OK
        ||  (rc = rows_fetch(&b->c, b->h_bytes, b->bytes, 1, b->byte_cap, most_bytes)) != SPANGPU_OK)
        return rc;
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    *recs = b->h_recs;
    *counts = h;
    *bytes = b->h_bytes;
    return b->rec_cap;
}

int spangpu_hdlc_rx_set_max_frame_len(spangpu_hdlc_rx_t *b, int channel, int len)
{
    if (b == NULL  ||  len < 0  ||  (channel != -1  &&  !channel_ok(&b->c, channel)))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const size_t n = (channel < 0)  ?  (size_t) b->c.n_ch  :  1;
    int32_t *w = (int32_t *) malloc(n*sizeof(int32_t));
    if (w == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "malloc");
    int rc = row_rw(&b->c, HR_CRC_BYTES, channel, w, false);
    for (size_t i = 0;  i < n;  i++)
        w[i] = ((long long) len + w[i] <= kHdlcBuf)  ?  (len + w[i])  :  kHdlcBuf;
    if (rc == SPANGPU_OK)
        rc = row_rw(&b->c, HR_MAX_FRAME_LEN, channel, w, true);
    free(w);
    return rc;
}

int spangpu_hdlc_rx_set_octet_counting_report_interval(spangpu_hdlc_rx_t *b, int channel, int interval)
{
    if (b == NULL  ||  (channel != -1  &&  !channel_ok(&b->c, channel)))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const size_t n = (channel < 0)  ?  (size_t) b->c.n_ch  :  1;
    int32_t *w = (int32_t *) malloc(n*sizeof(int32_t));
    if (w == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "malloc");
    for (size_t i = 0;  i < n;  i++)
        w[i] = interval;
    const int rc = row_rw(&b->c, HR_OCTET_COUNT_REPORT_INTERVAL, channel, w, true);
    free(w);
    return rc;
}

int spangpu_hdlc_rx_restart(spangpu_hdlc_rx_t *b, int channel)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w[kHdlcRxWords];
    const int rc = core_rw_words(&b->c, channel, 0, kHdlcRxWords, w, false);
    if (rc != SPANGPU_OK)
        return rc;
    hdlc_rx_words_restart(w);
    return core_rw_words(&b->c, channel, 0, kHdlcRxWords, w, true);
}

int spangpu_hdlc_rx_get_stats(spangpu_hdlc_rx_t *b, int channel, int32_t *stats)
{
    if (b == NULL  ||  stats == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, HR_RX_BYTES, 5, stats, false);
}

int spangpu_hdlc_rx_get_state(spangpu_hdlc_rx_t *b, int channel, int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, 0, b->c.words, words, false);
}

int spangpu_hdlc_rx_set_state(spangpu_hdlc_rx_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    // (a frame is stored below max_frame_len and checked up to len <= max_frame_len: inside the buffer with these)
    if ((words[HR_CRC_BYTES] != 2  &&  words[HR_CRC_BYTES] != 4)  ||  words[HR_MAX_FRAME_LEN] < 0  ||  words[HR_MAX_FRAME_LEN] > kHdlcBuf
        ||  words[HR_FRAMING_OK_THRESHOLD] < 1  ||  words[HR_LEN] < 0  ||  words[HR_LEN] > kHdlcBuf + 1  ||  words[HR_NUM_BITS] < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "not the words of a channel of this bank");
    return core_rw_words(&b->c, channel, 0, b->c.words, const_cast<int32_t *>(words), true);
}

int spangpu_hdlc_rx_get_buffer(spangpu_hdlc_rx_t *b, int channel, uint8_t *buffer)
{
    if (b == NULL  ||  buffer == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return buffer_rw(&b->c, b->buf, channel, buffer, false);
}

int spangpu_hdlc_rx_set_buffer(spangpu_hdlc_rx_t *b, int channel, const uint8_t *buffer)
{
    if (b == NULL  ||  buffer == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return buffer_rw(&b->c, b->buf, channel, const_cast<uint8_t *>(buffer), true);
}

// ---- senders ----------------------------------------------------------------------------------------------------------

void spangpu_hdlc_tx_destroy(spangpu_hdlc_tx_t *b)
{
    if (b == NULL)
        return;
    core_destroy(&b->c);
    (void) hipFree(b->buf);
    (void) hipFree(b->q_hdr);
    (void) hipFree(b->q_data);
    (void) hipFree(b->d_frames);
    (void) hipFree(b->d_cmd);
    (void) hipFree(b->d_bits);
    (void) hipFree(b->d_want);
    (void) hipFree(b->out);
    if (b->h_cmd)
        (void) hipHostFree(b->h_cmd);
    if (b->h_out)
        (void) hipHostFree(b->h_out);
    free(b->ev_channels);
    free(b->ev_kinds);
    free(b);
}

int spangpu_hdlc_tx_create(spangpu_hdlc_tx_t **out, int device, int n_channels, int crc32, int inter_frame_flags, int progressive,
                           int queue_depth)
{
    if (out == NULL  ||  n_channels <= 0  ||  queue_depth < 1  ||  queue_depth > 1024)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (a queue of 1 to 1024 commands)");
    *out = NULL;
    if (progressive)
        return spangpu_set_error(SPANGPU_ERR_UNSUPPORTED, "an HDLC sender bank does not run progressive mode");
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_hdlc_tx_s *b = (spangpu_hdlc_tx_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    if ((rc = core_create(&b->c, device, n_channels, kHdlcTxWords)) != SPANGPU_OK)
    {
        spangpu_hdlc_tx_destroy(b);
        return rc;
    }
    const size_t n = (size_t) n_channels;
    b->depth = queue_depth;
    b->ev_channels = (int32_t *) malloc(2*n*sizeof(int32_t));
    b->ev_kinds = (int32_t *) malloc(2*n*sizeof(int32_t));
    if (b->ev_channels == NULL  ||  b->ev_kinds == NULL
        ||  hipMalloc(&b->buf, n*kHdlcBufWords*sizeof(uint32_t)) != hipSuccess  ||  hipMalloc(&b->q_hdr, n*queue_depth*sizeof(int32_t)) != hipSuccess
        ||  hipMalloc(&b->q_data, n*queue_depth*kHdlcBufWords*sizeof(uint32_t)) != hipSuccess
        ||  hipMalloc(&b->d_cmd, 3*n*sizeof(int32_t)) != hipSuccess  ||  hipHostMalloc(&b->h_cmd, 3*n*sizeof(int32_t)) != hipSuccess
        ||  hipMalloc(&b->d_want, n*sizeof(int32_t)) != hipSuccess
        ||  hipMalloc(&b->out, 3*n*sizeof(int32_t)) != hipSuccess  ||  hipHostMalloc(&b->h_out, 3*n*sizeof(int32_t)) != hipSuccess)
    {
        spangpu_hdlc_tx_destroy(b);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the HDLC sender bank failed");
    }
    int32_t one[kHdlcTxWords];
    hdlc_tx_words_init(one, crc32, inter_frame_flags);
    rc = core_fill(&b->c, one);
    if (rc == SPANGPU_OK
        &&  (hipMemset(b->buf, 0, n*kHdlcBufWords*sizeof(uint32_t)) != hipSuccess  ||  hipMemset(b->q_hdr, 0, n*queue_depth*sizeof(int32_t)) != hipSuccess
             ||  hipMemset(b->q_data, 0, n*queue_depth*kHdlcBufWords*sizeof(uint32_t)) != hipSuccess))
        rc = spangpu_set_error(SPANGPU_ERR_HIP, "state upload failed");
    if (rc != SPANGPU_OK)
    {
        spangpu_hdlc_tx_destroy(b);
        return rc;
    }
    *out = b;
    return SPANGPU_OK;
}

int spangpu_hdlc_tx_channels(const spangpu_hdlc_tx_t *b) { return b  ?  b->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_hdlc_tx_state_words(const spangpu_hdlc_tx_t *b) { return b  ?  b->c.words  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_hdlc_tx_set_stream(spangpu_hdlc_tx_t *b, void *stream)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&b->c, stream);
}

int spangpu_hdlc_tx_sync(spangpu_hdlc_tx_t *b)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&b->c);
}

// one command for each of channels [first, first + n)
static int tx_command(spangpu_hdlc_tx_s *b, int first, int n, int kind, const uint8_t *frames, int stride, const int32_t *lens,
                      const int32_t *flags, int all, int32_t *results)
{
    if (b == NULL  ||  !range_ok(&b->c, first, n))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    SPG_TRY(hipSetDevice(b->c.device));
    const size_t nn = (size_t) b->c.n_ch;
    // (the pinned block may still be on its way from the last command)
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    for (int i = 0;  i < n;  i++)
    {
        b->h_cmd[i] = lens  ?  lens[i]  :  all;
        b->h_cmd[nn + i] = flags  ?  flags[i]  :  0;
    }
    if (kind == kHdlcCmdFrame)
    {
        const size_t bytes = (size_t) n*stride;
        const int rc = grow(&b->d_frames, &b->frames_cap, bytes, 1, b->c.stream);
        if (rc != SPANGPU_OK)
            return rc;
        SPG_TRY(hipMemcpyAsync(b->d_frames, frames, bytes, hipMemcpyHostToDevice, b->c.stream));
    }
    SPG_TRY(hipMemcpyAsync(b->d_cmd, b->h_cmd, 2*nn*sizeof(int32_t), hipMemcpyHostToDevice, b->c.stream));
    hipLaunchKernelGGL(hdlc_tx_enqueue_kernel, dim3((n + 63)/64), dim3(64), 0, b->c.stream, b->c.st, b->c.n_ch, b->q_hdr, b->q_data, b->depth,
                       first, first + n, kind, b->d_frames, stride, b->d_cmd, b->d_cmd + nn, b->d_cmd + 2*nn);
    SPG_TRY(hipGetLastError());
    SPG_TRY(hipMemcpyAsync(b->h_cmd + 2*nn, b->d_cmd + 2*nn, (size_t) n*sizeof(int32_t), hipMemcpyDeviceToHost, b->c.stream));
    // the caller's frames are pageable: they must not change under the copy
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    if (results)
        memcpy(results, b->h_cmd + 2*nn, (size_t) n*sizeof(int32_t));
    return SPANGPU_OK;
}

int spangpu_hdlc_tx_frames(spangpu_hdlc_tx_t *b, int first, int n, const uint8_t *frames, int stride, const int32_t *lens, const int32_t *flags,
                           int32_t *results)
{
    if (frames == NULL  ||  lens == NULL  ||  stride <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return tx_command(b, first, n, kHdlcCmdFrame, frames, stride, lens, flags, 0, results);
}

int spangpu_hdlc_tx_flags(spangpu_hdlc_tx_t *b, int first, int n, int len, int32_t *results)
{
    if (len < -(1 << 22)  ||  len > (1 << 22))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return tx_command(b, first, n, kHdlcCmdFlags, NULL, 0, NULL, NULL, len, results);
}

int spangpu_hdlc_tx_abort(spangpu_hdlc_tx_t *b, int first, int n, int32_t *results)
{
    return tx_command(b, first, n, kHdlcCmdAbort, NULL, 0, NULL, NULL, 0, results);
}

int spangpu_hdlc_tx_end(spangpu_hdlc_tx_t *b, int first, int n, int32_t *results)
{
    return tx_command(b, first, n, kHdlcCmdEnd, NULL, 0, NULL, NULL, 0, results);
}

int spangpu_hdlc_tx_queued(spangpu_hdlc_tx_t *b, int channel)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t count = 0;
    const int rc = core_rw_words(&b->c, channel, HT_Q_COUNT, 1, &count, false);
    return (rc != SPANGPU_OK)  ?  rc  :  count;
}

int spangpu_hdlc_tx_set_max_frame_len(spangpu_hdlc_tx_t *b, int channel, int len)
{
    if (b == NULL  ||  len < 0  ||  (channel != -1  &&  !channel_ok(&b->c, channel)))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const size_t n = (channel < 0)  ?  (size_t) b->c.n_ch  :  1;
    int32_t *w = (int32_t *) malloc(n*sizeof(int32_t));
    if (w == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "malloc");
    for (size_t i = 0;  i < n;  i++)
        w[i] = (len <= kHdlcMaxFrame)  ?  len  :  kHdlcMaxFrame;
    const int rc = row_rw(&b->c, HT_MAX_FRAME_LEN, channel, w, true);
    free(w);
    return rc;
}

// hdlc_tx_restart(); what was queued for the channel goes too
int spangpu_hdlc_tx_restart(spangpu_hdlc_tx_t *b, int channel)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int32_t w[kHdlcTxWords];
    const int rc = core_rw_words(&b->c, channel, 0, kHdlcTxWords, w, false);
    if (rc != SPANGPU_OK)
        return rc;
    hdlc_tx_words_restart(w);
    w[HT_Q_HEAD] = 0;
    w[HT_Q_COUNT] = 0;
    return core_rw_words(&b->c, channel, 0, kHdlcTxWords, w, true);
}

int spangpu_hdlc_tx_get_bits(spangpu_hdlc_tx_t *b, int mem_kind, uint8_t *bits, long long stride, const int32_t *want, int want_all, int32_t *lens)
{
    if (b == NULL  ||  bits == NULL  ||  stride <= 0  ||  stride*8 > kMaxSamples  ||  want_all < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int rc = mem_kind_ok(mem_kind);
    if (rc != SPANGPU_OK)
        return rc;
    const size_t n = (size_t) b->c.n_ch;
    for (size_t c = 0;  c < n;  c++)
    {
        const long long k = want  ?  want[c]  :  want_all;
        if (k < 0  ||  k > stride*8)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a channel's bits do not fit its row");
    }
    SPG_TRY(hipSetDevice(b->c.device));
    const bool host = (mem_kind == SPANGPU_MEM_HOST);
    if (host  &&  (rc = grow(&b->d_bits, &b->bits_cap, n*(size_t) stride, 1, b->c.stream)) != SPANGPU_OK)
        return rc;
    if (want)
    {
        SPG_TRY(hipMemcpyAsync(b->d_want, want, n*sizeof(int32_t), hipMemcpyHostToDevice, b->c.stream));
        // want[] is pageable host memory, borrowed for the call
        SPG_TRY(hipStreamSynchronize(b->c.stream));
    }
    HdlcTxLaunch L;
    memset(&L, 0, sizeof(L));
    L.st = b->c.st;
    L.buf = b->buf;
    L.n_ch = b->c.n_ch;
    L.q_hdr = b->q_hdr;
    L.q_data = b->q_data;
    L.depth = b->depth;
    L.bits = host  ?  b->d_bits  :  bits;
    L.stride = stride;
    L.want = want  ?  b->d_want  :  NULL;
    L.want_all = want_all;
    L.lens = (!host  &&  lens)  ?  lens  :  b->out;
    L.ended = b->out + n;
    L.underflows = b->out + 2*n;
    hipLaunchKernelGGL(hdlc_tx_kernel, dim3((b->c.n_ch + 63)/64), dim3(64), 0, b->c.stream, L);
    SPG_TRY(hipGetLastError());
    b->ran = true;
    if (host)
    {
        SPG_TRY(hipMemcpyAsync(bits, b->d_bits, n*(size_t) stride, hipMemcpyDeviceToHost, b->c.stream));
        if (lens)
            SPG_TRY(hipMemcpyAsync(lens, b->out, n*sizeof(int32_t), hipMemcpyDeviceToHost, b->c.stream));
        SPG_TRY(hipStreamSynchronize(b->c.stream));
    }
    return SPANGPU_OK;
}

int spangpu_hdlc_tx_events(spangpu_hdlc_tx_t *b, const int32_t **channels, const int32_t **kinds)
{
    if (b == NULL  ||  channels == NULL  ||  kinds == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (!b->ran)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no spangpu_hdlc_tx_get_bits() yet");
    SPG_TRY(hipSetDevice(b->c.device));
    const size_t n = (size_t) b->c.n_ch;
    SPG_TRY(hipMemcpyAsync(b->h_out + n, b->out + n, 2*n*sizeof(int32_t), hipMemcpyDeviceToHost, b->c.stream));
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    int k = 0;
    for (size_t c = 0;  c < n;  c++)
    {
        if (b->h_out[2*n + c] > 0)
        {
            b->ev_channels[k] = (int32_t) c;
            b->ev_kinds[k++] = b->h_out[2*n + c];
        }
        if (b->h_out[n + c])
        {
            b->ev_channels[k] = (int32_t) c;
            b->ev_kinds[k++] = kSigEndOfData;
        }
    }
    *channels = b->ev_channels;
    *kinds = b->ev_kinds;
    return k;
}

int spangpu_hdlc_tx_get_state(spangpu_hdlc_tx_t *b, int channel, int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, 0, b->c.words, words, false);
}

int spangpu_hdlc_tx_set_state(spangpu_hdlc_tx_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int crc_bytes = words[HT_CRC_BYTES];
    const int pos = words[HT_POS];
    const int len = words[HT_LEN];
    // (the position walks the frame, then the CRC behind the longest frame: nowhere else is inside the buffer)
    if ((crc_bytes != 2  &&  crc_bytes != 4)  ||  words[HT_PROGRESSIVE]  ||  words[HT_INTER_FRAME_FLAGS] < 1
        ||  words[HT_MAX_FRAME_LEN] < 0  ||  words[HT_MAX_FRAME_LEN] > kHdlcMaxFrame  ||  len < 0  ||  len > kHdlcMaxFrame
        ||  pos < 0  ||  (pos > len  &&  (pos < kHdlcMaxFrame  ||  pos > kHdlcMaxFrame + crc_bytes))
        ||  words[HT_NUM_BITS] < 0  ||  words[HT_NUM_BITS] > 15  ||  words[HT_BITS] < 0  ||  words[HT_BITS] > 8
        ||  words[HT_Q_HEAD] < 0  ||  words[HT_Q_HEAD] >= b->depth  ||  words[HT_Q_COUNT] < 0  ||  words[HT_Q_COUNT] > b->depth)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "not the words of a channel of this bank");
    return core_rw_words(&b->c, channel, 0, b->c.words, const_cast<int32_t *>(words), true);
}

int spangpu_hdlc_tx_get_buffer(spangpu_hdlc_tx_t *b, int channel, uint8_t *buffer)
{
    if (b == NULL  ||  buffer == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return buffer_rw(&b->c, b->buf, channel, buffer, false);
}

int spangpu_hdlc_tx_set_buffer(spangpu_hdlc_tx_t *b, int channel, const uint8_t *buffer)
{
    if (b == NULL  ||  buffer == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return buffer_rw(&b->c, b->buf, channel, const_cast<uint8_t *>(buffer), true);
}

}   // extern "C"
