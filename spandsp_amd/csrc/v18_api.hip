// v18_api.hip -- C ABI of the V.18 text banks (include/spangpu.h, "V.18 text banks"): batched v18_put() / v18_tx() /
// v18_rx() in the three Weitbrecht 5-bit modes with V18_AUTOMODING_NONE.  Device code: v18_dev.hpp.  No CPU implementation
// of the signal path exists behind these entry points; the two Baudot helpers at the end are plain host code, and the
// control-plane calls (restart, fill-in, state) edit one channel's words on the host, as the reference's own functions edit
// one object.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#define SPG_HDLC_STEP_FUNCTIONS_ONLY        // the HDLC banks' own kernels belong to hdlc_api.hip
#include "v18_dev.hpp"
#include "bank_host.hpp"

using namespace spg;

extern "C" void spangpu_fsk_words_init(int32_t *w, const spangpu_fsk_spec_t *spec, int framing_mode, int data_bits, int parity, int stop_bits);
extern "C" void spangpu_fsk_words_fillin(int32_t *w, int len);
extern "C" void spangpu_fsktx_words_restart(int32_t *w, const spangpu_fsk_spec_t *spec);

struct spangpu_v18_s
{
    BankCore c;
    PcmStage pcm;               // frames of a host caller, either way; d_lens: the sender's lengths
    int span;
    int max_baud;               // x 100, over the bank's channels: sizes the text records
    int16_t *quarter;
    uint8_t *ring;
    uint8_t *tables;
    VarLens rxlens;             // per-channel lengths of an rx_var call
    uint8_t *chars;             // [n_ch][last_cap]
    uint8_t *h_chars;
    CountRows counts;
    int cap;
    int last_cap;
    uint8_t *d_text;
    int32_t *d_tlens;
    int32_t *d_res;
    size_t text_cap;
};

// ---- Baudot (ITA2, US TTY figures) ------------------------------------------------------------------------------------

// what the 32 codes print in the letters and in the figures set; 0x1B and 0x1F are the two shifts
static const char k_letters[33] = "\bE\nA SIU\rDRJNFCKTZLWHYPQOBG^MXV^";
static const char k_figures[33] = "\b3\n- -87\r$4',!:(5\")2=6019?+^./;^";
// characters without a code of their own, and the character sent in their place (v18.c:770-900)
static const char k_stand_ins[][2] =
{
    {'\t', ' '}, {'\v', '\n'}, {'\f', '\n'}, {0x1A, '?'}, {0x1C, '\n'}, {0x1D, '\n'}, {0x1E, '\n'}, {0x1F, ' '},
    {'#', '$'}, {'%', '/'}, {'&', '+'}, {'*', '.'}, {'<', '('}, {'>', ')'}, {'@', 'X'}, {'[', '('}, {'\\', '/'}, {']', ')'},
    {'^', '\''}, {'_', ' '}, {'`', '\''}, {'{', '('}, {'|', '!'}, {'}', ')'}, {'~', ' '}
};

// [128] encode: 0xFF no such character, 0x40 | code present in both sets, 0x80 | code figures, code letters;
// then [2][32] decode
static void baudot_tables(uint8_t t[192])
{
    memset(t, 0xFF, 128);
    for (int c = 31;  c >= 0;  c--)
    {
        if (c == kV18FigureShift  ||  c == kV18LetterShift)
            continue;
        const int l = (unsigned char) k_letters[c];
        const int f = (unsigned char) k_figures[c];
        if (l == f)
        {
            t[l] = (uint8_t) (0x40 | c);
            continue;
        }
        t[f] = (uint8_t) (0x80 | c);      // going down: where a figure has two codes the lower one stays
        t[l] = (uint8_t) c;
        t[l + ('a' - 'A')] = (uint8_t) c;
    }
    for (size_t i = 0;  i < sizeof(k_stand_ins)/sizeof(k_stand_ins[0]);  i++)
        t[(unsigned char) k_stand_ins[i][0]] = t[(unsigned char) k_stand_ins[i][1]];
    memcpy(t + 128, k_letters, 32);
    memcpy(t + 160, k_figures, 32);
}

static const uint8_t *tables(void)
{
    static uint8_t t[192];
    static bool made = false;
    if (!made)
    {
        baudot_tables(t);
        made = true;
    }
    return t;
}

static int preset_of(int mode)
{
    switch (mode)
    {
    case SPANGPU_V18_MODE_WEITBRECHT_5BIT_4545:
        return SPANGPU_FSK_WEITBRECHT_4545;
    case SPANGPU_V18_MODE_WEITBRECHT_5BIT_476:
        return SPANGPU_FSK_WEITBRECHT_476;
    case SPANGPU_V18_MODE_WEITBRECHT_5BIT_50:
        return SPANGPU_FSK_WEITBRECHT_50;
    }
    return -1;
}

// v18_set_modem(), v18.c:1367-1424: fsk_tx_init(), async_tx_init(5, none, 2), fsk_rx_init(framed) +
// fsk_rx_set_frame_parameters(5, none, 2), the shifts and next_byte.  The ring, tx_signal_on, tx_draining and the
// suppression timer are not its business.
static void modem_words(int32_t *w, int words, int mode)
{
    spangpu_fsk_spec_t spec;
    spangpu_fsk_preset(preset_of(mode), &spec);
    w[V18_MODE] = mode;
    w[V18_BAUDOT_TX_SHIFT] = 2;
    w[V18_BAUDOT_RX_SHIFT] = 0;
    w[V18_NEXT_BYTE] = 0xFF;
    w[V18_A_BITPOS] = 0;
    w[V18_A_FRAME] = 0;
    w[V18_A_PRESEND] = 0;
    memset(w + kV18Words, 0, (size_t) (words - kV18Words)*sizeof(int32_t));
    spangpu_fsktx_words_restart(w + kV18Words, &spec);
    spangpu_fsk_words_init(w + kV18Words + kFskTxWords, &spec, SPANGPU_FSK_FRAME_MODE_FRAMED, 5, SPANGPU_ASYNC_PARITY_NONE, 2);
}

extern "C" {

void spangpu_v18_destroy(spangpu_v18_t *b)
{
    if (b == NULL)
        return;
    core_destroy(&b->c);
    stage_free(&b->pcm);
    (void) hipFree(b->quarter);
    (void) hipFree(b->ring);
    (void) hipFree(b->tables);
    lens_free(&b->rxlens);
    (void) hipFree(b->chars);
    if (b->h_chars)
        (void) hipHostFree(b->h_chars);
    counts_free(&b->counts);
    (void) hipFree(b->d_text);
    (void) hipFree(b->d_tlens);
    (void) hipFree(b->d_res);
    free(b);
}

int spangpu_v18_create(spangpu_v18_t **out, int device, int n_channels, const int32_t *modes, int n_modes, int calling_party)
{
    if (out == NULL  ||  n_channels <= 0  ||  modes == NULL  ||  (n_modes != 1  &&  n_modes != n_channels))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (n_channels > 0, one mode or one per channel)");
    *out = NULL;
    for (int i = 0;  i < n_modes;  i++)
    {
        if (preset_of(modes[i]) < 0)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a V.18 text bank runs the three Weitbrecht 5-bit modes only");
    }
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_v18_s *b = (spangpu_v18_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    b->span = kFskMaxWindow;        // 800000/baud is above the window's limit at all three rates
    const int n_words = kV18Words + kFskTxWords + kFskScalars + 4*b->span;
    if ((rc = core_create(&b->c, device, n_channels, n_words)) != SPANGPU_OK  ||  (rc = quarter_sine_upload(&b->quarter)) != SPANGPU_OK
        ||  (rc = stage_lens(&b->c, &b->pcm)) != SPANGPU_OK)
    {
        spangpu_v18_destroy(b);
        return rc;
    }
    const size_t n = (size_t) n_channels;
    const size_t words = (size_t) n_words*n;
    int32_t *one = (int32_t *) calloc(n_words, sizeof(int32_t));
    int32_t *host = (int32_t *) calloc(words, sizeof(int32_t));
    if (one == NULL  ||  host == NULL
        ||  hipMalloc(&b->ring, n*kV18Ring) != hipSuccess
        ||  hipMalloc(&b->tables, 192) != hipSuccess
        ||  counts_create(&b->c, &b->counts, 1, 1) != SPANGPU_OK)
    {
        free(one);
        free(host);
        spangpu_v18_destroy(b);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the V.18 bank failed");
    }
    // v18_init(), v18.c:2054-2115: memset, v18_set_modem(), an empty ring
    int last_mode = 0;
    for (int c = 0;  c < n_channels;  c++)
    {
        const int mode = modes[(n_modes == 1)  ?  0  :  c];
        if (mode != last_mode)
        {
            memset(one, 0, (size_t) b->c.words*sizeof(int32_t));
            modem_words(one, b->c.words, mode);
            one[V18_CALLING_PARTY] = calling_party  ?  1  :  0;
            last_mode = mode;
            spangpu_fsk_spec_t spec;
            spangpu_fsk_preset(preset_of(mode), &spec);
            b->max_baud = (spec.baud_rate > b->max_baud)  ?  spec.baud_rate  :  b->max_baud;
        }
        // (the correlation windows stay zero: only the scalars are written)
        for (int w = 0;  w < kV18Words + kFskTxWords + kFskScalars;  w++)
            host[(size_t) w*n + c] = one[w];
    }
    // (the modes differ by channel: the words go up as they were prepared, not from one prototype)
    rc = core_upload(&b->c, host);
    free(one);
    free(host);
    if (rc == SPANGPU_OK
        &&  (hipMemcpy(b->tables, tables(), 192, hipMemcpyHostToDevice) != hipSuccess  ||  hipMemset(b->ring, 0, n*kV18Ring) != hipSuccess))
        rc = spangpu_set_error(SPANGPU_ERR_HIP, "state upload failed");
    if (rc != SPANGPU_OK)
    {
        spangpu_v18_destroy(b);
        return rc;
    }
    *out = b;
    return SPANGPU_OK;
}

int spangpu_v18_channels(const spangpu_v18_t *b) { return b  ?  b->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_v18_state_words(const spangpu_v18_t *b) { return b  ?  b->c.words  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_v18_set_stream(spangpu_v18_t *b, void *stream)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&b->c, stream);
}

int spangpu_v18_sync(spangpu_v18_t *b)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&b->c);
}

int spangpu_v18_put(spangpu_v18_t *b, int first, int n, const uint8_t *text, int stride, const int32_t *lens, int32_t *results)
{
    if (b == NULL  ||  !range_ok(&b->c, first, n)  ||  text == NULL  ||  lens == NULL  ||  stride <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    for (int i = 0;  i < n;  i++)
    {
        if (lens[i] < 0  ||  lens[i] > stride)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a channel's text does not fit its row");
    }
    SPG_TRY(hipSetDevice(b->c.device));
    const size_t bytes = (size_t) n*stride;
    const int rc = grow(&b->d_text, &b->text_cap, bytes, 1, b->c.stream);
    if (rc != SPANGPU_OK)
        return rc;
    if ((b->d_tlens == NULL  &&  hipMalloc(&b->d_tlens, (size_t) b->c.n_ch*sizeof(int32_t)) != hipSuccess)
        ||  (b->d_res == NULL  &&  hipMalloc(&b->d_res, (size_t) b->c.n_ch*sizeof(int32_t)) != hipSuccess))
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "text staging");
    SPG_TRY(hipMemcpyAsync(b->d_text, text, bytes, hipMemcpyHostToDevice, b->c.stream));
    SPG_TRY(hipMemcpyAsync(b->d_tlens, lens, (size_t) n*sizeof(int32_t), hipMemcpyHostToDevice, b->c.stream));
    hipLaunchKernelGGL(v18_put_kernel, dim3((n + 63)/64), dim3(64), 0, b->c.stream, b->c.st, b->ring, b->c.n_ch, first, first + n, b->d_text, stride,
                       b->d_tlens, b->d_res);
    SPG_TRY(hipGetLastError());
    if (results)
        SPG_TRY(hipMemcpyAsync(results, b->d_res, (size_t) n*sizeof(int32_t), hipMemcpyDeviceToHost, b->c.stream));
    // the caller's arrays are pageable: they must not change under the copies
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    return SPANGPU_OK;
}

int spangpu_v18_tx(spangpu_v18_t *b, int mem_kind, int16_t *pcm, long long stride, int samples, int32_t *lens)
{
    int rc = tx_args_ok(b, mem_kind, pcm, stride, samples);
    if (rc != SPANGPU_OK)
        return rc;
    if (samples == 0)
    {
        // (an empty call zeroes a host caller's lens; the tone sender leaves them)
        if (lens  &&  mem_kind == SPANGPU_MEM_HOST)
            memset(lens, 0, (size_t) b->c.n_ch*sizeof(int32_t));
        return SPANGPU_OK;
    }
    SPG_TRY(hipSetDevice(b->c.device));
    V18TxLaunch L;
    memset(&L, 0, sizeof(L));
    if ((rc = stage_out_target(&b->c, &b->pcm, mem_kind, pcm, stride, samples, lens, &L.pcm, &L.stride, &L.lens, &L.vec)) != SPANGPU_OK)
        return rc;
    L.st = b->c.st;
    L.quarter = b->quarter;
    L.ring = b->ring;
    L.tables = b->tables;
    L.n_ch = b->c.n_ch;
    L.samples = samples;
    hipLaunchKernelGGL(v18_tx_kernel, dim3((b->c.n_ch + kFtxCpw*kFtxWaves - 1)/(kFtxCpw*kFtxWaves)), dim3(64*kFtxWaves), 0, b->c.stream, L);
    SPG_TRY(hipGetLastError());
    return stage_out_back(&b->c, &b->pcm, mem_kind, pcm, stride, samples, lens);
}

int spangpu_v18_text_capacity(const spangpu_v18_t *b, int samples)
{
    if (b == NULL  ||  samples < 0)
        return SPANGPU_ERR_BAD_ARG;
    // a character is at least 7 bit times (start, 5 data, the stop bit that is looked for): samples*baud/(8000*7), and one
    // each for the characters under way at either end of the call
    return (int) ((long long) samples*b->max_baud/(800000LL*7)) + 2;
}

static int rx_launch(spangpu_v18_s *b, const int16_t *amp, int mem_kind, int samples, long long stride)
{
    SPG_TRY(hipSetDevice(b->c.device));
    const int cap = spangpu_v18_text_capacity(b, samples);
    int rc = grow_pair(&b->chars, &b->h_chars, &b->cap, cap, (size_t) b->c.n_ch, b->c.stream);
    if (rc != SPANGPU_OK)
        return rc;
    V18RxLaunch V;
    memset(&V, 0, sizeof(V));
    FskLaunch &L = V.f;
    L.st = b->c.st + (size_t) (kV18Words + kFskTxWords)*b->c.n_ch;
    L.quarter = b->quarter;
    L.n_ch = b->c.n_ch;
    L.samples = samples;
    L.lens = b->rxlens.next;
    L.span = b->span;
    // the caller's buffer is only borrowed for the call: the copy in is waited for
    if ((rc = stage_in(&b->c, &b->pcm, mem_kind, amp, stride, samples, true, &L.pcm, &L.stride, &L.vec)) != SPANGPU_OK)
        return rc;
    V.sv = b->c.st;
    V.tables = b->tables;
    V.chars = b->chars;
    V.counts = b->counts.dev;
    V.cap = cap;
    const size_t lds = (size_t) (4*b->span*64 + 2*kFskMsgWords*64)*sizeof(int32_t);
    hipLaunchKernelGGL(v18_rx_kernel, dim3((b->c.n_ch + 63)/64), dim3(128), lds, b->c.stream, V);
    SPG_TRY(hipGetLastError());
    b->last_cap = cap;
    return SPANGPU_OK;
}

int spangpu_v18_rx(spangpu_v18_t *b, const int16_t *amp, int mem_kind, int samples, long long stride)
{
    if (samples > kMaxSamples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int rc = rx_args_ok(b, mem_kind, amp, samples, &stride);
    if (rc != SPANGPU_OK)
        return rc;
    return rx_launch(b, amp, mem_kind, samples, stride);
}

// spangpu_v18_rx() for a tick in which not every channel has a frame, or frames differ in length: channel c takes lens[c]
// samples of its row (0: it sits the call out: its state and its suppression timer as they were, an empty record).
int spangpu_v18_rx_var(spangpu_v18_t *b, const int16_t *amp, int mem_kind, const int32_t *lens, int max_samples, long long stride)
{
    if (b == NULL  ||  amp == NULL  ||  lens == NULL  ||  max_samples <= 0  ||  max_samples > kMaxSamples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (mem_kind != SPANGPU_MEM_HOST  &&  mem_kind != SPANGPU_MEM_DEVICE)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad mem kind");
    int longest;
    bool all;
    int rc = lens_check(lens, b->c.n_ch, max_samples, &longest, &all);
    if (rc != SPANGPU_OK)
        return rc;
    if (stride <= 0)
        stride = max_samples;
    if (stride < max_samples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "stride < max_samples");
    // always a launch of max_samples with the lengths: a call nobody takes part in leaves an empty record
    if ((rc = lens_upload(&b->c, &b->rxlens, lens)) != SPANGPU_OK)
        return rc;
    rc = rx_launch(b, amp, mem_kind, max_samples, stride);
    b->rxlens.next = NULL;
    return rc;
}

int spangpu_v18_text(spangpu_v18_t *b, const uint8_t **chars, const int32_t **counts)
{
    if (b == NULL  ||  chars == NULL  ||  counts == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (b->last_cap <= 0)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no spangpu_v18_rx() yet");
    int rc = counts_fetch(&b->c, &b->counts, 1);
    if (rc != SPANGPU_OK)
        return rc;
    // the record is sized from the frame format; a count above it would mean the sizing is wrong, and is not cut short quietly
    int most;
    if (!count_row_scan(b->counts.pinned, b->c.n_ch, b->last_cap, &most))
        return spangpu_set_error(SPANGPU_ERR_STATE, "a channel decoded more characters than a call of this length can carry");
    if ((rc = rows_fetch(&b->c, b->h_chars, b->chars, 1, b->last_cap, most)) != SPANGPU_OK)
        return rc;
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    *chars = b->h_chars;
    *counts = b->counts.pinned;
    return b->last_cap;
}

int spangpu_v18_get_state(spangpu_v18_t *b, int channel, int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, 0, b->c.words, words, false);
}

int spangpu_v18_set_state(spangpu_v18_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (preset_of(words[V18_MODE]) < 0  ||  words[kV18Words + kFskTxWords + FS_SPAN] != b->span
        ||  words[V18_Q_IPTR] < 0  ||  words[V18_Q_IPTR] >= kV18Ring  ||  words[V18_Q_OPTR] < 0  ||  words[V18_Q_OPTR] >= kV18Ring
        ||  words[kV18Words + kFskTxWords + FS_BUF_PTR] < 0  ||  words[kV18Words + kFskTxWords + FS_BUF_PTR] >= b->span
        ||  words[kV18Words + FT_BAUD_RATE] <= 0  ||  words[kV18Words + FT_BAUD_RATE] > kFtxBaudUnit)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "not the words of a channel of this bank");
    return core_rw_words(&b->c, channel, 0, b->c.words, const_cast<int32_t *>(words), true);
}

static int edit(spangpu_v18_s *b, int channel, int what, int a)
{
    int32_t *w = (int32_t *) malloc((size_t) b->c.words*sizeof(int32_t));
    if (w == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "malloc");
    int rc = core_rw_words(&b->c, channel, 0, b->c.words, w, false);
    if (rc == SPANGPU_OK)
    {
        if (what == 0)
        {
            modem_words(w, b->c.words, a);
        }
        else
        {
            // v18_rx_fillin(), v18.c:1943-1987
            if (w[V18_RX_SUPPRESSION] > 0)
                w[V18_RX_SUPPRESSION] = (w[V18_RX_SUPPRESSION] > a)  ?  (w[V18_RX_SUPPRESSION] - a)  :  0;
            spangpu_fsk_words_fillin(w + kV18Words + kFskTxWords, a);
        }
        rc = core_rw_words(&b->c, channel, 0, b->c.words, w, true);
    }
    free(w);
    return rc;
}

int spangpu_v18_restart(spangpu_v18_t *b, int channel, int mode)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel)  ||  preset_of(mode) < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (one of the three Weitbrecht 5-bit modes)");
    spangpu_fsk_spec_t spec;
    spangpu_fsk_preset(preset_of(mode), &spec);
    b->max_baud = (spec.baud_rate > b->max_baud)  ?  spec.baud_rate  :  b->max_baud;
    return edit(b, channel, 0, mode);
}

int spangpu_v18_fillin(spangpu_v18_t *b, int channel, int len)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel)  ||  len < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return edit(b, channel, 1, len);
}

// ---- the Baudot helpers: host only ------------------------------------------------------------------------------------

int spangpu_baudot_encode(const uint8_t *text, int n, uint8_t *codes_out, int max, int *shift_state)
{
    if (text == NULL  ||  n < 0  ||  codes_out == NULL  ||  max < 0  ||  shift_state == NULL  ||  *shift_state < 0  ||  *shift_state > 2)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (shift state 0 letters, 1 figures, 2 an explicit shift first)");
    const uint8_t *t = tables();
    int shift = *shift_state;
    int k = 0;
    for (int i = 0;  i < n;  i++)
    {
        const int e = t[text[i] & 0x7F];
        if (e == 0xFF)
            continue;
        if (!(e & 0x40))
        {
            const int set = (e & 0x80)  ?  1  :  0;
            if (shift != set)
            {
                if (k >= max)
                    return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "the codes do not fit");
                codes_out[k++] = (uint8_t) (set  ?  kV18FigureShift  :  kV18LetterShift);
                shift = set;
            }
        }
        if (k >= max)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "the codes do not fit");
        codes_out[k++] = (uint8_t) (e & 0x1F);
    }
    *shift_state = shift;
    return k;
}

int spangpu_baudot_decode(const uint8_t *codes, int n, uint8_t *text_out, int *shift_state)
{
    if (codes == NULL  ||  n < 0  ||  text_out == NULL  ||  shift_state == NULL  ||  *shift_state < 0  ||  *shift_state > 1)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (shift state 0 letters, 1 figures)");
    const uint8_t *t = tables() + 128;
    int shift = *shift_state;
    int k = 0;
    for (int i = 0;  i < n;  i++)
    {
        const int c = codes[i] & 0x1F;
        if (c == kV18FigureShift)
            shift = 1;
        else if (c == kV18LetterShift)
            shift = 0;
        else
            text_out[k++] = t[shift*32 + c];
    }
    *shift_state = shift;
    return k;
}

}   // extern "C"
