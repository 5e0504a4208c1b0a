// mct_api.hip -- C ABI of the modem connect tone detector banks (include/spangpu.h, "modem connect tone
// banks"): batched modem_connect_tones_rx().  Device code: mct_dev.hpp (+ fsk_dev.hpp for the V.21 preamble
// hunter).  No CPU implementation of the receive path exists behind these entry points.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#include "mct_dev.hpp"
#include "bank_host.hpp"

using namespace spg;

struct spangpu_mct_s
{
    VarLens lens;               // per-channel lengths of the call being prepared
    BankCore c;
    PcmStage pcm;
    int tone_type;              // after modem_connect_tones_rx_init()'s folding of the ANS variants
    int latch;
    int16_t *quarter;
    int32_t *events;            // [n_ch][ev_cap][2]
    int32_t *h_events;
    CountRows count;
    int ev_cap;
    int last_cap;
};

static const float kMaxPower = 3.14f + 3.02f;       // DBM0_MAX_POWER

// The level a report carries, from the integer the kernel recorded (libm's log10f, like the reference).
static int level_of(int tone, int32_t from)
{
    if (tone == MCT_NONE)
        return -99;
    if (tone == MCT_FAX_PREAMBLE)
    {
        // lfastrintf(fsk_rx_signal_power()): power_meter_current_dbm0(), power_meter.c:114-121
        const float dbm0 = (from <= 0)  ?  (-96.329f + kMaxPower)
                                        :  10.0f*log10f((float) from/(32767.0f*32767.0f) + 1.0e-10f) + kMaxPower;
        return (int) (long) dbm0;
    }
    // modem_connect_tones.c:561 (and :643,:659,:723,:777)
    const float db = (from == 0)  ?  (-96.329f + kMaxPower)  :  20.0f*log10f(from/32768.0f);
    return (int) (long) (db + kMaxPower + 0.8f);
}

static int32_t power_level_dbm0(float level)
{
    // power_meter_level_dbm0(), power_meter.c:82-92
    level -= kMaxPower;
    if (level > 0.0)
        level = 0.0;
    return (int32_t) (powf(10.0f, level/10.0f)*(32767.0f*32767.0f));
}

extern "C" int spangpu_fsk_waves_choice(void);       // fsk_api.hip: what spangpu_tune_fsk_waves() was given

template <int TYPE>
static void launch(const spangpu_mct_s *m, const MctLaunch &L)
{
    const bool fsk = (TYPE == MCT_FAX_PREAMBLE  ||  TYPE == MCT_FAX_CED_OR_PREAMBLE);
    const size_t lds = fsk  ?  (size_t) (4*kMctV21Span*64)*sizeof(int32_t)  :  0;
    if (TYPE == MCT_FAX_CED_OR_PREAMBLE  &&  spangpu_fsk_waves_choice() != 1)
        hipLaunchKernelGGL(mct_ced_pair_kernel, dim3((m->c.n_ch + 63)/64), dim3(128), lds + 3*64*sizeof(int32_t), m->c.stream, L);
    else
        hipLaunchKernelGGL(mct_bank_kernel<TYPE>, dim3((m->c.n_ch + 63)/64), dim3(64), lds, m->c.stream, L);
}

extern "C" {

int spangpu_mct_create(spangpu_mct_t **out, int device, int tone_type, int n_channels, int use_callback)
{
    if (out == NULL  ||  n_channels <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    *out = NULL;
    // modem_connect_tones_rx_init(), modem_connect_tones.c:812-834: modifiers off, the ANS family is one detector
    int type = tone_type & 0xFFF;
    if (type == MCT_ANS_PR  ||  type == MCT_ANSAM  ||  type == MCT_ANSAM_PR)
        type = MCT_ANS;
    if (type < MCT_FAX_CNG  ||  type > MCT_CALLING_TONE)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "not a modem connect tone type");
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_mct_s *m = (spangpu_mct_s *) calloc(1, sizeof(*m));
    if (m == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    m->tone_type = type;
    m->latch = use_callback  ?  0  :  1;
    const bool fsk = (type == MCT_FAX_PREAMBLE  ||  type == MCT_FAX_CED_OR_PREAMBLE);
    const int words = kMctWords + (fsk  ?  (kFskScalars + 4*kMctV21Span)  :  0);
    if ((rc = core_create(&m->c, device, n_channels, words)) != SPANGPU_OK  ||  (rc = quarter_sine_upload(&m->quarter)) != SPANGPU_OK)
    {
        spangpu_mct_destroy(m);
        return rc;
    }
    int32_t *one = (int32_t *) calloc(words, sizeof(int32_t));
    if (counts_create(&m->c, &m->count, 1, 1) != SPANGPU_OK  ||  one == NULL)
    {
        free(one);
        spangpu_mct_destroy(m);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the connect tone bank failed");
    }
    one[MC_TONE_TYPE] = type;
    if (fsk)
    {
        // fsk_rx_init(&preset_fsk_specs[FSK_V21CH2], FSK_FRAME_MODE_SYNC) + fsk_rx_set_signal_cutoff(-45.5),
        // modem_connect_tones.c:820-821 (fsk.c:660-742,270-276)
        int32_t *w = one + kMctWords;
        w[FS_BAUD_RATE] = 300*100;
        w[FS_FRAMING] = 1;
        w[FS_ON_POWER] = power_level_dbm0(-45.5f + 2.5f - 5.3f);
        w[FS_OFF_POWER] = power_level_dbm0(-45.5f - 2.5f - 5.3f);
        w[FS_RATE0] = (int32_t) ((float) (1750 + 100)*65536.0f*65536.0f/8000);
        w[FS_RATE1] = (int32_t) ((float) (1750 - 100)*65536.0f*65536.0f/8000);
        w[FS_SPAN] = kMctV21Span;
        w[FS_SHIFT] = 5;
        w[FS_FRAME_POS] = -2;
    }
    // (the preamble hunter's correlation window stays zero)
    rc = core_fill(&m->c, one, kMctWords + (fsk  ?  kFskScalars  :  0));
    free(one);
    if (rc != SPANGPU_OK)
    {
        spangpu_mct_destroy(m);
        return rc;
    }
    *out = m;
    return SPANGPU_OK;
}

void spangpu_mct_destroy(spangpu_mct_t *m)
{
    if (m == NULL)
        return;
    core_destroy(&m->c);
    stage_free(&m->pcm);
    (void) hipFree(m->quarter);
    lens_free(&m->lens);
    (void) hipFree(m->events);
    if (m->h_events)
        (void) hipHostFree(m->h_events);
    counts_free(&m->count);
    free(m);
}

int spangpu_mct_channels(const spangpu_mct_t *m) { return m  ?  m->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_mct_state_words(const spangpu_mct_t *m) { return m  ?  m->c.words  :  SPANGPU_ERR_BAD_ARG; }

int spangpu_mct_set_stream(spangpu_mct_t *m, void *stream)
{
    if (m == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_set_stream(&m->c, stream);
}

int spangpu_mct_sync(spangpu_mct_t *m)
{
    if (m == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&m->c);
}

int spangpu_mct_rx(spangpu_mct_t *m, const int16_t *amp, int mem_kind, int samples, long long stride)
{
    int rc = rx_args_ok(m, mem_kind, amp, samples, &stride);
    if (rc != SPANGPU_OK)
        return rc;
    SPG_TRY(hipSetDevice(m->c.device));
    // a tone needs >= 415 ms to be declared and can only be withdrawn once declared: two reports per ~3300
    // samples at the very most; the preamble hunter needs 40 bits (1067 samples) per declaration
    if ((rc = grow_pair(&m->events, &m->h_events, &m->ev_cap, 8 + samples/256, (size_t) m->c.n_ch*2, m->c.stream)) != SPANGPU_OK)
        return rc;
    MctLaunch L;
    memset(&L, 0, sizeof(L));
    L.st = m->c.st;
    L.quarter = m->quarter;
    L.events = m->events;
    L.ev_count = m->count.dev;
    L.n_ch = m->c.n_ch;
    L.samples = samples;
    L.lens = m->lens.next;
    L.ev_cap = m->ev_cap;
    L.latch = m->latch;
    // the caller's buffer is only borrowed for the call: the copy in is waited for
    if ((rc = stage_in(&m->c, &m->pcm, mem_kind, amp, stride, samples, true, &L.pcm, &L.stride, &L.vec)) != SPANGPU_OK)
        return rc;
    switch (m->tone_type)
    {
    case MCT_FAX_CNG:               launch<MCT_FAX_CNG>(m, L); break;
    case MCT_ANS:                   launch<MCT_ANS>(m, L); break;
    case MCT_FAX_PREAMBLE:          launch<MCT_FAX_PREAMBLE>(m, L); break;
    case MCT_FAX_CED_OR_PREAMBLE:   launch<MCT_FAX_CED_OR_PREAMBLE>(m, L); break;
    case MCT_BELL_ANS:              launch<MCT_BELL_ANS>(m, L); break;
    default:                        launch<MCT_CALLING_TONE>(m, L); break;
    }
    SPG_TRY(hipGetLastError());
    m->last_cap = m->ev_cap;
    return SPANGPU_OK;
}

// spangpu_mct_rx() for a tick in which not every channel has a frame, or frames differ in length: channel c takes lens[c] samples
// of its row (0: it sits the call out, its state as it was, no events).  lens[] is host memory.
int spangpu_mct_rx_var(spangpu_mct_t *m, const int16_t *amp, int mem_kind, const int32_t *lens, int max_samples, long long stride)
{
    if (m == NULL  ||  amp == NULL  ||  lens == NULL  ||  max_samples <= 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int longest;
    bool all;
    int rc = lens_check(lens, m->c.n_ch, max_samples, &longest, &all);
    // nobody brings a sample: no launch; everybody the same: the plain call
    if (rc != SPANGPU_OK  ||  longest == 0)
        return rc;
    if (stride <= 0)
        stride = max_samples;
    if (!all  &&  (rc = lens_upload(&m->c, &m->lens, lens)) != SPANGPU_OK)
        return rc;
    rc = spangpu_mct_rx(m, amp, mem_kind, longest, stride);
    m->lens.next = NULL;
    return rc;
}

int spangpu_mct_events(spangpu_mct_t *m, const int32_t **events, const int32_t **counts)
{
    if (m == NULL  ||  events == NULL  ||  counts == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (m->last_cap <= 0)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no spangpu_mct_rx() yet");
    int rc = counts_fetch(&m->c, &m->count, 1);
    if (rc != SPANGPU_OK)
        return rc;
    // (a count above the capacity is cut short: the entries that fitted are handed out)
    int most;
    (void) count_row_scan(m->count.pinned, m->c.n_ch, m->last_cap, &most);
    if ((rc = rows_fetch(&m->c, m->h_events, m->events, 2*sizeof(int32_t), m->last_cap, most)) != SPANGPU_OK)
        return rc;
    SPG_TRY(hipStreamSynchronize(m->c.stream));
    const int32_t *h_count = m->count.pinned;
    for (int c = 0;  c < m->c.n_ch;  c++)
    {
        int32_t *e = m->h_events + (size_t) c*m->last_cap*2;
        const int cnt = (h_count[c] < m->last_cap)  ?  h_count[c]  :  m->last_cap;
        for (int i = 0;  i < cnt;  i++)
            e[2*i + 1] = level_of(e[2*i], e[2*i + 1]);
    }
    *events = m->h_events;
    *counts = h_count;
    return m->last_cap;
}

int spangpu_mct_get(spangpu_mct_t *m, int channel)
{
    if (m == NULL  ||  !channel_ok(&m->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    // modem_connect_tones_rx_get(), modem_connect_tones.c:793-797: read and clear the latch
    SPG_TRY(hipSetDevice(m->c.device));
    int32_t hit = 0;
    const int32_t zero = 0;
    int32_t *at = m->c.st + (size_t) MC_HIT*m->c.n_ch + channel;
    SPG_TRY(hipMemcpyAsync(&hit, at, sizeof(hit), hipMemcpyDeviceToHost, m->c.stream));
    SPG_TRY(hipMemcpyAsync(at, &zero, sizeof(zero), hipMemcpyHostToDevice, m->c.stream));
    SPG_TRY(hipStreamSynchronize(m->c.stream));
    return hit;
}

int spangpu_mct_get_state(spangpu_mct_t *m, int channel, int32_t *words)
{
    if (m == NULL  ||  words == NULL  ||  !channel_ok(&m->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&m->c, channel, 0, m->c.words, words, false);
}

// The reverse of spangpu_mct_get_state(): a channel's words as a caller holds them.
int spangpu_mct_set_state(spangpu_mct_t *m, int channel, const int32_t *words)
{
    if (m == NULL  ||  words == NULL  ||  !channel_ok(&m->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&m->c, channel, 0, m->c.words, const_cast<int32_t *>(words), true);
}

}   // extern "C"
