// tone_state.hip -- one channel of a tone bank from outside: its state words, a reset, its DTMF parameters, and the
// detectors in the reference's struct layouts (include/spangpu_refstate.h).  No kernel; the struct is tone_bank.hpp.

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu_refstate.h"
#include "tone_bank.hpp"

using namespace spg;

// dtmf_rx_parms(), dtmf.c:421-445, on top of the defaults of dtmf_rx_init() (dtmf.c:470-476).  A field takes effect when
// its bit of set_mask is set and the reference's own test passes (twists >= 0 dB, threshold > -99 dBm0); without
// set_mask (a zeroed struct, or one from a caller built before the mask existed) a positive twist and a non-zero
// threshold do.
void dtmf_levels(const spangpu_tone_params_t &tp, float &threshold, float &normal_twist, float &reverse_twist)
{
    threshold = 171029200.0f;
    normal_twist = 6.309f;
    reverse_twist = 2.512f;
    const bool m = (tp.set_mask != 0);
    if (m  ?  ((tp.set_mask & SPANGPU_TP_TWIST)  &&  tp.twist_db >= 0.0f)  :  (tp.twist_db > 0.0f))
        normal_twist = powf(10.0f, tp.twist_db/10.0f);
    if (m  ?  ((tp.set_mask & SPANGPU_TP_REVERSE_TWIST)  &&  tp.reverse_twist_db >= 0.0f)  :  (tp.reverse_twist_db > 0.0f))
        reverse_twist = powf(10.0f, tp.reverse_twist_db/10.0f);
    if (m  ?  ((tp.set_mask & SPANGPU_TP_THRESHOLD)  &&  tp.threshold_dbm0 > -99.0f)
           :  (tp.threshold_dbm0 > -99.0f  &&  tp.threshold_dbm0 != 0.0f))
        threshold = (float) ((102*102*32768.0f*32768.0f/2.0f)*powf(10.0f, (tp.threshold_dbm0 - 3.14f)/10.0f));
}

// The per-channel parameter table of a DTMF bank, made on first use with the bank's values in every channel
static int ensure_chan_parms(spangpu_bank_t *b)
{
    const size_t n = (size_t) b->c.n_ch;
    if (b->chan_parms)
        return SPANGPU_OK;
    if ((b->h_chan_parms = (float *) malloc(4*n*sizeof(float))) == nullptr)
        return failf(SPANGPU_ERR_NO_MEMORY, "malloc");
    for (size_t c = 0;  c < n;  c++)
    {
        b->h_chan_parms[c] = b->threshold;
        b->h_chan_parms[n + c] = b->normal_twist;
        b->h_chan_parms[2*n + c] = b->reverse_twist;
        b->h_chan_parms[3*n + c] = b->tp.filter_dialtone  ?  1.0f  :  0.0f;
    }
    b->n_filter_on = b->tp.filter_dialtone  ?  b->c.n_ch  :  0;
    float *d = nullptr;
    if (hipMalloc(&d, 4*n*sizeof(float)) != hipSuccess)
    {
        free(b->h_chan_parms);
        b->h_chan_parms = nullptr;
        return failf(SPANGPU_ERR_NO_MEMORY, "hipMalloc of per-channel parameters failed");
    }
    SPG_TRY(hipMemcpy(d, b->h_chan_parms, 4*n*sizeof(float), hipMemcpyHostToDevice));
    b->chan_parms = d;
    return SPANGPU_OK;
}

// One channel's row of that table: the host mirror, the count of filters on, the device's copy through the bank's stream; waits.
static int chan_parms_put(spangpu_bank_t *b, int channel, float threshold, float normal_twist, float reverse_twist, bool filter_on)
{
    const size_t n = (size_t) b->c.n_ch;
    float *h = b->h_chan_parms + channel;
    b->n_filter_on += (int) filter_on - (int) h[3*n];
    h[0] = threshold;
    h[n] = normal_twist;
    h[2*n] = reverse_twist;
    h[3*n] = filter_on  ?  1.0f  :  0.0f;
    for (int i = 0;  i < 4;  i++)
        SPG_TRY(hipMemcpyAsync(b->chan_parms + (size_t) i*n + channel, &h[(size_t) i*n], sizeof(float), hipMemcpyHostToDevice, joined(b)));
    SPG_TRY(hipStreamSynchronize(joined(b)));
    return SPANGPU_OK;
}

extern "C" {

// Parameters of ONE channel of a DTMF bank: what dtmf_rx_parms() (dtmf.c:421-445) does to one detector.  The fields of
// `params` that count are filter_dialtone (< 0: leave as it is; else the notch states of the channel restart, as in
// dtmf.c:428-434), twist_db, reverse_twist_db and threshold_dbm0 under set_mask.  From the first such call on the bank
// carries its thresholds per channel (three loads per channel and block end more); channels never named keep the
// bank's values.
int spangpu_bank_set_channel_params(spangpu_bank_t *b, int channel, const spangpu_tone_params_t *params, size_t params_size)
{
    if (b == nullptr  ||  params == nullptr  ||  channel < 0  ||  channel >= b->c.n_ch)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (b->kind != SPANGPU_DTMF)
        return failf(SPANGPU_ERR_UNSUPPORTED, "per-channel parameters exist for DTMF banks only");
    spangpu_tone_params_t tp;
    memset(&tp, 0, sizeof(tp));
    memcpy(&tp, params, (params_size < sizeof(tp))  ?  params_size  :  sizeof(tp));
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipStreamSynchronize(joined(b)));
    const size_t n = (size_t) b->c.n_ch;
    const int rc0 = ensure_chan_parms(b);
    if (rc0 != SPANGPU_OK)
        return rc0;
    // the channel's present values stand where the call leaves a field alone
    const float *h = b->h_chan_parms + channel;
    spangpu_tone_params_t q = tp;
    if (q.set_mask == 0)
        q.set_mask = ((q.twist_db > 0.0f)  ?  SPANGPU_TP_TWIST  :  0)  |  ((q.reverse_twist_db > 0.0f)  ?  SPANGPU_TP_REVERSE_TWIST  :  0)
                     |  ((q.threshold_dbm0 > -99.0f  &&  q.threshold_dbm0 != 0.0f)  ?  SPANGPU_TP_THRESHOLD  :  0)  |  0x40000000;
    float thr, nt, rt;
    dtmf_levels(q, thr, nt, rt);
    if (!((q.set_mask & SPANGPU_TP_THRESHOLD)  &&  q.threshold_dbm0 > -99.0f))
        thr = h[0];
    if (!((q.set_mask & SPANGPU_TP_TWIST)  &&  q.twist_db >= 0.0f))
        nt = h[n];
    if (!((q.set_mask & SPANGPU_TP_REVERSE_TWIST)  &&  q.reverse_twist_db >= 0.0f))
        rt = h[2*n];
    if (tp.filter_dialtone >= 0)
    {
        for (int i = 0;  i < 4;  i++)
            SPG_TRY(hipMemsetAsync(b->sf + (size_t) (17 + i)*n + channel, 0, sizeof(float), joined(b)));
    }
    return chan_parms_put(b, channel, thr, nt, rt, (tp.filter_dialtone >= 0)  ?  (tp.filter_dialtone != 0)  :  (h[3*n] != 0.0f));
}

// State import/export: fstate[nsf] in device order (v2[nb], v3[nb], [energy], [z350[2], z440[2]]),
// istate[4] = {current_sample, w0 byte 2, w0 byte 3, w1}.
int spangpu_bank_get_state(spangpu_bank_t *b, int channel, float *fstate, int max_f, int32_t *istate, int max_i)
{
    if (b == nullptr  ||  channel < 0  ||  channel >= b->c.n_ch  ||  max_f < b->nsf  ||  max_i < 4)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipStreamSynchronize(joined(b)));
    SPG_TRY(hipMemcpy2D(fstate, sizeof(float), b->sf + channel, (size_t) b->c.n_ch*sizeof(float),
                        sizeof(float), b->nsf, hipMemcpyDeviceToHost));
    int32_t w[2];
    SPG_TRY(hipMemcpy2D(w, sizeof(int32_t), b->si + channel, (size_t) b->c.n_ch*sizeof(int32_t),
                        sizeof(int32_t), 2, hipMemcpyDeviceToHost));
    istate[0] = w[0] & 0xFFFF;
    istate[1] = (w[0] >> 16) & 0xFF;
    istate[2] = (w[0] >> 24) & 0xFF;
    istate[3] = w[1];
    return b->nsf;
}

int spangpu_bank_set_state(spangpu_bank_t *b, int channel, const float *fstate, int n_f, const int32_t *istate, int n_i)
{
    if (b == nullptr  ||  channel < 0  ||  channel >= b->c.n_ch  ||  n_f != b->nsf  ||  n_i != 4)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipStreamSynchronize(joined(b)));
    SPG_TRY(hipMemcpy2D(b->sf + channel, (size_t) b->c.n_ch*sizeof(float), fstate, sizeof(float),
                        sizeof(float), b->nsf, hipMemcpyHostToDevice));
    int32_t w[2];
    w[0] = (istate[0] & 0xFFFF) | ((istate[1] & 0xFF) << 16) | ((int32_t) ((uint32_t) (istate[2] & 0xFF) << 24));
    w[1] = istate[3];
    SPG_TRY(hipMemcpy2D(b->si + channel, (size_t) b->c.n_ch*sizeof(int32_t), w, sizeof(int32_t),
                        sizeof(int32_t), 2, hipMemcpyHostToDevice));
    return SPANGPU_OK;
}

// ---- one DTMF channel in the reference's struct layout (include/spangpu_refstate.h; src/spandsp/private/dtmf.h:54-117) --
int spangpu_dtmf_import_state(spangpu_bank_t *b, int channel, const spangpu_ref_dtmf_rx_t *s)
{
    if (b == nullptr  ||  s == nullptr  ||  channel < 0  ||  channel >= b->c.n_ch  ||  b->kind != SPANGPU_DTMF)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    float f[21];
    int32_t w[4];
    for (int i = 0;  i < 4;  i++)
    {
        f[i] = s->row_out[i].v2;
        f[4 + i] = s->col_out[i].v2;
        f[8 + i] = s->row_out[i].v3;
        f[12 + i] = s->col_out[i].v3;
    }
    f[16] = s->energy;
    f[17] = s->z350[0];
    f[18] = s->z350[1];
    f[19] = s->z440[0];
    f[20] = s->z440[1];
    w[0] = s->current_sample;
    w[1] = s->last_hit;
    w[2] = s->in_digit;
    w[3] = s->duration;
    int rc = spangpu_bank_set_state(b, channel, f, 21, w, 4);
    if (rc != SPANGPU_OK)
        return rc;
    // the detector's own thresholds: the bank's table takes them as they stand
    const bool differs = s->threshold != b->threshold  ||  s->normal_twist != b->normal_twist  ||  s->reverse_twist != b->reverse_twist
                         ||  (s->filter_dialtone  ?  1  :  0) != (b->tp.filter_dialtone  ?  1  :  0);
    if (b->chan_parms == nullptr  &&  !differs)
        return SPANGPU_OK;
    if ((rc = ensure_chan_parms(b)) != SPANGPU_OK)
        return rc;
    return chan_parms_put(b, channel, s->threshold, s->normal_twist, s->reverse_twist, s->filter_dialtone != 0);
}

int spangpu_dtmf_export_state(spangpu_bank_t *b, int channel, spangpu_ref_dtmf_rx_t *s)
{
    if (b == nullptr  ||  s == nullptr  ||  channel < 0  ||  channel >= b->c.n_ch  ||  b->kind != SPANGPU_DTMF)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    float f[2*kToneMaxBins + 8];
    int32_t w[4];
    const int rc = spangpu_bank_get_state(b, channel, f, 2*kToneMaxBins + 8, w, 4);
    if (rc < 0)
        return rc;
    const size_t n = (size_t) b->c.n_ch;
    for (int i = 0;  i < 4;  i++)
    {
        // dtmf_rx() drives its Goertzels through goertzel_samplex(): their own sample counters stay where
        // goertzel_init() left them (tone_detect.c:96-106), the block phase is the detector's current_sample
        s->row_out[i].v2 = f[i];
        s->col_out[i].v2 = f[4 + i];
        s->row_out[i].v3 = f[8 + i];
        s->col_out[i].v3 = f[12 + i];
        s->row_out[i].fac = b->fac[i];
        s->col_out[i].fac = b->fac[4 + i];
        s->row_out[i].samples = s->col_out[i].samples = 102;
        s->row_out[i].current_sample = s->col_out[i].current_sample = 0;
    }
    s->energy = f[16];
    s->z350[0] = f[17];
    s->z350[1] = f[18];
    s->z440[0] = f[19];
    s->z440[1] = f[20];
    s->current_sample = w[0];
    s->last_hit = (uint8_t) w[1];
    s->in_digit = (uint8_t) w[2];
    s->duration = w[3];
    if (b->chan_parms)
    {
        const float *h = b->h_chan_parms;
        s->threshold = h[channel];
        s->normal_twist = h[n + channel];
        s->reverse_twist = h[2*n + channel];
        s->filter_dialtone = (h[3*n + channel] != 0.0f);
    }
    else
    {
        s->threshold = b->threshold;
        s->normal_twist = b->normal_twist;
        s->reverse_twist = b->reverse_twist;
        s->filter_dialtone = (b->tp.filter_dialtone != 0);
    }
    return SPANGPU_OK;
}

// ---- Bell MF and MFC/R2 detectors in the reference's struct layout (src/spandsp/private/bell_r2_mf.h:62-116).  Both
// drive their six Goertzels through goertzel_samplex(), like dtmf_rx(): the block position is the detector's own
// current_sample, the Goertzels' counters stay where goertzel_init() left them.
int spangpu_bell_mf_import_state(spangpu_bank_t *b, int channel, const spangpu_ref_bell_mf_rx_t *s)
{
    if (b == nullptr  ||  s == nullptr  ||  channel < 0  ||  channel >= b->c.n_ch  ||  b->kind != SPANGPU_BELL_MF)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    float f[12];
    int32_t w[4];
    for (int i = 0;  i < 6;  i++)
    {
        f[i] = s->out[i].v2;
        f[6 + i] = s->out[i].v3;
    }
    // bell_r2_mf.c:629-661: hits[0] is the oldest of the five block results kept
    w[0] = s->current_sample;
    w[1] = s->hits[0];
    w[2] = s->hits[1];
    w[3] = (int32_t) ((uint32_t) s->hits[2] | ((uint32_t) s->hits[3] << 8) | ((uint32_t) s->hits[4] << 16));
    return spangpu_bank_set_state(b, channel, f, 12, w, 4);
}

int spangpu_bell_mf_export_state(spangpu_bank_t *b, int channel, spangpu_ref_bell_mf_rx_t *s)
{
    if (b == nullptr  ||  s == nullptr  ||  channel < 0  ||  channel >= b->c.n_ch  ||  b->kind != SPANGPU_BELL_MF)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    float f[2*kToneMaxBins + 8];
    int32_t w[4];
    const int rc = spangpu_bank_get_state(b, channel, f, 2*kToneMaxBins + 8, w, 4);
    if (rc < 0)
        return rc;
    for (int i = 0;  i < 6;  i++)
    {
        s->out[i].v2 = f[i];
        s->out[i].v3 = f[6 + i];
        s->out[i].fac = b->fac[i];
        s->out[i].samples = 120;
        s->out[i].current_sample = 0;
    }
    s->current_sample = w[0];
    s->hits[0] = (uint8_t) w[1];
    s->hits[1] = (uint8_t) w[2];
    s->hits[2] = (uint8_t) (w[3] & 0xFF);
    s->hits[3] = (uint8_t) ((w[3] >> 8) & 0xFF);
    s->hits[4] = (uint8_t) ((w[3] >> 16) & 0xFF);
    return SPANGPU_OK;
}

int spangpu_r2_mf_import_state(spangpu_bank_t *b, int channel, const spangpu_ref_r2_mf_rx_t *s)
{
    if (b == nullptr  ||  s == nullptr  ||  channel < 0  ||  channel >= b->c.n_ch  ||  b->kind != SPANGPU_R2_MF)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if ((s->fwd  ?  1  :  0) != (b->tp.r2_fwd  ?  1  :  0))
        return failf(SPANGPU_ERR_BAD_ARG, "the detector listens for the other direction's tones");
    float f[12];
    int32_t w[4];
    for (int i = 0;  i < 6;  i++)
    {
        f[i] = s->out[i].v2;
        f[6 + i] = s->out[i].v3;
    }
    w[0] = s->current_sample;
    w[1] = s->current_digit & 0xFF;
    w[2] = 0;
    w[3] = 0;
    return spangpu_bank_set_state(b, channel, f, 12, w, 4);
}

int spangpu_r2_mf_export_state(spangpu_bank_t *b, int channel, spangpu_ref_r2_mf_rx_t *s)
{
    if (b == nullptr  ||  s == nullptr  ||  channel < 0  ||  channel >= b->c.n_ch  ||  b->kind != SPANGPU_R2_MF)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if ((s->fwd  ?  1  :  0) != (b->tp.r2_fwd  ?  1  :  0))
        return failf(SPANGPU_ERR_BAD_ARG, "the detector listens for the other direction's tones");
    float f[2*kToneMaxBins + 8];
    int32_t w[4];
    const int rc = spangpu_bank_get_state(b, channel, f, 2*kToneMaxBins + 8, w, 4);
    if (rc < 0)
        return rc;
    for (int i = 0;  i < 6;  i++)
    {
        s->out[i].v2 = f[i];
        s->out[i].v3 = f[6 + i];
        s->out[i].fac = b->fac[i];
        s->out[i].samples = 133;
        s->out[i].current_sample = 0;
    }
    s->current_sample = w[0];
    s->current_digit = w[1];
    return SPANGPU_OK;
}

int spangpu_bank_reset_channel(spangpu_bank_t *b, int channel, int fillin_only)
{
    if (b == nullptr  ||  channel < 0  ||  channel >= b->c.n_ch)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    float f[2*kToneMaxBins + 8];
    int32_t w[4];
    int rc = spangpu_bank_get_state(b, channel, f, 2*kToneMaxBins + 8, w, 4);
    if (rc < 0)
        return rc;
    // Goertzel states, block energy and block position always restart (dtmf.c:363-379);
    // a full reset also clears the filters and the hit history (dtmf.c:447-504).
    const int nclear = (fillin_only)  ?  (2*b->nb + ((b->nsf > 2*b->nb)  ?  1  :  0))  :  b->nsf;
    for (int i = 0;  i < nclear;  i++)
        f[i] = 0.0f;
    w[0] = 0;
    if (!fillin_only)
        w[1] = w[2] = w[3] = 0;
    rc = spangpu_bank_set_state(b, channel, f, b->nsf, w, 4);
    if (rc < 0  ||  fillin_only  ||  b->h_chan_parms == nullptr)
        return rc;
    // A full reset is an init: the thresholds, twists and dial-tone filter an earlier dtmf_rx_parms() gave this channel go
    // back to the bank's (dtmf.c:447-504 sets them afresh), as ensure_chan_parms() first laid them out.
    return chan_parms_put(b, channel, b->threshold, b->normal_twist, b->reverse_twist, b->tp.filter_dialtone != 0);
}

}   // extern "C"
