/*
 * shim_fsk.c -- host side (plain C) of the spandsp-named entry points for the FSK receiver, the modem connect
 * tone detector and the DTMF sender, declared in include/spangpu_spandsp.h: fsk_rx*, modem_connect_tones_rx*,
 * dtmf_tx*.  No signal processing happens here: samples go to (or come from) a bank of include/spangpu.h, the
 * HIP kernel leaves each channel's put_bit / tone report stream in order, and this file replays it through the
 * caller's callbacks as the reference would (src/fsk.c:343-391, src/modem_connect_tones.c:416-435).
 * Without a GPU every init returns NULL: there is no CPU implementation.
 */
#include <math.h>

#include "spangpu_spandsp.h"
#include "shim_group.h"
#include "shim_object.h"

/* preset_fsk_specs[], src/fsk.c:60-155 */
const fsk_spec_t preset_fsk_specs[] =
{
    {"V21 ch 1", 1080 + 100, 1080 - 100, -14, -30, 300*100},
    {"V21 ch 2", 1750 + 100, 1750 - 100, -14, -30, 300*100},
    {"V23 ch 1", 1700 + 400, 1700 - 400, -14, -30, 1200*100},
    {"V23 ch 2", 420 + 30, 420 - 30, -14, -30, 75*100},
    {"Bell103 ch 1", 1170 - 100, 1170 + 100, -14, -30, 300*100},
    {"Bell103 ch 2", 2125 - 100, 2125 + 100, -14, -30, 300*100},
    {"Bell202", 1700 + 500, 1700 - 500, -14, -30, 1200*100},
    {"Weitbrecht 45.45", 1600 + 200, 1600 - 200, -14, -30, 4545},
    {"Weitbrecht 50", 1600 + 200, 1600 - 200, -14, -30, 50*100},
    {"Weitbrecht 47.6", 1600 + 200, 1600 - 200, -14, -30, 4760},
    {"V21 (110bps) ch 1", 1080 + 100, 1080 - 100, -14, -30, 110*100}
};

/* ---- one staging group for both receiver kinds ---------------------------------------------------------- */
struct spangpu_line_group_s
{
    grp_core_t core;            /* the staging protocol: shim_group.h */
    int is_mct;
    spangpu_fsk_t *fsk;
    spangpu_mct_t *mct;
    spangpu_fsk_spec_t spec;
    int tone_type;
    int16_t *stage;
    int32_t *pristine;          /* a channel's words as the bank was created: what xxx_rx_init() leaves, default cutoff included */
    /* the results of the tick being delivered (views into the bank's buffers) */
    const int16_t *fsk_events;
    const int32_t *mct_events;
    const int32_t *counts;
    int cap;
};

static spangpu_line_group_t *group_new(int n_channels, int max_samples, int (*run_tick)(grp_core_t *), void (*deliver)(grp_core_t *))
{
    spangpu_line_group_t *g;

    if (n_channels <= 0  ||  max_samples <= 0  ||  (g = (spangpu_line_group_t *) calloc(1, sizeof(*g))) == NULL)
        return NULL;
    g->stage = (int16_t *) calloc((size_t) n_channels*max_samples, sizeof(int16_t));
    if (grp_init(&g->core, n_channels, max_samples, run_tick, deliver) < 0  ||  g->stage == NULL)
    {
        spangpu_line_group_destroy(g);
        return NULL;
    }
    return g;
}

/* The tick of an FSK group: the launch and a view of each channel's put_bit / status stream ... */
static int fsk_run(grp_core_t *core)
{
    spangpu_line_group_t *g = (spangpu_line_group_t *) core;
    const int rc = spangpu_fsk_rx_var(g->fsk, g->stage, SPANGPU_MEM_HOST, core->lens, core->max_samples, core->max_samples);

    return g->cap = (rc < 0)  ?  rc  :  spangpu_fsk_events(g->fsk, &g->fsk_events, &g->counts);
}

/* ... replayed */
static void fsk_deliver(grp_core_t *core)
{
    spangpu_line_group_t *g = (spangpu_line_group_t *) core;
    const int cap = g->cap;
    int c;
    int i;
    int n;

    for (c = 0;  c < core->n_ch;  c++)
    {
        fsk_rx_state_t *s = (fsk_rx_state_t *) core->handles[c];

        n = (g->counts[c] < cap)  ?  g->counts[c]  :  cap;
        if (s  &&  core->run[c] > 0)
        {
            for (i = 0;  i < n;  i++)
            {
                const int v = g->fsk_events[(size_t) c*cap + i];

                /* report_status_change(), fsk.c:343-349: the status handler if there is one, else put_bit */
                if (v < 0  &&  s->status_handler)
                    s->status_handler(s->status_user_data, v);
                else if (s->put_bit)
                    s->put_bit(s->put_bit_user_data, v);
            }
        }
    }
}

/* The same pair for a connect-tone group: (tone, level) reports */
static int mct_run(grp_core_t *core)
{
    spangpu_line_group_t *g = (spangpu_line_group_t *) core;
    const int rc = spangpu_mct_rx_var(g->mct, g->stage, SPANGPU_MEM_HOST, core->lens, core->max_samples, core->max_samples);

    return g->cap = (rc < 0)  ?  rc  :  spangpu_mct_events(g->mct, &g->mct_events, &g->counts);
}

static void mct_deliver(grp_core_t *core)
{
    spangpu_line_group_t *g = (spangpu_line_group_t *) core;
    const int cap = g->cap;
    int c;
    int i;
    int n;

    for (c = 0;  c < core->n_ch;  c++)
    {
        modem_connect_tones_rx_state_t *s = (modem_connect_tones_rx_state_t *) core->handles[c];

        n = (g->counts[c] < cap)  ?  g->counts[c]  :  cap;
        if (s  &&  s->tone_callback  &&  core->run[c] > 0)
        {
            /* report_tone_state(), modem_connect_tones.c:420-423 */
            for (i = 0;  i < n;  i++)
                s->tone_callback(s->callback_data, g->mct_events[((size_t) c*cap + i)*2], g->mct_events[((size_t) c*cap + i)*2 + 1], 0);
        }
    }
}

spangpu_line_group_t *spangpu_fsk_group_create(int device, const fsk_spec_t *spec, int framing_mode, int n_channels, int max_samples)
{
    spangpu_line_group_t *g;

    if (spec == NULL  ||  (g = group_new(n_channels, max_samples, fsk_run, fsk_deliver)) == NULL)
        return NULL;
    g->spec.freq_zero = spec->freq_zero;
    g->spec.freq_one = spec->freq_one;
    g->spec.tx_level = spec->tx_level;
    g->spec.min_level = spec->min_level;
    g->spec.baud_rate = spec->baud_rate;
    if (spangpu_fsk_create(&g->fsk, device, n_channels, &g->spec, framing_mode) != SPANGPU_OK
        ||  (g->pristine = (int32_t *) calloc(spangpu_fsk_state_words(g->fsk), sizeof(int32_t))) == NULL
        ||  spangpu_fsk_get_state(g->fsk, 0, g->pristine) < 0)
    {
        spangpu_line_group_destroy(g);
        return NULL;
    }
    return g;
}

spangpu_line_group_t *spangpu_modem_connect_tones_group_create(int device, int tone_type, int use_callbacks, int n_channels,
                                                                int max_samples)
{
    spangpu_line_group_t *g;

    if ((g = group_new(n_channels, max_samples, mct_run, mct_deliver)) == NULL)
        return NULL;
    g->is_mct = 1;
    g->tone_type = tone_type;
    if (spangpu_mct_create(&g->mct, device, tone_type, n_channels, use_callbacks) != SPANGPU_OK
        ||  (g->pristine = (int32_t *) calloc(spangpu_mct_state_words(g->mct), sizeof(int32_t))) == NULL
        ||  spangpu_mct_get_state(g->mct, 0, g->pristine) < 0)
    {
        spangpu_line_group_destroy(g);
        return NULL;
    }
    return g;
}

int spangpu_line_group_destroy(spangpu_line_group_t *g)
{
    if (g == NULL)
        return 0;
    if (g->fsk)
        spangpu_fsk_destroy(g->fsk);
    if (g->mct)
        spangpu_mct_destroy(g->mct);
    free(g->stage);
    free(g->pristine);
    grp_free(&g->core);
    free(g);
    return 0;
}

int spangpu_line_group_flush(spangpu_line_group_t *g)
{
    return (g)  ?  grp_flush(&g->core)  :  SPANGPU_ERR_BAD_ARG;
}

/* A shared bank stages one frame per receiver and tick (any thread; one submitter per receiver); the tick runs when every
   attached receiver has staged, or when its owner calls spangpu_line_group_flush() at the deadline.  A frame longer than
   the group was made for, or a second frame for a receiver before the tick has run, is refused with -1 (a tone group tells
   the two apart): nothing is dropped silently. */
static int line_stage(grp_core_t *core, int channel, const int16_t amp[], int len)
{
    spangpu_line_group_t *g = (spangpu_line_group_t *) core;

    if (len > core->max_samples  ||  grp_stage_begin(core, channel) < 0)
        return -1;
    memcpy(g->stage + (size_t) channel*core->max_samples, amp, len*sizeof(int16_t));
    return (grp_stage_commit(core, channel, len) < 0)  ?  -1  :  0;
}

/* A piece of a private object's buffer: a tick that fails is not reported, and the pieces after it still run (a tone
   object stops at the first and returns -1). */
static int line_stage_private(grp_core_t *core, int channel, const int16_t amp[], int len)
{
    (void) line_stage(core, channel, amp, len);
    return 0;
}

/* One object's frame: a shared bank stages it, a private one runs it now (in slices). */
static int line_rx(spangpu_line_group_t *g, int channel, int private_grp, const int16_t amp[], int len)
{
    if (len <= 0)
        return 0;                           /* as the reference: nothing to do (fsk.c:330 loops over len) */
    if (!private_grp)
        return line_stage(&g->core, channel, amp, len);
    /* Called from inside its own callback: refused, not dropped (a tone object's frame is accepted, and runs when the
       delivery is over). */
    if (grp_in_callback(&g->core))
        return -1;
    return grp_feed_private(&g->core, amp, len, line_stage_private);
}

/* The slot is released whether or not it is held (a tone group looks first); a private object detaches, then destroys its
   group (a tone object only destroys it). */
static void line_detach(spangpu_line_group_t *g, int channel, int private_grp)
{
    grp_release(&g->core, channel);
    if (private_grp)
        spangpu_line_group_destroy(g);
}

/* The channel of a slot being claimed on a shared bank gets the words of a fresh receiver -- the slot may have served an
   earlier call whose object was freed mid-signal, with a cutoff of its own (fsk.c:723-742 and modem_connect_tones.c:799-857
   start from a memset()).  If that fails the attach is refused (a tone group does not look). */
static int line_fresh(grp_core_t *core, int channel, void *arg)
{
    spangpu_line_group_t *g = (spangpu_line_group_t *) core;

    (void) arg;
    return g->is_mct  ?  spangpu_mct_set_state(g->mct, channel, g->pristine)  :  spangpu_fsk_set_state(g->fsk, channel, g->pristine);
}

/* A private object's bank is new, and is left as it was made. */
static int line_attach(spangpu_line_group_t *g, int channel, int private_grp, void *handle)
{
    return grp_claim(&g->core, channel, handle, (private_grp)  ?  NULL  :  line_fresh, NULL);
}

/* ---- fsk_rx -------------------------------------------------------------------------------------------- */
static fsk_rx_state_t *fsk_obj(fsk_rx_state_t *s, spangpu_line_group_t *g, int channel, int private_grp, span_put_bit_func_t put_bit,
                               void *user_data)
{
    const int mine = (s != NULL);

    if (mine)
        memset(s, 0, sizeof(*s));
    else if ((s = (fsk_rx_state_t *) calloc(1, sizeof(*s))) == NULL)
        return NULL;
    s->caller_storage = mine;
    s->grp = g;
    s->channel = channel;
    s->private_grp = private_grp;
    s->put_bit = put_bit;
    s->put_bit_user_data = user_data;
    if (line_attach(g, channel, private_grp, s) < 0)
    {
        if (!mine)
            free(s);
        return NULL;
    }
    return s;
}

fsk_rx_state_t *fsk_rx_init(fsk_rx_state_t *s, const fsk_spec_t *spec, int framing_mode, span_put_bit_func_t put_bit, void *user_data)
{
    spangpu_line_group_t *g;

    /* s != NULL: the caller's storage (fsk.c:725-733); the handle goes there, the receiver itself is a private one-channel bank */
    if ((g = spangpu_fsk_group_create(0, spec, framing_mode, 1, 4096)) == NULL)
        return NULL;
    if ((s = fsk_obj(s, g, 0, 1, put_bit, user_data)) == NULL)
        spangpu_line_group_destroy(g);
    return s;
}

fsk_rx_state_t *spangpu_fsk_rx_attach(spangpu_line_group_t *g, int channel, span_put_bit_func_t put_bit, void *user_data)
{
    if (g == NULL  ||  g->is_mct  ||  channel < 0  ||  channel >= g->core.n_ch)
        return NULL;
    return fsk_obj(NULL, g, channel, 0, put_bit, user_data);
}

int fsk_rx(fsk_rx_state_t *s, const int16_t *amp, int len)
{
    return line_rx(s->grp, s->channel, s->private_grp, amp, len);
}

int fsk_rx_fillin(fsk_rx_state_t *s, int len)
{
    return (spangpu_fsk_fillin(s->grp->fsk, s->channel, len) < 0)  ?  -1  :  0;
}

int fsk_rx_restart(fsk_rx_state_t *s, const fsk_spec_t *spec, int framing_mode)
{
    if (spec == NULL)
        return -1;
    if (spec->freq_zero != s->grp->spec.freq_zero  ||  spec->freq_one != s->grp->spec.freq_one
        ||  spec->baud_rate != s->grp->spec.baud_rate  ||  spec->min_level != s->grp->spec.min_level)
    {
        /* Another modem (fsk.c:670-723 re-initialises everything but the callbacks).  A bank runs one spec -- its window
           length follows the baud rate -- so an object on a shared bank cannot leave it; an object of its own gets a new
           one-channel bank. */
        spangpu_line_group_t *g;

        if (!s->private_grp)
            return -1;
        if ((g = spangpu_fsk_group_create(0, spec, framing_mode, 1, 4096)) == NULL)
            return -1;
        line_detach(s->grp, s->channel, 1);
        s->grp = g;
        s->channel = 0;
        return line_attach(g, 0, 1, s);
    }
    return (spangpu_fsk_restart(s->grp->fsk, s->channel, framing_mode) < 0)  ?  -1  :  0;
}

int fsk_rx_release(fsk_rx_state_t *s)
{
    /* what ends an object in the caller's storage: its place on the bank (or its private bank) goes, the storage stays */
    if (s  &&  s->grp)
    {
        line_detach(s->grp, s->channel, s->private_grp);
        s->grp = NULL;
    }
    return 0;
}

int fsk_rx_free(fsk_rx_state_t *s)
{
    if (s == NULL)
        return 0;
    fsk_rx_release(s);
    if (!s->caller_storage)
        free(s);
    return 0;
}

void fsk_rx_set_put_bit(fsk_rx_state_t *s, span_put_bit_func_t put_bit, void *user_data)
{
    s->put_bit = put_bit;
    s->put_bit_user_data = user_data;
}

void fsk_rx_set_modem_status_handler(fsk_rx_state_t *s, span_modem_status_func_t handler, void *user_data)
{
    s->status_handler = handler;
    s->status_user_data = user_data;
}

void fsk_rx_set_signal_cutoff(fsk_rx_state_t *s, float cutoff)
{
    spangpu_fsk_set_signal_cutoff(s->grp->fsk, s->channel, cutoff);
}

void fsk_rx_set_frame_parameters(fsk_rx_state_t *s, int data_bits, int parity, int stop_bits)
{
    spangpu_fsk_set_frame_parameters(s->grp->fsk, s->channel, data_bits, parity, stop_bits);
}

/* State word positions (fsk_dev.hpp): 8 power reading, 26 parity errors, 27 framing errors */
static int fsk_word(fsk_rx_state_t *s, int idx, int reset)
{
    int32_t w[28 + 4*128];
    int v;

    if (spangpu_fsk_get_state(s->grp->fsk, s->channel, w) < 0)
        return 0;
    v = w[idx];
    if (reset  &&  v != 0)
    {
        w[idx] = 0;
        spangpu_fsk_set_state(s->grp->fsk, s->channel, w);
    }
    return v;
}

float fsk_rx_signal_power(fsk_rx_state_t *s)
{
    /* power_meter_current_dbm0(), power_meter.c:114-121 */
    const int32_t reading = fsk_word(s, 8, 0);

    if (reading <= 0)
        return -96.329f + (3.14f + 3.02f);
    return 10.0f*log10f((float) reading/(32767.0f*32767.0f) + 1.0e-10f) + (3.14f + 3.02f);
}

int fsk_rx_get_parity_errors(fsk_rx_state_t *s, bool reset)
{
    return fsk_word(s, 26, reset);
}

int fsk_rx_get_framing_errors(fsk_rx_state_t *s, bool reset)
{
    return fsk_word(s, 27, reset);
}

/* ---- modem_connect_tones_rx ---------------------------------------------------------------------------- */
static modem_connect_tones_rx_state_t *mct_obj(modem_connect_tones_rx_state_t *s, spangpu_line_group_t *g, int channel, int private_grp,
                                               span_tone_report_func_t tone_callback, void *user_data)
{
    const int mine = (s != NULL);

    if (mine)
        memset(s, 0, sizeof(*s));
    else if ((s = (modem_connect_tones_rx_state_t *) calloc(1, sizeof(*s))) == NULL)
        return NULL;
    s->caller_storage = mine;
    s->grp = g;
    s->channel = channel;
    s->private_grp = private_grp;
    s->tone_callback = tone_callback;
    s->callback_data = user_data;
    if (line_attach(g, channel, private_grp, s) < 0)
    {
        if (!mine)
            free(s);
        return NULL;
    }
    return s;
}

modem_connect_tones_rx_state_t *modem_connect_tones_rx_init(modem_connect_tones_rx_state_t *s, int tone_type,
                                                            span_tone_report_func_t tone_callback, void *user_data)
{
    spangpu_line_group_t *g;

    /* s != NULL: the caller's storage (modem_connect_tones.c:823-830) */
    if ((g = spangpu_modem_connect_tones_group_create(0, tone_type, tone_callback != NULL, 1, 4096)) == NULL)
        return NULL;
    if ((s = mct_obj(s, g, 0, 1, tone_callback, user_data)) == NULL)
        spangpu_line_group_destroy(g);
    return s;
}

modem_connect_tones_rx_state_t *spangpu_modem_connect_tones_rx_attach(spangpu_line_group_t *g, int channel,
                                                                      span_tone_report_func_t tone_callback, void *user_data)
{
    if (g == NULL  ||  !g->is_mct  ||  channel < 0  ||  channel >= g->core.n_ch)
        return NULL;
    return mct_obj(NULL, g, channel, 0, tone_callback, user_data);
}

int modem_connect_tones_rx(modem_connect_tones_rx_state_t *s, const int16_t amp[], int len)
{
    return line_rx(s->grp, s->channel, s->private_grp, amp, len);
}

int modem_connect_tones_rx_fillin(modem_connect_tones_rx_state_t *s, int len)
{
    /* modem_connect_tones.c:787-790: nothing to do */
    (void) s;
    (void) len;
    return 0;
}

int modem_connect_tones_rx_get(modem_connect_tones_rx_state_t *s)
{
    const int hit = spangpu_mct_get(s->grp->mct, s->channel);

    return (hit < 0)  ?  MODEM_CONNECT_TONES_NONE  :  hit;
}

int modem_connect_tones_rx_release(modem_connect_tones_rx_state_t *s)
{
    if (s  &&  s->grp)
    {
        line_detach(s->grp, s->channel, s->private_grp);
        s->grp = NULL;
    }
    return 0;
}

int modem_connect_tones_rx_free(modem_connect_tones_rx_state_t *s)
{
    if (s == NULL)
        return 0;
    modem_connect_tones_rx_release(s);
    if (!s->caller_storage)
        free(s);
    return 0;
}

const char *modem_connect_tone_to_str(int tone)
{
    /* modem_connect_tones.c:84-112 */
    static const char *names[] =
    {
        "No tone", "FAX CNG", "ANS or FAX CED", "ANS/", "ANSam", "ANSam/", "FAX preamble", "FAX CED or preamble", "Bell ANS",
        "Calling tone"
    };
    return (tone >= 0  &&  tone <= MODEM_CONNECT_TONES_CALLING_TONE)  ?  names[tone]  :  "???";
}

/* ---- dtmf_tx: one private sender per object ---------------------------------------------------------- */
dtmf_tx_state_t *dtmf_tx_init(dtmf_tx_state_t *s, digits_tx_callback_t callback, void *user_data)
{
    spangpu_txbank_t *bank;

    if (spangpu_txbank_create(&bank, 0, SPANGPU_TX_DTMF, 1) != SPANGPU_OK)
        return NULL;
    if ((s = OBJ_TAKE(s, dtmf_tx_state_t)) == NULL)
    {
        spangpu_txbank_destroy(bank);
        return NULL;
    }
    s->bank = bank;
    s->callback = callback;
    s->callback_data = user_data;
    return s;
}

int dtmf_tx_release(dtmf_tx_state_t *s)
{
    if (s  &&  s->bank)
    {
        spangpu_txbank_destroy(s->bank);
        s->bank = NULL;
    }
    return 0;
}

int dtmf_tx_free(dtmf_tx_state_t *s)
{
    if (s)
    {
        dtmf_tx_release(s);
        obj_drop(&s->obj, s);
    }
    return 0;
}

void dtmf_tx_set_level(dtmf_tx_state_t *s, int level, int twist)
{
    spangpu_txbank_set_level(s->bank, 0, 1, level, twist);
}

void dtmf_tx_set_timing(dtmf_tx_state_t *s, int on_time, int off_time)
{
    spangpu_txbank_set_timing(s->bank, 0, 1, on_time, off_time);
}

int dtmf_tx_put(dtmf_tx_state_t *s, const char *digits, int len)
{
    const int rc = spangpu_txbank_put(s->bank, 0, 1, digits, len);

    if (rc == 0)
        s->puts++;
    return (rc < 0)  ?  -1  :  rc;
}

int dtmf_tx(dtmf_tx_state_t *s, int16_t amp[], int max_samples)
{
    int len = 0;

    if (max_samples <= 0)
        return 0;
    for (;;)
    {
        int got = 0;
        int before;

        if (spangpu_txbank_tx(s->bank, SPANGPU_MEM_HOST, amp + len, max_samples - len, max_samples - len, &got) < 0)
            break;
        len += got;
        /* dtmf.c:566-573: the queue ran dry with room left in the buffer -- "see if we can get some more digits": the
           callback answers by calling dtmf_tx_put(), and the sender carries on where it stopped */
        if (len >= max_samples  ||  s->callback == NULL)
            break;
        before = s->puts;
        s->callback(s->callback_data);
        if (s->puts == before)
            break;
    }
    return len;
}

/* ---- bell_mf_tx / r2_mf_tx: one private sender per object (src/bell_r2_mf.c:281-372, 386-462) ----------------- */
bell_mf_tx_state_t *bell_mf_tx_init(bell_mf_tx_state_t *s)
{
    spangpu_txbank_t *bank;

    if (spangpu_txbank_create(&bank, 0, SPANGPU_TX_BELL_MF, 1) != SPANGPU_OK)
        return NULL;
    if ((s = OBJ_TAKE(s, bell_mf_tx_state_t)) == NULL)
    {
        spangpu_txbank_destroy(bank);
        return NULL;
    }
    s->bank = bank;
    return s;
}

int bell_mf_tx_release(bell_mf_tx_state_t *s)
{
    if (s  &&  s->bank)
    {
        spangpu_txbank_destroy(s->bank);
        s->bank = NULL;
    }
    return 0;
}

int bell_mf_tx_free(bell_mf_tx_state_t *s)
{
    if (s)
    {
        bell_mf_tx_release(s);
        obj_drop(&s->obj, s);
    }
    return 0;
}

int bell_mf_tx_put(bell_mf_tx_state_t *s, const char *digits, int len)
{
    const int rc = spangpu_txbank_put(s->bank, 0, 1, digits, len);

    return (rc < 0)  ?  -1  :  rc;
}

int bell_mf_tx(bell_mf_tx_state_t *s, int16_t amp[], int max_samples)
{
    int len = 0;

    if (max_samples <= 0  ||  spangpu_txbank_tx(s->bank, SPANGPU_MEM_HOST, amp, max_samples, max_samples, &len) < 0)
        return 0;
    return len;
}

r2_mf_tx_state_t *r2_mf_tx_init(r2_mf_tx_state_t *s, bool fwd)
{
    spangpu_txbank_t *bank;

    if (spangpu_txbank_create(&bank, 0, fwd  ?  SPANGPU_TX_R2_MF_FWD  :  SPANGPU_TX_R2_MF_BACK, 1) != SPANGPU_OK)
        return NULL;
    if ((s = OBJ_TAKE(s, r2_mf_tx_state_t)) == NULL)
    {
        spangpu_txbank_destroy(bank);
        return NULL;
    }
    s->bank = bank;
    return s;
}

int r2_mf_tx_release(r2_mf_tx_state_t *s)
{
    if (s  &&  s->bank)
    {
        spangpu_txbank_destroy(s->bank);
        s->bank = NULL;
    }
    return 0;
}

int r2_mf_tx_free(r2_mf_tx_state_t *s)
{
    if (s)
    {
        r2_mf_tx_release(s);
        obj_drop(&s->obj, s);
    }
    return 0;
}

int r2_mf_tx_put(r2_mf_tx_state_t *s, char digit)
{
    /* one signal at a time: the tone of `digit` until the next put, 0 switches it off (bell_r2_mf.c:414-434) */
    (void) spangpu_txbank_put(s->bank, 0, 1, &digit, 1);
    return 0;
}

int r2_mf_tx(r2_mf_tx_state_t *s, int16_t amp[], int samples)
{
    int len = 0;

    if (samples <= 0  ||  spangpu_txbank_tx(s->bank, SPANGPU_MEM_HOST, amp, samples, samples, &len) < 0)
        return 0;
    return len;
}
