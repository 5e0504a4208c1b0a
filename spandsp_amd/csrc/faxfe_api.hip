// faxfe_api.hip -- C ABI of the FAX receive front-end banks (include/spangpu.h, "FAX receive front-end banks"): the receive
// half of N fax_modems_state_t objects under fax_rx(), every per-channel decision in device memory.  The bank owns modem
// receiver banks, a V.21 FSK bank and an HDLC receiver bank, all on its own stream, and runs them off one staged copy of a
// tick's frames and off per-channel lengths it keeps on the device.  Device code: faxfe_dev.hpp.  No CPU implementation
// exists behind these entry points; the control-plane calls (start_slow_modem, start_fast_modem, the words) edit one
// channel on the host between ticks, as the reference's own functions edit one object.

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/spangpu.h"
#include "bank_host.hpp"
#define SPG_HDLC_STEP_FUNCTIONS_ONLY        // the HDLC banks' own kernels belong to hdlc_api.hip
#include "faxfe_dev.hpp"

using namespace spg;

// what the inner banks' units hand to this one (not part of the ABI)
extern "C" int spangpu_modem_words_fresh(int kind, uint32_t *w, int bit_rate, float cutoff_dbm0);
extern "C" int spangpu_modem_words_restart(int kind, uint32_t *w, int bit_rate, int train_flag);
extern "C" void spangpu_modem_event_rows(const spangpu_modem_t *m, const int8_t **events, const int32_t **counts, int *cap);
extern "C" void spangpu_fsk_event_rows(const spangpu_fsk_t *f, const int16_t **events, const int32_t **counts, int *cap);
extern "C" void spangpu_fsk_words_init(int32_t *w, const spangpu_fsk_spec_t *spec, int framing_mode, int data_bits, int parity, int stop_bits);
extern "C" int spangpu_fsk_cutoff_all(spangpu_fsk_t *f, float cutoff_dbm0);
extern "C" void spangpu_framer_rows(spangpu_hdlc_rx_t *b, int32_t **st, uint32_t **buf);

static constexpr int kMaxModemWords = 1024;
static constexpr float kV21Cutoff = -39.09f;            // fax_modems.c:343
static constexpr float kFastCutoff = -45.5f;            // fax_modems.c:416; what v17_rx_init() and v27ter_rx_init() set themselves
static constexpr int kFramingOkThreshold = 5;           // HDLC_FRAMING_OK_THRESHOLD, fax_modems.c:106

struct spangpu_faxfe_s
{
    BankCore c;                         // st = fe[kFaxFeWords][n_ch]
    int kinds_mask;
    int max_samples;
    int dc_restore;
    spangpu_modem_t *fast[kFaxFeSlots];
    int assigned[kFaxFeSlots];          // channels whose fast modem lives in the slot
    int32_t *h_slot;                    // [n_ch]: FE_SLOT of every channel, as the host set it
    spangpu_fsk_t *v21;
    spangpu_hdlc_rx_t *framer;
    int32_t *lens;                      // [kFaxFeSlots + 1][n_ch]
    int16_t *pcm;                       // [n_ch][pcm_stride]: the tick's frames, staged once
    long long pcm_stride;
    int32_t *recs;                      // [n_ch][rec_cap]
    int32_t *h_recs;                    // pinned
    int rec_room;
    uint8_t *bytes;                     // [n_ch][byte_cap]
    uint8_t *h_bytes;
    int byte_room;
    int8_t *put;                        // [n_ch][put_cap]
    int8_t *h_put;
    int put_room;
    CountRows counts;                   // [4][n_ch]; the pinned block has two more rows for spangpu_faxfe_handlers()
    int rec_cap;                        // of the last tick; 0: none yet
    int byte_cap;
    int put_cap;
};

static int kind_of(int which)
{
    return (which == SPANGPU_FAXFE_V17_RX)  ?  SPANGPU_V17  :  (which == SPANGPU_FAXFE_V29_RX)  ?  SPANGPU_V29
           :  (which == SPANGPU_FAXFE_V27TER_RX)  ?  SPANGPU_V27TER  :  -1;
}

static int mask_of(int kind)
{
    return (kind == SPANGPU_V17)  ?  SPANGPU_FAXFE_V17  :  (kind == SPANGPU_V29)  ?  SPANGPU_FAXFE_V29  :  SPANGPU_FAXFE_V27TER;
}

// the inner bank a kind at a rate lives in, -1: the kind has no such rate
static int slot_of(int kind, int bit_rate)
{
    switch (kind)
    {
    case SPANGPU_V27TER:
        return (bit_rate == 4800)  ?  kFaxFeSlotV27_4800  :  (bit_rate == 2400)  ?  kFaxFeSlotV27_2400  :  -1;
    case SPANGPU_V29:
        return (bit_rate == 9600  ||  bit_rate == 7200  ||  bit_rate == 4800)  ?  kFaxFeSlotV29  :  -1;
    case SPANGPU_V17:
        switch (bit_rate)
        {
        case 14400: return kFaxFeSlotV17_14400;
        case 12000: return kFaxFeSlotV17_12000;
        case 9600: return kFaxFeSlotV17_9600;
        case 7200: return kFaxFeSlotV17_7200;
        case 4800: return kFaxFeSlotV17_4800;
        }
        break;
    }
    return -1;
}

static int slot_kind(int slot)
{
    return (slot <= kFaxFeSlotV27_2400)  ?  SPANGPU_V27TER  :  (slot == kFaxFeSlotV29)  ?  SPANGPU_V29  :  SPANGPU_V17;
}

static int slot_rate(int slot)
{
    static const int rates[kFaxFeSlots] = {4800, 2400, 9600, 14400, 12000, 9600, 7200, 4800};
    return rates[slot];
}

// the slot's bank, made on first use (a V.27ter or V.17 bank runs one rate: its tables are per rate)
static int slot_bank(spangpu_faxfe_s *b, int slot)
{
    if (b->fast[slot])
        return SPANGPU_OK;
    int rc = spangpu_modem_create(&b->fast[slot], b->c.device, slot_kind(slot), b->c.n_ch, slot_rate(slot));
    if (rc == SPANGPU_OK  &&  (rc = spangpu_modem_set_stream(b->fast[slot], (void *) b->c.stream)) != SPANGPU_OK)
    {
        spangpu_modem_destroy(b->fast[slot]);
        b->fast[slot] = NULL;
    }
    return rc;
}

static int set_len(spangpu_faxfe_s *b, int row, int channel, int32_t len)
{
    return core_rw_at(&b->c, b->lens, channel, row, 1, &len, true);
}

// the channel's rows of lengths as its handler has them, after its fast modem moved from old_slot to fe[FE_SLOT]
static int set_lens(spangpu_faxfe_s *b, int channel, const int32_t *fe, int old_slot)
{
    const int slot = fe[FE_SLOT];
    int rc = SPANGPU_OK;
    if (old_slot >= 0  &&  old_slot != slot)
    {
        rc = set_len(b, old_slot, channel, 0);
        b->assigned[old_slot]--;
    }
    if (slot >= 0  &&  old_slot != slot)
        b->assigned[slot]++;
    b->h_slot[channel] = slot;
    if (rc == SPANGPU_OK  &&  slot >= 0)
        rc = set_len(b, slot, channel, faxfe_fast_len(fe[FE_HANDLER]));
    if (rc == SPANGPU_OK)
        rc = set_len(b, kFaxFeSlots, channel, faxfe_v21_len(fe[FE_HANDLER]));
    return rc;
}

extern "C" {

/*
 * Entry point                                  stands for (paths relative to the reference tree)
 *   spangpu_faxfe_create()                     the receive half of fax_modems_init() x N                          src/fax_modems.c:618-677
 *   spangpu_faxfe_start_slow_modem()           fax_modems_start_slow_modem(s, FAX_MODEM_V21_RX)                   src/fax_modems.c:336-372
 *   spangpu_faxfe_start_fast_modem()           fax_modems_start_fast_modem(s, FAX_MODEM_xxx_RX, ..)               src/fax_modems.c:375-513
 *   spangpu_faxfe_rx()                         fax_rx(): dc_restore(), then s->rx_handler(..) -- span_dummy_rx,    src/fax.c:176-184
 *                                              fax_modems_xxx_v21_rx(), xxx_rx() or fsk_rx() -- with the status   src/fax_modems.c:195-334
 *                                              handlers' and the handlers' own switching
 *   spangpu_faxfe_frames()                     the hdlc_accept calls behind fax_modems_hdlc_accept()              src/fax_modems.c:158-172
 *   spangpu_faxfe_put_bits()                   the non-ECM put_bit calls
 *   spangpu_faxfe_handlers()                   which function rx_handler points at, and rx_frame_received
 */

void spangpu_faxfe_destroy(spangpu_faxfe_t *b)
{
    if (b == NULL)
        return;
    // (the inner banks run on this bank's stream: they go first)
    for (int i = 0;  i < kFaxFeSlots;  i++)
        spangpu_modem_destroy(b->fast[i]);
    spangpu_fsk_destroy(b->v21);
    spangpu_hdlc_rx_destroy(b->framer);
    core_destroy(&b->c);
    free(b->h_slot);
    (void) hipFree(b->lens);
    (void) hipFree(b->pcm);
    (void) hipFree(b->recs);
    (void) hipFree(b->bytes);
    (void) hipFree(b->put);
    counts_free(&b->counts);
    if (b->h_recs)
        (void) hipHostFree(b->h_recs);
    if (b->h_bytes)
        (void) hipHostFree(b->h_bytes);
    if (b->h_put)
        (void) hipHostFree(b->h_put);
    free(b);
}

int spangpu_faxfe_create(spangpu_faxfe_t **out, int device, int n_channels, int kinds_mask, int max_samples, int dc_restore)
{
    const int all = SPANGPU_FAXFE_V27TER | SPANGPU_FAXFE_V29 | SPANGPU_FAXFE_V17;
    if (out == NULL  ||  n_channels <= 0  ||  kinds_mask <= 0  ||  (kinds_mask & ~all)  ||  max_samples <= 0  ||  max_samples > kMaxSamples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments (kinds_mask: SPANGPU_FAXFE_V27TER | _V29 | _V17, at least one)");
    *out = NULL;
    int rc = device_ok(device);
    if (rc != SPANGPU_OK)
        return rc;
    spangpu_faxfe_s *b = (spangpu_faxfe_s *) calloc(1, sizeof(*b));
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    b->kinds_mask = kinds_mask;
    b->max_samples = max_samples;
    b->dc_restore = dc_restore  ?  1  :  0;
    b->pcm_stride = ((long long) max_samples + 7) & ~7LL;
    if ((rc = core_create(&b->c, device, n_channels, kFaxFeWords)) != SPANGPU_OK)
    {
        spangpu_faxfe_destroy(b);
        return rc;
    }
    const size_t n = (size_t) n_channels;
    b->h_slot = (int32_t *) malloc(n*sizeof(int32_t));
    if (b->h_slot == NULL
        ||  hipMalloc(&b->lens, (kFaxFeSlots + 1)*n*sizeof(int32_t)) != hipSuccess
        ||  hipMalloc(&b->pcm, n*(size_t) b->pcm_stride*sizeof(int16_t)) != hipSuccess
        ||  counts_create(&b->c, &b->counts, 4, 6) != SPANGPU_OK)
    {
        spangpu_faxfe_destroy(b);
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "allocation of the FAX front-end bank failed");
    }
    for (size_t c = 0;  c < n;  c++)
        b->h_slot[c] = -1;
    // fax_modems_init(): memset, span_dummy_rx installed; nothing runs for a new channel
    int32_t one[kFaxFeWords];
    memset(one, 0, sizeof(one));
    one[FE_HANDLER] = kFaxFeNone;
    one[FE_SLOT] = -1;
    rc = core_fill(&b->c, one);
    if (rc == SPANGPU_OK  &&  hipMemsetAsync(b->lens, 0, (kFaxFeSlots + 1)*n*sizeof(int32_t), b->c.stream) != hipSuccess)
        rc = spangpu_set_error(SPANGPU_ERR_HIP, "state upload failed");
    // fax_modems_start_slow_modem(s, FAX_MODEM_V21_RX) as fax_modems_init() calls it, and the framer it makes once
    spangpu_fsk_spec_t spec;
    if (rc == SPANGPU_OK)
        rc = spangpu_fsk_preset(SPANGPU_FSK_V21CH2, &spec);
    if (rc == SPANGPU_OK)
        rc = spangpu_fsk_create(&b->v21, device, n_channels, &spec, SPANGPU_FSK_FRAME_MODE_SYNC);
    if (rc == SPANGPU_OK)
        rc = spangpu_fsk_cutoff_all(b->v21, kV21Cutoff);
    if (rc == SPANGPU_OK)
        rc = spangpu_fsk_set_stream(b->v21, (void *) b->c.stream);
    if (rc == SPANGPU_OK)
        rc = spangpu_hdlc_rx_create(&b->framer, device, n_channels, 0, 1, kFramingOkThreshold);
    if (rc == SPANGPU_OK)
        rc = spangpu_hdlc_rx_set_stream(b->framer, (void *) b->c.stream);
    // the bank of each kind at the rate a call starts on; the other rates' banks come with the first channel that asks
    if (rc == SPANGPU_OK  &&  (kinds_mask & SPANGPU_FAXFE_V27TER))
        rc = slot_bank(b, kFaxFeSlotV27_4800);
    if (rc == SPANGPU_OK  &&  (kinds_mask & SPANGPU_FAXFE_V29))
        rc = slot_bank(b, kFaxFeSlotV29);
    if (rc == SPANGPU_OK  &&  (kinds_mask & SPANGPU_FAXFE_V17))
        rc = slot_bank(b, kFaxFeSlotV17_14400);
    if (rc != SPANGPU_OK)
    {
        spangpu_faxfe_destroy(b);
        return rc;
    }
    *out = b;
    return SPANGPU_OK;
}

int spangpu_faxfe_channels(const spangpu_faxfe_t *b) { return b  ?  b->c.n_ch  :  SPANGPU_ERR_BAD_ARG; }
int spangpu_faxfe_state_words(const spangpu_faxfe_t *b) { return b  ?  b->c.words  :  SPANGPU_ERR_BAD_ARG; }

// Every inner bank follows: the tick is one sequence on one stream.  (A modem receiver bank reads a NULL stream as "make one
// of your own", so the null stream cannot carry the whole bank and is refused.)
int spangpu_faxfe_set_stream(spangpu_faxfe_t *b, void *stream)
{
    if (b == NULL  ||  stream == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank, or the null stream");
    // the inner banks first: they wait on the stream they leave, which is this bank's until the last line here
    int rc = SPANGPU_OK;
    for (int i = 0;  i < kFaxFeSlots  &&  rc == SPANGPU_OK;  i++)
    {
        if (b->fast[i])
            rc = spangpu_modem_set_stream(b->fast[i], stream);
    }
    if (rc == SPANGPU_OK)
        rc = spangpu_fsk_set_stream(b->v21, stream);
    if (rc == SPANGPU_OK)
        rc = spangpu_hdlc_rx_set_stream(b->framer, stream);
    if (rc == SPANGPU_OK)
        rc = core_set_stream(&b->c, stream);
    return rc;
}

int spangpu_faxfe_sync(spangpu_faxfe_t *b)
{
    if (b == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "null bank");
    return core_sync(&b->c);
}

spangpu_modem_t *spangpu_faxfe_fast_bank(spangpu_faxfe_t *b, int kind, int bit_rate)
{
    if (b == NULL)
        return NULL;
    const int slot = (bit_rate == 0)  ?  slot_of(kind, (kind == SPANGPU_V17)  ?  14400  :  (kind == SPANGPU_V29)  ?  9600  :  4800)
                                      :  slot_of(kind, bit_rate);
    return (slot < 0)  ?  NULL  :  b->fast[slot];
}

spangpu_fsk_t *spangpu_faxfe_v21_bank(spangpu_faxfe_t *b) { return b  ?  b->v21  :  NULL; }
spangpu_hdlc_rx_t *spangpu_faxfe_framer(spangpu_faxfe_t *b) { return b  ?  b->framer  :  NULL; }

int spangpu_faxfe_get_words(spangpu_faxfe_t *b, int channel, int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    return core_rw_words(&b->c, channel, 0, kFaxFeWords, words, false);
}

int spangpu_faxfe_set_words(spangpu_faxfe_t *b, int channel, const int32_t *words)
{
    if (b == NULL  ||  words == NULL  ||  !channel_ok(&b->c, channel))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    // the slot is the fast modem's kind and rate again, and its bank exists: nothing else points a lane at a row
    const int kind = kind_of(words[FE_FAST_MODEM]);
    const int slot = (kind < 0)  ?  -1  :  slot_of(kind, words[FE_BIT_RATE]);
    const int handler = words[FE_HANDLER];
    if (handler < kFaxFeNone  ||  handler > kFaxFeV21Only  ||  words[FE_SLOT] != slot  ||  (words[FE_FAST_MODEM] != 0  &&  slot < 0)
        ||  (slot >= 0  &&  b->fast[slot] == NULL)  ||  (slot < 0  &&  (handler == kFaxFeFastAndV21  ||  handler == kFaxFeFastOnly)))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "not the words of a channel of this bank");
    int32_t fe[kFaxFeWords];
    memcpy(fe, words, sizeof(fe));
    int rc = core_rw_words(&b->c, channel, 0, kFaxFeWords, fe, true);
    if (rc == SPANGPU_OK)
        rc = set_lens(b, channel, fe, b->h_slot[channel]);
    return rc;
}

int spangpu_faxfe_start_slow_modem(spangpu_faxfe_t *b, int channel, int which)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel)  ||  which < 0  ||  which > SPANGPU_FAXFE_V34_RX)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (which != SPANGPU_FAXFE_V21_RX)
        return spangpu_set_error(SPANGPU_ERR_UNSUPPORTED, "a FAX front-end bank starts FAX_MODEM_V21_RX only: the tone receivers and the senders are other banks");
    // fsk_rx_init(): the object from nothing, then the cutoff
    const int n_words = spangpu_fsk_state_words(b->v21);
    int32_t *w = (int32_t *) calloc((size_t) n_words, sizeof(int32_t));
    if (w == NULL)
        return spangpu_set_error(SPANGPU_ERR_NO_MEMORY, "calloc");
    spangpu_fsk_spec_t spec;
    (void) spangpu_fsk_preset(SPANGPU_FSK_V21CH2, &spec);
    spangpu_fsk_words_init(w, &spec, SPANGPU_FSK_FRAME_MODE_SYNC, 8, 0, 1);
    int rc = spangpu_fsk_set_state(b->v21, channel, w);
    free(w);
    if (rc == SPANGPU_OK)
        rc = spangpu_fsk_set_signal_cutoff(b->v21, channel, kV21Cutoff);
    int32_t fe[kFaxFeWords];
    if (rc == SPANGPU_OK)
        rc = core_rw_words(&b->c, channel, 0, kFaxFeWords, fe, false);
    if (rc != SPANGPU_OK)
        return rc;
    fe[FE_HANDLER] = kFaxFeV21Only;
    fe[FE_RX_FRAME_RECEIVED] = 0;
    if ((rc = core_rw_words(&b->c, channel, 0, kFaxFeWords, fe, true)) != SPANGPU_OK)
        return rc;
    return set_lens(b, channel, fe, b->h_slot[channel]);
}

int spangpu_faxfe_start_fast_modem(spangpu_faxfe_t *b, int channel, int which, int bit_rate, int short_train, int hdlc_mode)
{
    if (b == NULL  ||  !channel_ok(&b->c, channel)  ||  which < 0  ||  which > SPANGPU_FAXFE_V34_RX)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    const int kind = kind_of(which);
    if (kind < 0)
        return spangpu_set_error(SPANGPU_ERR_UNSUPPORTED, "a FAX front-end bank starts FAX_MODEM_V27TER_RX, _V29_RX and _V17_RX only");
    if (!(b->kinds_mask & mask_of(kind)))
        return spangpu_set_error(SPANGPU_ERR_UNSUPPORTED, "this bank was made without that kind of fast modem");
    const int slot = slot_of(kind, bit_rate);
    if (slot < 0)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bit rate not valid for this modem (V.29: 9600/7200/4800, V.27ter: 4800/2400, V.17: 14400/12000/9600/7200/4800)");
    int rc = slot_bank(b, slot);
    int32_t fe[kFaxFeWords];
    if (rc == SPANGPU_OK)
        rc = core_rw_words(&b->c, channel, 0, kFaxFeWords, fe, false);
    if (rc != SPANGPU_OK)
        return rc;
    const int old_slot = b->h_slot[channel];
    uint32_t w[kMaxModemWords];
    if (fe[FE_FAST_MODEM] != which  ||  old_slot < 0)
    {
        // another kind: xxx_rx_init().  The reference's modems overlap in memory, so nothing of an earlier stay survives.
        fe[FE_SHORT_TRAIN] = 0;
        if (spangpu_modem_words_fresh(kind, w, bit_rate, kFastCutoff) < 0)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bit rate not valid for this modem");
    }
    else
    {
        // the same kind: xxx_rx_restart() of the object as it stands.  A V.29 line carries its rate; a V.27ter or V.17 line
        // would have to move to the bank of the other rate, and no fixture holds the reference's restart at a changed rate yet
        if (slot != old_slot)
            return spangpu_set_error(SPANGPU_ERR_UNSUPPORTED, "a V.27ter or V.17 line restarts at the rate it was started with; start another kind first, or use another line");
        fe[FE_SHORT_TRAIN] = short_train  ?  1  :  0;
        if ((rc = spangpu_modem_get_state(b->fast[old_slot], channel, w)) < 0)
            return rc;
        if (spangpu_modem_words_restart(kind, w, bit_rate, (kind == SPANGPU_V17)  ?  fe[FE_SHORT_TRAIN]  :  0) < 0)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bit rate not valid for this modem");
    }
    if ((rc = spangpu_modem_set_state(b->fast[slot], channel, w)) < 0)
        return rc;
    fe[FE_HANDLER] = kFaxFeFastAndV21;
    fe[FE_FAST_MODEM] = which;
    fe[FE_BIT_RATE] = bit_rate;
    fe[FE_HDLC_MODE] = hdlc_mode  ?  1  :  0;
    fe[FE_RX_FRAME_RECEIVED] = 0;
    fe[FE_SLOT] = slot;
    if ((rc = core_rw_words(&b->c, channel, 0, kFaxFeWords, fe, true)) != SPANGPU_OK)
        return rc;
    return set_lens(b, channel, fe, old_slot);
}

int spangpu_faxfe_rx(spangpu_faxfe_t *b, const int16_t *amp, int mem, int samples, long long stride)
{
    int rc = rx_args_ok(b, mem, amp, samples, &stride);
    if (rc != SPANGPU_OK)
        return rc;
    if (samples > b->max_samples)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "samples > max_samples");
    SPG_TRY(hipSetDevice(b->c.device));
    const size_t n = (size_t) b->c.n_ch;
    // 1. the frames, once, into the bank's own rows (they start on 16 bytes); a host caller's are only borrowed for the call
    const bool host = (mem == SPANGPU_MEM_HOST);
    SPG_TRY(hipMemcpy2DAsync(b->pcm, (size_t) b->pcm_stride*sizeof(int16_t), amp, (size_t) stride*sizeof(int16_t), (size_t) samples*sizeof(int16_t), n,
                             host  ?  hipMemcpyHostToDevice  :  hipMemcpyDeviceToDevice, b->c.stream));
    if (host)
        SPG_TRY(hipStreamSynchronize(b->c.stream));
    const dim3 grid((b->c.n_ch + 63)/64);
    if (b->dc_restore)
    {
        hipLaunchKernelGGL(faxfe_dc_kernel, grid, dim3(64), 0, b->c.stream, b->c.st, b->c.n_ch, b->pcm, b->pcm_stride, samples);
        SPG_TRY(hipGetLastError());
    }
    // 2. the receivers, off the lengths the last tick and the control calls left
    FaxFeLaunch L;
    memset(&L, 0, sizeof(L));
    int fast_cap = 0;
    for (int i = 0;  i < kFaxFeSlots;  i++)
    {
        if (b->fast[i] == NULL  ||  b->assigned[i] <= 0)
            continue;
        if ((rc = spangpu_modem_rx_lens_dev(b->fast[i], b->pcm, SPANGPU_MEM_DEVICE, samples, b->pcm_stride, b->lens + (size_t) i*n)) != SPANGPU_OK)
            return rc;
        spangpu_modem_event_rows(b->fast[i], &L.fast_events[i], &L.fast_counts[i], &L.fast_cap[i]);
        fast_cap = (L.fast_cap[i] > fast_cap)  ?  L.fast_cap[i]  :  fast_cap;
    }
    if ((rc = spangpu_fsk_rx_lens_dev(b->v21, b->pcm, SPANGPU_MEM_DEVICE, samples, b->pcm_stride, b->lens + (size_t) kFaxFeSlots*n)) != SPANGPU_OK)
        return rc;
    spangpu_fsk_event_rows(b->v21, &L.v21_events, &L.v21_counts, &L.v21_cap);
    // 3. the rows into the framer and the non-ECM rows, and the handlers of the next tick
    int rec_cap;
    int byte_cap;
    (void) spangpu_hdlc_rx_capacity((long long) fast_cap + L.v21_cap, &rec_cap, &byte_cap);
    const int put_cap = (fast_cap > 16)  ?  fast_cap  :  16;
    if ((rc = grow_pair(&b->recs, &b->h_recs, &b->rec_room, rec_cap, n, b->c.stream)) != SPANGPU_OK
        ||  (rc = grow_pair(&b->bytes, &b->h_bytes, &b->byte_room, byte_cap, n, b->c.stream)) != SPANGPU_OK
        ||  (rc = grow_pair(&b->put, &b->h_put, &b->put_room, put_cap, n, b->c.stream)) != SPANGPU_OK)
        return rc;
    L.fe = b->c.st;
    spangpu_framer_rows(b->framer, &L.st, &L.buf);
    L.n_ch = b->c.n_ch;
    L.lens = b->lens;
    L.recs = b->recs;
    L.bytes = b->bytes;
    L.put = b->put;
    L.counts = b->counts.dev;
    L.rec_cap = rec_cap;
    L.byte_cap = byte_cap;
    L.put_cap = put_cap;
    hipLaunchKernelGGL(faxfe_route_kernel, grid, dim3(64), 0, b->c.stream, L);
    SPG_TRY(hipGetLastError());
    b->rec_cap = rec_cap;
    b->byte_cap = byte_cap;
    b->put_cap = put_cap;
    return SPANGPU_OK;
}

int spangpu_faxfe_capacities(const spangpu_faxfe_t *b, int *rec_cap, int *byte_cap, int *put_cap)
{
    if (b == NULL  ||  rec_cap == NULL  ||  byte_cap == NULL  ||  put_cap == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    *rec_cap = b->rec_cap;
    *byte_cap = b->byte_cap;
    *put_cap = b->put_cap;
    return SPANGPU_OK;
}

// the last tick's counts, and the most of the first three rows; a list or a row that did not fit (the fourth row says so
// too) is an error, never cut short quietly
static int fetch_counts(spangpu_faxfe_s *b, int most[4])
{
    if (b->rec_cap <= 0)
        return spangpu_set_error(SPANGPU_ERR_STATE, "no spangpu_faxfe_rx() yet");
    const int rc = counts_fetch(&b->c, &b->counts, 4);
    if (rc != SPANGPU_OK)
        return rc;
    const int caps[4] = {b->rec_cap, b->byte_cap, b->put_cap, 0};
    bool fits = true;
    for (int row = 0;  row < 4;  row++)
        fits &= count_row_scan(b->counts.pinned + (size_t) row*b->c.n_ch, b->c.n_ch, caps[row], &most[row]);
    if (!fits)
        return spangpu_set_error(SPANGPU_ERR_STATE, "a channel delivered more than a tick of this length can carry");
    return SPANGPU_OK;
}

int spangpu_faxfe_frames(spangpu_faxfe_t *b, const int32_t **recs, const int32_t **counts, const uint8_t **bytes)
{
    if (b == NULL  ||  recs == NULL  ||  counts == NULL  ||  bytes == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int most[4];
    int rc = fetch_counts(b, most);
    if (rc != SPANGPU_OK)
        return rc;
    if ((rc = rows_fetch(&b->c, b->h_recs, b->recs, sizeof(int32_t), b->rec_cap, most[0])) != SPANGPU_OK
        ||  (rc = rows_fetch(&b->c, b->h_bytes, b->bytes, 1, b->byte_cap, most[1])) != SPANGPU_OK)
        return rc;
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    *recs = b->h_recs;
    *counts = b->counts.pinned;
    *bytes = b->h_bytes;
    return b->rec_cap;
}

int spangpu_faxfe_put_bits(spangpu_faxfe_t *b, const int8_t **events, const int32_t **counts)
{
    if (b == NULL  ||  events == NULL  ||  counts == NULL)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    int most[4];
    int rc = fetch_counts(b, most);
    if (rc != SPANGPU_OK  ||  (rc = rows_fetch(&b->c, b->h_put, b->put, 1, b->put_cap, most[2])) != SPANGPU_OK)
        return rc;
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    *events = b->h_put;
    *counts = b->counts.pinned + 2*(size_t) b->c.n_ch;
    return b->put_cap;
}

int spangpu_faxfe_handlers(spangpu_faxfe_t *b, int32_t *handler, int32_t *frame_received)
{
    if (b == NULL  ||  (handler == NULL  &&  frame_received == NULL))
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
    SPG_TRY(hipSetDevice(b->c.device));
    const size_t n = (size_t) b->c.n_ch;
    int32_t *h = b->counts.pinned + 4*n;
    SPG_TRY(hipMemcpyAsync(h, b->c.st + (size_t) FE_HANDLER*n, n*sizeof(int32_t), hipMemcpyDeviceToHost, b->c.stream));
    SPG_TRY(hipMemcpyAsync(h + n, b->c.st + (size_t) FE_RX_FRAME_RECEIVED*n, n*sizeof(int32_t), hipMemcpyDeviceToHost, b->c.stream));
    SPG_TRY(hipStreamSynchronize(b->c.stream));
    if (handler)
        memcpy(handler, h, n*sizeof(int32_t));
    if (frame_received)
        memcpy(frame_received, h + n, n*sizeof(int32_t));
    return SPANGPU_OK;
}

}   // extern "C"
