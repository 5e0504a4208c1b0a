// faxtx_dev.hpp -- FAX transmit front-end banks: what fax_tx() and fax_set_tx_type() do for one channel around the senders
// (src/fax.c:221-256 and :327-421, src/fax_modems.c:581-596, src/silence_gen.c:60-108 of the reference), one lane per channel.
// The senders themselves are the tone, FSK and modem sender banks' kernels, run over per-channel spans of the row
// (txspan_dev.hpp); here are the silence generator in front of them, the plan of a tick -- which samples of the row go to
// silence, which to which sender -- and the resolution after the senders ran: the short return, fax_modems_set_next_tx_type(),
// the SEND_STEP_COMPLETE reports, the length fax_tx() returns and the zeros over what nobody wrote.  All integer.
//
// The per-channel functions are plain inline functions over a channel's words (int32_t fx[]); they compile for the host as they
// are (tests/c_callers/faxtx_host.cpp runs them one lane at a time).
//
// A channel runs at most one sender call in a tick: a sender is reached from silence (the 75 ms in front of V.21 and the fast
// modems) or is the handler at the tick's start, and behind a sender that returned short there is only silence of 0, as
// fax_set_tx_type() never gives a sender a next handler.  So a tick is: plan -> the sender banks over their spans -> resolve.

#pragma once

#include "txspan_dev.hpp"

namespace spg
{

// fx[]: what fax_modems_state_t keeps for its transmit side, then its silence_gen_state_t
enum
{
    FX_HANDLER = 0,             // kFaxTx*: which function tx_handler points at
    FX_NEXT_HANDLER,            // next_tx_handler, kFaxTxSilence: NULL
    FX_TRANSMIT,
    FX_CURRENT_TX_TYPE,         // T30_MODEM_*, -1 after fax_modems_restart()
    FX_TX_BIT_RATE,
    FX_FAST_MODEM,              // FAX_MODEM_*_TX of the last start_fast_modem, 0: none yet.  (The reference keeps one field for
                                // both halves; this bank keeps its own.)
    FX_BIT_RATE,
    FX_SHORT_TRAIN,
    FX_HDLC_MODE,               // the fast modem's get_bit is hdlc_tx_get_bit (1) or the non-ECM one (0)
    FX_USE_TEP,
    FX_SIL_REMAINING,           // silence_gen_state_t: remaining_samples, total_samples
    FX_SIL_TOTAL,
    FX_TONE,                    // the bank of the tone modem_connect_tones_tx_init() last set up (kFaxTxSendCed / kFaxTxSendCng, 0: none
                                // yet): the reference's connect_tx goes on with it whatever current_tx_type says after a restart
    kFaxTxWords
};

enum
{
    kFaxTxSilence = 0,          // silence_gen
    kFaxTxTone,                 // modem_connect_tones_tx
    kFaxTxV21,                  // fsk_tx
    kFaxTxFast                  // v17_tx, v27ter_tx, v29_tx
};

// T30_MODEM_*, spandsp/t30.h:328-337
enum
{
    kT30None = 0, kT30Pause, kT30Ced, kT30Cng, kT30V21, kT30V27ter, kT30V29, kT30V17, kT30V34hdx, kT30Done
};

// FAX_MODEM_*_TX, spandsp/fax_modems.h
enum
{
    kFaxModemV17Tx = 9, kFaxModemV27terTx = 10, kFaxModemV29Tx = 11
};

// the inner sender banks: the id a span carries
enum
{
    kFaxTxSendNone = 0, kFaxTxSendCed, kFaxTxSendCng, kFaxTxSendV21, kFaxTxSendV27ter, kFaxTxSendV29, kFaxTxSendV17, kFaxTxSenders
};

constexpr int kFaxTxIntMax = 0x7FFFFFFF;

// silence_gen(), silence_gen.c:60-80, without the samples: what it returns
HDLC_HD int faxtx_silence_gen(int32_t *fx, int max_len)
{
    if (fx[FX_SIL_REMAINING] != kFaxTxIntMax)
    {
        if (max_len >= fx[FX_SIL_REMAINING])
            max_len = fx[FX_SIL_REMAINING];
        fx[FX_SIL_REMAINING] -= max_len;
    }
    if (kFaxTxIntMax - fx[FX_SIL_TOTAL] >= max_len)
        fx[FX_SIL_TOTAL] += max_len;
    return max_len;
}

// silence_gen_alter(), silence_gen.c:96-108: it adds to what remains (the sums wrap as the reference's build makes them)
HDLC_HD void faxtx_silence_alter(int32_t *fx, int samples)
{
    if (samples < 0  &&  -samples > fx[FX_SIL_REMAINING])
        samples = -fx[FX_SIL_REMAINING];
    fx[FX_SIL_REMAINING] = (int32_t) ((uint32_t) fx[FX_SIL_REMAINING] + (uint32_t) samples);
    fx[FX_SIL_TOTAL] = (int32_t) ((uint32_t) fx[FX_SIL_TOTAL] + (uint32_t) samples);
}

// fax_modems_set_next_tx_type(), fax_modems.c:581-596, with fax_tx()'s test behind it: the number of SEND_STEP_COMPLETE reports
HDLC_HD int faxtx_set_next(int32_t *fx)
{
    if (fx[FX_NEXT_HANDLER] != kFaxTxSilence)
    {
        fx[FX_HANDLER] = fx[FX_NEXT_HANDLER];
        fx[FX_NEXT_HANDLER] = kFaxTxSilence;
        return 0;
    }
    faxtx_silence_alter(fx, 0);
    fx[FX_HANDLER] = kFaxTxSilence;
    fx[FX_TRANSMIT] = 0;
    return (fx[FX_CURRENT_TX_TYPE] != kT30None  &&  fx[FX_CURRENT_TX_TYPE] != kT30Done)  ?  1  :  0;
}

// the bank the installed sender lives in
HDLC_HD int faxtx_sender(const int32_t *fx)
{
    switch (fx[FX_HANDLER])
    {
    case kFaxTxTone:
        return (fx[FX_TONE] == kFaxTxSendCed  ||  fx[FX_TONE] == kFaxTxSendCng)  ?  fx[FX_TONE]  :  kFaxTxSendNone;
    case kFaxTxV21:
        return kFaxTxSendV21;
    case kFaxTxFast:
        return (fx[FX_FAST_MODEM] == kFaxModemV17Tx)  ?  kFaxTxSendV17  :  (fx[FX_FAST_MODEM] == kFaxModemV29Tx)  ?  kFaxTxSendV29
               :  (fx[FX_FAST_MODEM] == kFaxModemV27terTx)  ?  kFaxTxSendV27ter  :  kFaxTxSendNone;
    }
    return kFaxTxSendNone;
}

// The plan of a tick of `samples`: fax_tx()'s loop as far as it goes without a sender.  span[SPAN_START] is where the silence
// ended (the length so far), span[SPAN_COUNT] what the sender installed there is offered (0: none runs), span[SPAN_SENDER] its
// bank, span[SPAN_STEPS] the reports made on the way.
HDLC_HD void faxtx_plan(int32_t *fx, int samples, int32_t *span)
{
    int len = 0;
    int steps = 0;
    int sender = kFaxTxSendNone;
    // (a silence of nothing returns 0 < max_len at once; a handler chain has two links, and the third pass finds transmit off)
    while (fx[FX_TRANSMIT])
    {
        if (fx[FX_HANDLER] != kFaxTxSilence)
        {
            sender = faxtx_sender(fx);
            break;
        }
        if ((len += faxtx_silence_gen(fx, samples - len)) >= samples)
            break;
        steps += faxtx_set_next(fx);
    }
    // (words that name no bank: nothing runs, and resolve sees a sender that returned 0)
    span[SPAN_START] = len;
    span[SPAN_COUNT] = (fx[FX_TRANSMIT]  &&  fx[FX_HANDLER] != kFaxTxSilence)  ?  (samples - len)  :  0;
    span[SPAN_SENDER] = sender;
    span[SPAN_STEPS] = steps;
}

// What a tick left, for spangpu_faxtx_status()
enum
{
    FXO_LEN = 0,                // what fax_tx() returns without transmit_on_idle
    FXO_STEPS,
    FXO_UNDERFLOWS,
    FXO_HANDLER,
    FXO_TRANSMIT,
    kFaxTxOutRows
};

// After the senders: `ret` is what the channel's sender returned for its span, calls / empty the underflow handler calls of
// the span.  [*lo, *hi) is what the sender wrote of the row; the rest of it is zeros.
HDLC_HD void faxtx_resolve(int32_t *fx, int samples, const int32_t *span, int ret, int calls, int empty, int32_t *out, int *lo, int *hi)
{
    int len = span[SPAN_START];
    int steps = span[SPAN_STEPS];
    int under = 0;
    *lo = *hi = len;
    if (span[SPAN_COUNT] > 0)
    {
        ret = (ret < 0)  ?  0  :  (ret > span[SPAN_COUNT])  ?  span[SPAN_COUNT]  :  ret;
        len += ret;
        *hi = len;
        steps += calls;
        under = empty;
        if (len < samples)
            steps += faxtx_set_next(fx);
    }
    out[FXO_LEN] = len;
    out[FXO_STEPS] = steps;
    out[FXO_UNDERFLOWS] = under;
    out[FXO_HANDLER] = fx[FX_HANDLER];
    out[FXO_TRANSMIT] = fx[FX_TRANSMIT];
}

// What fax_set_tx_type() has the inner banks do, for the caller to carry out
struct FaxTxAct
{
    int acted;                  // 0: the same type, nothing happened
    int tone;                   // kFaxTxSendCed / kFaxTxSendCng: modem_connect_tones_tx_init()
    int v21;                    // fsk_tx_init()
    int flags;                  // hdlc_tx_flags(flags), 0: none
    int fast;                   // kFaxTxSendV27ter .. kFaxTxSendV17, 0: none
    int fast_init;              // xxx_tx_init() (1) or xxx_tx_restart() (0)
};

// fax_set_tx_type(), fax.c:327-421, with fax_modems_start_fast_modem()'s choice of path (fax_modems.c:402-510).  The type is one
// this bank runs (the caller has refused the others).
HDLC_HD void faxtx_set_tx_type(int32_t *fx, int type, int bit_rate, int short_train, int use_hdlc, FaxTxAct *act)
{
    act->acted = 0;
    act->tone = 0;
    act->v21 = 0;
    act->flags = 0;
    act->fast = 0;
    act->fast_init = 0;
    if (fx[FX_CURRENT_TX_TYPE] == type)
        return;
    act->acted = 1;
    switch (type)
    {
    case kT30Pause:
        faxtx_silence_alter(fx, short_train*8);
        fx[FX_HANDLER] = kFaxTxSilence;
        fx[FX_NEXT_HANDLER] = kFaxTxSilence;
        fx[FX_TRANSMIT] = 1;
        break;
    case kT30Ced:
    case kT30Cng:
        act->tone = (type == kT30Ced)  ?  kFaxTxSendCed  :  kFaxTxSendCng;
        fx[FX_TONE] = act->tone;
        fx[FX_HANDLER] = kFaxTxTone;
        fx[FX_NEXT_HANDLER] = kFaxTxSilence;
        fx[FX_TRANSMIT] = 1;
        break;
    case kT30V21:
        act->v21 = 1;
        act->flags = 32;
        faxtx_silence_alter(fx, 75*8);
        fx[FX_HANDLER] = kFaxTxSilence;
        fx[FX_NEXT_HANDLER] = kFaxTxV21;
        fx[FX_TRANSMIT] = 1;
        break;
    case kT30V17:
    case kT30V27ter:
    case kT30V29:
    {
        const int which = (type == kT30V17)  ?  kFaxModemV17Tx  :  (type == kT30V29)  ?  kFaxModemV29Tx  :  kFaxModemV27terTx;
        faxtx_silence_alter(fx, 75*8);
        act->flags = bit_rate/40;
        act->fast = (type == kT30V17)  ?  kFaxTxSendV17  :  (type == kT30V29)  ?  kFaxTxSendV29  :  kFaxTxSendV27ter;
        fx[FX_BIT_RATE] = bit_rate;
        fx[FX_HDLC_MODE] = use_hdlc  ?  1  :  0;
        if (fx[FX_FAST_MODEM] != which)
        {
            fx[FX_SHORT_TRAIN] = 0;
            fx[FX_FAST_MODEM] = which;
            act->fast_init = 1;
        }
        else
        {
            fx[FX_SHORT_TRAIN] = short_train;
        }
        fx[FX_HANDLER] = kFaxTxSilence;
        fx[FX_NEXT_HANDLER] = kFaxTxFast;
        fx[FX_TRANSMIT] = 1;
        break;
    }
    default:
        faxtx_silence_alter(fx, 0);
        fx[FX_HANDLER] = kFaxTxSilence;
        fx[FX_NEXT_HANDLER] = kFaxTxSilence;
        fx[FX_TRANSMIT] = 0;
        break;
    }
    fx[FX_TX_BIT_RATE] = bit_rate;
    fx[FX_CURRENT_TX_TYPE] = type;
}

// fax_modems_init()'s transmit side, fax_modems.c:618-677
HDLC_HD void faxtx_words_init(int32_t *fx, int use_tep)
{
    for (int i = 0;  i < kFaxTxWords;  i++)
        fx[i] = 0;
    fx[FX_USE_TEP] = use_tep  ?  1  :  0;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------

#ifdef __HIPCC__

struct FaxTxLaunch
{
    int32_t *fx;                // [kFaxTxWords][n_ch]
    int n_ch;
    int samples;
    int32_t *span;              // [kSpanRows][n_ch]
    int32_t *ret;               // [n_ch]
    int32_t *cnt;               // [2][n_ch]
    int32_t *out;               // [kFaxTxOutRows][n_ch]
    int16_t *pcm;               // [n_ch][stride]
    long long stride;
};

// Neighbouring lanes are on different handlers as a rule; every lane goes its own way through the plan.
__global__ __launch_bounds__(64) void faxtx_plan_kernel(FaxTxLaunch L)
{
    const int ch = blockIdx.x*64 + threadIdx.x;
    if (ch >= L.n_ch)
        return;
    const size_t n = (size_t) L.n_ch;
    int32_t fx[kFaxTxWords];
#pragma unroll
    for (int i = 0;  i < kFaxTxWords;  i++)
        fx[i] = L.fx[(size_t) i*n + ch];
    int32_t span[kSpanRows];
    faxtx_plan(fx, L.samples, span);
    L.fx[(size_t) FX_HANDLER*n + ch] = fx[FX_HANDLER];
    L.fx[(size_t) FX_NEXT_HANDLER*n + ch] = fx[FX_NEXT_HANDLER];
    L.fx[(size_t) FX_TRANSMIT*n + ch] = fx[FX_TRANSMIT];
    L.fx[(size_t) FX_SIL_REMAINING*n + ch] = fx[FX_SIL_REMAINING];
    L.fx[(size_t) FX_SIL_TOTAL*n + ch] = fx[FX_SIL_TOTAL];
#pragma unroll
    for (int i = 0;  i < kSpanRows;  i++)
        L.span[(size_t) i*n + ch] = span[i];
    L.ret[ch] = 0;
    L.cnt[ch] = 0;
    L.cnt[n + ch] = 0;
}

// One lane per channel resolves; then the 64 lanes of the block go over its channels' rows side by side and write the zeros
// in front of and behind what the sender wrote.  A row a sender filled whole (the usual one in page data) is not touched.
__global__ __launch_bounds__(64) void faxtx_resolve_kernel(FaxTxLaunch L)
{
    __shared__ int s_lo[64];
    __shared__ int s_hi[64];
    const int ch0 = blockIdx.x*64;
    const int ch = ch0 + threadIdx.x;
    const size_t n = (size_t) L.n_ch;
    if (ch < L.n_ch)
    {
        int32_t fx[kFaxTxWords];
#pragma unroll
        for (int i = 0;  i < kFaxTxWords;  i++)
            fx[i] = L.fx[(size_t) i*n + ch];
        int32_t span[kSpanRows];
#pragma unroll
        for (int i = 0;  i < kSpanRows;  i++)
            span[i] = L.span[(size_t) i*n + ch];
        int32_t out[kFaxTxOutRows];
        int lo;
        int hi;
        faxtx_resolve(fx, L.samples, span, L.ret[ch], L.cnt[ch], L.cnt[n + ch], out, &lo, &hi);
        L.fx[(size_t) FX_HANDLER*n + ch] = fx[FX_HANDLER];
        L.fx[(size_t) FX_NEXT_HANDLER*n + ch] = fx[FX_NEXT_HANDLER];
        L.fx[(size_t) FX_TRANSMIT*n + ch] = fx[FX_TRANSMIT];
        L.fx[(size_t) FX_SIL_REMAINING*n + ch] = fx[FX_SIL_REMAINING];
        L.fx[(size_t) FX_SIL_TOTAL*n + ch] = fx[FX_SIL_TOTAL];
#pragma unroll
        for (int i = 0;  i < kFaxTxOutRows;  i++)
            L.out[(size_t) i*n + ch] = out[i];
        // (bounded to the row whatever the words say)
        s_lo[threadIdx.x] = (lo < 0)  ?  0  :  (lo > L.samples)  ?  L.samples  :  lo;
        s_hi[threadIdx.x] = (hi < 0)  ?  0  :  (hi > L.samples)  ?  L.samples  :  hi;
    }
    __syncthreads();
    const int nchan = (L.n_ch - ch0 < 64)  ?  (L.n_ch - ch0)  :  64;
    for (int c = 0;  c < nchan;  c++)
    {
        int16_t *row = L.pcm + (size_t) (ch0 + c)*L.stride;
        const int lo = s_lo[c];
        const int hi = s_hi[c];
        for (int i = threadIdx.x;  i < lo;  i += 64)
            row[i] = 0;
        for (int i = hi + threadIdx.x;  i < L.samples;  i += 64)
            row[i] = 0;
    }
}

#endif  // __HIPCC__

}   // namespace spg
