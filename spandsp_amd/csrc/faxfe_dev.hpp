// faxfe_dev.hpp -- FAX receive front-end banks: what fax_rx() and the handler fax_modems_state_t has installed do for one channel
// between the receivers and the caller (src/fax.c:176-184, src/fax_modems.c:158-172 and :195-334 of the reference), one lane
// per channel.  The receivers themselves are the modem and FSK banks' kernels; here are dc_restore() over the staged frames
// ahead of them, and behind them the walk over the two event rows a tick leaves: into the shared HDLC framer
// (hdlc_dev.hpp) or the non-ECM row, and the choice of the handler for the next tick.  All integer.
//
// The per-channel functions are plain inline functions over a channel's words (int32_t fe[], the framer's w[]); they compile
// for the host as they are (tests/c_callers/faxfe_host.cpp runs them one lane at a time).
//
// State is fe[word][n_ch].  Beside it the bank keeps one row of lengths per inner receiver bank, lens[slot][n_ch]: what the
// receiver's kernel takes as the channel's length in the coming tick (0: it sits the tick out; kFaxFeTakesPart: the whole
// frame, whatever its length will be -- a receiver kernel takes the smaller of this and the call's samples).

#pragma once

// (the step functions alone: a unit that includes this file defines SPG_HDLC_STEP_FUNCTIONS_ONLY ahead of it, or has included
// hdlc_dev.hpp whole already)
#include "hdlc_dev.hpp"

namespace spg
{

// fe[]: what fax_modems_state_t keeps for its receive side, then fax_rx()'s dc_restore_state_t
enum
{
    FE_HANDLER = 0,             // kFaxFe*: which function rx_handler points at
    FE_FAST_MODEM,              // FAX_MODEM_*_RX of the last start_fast_modem, 0: none yet (the reference's memset)
    FE_BIT_RATE,
    FE_SHORT_TRAIN,
    FE_HDLC_MODE,               // the fast modem's put_bit is the framer's (1) or the non-ECM one (0)
    FE_RX_FRAME_RECEIVED,
    FE_DC_STATE,
    FE_SLOT,                    // the inner fast bank this channel's fast modem lives in, -1: none
    kFaxFeWords
};

enum
{
    kFaxFeNone = 0,             // span_dummy_rx
    kFaxFeFastAndV21,           // fax_modems_xxx_v21_rx
    kFaxFeFastOnly,             // xxx_rx
    kFaxFeV21Only               // fsk_rx
};

// the inner fast banks: one per kind and bit rate a V.27ter or V.17 bank can run, one V.29 bank (its channels carry their rate)
enum
{
    kFaxFeSlotV27_4800 = 0,
    kFaxFeSlotV27_2400,
    kFaxFeSlotV29,
    kFaxFeSlotV17_14400,
    kFaxFeSlotV17_12000,
    kFaxFeSlotV17_9600,
    kFaxFeSlotV17_7200,
    kFaxFeSlotV17_4800,
    kFaxFeSlots
};

constexpr int kFaxFeTakesPart = 1 << 24;        // (= kMaxSamples, bank_host.hpp: no call is longer)

// dc_restore(), spandsp/dc_restore.h:73-77
HDLC_HD int16_t faxfe_dc_restore(int32_t *state, int16_t sample)
{
    *state += (((int32_t) sample*32768 - *state) >> 14);
    return (int16_t) (sample - (*state >> 15));
}

// the two event rows of a tick, and where the non-ECM put_bit calls go
struct FaxFeRows
{
    const int8_t *fast;
    int n_fast;
    const int16_t *v21;
    int n_v21;
    int8_t *put;                // [put_cap]
    int put_cap;
    int n_put;                  // counts on past put_cap; nothing is written there
};

// hdlc_rx_put_bit() with fax_modems_hdlc_accept() behind it: a good frame sets rx_frame_received
HDLC_HD void faxfe_framer_event(int32_t *fe, int32_t *w, HdlcBuf &buf, HdlcRxSink &out, int ev)
{
    const int32_t good = w[HR_RX_FRAMES];
    hdlc_rx_event(w, buf, out, ev);
    if (w[HR_RX_FRAMES] != good)
        fe[FE_RX_FRAME_RECEIVED] = 1;
}

// One tick of one channel behind its receivers: the fast modem's row first, then the V.21 receiver's, as
// fax_modems_xxx_v21_rx() calls them; then the handler for the next tick.
HDLC_HD void faxfe_route_channel(int32_t *fe, int32_t *w, HdlcBuf &buf, HdlcRxSink &out, FaxFeRows &r)
{
    const int handler = fe[FE_HANDLER];
    bool trained = false;
    r.n_put = 0;
    if (handler == kFaxFeFastAndV21  ||  handler == kFaxFeFastOnly)
    {
        const bool framed = fe[FE_HDLC_MODE] != 0;
        for (int i = 0;  i < r.n_fast;  i++)
        {
            const int ev = r.fast[i];
            // xxx_rx_status_handler(): the switch, then the status goes on to put_bit like any other
            trained |= (ev == kSigTrainingSucceeded);
            if (framed)
                faxfe_framer_event(fe, w, buf, out, ev);
            else
            {
                if (r.n_put < r.put_cap)
                    r.put[r.n_put] = (int8_t) ev;
                r.n_put++;
            }
        }
    }
    if (handler == kFaxFeFastAndV21  ||  handler == kFaxFeV21Only)
    {
        for (int i = 0;  i < r.n_v21;  i++)
            faxfe_framer_event(fe, w, buf, out, r.v21[i]);
    }
    if (handler == kFaxFeFastAndV21)
    {
        // the status handler switched in the middle of fax_modems_xxx_v21_rx(), whose own test comes after both receivers ran
        if (trained)
            fe[FE_HANDLER] = kFaxFeFastOnly;
        if (fe[FE_RX_FRAME_RECEIVED])
            fe[FE_HANDLER] = kFaxFeV21Only;
    }
}

// what the two kinds of receiver take of the coming tick under a handler
HDLC_HD int faxfe_fast_len(int handler)
{
    return (handler == kFaxFeFastAndV21  ||  handler == kFaxFeFastOnly)  ?  kFaxFeTakesPart  :  0;
}

HDLC_HD int faxfe_v21_len(int handler)
{
    return (handler == kFaxFeFastAndV21  ||  handler == kFaxFeV21Only)  ?  kFaxFeTakesPart  :  0;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------

#ifdef __HIPCC__

// dc_restore() over the staged row of every channel whose handler is not NONE, in place.  Rows start on 16 bytes (the
// bank's staging buffer), so a lane takes eight samples a load.
__global__ __launch_bounds__(64) void faxfe_dc_kernel(int32_t *fe, int n_ch, int16_t *pcm, long long stride, int samples)
{
    const int ch = blockIdx.x*64 + threadIdx.x;
    if (ch >= n_ch)
        return;
    const size_t n = (size_t) n_ch;
    if (fe[(size_t) FE_HANDLER*n + ch] == kFaxFeNone)
        return;
    int32_t state = fe[(size_t) FE_DC_STATE*n + ch];
    int16_t *row = pcm + (size_t) ch*stride;
    int i = 0;
    for (  ;  i + 8 <= samples;  i += 8)
    {
        uint4 v = *reinterpret_cast<const uint4 *>(row + i);
        uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0;  k < 4;  k++)
        {
            const int16_t lo = faxfe_dc_restore(&state, (int16_t) (q[k] & 0xFFFFu));
            const int16_t hi = faxfe_dc_restore(&state, (int16_t) (q[k] >> 16));
            q[k] = (uint32_t) (uint16_t) lo | ((uint32_t) (uint16_t) hi << 16);
        }
        *reinterpret_cast<uint4 *>(row + i) = make_uint4(q[0], q[1], q[2], q[3]);
    }
    for (  ;  i < samples;  i++)
        row[i] = faxfe_dc_restore(&state, row[i]);
    fe[(size_t) FE_DC_STATE*n + ch] = state;
}

struct FaxFeLaunch
{
    int32_t *fe;                        // [kFaxFeWords][n_ch]
    int32_t *st;                        // the framer bank's words and buffers
    uint32_t *buf;
    int n_ch;
    const int8_t *fast_events[kFaxFeSlots];     // [n_ch][fast_cap[slot]] of the fast bank in each slot, NULL: no such bank
    const int32_t *fast_counts[kFaxFeSlots];
    int fast_cap[kFaxFeSlots];
    const int16_t *v21_events;          // [n_ch][v21_cap]
    const int32_t *v21_counts;
    int v21_cap;
    int32_t *lens;                      // [kFaxFeSlots + 1][n_ch]: the fast banks' rows, then the V.21 bank's
    int32_t *recs;                      // [n_ch][rec_cap]
    uint8_t *bytes;                     // [n_ch][byte_cap]
    int8_t *put;                        // [n_ch][put_cap]
    int32_t *counts;                    // [4][n_ch]: records, octets, non-ECM calls, rows that did not fit (bit 0 fast, 1 V.21)
    int rec_cap;
    int byte_cap;
    int put_cap;
};

__global__ __launch_bounds__(64) void faxfe_route_kernel(FaxFeLaunch L)
{
    const int ch = blockIdx.x*64 + threadIdx.x;
    if (ch >= L.n_ch)
        return;
    const size_t n = (size_t) L.n_ch;
    HdlcRxSink out;
    out.recs = L.recs + (size_t) ch*L.rec_cap;
    out.bytes = L.bytes + (size_t) ch*L.byte_cap;
    out.rec_cap = L.rec_cap;
    out.byte_cap = L.byte_cap;
    out.n_recs = 0;
    out.n_bytes = 0;
    int n_put = 0;
    int short_rows = 0;
    // (a channel with nothing installed takes no part: its words, the framer's and its lengths stay as they are)
    if (L.fe[(size_t) FE_HANDLER*n + ch] != kFaxFeNone)
    {
        int32_t fe[kFaxFeWords];
        for (int i = 0;  i < kFaxFeWords;  i++)
            fe[i] = L.fe[(size_t) i*n + ch];
        const int handler = fe[FE_HANDLER];
        const int slot = fe[FE_SLOT];
        FaxFeRows r;
        r.fast = nullptr;
        r.n_fast = 0;
        // (the slot is bounded here, not trusted: the words can be set from outside)
        if (handler != kFaxFeV21Only  &&  slot >= 0  &&  slot < kFaxFeSlots  &&  L.fast_events[slot] != nullptr)
        {
            const int cap = L.fast_cap[slot];
            const int count = L.fast_counts[slot][ch];
            short_rows |= (count > cap)  ?  1  :  0;
            r.fast = L.fast_events[slot] + (size_t) ch*cap;
            r.n_fast = (count < 0)  ?  0  :  (count > cap)  ?  cap  :  count;
        }
        const int count = (handler != kFaxFeFastOnly)  ?  L.v21_counts[ch]  :  0;
        short_rows |= (count > L.v21_cap)  ?  2  :  0;
        r.v21 = L.v21_events + (size_t) ch*L.v21_cap;
        r.n_v21 = (count < 0)  ?  0  :  (count > L.v21_cap)  ?  L.v21_cap  :  count;
        r.put = L.put + (size_t) ch*L.put_cap;
        r.put_cap = L.put_cap;
        r.n_put = 0;

        int32_t w[kHdlcRxWords];
        for (int i = 0;  i < kHdlcRxWords;  i++)
            w[i] = L.st[(size_t) i*n + ch];
        HdlcBuf buf;
        buf.open(L.buf + ch, n);
        faxfe_route_channel(fe, w, buf, out, r);
        buf.close();
        for (int i = 0;  i < kHdlcRxWords;  i++)
            L.st[(size_t) i*n + ch] = w[i];
        n_put = r.n_put;

        if (fe[FE_HANDLER] != handler)
        {
            L.fe[(size_t) FE_HANDLER*n + ch] = fe[FE_HANDLER];
            if (slot >= 0  &&  slot < kFaxFeSlots)
                L.lens[(size_t) slot*n + ch] = faxfe_fast_len(fe[FE_HANDLER]);
            L.lens[(size_t) kFaxFeSlots*n + ch] = faxfe_v21_len(fe[FE_HANDLER]);
        }
        L.fe[(size_t) FE_RX_FRAME_RECEIVED*n + ch] = fe[FE_RX_FRAME_RECEIVED];
    }
    L.counts[ch] = out.n_recs;
    L.counts[n + ch] = out.n_bytes;
    L.counts[2*n + ch] = n_put;
    L.counts[3*n + ch] = short_rows;
}

#endif  // __HIPCC__

}   // namespace spg
