// txspan_dev.hpp -- what a sender bank's kernel takes when it runs under the FAX transmit front end (faxtx_dev.hpp): a span of
// the row per channel, read from device memory, and hdlc_tx_get_bit() on the front end's framer bank as the source of its bits.
//
// span[4][n_ch]: start, count, sender id, (the front end's own).  A channel whose sender id is not the launch's, or whose count
// is 0, sits the launch out: its state and its row stay untouched.  Otherwise the channel makes one xxx_tx() call of `count`
// samples into row[start .. start + count), with the tests xxx_tx() makes at the start of a call, and leaves what the call
// returned in ret[ch].
//
// A channel whose mode word is set (the V.21 sender: always) takes its bits from hdlc_tx_get_bit() on the framer's words, buffer
// and command queue, called exactly where the reference calls get_bit; the queue is offered at the top of the span.  cnt[2][n_ch]:
// how often the underflow handler was called in the span, and how many of those calls found the queue empty.

#pragma once

// (the step functions alone: a unit that includes this file defines SPG_HDLC_STEP_FUNCTIONS_ONLY ahead of it, as faxfe_api.hip
// does -- the HDLC banks' own kernels belong to hdlc_api.hip, and a second unit that defined them would not link)
#include "hdlc_dev.hpp"

namespace spg
{

enum
{
    SPAN_START = 0,
    SPAN_COUNT,
    SPAN_SENDER,
    SPAN_STEPS,             // SEND_STEP_COMPLETE reports the plan of the tick made itself
    kSpanRows
};

struct TxSpans
{
    const int32_t *span;    // [kSpanRows][n_ch]
    int id;                 // the sender this launch is
    int32_t *ret;           // [n_ch]
    // the framer bank
    int32_t *hst;           // [kHdlcTxWords][n_ch]
    uint32_t *hbuf;         // [101][n_ch]
    int32_t *q_hdr;         // [n_ch][depth]
    const uint32_t *q_data; // [n_ch][depth][101]
    int depth;
    const int32_t *mode;    // [n_ch] hdlc_mode, NULL: every channel is framed
    int32_t *cnt;           // [2][n_ch]
};

#ifdef __HIPCC__

// the channel's span in a call of `samples`, bounded to the row whatever the words say; false: it sits the launch out
__device__ __forceinline__ bool span_of(const TxSpans &S, size_t n, int ch, int samples, int &start, int &count)
{
    start = S.span[(size_t) SPAN_START*n + ch];
    count = S.span[(size_t) SPAN_COUNT*n + ch];
    if (S.span[(size_t) SPAN_SENDER*n + ch] != S.id  ||  start < 0  ||  start >= samples  ||  count <= 0)
        return false;
    count = (count > samples - start)  ?  (samples - start)  :  count;
    return true;
}

// a lane's hdlc_tx while a span runs
struct SpanFramer
{
    int32_t w[kHdlcTxWords];
    HdlcBuf buf;
    HdlcTxQueue q;

    __device__ __forceinline__ void open(const TxSpans &S, size_t n, int ch)
    {
#pragma unroll
        for (int i = 0;  i < kHdlcTxWords;  i++)
            w[i] = S.hst[(size_t) i*n + ch];
        buf.open(S.hbuf + ch, n);
        q.hdr = S.q_hdr + (size_t) ch*S.depth;
        q.data = S.q_data + (size_t) ch*S.depth*kHdlcBufWords;
        q.depth = S.depth;
        q.underflows = 0;
        q.calls = 0;
        hdlc_tx_offer(w, buf, q);
    }

    __device__ __forceinline__ int bit()
    {
        return hdlc_tx_get_bit(w, buf, q);
    }

    __device__ __forceinline__ void close(const TxSpans &S, size_t n, int ch)
    {
        buf.close();
#pragma unroll
        for (int i = 0;  i < kHdlcTxWords;  i++)
            S.hst[(size_t) i*n + ch] = w[i];
        S.cnt[ch] = q.calls;
        S.cnt[n + ch] = q.underflows;
    }
};

#endif  // __HIPCC__

}   // namespace spg
