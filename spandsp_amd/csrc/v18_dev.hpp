// v18_dev.hpp -- device side of the V.18 text banks: N Baudot text telephones in one of the three Weitbrecht modes, text in
// and text out, one channel per lane, state in HBM, one launch per tx call and one per rx call.  Integer arithmetic
// throughout, so the results equal the reference's by construction.
//
// What is restated (paths relative to the reference tree):
//   v18_tdd_get_async_byte()   src/v18.c:959-1017      the lazy pull from the text ring, tx_signal_on, tx_draining
//   encode_baudot()            src/v18.c:768-931       as a 128-entry table the host builds (v18_api.hip)
//   v18_tdd_put_async_byte()   src/v18.c:1155-1213     decode_baudot() :934-956
//   v18_tx() / v18_rx()        src/v18.c:1806-1871, 1874-1940   (V18_AUTOMODING_NONE: the _42 states)
//   async_tx_get_bit()         src/async.c:277-338     5 data bits, no parity, 2 stop bits
//   queue_read_byte()          src/queue.c:197-220     a ring of 129 bytes that takes 128
// What is used as it stands: the modulator and its round loop (ftx_rounds(), fskmod_dev.hpp) with the character framer as
// its bit source, and the framed demodulator over two waves (fsk_pair_body(), fsk_dev.hpp) with the Baudot decoder as its
// sink.
//
// State is structure-of-arrays int32 words [kV18Words + kFskTxWords + kFskScalars + 4*span][n_channels]: the text layer's
// words, then the sender's in the layout of fskmod_dev.hpp, then the receiver's in the layout of fsk_dev.hpp.  The sender
// and the receiver of a channel share V18_RX_SUPPRESSION; both kernels run on the bank's stream, in the caller's order.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fsk_dev.hpp"
#include "fskmod_dev.hpp"

namespace spg
{

enum
{
    V18_MODE = 0,
    V18_TX_SIGNAL_ON = 1,       // 0 off, 1 a put turned it on, 2 the first character has been pulled
    V18_TX_DRAINING = 2,
    V18_BAUDOT_TX_SHIFT = 3,    // 0 letters, 1 figures, 2 an explicit shift is due
    V18_BAUDOT_RX_SHIFT = 4,
    V18_NEXT_BYTE = 5,          // the code that follows a shift, or 0xFF
    V18_RX_SUPPRESSION = 6,     // samples for which the receiver drops what it hears
    V18_Q_IPTR = 7,             // the text ring: write and read positions
    V18_Q_OPTR = 8,
    V18_A_BITPOS = 9,           // async_tx: bitpos, frame_in_progress, presend_bits
    V18_A_FRAME = 10,
    V18_A_PRESEND = 11,
    V18_RX_STATUS = 12,         // the last rx call: bit 0 SIG_STATUS_CARRIER_UP seen, bit 1 SIG_STATUS_CARRIER_DOWN seen
    V18_CALLING_PARTY = 13,
    kV18Words = 16
};

constexpr int kV18Ring = 129;               // queue_init(.., 128, ..): len + 1 bytes, of which len can be in use
constexpr int kV18Suppress = 300*8;         // milliseconds_to_samples(300)
constexpr int kV18EndOfData = -7;           // SIG_STATUS_END_OF_DATA
constexpr int kV18LinkIdle = -17;           // SIG_STATUS_LINK_IDLE
constexpr int kV18FigureShift = 0x1B;
constexpr int kV18LetterShift = 0x1F;

// The text layer of one sender while a call runs
struct V18Tx
{
    int signal_on, draining, shift, next_byte, suppression;
    int iptr, optr;
    int bitpos, frame, presend;
    const uint8_t *ring;        // this channel's kV18Ring bytes
    const uint8_t *encode;      // [128]: 0xFF no such character, 0x40 | code in both sets, 0x80 | code figures, code letters
};

// encode_baudot() with repeat_shifts off, as v18_init() leaves it: 0 = nothing to send for this character
__device__ __forceinline__ int v18_encode(V18Tx &t, int ch)
{
    const int e = t.encode[ch & 0x7F];
    if (e == 0xFF)
        return 0;
    if (e & 0x40)
        return 0x8000 | (e & 0x1F);
    const int set = (e & 0x80)  ?  1  :  0;
    if (t.shift == set)
        return e & 0x1F;
    t.shift = set;
    return 0x8000 | ((set  ?  kV18FigureShift  :  kV18LetterShift) << 5) | (e & 0x1F);
}

// v18_tdd_get_async_byte()
__device__ __forceinline__ int v18_get_byte(V18Tx &t)
{
    if (t.next_byte != 0xFF)
    {
        t.suppression = kV18Suppress;
        const int x = t.next_byte;
        t.next_byte = 0xFF;
        return x;
    }
    int x;
    for (;;)
    {
        if (t.optr == t.iptr)
        {
            if (t.draining)
            {
                t.draining = 0;
                return kV18EndOfData;
            }
            t.presend = 14;
            t.draining = 1;
            t.suppression = kV18Suppress;
            return kV18LinkIdle;
        }
        const int ch = t.ring[t.optr];
        t.optr = (t.optr + 1 >= kV18Ring)  ?  0  :  (t.optr + 1);
        if ((x = v18_encode(t, ch)) != 0)
            break;
    }
    t.suppression = kV18Suppress;
    if (t.signal_on == 1)
    {
        t.presend = 7;
        t.signal_on = 2;
    }
    if (x & 0x3E0)
    {
        t.next_byte = x & 0x1F;
        return (x >> 5) & 0x1F;
    }
    t.next_byte = 0xFF;
    return x & 0x1F;
}

// async_tx_get_bit() for 5N2: 0 or 1, or -1 for SIG_STATUS_END_OF_DATA
__device__ __forceinline__ int v18_next_bit(V18Tx &t)
{
    if (t.bitpos == 0)
    {
        if (t.presend > 0)
        {
            t.presend--;
            return 1;
        }
        const int byte = v18_get_byte(t);
        if (byte < 0)
            return (byte != kV18LinkIdle)  ?  -1  :  1;
        t.frame = (byte & 0x1F) | (0xFFFF << 5);
        t.bitpos = 1;
        return 0;
    }
    const int bit = t.frame & 1;
    t.frame >>= 1;
    if (++t.bitpos > 7)
        t.bitpos = 0;
    return bit;
}

struct V18TxLaunch
{
    int32_t *st;                // the bank's words
    const int16_t *quarter;     // [257] in HBM
    const uint8_t *ring;        // [n_ch][kV18Ring]
    const uint8_t *tables;      // [128] encode, then [2][32] decode
    int16_t *pcm;               // [n_ch][stride]
    int32_t *lens;              // [n_ch] or null
    long long stride;
    int n_ch;
    int samples;
    int vec;
};

// v18_tx() x N: the FSK modulator (fskmod_dev.hpp) with the Baudot framer as its bit source.  The character pull happens in
// phase 1, at the bit boundary that starts a character: nothing of it is on the per-sample path.
__global__ __launch_bounds__(64*kFtxWaves) void v18_tx_kernel(const V18TxLaunch L)
{
    const int lane = threadIdx.x & 63;
    const int ch0 = (blockIdx.x*kFtxWaves + (threadIdx.x >> 6))*kFtxCpw;
    const int ch = ch0 + lane;
    const bool owner = (lane < kFtxCpw)  &&  (ch < L.n_ch);
    const FtxLds lds = ftx_lds(L.quarter);

    const size_t n = (size_t) L.n_ch;
    int32_t *sv = L.st + (owner  ?  ch  :  0);
    int32_t *st = sv + (size_t) kV18Words*n;
    const int samples = L.samples;
    V18Tx t;
    t.signal_on = 0;
    t.draining = 0;
    t.shift = 0;
    t.next_byte = 0xFF;
    t.suppression = 0;
    t.iptr = 0;
    t.optr = 0;
    t.bitpos = 0;
    t.frame = 0;
    t.presend = 0;
    t.ring = L.ring + (size_t) (owner  ?  ch  :  0)*kV18Ring;
    t.encode = L.tables;
    if (owner)
    {
        t.signal_on = sv[V18_TX_SIGNAL_ON*n];
        t.draining = sv[V18_TX_DRAINING*n];
        t.shift = sv[V18_BAUDOT_TX_SHIFT*n];
        t.next_byte = sv[V18_NEXT_BYTE*n];
        t.suppression = sv[V18_RX_SUPPRESSION*n];
        t.iptr = sv[V18_Q_IPTR*n];
        t.optr = sv[V18_Q_OPTR*n];
        t.bitpos = sv[V18_A_BITPOS*n];
        t.frame = sv[V18_A_FRAME*n];
        t.presend = sv[V18_A_PRESEND*n];
    }
    FtxChan c;
    ftx_chan_load(c, st, n, owner);
    // v18.c:1842-1865: with tx_signal_on clear nothing is asked of the modulator; a modulator that is shut down returns 0
    const bool asked = owner  &&  t.signal_on != 0;
    const bool silent = !asked  ||  c.shutdown;
    int done = owner  ?  0  :  samples;
    int len = samples;
    int zero_from = 0x7FFFFFFF;
    if (owner  &&  silent)
    {
        len = 0;
        zero_from = 0;
    }
    __syncthreads();

    ftx_rounds(lds, c, owner, silent, done, samples, len, zero_from, 0, L.pcm, L.stride, ch0, L.n_ch, samples, L.vec != 0,
               [&]() __attribute__((always_inline)) { return v18_next_bit(t); });

    if (owner)
    {
        if (asked)
        {
            if (!c.was_shutdown)
            {
                ftx_chan_store(c, st, n);
                sv[V18_TX_DRAINING*n] = t.draining;
                sv[V18_BAUDOT_TX_SHIFT*n] = t.shift;
                sv[V18_NEXT_BYTE*n] = t.next_byte;
                sv[V18_RX_SUPPRESSION*n] = t.suppression;
                sv[V18_Q_OPTR*n] = t.optr;
                sv[V18_A_BITPOS*n] = t.bitpos;
                sv[V18_A_FRAME*n] = t.frame;
                sv[V18_A_PRESEND*n] = t.presend;
            }
            // v18.c:1856-1857: a call that gets nothing out of the modulator turns the signal off
            sv[V18_TX_SIGNAL_ON*n] = (len <= 0)  ?  0  :  t.signal_on;
        }
        ftx_event_store(c, st, n);
        if (L.lens)
            L.lens[ch] = len;
    }
}

// v18_put() on channels [lo, hi): text[(c - lo)*tstride ...], lens[c - lo] bytes of it.  queue_write() with
// QUEUE_WRITE_ATOMIC (queue.c:223-273): the whole message or nothing; results[c - lo] = what v18_put() returns.
__global__ void v18_put_kernel(int32_t *st, uint8_t *ring, int n_ch, int lo, int hi, const uint8_t *text, int tstride, const int32_t *lens,
                               int32_t *results)
{
    const int ch = lo + blockIdx.x*blockDim.x + threadIdx.x;
    if (ch >= hi)
        return;
    const size_t n = (size_t) n_ch;
    int32_t *sv = st + ch;
    const uint8_t *src = text + (size_t) (ch - lo)*tstride;
    uint8_t *mine = ring + (size_t) ch*kV18Ring;
    const int len = lens[ch - lo];
    int iptr = sv[V18_Q_IPTR*n];
    const int optr = sv[V18_Q_OPTR*n];
    int room = optr - iptr - 1;
    room += (room < 0)  ?  kV18Ring  :  0;
    if (room < len)
    {
        results[ch - lo] = -1;
        return;
    }
    for (int i = 0;  i < len;  i++)
    {
        mine[iptr] = src[i];
        iptr = (iptr + 1 >= kV18Ring)  ?  0  :  (iptr + 1);
    }
    sv[V18_Q_IPTR*n] = iptr;
    if (sv[V18_TX_SIGNAL_ON*n] == 0)
        sv[V18_TX_SIGNAL_ON*n] = 1;
    results[ch - lo] = len;
}

struct V18RxLaunch
{
    FskLaunch f;                // st = the receiver's words inside the bank's; events / ev_count are not used
    int32_t *sv;                // the bank's words (the text layer's come first)
    const uint8_t *tables;
    uint8_t *chars;             // [n_ch][cap]
    int32_t *counts;            // [n_ch]
    int cap;
};

// The text layer of one receiver while a call runs: v18_tdd_put_async_byte() as the demodulator's put_bit, the sink of
// fsk_pair_body() (fsk_dev.hpp)
struct V18RxSink
{
    const V18RxLaunch &V;
    int32_t *sv;
    uint8_t *out;
    int cap;
    int shift, suppression, status, count;

    __device__ __forceinline__ void open(bool live, int ch, size_t n, int mylen)
    {
        sv = V.sv + ch;
        shift = sv[V18_BAUDOT_RX_SHIFT*n];
        suppression = sv[V18_RX_SUPPRESSION*n];
        status = 0;
        count = 0;
        // v18.c:1876-1884, ahead of the samples
        suppression = (suppression > mylen)  ?  (suppression - mylen)  :  0;
        out = V.chars + (size_t) ch*V.cap;
        cap = live  ?  V.cap  :  0;
    }

    __device__ __forceinline__ void put(FskBitSide &, int byte)
    {
        if (byte < 0)
        {
            // carrier up and down only reset rx_msg_len, which is always 0 between characters in these modes
            status |= (byte == -2)  ?  1  :  2;
            return;
        }
        if (suppression > 0)
            return;
        if (byte == kV18FigureShift)
        {
            shift = 1;
        }
        else if (byte == kV18LetterShift)
        {
            shift = 0;
        }
        else
        {
            if (count < cap)
                out[count] = V.tables[128 + shift*32 + (byte & 0x1F)];
            count++;
        }
    }

    __device__ __forceinline__ void close(FskBitSide &, int ch, size_t n)
    {
        sv[V18_BAUDOT_RX_SHIFT*n] = shift;
        sv[V18_RX_SUPPRESSION*n] = suppression;
        sv[V18_RX_STATUS*n] = status;
        V.counts[ch] = count;
    }
};

// v18_rx() x N: the two-wave receiver (fsk_pair_body(), fsk_dev.hpp), framed, with the suppression timer stepped ahead of
// the samples and the Baudot decoder behind the framer.
__global__ __launch_bounds__(128) void v18_rx_kernel(const V18RxLaunch V)
{
    V18RxSink sink = {V};
    fsk_pair_body<FSK_FRAMING_ALWAYS>(V.f, sink);
}

}   // namespace spg
