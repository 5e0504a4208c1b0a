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
// What is used as it stands: the modulator (ftx_walk() / ftx_render(), fsktx_dev.hpp) with the character framer as its bit
// source, and the framed demodulator over two waves (fsk_sig_block() / fsk_bit_block(), fsk_dev.hpp) with the Baudot
// decoder as its put_bit.
//
// State is structure-of-arrays int32 words [kV18Words + kFskTxWords + kFskScalars + 4*span][n_channels]: the text layer's
// words, then the sender's in the layout of fsktx_dev.hpp, then the receiver's in the layout of fsk_dev.hpp.  The sender
// and the receiver of a channel share V18_RX_SUPPRESSION; both kernels run on the bank's stream, in the caller's order.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "fsk_dev.hpp"
#define SPG_FTX_WITHOUT_KERNELS
#include "fsktx_dev.hpp"

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

// v18_tx() x N: the shape of fsktx_bank_kernel, with the Baudot framer as the modulator's bit source.  The character pull
// happens in phase 1, at the bit boundary that starts a character: nothing of it is on the per-sample path.
__global__ __launch_bounds__(64*kFtxWaves) void v18_tx_kernel(const V18TxLaunch L)
{
    __shared__ int16_t quarter[258];
    __shared__ int32_t all_start[kFtxWaves][kFtxCpw][kFtxRunStride];
    __shared__ int32_t all_phase[kFtxWaves][kFtxCpw][kFtxRunStride];
    __shared__ int32_t all_rate[kFtxWaves][kFtxCpw][kFtxRunStride];
    __shared__ __attribute__((aligned(16))) int32_t all_hdr[kFtxWaves][kFtxCpw][8];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    int32_t (*r_start)[kFtxRunStride] = all_start[wave];
    int32_t (*r_phase)[kFtxRunStride] = all_phase[wave];
    int32_t (*r_rate)[kFtxRunStride] = all_rate[wave];
    int32_t (*r_hdr)[8] = all_hdr[wave];
    const int ch0 = (blockIdx.x*kFtxWaves + wave)*kFtxCpw;
    const int ch = ch0 + lane;
    const bool owner = (lane < kFtxCpw)  &&  (ch < L.n_ch);

    for (int i = threadIdx.x;  i < 257;  i += 64*kFtxWaves)
        quarter[i] = L.quarter[i];

    const size_t n = (size_t) L.n_ch;
    int32_t *sv = L.st + (owner  ?  ch  :  0);
    int32_t *st = sv + (size_t) kV18Words*n;
    const int samples = L.samples;
    FtxMod m = {1, 0, 0, 0, 0, 0u};
    int scaling = 0;
    bool shutdown = true;
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
        m.baud_rate = st[FT_BAUD_RATE*n];
        m.rate0 = st[FT_RATE0*n];
        m.rate1 = st[FT_RATE1*n];
        scaling = st[FT_SCALING*n];
        m.cur_rate = st[FT_CUR_RATE*n];
        m.phase = (uint32_t) st[FT_PHASE*n];
        m.baud_frac = st[FT_BAUD_FRAC*n];
        shutdown = st[FT_SHUTDOWN*n] != 0;
    }
    // v18.c:1842-1865: with tx_signal_on clear nothing is asked of the modulator; a modulator that is shut down returns 0
    const bool asked = owner  &&  t.signal_on != 0;
    const bool was_shutdown = shutdown;
    bool silent = !asked  ||  shutdown;
    int done = owner  ?  0  :  samples;
    int len = samples;
    int zero_from = 0x7FFFFFFF;
    if (owner  &&  silent)
    {
        len = 0;
        zero_from = 0;
    }
    __syncthreads();

    auto next_bit = [&]() __attribute__((always_inline)) { return v18_next_bit(t); };

    for (;;)
    {
        const int lo = done;
        int nr = 0;
        if (owner  &&  done < samples)
        {
            if (silent)
                done = samples;
            else
                nr = ftx_walk(m, done, samples, shutdown, len, zero_from, r_start[lane], r_phase[lane], r_rate[lane], next_bit);
            silent = silent  ||  shutdown;
        }
        if (lane < kFtxCpw)
        {
            r_hdr[lane][0] = lo;
            r_hdr[lane][1] = done;
            r_hdr[lane][2] = nr;
            r_hdr[lane][3] = zero_from;
            r_hdr[lane][4] = scaling;
        }
        __syncthreads();
        ftx_render(quarter, r_hdr, r_start, r_phase, r_rate, L.pcm, L.stride, ch0, L.n_ch, samples, lane, L.vec != 0);
        if (!__syncthreads_or(done < samples))
            break;
    }

    if (owner)
    {
        if (asked)
        {
            if (!was_shutdown)
            {
                st[FT_CUR_RATE*n] = m.cur_rate;
                st[FT_PHASE*n] = (int32_t) m.phase;
                st[FT_BAUD_FRAC*n] = m.baud_frac;
                st[FT_SHUTDOWN*n] = shutdown  ?  1  :  0;
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
        st[FT_EVENT*n] = (shutdown  &&  !was_shutdown)  ?  1  :  0;
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

// The text layer of one receiver while a call runs: v18_tdd_put_async_byte() as the demodulator's put_bit
struct V18Rx
{
    int shift, suppression, status, count;
};

__device__ __forceinline__ void v18_put_byte(V18Rx &v, const uint8_t *decode, uint8_t *out, int cap, int byte)
{
    if (byte < 0)
    {
        // carrier up and down only reset rx_msg_len, which is always 0 between characters in these modes
        v.status |= (byte == -2)  ?  1  :  2;
        return;
    }
    if (v.suppression > 0)
        return;
    if (byte == kV18FigureShift)
    {
        v.shift = 1;
    }
    else if (byte == kV18LetterShift)
    {
        v.shift = 0;
    }
    else
    {
        if (v.count < cap)
            out[v.count] = decode[v.shift*32 + (byte & 0x1F)];
        v.count++;
    }
}

// v18_rx() x N: fsk_pair_kernel's two waves per 64 channels (fsk_dev.hpp, "A receiver over two waves"), framed, with the
// suppression timer stepped ahead of the samples and the Baudot decoder behind the framer.
__global__ __launch_bounds__(128) void v18_rx_kernel(const V18RxLaunch V)
{
    extern __shared__ int32_t win[];        // [4*span][64], then the two message buffers [2][kFskMsgWords][64]
    __shared__ uint32_t wave[kFskWave];
    const FskLaunch &L = V.f;
    const int lane = threadIdx.x & 63;
    const int side = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int ch = blockIdx.x*64 + lane;
    const bool live = ch < L.n_ch;
    const size_t n = (size_t) L.n_ch;
    const int span = L.span;
    int32_t *msg = win + 4*span*64;

    fsk_fill_wave(wave, L.quarter, threadIdx.x, 128);
    int32_t *st = L.st + (live  ?  ch  :  0);
    fsk_load_window_half(win, st + (size_t) kFskScalars*n, n, span, lane, side);
    __syncthreads();

    const int mylen = !live  ?  0  :  L.lens  ?  min(max(L.lens[ch], 0), L.samples)  :  L.samples;
    const int n_blk = (L.samples + 7) >> 3;
    const int16_t *pcm_row = L.pcm + (size_t) (live  ?  ch  :  0)*L.stride;
    if (side == 0)
    {
        FskSigSide s;
        fsk_sig_load(s, st, n);
        auto frame = [&](auto aligned) __attribute__((always_inline))
        {
            FskRow<decltype(aligned)::value> row;
            fsk_row_begin(row, pcm_row, mylen);
            for (int blk = 0;  blk <= n_blk;  blk++)
            {
                if (blk < n_blk)
                    fsk_sig_block(s, win, wave, msg + (blk & 1)*kFskMsgWords*64, lane, span, row, blk*8, max(0, min(8, mylen - blk*8)));
                __syncthreads();
            }
        };
        if (L.vec)
            frame(std::true_type{});
        else
            frame(std::false_type{});
        if (live)
            fsk_sig_store(s, st, n);
    }
    else
    {
        FskBitSide t;
        fsk_bit_load(t, st, n);
        int32_t *sv = V.sv + (live  ?  ch  :  0);
        V18Rx v;
        v.shift = sv[V18_BAUDOT_RX_SHIFT*n];
        v.suppression = sv[V18_RX_SUPPRESSION*n];
        v.status = 0;
        v.count = 0;
        // v18.c:1876-1884, ahead of the samples
        v.suppression = (v.suppression > mylen)  ?  (v.suppression - mylen)  :  0;
        const uint8_t *decode = V.tables + 128;
        uint8_t *out = V.chars + (size_t) (live  ?  ch  :  0)*V.cap;
        const int cap = live  ?  V.cap  :  0;
        auto emit = [&](int b) __attribute__((always_inline)) { v18_put_byte(v, decode, out, cap, b); };
        auto frame = [&](auto aligned) __attribute__((always_inline))
        {
            FskRow<decltype(aligned)::value> row;
            fsk_row_begin(row, pcm_row, mylen);
            for (int blk = 0;  blk <= n_blk;  blk++)
            {
                if (blk > 0)
                    fsk_bit_block<decltype(aligned)::value, true>(t, win, wave, msg + ((blk - 1) & 1)*kFskMsgWords*64, lane, span, row, (blk - 1)*8,
                                  max(0, min(8, mylen - (blk - 1)*8)), emit);
                __syncthreads();
            }
        };
        if (L.vec)
            frame(std::true_type{});
        else
            frame(std::false_type{});
        if (live)
        {
            fsk_bit_store(t, st, n);
            sv[V18_BAUDOT_RX_SHIFT*n] = v.shift;
            sv[V18_RX_SUPPRESSION*n] = v.suppression;
            sv[V18_RX_STATUS*n] = v.status;
            V.counts[ch] = v.count;
        }
    }
    if (live)
        fsk_store_window_half(win, st + (size_t) kFskScalars*n, n, span, lane, side);
}

}   // namespace spg
