// plc_dev.hpp -- packet loss concealment banks (the shape of spandsp's plc.c): one lane per line, plc_rx() on the lines that
// were heard and plc_fillin() on the lines that were not, mixed within a wave.
//
// The per-line functions are __host__ __device__ templates over the line's memory (its state words and its row), and the
// file compiles for the host (tests/c_callers/plc_host.cpp runs them one line at a time under ASan and UBSan); the kernel at
// the end is HIP only.
//
// State words of a line, st[word*n + ch], in the order of the reference's fields (src/spandsp/private/plc.h):
// missing_samples, pitch_offset, pitch, pitchbuf[0..119] (float bit patterns), history[0..279] (sign-extended, the
// reference's ring as it lies, not in time order), buf_ptr: 404.  The store is the reference's own form: get_state and
// set_state copy words, save_history() is the reference's three cases on one index, and normalise_history() is a rotation
// the wave does while it has the line's history in LDS for the search anyway.
//
// A line works on its history words in HBM.  A heard line with nothing missing (nearly every line of nearly every tick) reads
// its row in 16-byte chunks and writes `len` history words, and nothing else.  Two things have a working memory in LDS.  The
// pitch search of a line whose gap starts: 81 lags x 160 differences, run by the wave across its lanes on a row-major copy of
// the line's 280 samples (560 bytes a wave), where amp[lag + j] of neighbouring lanes are neighbouring halves and amp[j] is a
// broadcast.  And the cycle of pitch (pitchbuf) of a line inside a gap, a column of 120 floats a lane (30 720 bytes a wave, the
// lane as the fast index): read from the state in one burst before the line's loop and, where the gap starts, written to it
// in one burst behind it, so that the loop itself has no load from HBM between its stores.  What that bought was measured
// and is small; DESIGN.md 4.15 and profiles/plc_bank.md have the figures.
//
// Float arithmetic is the reference's, operation by operation, under -ffp-contract=off: the weights and the gain are serial
// chains of additions and subtractions (401 subtractions of 0.0025f take 1.0f to zero or below, not 400), 1.0f/overlap comes
// from a table the compiler folds (correctly rounded), fsaturate() is rintf() (round half to even) between the rails, and
// the fill loop truncates toward zero.

#pragma once

#include <stddef.h>
#include <stdint.h>
#include <math.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define PLC_HD __host__ __device__ __forceinline__
#define PLC_UNROLL _Pragma("unroll")
#define PLC_UNROLL_16 _Pragma("unroll 16")
#else
#define PLC_HD static inline
#define PLC_UNROLL
#define PLC_UNROLL_16
#endif

namespace spg
{

enum
{
    PW_MISSING = 0, PW_OFFSET, PW_PITCH,
    PW_PITCHBUF,                            // .. + 119
    PW_HISTORY = PW_PITCHBUF + 120,         // .. + 279
    PW_BUF_PTR = PW_HISTORY + 280,
    kPlcWords
};

// PLC_PITCH_MAX (the shortest lag), PLC_PITCH_MIN (the longest), CORRELATION_SPAN, PLC_HISTORY_LEN
enum { kPlcLagFirst = 40, kPlcLagLast = 120, kPlcSpan = 160, kPlcHist = 280 };

#define PLC_ATTENUATION_INCREMENT   0.0025f

// the scalar fields of a line, in registers
struct Plc
{
    int32_t missing, offset, pitch, buf_ptr;
};

// words a plc_state_t could hold, and a lane can index its words with
static inline bool plc_words_ok(const int32_t *w)
{
    // (280 is what an append that exactly fills the ring leaves, plc.c:78-79; it reads as 0 does)
    if (w[PW_BUF_PTR] < 0  ||  w[PW_BUF_PTR] > kPlcHist  ||  w[PW_MISSING] < 0)
        return false;
    for (int i = 0;  i < kPlcHist;  i++)
    {
        if (w[PW_HISTORY + i] < -32768  ||  w[PW_HISTORY + i] > 32767)
            return false;
    }
    if (w[PW_MISSING] > 0  &&  (w[PW_PITCH] < kPlcLagFirst  ||  w[PW_PITCH] > kPlcLagLast))
        return false;
    return w[PW_OFFSET] >= 0  &&  w[PW_OFFSET] <= ((w[PW_PITCH] > 1)  ?  w[PW_PITCH]  :  1) - 1;
}

// 1.0f/n for the overlaps there are (1 .. 30), folded by the compiler: correctly rounded on either side
PLC_HD float plc_recip(int n)
{
    constexpr float r[32] = {0.0f, 1.0f/1, 1.0f/2, 1.0f/3, 1.0f/4, 1.0f/5, 1.0f/6, 1.0f/7, 1.0f/8, 1.0f/9, 1.0f/10, 1.0f/11, 1.0f/12, 1.0f/13,
                             1.0f/14, 1.0f/15, 1.0f/16, 1.0f/17, 1.0f/18, 1.0f/19, 1.0f/20, 1.0f/21, 1.0f/22, 1.0f/23, 1.0f/24, 1.0f/25, 1.0f/26,
                             1.0f/27, 1.0f/28, 1.0f/29, 1.0f/30, 1.0f/31};
    return r[n & 31];
}

// fsaturate(): the float widens to the double exactly, lrint() of it is rintf() of the float
PLC_HD int32_t plc_fsaturate(float f)
{
    if (f > 32767.0f)
        return 32767;
    if (f < -32768.0f)
        return -32768;
    return (int32_t) rintf(f);
}

// ---- the pitch search, amdf_pitch() (plc.c:97-122), by parts: one lag's sum, and the combination of two (sum, lag) pairs.
// amp[] is the history in time order.  The reference scans the lags upward and takes the first strictly smaller sum: the
// lexicographic minimum of (sum, lag), which any order of combination finds.  (A sum is at most 160*65535.)

PLC_HD int32_t plc_lag_sum(const int16_t *amp, int lag)
{
    int32_t acc = 0;
    // (sixteen terms' reads at a time)
PLC_UNROLL_16
    for (int j = 0;  j < kPlcSpan;  j++)
    {
        const int32_t d = (int32_t) amp[lag + j] - (int32_t) amp[j];
        acc += (d < 0)  ?  -d  :  d;
    }
    return acc;
}

PLC_HD void plc_pair_min(int32_t &acc, int32_t &lag, int32_t acc2, int32_t lag2)
{
    const bool take = (acc2 < acc)  ||  (acc2 == acc  &&  lag2 < lag);
    acc = take  ?  acc2  :  acc;
    lag = take  ?  lag2  :  lag;
}

PLC_HD int plc_ring(int i)
{
    return (i >= kPlcHist)  ?  (i - kPlcHist)  :  i;
}

// ---- a line's memory M: hist(i) / set_hist(i, v), pb(i) / set_pb(i, f), set_row(i, v), row_load8(k, v[8]), row_store8(k, v[8])

// One cycle of pitch out of a history in time order (buf_ptr 0): plc.c:194-209
template <class M>
PLC_HD void plc_build_pitchbuf(M &m, int pitch)
{
    const int overlap = pitch >> 2;
    const int plain = pitch - overlap;
    const float new_step = plc_recip(overlap);
    float new_weight = new_step;
    // eight samples' loads, then their stores
    for (int b = 0;  b < pitch;  b += 8)
    {
        float h1[8];
        float h2[8];
PLC_UNROLL
        for (int e = 0;  e < 8;  e++)
        {
            const int i = b + e;
            h1[e] = (i < pitch)  ?  (float) m.hist(kPlcHist - pitch + i)  :  0.0f;
            h2[e] = (i >= plain  &&  i < pitch)  ?  (float) m.hist(kPlcHist - 2*pitch + i)  :  0.0f;
        }
PLC_UNROLL
        for (int e = 0;  e < 8;  e++)
        {
            const int i = b + e;
            if (i < plain)
                m.set_pb(i, h1[e]);
            else if (i < pitch)
            {
                m.set_pb(i, h1[e]*(1.0f - new_weight) + h2[e]*new_weight);
                new_weight += new_step;
            }
        }
    }
}

// plc_rx() (plc.c:125-172) for len > 0: the overlap with the synthetic signal where samples were missing, and save_history()
// (plc.c:57-80), in one pass over the row's chunks.  Only the overlapped samples are written to the row.
template <class M>
PLC_HD void plc_rx_line(M &m, Plc &s, int len)
{
    int overlap = 0;
    float old_step = 0.0f;
    float new_step = 0.0f;
    float old_weight = 0.0f;
    float new_weight = 0.0f;
    if (s.missing)
    {
        overlap = s.pitch >> 2;
        if (overlap > len)
            overlap = len;
        float gain = 1.0f - (float) s.missing*PLC_ATTENUATION_INCREMENT;
        if (gain < 0.0f)
            gain = 0.0f;
        new_step = plc_recip(overlap);
        old_step = new_step*gain;
        new_weight = new_step;
        old_weight = (1.0f - new_step)*gain;
        s.missing = 0;
    }
    const int start = (len > kPlcHist)  ?  (len - kPlcHist)  :  0;
    const int bp = (len >= kPlcHist)  ?  0  :  s.buf_ptr;
    // four chunks' loads, then their stores (see plc_build_pitchbuf())
    for (int k = (overlap > 0)  ?  0  :  (start >> 3);  8*k < len;  k += 4)
    {
        int16_t v[32] = {0};
PLC_UNROLL
        for (int c = 0;  c < 4;  c++)
        {
            if (8*(k + c) < len)
                m.row_load8(k + c, v + 8*c);
        }
PLC_UNROLL
        for (int e = 0;  e < 32;  e++)
        {
            const int i = 8*k + e;
            if (i < len)
            {
                int32_t x = v[e];
                if (i < overlap)
                {
                    x = plc_fsaturate(old_weight*m.pb(s.offset) + new_weight*(float) x);
                    m.set_row(i, x);
                    if (++s.offset >= s.pitch)
                        s.offset = 0;
                    new_weight += new_step;
                    old_weight -= old_step;
                    if (old_weight < 0.0f)
                        old_weight = 0.0f;
                }
                if (i >= start)
                    m.set_hist(plc_ring(bp + i - start), x);
            }
        }
    }
    s.buf_ptr = (len >= kPlcHist)  ?  0  :  ((bp + len > kPlcHist)  ?  (bp + len - kPlcHist)  :  (bp + len));
}

// plc_fillin() (plc.c:175-258) for len > 0.  Where the gap starts here (missing == 0) the caller has normalised the history
// (buf_ptr 0) and put the search's answer into s.pitch.  The reversed overlap, the decaying cycles, the zeros and
// save_history() in one pass; the row is written in whole chunks, zeros past len.
// (The overlap reads history[279 - i] for i < 30 while the pass has written history[0 .. i) at the most.)
template <class M>
PLC_HD void plc_fillin_line(M &m, Plc &s, int len)
{
    int overlap = 0;
    float old_step = 0.0f;
    float new_step = 0.0f;
    float old_weight = 0.0f;
    float new_weight = 0.0f;
    float gain;
    if (s.missing == 0)
    {
        plc_build_pitchbuf(m, s.pitch);
        overlap = s.pitch >> 2;
        new_step = plc_recip(overlap);
        old_step = new_step;
        new_weight = new_step;
        old_weight = 1.0f - new_step;
        if (overlap > len)
            overlap = len;
        gain = 1.0f;
        s.offset = overlap;
    }
    else
        gain = 1.0f - (float) s.missing*PLC_ATTENUATION_INCREMENT;
    const int start = (len > kPlcHist)  ?  (len - kPlcHist)  :  0;
    const int bp = (len >= kPlcHist)  ?  0  :  s.buf_ptr;
    int ahead = s.offset;
    for (int k = 0;  8*k < len;  k++)
    {
        // the chunk's loads first (see plc_build_pitchbuf()): the cycle's samples from where the offset will be -- it moves on
        // by one a sample for as long as the gain lasts, and past that nothing loaded is used
        float p[8];
        float h[8];
        int16_t v[8];
PLC_UNROLL
        for (int e = 0;  e < 8;  e++)
        {
            const int i = 8*k + e;
            p[e] = 0.0f;
            h[e] = 0.0f;
            if (i < overlap)
            {
                p[e] = m.pb(i);
                h[e] = (float) m.hist(kPlcHist - 1 - i);
            }
            else if (i < len  &&  gain > 0.0f)
            {
                p[e] = m.pb(ahead);
                if (++ahead >= s.pitch)
                    ahead = 0;
            }
        }
PLC_UNROLL
        for (int e = 0;  e < 8;  e++)
        {
            const int i = 8*k + e;
            int32_t x = 0;
            if (i < len)
            {
                if (i < overlap)
                {
                    x = plc_fsaturate(old_weight*h[e] + new_weight*p[e]);
                    new_weight += new_step;
                    old_weight -= old_step;
                    if (old_weight < 0.0f)
                        old_weight = 0.0f;
                }
                else if (gain > 0.0f)
                {
                    x = (int16_t) (int32_t) (p[e]*gain);
                    gain -= PLC_ATTENUATION_INCREMENT;
                    if (++s.offset >= s.pitch)
                        s.offset = 0;
                }
                if (i >= start)
                    m.set_hist(plc_ring(bp + i - start), x);
            }
            v[e] = (int16_t) x;
        }
        m.row_store8(k, v);
    }
    s.missing += len;
    s.buf_ptr = (len >= kPlcHist)  ?  0  :  ((bp + len > kPlcHist)  ?  (bp + len - kPlcHist)  :  (bp + len));
}

#if defined(__HIPCC__)

struct PlcLaunch
{
    int32_t *st;                // [kPlcWords][n_ch]
    uint8_t *rows;              // rows of `stride` bytes, 16-byte aligned
    const int32_t *ctl;         // [n_ch] 2*len + lost, or NULL: `ctl_all` for all
    const int32_t *counts;      // [n_ch] or NULL.  A count above 0: heard, that many samples (max_len at the most); 0: ctl
    long long stride;
    int n_ch;
    int ctl_all;
    int max_len;
};

struct PlcDevMem
{
    int32_t *st;                // the line's word 0
    size_t n;
    uint8_t *row;
    float *cycle;               // the lane's column of the wave's pitchbuf in LDS: sample i at cycle[64*i]

    __device__ __forceinline__ int32_t hist(int i) const { return st[(size_t) (PW_HISTORY + i)*n]; }
    __device__ __forceinline__ void set_hist(int i, int32_t v) { st[(size_t) (PW_HISTORY + i)*n] = v; }
    __device__ __forceinline__ float pb(int i) const { return cycle[64*i]; }
    __device__ __forceinline__ void set_pb(int i, float f) { cycle[64*i] = f; }
    // the state's pitchbuf[0 .. pitch) into the column (a line inside a gap), and back (a line whose gap started)
    __device__ __forceinline__ void cycle_load(int pitch)
    {
        for (int b = 0;  b < pitch;  b += 8)
        {
            int32_t t[8];
_Pragma("unroll")
            for (int e = 0;  e < 8;  e++)
                t[e] = (b + e < pitch)  ?  st[(size_t) (PW_PITCHBUF + b + e)*n]  :  0;
_Pragma("unroll")
            for (int e = 0;  e < 8;  e++)
            {
                if (b + e < pitch)
                    cycle[64*(b + e)] = __int_as_float(t[e]);
            }
        }
    }
    __device__ __forceinline__ void cycle_store(int pitch)
    {
        for (int i = 0;  i < pitch;  i++)
            st[(size_t) (PW_PITCHBUF + i)*n] = __float_as_int(cycle[64*i]);
    }
    __device__ __forceinline__ void set_row(int i, int32_t v) { ((int16_t *) row)[i] = (int16_t) v; }
    __device__ __forceinline__ void row_load8(int k, int16_t v[8]) const
    {
        const uint4 q = *(const uint4 *) (row + 16*(size_t) k);
        v[0] = (int16_t) q.x;  v[1] = (int16_t) (q.x >> 16);  v[2] = (int16_t) q.y;  v[3] = (int16_t) (q.y >> 16);
        v[4] = (int16_t) q.z;  v[5] = (int16_t) (q.z >> 16);  v[6] = (int16_t) q.w;  v[7] = (int16_t) (q.w >> 16);
    }
    __device__ __forceinline__ void row_store8(int k, const int16_t v[8])
    {
        *(uint4 *) (row + 16*(size_t) k) = make_uint4((uint16_t) v[0] | ((uint32_t) (uint16_t) v[1] << 16), (uint16_t) v[2] | ((uint32_t) (uint16_t) v[3] << 16),
                                                      (uint16_t) v[4] | ((uint32_t) (uint16_t) v[5] << 16), (uint16_t) v[6] | ((uint32_t) (uint16_t) v[7] << 16));
    }
};

// One wave a block, one lane a line.  First the wave, together, for each of its lines whose gap starts in this call: the
// line's history in time order into LDS, the 81 lags over the lanes (40 .. 103, then 104 .. 120 on lanes 0 .. 16), the
// lexicographic minimum across the lanes, and the history back in time order (normalise_history()).  Then every lane its line.
__global__ __launch_bounds__(64) void plc_kernel(const PlcLaunch L)
{
    __shared__ __attribute__((aligned(16))) int16_t amp[kPlcHist];
    __shared__ float cycles[kPlcLagLast*64];
    const int lane = threadIdx.x;
    const int ch = blockIdx.x*64 + lane;
    const size_t n = (size_t) L.n_ch;
    int len = 0;
    bool lost = false;
    if (ch < L.n_ch)
    {
        const int ctl = L.ctl  ?  L.ctl[ch]  :  L.ctl_all;
        const int heard = L.counts  ?  L.counts[ch]  :  0;
        lost = (heard <= 0)  &&  (ctl & 1);
        len = (heard > 0)  ?  heard  :  (ctl >> 1);
        len = min(max(len, 0), L.max_len);
    }
    Plc s = {0, 0, 0, 0};
    PlcDevMem m = {L.st + ((ch < L.n_ch)  ?  ch  :  0), n, L.rows + (size_t) ((ch < L.n_ch)  ?  ch  :  0)*(size_t) L.stride, cycles + lane};
    if (len > 0)
    {
        s.missing = m.st[(size_t) PW_MISSING*n];
        s.offset = m.st[(size_t) PW_OFFSET*n];
        s.pitch = m.st[(size_t) PW_PITCH*n];
        s.buf_ptr = m.st[(size_t) PW_BUF_PTR*n];
    }
    // (the ballot is the wave's: every lane of the block is here, and the loop below is uniform)
    unsigned long long starting = __ballot(len > 0  &&  lost  &&  s.missing == 0);
    while (starting)
    {
        const int owner = __ffsll((long long) starting) - 1;
        starting &= starting - 1;
        int32_t *line = L.st + (size_t) (blockIdx.x*64 + owner);
        const int bp = __shfl(s.buf_ptr, owner);
        for (int i = lane;  i < kPlcHist;  i += 64)
            amp[i] = (int16_t) line[(size_t) (PW_HISTORY + plc_ring(bp + i))*n];
        __syncthreads();
        int32_t lag = kPlcLagFirst + lane;
        int32_t acc = plc_lag_sum(amp, lag);
        if (lane <= kPlcLagLast - kPlcLagFirst - 64)
            plc_pair_min(acc, lag, plc_lag_sum(amp, lag + 64), lag + 64);
        for (int off = 32;  off > 0;  off >>= 1)
        {
            const int32_t acc2 = __shfl_xor(acc, off);
            const int32_t lag2 = __shfl_xor(lag, off);
            plc_pair_min(acc, lag, acc2, lag2);
        }
        if (bp != 0)
        {
            for (int i = lane;  i < kPlcHist;  i += 64)
                line[(size_t) (PW_HISTORY + i)*n] = amp[i];
        }
        if (lane == owner)
        {
            s.pitch = lag;
            s.buf_ptr = 0;
        }
        // the owner reads these words below, and the next line's samples replace these
        __syncthreads();
    }
    if (len == 0)
        return;
    const bool in_gap = (s.missing > 0);
    if (in_gap)
        m.cycle_load(s.pitch);
    if (lost)
        plc_fillin_line(m, s, len);
    else
        plc_rx_line(m, s, len);
    if (lost  &&  !in_gap)
        m.cycle_store(s.pitch);
    m.st[(size_t) PW_MISSING*n] = s.missing;
    m.st[(size_t) PW_OFFSET*n] = s.offset;
    m.st[(size_t) PW_PITCH*n] = s.pitch;
    m.st[(size_t) PW_BUF_PTR*n] = s.buf_ptr;
}

#endif  // __HIPCC__

}   // namespace spg
