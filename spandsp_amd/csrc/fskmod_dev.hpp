// fskmod_dev.hpp -- the FSK modulator of the sender banks: fsk_tx() as every family with an FSK sender in it runs it (the
// FSK banks themselves and the FAX transmit front end, fsktx_dev.hpp; the V.18 text banks, v18_dev.hpp; the caller-ID banks,
// adsi_dev.hpp).  A family brings its bit source and says whether the modulator is asked at all; the rest is here.
//
// What is restated (reference paths relative to the reference tree):
//   fsk_tx()                       src/fsk.c:162-198
//   dds_mod()                      src/dds_int.c:380-387   (dds_lookup(): dds_dev.hpp)
//
// The generator is integer only, and its DDS phase accumulator is uint32 and wraps, so every sample is a closed form of its
// index: phase(i) = phase0 + (number of samples before i)*rate.  A call is rounds of two phases (the shape of tx_bank_kernel,
// txgen_dev.hpp), 16 channels to a wave:
//   phase 1 (one lane per channel): walk the channel's bit boundaries and leave RUNS -- stretches of samples with one
//            phase rate -- in LDS, consuming bits as it goes; no per-sample work;
//   phase 2 (all 64 lanes over the wave's channels): a lane renders 8 adjacent samples (16 bytes) from the run(s) they
//            fall in, so the stores of a channel's row are full and contiguous.
// A channel with more runs than fit takes another round.  Samples a channel does not produce (after shutdown) are written
// as 0; the per-channel length is what the reference would have returned.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dds_dev.hpp"

namespace spg
{

// dds_mod() without the accumulator update, dds_int.c:380-387
__device__ __forceinline__ int ftx_dds_mod(const int16_t *quarter, uint32_t phase, int scale)
{
    return (int) (int16_t) ((dds_int_lookup(quarter, phase)*scale) >> 15);
}

// Eight samples of one row: one 16-byte store when the chunk is whole and the row allows it.
__device__ __forceinline__ void ftx_store8(int16_t *at, const int v[8], int first, int last, bool vec)
{
    if (vec  &&  first == 0  &&  last == 8)
    {
        uint4 w;
        w.x = ((uint32_t) v[0] & 0xFFFFu) | ((uint32_t) v[1] << 16);
        w.y = ((uint32_t) v[2] & 0xFFFFu) | ((uint32_t) v[3] << 16);
        w.z = ((uint32_t) v[4] & 0xFFFFu) | ((uint32_t) v[5] << 16);
        w.w = ((uint32_t) v[6] & 0xFFFFu) | ((uint32_t) v[7] << 16);
        *reinterpret_cast<uint4 *>(at) = w;
        return;
    }
#pragma unroll
    for (int j = 0;  j < 8;  j++)
    {
        if (j >= first  &&  j < last)
            at[j] = (int16_t) v[j];
    }
}

enum
{
    FT_BAUD_RATE = 0,       // baud x 100
    FT_RATE0 = 1,           // phase_rates[0] (space), [1] (mark)
    FT_RATE1 = 2,
    FT_SCALING = 3,
    FT_CUR_RATE = 4,        // current_phase_rate
    FT_PHASE = 5,           // phase_acc
    FT_BAUD_FRAC = 6,
    FT_SHUTDOWN = 7,
    FT_LFSR = 8,            // bit source SPANGPU_FSKTX_LFSR: the x^15 + x^14 + 1 register
    FT_QRD = 9,             // bit source SPANGPU_FSKTX_QUEUE: read position and fill of the channel's ring, in bits
    FT_QCOUNT = 10,
    FT_EOD = 11,            // an empty ring answers SIG_STATUS_END_OF_DATA instead of a mark
    FT_EVENT = 12,          // the channel shut down in the last call
    kFskTxWords = 13
};

constexpr int kFtxBaudUnit = 8000*100;      // SAMPLE_RATE*100
constexpr int kFtxWaves = 4;                // waves per workgroup; they share one copy of the quarter sine
constexpr int kFtxCpw = 16;                 // channels per wave
constexpr int kFtxRuns = 32;                // runs of a channel per round: 1200 baud x 160 samples has 25
constexpr int kFtxRunStride = kFtxRuns + 1; // odd: the 16 owner lanes write 16 different LDS banks

// The modulator's words while a call runs (fsk.c: baud_rate, phase_rates[], current_phase_rate, phase_acc, baud_frac)
struct FtxMod
{
    int baud_rate;
    int rate0;
    int rate1;
    int cur_rate;
    int baud_frac;
    uint32_t phase;
};

// Phase 1 of a round for one channel: the runs from sample `done` on, at most kFtxRuns of them, into the channel's LDS rows.
// next_bit() stands for get_bit(): 0 or 1, or a negative value for SIG_STATUS_END_OF_DATA (fsk.c:179-189: the sample is not
// made, the channel is shut down, `len` is what fsk_tx() returns).  Returns the number of runs.
template <class NextBit>
__device__ __forceinline__ int ftx_walk(FtxMod &m, int &done, int samples, bool &shutdown, int &len, int &zero_from, int32_t *r_start,
                                        int32_t *r_phase, int32_t *r_rate, NextBit &&next_bit)
{
    r_start[0] = done;
    r_phase[0] = (int32_t) m.phase;
    r_rate[0] = m.cur_rate;
    int nr = 1;
    while (nr < kFtxRuns)
    {
        // the first sample k >= 0 ahead with baud_frac + (k + 1)*baud_rate >= 800000 (fsk.c:176); advancing
        // run by run keeps every product inside 32 bits whatever the length of the call
        const int kb = (kFtxBaudUnit - m.baud_frac + m.baud_rate - 1)/m.baud_rate - 1;
        if (kb >= samples - done)
        {
            const int k = samples - done;
            m.phase += (uint32_t) k*(uint32_t) m.cur_rate;
            m.baud_frac += k*m.baud_rate;
            done = samples;
            break;
        }
        m.phase += (uint32_t) kb*(uint32_t) m.cur_rate;
        done += kb;
        m.baud_frac += (kb + 1)*m.baud_rate - kFtxBaudUnit;
        const int bit = next_bit();
        if (bit < 0)
        {
            // SIG_STATUS_END_OF_DATA, fsk.c:179-189: this sample is not made
            shutdown = true;
            len = done;
            zero_from = done;
            done = samples;
            break;
        }
        m.cur_rate = bit  ?  m.rate1  :  m.rate0;
        r_start[nr] = done;
        r_phase[nr] = (int32_t) m.phase;
        r_rate[nr] = m.cur_rate;
        nr++;
        m.phase += (uint32_t) m.cur_rate;
        done++;
        if (done >= samples)
            break;
    }
    return nr;
}

// Phase 2 of a round for a wave: the samples of its channels' runs, 8 per lane.  r_hdr[c] = lo, hi, runs, zero_from, scaling, and
// with SPANS the sample of the row the channel's call starts at.
template <bool SPANS = false>
__device__ __forceinline__ void ftx_render(const int16_t *quarter, const int32_t (*r_hdr)[8], const int32_t (*r_start)[kFtxRunStride],
                                           const int32_t (*r_phase)[kFtxRunStride], const int32_t (*r_rate)[kFtxRunStride], int16_t *pcm,
                                           long long stride, int ch0, int n_ch, int samples, int lane, bool vec)
{
    const int nchan = (n_ch - ch0 < kFtxCpw)  ?  (n_ch - ch0)  :  kFtxCpw;
    const int cpr = (samples + 7) >> 3;
    const int total = nchan*cpr;
    for (int idx = lane;  idx < total;  idx += 64)
    {
        const int c = idx/cpr;
        const int i0 = (idx - c*cpr)*8;
        const int4 hdr = *reinterpret_cast<const int4 *>(&r_hdr[c][0]);     // lo, hi, runs, zero_from
        const int a = (i0 > hdr.x)  ?  i0  :  hdr.x;
        const int b = (i0 + 8 < hdr.y)  ?  (i0 + 8)  :  hdr.y;
        if (a >= b)
            continue;
        const int scale = r_hdr[c][4];
        const int32_t *S = r_start[c];
        int r = 0;
#pragma unroll
        for (int step = kFtxRuns/2;  step > 0;  step >>= 1)
            r += (r + step < hdr.z  &&  S[r + step] <= a)  ?  step  :  0;
        int rate = 0;
        uint32_t ph = 0u;
        int next = 0x7FFFFFFF;
        if (hdr.z > 0)
        {
            rate = r_rate[c][r];
            ph = (uint32_t) r_phase[c][r] + (uint32_t) (a - S[r])*(uint32_t) rate;
            next = (r + 1 < hdr.z)  ?  S[r + 1]  :  0x7FFFFFFF;
        }
        int v[8];
#pragma unroll
        for (int j = 0;  j < 8;  j++)
        {
            const int i = i0 + j;
            v[j] = 0;
            if (i >= a  &&  i < b)
            {
                while (i >= next)
                {
                    r++;
                    rate = r_rate[c][r];
                    ph = (uint32_t) r_phase[c][r];
                    next = (r + 1 < hdr.z)  ?  S[r + 1]  :  0x7FFFFFFF;
                }
                if (i < hdr.w  &&  hdr.z > 0)
                    v[j] = ftx_dds_mod(quarter, ph, scale);
                ph += (uint32_t) rate;
            }
        }
        ftx_store8(pcm + (size_t) (ch0 + c)*stride + (SPANS  ?  r_hdr[c][5]  :  0) + i0, v, a - i0, b - i0, vec);
    }
}

// The LDS of a sender workgroup: the quarter sine, and this wave's rows of the runs and their headers
struct FtxLds
{
    const int16_t *quarter;
    int32_t (*r_start)[kFtxRunStride];
    int32_t (*r_phase)[kFtxRunStride];
    int32_t (*r_rate)[kFtxRunStride];
    int32_t (*r_hdr)[8];
};

// (the caller's next barrier completes the fill of the quarter sine)
__device__ __forceinline__ FtxLds ftx_lds(const int16_t *quarter_hbm)
{
    __shared__ int16_t quarter[258];
    __shared__ int32_t all_start[kFtxWaves][kFtxCpw][kFtxRunStride];
    __shared__ int32_t all_phase[kFtxWaves][kFtxCpw][kFtxRunStride];
    __shared__ int32_t all_rate[kFtxWaves][kFtxCpw][kFtxRunStride];
    __shared__ __attribute__((aligned(16))) int32_t all_hdr[kFtxWaves][kFtxCpw][8];

    const int wave = threadIdx.x >> 6;
    for (int i = threadIdx.x;  i < 257;  i += 64*kFtxWaves)
        quarter[i] = quarter_hbm[i];
    return {quarter, all_start[wave], all_phase[wave], all_rate[wave], all_hdr[wave]};
}

// One channel's modulator while a call runs; a lane that owns no channel has one that is shut down
struct FtxChan
{
    FtxMod m;
    int scaling;
    bool shutdown;
    bool was_shutdown;
};

__device__ __forceinline__ void ftx_chan_load(FtxChan &c, const int32_t *st, size_t n, bool owner)
{
    c.m = {1, 0, 0, 0, 0, 0u};
    c.scaling = 0;
    c.shutdown = true;
    if (owner)
    {
        c.m.baud_rate = st[FT_BAUD_RATE*n];
        c.m.rate0 = st[FT_RATE0*n];
        c.m.rate1 = st[FT_RATE1*n];
        c.scaling = st[FT_SCALING*n];
        c.m.cur_rate = st[FT_CUR_RATE*n];
        c.m.phase = (uint32_t) st[FT_PHASE*n];
        c.m.baud_frac = st[FT_BAUD_FRAC*n];
        c.shutdown = st[FT_SHUTDOWN*n] != 0;
    }
    c.was_shutdown = c.shutdown;
}

// (for an owner whose modulator was asked and was not shut down when the call began; FT_EVENT is every owner's)
__device__ __forceinline__ void ftx_chan_store(const FtxChan &c, int32_t *st, size_t n)
{
    st[FT_CUR_RATE*n] = c.m.cur_rate;
    st[FT_PHASE*n] = (int32_t) c.m.phase;
    st[FT_BAUD_FRAC*n] = c.m.baud_frac;
    st[FT_SHUTDOWN*n] = c.shutdown  ?  1  :  0;
}

__device__ __forceinline__ void ftx_event_store(const FtxChan &c, int32_t *st, size_t n)
{
    st[FT_EVENT*n] = (c.shutdown  &&  !c.was_shutdown)  ?  1  :  0;
}

// The rounds of a call, for the whole workgroup: an owner walks its channel from `done` to `samples` (a silent one -- its
// modulator is not asked, or is shut down -- makes no runs, and what is left of its call is written as 0), then the wave
// renders.  len = what fsk_tx() returns so far, zero_from = the first sample that is not made; both in the coordinates of
// `done`.  With SPANS a channel's call is `samples` long from sample `start` of its row; row_samples is the row's length.
template <bool SPANS = false, class NextBit>
__device__ __forceinline__ void ftx_rounds(const FtxLds &lds, FtxChan &c, bool owner, bool silent, int &done, int samples, int &len,
                                           int &zero_from, int start, int16_t *pcm, long long stride, int ch0, int n_ch, int row_samples,
                                           bool vec, NextBit &&next_bit)
{
    const int lane = threadIdx.x & 63;
    for (;;)
    {
        // ---- phase 1: the next runs of my channel ----
        const int lo = done;
        int nr = 0;
        if (owner  &&  done < samples)
        {
            if (silent)
                done = samples;
            else
                nr = ftx_walk(c.m, done, samples, c.shutdown, len, zero_from, lds.r_start[lane], lds.r_phase[lane], lds.r_rate[lane], next_bit);
            silent = silent  ||  c.shutdown;
        }
        if (lane < kFtxCpw)
        {
            lds.r_hdr[lane][0] = lo;
            lds.r_hdr[lane][1] = done;
            lds.r_hdr[lane][2] = nr;
            lds.r_hdr[lane][3] = zero_from;
            lds.r_hdr[lane][4] = c.scaling;
            if (SPANS)
                lds.r_hdr[lane][5] = start;
        }
        __syncthreads();

        // ---- phase 2: the samples of those runs, 8 per lane ----
        ftx_render<SPANS>(lds.quarter, lds.r_hdr, lds.r_start, lds.r_phase, lds.r_rate, pcm, stride, ch0, n_ch, row_samples, lane, vec);
        if (!__syncthreads_or(done < samples))
            break;
    }
}

}   // namespace spg
