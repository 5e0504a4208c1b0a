// fsktx_dev.hpp -- device side of the FSK and modem connect tone transmitter banks (the last
// two signal sources): N fsk_tx() / modem_connect_tones_tx() generators, state in HBM, one launch per call.
//
// What is restated (reference paths relative to the reference tree):
//   fsk_tx()                       src/fsk.c:162-198       fsk_tx_restart()   src/fsk.c:221-235
//   modem_connect_tones_tx()       src/modem_connect_tones.c:114-299          _tx_init()   :302-403
//
// The FSK modulator -- the runs, their walk and their rendering, the round loop -- is fskmod_dev.hpp, which the V.18 and
// caller-ID senders share; here are the FSK banks' bit sources around it, and the connect tone sender, which has the same
// two phases per round (phase 1, a lane per channel, leaves tone bursts in LDS; phase 2, all 64 lanes, renders 8 samples
// each) with a round of its own.  State is structure-of-arrays int32 words [words][n_channels].
//
// Under the FAX transmit front end (txspan_dev.hpp) the same two kernel bodies run with every channel on its own span of the
// row: phase 1 walks the channel's `count` samples, phase 2 renders them at row[start ..], unaligned.  The FSK sender then takes
// hdlc_tx_get_bit() as its get_bit.
//
// Samples a channel does not produce (after shutdown, after a finite tone's end, the sample the reference skips when a
// cadence wraps inside a call) are written as 0; the per-channel length is what the reference would have returned.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fskmod_dev.hpp"
#include "txspan_dev.hpp"

namespace spg
{

// ---- fsk_tx() ---------------------------------------------------------------------------------------------------------

enum { FTX_SRC_LFSR = 0, FTX_SRC_QUEUE = 1 };

struct FskTxLaunch
{
    int32_t *st;
    const int16_t *quarter;     // [257] in HBM
    uint32_t *queue;            // [qring/32][n_ch] packed bits, LSB first, or null
    int16_t *pcm;               // [n_ch][stride]
    int32_t *lens;              // [n_ch] or null
    long long stride;
    int n_ch;
    int samples;
    int source;
    int qring;                  // ring size in bits, a multiple of 32
    int vec;                    // rows are 16-byte aligned
    TxSpans sp;                 // fsktx_span_kernel only
};

template <bool SPANS>
__device__ __forceinline__ void fsktx_bank_body(const FskTxLaunch &L)
{
    const int lane = threadIdx.x & 63;
    const int ch0 = (blockIdx.x*kFtxWaves + (threadIdx.x >> 6))*kFtxCpw;
    const int ch = ch0 + lane;
    const size_t n = (size_t) L.n_ch;
    bool owner = (lane < kFtxCpw)  &&  (ch < L.n_ch);
    // the call my channel makes: the whole row, or its span of it (a channel without one is nobody's: nothing of it is touched)
    int samples = L.samples;
    int start = 0;
    if (SPANS)
    {
        if (owner)
            owner = span_of(L.sp, n, ch, L.samples, start, samples);
        samples = owner  ?  samples  :  0;
    }
    const FtxLds lds = ftx_lds(L.quarter);

    int32_t *st = L.st + (owner  ?  ch  :  0);
    SpanFramer fr;
    FtxChan c;
    ftx_chan_load(c, st, n, owner);
    uint32_t lfsr = 0u;
    int qrd = 0;
    int qcount = 0;
    bool eod = false;
    if (owner)
    {
        if (SPANS)
        {
            fr.open(L.sp, n, ch);
        }
        else if (L.source == FTX_SRC_LFSR)
        {
            lfsr = (uint32_t) st[FT_LFSR*n];
        }
        else
        {
            qrd = st[FT_QRD*n];
            qcount = st[FT_QCOUNT*n];
            eod = st[FT_EOD*n] != 0;
        }
    }
    int done = owner  ?  0  :  samples;
    int len = samples;          // what fsk_tx() returns
    int zero_from = 0x7FFFFFFF;
    if (owner  &&  c.shutdown)
    {
        len = 0;
        zero_from = 0;
    }
    __syncthreads();

    auto next_bit = [&]() __attribute__((always_inline))
    {
        int bit;
        if (SPANS)
        {
            bit = fr.bit();         // hdlc_tx_get_bit(): 0, 1 or SIG_STATUS_END_OF_DATA
        }
        else if (L.source == FTX_SRC_LFSR)
        {
            bit = (int) (((lfsr >> 14) ^ (lfsr >> 13)) & 1u);
            lfsr = ((lfsr << 1) | (uint32_t) bit) & 0x7FFFu;
        }
        else if (qcount > 0)
        {
            bit = (int) ((L.queue[(size_t) (qrd >> 5)*n + ch] >> (qrd & 31)) & 1u);
            qrd = (qrd + 1 == L.qring)  ?  0  :  (qrd + 1);
            qcount--;
        }
        else
        {
            bit = eod  ?  -1  :  1;     // SIG_STATUS_END_OF_DATA, or an idle mark with nothing consumed
        }
        return bit;
    };
    // (a span starts at any sample of its row: no 16-byte stores)
    ftx_rounds<SPANS>(lds, c, owner, c.shutdown, done, samples, len, zero_from, start, L.pcm, L.stride, ch0, L.n_ch, L.samples,
                      !SPANS  &&  L.vec != 0, next_bit);

    if (owner)
    {
        if (!c.was_shutdown)
        {
            ftx_chan_store(c, st, n);
            if (SPANS)
            {
                // (nothing of the bank's own bit sources moved)
            }
            else if (L.source == FTX_SRC_LFSR)
            {
                st[FT_LFSR*n] = (int32_t) lfsr;
            }
            else
            {
                st[FT_QRD*n] = qrd;
                st[FT_QCOUNT*n] = qcount;
            }
        }
        ftx_event_store(c, st, n);
        if (SPANS)
        {
            fr.close(L.sp, n, ch);
            L.sp.ret[ch] = len;
        }
        else if (L.lens)
            L.lens[ch] = len;
    }
}

__global__ __launch_bounds__(64*kFtxWaves) void fsktx_bank_kernel(const FskTxLaunch L)
{
    fsktx_bank_body<false>(L);
}

// every channel on its own span of the row, its bits from hdlc_tx_get_bit() (txspan_dev.hpp)
__global__ __launch_bounds__(64*kFtxWaves) void fsktx_span_kernel(const FskTxLaunch L)
{
    fsktx_bank_body<true>(L);
}

// ---- modem_connect_tones_tx() -----------------------------------------------------------------------------------------

enum
{
    MTX_TIMER = 0,          // duration_timer
    MTX_HOP = 1,            // hop_timer
    MTX_TONE_PHASE = 2,
    MTX_MOD_PHASE = 3,
    kMctTxWords = 4
};

constexpr int kMtxRuns = 4;         // tone bursts of a channel per round
constexpr int kMtxHop = 3600;       // milliseconds_to_samples(450)

struct MctTxLaunch
{
    int32_t *st;
    const int16_t *quarter;
    int16_t *pcm;
    int32_t *lens;
    long long stride;
    int n_ch;
    int samples;
    int vec;
    // the tone type, as modem_connect_tones_tx_init() sets it up
    int cadenced;           // FAX CNG and the calling tone: tone and silence for ever; the others end
    int hops;               // the /PR types
    int am;                 // the ANSam types
    int tone_rate;
    int mod_rate;
    int level;
    int mod_level;
    int tone_len;           // finite: samples of tone at the end of the timer; cadenced: samples of silence per cycle
    int period;             // cadenced: samples per cycle
    TxSpans sp;             // mcttx_span_kernel only
};

template <bool SPANS>
__device__ __forceinline__ void mcttx_bank_body(const MctTxLaunch &L)
{
    __shared__ int16_t quarter[258];
    __shared__ __attribute__((aligned(16))) int32_t all_runs[kFtxWaves][kFtxCpw][kMtxRuns][4];  // start, end, phase
    __shared__ __attribute__((aligned(16))) int32_t all_hdr[kFtxWaves][kFtxCpw][8];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    int32_t (*runs)[kMtxRuns][4] = all_runs[wave];
    int32_t (*r_hdr)[8] = all_hdr[wave];
    const int ch0 = (blockIdx.x*kFtxWaves + wave)*kFtxCpw;
    const int ch = ch0 + lane;
    const size_t n = (size_t) L.n_ch;
    bool owner = (lane < kFtxCpw)  &&  (ch < L.n_ch);
    int samples = L.samples;
    int start = 0;
    if (SPANS)
    {
        if (owner)
            owner = span_of(L.sp, n, ch, L.samples, start, samples);
        samples = owner  ?  samples  :  0;
    }

    for (int i = threadIdx.x;  i < 257;  i += 64*kFtxWaves)
        quarter[i] = L.quarter[i];

    int32_t *st = L.st + (owner  ?  ch  :  0);
    int timer = 0;
    int hop = 0;
    uint32_t tone_phase = 0u;
    uint32_t mod_phase = 0u;
    if (owner)
    {
        timer = st[MTX_TIMER*n];
        hop = st[MTX_HOP*n];
        tone_phase = (uint32_t) st[MTX_TONE_PHASE*n];
        mod_phase = (uint32_t) st[MTX_MOD_PHASE*n];
    }
    int done = owner  ?  0  :  samples;
    int len = samples;
    __syncthreads();

    for (;;)
    {
        // ---- phase 1 ----
        const int lo = done;
        int nr = 0;
        int hop0 = 0x7FFFFFFF;
        const uint32_t mod0 = mod_phase;
        if (owner  &&  done < samples)
        {
            if (!L.cadenced)
            {
                // modem_connect_tones.c:155-172 and its four likes: the call is clipped to what is left of the tone
                len = (timer < samples)  ?  timer  :  samples;
                int lead = 0;
                if (timer > L.tone_len)
                    lead = (timer - L.tone_len > len)  ?  len  :  (timer - L.tone_len);
                const int m = len - lead;
                runs[lane][0][0] = lead;
                runs[lane][0][1] = len;
                runs[lane][0][2] = (int32_t) tone_phase;
                nr = 1;
                uint32_t nh = 0u;
                if (L.hops)
                {
                    // --hop_timer <= 0 before tone sample k (from 0): k + 1 >= hop, then every 3600 samples
                    hop0 = hop;
                    if (m >= hop)
                    {
                        nh = 1u + (uint32_t) (m - hop)/(uint32_t) kMtxHop;
                        hop = kMtxHop - (m - hop)%kMtxHop;
                    }
                    else
                    {
                        hop -= m;
                    }
                }
                tone_phase += (uint32_t) m*(uint32_t) L.tone_rate + (nh << 31);
                mod_phase += (uint32_t) m*(uint32_t) L.mod_rate;
                timer -= len;
                done = samples;
            }
            else
            {
                // modem_connect_tones.c:125-154 / :264-293
                while (done < samples  &&  nr < kMtxRuns)
                {
                    if (timer > L.tone_len)
                    {
                        int m = timer - L.tone_len;
                        m = (m > samples - done)  ?  (samples - done)  :  m;
                        runs[lane][nr][0] = done;
                        runs[lane][nr][1] = done + m;
                        runs[lane][nr][2] = (int32_t) tone_phase;
                        nr++;
                        tone_phase += (uint32_t) m*(uint32_t) L.tone_rate;
                        timer -= m;
                        done += m;
                    }
                    if (timer > 0)
                    {
                        int m = timer;
                        m = (m > samples - done)  ?  (samples - done)  :  m;
                        timer -= m;
                        done += m;
                    }
                    if (timer == 0)
                    {
                        // the cycle starts again; inside a call the reference's loop increment steps over one sample,
                        // which is neither written nor counted
                        timer = L.period;
                        if (done < samples)
                            done++;
                    }
                }
            }
        }
        if (lane < kFtxCpw)
        {
            r_hdr[lane][0] = lo;
            r_hdr[lane][1] = done;
            r_hdr[lane][2] = nr;
            r_hdr[lane][3] = hop0;
            r_hdr[lane][4] = (int32_t) mod0;
            if (SPANS)
                r_hdr[lane][5] = start;
        }
        __syncthreads();

        // ---- phase 2 ----
        {
            const int nchan = (L.n_ch - ch0 < kFtxCpw)  ?  (L.n_ch - ch0)  :  kFtxCpw;
            const int cpr = (L.samples + 7) >> 3;
            const int total = nchan*cpr;
            for (int idx = lane;  idx < total;  idx += 64)
            {
                const int c = idx/cpr;
                const int i0 = (idx - c*cpr)*8;
                const int4 hdr = *reinterpret_cast<const int4 *>(&r_hdr[c][0]);     // lo, hi, runs, hop timer
                const int a = (i0 > hdr.x)  ?  i0  :  hdr.x;
                const int b = (i0 + 8 < hdr.y)  ?  (i0 + 8)  :  hdr.y;
                if (a >= b)
                    continue;
                const uint32_t mod0c = (uint32_t) r_hdr[c][4];
                int4 run = make_int4(0, 0, 0, 0);
                int r = -1;
                int v[8];
#pragma unroll
                for (int j = 0;  j < 8;  j++)
                {
                    const int i = i0 + j;
                    v[j] = 0;
                    if (i >= a  &&  i < b)
                    {
                        while (i >= run.y  &&  r + 1 < hdr.z)
                        {
                            r++;
                            run = *reinterpret_cast<const int4 *>(&runs[c][r][0]);
                        }
                        if (i >= run.x  &&  i < run.y)
                        {
                            const uint32_t k = (uint32_t) (i - run.x);
                            uint32_t ph = (uint32_t) run.z + k*(uint32_t) L.tone_rate;
                            if ((int) (k + 1u) >= hdr.w)
                                ph += (1u + (k + 1u - (uint32_t) hdr.w)/(uint32_t) kMtxHop) << 31;
                            int scale = L.level;
                            if (L.am)
                                scale = (int) (int16_t) (L.level + ftx_dds_mod(quarter, mod0c + k*(uint32_t) L.mod_rate, L.mod_level));
                            v[j] = ftx_dds_mod(quarter, ph, scale);
                        }
                    }
                }
                ftx_store8(L.pcm + (size_t) (ch0 + c)*L.stride + (SPANS  ?  r_hdr[c][5]  :  0) + i0, v, a - i0, b - i0, !SPANS  &&  L.vec != 0);
            }
        }
        if (!__syncthreads_or(done < samples))
            break;
    }

    if (owner)
    {
        st[MTX_TIMER*n] = timer;
        st[MTX_HOP*n] = hop;
        st[MTX_TONE_PHASE*n] = (int32_t) tone_phase;
        st[MTX_MOD_PHASE*n] = (int32_t) mod_phase;
        if (SPANS)
            L.sp.ret[ch] = len;
        else if (L.lens)
            L.lens[ch] = len;
    }
}

__global__ __launch_bounds__(64*kFtxWaves) void mcttx_bank_kernel(const MctTxLaunch L)
{
    mcttx_bank_body<false>(L);
}

__global__ __launch_bounds__(64*kFtxWaves) void mcttx_span_kernel(const MctTxLaunch L)
{
    mcttx_bank_body<true>(L);
}


}   // namespace spg
