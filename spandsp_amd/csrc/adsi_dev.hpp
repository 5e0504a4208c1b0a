// adsi_dev.hpp -- device side of the caller-ID (ADSI) banks: N adsi_tx senders or N adsi_rx receivers in the four FSK
// standards (CLASS on Bell 202; CLIP, A-CLIP and J-CLIP on V.23 channel 1), messages in and messages out, one channel per
// lane, state in HBM, one launch per call.  Integer arithmetic throughout but for the alert tone, which is tone_gen()'s
// binary32 arithmetic as txgen_dev.hpp restates it; the results equal the reference's by construction.
//
// What is restated (paths relative to the reference tree):
//   adsi_tx_get_bit()          src/adsi.c:94-170       preamble, marks, start / 8 data / stop bits, postamble, end of data
//   adsi_tx()                  src/adsi.c:525-555      the alert tone first, the modem in the remainder of the row
//   adsi_tx_put_message()      src/adsi.c:637-646, 718-722   the busy check, start_tx() :409-433 and the bit sequencing;
//                                                      the packing itself runs on the host (adsi_host.c)
//   adsi_rx_put_bit()          src/adsi.c:192-328      the asynchronous framer, the sum check, J-CLIP's CRC and parity strip
//   crc_itu16_calc()           src/crc.c:161-169       bit by bit
//   tone_gen()                 src/tone_generate.c:128-229   for a descriptor of two tones, one on and one off section, no
//                                                      repeat: the sample arithmetic is that of tx_bank_kernel (txgen_dev.hpp)
// What is used as it stands: the modulator and its round loop (ftx_rounds(), fskmod_dev.hpp) with the message framer as
// its bit source, and the asynchronous demodulator over two waves (fsk_pair_body(), fsk_dev.hpp) with the message framer
// as its sink.
//
// State is structure-of-arrays int32 words.  A sender bank: [kAdsiTxWords + kFskTxWords][n_channels], the message layer's
// words, then the modulator's in the layout of fskmod_dev.hpp.  A receiver bank: [kAdsiRxWords + kFskScalars + 4*span]
// [n_channels], the framer's words, then the demodulator's in the layout of fsk_dev.hpp.  A channel's message bytes (256,
// either way) live in HBM beside the words, channel-major.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adsi_frame.hpp"
#include "fsk_dev.hpp"
#include "fskmod_dev.hpp"

namespace spg
{

enum
{
    ADT_STANDARD = 0,
    ADT_PREAMBLE_LEN = 1,
    ADT_PREAMBLE_ONES_LEN = 2,
    ADT_POSTAMBLE_ONES_LEN = 3,
    ADT_STOP_BITS = 4,
    ADT_BYTE_NO = 5,
    ADT_BIT_POS = 6,
    ADT_BIT_NO = 7,
    ADT_MSG_LEN = 8,
    ADT_TX_SIGNAL_ON = 9,
    ADT_TONE_SECTION = 10,      // alert_tone_gen: current_section (-1: finished), current_position, phase[0..1], duration[0..1]
    ADT_TONE_POS = 11,
    ADT_TONE_PHASE0 = 12,
    ADT_TONE_PHASE1 = 13,
    ADT_TONE_DUR0 = 14,
    ADT_TONE_DUR1 = 15,
    kAdsiTxWords = 16
};

enum
{
    ADR_STANDARD = 0,
    ADR_CONSECUTIVE_ONES = 1,
    ADR_BIT_POS = 2,
    ADR_IN_PROGRESS = 3,
    ADR_MSG_LEN = 4,
    ADR_FRAMING_ERRORS = 5,
    kAdsiRxWords = 8
};


struct AdsiTxLaunch
{
    int32_t *st;                // the bank's words
    const int16_t *quarter;     // [257] in HBM
    const float *sine;          // [2048] in HBM: the alert tone is a burst per call set-up, read where it lies
    const uint8_t *msgs;        // [n_ch][kAdsiMsg]
    int16_t *pcm;               // [n_ch][stride]
    int32_t *lens;              // [n_ch] or null
    long long stride;
    int n_ch;
    int samples;
    int vec;
    int32_t tone_rate[2];       // the alert tone descriptor: 2130 Hz + 2750 Hz at -13 dBm0 each
    float tone_gain[2];
};

// adsi_tx() x N: the FSK modulator (fskmod_dev.hpp) with the message framer as its bit source.  A channel's row is the alert
// tone's samples [0, T) -- for almost every call T is 0 -- and the modem's in [T, samples): the modulator walks and renders
// in row coordinates, from T on.  The byte pull happens in phase 1, at a bit boundary.
__global__ __launch_bounds__(64*kFtxWaves) void adsi_tx_kernel(const AdsiTxLaunch L)
{
    __shared__ __attribute__((aligned(16))) int32_t all_tone[kFtxWaves][kFtxCpw][8];    // T, sound from, sound to, phase0, phase1

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    int32_t (*r_tone)[8] = all_tone[wave];
    const int ch0 = (blockIdx.x*kFtxWaves + wave)*kFtxCpw;
    const int ch = ch0 + lane;
    const bool owner = (lane < kFtxCpw)  &&  (ch < L.n_ch);
    const FtxLds lds = ftx_lds(L.quarter);

    const size_t n = (size_t) L.n_ch;
    int32_t *sv = L.st + (owner  ?  ch  :  0);
    int32_t *st = sv + (size_t) kAdsiTxWords*n;
    const int samples = L.samples;
    AdsiTx t;
    t.preamble_len = t.preamble_ones_len = t.postamble_ones_len = t.stop_bits = 0;
    t.byte_no = t.bit_pos = t.bit_no = t.msg_len = t.signal_on = 0;
    t.msg = L.msgs + (size_t) (owner  ?  ch  :  0)*kAdsiMsg;
    int section = -1;
    int pos = 0;
    uint32_t tph0 = 0u;
    uint32_t tph1 = 0u;
    int dur0 = 0;
    int dur1 = 0;
    if (owner)
    {
        t.preamble_len = sv[ADT_PREAMBLE_LEN*n];
        t.preamble_ones_len = sv[ADT_PREAMBLE_ONES_LEN*n];
        t.postamble_ones_len = sv[ADT_POSTAMBLE_ONES_LEN*n];
        t.stop_bits = sv[ADT_STOP_BITS*n];
        t.byte_no = sv[ADT_BYTE_NO*n];
        t.bit_pos = sv[ADT_BIT_POS*n];
        t.bit_no = sv[ADT_BIT_NO*n];
        t.msg_len = sv[ADT_MSG_LEN*n];
        t.signal_on = sv[ADT_TX_SIGNAL_ON*n];
        section = sv[ADT_TONE_SECTION*n];
        pos = sv[ADT_TONE_POS*n];
        tph0 = (uint32_t) sv[ADT_TONE_PHASE0*n];
        tph1 = (uint32_t) sv[ADT_TONE_PHASE1*n];
        dur0 = sv[ADT_TONE_DUR0*n];
        dur1 = sv[ADT_TONE_DUR1*n];
    }
    FtxChan c;
    ftx_chan_load(c, st, n, owner);

    // tone_gen(&s->alert_tone_gen, amp, max_len), tone_generate.c:139-228, for sections 0 (the two tones) and 1 (silence)
    int tone_len = 0;
    int snd_from = 0;
    int snd_to = 0;
    const uint32_t snd_ph0 = tph0;
    const uint32_t snd_ph1 = tph1;
    if (owner  &&  section >= 0)
    {
        while (tone_len < samples)
        {
            const int dur = (section == 0)  ?  dur0  :  ((section == 1)  ?  dur1  :  0);
            int limit = tone_len + dur - pos;
            limit = (limit > samples)  ?  samples  :  limit;
            pos += limit - tone_len;
            if (section == 0)
            {
                snd_from = tone_len;
                snd_to = limit;
                tph0 += (uint32_t) (limit - tone_len)*(uint32_t) L.tone_rate[0];
                tph1 += (uint32_t) (limit - tone_len)*(uint32_t) L.tone_rate[1];
            }
            tone_len = limit;
            if (pos >= dur)
            {
                pos = 0;
                section++;
                const int nd = (section == 1)  ?  dur1  :  0;
                if (section > 3  ||  nd == 0)
                {
                    section = -1;       // no repeat
                    break;
                }
            }
        }
    }
    if (lane < kFtxCpw)
    {
        r_tone[lane][0] = owner  ?  tone_len  :  0;
        r_tone[lane][1] = snd_from;
        r_tone[lane][2] = snd_to;
        r_tone[lane][3] = (int32_t) snd_ph0;
        r_tone[lane][4] = (int32_t) snd_ph1;
    }

    // adsi.c:531-547: with tx_signal_on clear, or a row the tone fills, nothing is asked of the modulator; a modulator that
    // is shut down returns 0
    const bool asked = owner  &&  t.signal_on != 0  &&  tone_len < samples;
    const bool silent = !asked  ||  c.shutdown;
    int done = owner  ?  tone_len  :  samples;
    int len = samples;
    int zero_from = 0x7FFFFFFF;
    if (owner  &&  silent)
    {
        len = tone_len;
        zero_from = tone_len;
    }
    __syncthreads();

    // ---- the alert tone's samples: the wave's channels x chunks of 8, as in ftx_render() ----
    if (__any(tone_len > 0))
    {
        const int nchan = (L.n_ch - ch0 < kFtxCpw)  ?  (L.n_ch - ch0)  :  kFtxCpw;
        const int cpr = (samples + 7) >> 3;
        const int total = nchan*cpr;
        for (int idx = lane;  idx < total;  idx += 64)
        {
            const int c = idx/cpr;
            const int i0 = (idx - c*cpr)*8;
            const int4 hdr = *reinterpret_cast<const int4 *>(&r_tone[c][0]);        // T, sound from, sound to, phase0
            const int b = (i0 + 8 < hdr.x)  ?  (i0 + 8)  :  hdr.x;
            if (i0 >= b)
                continue;
            const uint32_t ph1 = (uint32_t) r_tone[c][4];
            int v[8];
#pragma unroll
            for (int j = 0;  j < 8;  j++)
            {
                const int i = i0 + j;
                v[j] = 0;
                if (i >= hdr.y  &&  i < hdr.z)
                {
                    // dds_modf() twice and the sum, tone_generate.c:190-204; lfastrintf() on x86-64 truncates
                    const uint32_t k = (uint32_t) (i - hdr.y);
                    const float t0 = __fmul_rn(L.sine[((uint32_t) hdr.w + k*(uint32_t) L.tone_rate[0]) >> 21], L.tone_gain[0]);
                    const float t1 = __fmul_rn(L.sine[(ph1 + k*(uint32_t) L.tone_rate[1]) >> 21], L.tone_gain[1]);
                    v[j] = (int) __fadd_rn(t0, t1);
                }
            }
            ftx_store8(L.pcm + (size_t) (ch0 + c)*L.stride + i0, v, 0, b - i0, L.vec != 0);
        }
    }

    ftx_rounds(lds, c, owner, silent, done, samples, len, zero_from, 0, L.pcm, L.stride, ch0, L.n_ch, samples, L.vec != 0,
               [&]() __attribute__((always_inline)) { return adsi_next_bit(t); });

    if (owner)
    {
        sv[ADT_TONE_SECTION*n] = section;
        sv[ADT_TONE_POS*n] = pos;
        sv[ADT_TONE_PHASE0*n] = (int32_t) tph0;
        sv[ADT_TONE_PHASE1*n] = (int32_t) tph1;
        if (asked)
        {
            if (!c.was_shutdown)
            {
                ftx_chan_store(c, st, n);
                sv[ADT_BYTE_NO*n] = t.byte_no;
                sv[ADT_BIT_POS*n] = t.bit_pos;
                sv[ADT_BIT_NO*n] = t.bit_no;
                sv[ADT_MSG_LEN*n] = t.msg_len;
            }
            // adsi.c:542-543: a call that gets nothing out of the modulator turns the signal off
            sv[ADT_TX_SIGNAL_ON*n] = (len - tone_len <= 0)  ?  0  :  t.signal_on;
        }
        ftx_event_store(c, st, n);
        if (L.lens)
            L.lens[ch] = len;
    }
}

// adsi_tx_put_message() on channels [lo, hi), after the packing: packed[(c - lo)*kAdsiMsg ...], plens[c - lo] bytes of it,
// or -1 for a message that is too long.  results[c - lo]: 0 a message is in progress (nothing changes), -1 too long, 1 taken.
// start_tx() comes ahead of the length check, as in the reference: a sender whose signal is off has its modulator
// restarted (fsk_tx_init(): the spec's words do not change within a standard) even by a message that is then refused.
__global__ void adsi_put_kernel(int32_t *st, uint8_t *msgs, int n_ch, int lo, int hi, const uint8_t *packed, const int32_t *plens,
                                int32_t *results)
{
    const int ch = lo + blockIdx.x*blockDim.x + threadIdx.x;
    if (ch >= hi)
        return;
    const size_t n = (size_t) n_ch;
    int32_t *sv = st + ch;
    int32_t *ft = sv + (size_t) kAdsiTxWords*n;
    if (sv[ADT_MSG_LEN*n] > 0)
    {
        results[ch - lo] = 0;
        return;
    }
    if (sv[ADT_TX_SIGNAL_ON*n] == 0)
    {
        // fsk_tx_restart(), fsk.c:221-235
        ft[FT_PHASE*n] = 0;
        ft[FT_BAUD_FRAC*n] = 0;
        ft[FT_CUR_RATE*n] = ft[FT_RATE1*n];
        ft[FT_SHUTDOWN*n] = 0;
        sv[ADT_TX_SIGNAL_ON*n] = 1;
    }
    const int len = plens[ch - lo];
    if (len < 0  ||  len > kAdsiMsg)
    {
        results[ch - lo] = -1;
        return;
    }
    const uint8_t *src = packed + (size_t) (ch - lo)*kAdsiMsg;
    uint8_t *mine = msgs + (size_t) ch*kAdsiMsg;
    for (int i = 0;  i < len;  i++)
        mine[i] = src[i];
    sv[ADT_MSG_LEN*n] = len;
    sv[ADT_BYTE_NO*n] = 0;
    sv[ADT_BIT_POS*n] = 0;
    sv[ADT_BIT_NO*n] = 0;
    results[ch - lo] = 1;
}

struct AdsiRxLaunch
{
    FskLaunch f;                // st = the demodulator's words inside the bank's; events / ev_count are not used
    int32_t *sv;                // the bank's words (the framer's come first)
    uint8_t *msgs;              // [n_ch][kAdsiMsg]: the message being collected
    uint8_t *rec_bytes;         // [n_ch][cap][kAdsiMsg]: the call's record
    int32_t *rec_lens;          // [n_ch][cap]
    int32_t *counts;            // [n_ch]
    int cap;
};


// The sink of fsk_pair_body() (fsk_dev.hpp): the framer's words in and out around adsi_put_bit()
struct AdsiRxSink
{
    const AdsiRxLaunch &V;
    int32_t *sv;
    AdsiRx v;

    __device__ __forceinline__ void open(bool live, int ch, size_t n, int mylen)
    {
        sv = V.sv + ch;
        v.standard = sv[ADR_STANDARD*n];
        v.ones = sv[ADR_CONSECUTIVE_ONES*n];
        v.bit_pos = sv[ADR_BIT_POS*n];
        v.in_progress = sv[ADR_IN_PROGRESS*n];
        v.msg_len = sv[ADR_MSG_LEN*n];
        v.framing_errors = sv[ADR_FRAMING_ERRORS*n];
        v.count = 0;
        v.msg = V.msgs + (size_t) ch*kAdsiMsg;
        v.rec_bytes = V.rec_bytes + (size_t) ch*V.cap*kAdsiMsg;
        v.rec_lens = V.rec_lens + (size_t) ch*V.cap;
        v.cap = live  ?  V.cap  :  0;
    }

    __device__ __forceinline__ void put(FskBitSide &, int bit)
    {
        adsi_put_bit(v, bit);
    }

    __device__ __forceinline__ void close(FskBitSide &, int ch, size_t n)
    {
        sv[ADR_CONSECUTIVE_ONES*n] = v.ones;
        sv[ADR_BIT_POS*n] = v.bit_pos;
        sv[ADR_IN_PROGRESS*n] = v.in_progress;
        sv[ADR_MSG_LEN*n] = v.msg_len;
        sv[ADR_FRAMING_ERRORS*n] = v.framing_errors;
        V.counts[ch] = v.count;
    }
};

// adsi_rx() x N: the two-wave receiver (fsk_pair_body(), fsk_dev.hpp), asynchronous, with the message framer behind the
// bit clock.
__global__ __launch_bounds__(128) void adsi_rx_kernel(const AdsiRxLaunch V)
{
    AdsiRxSink sink = {V};
    fsk_pair_body<FSK_FRAMING_NEVER>(V.f, sink);
}

}   // namespace spg
