// gsm0610_dev.hpp -- GSM 06.10 full-rate codec banks (ETSI GSM 06.10, the shape of spandsp's gsm0610_*.c): one lane per channel,
// every channel with a packing of its own (76 unpacked bytes a frame, 33 bytes in the VoIP layout, or two frames in the 65
// bytes of WAV49).  The first block codec of the banks: the item is a 160-sample frame, not a sample.
//
// The per-frame functions are __host__ __device__ templates over the channel's working memory, and the file compiles for the
// host (tests/c_callers/gsm0610_host.cpp runs them one lane at a time under ASan and UBSan); the two kernels at the end are
// HIP only.
//
// Working memory.  A channel works in 280 int16_t, the reference's dp0[]: [0..119] is the history of the reconstructed
// short-term residual, [120..279] the frame.  The encoder puts the pre-processed samples there, the short-term analysis
// filter turns them into d[] in place, and each 40-sample subframe is overwritten by its reconstructed residual d'[] once
// its parameters are found, so the lag search of the next subframe finds its 120 samples of history right below it, as it
// does in the reference.  The long-term residual e[], the estimate d''[] and the weighted x[] of a subframe are 40 values
// with compile-time indices: registers.  The decoder writes the reconstructed residual of the four subframes to [120..279]
// (the reference's wt[] and its drp[] are the same samples), filters from there, and stages the frame's code bytes in
// [240..279] until the fourth subframe's parameters are read.  After a frame [160..279] move to [0..119].
// In the kernels the memory is LDS, lane L's sample i in half (i & 1) of dword (i >> 1)*64 + L: a lane owns a column of
// banks, and an index that differs from lane to lane (the lag) meets no bank conflict.  35 840 bytes a wave.
//
// int16_t arithmetic.  Every value is an int32_t and each truncation is an explicit gsm_s16(); a right shift of a negative
// value is arithmetic; a left shift of a value that may be negative is a multiplication, and sums that the reference lets
// wrap are unsigned here, so the host build has nothing for UBSan to report.
//
// Bits.  The three packings carry the same 76 parameters in the same order: LARc[8] (6,6,5,5,4,4,3,3 bits), then per subframe
// Nc (7), bc (2), Mc (2), xmaxc (6) and xMc[13] (3 each), 260 bits.  VoIP: the nibble 0xD, then the parameters, first bit in
// the top bit of the first byte.  WAV49: the parameters of two frames, first bit in the bottom bit of the first byte.
// Unpacked: a byte a parameter.  An encoder's call is one bit stream (a frame is whole bytes, and a WAV49 pair is one run of
// 520 bits), which leaves as 32-bit words; a decoder reads a parameter from the two bytes that hold it.  Decoders mask every
// parameter to its width: wider unpacked bytes index past the reference's tables.
//
// State words of a channel, st[word*n + ch], in the order of the reference's fields: packing, dp0[0..119], z1, L_z2, mp, u[8],
// LARpp[2][8], j, nrp, v[9], msr (160).  dp0[120..279] and e[] are workspace there as here and are left out.

#pragma once

#include <stddef.h>
#include <stdint.h>

#include "codec_rows.hpp"

#ifdef __HIPCC__
#define GSM_HD __host__ __device__ __forceinline__
#define GSM_UNROLL _Pragma("unroll")
#define GSM_ROLLED _Pragma("nounroll")
#else
#define GSM_HD static inline
#define GSM_UNROLL
#define GSM_ROLLED
#endif

namespace spg
{

enum
{
    GW_PACKING = 0,
    GW_DP0,                         // .. GW_DP0 + 119
    GW_Z1 = GW_DP0 + 120, GW_LZ2, GW_MP,
    GW_U0,                          // .. + 7
    GW_LARPP = GW_U0 + 8,           // [2][8]
    GW_J = GW_LARPP + 16, GW_NRP,
    GW_V0,                          // .. + 8
    GW_MSR = GW_V0 + 9,
    kGsmWords
};

enum { kGsmNone = 0, kGsmWav49 = 1, kGsmVoip = 2 };             // GSM0610_PACKING_NONE, _WAV49, _VOIP
enum { kGsmFrame = 160, kGsmHist = 120, kGsmMem = 280, kGsmStage = 240, kGsmStageBytes = 80 };

// the widths of a frame's parameters in stream order
static constexpr int32_t kGsmLarBits[8] = {6, 6, 5, 5, 4, 4, 3, 3};
// 4.2.7 / 4.2.8 (table 4.1 and 4.2): A, B, MAC, MIC and INVA of the eight log area ratios
static constexpr int32_t kGsmA[8] = {20480, 20480, 20480, 20480, 13964, 15360, 8534, 9036};
static constexpr int32_t kGsmB[8] = {0, 0, 2048, -2560, 94, -1792, -341, -1144};
static constexpr int32_t kGsmMac[8] = {31, 31, 15, 15, 7, 7, 3, 3};
static constexpr int32_t kGsmMic[8] = {-32, -32, -16, -16, -8, -8, -4, -4};
static constexpr int32_t kGsmInvA[8] = {13107, 13107, 13107, 13107, 19223, 17476, 31454, 29708};
// table 4.4: the weighting filter
static constexpr int32_t kGsmH[11] = {-134, -374, 0, 2054, 5741, 8192, 5741, 2054, 0, -374, -134};

struct Gsm
{
    int32_t packing;
    int32_t z1, L_z2, mp;
    int32_t u[8];
    int32_t larpp[2][8];
    int32_t j, nrp;
    int32_t v[9];
    int32_t msr;
};

static inline bool gsm0610_packing_ok(int packing)
{
    return packing == kGsmNone  ||  packing == kGsmWav49  ||  packing == kGsmVoip;
}

// gsm0610_init(), gsm0610_encode.c:313-326.  false: a packing this bank refuses
static inline bool gsm0610_init_words(int32_t w[kGsmWords], int packing)
{
    if (!gsm0610_packing_ok(packing))
        return false;
    for (int i = 0;  i < kGsmWords;  i++)
        w[i] = 0;
    w[GW_PACKING] = packing;
    w[GW_NRP] = 40;
    return true;
}

// what a call takes and makes, in whole units: samples and bytes of an encoder's unit, bytes and samples of a decoder's
GSM_HD int gsm0610_unit_samples(int packing) { return (packing == kGsmWav49)  ?  320  :  160; }
GSM_HD int gsm0610_unit_bytes(int packing) { return (packing == kGsmWav49)  ?  65  :  ((packing == kGsmVoip)  ?  33  :  76); }
// (no call is longer than 2^24 items: the products stay inside 32 bits)
GSM_HD int gsm0610_encode_capacity(int packing, int samples)
{
    return (samples/gsm0610_unit_samples(packing))*gsm0610_unit_bytes(packing);
}
GSM_HD int gsm0610_decode_capacity(int packing, int bytes)
{
    return (bytes/gsm0610_unit_bytes(packing))*gsm0610_unit_samples(packing);
}

// ---- 16- and 32-bit saturating arithmetic ---------------------------------------------------------------------------------

GSM_HD int32_t gsm_s16(int32_t x)
{
    return (int32_t) (int16_t) (uint16_t) (uint32_t) x;
}

GSM_HD int32_t gsm_sat16(int32_t x)
{
    return (x > 32767)  ?  32767  :  ((x < -32768)  ?  -32768  :  x);
}

GSM_HD int32_t gsm_add(int32_t a, int32_t b) { return gsm_sat16(a + b); }
GSM_HD int32_t gsm_sub(int32_t a, int32_t b) { return gsm_sat16(a - b); }

GSM_HD int32_t gsm_abs(int32_t a)
{
    return (a == -32768)  ?  32767  :  ((a < 0)  ?  -a  :  a);
}

GSM_HD int32_t gsm_add32(int32_t a, int32_t b)
{
    const int64_t z = (int64_t) a + b;
    return (z > 2147483647LL)  ?  2147483647  :  ((z < -2147483648LL)  ?  (int32_t) -2147483648LL  :  (int32_t) z);
}

// gsm_mult_r(): the rounded product of two Q15 values
GSM_HD int32_t gsm_mult_r(int32_t a, int32_t b)
{
    return (a == -32768  &&  b == -32768)  ?  32767  :  gsm_s16((a*b + 16384) >> 15);
}

// sat_mul16(): the truncated product
GSM_HD int32_t gsm_mult(int32_t a, int32_t b)
{
    const int32_t z = a*b;
    return (z == 0x40000000)  ?  32767  :  gsm_s16(z >> 15);
}

GSM_HD int32_t gsm_clz(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __clz((int) x);
#else
    return x  ?  __builtin_clz(x)  :  32;
#endif
}

GSM_HD uint32_t gsm_brev(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(x);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    return (x >> 16) | (x << 16);
#endif
}

GSM_HD uint32_t gsm_bswap(uint32_t x)
{
    return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
}

// gsm0610_norm() of a positive value: the left shifts that bring it to 0x40000000 .. 0x7FFFFFFF
GSM_HD int32_t gsm_norm(int32_t x)
{
    return gsm_clz((uint32_t) x) - 1;
}

GSM_HD int32_t gsm_shl32(int32_t x, int32_t n)
{
    return (int32_t) ((uint32_t) x << n);
}

GSM_HD int32_t gsm_pick4(int32_t i, int32_t a, int32_t b, int32_t c, int32_t d)
{
    const int32_t lo = (i & 1)  ?  b  :  a;
    const int32_t hi = (i & 1)  ?  d  :  c;
    return (i & 2)  ?  hi  :  lo;
}

// table 4.3b, the levels of the LTP gain
GSM_HD int32_t gsm_qlb(int32_t bc)
{
    return gsm_pick4(bc, 3277, 11469, 21299, 32767);
}

// ---- state ----------------------------------------------------------------------------------------------------------------

// The words but the history: st[word*n].  The history goes to the working memory and back (gsm_load_hist, gsm_store_hist).
GSM_HD void gsm_load(Gsm &s, const int32_t *st, size_t n)
{
    s.packing = st[GW_PACKING*n];
    s.z1 = st[GW_Z1*n];
    s.L_z2 = st[GW_LZ2*n];
    s.mp = st[GW_MP*n];
GSM_UNROLL
    for (int i = 0;  i < 8;  i++)
    {
        s.u[i] = st[(GW_U0 + i)*n];
        s.larpp[0][i] = st[(GW_LARPP + i)*n];
        s.larpp[1][i] = st[(GW_LARPP + 8 + i)*n];
    }
    s.j = st[GW_J*n];
    s.nrp = st[GW_NRP*n];
GSM_UNROLL
    for (int i = 0;  i < 9;  i++)
        s.v[i] = st[(GW_V0 + i)*n];
    s.msr = st[GW_MSR*n];
}

GSM_HD void gsm_store(const Gsm &s, int32_t *st, size_t n)
{
    st[GW_PACKING*n] = s.packing;
    st[GW_Z1*n] = s.z1;
    st[GW_LZ2*n] = s.L_z2;
    st[GW_MP*n] = s.mp;
GSM_UNROLL
    for (int i = 0;  i < 8;  i++)
    {
        st[(GW_U0 + i)*n] = s.u[i];
        st[(GW_LARPP + i)*n] = s.larpp[0][i];
        st[(GW_LARPP + 8 + i)*n] = s.larpp[1][i];
    }
    st[GW_J*n] = s.j;
    st[GW_NRP*n] = s.nrp;
GSM_UNROLL
    for (int i = 0;  i < 9;  i++)
        st[(GW_V0 + i)*n] = s.v[i];
    st[GW_MSR*n] = s.msr;
}

template <class M>
GSM_HD void gsm_load_hist(M &m, const int32_t *st, size_t n)
{
GSM_ROLLED
    for (int i = 0;  i < kGsmHist;  i++)
        m.st(i, st[(GW_DP0 + i)*n]);
}

template <class M>
GSM_HD void gsm_store_hist(const M &m, int32_t *st, size_t n)
{
GSM_ROLLED
    for (int i = 0;  i < kGsmHist;  i++)
        st[(GW_DP0 + i)*n] = m.ld(i);
}

// the end of a frame: the last 120 samples of the reconstructed residual are the next frame's history
template <class M>
GSM_HD void gsm_shift_hist(M &m)
{
GSM_ROLLED
    for (int i = 0;  i < kGsmHist;  i++)
        m.st(i, m.ld(i + kGsmFrame));
}

// ---- bits out -------------------------------------------------------------------------------------------------------------

// An encoder's bit stream.  The accumulator takes every field at its bottom; a channel whose first bit is a byte's bottom bit
// (WAV49, and the byte-a-parameter layout) brings its fields bit-reversed and reverses each word as it leaves.
struct GsmBitsOut
{
    uint64_t acc;
    int32_t nbits;              // < 32 between pushes
    int32_t lsb_first;
    int32_t bytewise;           // kGsmNone: every parameter is 8 bits of the stream
    int32_t voip;
};

GSM_HD void gsm_bits_begin(GsmBitsOut &b, int packing)
{
    b.acc = 0;
    b.nbits = 0;
    b.lsb_first = (packing != kGsmVoip);
    b.bytewise = (packing == kGsmNone);
    b.voip = (packing == kGsmVoip);
}

// `bits` (0 .. 8) of v; SINK::word() takes the stream 32 bits at a time, as the four bytes in memory order
template <class SINK>
GSM_HD void gsm_bits_raw(GsmBitsOut &b, SINK &sink, uint32_t v, int32_t bits)
{
    const uint32_t x = b.lsb_first  ?  (bits  ?  (gsm_brev(v) >> (32 - bits))  :  0u)  :  v;
    b.acc = (b.acc << bits) | x;
    b.nbits += bits;
    if (b.nbits >= 32)
    {
        const uint32_t be = (uint32_t) (b.acc >> (b.nbits - 32));
        b.nbits -= 32;
        sink.word(b.lsb_first  ?  gsm_brev(be)  :  gsm_bswap(be));
    }
}

// a parameter of `width` bits
template <class SINK>
GSM_HD void gsm_bits_put(GsmBitsOut &b, SINK &sink, int32_t v, int32_t width)
{
    gsm_bits_raw(b, sink, (uint32_t) v & ((1u << width) - 1u), b.bytewise  ?  8  :  width);
}

// the end of a call: the bytes that wait leave in a last word, zeros behind them
template <class SINK>
GSM_HD void gsm_bits_end(GsmBitsOut &b, SINK &sink)
{
    if (b.nbits > 0)
    {
        const uint32_t be = (uint32_t) (b.acc << (32 - b.nbits));
        b.nbits = 0;
        sink.word(b.lsb_first  ?  gsm_brev(be)  :  gsm_bswap(be));
    }
}

// ---- bits in --------------------------------------------------------------------------------------------------------------

// A decoder's frame, staged in the working memory: M::byte(n) is byte n of the stage.  `at` is the next bit.
struct GsmBitsIn
{
    int32_t at;
    int32_t lsb_first;
    int32_t bytewise;
};

GSM_HD void gsm_bits_from(GsmBitsIn &b, int packing, int32_t first_bit)
{
    b.at = first_bit + ((packing == kGsmVoip)  ?  4  :  0);         // past the 0xD nibble, whatever it holds
    b.lsb_first = (packing != kGsmVoip);
    b.bytewise = (packing == kGsmNone);
}

// the next parameter, masked to its width
template <class M>
GSM_HD int32_t gsm_bits_get(GsmBitsIn &b, const M &m, int32_t width)
{
    const int32_t n = b.at >> 3;
    const int32_t sh = b.at & 7;
    const uint32_t b0 = m.byte(n);
    const uint32_t b1 = m.byte(n + 1);
    const uint32_t down = ((b1 << 8) | b0) >> sh;
    const uint32_t up = ((b0 << 8) | b1) >> (16 - sh - width);
    b.at += b.bytewise  ?  8  :  width;
    return (int32_t) ((b.lsb_first  ?  down  :  up) & ((1u << width) - 1u));
}

// ---- the encoder ----------------------------------------------------------------------------------------------------------

// 4.2.1 - 4.2.3: downscaling, offset compensation and pre-emphasis of one sample (gsm0610_preprocess.c:71-148, the branch a
// GNU compiler takes: a 64-bit product)
GSM_HD int32_t gsm_preprocess(Gsm &s, int32_t amp)
{
    const int32_t so = (gsm_s16(amp) >> 1) & ~3;
    const int32_t s1 = gsm_s16(so - s.z1);
    s.z1 = so;
    const int32_t L_s2 = s1*32768;
    const int32_t z2 = (int32_t) (((int64_t) s.L_z2*32735 + 0x4000) >> 15);
    s.L_z2 = gsm_add32(z2, L_s2);
    const int32_t L_temp = gsm_add32(s.L_z2, 16384);
    const int32_t msp = gsm_mult_r(s.mp, -28180);
    s.mp = gsm_s16(L_temp >> 15);
    return gsm_add(s.mp, msp);
}

// gsm_div(): num/denom in Q15, 0 <= num <= denom
GSM_HD int32_t gsm_div(int32_t num, int32_t denom)
{
    int32_t div = 0;
    int32_t n = num;
GSM_UNROLL
    for (int k = 0;  k < 15;  k++)
    {
        div <<= 1;
        n <<= 1;
        const bool ge = (n >= denom);
        n -= ge  ?  denom  :  0;
        div += ge  ?  1  :  0;
    }
    return (num == 0)  ?  0  :  gsm_s16(div);
}

// 4.2.4 - 4.2.7: the frame at m[120..279] gives LARc[8] (gsm0610_lpc.c).  The scaled samples are not kept: a sample is
// scaled as it is read and goes back the way the reference's rescaling leaves it.
template <class M>
GSM_HD void gsm_lpc_analysis(M &m, int32_t LARc[8])
{
    // 4.2.4 autocorrelation, with its dynamic scaling
    int32_t smax = 0;
GSM_ROLLED
    for (int k = 0;  k < kGsmFrame;  k++)
    {
        const int32_t t = gsm_abs(m.ld(kGsmHist + k));
        smax = (t > smax)  ?  t  :  smax;
    }
    const int32_t scalauto = (smax == 0)  ?  0  :  (4 - gsm_norm(smax*65536));
    const int32_t factor = (scalauto > 0)  ?  (16384 >> (scalauto - 1))  :  0;
    uint32_t acf[9];
    int32_t w[9];
GSM_UNROLL
    for (int i = 0;  i < 9;  i++)
    {
        acf[i] = 0;
        w[i] = 0;
    }
GSM_ROLLED
    for (int k = 0;  k < kGsmFrame;  k++)
    {
        int32_t sl = m.ld(kGsmHist + k);
        if (scalauto > 0)
        {
            sl = gsm_mult_r(sl, factor);
            m.st(kGsmHist + k, gsm_s16(gsm_shl32(sl, scalauto)));
        }
GSM_UNROLL
        for (int i = 8;  i > 0;  i--)
            w[i] = w[i - 1];
        w[0] = sl;
GSM_UNROLL
        for (int i = 0;  i < 9;  i++)
            acf[i] += (uint32_t) (sl*w[i]);
    }
    int32_t L_ACF[9];
GSM_UNROLL
    for (int i = 0;  i < 9;  i++)
        L_ACF[i] = (int32_t) (acf[i] << 1);

    // 4.2.5 the Schur recursion.  A lane that is through (a power of zero, or an unstable stage) carries zeros on.
    int32_t r[8];
    bool done = (L_ACF[0] == 0);
    const int32_t sh = done  ?  0  :  gsm_norm(L_ACF[0]);
    int32_t P[9], K[9];
GSM_UNROLL
    for (int i = 0;  i < 9;  i++)
    {
        P[i] = gsm_s16(gsm_shl32(L_ACF[i], sh) >> 16);
        K[i] = P[i];
    }
GSM_UNROLL
    for (int n = 1;  n <= 8;  n++)
    {
        const int32_t t = gsm_abs(P[1]);
        done = done  ||  (P[0] < t);
        // (gsm_div() wants num <= denom, which holds where the lane is not through)
        int32_t rn = gsm_div(done  ?  0  :  t, done  ?  1  :  P[0]);
        rn = (P[1] > 0)  ?  -rn  :  rn;
        rn = done  ?  0  :  rn;
        r[n - 1] = rn;
        if (n < 8)
        {
            P[0] = gsm_add(P[0], gsm_mult_r(P[1], rn));
GSM_UNROLL
            for (int mm = 1;  mm <= 8 - n;  mm++)
            {
                const int32_t pm1 = P[mm + 1];
                P[mm] = gsm_add(pm1, gsm_mult_r(K[mm], rn));
                K[mm] = gsm_add(K[mm], gsm_mult_r(pm1, rn));
            }
        }
    }
    // 4.2.6 to log area ratios, 4.2.7 their quantization and coding
GSM_UNROLL
    for (int i = 0;  i < 8;  i++)
    {
        int32_t t = gsm_abs(r[i]);
        t = (t < 22118)  ?  (t >> 1)  :  ((t < 31130)  ?  (t - 11059)  :  gsm_s16((t - 26112)*4));
        const int32_t lar = (r[i] < 0)  ?  -t  :  t;
        int32_t q = gsm_mult(kGsmA[i], lar);
        q = gsm_add(q, kGsmB[i] + 256) >> 9;
        LARc[i] = (q > kGsmMac[i])  ?  (kGsmMac[i] - kGsmMic[i])  :  ((q < kGsmMic[i])  ?  0  :  (q - kGsmMic[i]));
    }
}

// 4.2.8: the coded log area ratios back to LARpp, into the set of this frame; the other set is the last frame's.  j flips,
// as gsm0610_short_term.c:307-308 has it.
GSM_HD void gsm_decode_lar(Gsm &s, const int32_t LARc[8], int32_t cur[8], int32_t prev[8])
{
    const bool j = (s.j != 0);
GSM_UNROLL
    for (int i = 0;  i < 8;  i++)
    {
        int32_t t = gsm_s16(gsm_add(LARc[i], kGsmMic[i])*1024);
        t = gsm_sub(t, kGsmB[i]*2);
        t = gsm_mult_r(kGsmInvA[i], t);
        cur[i] = gsm_add(t, t);
        prev[i] = j  ?  s.larpp[0][i]  :  s.larpp[1][i];
        s.larpp[0][i] = j  ?  s.larpp[0][i]  :  cur[i];
        s.larpp[1][i] = j  ?  cur[i]  :  s.larpp[1][i];
    }
    s.j = j  ?  0  :  1;
}

// 4.2.9.1 and 4.2.9.2: the interpolated ratios of one of the four ranges of a frame, as reflection coefficients
GSM_HD void gsm_range_rp(int range, const int32_t cur[8], const int32_t prev[8], int32_t rp[8])
{
GSM_UNROLL
    for (int i = 0;  i < 8;  i++)
    {
        int32_t t;
        if (range == 0)
            t = gsm_add(gsm_add(prev[i] >> 2, cur[i] >> 2), prev[i] >> 1);
        else if (range == 1)
            t = gsm_add(prev[i] >> 1, cur[i] >> 1);
        else if (range == 2)
            t = gsm_add(gsm_add(prev[i] >> 2, cur[i] >> 2), cur[i] >> 1);
        else
            t = cur[i];
        int32_t a = gsm_abs(t);
        a = (a < 11059)  ?  (a << 1)  :  ((a < 20070)  ?  (a + 11059)  :  gsm_add(a >> 2, 26112));
        rp[i] = (t < 0)  ?  -a  :  a;
    }
}

// where the four ranges start: samples 0-12, 13-26, 27-39, 40-159
GSM_HD int gsm_range_start(int range)
{
    return (range == 0)  ?  0  :  ((range == 1)  ?  13  :  ((range == 2)  ?  27  :  ((range == 3)  ?  40  :  kGsmFrame)));
}

// 4.2.10: the short-term analysis lattice over the frame, in place
template <class M>
GSM_HD void gsm_short_term_analysis(Gsm &s, M &m, const int32_t LARc[8])
{
    int32_t cur[8], prev[8], rp[8];
    gsm_decode_lar(s, LARc, cur, prev);
GSM_UNROLL
    for (int range = 0;  range < 4;  range++)
    {
        gsm_range_rp(range, cur, prev, rp);
GSM_ROLLED
        for (int k = gsm_range_start(range);  k < gsm_range_start(range + 1);  k++)
        {
            int32_t di = m.ld(kGsmHist + k);
            int32_t u_out = di;
GSM_UNROLL
            for (int i = 0;  i < 8;  i++)
            {
                const int32_t ui = s.u[i];
                s.u[i] = u_out;
                u_out = gsm_sat16(ui + ((rp[i]*di + 0x4000) >> 15));
                di = gsm_sat16(di + ((rp[i]*ui + 0x4000) >> 15));
            }
            m.st(kGsmHist + k, di);
        }
    }
}

// 4.2.15, the part both directions share: exponent and mantissa of a coded block maximum
GSM_HD void gsm_exp_mant(int32_t xmaxc, int32_t &exp_out, int32_t &mant_out)
{
    int32_t exp = (xmaxc > 15)  ?  ((xmaxc >> 3) - 1)  :  0;
    int32_t mant = xmaxc - exp*8;
    const bool zero = (mant == 0);
    // (a mantissa of 1 .. 7 takes up to three steps to reach 8 .. 15)
GSM_UNROLL
    for (int i = 0;  i < 3;  i++)
    {
        const bool more = (mant <= 7);
        mant = more  ?  ((mant << 1) | 1)  :  mant;
        exp -= more  ?  1  :  0;
    }
    exp_out = zero  ?  -4  :  exp;
    mant_out = zero  ?  7  :  (mant - 8);
}

// 4.2.16: the 13 coded samples back to xMp (table 4.6 is 18431 + 2048*mant)
GSM_HD void gsm_apcm_inverse(const int32_t xMc[13], int32_t mant, int32_t exp, int32_t xMp[13])
{
    const int32_t fac = 18431 + 2048*mant;
    const int32_t shift = gsm_sub(6, exp);                      // 0 .. 10
    const int32_t half = (shift >= 1)  ?  (1 << (shift - 1))  :  0;
GSM_UNROLL
    for (int i = 0;  i < 13;  i++)
    {
        int32_t t = (xMc[i]*2 - 7)*4096;
        t = gsm_mult_r(fac, t);
        t = gsm_add(t, half);
        xMp[i] = t >> shift;
    }
}

// 4.2.17: sample k of the grid Mc holds xMp[(k - Mc)/3]; the others are zero
GSM_HD int32_t gsm_grid_sample(int k, int32_t Mc, const int32_t xMp[13])
{
    int32_t v = 0;
    if (k/3 < 13)
        v = (Mc == k % 3)  ?  xMp[k/3]  :  v;
    if (k % 3 == 0  &&  k >= 3)
        v = (Mc == 3)  ?  xMp[k/3 - 1]  :  v;
    return v;
}

// One subframe of the encoder, 4.2.11 - 4.2.17 (gsm0610_long_term.c, gsm0610_rpe.c): d[] is m[base .. base + 39] with the
// reconstructed residual below it; the 17 parameters go to the bit stream, and d'[] takes d[]'s place.
template <class M, class SINK>
GSM_HD void gsm_encode_subframe(M &m, int base, GsmBitsOut &bits, SINK &sink)
{
    int32_t d[40];
    // 4.2.11: the scaling of d[]
    int32_t dmax = 0;
GSM_UNROLL
    for (int k = 0;  k < 40;  k++)
    {
        d[k] = m.ld(base + k);
        const int32_t t = gsm_abs(d[k]);
        dmax = (t > dmax)  ?  t  :  dmax;
    }
    const int32_t nrm = (dmax == 0)  ?  0  :  gsm_norm(dmax*65536);
    const int32_t scale = (nrm > 6)  ?  0  :  (6 - nrm);
    int32_t wt[40];
GSM_UNROLL
    for (int k = 0;  k < 40;  k++)
        wt[k] = d[k] >> scale;
    // the cross-correlation at lags 40 .. 120, three lags a pass over the window; the first strict maximum wins.  The index
    // is the same in every lane here.  32-bit sums as the reference's: no product passes 2^24 and no sum 2^30.
    int32_t best = 0;
    int32_t Nc = 40;
GSM_ROLLED
    for (int lag = 40;  lag <= 120;  lag += 3)
    {
        uint32_t a0 = 0, a1 = 0, a2 = 0;
        int32_t p2 = m.ld(base - lag - 2);
        int32_t p1 = m.ld(base - lag - 1);
GSM_UNROLL
        for (int k = 0;  k < 40;  k++)
        {
            const int32_t p0 = m.ld(base - lag + k);
            a0 += (uint32_t) (wt[k]*p0);
            a1 += (uint32_t) (wt[k]*p1);
            a2 += (uint32_t) (wt[k]*p2);
            p2 = p1;
            p1 = p0;
        }
        const bool g0 = ((int32_t) a0 > best);
        best = g0  ?  (int32_t) a0  :  best;
        Nc = g0  ?  lag  :  Nc;
        const bool g1 = ((int32_t) a1 > best);
        best = g1  ?  (int32_t) a1  :  best;
        Nc = g1  ?  (lag + 1)  :  Nc;
        const bool g2 = ((int32_t) a2 > best);
        best = g2  ?  (int32_t) a2  :  best;
        Nc = g2  ?  (lag + 2)  :  Nc;
    }
    const int32_t L_max = gsm_shl32(best, 1) >> (6 - scale);
    // the power of the residual at the lag: an index of the lane's own
    uint32_t power = 0;
    int32_t hist[40];
GSM_UNROLL
    for (int k = 0;  k < 40;  k++)
    {
        hist[k] = m.ld(base + k - Nc);
        const int32_t t = hist[k] >> 3;
        power += (uint32_t) (t*t);
    }
    const int32_t L_power = (int32_t) (power << 1);
    // the gain against table 4.3a
    int32_t bc;
    {
        const int32_t ns = (L_power > 0)  ?  gsm_norm(L_power)  :  0;
        const int32_t R = gsm_s16(gsm_shl32(L_max, ns) >> 16);
        const int32_t S = gsm_s16(gsm_shl32(L_power, ns) >> 16);
        bc = (R <= gsm_mult(S, 6554))  ?  0  :  ((R <= gsm_mult(S, 16384))  ?  1  :  ((R <= gsm_mult(S, 26214))  ?  2  :  3));
        bc = (L_max >= L_power)  ?  3  :  bc;
        bc = (L_max <= 0)  ?  0  :  bc;
    }
    // 4.2.12: the estimate d''[] and the long-term residual e[]
    const int32_t gain = gsm_qlb(bc);
    int32_t dpp[40], e[40];
GSM_UNROLL
    for (int k = 0;  k < 40;  k++)
    {
        dpp[k] = gsm_mult_r(gain, hist[k]);
        e[k] = gsm_sub(d[k], dpp[k]);
    }
    // 4.2.13: the weighting filter, five zeros either side of e[]
    int32_t x[40];
GSM_UNROLL
    for (int k = 0;  k < 40;  k++)
    {
        int32_t acc = 4096;
GSM_UNROLL
        for (int i = 0;  i < 11;  i++)
        {
            if (kGsmH[i] != 0  &&  k + i - 5 >= 0  &&  k + i - 5 < 40)
                acc += e[k + i - 5]*kGsmH[i];
        }
        x[k] = gsm_sat16(acc >> 13);
    }
    // 4.2.14: the grid with the most energy; a later grid has to beat the earlier ones
    uint32_t em[4] = {0, 0, 0, 0};
GSM_UNROLL
    for (int i = 0;  i < 13;  i++)
    {
GSM_UNROLL
        for (int g = 0;  g < 4;  g++)
        {
            const int32_t t = x[g + 3*i] >> 2;
            em[g] += (uint32_t) (t*t);
        }
    }
    int32_t Mc = 0;
    int32_t EM = (int32_t) (em[0] << 1);
GSM_UNROLL
    for (int g = 1;  g < 4;  g++)
    {
        const int32_t v = (int32_t) (em[g] << 1);
        const bool up = (v > EM);
        Mc = up  ?  g  :  Mc;
        EM = up  ?  v  :  EM;
    }
    int32_t xM[13];
    int32_t xmax = 0;
GSM_UNROLL
    for (int i = 0;  i < 13;  i++)
    {
        xM[i] = gsm_pick4(Mc, x[3*i], x[3*i + 1], x[3*i + 2], x[3*i + 3]);
        const int32_t t = gsm_abs(xM[i]);
        xmax = (t > xmax)  ?  t  :  xmax;
    }
    // 4.2.15: the block maximum, coded; then the samples against it
    int32_t exp = 0;
    {
        int32_t t = xmax >> 9;
        bool stop = false;
GSM_UNROLL
        for (int i = 0;  i <= 5;  i++)
        {
            stop = stop  ||  (t <= 0);
            t >>= 1;
            exp += stop  ?  0  :  1;
        }
    }
    const int32_t xmaxc = gsm_add(xmax >> (exp + 5), exp*8);
    int32_t mant;
    gsm_exp_mant(xmaxc, exp, mant);
    const int32_t up = 1 << (6 - exp);
    // table 4.5, the inverse mantissa
    const int32_t nrfac = (mant & 4)  ?  gsm_pick4(mant, 20165, 18725, 17476, 16384)  :  gsm_pick4(mant, 29128, 26215, 23832, 21846);
    int32_t xMc[13], xMp[13];
GSM_UNROLL
    for (int i = 0;  i < 13;  i++)
        xMc[i] = (gsm_mult(gsm_s16(xM[i]*up), nrfac) >> 12) + 4;
    // 4.2.16, 4.2.17 and the update of the reconstructed residual
    gsm_apcm_inverse(xMc, mant, exp, xMp);
GSM_UNROLL
    for (int k = 0;  k < 40;  k++)
        m.st(base + k, gsm_add(gsm_grid_sample(k, Mc, xMp), dpp[k]));
    gsm_bits_put(bits, sink, Nc, 7);
    gsm_bits_put(bits, sink, bc, 2);
    gsm_bits_put(bits, sink, Mc, 2);
    gsm_bits_put(bits, sink, xmaxc, 6);
GSM_UNROLL
    for (int i = 0;  i < 13;  i++)
        gsm_bits_put(bits, sink, xMc[i], 3);
}

// The frame whose pre-processed samples are at m[120..279]: its 260 bits (behind the nibble 0xD where the packing has one)
// go to the stream, and the history moves on.
template <class M, class SINK>
GSM_HD void gsm_encode_frame(Gsm &s, M &m, GsmBitsOut &bits, SINK &sink)
{
    int32_t LARc[8];
    gsm_lpc_analysis(m, LARc);
    gsm_short_term_analysis(s, m, LARc);
    gsm_bits_raw(bits, sink, 0xDu, bits.voip  ?  4  :  0);
GSM_UNROLL
    for (int i = 0;  i < 8;  i++)
        gsm_bits_put(bits, sink, LARc[i], kGsmLarBits[i]);
GSM_ROLLED
    for (int k = 0;  k < 4;  k++)
        gsm_encode_subframe(m, kGsmHist + 40*k, bits, sink);
    gsm_shift_hist(m);
}

// ---- the decoder ----------------------------------------------------------------------------------------------------------

// One frame from the stage (bit `first_bit` of it on): 4.3.1 - 4.3.2 per subframe into m[120..279], the history moved on.
// The frame's LARc stay with the caller for gsm_decode_sample().
template <class M>
GSM_HD void gsm_decode_residual(Gsm &s, M &m, int32_t first_bit, int32_t LARc[8])
{
    GsmBitsIn bits;
    gsm_bits_from(bits, s.packing, first_bit);
GSM_UNROLL
    for (int i = 0;  i < 8;  i++)
        LARc[i] = gsm_bits_get(bits, m, kGsmLarBits[i]);
GSM_ROLLED
    for (int j = 0;  j < 4;  j++)
    {
        const int base = kGsmHist + 40*j;
        // (all 17 before a sample is written: the fourth subframe lands on the stage)
        const int32_t Nc = gsm_bits_get(bits, m, 7);
        const int32_t bc = gsm_bits_get(bits, m, 2);
        const int32_t Mc = gsm_bits_get(bits, m, 2);
        const int32_t xmaxc = gsm_bits_get(bits, m, 6);
        int32_t xMc[13], xMp[13];
GSM_UNROLL
        for (int i = 0;  i < 13;  i++)
            xMc[i] = gsm_bits_get(bits, m, 3);
        int32_t exp, mant;
        gsm_exp_mant(xmaxc, exp, mant);
        gsm_apcm_inverse(xMc, mant, exp, xMp);
        // a lag outside 40 .. 120 keeps the last one
        const int32_t Nr = (Nc < 40  ||  Nc > 120)  ?  s.nrp  :  Nc;
        s.nrp = Nr;
        const int32_t gain = gsm_qlb(bc);
GSM_UNROLL
        for (int k = 0;  k < 40;  k++)
            m.st(base + k, gsm_add(gsm_grid_sample(k, Mc, xMp), gsm_mult_r(gain, m.ld(base + k - Nr))));
    }
}

// 4.3.3 - 4.3.7: sample k of the frame through the short-term synthesis lattice (rrp: this range's coefficients),
// de-emphasis, upscaling and truncation
template <class M>
GSM_HD int32_t gsm_decode_sample(Gsm &s, const M &m, int k, const int32_t rrp[8])
{
    int32_t sri = m.ld(kGsmHist + k);
GSM_UNROLL
    for (int i = 7;  i >= 0;  i--)
    {
        sri = gsm_sub(sri, gsm_mult_r(rrp[i], s.v[i]));
        s.v[i + 1] = gsm_add(s.v[i], gsm_mult_r(rrp[i], sri));
    }
    s.v[0] = sri;
    s.msr = gsm_add(sri, gsm_mult_r(s.msr, 28180));
    return gsm_s16(gsm_add(s.msr, s.msr) & 0xFFF8);
}

// ---- the working memory of a host lane ------------------------------------------------------------------------------------

struct GsmHostMem
{
    int16_t a[kGsmMem];
    int32_t ld(int i) const { return a[i]; }
    void st(int i, int32_t v) { a[i] = (int16_t) v; }
    // the stage shares a[240..279], as it does in the kernels
    uint32_t byte(int n) const
    {
        uint8_t b;
        __builtin_memcpy(&b, (const uint8_t *) &a[kGsmStage] + n, 1);
        return b;
    }
    void stage_byte(int n, uint8_t b) { __builtin_memcpy((uint8_t *) &a[kGsmStage] + n, &b, 1); }
};

}   // namespace spg

#if defined(__HIPCC__)

namespace spg
{

// lane L's column of the wave's LDS: sample i in half (i & 1) of dword (i >> 1)*64 + L
struct GsmLds
{
    int16_t *col;
    __device__ __forceinline__ int32_t ld(int i) const { return col[(i >> 1)*128 + (i & 1)]; }
    __device__ __forceinline__ void st(int i, int32_t v) { col[(i >> 1)*128 + (i & 1)] = (int16_t) v; }
    __device__ __forceinline__ uint32_t byte(int n) const { return ((const uint8_t *) col)[(kGsmStage/2 + (n >> 2))*256 + (n & 3)]; }
    __device__ __forceinline__ void stage_word(int t, uint32_t w) { ((uint32_t *) col)[(kGsmStage/2 + t)*64] = w; }
};

enum { kGsmLdsWords = (kGsmMem/2)*64 };

// an encoder's words out: four make a chunk of the row
struct GsmRowSink
{
    RowOut out;
    uint8_t *dst;
    __device__ __forceinline__ void word(uint32_t w)
    {
        row_out_push<4>(out, w, 4);
        if (out.fill == 16)
        {
            row_flush(dst, out);
            out.w[0] = out.w[1] = 0;
            out.fill = 0;
            out.chunk++;
        }
    }
};

// lens are samples (whole units of the channel's packing: the host has checked) and counts bytes
__global__ __launch_bounds__(64) void gsm0610_encode_kernel(const CodecLaunch L)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[kGsmLdsWords];
    const int lane = threadIdx.x;
    const int ch = blockIdx.x*64 + lane;
    if (ch >= L.n_ch)
        return;
    const size_t n = (size_t) L.n_ch;
    int32_t *st = L.st + ch;
    const int mylen = L.lens  ?  min(max(L.lens[ch], 0), L.len)  :  L.len;
    const int frames = mylen/kGsmFrame;
    if (frames == 0)
    {
        L.counts[ch] = 0;
        return;
    }
    GsmLds m = {(int16_t *) (lds + lane)};
    Gsm s;
    gsm_load(s, st, n);
    gsm_load_hist(m, st, n);
    const uint8_t *src = L.in + (size_t) ch*L.in_stride;
    GsmRowSink sink;
    sink.out.w[0] = sink.out.w[1] = sink.out.w[2] = 0;
    sink.out.fill = 0;
    sink.out.chunk = 0;
    sink.dst = L.out + (size_t) ch*L.out_stride;
    GsmBitsOut bits;
    gsm_bits_begin(bits, s.packing);
_Pragma("nounroll")
    for (int f = 0;  f < frames;  f++)
    {
        // a frame is 20 chunks of the row, and starts on one
_Pragma("nounroll")
        for (int c = 0;  c < 20;  c++)
        {
            const uint4 q = *(const uint4 *) (src + 16*(size_t) (20*f + c));
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
_Pragma("unroll")
            for (int i = 0;  i < 4;  i++)
            {
                m.st(kGsmHist + 8*c + 2*i, gsm_preprocess(s, (int32_t) (w[i] & 0xFFFFu)));
                m.st(kGsmHist + 8*c + 2*i + 1, gsm_preprocess(s, (int32_t) (w[i] >> 16)));
            }
        }
        gsm_encode_frame(s, m, bits, sink);
    }
    gsm_bits_end(bits, sink);
    // what is left leaves as a chunk too: the row is written up to the next 16-byte boundary past its count
    if (sink.out.fill > 0)
        row_flush(sink.dst, sink.out);
    L.counts[ch] = (int32_t) gsm0610_encode_capacity(s.packing, mylen);
    gsm_store(s, st, n);
    gsm_store_hist(m, st, n);
}

// lens are bytes (whole units) and counts samples
__global__ __launch_bounds__(64) void gsm0610_decode_kernel(const CodecLaunch L)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[kGsmLdsWords];
    const int lane = threadIdx.x;
    const int ch = blockIdx.x*64 + lane;
    if (ch >= L.n_ch)
        return;
    const size_t n = (size_t) L.n_ch;
    int32_t *st = L.st + ch;
    const int mylen = L.lens  ?  min(max(L.lens[ch], 0), L.len)  :  L.len;
    const int packing = st[GW_PACKING*n];
    const int frames = (int) (gsm0610_decode_capacity(packing, mylen)/kGsmFrame);
    if (frames == 0)
    {
        L.counts[ch] = 0;
        return;
    }
    GsmLds m = {(int16_t *) (lds + lane)};
    Gsm s;
    gsm_load(s, st, n);
    gsm_load_hist(m, st, n);
    const uint8_t *src = L.in + (size_t) ch*L.in_stride;
    uint8_t *dst = L.out + (size_t) ch*L.out_stride;
    const int last = (mylen - 1) >> 4;
_Pragma("nounroll")
    for (int f = 0;  f < frames;  f++)
    {
        // where the frame starts in the row, in bits; the six chunks that hold its bytes go to the stage, from the 32-bit
        // word that holds the first byte on
        const int start = (packing == kGsmWav49)  ?  ((f >> 1)*520 + (f & 1)*260)  :  (f*8*gsm0610_unit_bytes(packing));
        const int byte0 = start >> 3;
        const int chunk0 = byte0 >> 4;
        const int skip = (byte0 & 15) >> 2;
_Pragma("unroll")
        for (int c = 0;  c < 6;  c++)
        {
            const uint4 q = row_chunk(src, chunk0 + c, last);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
_Pragma("unroll")
            for (int i = 0;  i < 4;  i++)
            {
                const int t = 4*c + i - skip;
                if (t >= 0  &&  t < kGsmStageBytes/4)
                    m.stage_word(t, w[i]);
            }
        }
        int32_t LARc[8], cur[8], prev[8], rrp[8];
        gsm_decode_residual(s, m, 8*(byte0 & 3) + (start & 7), LARc);
        gsm_decode_lar(s, LARc, cur, prev);
        // eight samples make a chunk of the row
        uint32_t w[4] = {0, 0, 0, 0};
        uint8_t *to = dst + 320*(size_t) f;
        int range = 0;
        gsm_range_rp(0, cur, prev, rrp);
_Pragma("nounroll")
        for (int c = 0;  c < 20;  c++)
        {
_Pragma("unroll")
            for (int i = 0;  i < 8;  i++)
            {
                const int k = 8*c + i;
                // (k is the same in every lane: the next range's coefficients are a branch of the wave; the last range
                // starts at sample 40, in the sixth chunk)
                if (c <= 5  &&  k == gsm_range_start(range + 1))
                    gsm_range_rp(++range, cur, prev, rrp);
                const uint32_t v = (uint32_t) gsm_decode_sample(s, m, k, rrp) & 0xFFFFu;
                w[i >> 1] = (i & 1)  ?  (w[i >> 1] | (v << 16))  :  v;
            }
            *(uint4 *) (to + 16*c) = make_uint4(w[0], w[1], w[2], w[3]);
        }
        gsm_shift_hist(m);
    }
    L.counts[ch] = frames*kGsmFrame;
    gsm_store(s, st, n);
    gsm_store_hist(m, st, n);
}

}   // namespace spg

#endif  // __HIPCC__
