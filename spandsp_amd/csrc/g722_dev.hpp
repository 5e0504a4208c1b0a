// g722_dev.hpp -- G.722 wideband codec banks (ITU-T G.722, the shape of spandsp's g722.c): one lane per channel, every channel
// with a rate (48 / 56 / 64 kbit/s), a sample rate (16 kHz through the QMF, or the low band alone as 8 kHz) and a packing
// (one code per byte, or the codes back to back, LSB first) of its own.
//
// The per-code functions are __host__ __device__ and the file compiles for the host (tests/c_callers/g722_host.cpp runs
// them one lane at a time under ASan and UBSan); G722Codec at the end, what codec_kernel<> (codec_rows.hpp) runs
// these functions through, is HIP only.
//
// int16_t arithmetic.  The reference leans on the truncation of its int16_t locals; here every value is an int32_t and each
// truncation is an explicit g722_s16().  A right shift of a negative value is arithmetic, as everywhere the reference is
// built; a left shift of a value that may be negative is written as a multiplication, so the host build has nothing for
// UBSan to report.
//
// The QMF history.  The reference keeps x[12] and y[12] as rings written at `ptr`.  A lane holds them in logical order
// (oldest first, the order the 12 coefficients meet them in), loads them with a per-lane address, x[(ptr + i) % 12], shifts
// them with compile-time indices and stores them back where the reference's ring would have them, with ptr advanced: no
// register is indexed by a run-time value, and get_state shows the reference's struct.
//
// The low-band quantizer.  g722.c:523-530 searches q6[1..29] for the first level above the error magnitude, each level
// scaled as (q6[i]*det) >> 12.  The scaled levels do not decrease with i, so the index is one more than the count of levels
// not above the magnitude, and wd >= (q*det) >> 12 is q*det < (wd + 1) << 12: 29 multiplies and compares with the levels as
// literals, and no per-lane loop.  The tables that lanes look up at indices of their own sit in one array, which the kernels
// keep in LDS; the high band's tables (qm2, wh, rh2, ihn, ihp) are selects.
//
// State words of a channel, st[word*n + ch], in the order of the reference's fields: packed, eight_k, bits_per_sample,
// x[12], y[12], ptr, band[0] then band[1] each as nb, det, s, sz, r, p[2], a[2], b[6], d[7], then in_buffer / out_buffer and
// in_bits / out_bits (74).  itu_test_mode is left out: no public call sets it.

#pragma once

#include <stddef.h>
#include <stdint.h>

#include "codec_rows.hpp"

#ifdef __HIPCC__
#define G722_HD __host__ __device__ __forceinline__
#define G722_UNROLL _Pragma("unroll")
#else
#define G722_HD static inline
#define G722_UNROLL
#endif

namespace spg
{

enum
{
    G2_PACKED = 0, G2_EIGHT_K, G2_BPS,
    G2_X0,                          // .. G2_X0 + 11
    G2_Y0 = G2_X0 + 12,             // .. G2_Y0 + 11
    G2_PTR = G2_Y0 + 12,
    G2_BAND0,                       // 22 words
    G2_BAND1 = G2_BAND0 + 22,
    G2_BUFFER = G2_BAND1 + 22, G2_BITS,
    kG722Words
};
// within a band
enum { G2B_NB = 0, G2B_DET, G2B_S, G2B_SZ, G2B_R, G2B_P0, G2B_P1, G2B_A0, G2B_A1, G2B_B0, G2B_D0 = G2B_B0 + 6, kG722BandWords = G2B_D0 + 7 };

enum { kG722EightK = 1, kG722Packed = 2 };          // G722_SAMPLE_RATE_8000, G722_PACKED

// The tables a lane looks up at an index of its own (G.722 tables 14 to 21): the codes of the 30 low-band intervals for a
// negative and then for a positive difference, the linear step sizes, the 4-, 5- and 6-bit inverse quantizers of the low
// band, the log scale factor multipliers and the index into them.
enum
{
    G2T_ILN = 0, G2T_ILP = 32, G2T_ILB = 64, G2T_QM4 = 96, G2T_QM5 = 112, G2T_QM6 = 144, G2T_WL = 208, G2T_RL42 = 216,
    kG722TabUsed = 232, kG722TabWords = 256
};
#define G2_TABLE_INIT                                                                                                          \
{                                                                                                                              \
    /* iln */                                                                                                                  \
    0, 63, 62, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20, 19, 18, 17, 16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 0,   \
    /* ilp */                                                                                                                  \
    0, 61, 60, 59, 58, 57, 56, 55, 54, 53, 52, 51, 50, 49, 48, 47, 46, 45, 44, 43, 42, 41, 40, 39, 38, 37, 36, 35, 34, 33, 32, 0, \
    /* ilb */                                                                                                                  \
    2048, 2093, 2139, 2186, 2233, 2282, 2332, 2383, 2435, 2489, 2543, 2599, 2656, 2714, 2774, 2834,                            \
    2896, 2960, 3025, 3091, 3158, 3228, 3298, 3371, 3444, 3520, 3597, 3676, 3756, 3838, 3922, 4008,                            \
    /* qm4 */                                                                                                                  \
    0, -20456, -12896, -8968, -6288, -4240, -2584, -1200, 20456, 12896, 8968, 6288, 4240, 2584, 1200, 0,                       \
    /* qm5 */                                                                                                                  \
    -280, -280, -23352, -17560, -14120, -11664, -9752, -8184, -6864, -5712, -4696, -3784, -2960, -2208, -1520, -880,           \
    23352, 17560, 14120, 11664, 9752, 8184, 6864, 5712, 4696, 3784, 2960, 2208, 1520, 880, 280, -280,                          \
    /* qm6 */                                                                                                                  \
    -136, -136, -136, -136, -24808, -21904, -19008, -16704, -14984, -13512, -12280, -11192, -10232, -9360, -8576, -7856,       \
    -7192, -6576, -6000, -5456, -4944, -4464, -4008, -3576, -3168, -2776, -2400, -2032, -1688, -1360, -1040, -728,             \
    24808, 21904, 19008, 16704, 14984, 13512, 12280, 11192, 10232, 9360, 8576, 7856, 7192, 6576, 6000, 5456,                   \
    4944, 4464, 4008, 3576, 3168, 2776, 2400, 2032, 1688, 1360, 1040, 728, 432, 136, -432, -136,                               \
    /* wl */                                                                                                                   \
    -60, -30, 58, 172, 334, 538, 1198, 3042,                                                                                   \
    /* rl42 */                                                                                                                 \
    0, 7, 6, 5, 4, 3, 2, 1, 7, 6, 5, 4, 3, 2, 1, 0,                                                                            \
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0                                                     \
}

#if defined(__HIPCC__)
__device__ const int32_t kG722TabDev[kG722TabWords] = G2_TABLE_INIT;
#endif
static const int32_t kG722TabHost[kG722TabWords] = G2_TABLE_INIT;

// the decision levels of the low-band quantizer, q6[1 .. 29] (G.722 table 14), and the two QMF halves (table 11): the
// same for every lane, so literals
static constexpr int32_t kG722Q6[29] = {35, 72, 110, 150, 190, 233, 276, 323, 370, 422, 473, 530, 587, 650, 714, 786, 858, 940, 1023,
                                        1121, 1219, 1339, 1458, 1612, 1765, 1980, 2195, 2557, 2919};
static constexpr int32_t kG722Qmf[12] = {3, -11, 12, 32, -210, 951, 3876, -805, 362, -156, 53, -11};

struct G722Band
{
    int32_t nb, det, s, sz, r;
    int32_t p[2], a[2], b[6], d[7];
};

struct G722
{
    int32_t packed, eight_k, bps;       // this channel's configuration
    int32_t x[12], y[12];               // in logical order: [0] the oldest
    int32_t ptr;
    G722Band band[2];
    uint32_t buffer;
    int32_t bits;
};

G722_HD int32_t g722_s16(int32_t x)
{
    return (int32_t) (int16_t) (uint16_t) (uint32_t) x;
}

G722_HD int32_t g722_sat16(int32_t x)
{
    return (x > 32767)  ?  32767  :  ((x < -32768)  ?  -32768  :  x);
}

G722_HD int32_t g722_sat15(int32_t x)
{
    return (x > 16383)  ?  16383  :  ((x < -16384)  ?  -16384  :  x);
}

G722_HD int32_t g722_abs(int32_t x)
{
    return (x < 0)  ?  -x  :  x;
}

// do two int16_t values differ in sign
G722_HD bool g722_signs_differ(int32_t a, int32_t b)
{
    return ((a ^ b) & 0x8000) != 0;
}

// bits per sample of a rate as g722_*_init() has it (g722.c:423-428): every rate but 48000 and 56000 is 8 bits
static inline int g722_bits_of_rate(int rate)
{
    return (rate == 48000)  ?  6  :  ((rate == 56000)  ?  7  :  8);
}

// g722_encode_init() / g722_decode_init(), g722.c:413-441, 621-648.  false: a rate or option bits this bank refuses
static inline bool g722_init_words(int32_t w[kG722Words], int rate, int options)
{
    if ((rate != 48000  &&  rate != 56000  &&  rate != 64000)  ||  (options & ~(kG722EightK | kG722Packed)) != 0)
        return false;
    for (int i = 0;  i < kG722Words;  i++)
        w[i] = 0;
    w[G2_BPS] = g722_bits_of_rate(rate);
    w[G2_EIGHT_K] = (options & kG722EightK)  ?  1  :  0;
    w[G2_PACKED] = ((options & kG722Packed)  &&  w[G2_BPS] != 8)  ?  1  :  0;
    w[G2_BAND0 + G2B_DET] = 32;
    w[G2_BAND1 + G2B_DET] = 8;
    return true;
}

// ---- the blocks of the recommendation ---------------------------------------------------------------------------------

// block4(), g722.c:184-258: the adaptive predictor of one band takes the quantized difference dx
G722_HD void g722_block4(G722Band &b, int32_t dx)
{
    // RECONS, PARREC
    const int32_t r = g722_sat16(b.s + dx);
    const int32_t p = g722_sat16(b.sz + dx);
    // UPPOL2
    const bool sg0 = g722_signs_differ(p, b.p[0]);
    const bool sg1 = g722_signs_differ(p, b.p[1]);
    const int32_t a0x4 = g722_sat16(b.a[0]*4);
    int32_t wd32 = sg0  ?  a0x4  :  -a0x4;
    wd32 = (wd32 > 32767)  ?  32767  :  wd32;
    int32_t ap1 = g722_s16((sg1  ?  -128  :  128) + (wd32 >> 7) + ((b.a[1]*32512) >> 15));
    ap1 = (ap1 > 12288)  ?  12288  :  ((ap1 < -12288)  ?  -12288  :  ap1);
    // UPPOL1
    int32_t ap0 = g722_sat16((sg0  ?  -192  :  192) + g722_s16((b.a[0]*32640) >> 15));
    const int32_t lim = g722_sat16(15360 - ap1);
    ap0 = (ap0 > lim)  ?  lim  :  ((ap0 < -lim)  ?  -lim  :  ap0);
    // FILTEP
    const int32_t wd1 = g722_s16((ap0*g722_sat16(r + r)) >> 15);
    const int32_t wd2 = g722_s16((ap1*g722_sat16(b.r + b.r)) >> 15);
    const int32_t sp = g722_sat16(wd1 + wd2);
    b.r = r;
    b.a[1] = ap1;
    b.a[0] = ap0;
    b.p[1] = b.p[0];
    b.p[0] = p;
    // UPZERO, DELAYA, FILTEZ
    const int32_t step = (dx == 0)  ?  0  :  128;
    b.d[0] = dx;
    int32_t sz = 0;
G722_UNROLL
    for (int i = 5;  i >= 0;  i--)
    {
        const int32_t up = g722_signs_differ(b.d[i + 1], dx)  ?  -step  :  step;
        b.b[i] = g722_sat16(up + g722_s16((b.b[i]*32640) >> 15));
        sz += (b.b[i]*g722_sat16(b.d[i] + b.d[i])) >> 15;
        b.d[i + 1] = b.d[i];
    }
    b.sz = g722_sat16(sz);
    // PREDIC
    b.s = g722_sat16(sp + b.sz);
}

// the linear scale factor of a band from its log one: SCALEL (shift 8) / SCALEH (shift 10)
template <typename TAB>
G722_HD int32_t g722_scale(TAB tab, int32_t nb, int32_t base)
{
    const int32_t v = tab[G2T_ILB + ((nb >> 6) & 31)];
    const int32_t sh = base - (nb >> 11);
    const int32_t wd3 = (sh < 0)  ?  (v << ((-sh) & 31))  :  (v >> (sh & 31));
    return g722_s16(wd3*4);
}

// Blocks 2L, 3L and 4L, which the encoder and the decoder share: ril is the 4-bit index
template <typename TAB>
G722_HD void g722_low_band(G722Band &b, TAB tab, int32_t ril)
{
    // INVQAL
    const int32_t dlow = g722_s16((b.det*tab[G2T_QM4 + ril]) >> 15);
    // LOGSCL
    int32_t nb = ((b.nb*127) >> 7) + tab[G2T_WL + tab[G2T_RL42 + ril]];
    nb = (nb < 0)  ?  0  :  ((nb > 18432)  ?  18432  :  nb);
    b.nb = nb;
    // SCALEL
    b.det = g722_scale(tab, nb, 8);
    g722_block4(b, dlow);
}

// Blocks 2H, 3H and 4H; the dhigh they are made with is returned (the decoder rebuilds rhigh with the old s before this)
template <typename TAB>
G722_HD void g722_high_band(G722Band &b, TAB tab, int32_t ihigh, int32_t dhigh)
{
    // LOGSCH: wh[rh2[ihigh]]
    int32_t nb = ((b.nb*127) >> 7) + ((ihigh & 1)  ?  -214  :  798);
    nb = (nb < 0)  ?  0  :  ((nb > 22528)  ?  22528  :  nb);
    b.nb = nb;
    // SCALEH
    b.det = g722_scale(tab, nb, 10);
    g722_block4(b, dhigh);
}

// INVQAH: qm2[ihigh] scaled
G722_HD int32_t g722_dhigh(const G722Band &b, int32_t ihigh)
{
    const int32_t mag = (ihigh & 1)  ?  1616  :  7408;
    return g722_s16((b.det*((ihigh & 2)  ?  mag  :  -mag)) >> 15);
}

// the two halves of the QMF on the histories in logical order: x meets the coefficients forwards, y backwards.  Both sums are
// exact in an int32_t (|sum| <= 32768*6482), so their order is free.
G722_HD void g722_qmf(const G722 &s, int32_t *sumx, int32_t *sumy)
{
    int32_t ax = 0;
    int32_t ay = 0;
G722_UNROLL
    for (int i = 0;  i < 12;  i++)
    {
        ax += s.x[i]*kG722Qmf[i];
        ay += s.y[i]*kG722Qmf[11 - i];
    }
    *sumx = ax;
    *sumy = ay;
}

G722_HD void g722_qmf_shift(G722 &s, int32_t x, int32_t y)
{
G722_UNROLL
    for (int i = 0;  i < 11;  i++)
    {
        s.x[i] = s.x[i + 1];
        s.y[i] = s.y[i + 1];
    }
    s.x[11] = x;
    s.y[11] = y;
    s.ptr = (s.ptr >= 11)  ?  0  :  (s.ptr + 1);
}

// One code of g722_encode(), g722.c:485-615, before the packing: a0 is the sample of an 8 kHz lane, a0 and a1 the pair of
// a 16 kHz one
template <typename TAB>
G722_HD int32_t g722_encode_code(G722 &s, TAB tab, int32_t a0, int32_t a1)
{
    int32_t xlow = g722_s16(a0) >> 1;
    int32_t xhigh = 0;
    if (!s.eight_k)
    {
        // the transmit QMF
        int32_t sumodd;
        int32_t sumeven;
        g722_qmf_shift(s, g722_s16(a0), g722_s16(a1));
        g722_qmf(s, &sumodd, &sumeven);
        xlow = g722_s16((sumeven + sumodd) >> 14);
        xhigh = g722_s16((sumeven - sumodd) >> 14);
    }
    // Block 1L: SUBTRA, QUANTL
    G722Band &lo = s.band[0];
    const int32_t el = g722_sat16(xlow - lo.s);
    const int32_t wd = (el >= 0)  ?  el  :  ~el;
    const uint32_t edge = ((uint32_t) wd + 1) << 12;
    const uint32_t det = (uint32_t) lo.det;
    int32_t i = 1;
G722_UNROLL
    for (int k = 0;  k < 29;  k++)
        i += ((uint32_t) kG722Q6[k]*det < edge)  ?  1  :  0;
    const int32_t ilow = tab[((el < 0)  ?  G2T_ILN  :  G2T_ILP) + i];
    g722_low_band(lo, tab, ilow >> 2);
    int32_t ihigh = 3;
    if (!s.eight_k)
    {
        // Block 1H: SUBTRA, QUANTH
        G722Band &hi = s.band[1];
        const int32_t eh = g722_sat16(xhigh - hi.s);
        const int32_t wh = (eh >= 0)  ?  eh  :  ~eh;
        const int32_t mih = (wh >= ((564*hi.det) >> 12))  ?  2  :  1;
        // ihn[] = {0, 1, 0}, ihp[] = {0, 3, 2}
        ihigh = (eh < 0)  ?  ((mih == 1)  ?  1  :  0)  :  ((mih == 1)  ?  3  :  2);
        const int32_t dhigh = g722_dhigh(hi, ihigh);
        g722_high_band(hi, tab, ihigh, dhigh);
    }
    return ((ihigh << 6) | ilow) >> (8 - s.bps);
}

// One code of g722_decode(), g722.c:298-406, after the unpacking.  out[0] (and out[1] on a 16 kHz lane) are the samples.
template <typename TAB>
G722_HD void g722_decode_code(G722 &s, TAB tab, int32_t code, int32_t out[2])
{
    // the three bits_per_sample cases: the low bits are 6, 5 or 4 wide
    const int32_t lowbits = s.bps - 2;
    const int32_t wide = code & ((1 << lowbits) - 1);
    const int32_t ihigh = (code >> lowbits) & 3;
    const int32_t qbase = (s.bps == 8)  ?  G2T_QM6  :  ((s.bps == 7)  ?  G2T_QM5  :  G2T_QM4);
    const int32_t ril = wide >> (lowbits - 4);
    G722Band &lo = s.band[0];
    // Blocks 5L, 6L: INVQBL, RECONS, LIMIT
    const int32_t rlow = g722_sat15(lo.s + ((lo.det*tab[qbase + wide]) >> 15));
    g722_low_band(lo, tab, ril);
    if (s.eight_k)
    {
        out[0] = g722_s16(rlow*2);
        out[1] = 0;
    }
    else
    {
        G722Band &hi = s.band[1];
        const int32_t dhigh = g722_dhigh(hi, ihigh);
        // Blocks 5H, 6H
        const int32_t rhigh = g722_sat15(dhigh + hi.s);
        g722_high_band(hi, tab, ihigh, dhigh);
        // the receive QMF
        int32_t sumx;
        int32_t sumy;
        g722_qmf_shift(s, g722_s16(rlow + rhigh), g722_s16(rlow - rhigh));
        g722_qmf(s, &sumx, &sumy);
        out[0] = g722_sat16(sumy >> 11);
        out[1] = g722_sat16(sumx >> 11);
    }
}

// ---- packing, LSB first: g722.c:279-296 and 597-614 --------------------------------------------------------------------

// the encoder's side: one code in; true: *byte comes out
G722_HD bool g722_pack(G722 &s, int32_t code, int32_t *byte)
{
    const uint32_t buf = s.buffer | ((uint32_t) code << (s.bits & 31));
    const int32_t bits = s.bits + s.bps;
    const bool full = (bits >= 8);
    *byte = (int32_t) ((s.packed  ?  buf  :  (uint32_t) code) & 0xFF);
    s.buffer = s.packed  ?  (full  ?  (buf >> 8)  :  buf)  :  s.buffer;
    s.bits = s.packed  ?  (full  ?  (bits - 8)  :  bits)  :  s.bits;
    return !s.packed  ||  full;
}

// the decoder's side: does the next code take another byte first
G722_HD bool g722_unpack_needs(const G722 &s)
{
    return !s.packed  ||  s.bits < s.bps;
}

// ... and the code (an unpacked channel's still has its bits above the width); `byte` is taken only if g722_unpack_needs()
G722_HD int32_t g722_unpack(G722 &s, int32_t byte)
{
    const bool need = s.bits < s.bps;
    const uint32_t ub = (uint32_t) byte & 0xFF;
    const uint32_t buf = need  ?  (s.buffer | (ub << (s.bits & 31)))  :  s.buffer;
    const int32_t bits = s.bits + (need  ?  8  :  0);
    const uint32_t code = buf & ((1u << s.bps) - 1);
    s.buffer = s.packed  ?  (buf >> s.bps)  :  s.buffer;
    s.bits = s.packed  ?  (bits - s.bps)  :  s.bits;
    return (int32_t) (s.packed  ?  code  :  ub);
}

// Codes g722_decode() makes of `bytes` (> 0) bytes: its loop ends with the code for which the last byte was read, so a
// whole code may stay buffered, and the next call starts with it
G722_HD int32_t g722_decode_codes(const G722 &s, int32_t bytes)
{
    return s.packed  ?  ((s.bits + 8*(bytes - 1))/s.bps + 1)  :  bytes;
}

// Bytes a row must hold for `samples` samples encoded (up to 7 bits may wait in the buffer), and samples for `bytes` bytes
// decoded (up to 7 bits may wait as well)
static inline long long g722_encode_capacity(int bps, int packed, int eight_k, long long samples)
{
    const long long codes = eight_k  ?  samples  :  (samples/2);
    return packed  ?  ((codes*bps + 7)/8)  :  codes;
}

static inline long long g722_decode_capacity(int bps, int packed, int eight_k, long long bytes)
{
    const long long codes = (bytes <= 0)  ?  0  :  (packed  ?  ((7 + 8*bytes)/bps)  :  bytes);
    return eight_k  ?  codes  :  (2*codes);
}

G722_HD void g722_band_load(G722Band &b, const int32_t *st, size_t n)
{
    b.nb = st[G2B_NB*n];
    b.det = st[G2B_DET*n];
    b.s = st[G2B_S*n];
    b.sz = st[G2B_SZ*n];
    b.r = st[G2B_R*n];
    b.p[0] = st[G2B_P0*n];
    b.p[1] = st[G2B_P1*n];
    b.a[0] = st[G2B_A0*n];
    b.a[1] = st[G2B_A1*n];
G722_UNROLL
    for (int i = 0;  i < 6;  i++)
        b.b[i] = st[(G2B_B0 + i)*n];
G722_UNROLL
    for (int i = 0;  i < 7;  i++)
        b.d[i] = st[(G2B_D0 + i)*n];
}

G722_HD void g722_band_store(const G722Band &b, int32_t *st, size_t n)
{
    st[G2B_NB*n] = b.nb;
    st[G2B_DET*n] = b.det;
    st[G2B_S*n] = b.s;
    st[G2B_SZ*n] = b.sz;
    st[G2B_R*n] = b.r;
    st[G2B_P0*n] = b.p[0];
    st[G2B_P1*n] = b.p[1];
    st[G2B_A0*n] = b.a[0];
    st[G2B_A1*n] = b.a[1];
G722_UNROLL
    for (int i = 0;  i < 6;  i++)
        st[(G2B_B0 + i)*n] = b.b[i];
G722_UNROLL
    for (int i = 0;  i < 7;  i++)
        st[(G2B_D0 + i)*n] = b.d[i];
}

// where the ring of the reference has logical position i
G722_HD int g722_ring(int32_t ptr, int i)
{
    const int at = ptr + i;
    return (at >= 12)  ?  (at - 12)  :  at;
}

G722_HD void g722_load(G722 &s, const int32_t *st, size_t n)
{
    s.packed = st[G2_PACKED*n];
    s.eight_k = st[G2_EIGHT_K*n];
    s.bps = st[G2_BPS*n];
    s.ptr = st[G2_PTR*n];
G722_UNROLL
    for (int i = 0;  i < 12;  i++)
    {
        const size_t at = (size_t) g722_ring(s.ptr, i);
        s.x[i] = st[(G2_X0 + at)*n];
        s.y[i] = st[(G2_Y0 + at)*n];
    }
    g722_band_load(s.band[0], st + G2_BAND0*n, n);
    g722_band_load(s.band[1], st + G2_BAND1*n, n);
    s.buffer = (uint32_t) st[G2_BUFFER*n];
    s.bits = st[G2_BITS*n];
}

// (an 8 kHz channel touches neither its histories nor its high band: they are written back as they were read)
G722_HD void g722_store(const G722 &s, int32_t *st, size_t n)
{
    st[G2_PTR*n] = s.ptr;
G722_UNROLL
    for (int i = 0;  i < 12;  i++)
    {
        const size_t at = (size_t) g722_ring(s.ptr, i);
        st[(G2_X0 + at)*n] = s.x[i];
        st[(G2_Y0 + at)*n] = s.y[i];
    }
    g722_band_store(s.band[0], st + G2_BAND0*n, n);
    g722_band_store(s.band[1], st + G2_BAND1*n, n);
    st[G2_BUFFER*n] = (int32_t) s.buffer;
    st[G2_BITS*n] = s.bits;
}

// ---- the kernels: codec_kernel<G722Codec, ENCODE> (codec_rows.hpp) ------------------------------------------------------

#if defined(__HIPCC__)  &&  !defined(SPG_G722_STEP_FUNCTIONS_ONLY)

// Four codes between two advances of the window: a 16 kHz encoder's four pairs are 16 bytes in, and a 16 kHz decoder makes
// 16 bytes of four codes.  A 16 kHz encoder's position in its row is a multiple of 4 (the whole word, both samples), an
// 8 kHz one's a multiple of 2.
struct G722Codec
{
    typedef G722 State;
    static constexpr int kTabWords = kG722TabWords;
    static constexpr int kGroup = 4;
    static constexpr int kWidest = 4;

    static __device__ __forceinline__ const int32_t *table() { return kG722TabDev; }
    static __device__ __forceinline__ void load(G722 &s, const int32_t *st, size_t n) { g722_load(s, st, n); }
    static __device__ __forceinline__ void store(const G722 &s, int32_t *st, size_t n) { g722_store(s, st, n); }
    static __device__ __forceinline__ int pcm_bytes(int) { return 2; }

    // samples of a code
    static __device__ __forceinline__ int unit(const G722 &s)
    {
        return s.eight_k  ?  1  :  2;
    }

    // (a decoder's count follows from the bits waiting in its state: never past the row, whatever a caller has set there)
    template <bool ENCODE>
    static __device__ __forceinline__ int todo(const G722 &s, int per, int mylen, long long out_stride)
    {
        return ENCODE  ?  (mylen/per)  :  (int) min((long long) g722_decode_codes(s, mylen), out_stride/(2*per));
    }

    template <bool ENCODE>
    static __device__ __forceinline__ int32_t take(const G722 &s, int per)
    {
        return ENCODE  ?  (2*per)  :  (g722_unpack_needs(s)  ?  1  :  0);
    }

    template <bool ENCODE>
    static __device__ __forceinline__ RowPush step(G722 &s, const int32_t *table, int per, uint32_t raw)
    {
        if (ENCODE)
        {
            const int32_t code = g722_encode_code(s, table, (int32_t) (raw & 0xFFFF), (int32_t) (raw >> 16));
            int32_t byte;
            const bool full = g722_pack(s, code, &byte);
            return {(uint32_t) byte, full  ?  1  :  0};
        }
        else
        {
            const int32_t code = g722_unpack(s, (int32_t) raw);
            int32_t amp[2];
            g722_decode_code(s, table, code, amp);
            return {((uint32_t) amp[0] & 0xFFFF) | ((uint32_t) amp[1] << 16), 2*per};
        }
    }
};

#endif  // __HIPCC__

}   // namespace spg
