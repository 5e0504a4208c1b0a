// g726_dev.hpp -- G.726 ADPCM codec banks (ITU-T G.726, the shape of spandsp's g726.c): one lane per channel, every channel
// with a rate (16 / 24 / 32 / 40 kbit/s), an external coding (linear, u-law, A-law) and a packing (none, left, right) of its own.
//
// The per-sample functions are __host__ __device__ and the file compiles for the host (tests/c_callers/g726_host.cpp runs
// them one lane at a time under ASan and UBSan); G726Codec at the end, what codec_kernel<> (codec_rows.hpp) runs
// these functions through, is HIP only.
//
// How the reference's four encoders and four decoders become one body.  They differ in the tables, in the mask applied
// to dq when sr is rebuilt (0x7FFF at 40 kbit/s, 0x3FFF otherwise), in the leak of the zero predictor (>> 9 at 40 kbit/s) and in
// the quantizer's size; all four follow from the bits per sample, so a lane carries `bps` and the tables sit in one array,
// 112 words per rate, which the kernels keep in LDS: the lanes of a wave look them up at different indices.
//
// int16_t arithmetic.  The reference leans on the truncation of its int16_t locals; here every value is an int32_t and each
// truncation is an explicit g726_s16().  Shifts of values that may be negative are written as multiplications or on the
// magnitude, so the host build has nothing for UBSan to report.
//
// State words of a channel, st[word*n + ch], in the order of the reference's fields: yl, yu, dms, dml, ap, a[2], b[6],
// pk[2], dq[6], sr[2], td, bs.bitstream, bs.residue, then rate, ext_coding, bits_per_sample, packing.

#pragma once

#include <stddef.h>
#include <stdint.h>

#include "codec_rows.hpp"

#ifdef __HIPCC__
#define G726_HD __host__ __device__ __forceinline__
#define G726_UNROLL _Pragma("unroll")
#else
#define G726_HD static inline
#define G726_UNROLL
#endif

// a condition some lane of the wave meets (the host runs one lane)
#if defined(__HIP_DEVICE_COMPILE__)
#define G726_ANY(x) (__any(x))
#else
#define G726_ANY(x) (x)
#endif

namespace spg
{

enum
{
    G7_YL = 0, G7_YU, G7_DMS, G7_DML, G7_AP,
    G7_A0, G7_A1,
    G7_B0,                      // .. G7_B0 + 5
    G7_PK0 = G7_B0 + 6, G7_PK1,
    G7_DQ0,                     // .. G7_DQ0 + 5
    G7_SR0 = G7_DQ0 + 6, G7_SR1,
    G7_TD, G7_BITSTREAM, G7_RESIDUE,
    G7_RATE, G7_CODING, G7_BPS, G7_PACKING,
    kG726Words
};
constexpr int kG726Dynamic = G7_RATE;       // the words a call changes

enum { kG726Linear = 0, kG726Ulaw = 1, kG726Alaw = 2 };         // G726_ENCODING_*
enum { kG726PackNone = 0, kG726PackLeft = 1, kG726PackRight = 2 };      // G726_PACKING_*

// Per rate: 16 quantizer decision levels (ascending, padded with a level no dln reaches), then 32 entries each of the
// reconstruction levels, the scale factor multipliers and the speed control inputs (G.726 tables 5-10, g726.c:88-215).
constexpr int kG726TabStride = 112;
constexpr int kG726TabWords = 4*kG726TabStride;
#define G7P 0x7FFFFFFF
#define G7_TABLE_INIT                                                                                                          \
{                                                                                                                              \
    /* 16 kbit/s */                                                                                                            \
    261, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P,                                            \
    116, 365, 365, 116, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,                    \
    -704, 14048, 14048, -704, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,              \
    0x000, 0xE00, 0xE00, 0x000, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,            \
    /* 24 kbit/s */                                                                                                            \
    8, 218, 331, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P,                                              \
    -2048, 135, 273, 373, 373, 273, 135, -2048, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,        \
    -128, 960, 4384, 18624, 18624, 4384, 960, -128, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,    \
    0x000, 0x200, 0x400, 0xE00, 0xE00, 0x400, 0x200, 0x000, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, \
    /* 32 kbit/s */                                                                                                            \
    -124, 80, 178, 246, 300, 349, 400, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P, G7P,                                            \
    -2048, 4, 135, 213, 273, 323, 373, 425, 425, 373, 323, 273, 213, 135, 4, -2048, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, \
    -384, 576, 1312, 2048, 3584, 6336, 11360, 35904, 35904, 11360, 6336, 3584, 2048, 1312, 576, -384,                          \
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,                                                                            \
    0x000, 0x000, 0x000, 0x200, 0x200, 0x200, 0x600, 0xE00, 0xE00, 0x600, 0x200, 0x200, 0x200, 0x000, 0x000, 0x000,            \
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,                                                                            \
    /* 40 kbit/s */                                                                                                            \
    -122, -16, 68, 139, 198, 250, 298, 339, 378, 413, 445, 475, 502, 528, 553, G7P,                                            \
    -2048, -66, 28, 104, 169, 224, 274, 318, 358, 395, 429, 459, 488, 514, 539, 566,                                           \
    566, 539, 514, 488, 459, 429, 395, 358, 318, 274, 224, 169, 104, 28, -66, -2048,                                           \
    448, 448, 768, 1248, 1280, 1312, 1856, 3200, 4512, 5728, 7008, 8960, 11456, 14080, 16928, 22272,                           \
    22272, 16928, 14080, 11456, 8960, 7008, 5728, 4512, 3200, 1856, 1312, 1280, 1248, 768, 448, 448,                           \
    0x000, 0x000, 0x000, 0x000, 0x000, 0x200, 0x200, 0x200, 0x200, 0x200, 0x400, 0x600, 0x800, 0xA00, 0xC00, 0xC00,            \
    0xC00, 0xC00, 0xA00, 0x800, 0x600, 0x400, 0x200, 0x200, 0x200, 0x200, 0x200, 0x000, 0x000, 0x000, 0x000, 0x000             \
}

#if defined(__HIPCC__)
__device__ const int32_t kG726TabDev[kG726TabWords] = G7_TABLE_INIT;
#endif
static const int32_t kG726TabHost[kG726TabWords] = G7_TABLE_INIT;
#undef G7P

struct G726
{
    int32_t yl, yu, dms, dml, ap;
    int32_t a[2], b[6], pk[2], dq[6], sr[2];
    int32_t td;
    uint32_t bitstream;
    int32_t residue;
    int32_t coding, bps, packing;       // this channel's configuration
};

G726_HD int32_t g726_s16(int32_t x)
{
    return (int32_t) (int16_t) (uint16_t) (uint32_t) x;
}

G726_HD int32_t g726_abs(int32_t x)
{
    return (x < 0)  ?  -x  :  x;
}

// top_bit(), bit_operations.h: the highest bit set, -1 for 0
G726_HD int g726_top_bit(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return 31 - __clz((int) x);
#else
    return x  ?  (31 - __builtin_clz(x))  :  -1;
#endif
}

// g726_init(), g726.c:1175-1238.  false: a rate, coding or packing it (or this bank) refuses
static inline bool g726_init_words(int32_t w[kG726Words], int rate, int coding, int packing)
{
    if ((rate != 16000  &&  rate != 24000  &&  rate != 32000  &&  rate != 40000)
        ||  coding < kG726Linear  ||  coding > kG726Alaw  ||  packing < kG726PackNone  ||  packing > kG726PackRight)
        return false;
    for (int i = 0;  i < kG726Words;  i++)
        w[i] = 0;
    w[G7_YL] = 34816;
    w[G7_YU] = 544;
    w[G7_SR0] = w[G7_SR1] = 32;
    for (int i = 0;  i < 6;  i++)
        w[G7_DQ0 + i] = 32;
    w[G7_RATE] = rate;
    w[G7_CODING] = coding;
    w[G7_BPS] = rate/8000;
    w[G7_PACKING] = packing;
    return true;
}

// ---- G.711, spandsp/g711.h:128-252 ------------------------------------------------------------------------------------

G726_HD int32_t g726_ulaw_to_linear(int32_t code)
{
    const int32_t u = ~code & 0xFF;
    const int32_t t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4);
    return (u & 0x80)  ?  (0x84 - t)  :  (t - 0x84);
}

G726_HD int32_t g726_alaw_to_linear(int32_t code)
{
    const int32_t a = (code ^ 0x55) & 0xFF;
    const int32_t i = (a & 0x0F) << 4;
    const int32_t sg = (a & 0x70) >> 4;
    const int32_t v = sg  ?  ((i + 0x108) << ((sg - 1) & 7))  :  (i + 8);
    return (a & 0x80)  ?  v  :  -v;
}

G726_HD int32_t g726_linear_to_ulaw(int32_t linear)
{
    const int32_t mask = (linear >= 0)  ?  0xFF  :  0x7F;
    const int32_t mag = 0x84 + g726_abs(linear);
    const int seg = g726_top_bit((uint32_t) mag | 0xFF) - 7;
    const int32_t v = (seg >= 8)  ?  0x7F  :  ((seg << 4) | ((mag >> ((seg + 3) & 31)) & 0xF));
    return v ^ mask;
}

G726_HD int32_t g726_linear_to_alaw(int32_t linear)
{
    const int32_t mask = (linear >= 0)  ?  (0x55 | 0x80)  :  0x55;
    const int32_t mag = (linear >= 0)  ?  linear  :  (-linear - 1);
    const int seg = g726_top_bit((uint32_t) mag | 0xFF) - 7;
    const int32_t v = (seg >= 8)  ?  0x7F  :  ((seg << 4) | ((mag >> (seg  ?  ((seg + 3) & 31)  :  4)) & 0x0F));
    return v ^ mask;
}

// ---- the blocks of the recommendation ---------------------------------------------------------------------------------

// fmult(), g726.c:221-239: an is a 14-bit coefficient, srn a 4-bit exponent / 6-bit mantissa value
G726_HD int32_t g726_fmult(int32_t an, int32_t srn)
{
    const int32_t anmag = (an > 0)  ?  an  :  ((-an) & 0x1FFF);
    const int32_t anexp = g726_top_bit((uint32_t) anmag) - 5;
    const int32_t up = (anexp < 0)  ?  -anexp  :  0;
    const int32_t down = (anexp > 0)  ?  anexp  :  0;
    const int32_t anmant = (anmag == 0)  ?  32  :  g726_s16((anmag << up) >> down);
    const int32_t wanexp = anexp + ((srn >> 6) & 0xF) - 13;
    const int32_t wanmant = (anmant*(srn & 0x3F) + 0x30) >> 4;
    const int32_t l = (wanexp > 0)  ?  wanexp  :  0;
    const int32_t r = (wanexp < 0)  ?  -wanexp  :  0;
    const int32_t retval = (wanexp >= 0)  ?  (int32_t) (((uint32_t) wanmant << (l & 31)) & 0x7FFF)  :  (wanmant >> (r & 31));
    return ((an ^ srn) < 0)  ?  -retval  :  retval;
}

// step_size(), g726.c:271-288
G726_HD int32_t g726_step_size(const G726 &s)
{
    const int32_t y = s.yl >> 6;
    const int32_t dif = s.yu - y;
    const int32_t al = s.ap >> 2;
    // (dif*al) >> 6 towards zero for a negative dif: + 0x3F first; the shift of a negative value is arithmetic here
    const int32_t mixed = y + ((dif*al + ((dif < 0)  ?  0x3F  :  0)) >> 6);
    return (s.ap >= 256)  ?  s.yu  :  mixed;
}

// quantize(), g726.c:298-356.  tab: this rate's 112 words
template <typename TAB>
G726_HD int32_t g726_quantize(int32_t d, int32_t y, TAB tab, int32_t bps)
{
    // LOG
    const int32_t dqm = g726_s16(g726_abs(d));
    const int32_t e = g726_top_bit((uint32_t) (dqm >> 1)) + 1;
    const int32_t mant = ((dqm*128) >> (e & 31)) & 0x7F;
    const int32_t dl = g726_s16((e << 7) + mant);
    // SUBTB
    const int32_t dln = g726_s16(dl - g726_s16(y >> 2));
    // QUAN: the table ascends, so the early-exit search is the count of levels not above dln
    int32_t i = 0;
G726_UNROLL
    for (int k = 0;  k < 16;  k++)
        i += (dln >= tab[k])  ?  1  :  0;
    const int32_t top = (1 << bps) - 1;
    // a negative d: the one's complement of i; zero is no code where the number of states is odd (every rate but 16 kbit/s)
    return (d < 0)  ?  (top - i)  :  ((i == 0  &&  bps != 2)  ?  top  :  i);
}

// reconstruct(), g726.c:364-383
G726_HD int32_t g726_reconstruct(bool sign, int32_t dqln, int32_t y)
{
    const int32_t dql = g726_s16(dqln + (y >> 2));
    const int32_t dex = (dql >> 7) & 15;
    const int32_t dqt = 128 + (dql & 127);
    const int32_t dq = g726_s16((dqt << 7) >> ((14 - dex) & 31));
    const int32_t v = (dql < 0)  ?  0  :  dq;
    return sign  ?  g726_s16(v - 0x8000)  :  v;
}

// FLOAT A / FLOAT B of update(): a magnitude to 4-bit exponent, 6-bit mantissa
G726_HD int32_t g726_float(int32_t mag)
{
    const int32_t e = g726_top_bit((uint32_t) mag) + 1;
    return (e << 6) + ((mag << 6) >> (e & 31));
}

// update(), g726.c:389-621
G726_HD void g726_update(G726 &s, int32_t y, int32_t wi, int32_t fi, int32_t dq, int32_t sr, int32_t dqsez)
{
    const int32_t pk0 = (dqsez < 0)  ?  1  :  0;
    const int32_t mag = dq & 0x7FFF;
    // TRANS
    const int32_t ylint = g726_s16(s.yl >> 15);
    const int32_t ylfrac = (s.yl >> 10) & 0x1F;
    const int32_t thr = (ylint > 9)  ?  (31 << 10)  :  g726_s16((32 + ylfrac) << (ylint & 15));
    const int32_t dqthr = g726_s16((thr + (thr >> 1)) >> 1);
    const bool tr = (s.td != 0)  &&  (mag > dqthr);
    // FUNCTW, FILTD, LIMB, FILTE
    int32_t yu = g726_s16(y + ((wi - y) >> 5));
    yu = (yu < 544)  ?  544  :  ((yu > 5120)  ?  5120  :  yu);
    s.yu = yu;
    s.yl = (int32_t) ((uint32_t) s.yl + (uint32_t) yu + (uint32_t) ((-s.yl) >> 6));
    // UPA2, LIMC
    const int32_t pks1 = pk0 ^ s.pk[0];
    const bool moved = (dqsez != 0);
    int32_t a2p = g726_s16(s.a[1] - (s.a[1] >> 7));
    const int32_t fa1 = pks1  ?  s.a[0]  :  g726_s16(-s.a[0]);
    const int32_t a2q = g726_s16(a2p + ((fa1 < -8191)  ?  -0x100  :  ((fa1 > 8191)  ?  0xFF  :  (fa1 >> 5))));
    const bool flip = (pk0 ^ s.pk[1]) != 0;
    const int32_t lo = flip  ?  -12160  :  -12416;
    const int32_t hi = flip  ?  12416  :  12160;
    const int32_t a2r = (a2q <= lo)  ?  -12288  :  ((a2q >= hi)  ?  12288  :  g726_s16(a2q + (flip  ?  -0x80  :  0x80)));
    a2p = moved  ?  a2r  :  a2p;
    // UPA1, LIMD
    int32_t a1 = g726_s16(s.a[0] - (s.a[0] >> 8));
    a1 = moved  ?  g726_s16(a1 + (pks1  ?  -192  :  192))  :  a1;
    const int32_t a1ul = g726_s16(15360 - a2p);
    a1 = (a1 < -a1ul)  ?  -a1ul  :  ((a1 > a1ul)  ?  a1ul  :  a1);
    // TRIGB
    s.a[1] = tr  ?  0  :  a2p;
    s.a[0] = tr  ?  0  :  g726_s16(a1);
    // UPB: the leak is slower at 40 kbit/s
    const int32_t leak = (s.bps == 5)  ?  9  :  8;
G726_UNROLL
    for (int i = 0;  i < 6;  i++)
    {
        int32_t b = g726_s16(s.b[i] - (s.b[i] >> leak));
        b = mag  ?  g726_s16(b + (((dq ^ s.dq[i]) >= 0)  ?  128  :  -128))  :  b;
        s.b[i] = tr  ?  0  :  b;
    }
G726_UNROLL
    for (int i = 5;  i > 0;  i--)
        s.dq[i] = s.dq[i - 1];
    // FLOAT A
    const int32_t fa = (mag == 0)  ?  0x20  :  g726_float(mag);
    s.dq[0] = (dq >= 0)  ?  g726_s16(fa)  :  g726_s16(fa - 0x400);
    // FLOAT B: sr == -32768 has no magnitude an int16_t holds
    s.sr[1] = s.sr[0];
    const int32_t smag = g726_abs(sr);
    const int32_t fb = (sr == 0  ||  sr <= -32768)  ?  0x20  :  g726_float(smag);
    s.sr[0] = (sr >= 0)  ?  g726_s16(fb)  :  g726_s16(fb - 0x400);
    // DELAY A
    s.pk[1] = s.pk[0];
    s.pk[0] = pk0;
    // TONE
    s.td = (!tr  &&  a2p < -11776)  ?  1  :  0;
    // FILTA, FILTB
    s.dms = g726_s16(s.dms + ((g726_s16(fi) - s.dms) >> 5));
    s.dml = g726_s16(s.dml + ((g726_s16(fi*4) - s.dml) >> 7));
    // SUBTC, FILTC
    const bool fast = (y < 1536)  ||  (s.td != 0)  ||  (g726_abs(s.dms*4 - s.dml) >= (s.dml >> 3));
    const int32_t ap = g726_s16(s.ap + (((fast  ?  0x200  :  0) - s.ap) >> 4));
    s.ap = tr  ?  256  :  ap;
}

// What the encoder and the decoder of a rate share: the eight independent fmult()s, se and y
struct G726Est
{
    int32_t sezi, se, y;
};

G726_HD G726Est g726_estimate(const G726 &s)
{
    // predictor_zero() and predictor_pole(), g726.c:245-265
    const int32_t z0 = g726_fmult(s.b[0] >> 2, s.dq[0]);
    const int32_t z1 = g726_fmult(s.b[1] >> 2, s.dq[1]);
    const int32_t z2 = g726_fmult(s.b[2] >> 2, s.dq[2]);
    const int32_t z3 = g726_fmult(s.b[3] >> 2, s.dq[3]);
    const int32_t z4 = g726_fmult(s.b[4] >> 2, s.dq[4]);
    const int32_t z5 = g726_fmult(s.b[5] >> 2, s.dq[5]);
    const int32_t p1 = g726_fmult(s.a[1] >> 2, s.sr[1]);
    const int32_t p0 = g726_fmult(s.a[0] >> 2, s.sr[0]);
    G726Est e;
    e.sezi = g726_s16((z0 + z1) + (z2 + z3) + (z4 + z5));
    const int32_t sei = g726_s16(e.sezi + g726_s16(p1 + p0));
    e.se = sei >> 1;
    e.y = g726_step_size(s);
    return e;
}

// the tail of all eight: dq from the code, sr, dqsez, update().  Returns sr.
template <typename TAB>
G726_HD int32_t g726_advance(G726 &s, TAB tab, const G726Est &e, int32_t code)
{
    const int32_t dq = g726_reconstruct((code >> (s.bps - 1)) & 1, tab[16 + code], e.y);
    const int32_t srmask = (s.bps == 5)  ?  0x7FFF  :  0x3FFF;
    const int32_t sr = g726_s16((dq < 0)  ?  (e.se - (dq & srmask))  :  (e.se + dq));
    const int32_t dqsez = g726_s16(sr + (e.sezi >> 1) - e.se);
    g726_update(s, e.y, tab[48 + code], tab[80 + code], dq, sr, dqsez);
    return sr;
}

// g726_{16,24,32,40}_encoder(), g726.c:730-999: a 14-bit linear sample in, a code out.  table: all kG726TabWords
template <typename TAB>
G726_HD int32_t g726_encode_sample(G726 &s, TAB table, int32_t amp14)
{
    const auto tab = table + (s.bps - 2)*kG726TabStride;
    const G726Est e = g726_estimate(s);
    const int32_t d = g726_s16(amp14 - e.se);
    const int32_t code = g726_quantize(d, e.y, tab, s.bps);
    (void) g726_advance(s, tab, e, code);
    return code;
}

// the sample the encoder takes from one element of a caller's row, g726.c:1121-1134
G726_HD int32_t g726_linearize(int32_t coding, int32_t raw)
{
    const int32_t lin = g726_s16(raw);
    const int32_t u = g726_ulaw_to_linear(raw & 0xFF);
    const int32_t a = g726_alaw_to_linear(raw & 0xFF);
    return ((coding == kG726Ulaw)  ?  u  :  ((coding == kG726Alaw)  ?  a  :  lin)) >> 2;
}

// tandem_adjust_alaw() / tandem_adjust_ulaw(), g726.c:624-725: the G.711 code that encodes back to the code just decoded
template <typename TAB>
G726_HD int32_t g726_tandem(bool alaw, int32_t sr, int32_t se, int32_t y, int32_t code, TAB tab, int32_t bps)
{
    const int32_t sign = 1 << (bps - 1);
    int32_t sp;
    int32_t lin;
    if (alaw)
    {
        const int32_t v = (sr <= -32768)  ?  -1  :  sr;
        sp = g726_linear_to_alaw((v >> 1)*8);
        lin = g726_alaw_to_linear(sp);
    }
    else
    {
        const int32_t v = (sr <= -32768)  ?  0  :  sr;
        sp = g726_linear_to_ulaw(v*4);
        lin = g726_ulaw_to_linear(sp);
    }
    const int32_t dx = g726_s16((lin >> 2) - se);
    const int32_t id = g726_quantize(dx, y, tab, bps);
    const bool lower = (id ^ sign) > (code ^ sign);
    const bool neg = (sp & 0x80) != 0;
    int32_t sd;
    if (alaw)
    {
        const int32_t x = sp ^ 0x55;
        const int32_t dn = neg  ?  ((sp == 0xD5)  ?  0x55  :  ((x - 1) ^ 0x55))  :  ((sp == 0x2A)  ?  0x2A  :  ((x + 1) ^ 0x55));
        const int32_t up = neg  ?  ((sp == 0xAA)  ?  0xAA  :  ((x + 1) ^ 0x55))  :  ((sp == 0x55)  ?  0xD5  :  ((x - 1) ^ 0x55));
        sd = lower  ?  dn  :  up;
    }
    else
    {
        const int32_t dn = neg  ?  ((sp == 0xFF)  ?  0x7E  :  (sp + 1))  :  ((sp == 0x00)  ?  0x00  :  (sp - 1));
        const int32_t up = neg  ?  ((sp == 0x80)  ?  0x80  :  (sp - 1))  :  ((sp == 0x7F)  ?  0xFE  :  (sp + 1));
        sd = lower  ?  dn  :  up;
    }
    return ((id == code)  ?  sp  :  sd) & 0xFF;
}

// g726_{16,24,32,40}_decoder(), g726.c:767-1041: a code in (its bits above the width are dropped), one element of the
// caller's row out: an int16_t, or a G.711 byte after the tandem adjustment
template <typename TAB>
G726_HD int32_t g726_decode_code(G726 &s, TAB table, int32_t code)
{
    const auto tab = table + (s.bps - 2)*kG726TabStride;
    code &= (1 << s.bps) - 1;
    const G726Est e = g726_estimate(s);
    const int32_t sr = g726_advance(s, tab, e, code);
    int32_t out = g726_s16(sr*4);
    // the lanes of a wave may hold all three codings: a coding no lane has costs nothing
    if (G726_ANY(s.coding == kG726Alaw))
    {
        const int32_t t = g726_tandem(true, sr, e.se, e.y, code, tab, s.bps);
        out = (s.coding == kG726Alaw)  ?  t  :  out;
    }
    if (G726_ANY(s.coding == kG726Ulaw))
    {
        const int32_t t = g726_tandem(false, sr, e.se, e.y, code, tab, s.bps);
        out = (s.coding == kG726Ulaw)  ?  t  :  out;
    }
    return out;
}

// ---- packing, g726.c:1056-1096 and :1136-1168 -------------------------------------------------------------------------

// the encoder's side: one code in; true: *byte comes out
G726_HD bool g726_pack(G726 &s, int32_t code, int32_t *byte)
{
    const bool left = (s.packing == kG726PackLeft);
    const bool none = (s.packing == kG726PackNone);
    const uint32_t ucode = (uint32_t) code;
    const uint32_t bs = left  ?  ((s.bitstream << s.bps) | ucode)  :  (s.bitstream | (ucode << (s.residue & 31)));
    const int32_t res = s.residue + s.bps;
    const bool full = (res >= 8);
    const int32_t after = full  ?  (res - 8)  :  res;
    const uint32_t out = left  ?  (bs >> (after & 31))  :  bs;
    *byte = (int32_t) ((none  ?  ucode  :  out) & 0xFF);
    s.bitstream = none  ?  s.bitstream  :  ((full  &&  !left)  ?  (bs >> 8)  :  bs);
    s.residue = none  ?  s.residue  :  after;
    return none  ||  full;
}

// the decoder's side: does the next code need another byte first
G726_HD bool g726_unpack_needs(const G726 &s)
{
    return s.packing == kG726PackNone  ||  s.residue < s.bps;
}

// ... and the code (not yet masked where the channel is unpacked); `byte` is taken only if g726_unpack_needs()
G726_HD int32_t g726_unpack(G726 &s, int32_t byte)
{
    const bool left = (s.packing == kG726PackLeft);
    const bool none = (s.packing == kG726PackNone);
    const bool need = s.residue < s.bps;
    const uint32_t ub = (uint32_t) byte & 0xFF;
    const uint32_t mask = (1u << s.bps) - 1;
    const uint32_t in = left  ?  ((s.bitstream << 8) | ub)  :  (s.bitstream | (ub << (s.residue & 31)));
    const uint32_t bs = need  ?  in  :  s.bitstream;
    const int32_t res = s.residue + (need  ?  8  :  0) - s.bps;
    const uint32_t code = left  ?  ((bs >> (res & 31)) & mask)  :  (bs & mask);
    s.bitstream = none  ?  s.bitstream  :  (left  ?  bs  :  (bs >> s.bps));
    s.residue = none  ?  s.residue  :  res;
    return (int32_t) (none  ?  ub  :  code);
}

// samples g726_decode() makes of `bytes` bytes: every whole code in the residue and the bytes together
G726_HD int32_t g726_decode_count(const G726 &s, int32_t bytes)
{
    return (s.packing == kG726PackNone)  ?  bytes  :  ((s.residue + 8*bytes)/s.bps);
}

// Bytes a row must hold for `samples` samples encoded on the worst channel (40 kbit/s with 7 bits of residue), and the
// samples for `bytes` bytes decoded (16 kbit/s with one bit of residue); an unpacked channel is one for one either way.
static inline long long g726_encode_capacity(int bps, int packing, long long samples)
{
    return (packing == kG726PackNone)  ?  samples  :  ((samples*bps + 7)/8);
}

static inline long long g726_decode_capacity(int bps, int packing, long long bytes)
{
    return (packing == kG726PackNone)  ?  bytes  :  ((8*bytes + bps - 1)/bps);
}

G726_HD void g726_load(G726 &s, const int32_t *st, size_t n)
{
    s.yl = st[G7_YL*n];
    s.yu = st[G7_YU*n];
    s.dms = st[G7_DMS*n];
    s.dml = st[G7_DML*n];
    s.ap = st[G7_AP*n];
    s.a[0] = st[G7_A0*n];
    s.a[1] = st[G7_A1*n];
G726_UNROLL
    for (int i = 0;  i < 6;  i++)
    {
        s.b[i] = st[(G7_B0 + i)*n];
        s.dq[i] = st[(G7_DQ0 + i)*n];
    }
    s.pk[0] = st[G7_PK0*n];
    s.pk[1] = st[G7_PK1*n];
    s.sr[0] = st[G7_SR0*n];
    s.sr[1] = st[G7_SR1*n];
    s.td = st[G7_TD*n];
    s.bitstream = (uint32_t) st[G7_BITSTREAM*n];
    s.residue = st[G7_RESIDUE*n];
    s.coding = st[G7_CODING*n];
    s.bps = st[G7_BPS*n];
    s.packing = st[G7_PACKING*n];
}

G726_HD void g726_store(const G726 &s, int32_t *st, size_t n)
{
    st[G7_YL*n] = s.yl;
    st[G7_YU*n] = s.yu;
    st[G7_DMS*n] = s.dms;
    st[G7_DML*n] = s.dml;
    st[G7_AP*n] = s.ap;
    st[G7_A0*n] = s.a[0];
    st[G7_A1*n] = s.a[1];
G726_UNROLL
    for (int i = 0;  i < 6;  i++)
    {
        st[(G7_B0 + i)*n] = s.b[i];
        st[(G7_DQ0 + i)*n] = s.dq[i];
    }
    st[G7_PK0*n] = s.pk[0];
    st[G7_PK1*n] = s.pk[1];
    st[G7_SR0*n] = s.sr[0];
    st[G7_SR1*n] = s.sr[1];
    st[G7_TD*n] = s.td;
    st[G7_BITSTREAM*n] = (int32_t) s.bitstream;
    st[G7_RESIDUE*n] = s.residue;
}

// ---- the kernels: codec_kernel<G726Codec, ENCODE> (codec_rows.hpp) ------------------------------------------------------

#if defined(__HIPCC__)  &&  !defined(SPG_G726_STEP_FUNCTIONS_ONLY)

// Eight samples between two advances of the window: 16 bytes of linear PCM in, or 16 out.
struct G726Codec
{
    typedef G726 State;
    static constexpr int kTabWords = kG726TabWords;
    static constexpr int kGroup = 8;
    static constexpr int kWidest = 2;

    static __device__ __forceinline__ const int32_t *table() { return kG726TabDev; }
    static __device__ __forceinline__ void load(G726 &s, const int32_t *st, size_t n) { g726_load(s, st, n); }
    static __device__ __forceinline__ void store(const G726 &s, int32_t *st, size_t n) { g726_store(s, st, n); }
    static __device__ __forceinline__ int pcm_bytes(int el) { return el; }

    // bytes of an element of the PCM row
    static __device__ __forceinline__ int unit(const G726 &s)
    {
        return (s.coding == kG726Linear)  ?  2  :  1;
    }

    // (a decoder's count follows from the residue in its state: never past the row, whatever a caller has set there)
    template <bool ENCODE>
    static __device__ __forceinline__ int todo(const G726 &s, int el, int mylen, long long out_stride)
    {
        return ENCODE  ?  mylen  :  (int) min((long long) g726_decode_count(s, mylen), out_stride/el);
    }

    template <bool ENCODE>
    static __device__ __forceinline__ int32_t take(const G726 &s, int el)
    {
        return ENCODE  ?  el  :  (g726_unpack_needs(s)  ?  1  :  0);
    }

    template <bool ENCODE>
    static __device__ __forceinline__ RowPush step(G726 &s, const int32_t *table, int el, uint32_t raw)
    {
        if (ENCODE)
        {
            const int32_t code = g726_encode_sample(s, table, g726_linearize(s.coding, (int32_t) raw));
            int32_t byte;
            const bool full = g726_pack(s, code, &byte);
            return {(uint32_t) byte, full  ?  1  :  0};
        }
        else
        {
            const int32_t code = g726_unpack(s, (int32_t) raw);
            return {(uint32_t) g726_decode_code(s, table, code), el};
        }
    }
};

#endif  // __HIPCC__

}   // namespace spg
