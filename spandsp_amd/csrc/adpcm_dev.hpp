// adpcm_dev.hpp -- the two small ADPCM families as codec banks: IMA ADPCM in its three variants (IMA4, and the RTP payloads
// DVI4 and VDVI; the shape of spandsp's ima_adpcm.c) and OKI / Dialogic "VOX" ADPCM at 32 and 24 kbit/s (oki_adpcm.c, the
// latter with its 6 kHz <-> 8 kHz rate converter).  One lane per channel; every channel has a configuration of its own, and
// the lanes of a wave may hold all of them.
//
// The per-item functions and the per-call bodies are __host__ __device__ templates over a reader, a writer and (OKI) a
// history, and the file compiles for the host with no HIP (tests/c_callers/adpcm_host.cpp runs them one lane at a time
// under ASan and UBSan).  The kernels at the end are HIP only.  They are kernels of their own, not codec_kernel<>
// (codec_rows.hpp): an item here takes 0, 1 or 4 bytes and makes 0 .. 4, and a VDVI decoder does not know its item count
// before it has read its bits, so each lane runs its own loop over its row.  A lane reads its row in aligned 8-byte words,
// one word ahead of the one in use, and writes 8-byte words; what codec_host.hpp says of rows (16-byte alignment, the last
// chunk whole) covers both.
//
// One table.  The 89 step sizes of IMA sit in LDS; OKI's 49 are entries 8 .. 56 of them.  The 81 taps of OKI's rate
// converter sit beside them: the lanes of a wave index both at different places.
//
// IMA state words, in the order of the reference's fields: variant, chunk_size, last, step_index, ima_byte, bits.
// OKI state words: bit_rate, last, step_index, oki_byte, history[32], ptr, mark, phase (39).  On the device the ring of a
// 24 kbit/s lane lives in LDS for the length of a call (a column of 32 int16_t per lane); the 32 kbit/s lanes neither
// load nor store it.
//
// Narrowing.  The 24 kbit/s paths convert a binary32 sum to int16_t, and the sum does leave the int16_t range (the
// interpolator's per-phase L1 gain is up to 2.18, times 4.0f).  The C conversion is then undefined; this code does what the
// reference's x86-64 build does, written out: to int32_t truncating toward zero, then the low 16 bits (adpcm_narrow()).
// The sum is formed in the reference's tap order, every product and sum rounded on its own (the library and the host
// program are built with -ffp-contract=off).
//
// Where the reference reads outside its arguments, this code does not:
//   a length of 0                    the reference's IMA4 and OKI 24k encoders read amp[0], its DVI4/VDVI encoders emit a bare
//                                    header; here a call of length 0 changes nothing and counts 0 (the codec banks' rule)
//   an IMA decode call with chunk_size == 0 and fewer than 4 bytes
//                                    the reference reads the header beyond the data; here the call produces nothing and
//                                    leaves the state alone
//   a header step_index above 88     the reference reads past its table; here it is taken as 88

#pragma once

#include <stddef.h>
#include <stdint.h>

#include "codec_rows.hpp"

#ifdef __HIPCC__
#define ADPCM_HD __host__ __device__ __forceinline__
#else
#define ADPCM_HD static inline
#endif

namespace spg
{

enum { IM_VARIANT = 0, IM_CHUNK, IM_LAST, IM_STEP, IM_BYTE, IM_BITS, kImaWords };
enum { kImaIma4 = 0, kImaDvi4 = 1, kImaVdvi = 2 };         // IMA_ADPCM_*

enum { OK_RATE = 0, OK_LAST, OK_STEP, OK_BYTE, OK_HIST, OK_PTR = OK_HIST + 32, OK_MARK, OK_PHASE, kOkiWords };

constexpr int kImaStepMax = 88;
constexpr int kOkiStepMax = 48;
constexpr int kOkiStepBase = 8;         // OKI's step_size[i] is IMA's step_size[8 + i]
constexpr int kAdpcmStepWords = 128;    // 89 used
constexpr int kAdpcmCoefWords = 128;    // 81 used

// step_size[], ima_adpcm.c:121-135 (oki_adpcm.c:50-59 is entries 8 .. 56)
#define ADPCM_STEP_INIT                                                                                                        \
{                                                                                                                              \
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, \
    157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, \
    1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493,   \
    10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767                                  \
}

// cutoff_coeffs[], oki_adpcm.c:68-151: symmetric, so written as its first 41 taps and mirrored below
#define ADPCM_HALF_INIT                                                                                                        \
{                                                                                                                              \
    -3.648392e-4f, 5.062391e-4f, 1.206247e-3f, 1.804452e-3f, 1.691750e-3f, 4.083405e-4f, -1.931085e-3f, -4.452107e-3f,         \
    -5.794821e-3f, -4.778489e-3f, -1.161266e-3f, 3.928504e-3f, 8.259786e-3f, 9.500425e-3f, 6.512800e-3f, 2.227856e-4f,         \
    -6.531275e-3f, -1.026843e-2f, -8.718062e-3f, -2.280487e-3f, 5.817733e-3f, 1.096777e-2f, 9.634404e-3f, 1.569301e-3f,        \
    -9.522632e-3f, -1.748273e-2f, -1.684408e-2f, -6.100054e-3f, 1.071206e-2f, 2.525209e-2f, 2.871779e-2f, 1.664411e-2f,        \
    -7.706268e-3f, -3.331083e-2f, -4.521249e-2f, -3.085962e-2f, 1.373653e-2f, 8.089593e-2f, 1.529060e-1f, 2.080487e-1f,        \
    2.286834e-1f                                                                                                               \
}

#if defined(__HIPCC__)
__device__ const int32_t kAdpcmStepDev[kAdpcmStepWords] = ADPCM_STEP_INIT;
__device__ const float kAdpcmHalfDev[41] = ADPCM_HALF_INIT;
#endif
static const int32_t kAdpcmStepHost[kAdpcmStepWords] = ADPCM_STEP_INIT;
static const float kAdpcmHalfHost[41] = ADPCM_HALF_INIT;

// tap l of the 81
ADPCM_HD int adpcm_half_index(int l)
{
    return (l <= 40)  ?  l  :  (80 - l);
}

ADPCM_HD int32_t adpcm_s16(int32_t x)
{
    return (int32_t) (int16_t) (uint16_t) (uint32_t) x;
}

// saturate16(), spandsp/saturated.h
ADPCM_HD int32_t adpcm_sat16(int32_t x)
{
    return (x > 32767)  ?  32767  :  ((x < -32768)  ?  -32768  :  x);
}

// (int16_t) of a binary32 value as the reference's x86-64 build does it: see "Narrowing" above.  |v| is far inside int32_t.
ADPCM_HD int32_t adpcm_narrow(float v)
{
    const int32_t t = (int32_t) v;
    return adpcm_s16(t);
}

// step_adjustment[], both families: -1, -1, -1, -1, 2, 4, 6, 8
ADPCM_HD int32_t adpcm_step_adjust(int32_t code)
{
    return (code & 4)  ?  (2*((code & 3) + 1))  :  -1;
}

// ---- IMA ----------------------------------------------------------------------------------------------------------------

struct Ima
{
    int32_t variant, chunk, last, step, byte, bits;
};

// ima_adpcm_init(), ima_adpcm.c:280-294.  false: a variant outside the three (the reference takes any, and then codes nothing)
static inline bool ima_init_words(int32_t w[kImaWords], int variant, int chunk_size)
{
    if (variant < kImaIma4  ||  variant > kImaVdvi)
        return false;
    for (int i = 0;  i < kImaWords;  i++)
        w[i] = 0;
    w[IM_VARIANT] = variant;
    w[IM_CHUNK] = chunk_size;
    return true;
}

// words a channel can hold: what init and the calls leave, and nothing that would index outside a table
static inline bool ima_words_ok(const int32_t w[kImaWords])
{
    return w[IM_VARIANT] >= kImaIma4  &&  w[IM_VARIANT] <= kImaVdvi  &&  w[IM_LAST] >= -32768  &&  w[IM_LAST] <= 32767
        &&  w[IM_STEP] >= 0  &&  w[IM_STEP] <= kImaStepMax  &&  w[IM_BYTE] >= 0  &&  w[IM_BYTE] <= 0xFFFF  &&  w[IM_BITS] >= 0;
}

// decode(), ima_adpcm.c:191-221
template <typename TAB>
ADPCM_HD int32_t ima_decode_code(Ima &s, TAB tab, int32_t code)
{
    const int32_t ss = tab[s.step];
    int32_t e = ss >> 3;
    e += (code & 1)  ?  (ss >> 2)  :  0;
    e += (code & 2)  ?  (ss >> 1)  :  0;
    e += (code & 4)  ?  ss  :  0;
    e = (code & 8)  ?  -e  :  e;
    const int32_t linear = adpcm_sat16(s.last + e);
    s.last = linear;
    const int32_t idx = s.step + adpcm_step_adjust(code);
    s.step = (idx < 0)  ?  0  :  ((idx > kImaStepMax)  ?  kImaStepMax  :  idx);
    return linear;
}

// encode(), ima_adpcm.c:224-277
template <typename TAB>
ADPCM_HD int32_t ima_encode_sample(Ima &s, TAB tab, int32_t linear)
{
    int32_t ss = tab[s.step];
    const int32_t initial_e = linear - s.last;
    int32_t e = initial_e;
    int32_t diff = ss >> 3;
    int32_t code = 0;
    if (e < 0)
    {
        code = 8;
        e = -e;
    }
    if (e >= ss)
    {
        code |= 4;
        e -= ss;
    }
    ss >>= 1;
    if (e >= ss)
    {
        code |= 2;
        e -= ss;
    }
    ss >>= 1;
    if (e >= ss)
    {
        code |= 1;
        e -= ss;
    }
    diff = (initial_e < 0)  ?  -(diff - initial_e - e)  :  (diff + initial_e - e);
    s.last = adpcm_sat16(diff + s.last);
    const int32_t idx = s.step + adpcm_step_adjust(code);
    s.step = (idx < 0)  ?  0  :  ((idx > kImaStepMax)  ?  kImaStepMax  :  idx);
    return code;
}

// vdvi_encode[], ima_adpcm.c:142-164: the bits of code c depend on c & 7 alone (2, 3, 4, 5, 6, 7, 8, 8), and its pattern is a
// byte of one of two 64-bit words.  vdvi_decode[] (:166-189) is the same table seen from the top of a 16-bit word: pattern
// << (16 - bits) under a mask of `bits` ones.
ADPCM_HD int32_t vdvi_bits(int32_t c)
{
    return (int32_t) ((0x88765432u >> (4*(c & 7))) & 0xF);
}

ADPCM_HD int32_t vdvi_pattern(int32_t c)
{
    const uint64_t t = (c & 8)  ?  0xFFFD7D3D1D0D0302ull  :  0xFEFC7C3C1C0C0200ull;
    return (int32_t) ((t >> (8*(c & 7))) & 0xFF);
}

// the code at the top of the 16 bits of `word`.  The sixteen patterns are a complete prefix code (their Kraft sum is 1), so
// exactly one matches and the reference's search order (:378-389) does not matter.
ADPCM_HD int32_t vdvi_match(uint32_t word)
{
    int32_t found = 0;
    for (int32_t c = 0;  c < 16;  c++)
    {
        const int32_t n = vdvi_bits(c);
        const uint32_t mask = (0xFFFFu << (16 - n)) & 0xFFFFu;
        const uint32_t want = (uint32_t) vdvi_pattern(c) << (16 - n);
        found = ((word & mask) == want)  ?  c  :  found;
    }
    return found;
}

// ima_adpcm_encode(), ima_adpcm.c:426-508.  in: int16_t samples; out: bytes.
template <typename TAB, class In, class Out>
ADPCM_HD void ima_encode_call(Ima &s, TAB tab, In &in, Out &out, int len)
{
    if (len <= 0)
        return;         // nothing brought: nothing read, written or changed
    int i = 0;
    if (s.chunk == 0)
    {
        if (s.variant == kImaIma4)
        {
            const int32_t a0 = in.s16();
            out.put8(a0 & 0xFF);
            out.put8((a0 >> 8) & 0xFF);
            s.last = a0;
            s.bits = 0;
            i = 1;
        }
        else
        {
            out.put8((s.last >> 8) & 0xFF);
            out.put8(s.last & 0xFF);
        }
        out.put8(s.step & 0xFF);
        out.put8(0);
    }
    if (s.variant == kImaVdvi)
    {
        s.bits = 0;
        for (  ;  i < len;  i++)
        {
            const int32_t code = ima_encode_sample(s, tab, in.s16());
            const int32_t n = vdvi_bits(code);
            s.byte = ((s.byte << n) | vdvi_pattern(code)) & 0xFFFF;
            s.bits += n;
            if (s.bits >= 8)
            {
                s.bits -= 8;
                out.put8((s.byte >> s.bits) & 0xFF);
            }
        }
        if (s.bits)
            out.put8((((s.byte << 8) | 0xFF) >> s.bits) & 0xFF);
    }
    else
    {
        const bool low_first = (s.variant == kImaIma4);
        for (  ;  i < len;  i++)
        {
            const int32_t code = ima_encode_sample(s, tab, in.s16());
            s.byte = (low_first  ?  ((s.byte >> 4) | (code << 4))  :  ((s.byte << 4) | code)) & 0xFF;
            if ((s.bits & 1))
                out.put8(s.byte);
            s.bits = (int32_t) ((uint32_t) s.bits + 1u);
        }
    }
}

// ima_adpcm_decode(), ima_adpcm.c:310-424.  in: bytes; out: int16_t samples.
template <typename TAB, class In, class Out>
ADPCM_HD void ima_decode_call(Ima &s, TAB tab, In &in, Out &out, int bytes)
{
    if (bytes <= 0)
        return;         // nothing brought: nothing read, written or changed
    int i = 0;
    if (s.chunk == 0)
    {
        if (bytes < 4)
            return;
        const int32_t b0 = in.u8();
        const int32_t b1 = in.u8();
        const int32_t b2 = in.u8();
        (void) in.u8();
        if (s.variant == kImaIma4)
        {
            s.last = adpcm_s16((b1 << 8) | b0);
            out.put16(s.last);
        }
        else
        {
            s.last = adpcm_s16((b0 << 8) | b1);
        }
        s.step = (b2 > kImaStepMax)  ?  kImaStepMax  :  b2;
        i = 4;
    }
    if (s.variant == kImaVdvi)
    {
        uint32_t word = 0;              // the reference's uint16_t code
        s.bits = 0;
        for (;;)
        {
            if (s.bits <= 8)
            {
                if (i >= bytes)
                    break;
                word |= (uint32_t) in.u8() << (8 - s.bits);
                i++;
                s.bits += 8;
            }
            const int32_t c = vdvi_match(word);
            out.put16(ima_decode_code(s, tab, c));
            word = (word << vdvi_bits(c)) & 0xFFFFu;
            s.bits -= vdvi_bits(c);
        }
        // what is left of the last octet
        while (s.bits > 0)
        {
            const int32_t c = vdvi_match(word);
            if (vdvi_bits(c) > s.bits)
                break;
            out.put16(ima_decode_code(s, tab, c));
            word = (word << vdvi_bits(c)) & 0xFFFFu;
            s.bits -= vdvi_bits(c);
        }
    }
    else
    {
        const bool low_first = (s.variant == kImaIma4);
        for (  ;  i < bytes;  i++)
        {
            const int32_t b = in.u8();
            const int32_t lo = b & 0xF;
            const int32_t hi = (b >> 4) & 0xF;
            out.put16(ima_decode_code(s, tab, low_first  ?  lo  :  hi));
            out.put16(ima_decode_code(s, tab, low_first  ?  hi  :  lo));
        }
    }
}

// Bytes one call of `samples` >= 1 samples can make, from ima_encode_call():
//   the header is 4 bytes where chunk_size == 0;
//   IMA4 / DVI4 put a byte out at every second code, and the parity in `bits` may stand at odd when the call begins: (codes + 1)/2
//   bytes, where IMA4 under a header codes samples - 1 samples from an even parity: (samples - 1)/2;
//   VDVI starts every call at bits == 0 and a code is 8 bits at the most, so the whole octets and the pad octet together are
//   ceil(bits/8) <= samples: a pad octet only follows where some code was shorter than 8.
static inline long long ima_encode_capacity(int variant, bool header, long long samples)
{
    if (samples <= 0)
        return 0;
    if (variant == kImaVdvi)
        return (header  ?  4  :  0) + samples;
    if (variant == kImaIma4  &&  header)
        return 4 + (samples - 1)/2;
    return (header  ?  4  :  0) + (samples + 1)/2;
}

// Samples one call of `bytes` >= 1 bytes can make, from ima_decode_call(): two a byte behind the header (IMA4's header is a
// sample itself); VDVI's shortest code is 2 bits and the tail loop uses up the last octet, so 4 a byte.
static inline long long ima_decode_capacity(int variant, bool header, long long bytes)
{
    const long long body = header  ?  (bytes - 4)  :  bytes;
    if (bytes <= 0  ||  body < 0)
        return 0;
    if (variant == kImaVdvi)
        return 4*body;
    return 2*body + ((variant == kImaIma4  &&  header)  ?  1  :  0);
}

// ---- OKI ----------------------------------------------------------------------------------------------------------------

// (the history is not in here: a call's body takes it as an object with get(i) and set(i, v), i = 0 .. 31)
struct Oki
{
    int32_t rate, last, step, byte, ptr, mark, phase;
};

// oki_adpcm_init(), oki_adpcm.c:244-257.  false: a rate it refuses
static inline bool oki_init_words(int32_t w[kOkiWords], int bit_rate)
{
    if (bit_rate != 32000  &&  bit_rate != 24000)
        return false;
    for (int i = 0;  i < kOkiWords;  i++)
        w[i] = 0;
    w[OK_RATE] = bit_rate;
    return true;
}

static inline bool oki_words_ok(const int32_t w[kOkiWords])
{
    if ((w[OK_RATE] != 32000  &&  w[OK_RATE] != 24000)  ||  w[OK_LAST] < -2048  ||  w[OK_LAST] > 2047  ||  w[OK_STEP] < 0
        ||  w[OK_STEP] > kOkiStepMax  ||  w[OK_BYTE] < 0  ||  w[OK_BYTE] > 0xFF  ||  w[OK_PTR] < 0  ||  w[OK_PTR] > 31  ||  w[OK_MARK] < 0
        ||  w[OK_PHASE] < 0  ||  w[OK_PHASE] > 3)
        return false;
    for (int i = 0;  i < 32;  i++)
    {
        if (w[OK_HIST + i] < -32768  ||  w[OK_HIST + i] > 32767)
            return false;
    }
    return true;
}

// decode(), oki_adpcm.c:153-203: a 12-bit value
template <typename TAB>
ADPCM_HD int32_t oki_decode_code(Oki &s, TAB tab, int32_t code)
{
    const int32_t ss = tab[kOkiStepBase + s.step];
    int32_t d = ss >> 3;
    d += (code & 1)  ?  (ss >> 2)  :  0;
    d += (code & 2)  ?  (ss >> 1)  :  0;
    d += (code & 4)  ?  ss  :  0;
    d = (code & 8)  ?  -d  :  d;
    int32_t linear = s.last + d;
    linear = (linear > 2047)  ?  2047  :  ((linear < -2048)  ?  -2048  :  linear);
    s.last = linear;
    const int32_t idx = s.step + adpcm_step_adjust(code);
    s.step = (idx < 0)  ?  0  :  ((idx > kOkiStepMax)  ?  kOkiStepMax  :  idx);
    return linear;
}

// encode(), oki_adpcm.c:206-241.  linear: an int16_t value
template <typename TAB>
ADPCM_HD int32_t oki_encode_sample(Oki &s, TAB tab, int32_t linear)
{
    const int32_t ss = tab[kOkiStepBase + s.step];
    int32_t d = (linear >> 4) - s.last;
    int32_t code = 0;
    if (d < 0)
    {
        code = 8;
        d = -d;
    }
    if (d >= ss)
    {
        code |= 4;
        d -= ss;
    }
    if (d >= (ss >> 1))
    {
        code |= 2;
        d -= (ss >> 1);
    }
    if (d >= (ss >> 2))
        code |= 1;
    (void) oki_decode_code(s, tab, code);
    return code;
}

// The sum over every STEP-th tap from tap l down, against the history from `newest` backwards (oki_adpcm.c:311-313, :366-369):
// the reference's loop runs while l >= 0, which is COUNT rounds or one fewer (27 always for the encoder's l = 80 - phase by
// 3; 20, or 21 at phase 3, for the decoder's l = 77 + phase by 4).  Written with a fixed count and the last round under a
// condition, so that the loads of all taps can be issued ahead of the chain of sums; the sums are the same ones in the same order.
template <int STEP, int COUNT, typename COEF, class Hist>
ADPCM_HD float oki_taps(COEF half, const Hist &h, int l, int newest)
{
    float z = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
_Pragma("unroll")
#endif
    for (int k = 0;  k < COUNT;  k++)
    {
        const int tap = l - STEP*k;
        const int at = (tap >= 0)  ?  tap  :  0;
        const float sum = z + half[adpcm_half_index(at)]*(float) h.get((newest - k) & 31);
        z = (tap >= 0)  ?  sum  :  z;
    }
    return z;
}

// oki_adpcm_encode(), oki_adpcm.c:326-384.  in: int16_t samples; out: bytes.
template <typename TAB, typename COEF, class Hist, class In, class Out>
ADPCM_HD void oki_encode_call(Oki &s, TAB tab, COEF half, Hist &h, In &in, Out &out, int len)
{
    if (len <= 0)
        return;         // nothing brought: nothing read, written or changed
    if (s.rate == 32000)
    {
        for (int n = 0;  n < len;  n++)
        {
            s.byte = ((s.byte << 4) | oki_encode_sample(s, tab, in.s16())) & 0xFF;
            if ((s.mark & 1))
                out.put8(s.byte);
            s.mark = (int32_t) ((uint32_t) s.mark + 1u);
        }
        return;
    }
    int n = 0;
    for (;;)
    {
        // 8k to 6k samples/second: every fourth sample goes into the history alone
        if (s.phase > 2)
        {
            h.set(s.ptr, in.s16());
            s.ptr = (s.ptr + 1) & 31;
            s.phase = 0;
            if (++n >= len)
                break;
        }
        h.set(s.ptr, in.s16());
        s.ptr = (s.ptr + 1) & 31;
        const float z = oki_taps<3, 27>(half, h, 80 - s.phase, s.ptr - 1);
        s.byte = ((s.byte << 4) | oki_encode_sample(s, tab, adpcm_narrow(z*3.0f))) & 0xFF;
        if ((s.mark & 1))
            out.put8(s.byte);
        s.mark = (int32_t) ((uint32_t) s.mark + 1u);
        s.phase++;
        if (++n >= len)
            break;
    }
}

// oki_adpcm_decode(), oki_adpcm.c:273-323.  in: bytes; out: int16_t samples.
template <typename TAB, typename COEF, class Hist, class In, class Out>
ADPCM_HD void oki_decode_call(Oki &s, TAB tab, COEF half, Hist &h, In &in, Out &out, int bytes)
{
    if (bytes <= 0)
        return;         // nothing brought: nothing read, written or changed
    if (s.rate == 32000)
    {
        for (int i = 0;  i < bytes;  i++)
        {
            const int32_t b = in.u8();
            out.put16(oki_decode_code(s, tab, (b >> 4) & 0xF)*16);
            out.put16(oki_decode_code(s, tab, b & 0xF)*16);
        }
        return;
    }
    int n = 0;          // the nibble counter restarts with each call
    int32_t b = 0;
    for (int i = 0;  i < bytes;  )
    {
        // 6k to 8k samples/second: three phases of four take a nibble
        if (s.phase)
        {
            int32_t code;
            if ((n++ & 1))
            {
                code = b & 0xF;
                i++;
            }
            else
            {
                b = in.u8();
                code = (b >> 4) & 0xF;
            }
            h.set(s.ptr, oki_decode_code(s, tab, code)*16);
            s.ptr = (s.ptr + 1) & 31;
        }
        const float z = oki_taps<4, 21>(half, h, 80 - 3 + s.phase, s.ptr - 1);
        out.put16(adpcm_narrow(z*4.0f));
        if (++s.phase > 3)
            s.phase = 0;
    }
}

// Bytes one call of `samples` >= 1 samples can make, from oki_encode_call(): a byte at every second code with the parity in
// `mark` at odd when the call begins, (codes + 1)/2.  At 32 kbit/s every sample is a code.  At 24 kbit/s every fourth sample
// makes none, and a call that begins at phase 0 loses the fewest: samples - samples/4 codes.
static inline long long oki_encode_capacity(int bit_rate, long long samples)
{
    if (samples <= 0)
        return 0;
    const long long codes = (bit_rate == 24000)  ?  (samples - samples/4)  :  samples;
    return (codes + 1)/2;
}

// Samples one call of `bytes` >= 1 bytes can make, from oki_decode_call(): two a byte at 32 kbit/s.  At 24 kbit/s the call runs
// until its 2*bytes nibbles are taken, one sample per round; a round at phase 0 takes no nibble, and a call that begins at
// phase 0 has the most of those: one in front of every third nibble, ceil(2*bytes/3).  That is the "4 samples per 3 nibbles,
// plus one" of a call, counted exactly.
static inline long long oki_decode_capacity(int bit_rate, long long bytes)
{
    if (bytes <= 0)
        return 0;
    return (bit_rate == 24000)  ?  (2*bytes + (2*bytes + 2)/3)  :  (2*bytes);
}

// ---- the kernels ----------------------------------------------------------------------------------------------------------

#if defined(__HIPCC__)  &&  !defined(SPG_ADPCM_STEP_FUNCTIONS_ONLY)

// A lane's input row, read front to back: the 8-byte word in use and the next one, asked for when the one before it is taken
// up.  `bytes` >= 1 is what the lane may read; the row is whole up to the next 16-byte boundary (codec_host.hpp).
struct AdpcmIn
{
    const uint8_t *row;
    uint64_t cur, next;
    int32_t pos;                // the next byte
    int32_t last;               // the row's last 8-byte word

    __device__ __forceinline__ AdpcmIn(const uint8_t *p, int32_t bytes) : row(p), cur(0), pos(0), last((bytes - 1) >> 3)
    {
        next = *(const uint64_t *) row;
    }

    __device__ __forceinline__ void refill()
    {
        const int32_t k = (pos >> 3) + 1;
        cur = next;
        // (a word past the row's last is never used: the load stays inside the row)
        next = *(const uint64_t *) (row + 8*(size_t) ((k <= last)  ?  k  :  0));
    }

    __device__ __forceinline__ int32_t u8()
    {
        if ((pos & 7) == 0)
            refill();
        const int32_t v = (int32_t) ((cur >> (8*(pos & 7))) & 0xFF);
        pos += 1;
        return v;
    }

    // (at an even position always: an encoder's row holds samples alone)
    __device__ __forceinline__ int32_t s16()
    {
        if ((pos & 7) == 0)
            refill();
        const int32_t v = adpcm_s16((int32_t) ((cur >> (8*(pos & 7))) & 0xFFFF));
        pos += 2;
        return v;
    }
};

// A lane's output row: bytes gather in one 8-byte word, which leaves when it is full.  Nothing is written at or past
// `limit` bytes (the row's stride; the capacity functions keep every count below it).
struct AdpcmOut
{
    uint8_t *row;
    uint64_t acc;
    int32_t pos;
    long long limit;

    __device__ __forceinline__ AdpcmOut(uint8_t *p, long long stride) : row(p), acc(0), pos(0), limit(stride) {}

    __device__ __forceinline__ void leave()
    {
        const int32_t at = (pos - 1) & ~7;
        if ((long long) at + 8 <= limit)
            *(uint64_t *) (row + at) = acc;
        acc = 0;
    }

    __device__ __forceinline__ void put8(int32_t v)
    {
        acc |= (uint64_t) ((uint32_t) v & 0xFFu) << (8*(pos & 7));
        pos += 1;
        if ((pos & 7) == 0)
            leave();
    }

    // (at an even position always: a decoder's row holds samples alone)
    __device__ __forceinline__ void put16(int32_t v)
    {
        acc |= (uint64_t) ((uint32_t) v & 0xFFFFu) << (8*(pos & 7));
        pos += 2;
        if ((pos & 7) == 0)
            leave();
    }

    // what is left, zeros behind it up to the 8-byte boundary
    __device__ __forceinline__ void finish()
    {
        if ((pos & 7) != 0)
            leave();
    }
};

// a 24 kbit/s lane's ring in LDS: entry i of lane `lane` at [i*64 + lane]
struct OkiRing
{
    int16_t *col;

    __device__ __forceinline__ int32_t get(int i) const { return col[i*64]; }
    __device__ __forceinline__ void set(int i, int32_t v) { col[i*64] = (int16_t) v; }
};

// ENCODE: lens are samples and counts bytes; else lens are bytes and counts samples
template <bool ENCODE>
__global__ __launch_bounds__(64) void ima_adpcm_kernel(const CodecLaunch L)
{
    __shared__ int32_t step[kAdpcmStepWords];
    const int lane = threadIdx.x;
    step[lane] = kAdpcmStepDev[lane];
    step[64 + lane] = kAdpcmStepDev[64 + lane];
    __syncthreads();
    const int ch = blockIdx.x*64 + lane;
    if (ch >= L.n_ch)
        return;
    const size_t n = (size_t) L.n_ch;
    int32_t *st = L.st + ch;
    const int mylen = L.lens  ?  min(max(L.lens[ch], 0), L.len)  :  L.len;
    if (mylen == 0)
    {
        L.counts[ch] = 0;
        return;
    }
    Ima s;
    s.variant = st[IM_VARIANT*n];
    s.chunk = st[IM_CHUNK*n];
    s.last = st[IM_LAST*n];
    s.step = min(max(st[IM_STEP*n], 0), kImaStepMax);
    s.byte = st[IM_BYTE*n];
    s.bits = st[IM_BITS*n];
    AdpcmIn in(L.in + (size_t) ch*L.in_stride, ENCODE  ?  2*mylen  :  mylen);
    AdpcmOut out(L.out + (size_t) ch*L.out_stride, L.out_stride);
    if (ENCODE)
        ima_encode_call(s, step, in, out, mylen);
    else
        ima_decode_call(s, step, in, out, mylen);
    out.finish();
    L.counts[ch] = ENCODE  ?  out.pos  :  (out.pos >> 1);
    st[IM_LAST*n] = s.last;
    st[IM_STEP*n] = s.step;
    st[IM_BYTE*n] = s.byte;
    st[IM_BITS*n] = s.bits;
}

template <bool ENCODE>
__global__ __launch_bounds__(64) void oki_adpcm_kernel(const CodecLaunch L)
{
    __shared__ int32_t step[kAdpcmStepWords];
    __shared__ float half[64];
    __shared__ int16_t ring[32*64];
    const int lane = threadIdx.x;
    step[lane] = kAdpcmStepDev[lane];
    step[64 + lane] = kAdpcmStepDev[64 + lane];
    half[lane] = (lane < 41)  ?  kAdpcmHalfDev[lane]  :  0.0f;
    __syncthreads();
    const int ch = blockIdx.x*64 + lane;
    if (ch >= L.n_ch)
        return;
    const size_t n = (size_t) L.n_ch;
    int32_t *st = L.st + ch;
    const int mylen = L.lens  ?  min(max(L.lens[ch], 0), L.len)  :  L.len;
    if (mylen == 0)
    {
        L.counts[ch] = 0;
        return;
    }
    Oki s;
    s.rate = st[OK_RATE*n];
    s.last = st[OK_LAST*n];
    s.step = min(max(st[OK_STEP*n], 0), kOkiStepMax);
    s.byte = st[OK_BYTE*n];
    s.ptr = st[OK_PTR*n] & 31;
    s.mark = st[OK_MARK*n];
    s.phase = st[OK_PHASE*n] & 3;
    OkiRing h = {ring + lane};
    const bool slow = (s.rate == 24000);
    if (slow)
    {
        for (int i = 0;  i < 32;  i++)
            h.set(i, st[(OK_HIST + i)*n]);
    }
    AdpcmIn in(L.in + (size_t) ch*L.in_stride, ENCODE  ?  2*mylen  :  mylen);
    AdpcmOut out(L.out + (size_t) ch*L.out_stride, L.out_stride);
    if (ENCODE)
        oki_encode_call(s, step, half, h, in, out, mylen);
    else
        oki_decode_call(s, step, half, h, in, out, mylen);
    out.finish();
    L.counts[ch] = ENCODE  ?  out.pos  :  (out.pos >> 1);
    st[OK_LAST*n] = s.last;
    st[OK_STEP*n] = s.step;
    st[OK_BYTE*n] = s.byte;
    if (slow)
    {
        for (int i = 0;  i < 32;  i++)
            st[(OK_HIST + i)*n] = h.get(i);
    }
    st[OK_PTR*n] = s.ptr;
    st[OK_MARK*n] = s.mark;
    st[OK_PHASE*n] = s.phase;
}

#endif  // __HIPCC__

}   // namespace spg
