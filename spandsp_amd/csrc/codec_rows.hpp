// codec_rows.hpp -- what the codec banks' kernels share (g726_dev.hpp, g722_dev.hpp): a lane's row in 16-byte chunks, the
// launch struct, and the kernel itself, codec_kernel<Codec, ENCODE>, whose per-item step and sizes come from the family's
// Codec struct.  HIP only: a host build of a _dev.hpp (tests/c_callers/g72x_host.cpp) takes the step functions and sees
// nothing of this file.
//
// In: a window of two chunks; an element is picked out of it by selects (the position differs from lane to lane), and once a
// group of items is through (Codec::kGroup of them, 16 input bytes at the most), a lane whose position has left the first
// chunk moves on to the chunk requested before that group.  Out: bytes gather in three 8-byte words; sixteen of them leave
// as one chunk (a group makes 16 bytes at the most).
//
// What a Codec holds:
//   State                       a channel's state in registers
//   kTabWords, table()          the lookup table the kernel copies to LDS (a multiple of 64 words) and where it lies
//   kGroup                      items between two advances of the window: 8 (G.726, a sample takes 2 bytes at the most) or
//                               4 (G.722, a code takes or makes 4)
//   kWidest                     the widest element pushed, in bytes
//   load(), store()             the state from and to st[word*n]
//   unit()                      the per-lane size the others go by (G.726: bytes of a PCM element; G.722: samples of a code)
//   pcm_bytes()                 bytes of a PCM element: an encoder's lengths and a decoder's counts are in elements
//   todo<ENCODE>()              items of this call, from the state, the lane's length and the output stride
//   take<ENCODE>()              the input bytes the next item consumes, asked before its step
//   step<ENCODE>()              one item, from the word at the lane's position: the value and the width to push (RowPush)

#pragma once

#if defined(__HIPCC__)

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace spg
{

struct RowIn
{
    uint32_t w[8];
    int32_t pos;            // the next byte, 0 .. 31
    int32_t chunk;          // the row's chunk in w[0 .. 3]
};

// (the eight words by value: picked through a reference to the struct, the compiler keeps the window in LDS)
__device__ __forceinline__ uint32_t row_pick(int i, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t w5, uint32_t w6, uint32_t w7)
{
    const uint32_t a = (i & 1)  ?  w1  :  w0;
    const uint32_t b = (i & 1)  ?  w3  :  w2;
    const uint32_t c = (i & 1)  ?  w5  :  w4;
    const uint32_t d = (i & 1)  ?  w7  :  w6;
    const uint32_t e = (i & 2)  ?  b  :  a;
    const uint32_t f = (i & 2)  ?  d  :  c;
    return (i & 4)  ?  f  :  e;
}

// the word that holds the next byte, shifted down to it (an element never straddles a word: its position is a multiple of
// its width)
__device__ __forceinline__ uint32_t row_in_peek(const RowIn &in)
{
    return row_pick(in.pos >> 2, in.w[0], in.w[1], in.w[2], in.w[3], in.w[4], in.w[5], in.w[6], in.w[7]) >> (8*(in.pos & 3));
}

struct RowOut
{
    uint64_t w[3];
    int32_t fill;           // bytes held, 0 .. 23
    int32_t chunk;          // the next chunk of the row to write
};

// what an item leaves: `bytes` of v
struct RowPush
{
    uint32_t v;
    int32_t bytes;
};

// `bytes` (0, 1, 2 or, where WIDEST is 4, 4; at a fill that is a multiple of it) of v.  One body for both families: with
// a mask chosen four ways for everybody, the G.726 kernels' code moved (same registers, other instructions).
template <int WIDEST>
__device__ __forceinline__ void row_out_push(RowOut &o, uint32_t v, int32_t bytes)
{
    const uint32_t mask = (WIDEST == 4  &&  bytes == 4)  ?  0xFFFFFFFFu  :  ((bytes == 2)  ?  0xFFFFu  :  0xFFu);
    const uint64_t x = (uint64_t) (bytes  ?  (v & mask)  :  0) << (8*(o.fill & 7));
    const int k = o.fill >> 3;
    o.w[0] |= (k == 0)  ?  x  :  0;
    o.w[1] |= (k == 1)  ?  x  :  0;
    o.w[2] |= (k == 2)  ?  x  :  0;
    o.fill += bytes;
}

// chunk `chunk` of a row whose last chunk is `last`; past it, chunk 0 again: a load that is never used stays inside the row
__device__ __forceinline__ uint4 row_chunk(const uint8_t *row, int chunk, int last)
{
    return *(const uint4 *) (row + 16*(size_t) ((chunk <= last)  ?  chunk  :  0));
}

__device__ __forceinline__ void row_flush(uint8_t *dst, const RowOut &o)
{
    *(uint4 *) (dst + 16*(size_t) o.chunk) = make_uint4((uint32_t) o.w[0], (uint32_t) (o.w[0] >> 32), (uint32_t) o.w[1], (uint32_t) (o.w[1] >> 32));
}

struct CodecLaunch
{
    int32_t *st;                // [words][n_ch]
    const uint8_t *in;          // rows of in_stride bytes, 16-byte aligned
    uint8_t *out;               // rows of out_stride bytes, 16-byte aligned
    const int32_t *lens;        // [n_ch] samples (encode) or bytes (decode), or NULL: `len` for all
    int32_t *counts;            // [n_ch] bytes written (encode) or samples (decode)
    long long in_stride;
    long long out_stride;
    int n_ch;
    int len;
};

// ENCODE: lens are samples and counts bytes; else lens are bytes and counts samples
template <class Codec, bool ENCODE>
__global__ __launch_bounds__(64) void codec_kernel(const CodecLaunch L)
{
    __shared__ __attribute__((aligned(16))) int32_t table[Codec::kTabWords];
    const int lane = threadIdx.x;
_Pragma("unroll")
    for (int i = 0;  i < Codec::kTabWords/64;  i++)
        table[i*64 + lane] = Codec::table()[i*64 + lane];
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
    typename Codec::State s;
    Codec::load(s, st, n);
    const int unit = Codec::unit(s);
    const int todo = Codec::template todo<ENCODE>(s, unit, mylen, L.out_stride);
    const int el = Codec::pcm_bytes(unit);
    const int in_bytes = ENCODE  ?  mylen*el  :  mylen;
    const int last = (in_bytes - 1) >> 4;
    const uint8_t *src = L.in + (size_t) ch*L.in_stride;
    uint8_t *dst = L.out + (size_t) ch*L.out_stride;

    RowIn in;
    RowOut out;
    {
        const uint4 q0 = row_chunk(src, 0, last);
        const uint4 q1 = row_chunk(src, 1, last);
        in.w[0] = q0.x;  in.w[1] = q0.y;  in.w[2] = q0.z;  in.w[3] = q0.w;
        in.w[4] = q1.x;  in.w[5] = q1.y;  in.w[6] = q1.z;  in.w[7] = q1.w;
    }
    in.pos = 0;
    in.chunk = 0;
    out.w[0] = out.w[1] = out.w[2] = 0;
    out.fill = 0;
    out.chunk = 0;
    uint4 ahead = {0, 0, 0, 0};
    for (int i = 0;  i < todo;  i++)
    {
        // (i is the same in every lane still in the loop, so the two branches on it are the wave's)
        if ((i & (Codec::kGroup - 1)) == 0)
            ahead = row_chunk(src, in.chunk + 2, last);
        const uint32_t raw = row_in_peek(in);
        // (a call of its own, ahead of the step: folded into the step's result, the G.722 decoder's code moved)
        in.pos += Codec::template take<ENCODE>(s, unit);
        const RowPush p = Codec::template step<ENCODE>(s, table, unit, raw);
        row_out_push<Codec::kWidest>(out, p.v, p.bytes);
        if ((i & (Codec::kGroup - 1)) == Codec::kGroup - 1)
        {
            const bool on = (in.pos >= 16);
            in.w[0] = on  ?  in.w[4]  :  in.w[0];
            in.w[1] = on  ?  in.w[5]  :  in.w[1];
            in.w[2] = on  ?  in.w[6]  :  in.w[2];
            in.w[3] = on  ?  in.w[7]  :  in.w[3];
            in.w[4] = on  ?  ahead.x  :  in.w[4];
            in.w[5] = on  ?  ahead.y  :  in.w[5];
            in.w[6] = on  ?  ahead.z  :  in.w[6];
            in.w[7] = on  ?  ahead.w  :  in.w[7];
            in.pos -= on  ?  16  :  0;
            in.chunk += on  ?  1  :  0;
            if (out.fill >= 16)
            {
                row_flush(dst, out);
                out.w[0] = out.w[2];
                out.w[1] = 0;
                out.w[2] = 0;
                out.fill -= 16;
                out.chunk++;
            }
        }
    }
    // what is left leaves as chunks too: the row is written up to the next 16-byte boundary past its count
    const int32_t total = 16*out.chunk + out.fill;
    if (out.fill > 0)
        row_flush(dst, out);
    if (out.fill > 16)
        *(uint4 *) (dst + 16*(size_t) (out.chunk + 1)) = make_uint4((uint32_t) out.w[2], (uint32_t) (out.w[2] >> 32), 0u, 0u);
    L.counts[ch] = ENCODE  ?  total  :  (total/el);
    Codec::store(s, st, n);
}

}   // namespace spg

#endif  // __HIPCC__
