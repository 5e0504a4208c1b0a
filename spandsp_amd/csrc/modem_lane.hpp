// modem_lane.hpp -- the lane frame of the one-channel-per-lane modem receivers (v29_dev.hpp, v27ter_dev.hpp,
// v17_dev.hpp): what a lane does the same way whatever the modem, once.  The kernels keep their tables, word maps and
// state variables, restart constants, slicers, descramblers, trellis, training state machines, timing detectors and
// the round skeleton itself (the __any loops of phases A, B and C): those bodies differ per modem, and a shared one
// would branch on its caller.
//
// Form.  The pulse shaper's inner product is a function template (rrc_dot below).  The other parts are TEXT,
// modem_lane.inc, included inside the kernel body as quad_round_front.inc is in the four-lane kernels:
//     #define LANE_PART LANE_SAMPLE
//     #include "modem_lane.inc"
// They were tried as __forceinline__ function templates and small structs first.  These kernels fill the register file
// and overflow into AGPRs and scratch, and their code is what the register allocator makes of one particular stream of
// IR: a callee is simplified on its own before it is inlined, which reorders instructions, blocks and phis of the
// caller, and every such part but rrc_dot changed the kernels' instructions, most of them registers and scratch too
// (V.29 <16>: 10 -> 42 spilled VGPRs with all of them as functions).  As text the twelve kernels are the instructions
// they were.  profiles/modem_lane_frame.md has the outcome per part.
//
// Before the first part a kernel #defines its constants, and LANE_END at its end takes them away again:
//   LF_FLOATS       float words of state per channel (the integer words follow them)
//   LF_F(x), LF_I(x) the kernel's word map: LF_F(RRC) -> VF_RRC / WF_RRC, LF_I(EQ_STEP) -> VI_ / WI_ / XI_EQ_STEP
//   LF_TILE         samples of PCM staged per lane at a time
//   LF_EQLEN        equaliser length (the delay line's index wraps by mask where that is a power of two)
//   LF_PARKED       its training stage "parked"
//   LF_DELTA        the LMS step size LANE_CARRY_OUT uses; LF_DELTA_MOVES if the training changes it (V.17): a tap
//                   update asked for then uses the one of the moment it was asked, use_delta
// and TAP(i), the lane's equaliser tap i in LDS.  The parts use the kernel's state under the reference's names (rrc_step,
// power_reading, eq_step, carrier_phase_rate ...), L, N, ch, lane, wv and the LDS arrays lanes, lanes16, pcm, t_sqrt.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "v29_common.hpp"

// the parts, in the order a kernel uses them
#define LANE_STATE          1       // ldf / ldi / stf / sti; rrc2 / rrc16, pcmw, rrc_put, rrc_at
#define LANE_RRC_LOAD       2       // state -> RRC delay line
#define LANE_EQ_LOAD        3       // state -> equaliser taps; xre[] / xim[] in age order; eq_clear_pending, restart_pending
#define LANE_RECORDS        4       // evp, n_ev, emit; n_q, qam_report
#define LANE_RRC_CLEAR      5       // restart: the RRC delay line
#define LANE_REQUESTS       6       // do_track / do_tune / do_save, tgt_*, use_track_*; track_carrier, tune_equalizer
#define LANE_STAGE_PCM      7       // a tile of PCM -> LDS
#define LANE_SAMPLE         8       // phase A: next sample -> delay line, signal_detect(); leaves `power`, or breaks
#define LANE_EQ_CLEAR       9       // the restart's deferred clear of xre[] / xim[]
#define LANE_ROOT_POWER     10      // int root_power = fixed_sqrt32(power), at least 1
#define LANE_EQ_PUSH        11      // {hre, him} -> xre[] / xim[], eq_step
#define LANE_EQ_DOT         12      // {zre, zim} = equalizer_get()
#define LANE_CARRY_OUT      13      // the requested carrier update, LMS tap update, save of taps and carrier rate
#define LANE_LINES_STORE    14      // RRC delay line, equaliser taps -> state
#define LANE_EQ_STORE       15      // xre[] / xim[] -> state, in eq_buf's order
#define LANE_END            16      // #undef of the LF_ constants

// eq_buf's index: wraps by mask where the length is a power of two, by compare where it is not (a constant condition)
#define LF_EQ_WRAP(k)       (((LF_EQLEN & (LF_EQLEN - 1)) == 0)  ?  ((k) & (LF_EQLEN - 1))  :  ((k) >= LF_EQLEN)  ?  ((k) - LF_EQLEN)  :  (k))

namespace spg {

// vec_circular_dot_prodf(rrc_filter, coeffs[row], 27, rrc_step)   (vector_float.c:890-939) on the zero padded pairs of
// the RRC delay line (LANE_STATE): rrc2 / rrc16 are the lane's column, the coefficient table is [tap][STRIDE rows].
// The LDS reads go out GROUP taps at a time, ahead of that group's part of the summation chain: V.29, whose filter runs
// on every sample, takes nine (all 54 at once kept 81 registers live across a kernel that already overflows into
// AGPRs), the others all 27.
template <int STRIDE, int GROUP, int CPW, bool PK16>
__device__ __forceinline__ float rrc_dot(const float2 *rrc2, const uint32_t *rrc16, int rrc_step, const float *table, int row)
{
    static_assert(kRrcLen%GROUP == 0, "whole groups of taps");
    const float *y = table + row;
    const float2 *x = rrc2 + rrc_step*CPW;
    const uint32_t *xq = rrc16 + rrc_step*CPW;
    f32x2v a = {0.0f, 0.0f};
#pragma unroll
    for (int i0 = 0;  i0 < kRrcLen;  i0 += GROUP)
    {
        f32x2v xs[GROUP];
        float ys[GROUP];
#pragma unroll
        for (int i = 0;  i < GROUP;  i++)
        {
            if (PK16)
            {
                const uint32_t q = xq[(i0 + i)*CPW];
                xs[i] = (f32x2v) {(float) (int) (short) (q & 0xFFFFu), (float) ((int) q >> 16)};
            }
            else
            {
                const float2 w = x[(i0 + i)*CPW];
                xs[i] = (f32x2v) {w.x, w.y};
            }
            ys[i] = y[(i0 + i)*STRIDE];
        }
        // .x: x[pos..n) . y[0..n-pos) then + 0*y (exact: a running sum that starts at +0 is never -0);
        // .y: 0*y then x[0..pos) . y[n-pos..n) -- the reference's two partial sums, each in its own order
#pragma unroll
        for (int i = 0;  i < GROUP;  i++)
            a += xs[i]*(f32x2v) {ys[i], ys[i]};
    }
    return a.x + a.y;
}

}   // namespace spg
