// v27ter_dev.hpp -- device side of the batched V.27ter receiver (reference: src/v27ter_rx.c:197-1028;
// primitives as in v29_dev.hpp).  Same mapping and baud-aligned execution as the V.29 bank (its header has the reasoning):
// one channel per lane, RRC delay line, PCM tile and equaliser taps index-major in LDS, the equaliser delay line in VGPRs
// in age order, the reference's summation order kept -- the lane frame of modem_lane.hpp, included part by part.
// Differences from V.29 that shape the kernel: the pulse-shaping filter only runs at the T/2
// instants (no per-sample timing-error filter; symbol timing is a Gardner detector on the
// equaliser delay line), 32 taps, an 8-point PSK slicer, and a descrambler with the V.27ter
// repeated-pattern guard.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "v29_dev.hpp"

#include "v27ter_common.hpp"

namespace spg {

// the lane frame's constants (modem_lane.hpp)
#define LF_FLOATS   kV27Floats
#define LF_F(x)     WF_##x
#define LF_I(x)     WI_##x
#define LF_TILE     TILE
#define LF_EQLEN    kV27EqLen
#define LF_PARKED   V27_PARKED
#define LF_DELTA    eq_delta

// WPB, TILE, PK16: several waves per workgroup sharing the tables, a short PCM tile and the RRC delay line as packed
// int16 pairs, for banks of full waves -- see v29_bank_kernel.
template <int CPW, bool QAM = false, int WPB = 1, int TILE = kPcmTile, bool PK16 = false>
__global__ __launch_bounds__(64*WPB)
void v27ter_bank_kernel(const V27Launch L)
{
    static_assert(WPB == 1  ||  CPW == 64, "several waves per workgroup: full waves only");
    __shared__ float t_rrc_re[kV27MaxSets*kRrcLen];     // [tap][set]
    __shared__ float t_rrc_im[kV27MaxSets*kRrcLen];
    __shared__ float t_sine[2048];
    __shared__ uint16_t t_sqrt[194];
    // per-lane RRC delay line (doubled) and PCM tile, index-major [word][CPW]; equaliser taps {re, im} [tap][lane]
    __shared__ float2 lanes[PK16  ?  1  :  WPB*CPW*2*kRrcLen];
    __shared__ uint32_t lanes16[PK16  ?  WPB*CPW*2*kRrcLen  :  1];
    __shared__ uint32_t pcm[WPB*CPW*(TILE/2)];
    __shared__ float2 taps[WPB*kV27EqLen*CPW];

    const int lane = threadIdx.x & 63;
    const int wv = (WPB == 1)  ?  0  :  (int) (threadIdx.x >> 6);
    const int ch = (blockIdx.x*WPB + wv)*CPW + lane;
    constexpr int kThreads = 64*WPB;
    const int tid = threadIdx.x;
    const V27Tables &TB = *L.tab;
    const bool fast = (L.bit_rate == 4800);
    const int sets = fast  ?  8  :  12;
    const int put_add = fast  ?  8*5/2  :  12*20/(3*2);

    {
        const float *sre = fast  ?  TB.re4800  :  TB.re2400;
        const float *sim = fast  ?  TB.im4800  :  TB.im2400;
        for (int i = tid;  i < sets*kRrcLen;  i += kThreads)
        {
            const int set = i/kRrcLen;
            const int tap = i - set*kRrcLen;
            t_rrc_re[tap*kV27MaxSets + set] = sre[i];
            t_rrc_im[tap*kV27MaxSets + set] = sim[i];
        }
    }
    for (int i = tid;  i < 2048;  i += kThreads)
        t_sine[i] = TB.sine[i];
    for (int i = tid;  i < 194;  i += kThreads)
        t_sqrt[i] = TB.sqrt_tab[i];
    __syncthreads();
    if (lane >= CPW  ||  ch >= L.n_ch)
        return;

    const size_t N = (size_t) L.n_ch;
    const int mylen = L.lens  ?  min(max(L.lens[ch], 0), L.samples)  :  L.samples;
#define LANE_PART LANE_STATE
#include "modem_lane.inc"
    float2 *ctap = &taps[wv*kV27EqLen*CPW + lane];
#define TAP(i)      ctap[(i)*CPW]
    constexpr int EQN = kV27EqLen;

    float agc_scaling = ldf(WF_AGC);
    float agc_scaling_save = ldf(WF_AGC_SAVE);
    const float eq_delta = ldf(WF_EQ_DELTA);
    float training_error = ldf(WF_TRAIN_ERR);
    float carrier_track_p = ldf(WF_TRACK_P);
    float carrier_track_i = ldf(WF_TRACK_I);
#define LANE_PART LANE_RRC_LOAD
#include "modem_lane.inc"
#define LANE_PART LANE_EQ_LOAD
#include "modem_lane.inc"
    int rrc_step = ldi(WI_RRC_STEP);
    uint32_t scramble_reg = (uint32_t) ldi(WI_SCRAMBLE);
    int pattern_count = ldi(WI_PATTERN_COUNT);
    int training_bc = ldi(WI_TRAINING_BC);
    int stage = ldi(WI_STAGE);
    int training_count = ldi(WI_TRAIN_COUNT);
    int last_sample = ldi(WI_LAST_SAMPLE);
    int signal_present = ldi(WI_SIGNAL_PRESENT);
    int drop_pending = ldi(WI_DROP_PENDING);
    int low_samples = ldi(WI_LOW_SAMPLES);
    int high_sample = ldi(WI_HIGH_SAMPLE);
    int constellation_state = ldi(WI_CONSTEL);
    uint32_t carrier_phase = (uint32_t) ldi(WI_CARRIER_PHASE);
    int32_t carrier_phase_rate = ldi(WI_PHASE_RATE);
    int32_t carrier_phase_rate_save = ldi(WI_PHASE_RATE_SAVE);
    int32_t power_reading = ldi(WI_POWER);
    const int32_t carrier_on_power = ldi(WI_ON_POWER);
    const int32_t carrier_off_power = ldi(WI_OFF_POWER);
    int eq_step = ldi(WI_EQ_STEP);
    int eq_put_step = ldi(WI_EQ_PUT_STEP);
    int eq_skip = ldi(WI_EQ_SKIP);
    int baud_half = ldi(WI_BAUD_HALF);
    int gardner_integrate = ldi(WI_GARDNER_INT);
    int gardner_step = ldi(WI_GARDNER_STEP);
    int total_corr = ldi(WI_TOTAL_CORR);
    int32_t last_angle0 = ldi(WI_LAST_ANGLES);
    int32_t last_angle1 = ldi(WI_LAST_ANGLES + 1);
    auto diff_ld = [&](int k) { return ldi(WI_DIFF_ANGLES + (k & 0xF)); };
    auto diff_st = [&](int k, int32_t v) { sti(WI_DIFF_ANGLES + (k & 0xF), v); };

#define LANE_PART LANE_RECORDS
#include "modem_lane.inc"

    // v27ter_rx_restart() as the receive path reaches it (v27ter_rx.c:1091-1160; s->old_train is never set)
    auto restart = [&]()
    {
#define LANE_PART LANE_RRC_CLEAR
#include "modem_lane.inc"
        training_error = 0.0f;
        rrc_step = 0;
        scramble_reg = 0x3C;
        pattern_count = 0;
        stage = V27_SYMBOL_ACQUISITION;
        training_bc = 0;
        training_count = 0;
        signal_present = 0;
        high_sample = 0;
        low_samples = 0;
        drop_pending = 0;
        for (int k = 0;  k < 16;  k++)
            diff_st(k, 0);
        carrier_phase = 0;
        carrier_track_i = 200000.0f;
        carrier_track_p = 10000000.0f;
        power_reading = 0;
        constellation_state = 0;
        carrier_phase_rate = v29_f2i(1800.0f*65536.0f*65536.0f/8000);
        agc_scaling = (1.414f/1.000000f)/283.0f;
        for (int i = 0;  i < EQN;  i++)
            TAP(i) = make_float2((i == 17)  ?  1.414f  :  0.0f, 0.0f);      // V27TER_EQUALIZER_PRE_LEN + 1
        eq_clear_pending = true;                            // (LANE_EQ_CLEAR)
        eq_put_step = put_add;
        eq_step = 0;
        eq_skip = 0;
        last_sample = 0;
        gardner_integrate = 0;
        total_corr = 0;
        gardner_step = 512;
        baud_half = 0;
    };

    // the pulse shaper only runs at the T/2 instants: all 27 of its LDS reads go out at once
    auto rrc_dot = [&](const float *table, int row)
    {
        return spg::rrc_dot<kV27MaxSets, kRrcLen, CPW, PK16>(rrc2, rrc16, rrc_step, table, row);
    };
#define LANE_PART LANE_REQUESTS
#include "modem_lane.inc"
    // v27ter_rx.c:380-414
    auto descramble = [&](int in_bit)
    {
        const bool training = (stage > V27_NORMAL  &&  stage < V27_TEST_ONES);
        in_bit &= 1;
        int out_bit = (in_bit ^ (int) (scramble_reg >> 5) ^ (int) (scramble_reg >> 6)) & 1;
        if (pattern_count >= 33)
        {
            out_bit ^= 1;
            pattern_count = 0;
        }
        else if (training)
        {
            pattern_count = 0;
        }
        else
        {
            const uint32_t m = ((scramble_reg >> 7) ^ (uint32_t) in_bit) & ((scramble_reg >> 8) ^ (uint32_t) in_bit)
                             & ((scramble_reg >> 11) ^ (uint32_t) in_bit) & 1u;
            pattern_count = m  ?  0  :  (pattern_count + 1);
        }
        scramble_reg = (scramble_reg << 1) | (uint32_t) (training  ?  out_bit  :  in_bit);
        return out_bit;
    };
    auto put_bit = [&](int bit)
    {
        const int out_bit = descramble(bit);
        if (stage == V27_NORMAL)
            emit(out_bit);
    };
    auto target_of = [&](int k, float &tre, float &tim)
    {
        // v27ter_constellation[8], v27ter_rx.c:125-134
        const float mag = (k & 1)  ?  1.0f  :  1.414f;
        const int q = k >> 1;                               // 0: +re, 1: +im, 2: -re, 3: -im (even k); diagonals for odd k
        if (k & 1)
        {
            tre = (q == 0  ||  q == 3)  ?  1.0f  :  -1.0f;
            tim = (q == 0  ||  q == 1)  ?  1.0f  :  -1.0f;
        }
        else
        {
            tre = (q == 0)  ?  mag  :  (q == 2)  ?  -mag  :  0.0f;
            tim = (q == 1)  ?  mag  :  (q == 3)  ?  -mag  :  0.0f;
        }
    };
    // v27ter_rx.c:441-484
    auto decode_baud = [&](float zre, float zim)
    {
        int nearest;
        if (!fast)
        {
            const int b1 = (zim > zre);
            const int b2 = (zim < -zre);
            nearest = (b2 << 1) | (b1 ^ b2);
            const int raw_bits = (0x1320 >> (4*((nearest - constellation_state) & 3))) & 0xF;      // {0, 2, 3, 1}
            put_bit(raw_bits);
            put_bit(raw_bits >> 1);
            constellation_state = nearest;
            nearest <<= 1;
        }
        else
        {
            const float abs_re = fabsf(zre);
            const float abs_im = fabsf(zim);
            if (abs_im*1.0f > abs_re*0.4142136f  &&  abs_im*1.0f < abs_re*2.4142136f)
            {
                const int b1 = (zre < 0.0f);
                const int b2 = (zim < 0.0f);
                nearest = (b2 << 2) | ((b1 ^ b2) << 1) | 1;
            }
            else
            {
                const int b1 = (zim > zre);
                const int b2 = (zim < -zre);
                nearest = (b2 << 2) | ((b1 ^ b2) << 1);
            }
            const int raw_bits = (int) ((0x51376204u >> (4*((nearest - constellation_state) & 7))) & 0xF);  // {4,0,2,6,7,3,1,5}
            put_bit(raw_bits);
            put_bit(raw_bits >> 1);
            put_bit(raw_bits >> 2);
            constellation_state = nearest;
        }
        float tre;
        float tim;
        target_of(nearest, tre, tim);
        track_carrier(tre, tim);
        if (--eq_skip <= 0)
        {
            eq_skip = 100;
            tune_equalizer(tre, tim);
        }
    };
    auto park = [&]()
    {
        stage = V27_PARKED;
        emit(-5);                                           // SIG_STATUS_TRAINING_FAILED
    };

    const int16_t *src = L.amp + (size_t) ch*L.stride;
    for (int tile = 0;  tile < L.samples;  tile += TILE)
    {
    const int tn = max(0, min(TILE, mylen - tile));         // per lane when the call carries per-channel lengths
#define LANE_PART LANE_STAGE_PCM
#include "modem_lane.inc"
    int pos = 0;
    for (;;)
    {
    // One round = one baud of every lane (see v29_dev.hpp): two T/2 instants, then the baud phase with all lanes in step.
    bool any_ready = false;
    bool restarted = false;
    bool baud_done = false;
    float zre = 0.0f;
    float zim = 0.0f;
    for (int half = 0;  half < 2;  half++)
    {
    const bool take = (half == 1)  ||  (baud_half == 0);
    // ---- phase A: every lane runs its own samples up to its next T/2 instant (cheap here: no per-sample filter) ----
    bool ready = false;
    int power = 0;
    while (__any(take  &&  !ready  &&  !restart_pending  &&  pos < tn))
    {
    if (take  &&  !ready  &&  !restart_pending  &&  pos < tn)
    {
        do
        {
        // ---- v27ter_rx(), v27ter_rx.c:863-1028 ----
#define LANE_PART LANE_SAMPLE
#include "modem_lane.inc"

        eq_put_step -= sets;
        if (eq_put_step <= 0)
            ready = true;
        else
            carrier_phase += (uint32_t) carrier_phase_rate;
        }
        while (0);
    }
    }
    // ---- phase B: the T/2 instant, for all lanes that reached one ----------------------------------------------
    if (__any(restart_pending))
    {
        if (restart_pending)
        {
            restart();
            restart_pending = false;
            restarted = true;
        }
    }
    // (and the restart leaves the clearing of the equaliser delay line to here)
#define LANE_PART LANE_EQ_CLEAR
#include "modem_lane.inc"
    if (ready)
    {
        any_ready = true;
            if (stage == V27_SYMBOL_ACQUISITION)
            {
#define LANE_PART LANE_ROOT_POWER
#include "modem_lane.inc"
                agc_scaling = (1.414f/1.000000f)/(float) root_power;
            }
            const int step = min(-eq_put_step, sets - 1);
            float v = rrc_dot(t_rrc_re, step);
            const float sre = v*agc_scaling;
            v = rrc_dot(t_rrc_im, step);
            const float sim = v*agc_scaling;
            const float dre = t_sine[(uint32_t) (carrier_phase + (1u << 30)) >> 21];
            const float dim = t_sine[carrier_phase >> 21];
            const float hre = sre*dre - sim*dim;
            const float him = -sre*dim - sim*dre;
            eq_put_step += put_add;

            // ---- process_half_baud(), v27ter_rx.c:531-777 ----
#define LANE_PART LANE_EQ_PUSH
#include "modem_lane.inc"
            baud_half ^= 1;
            if (baud_half == 0)
                baud_done = true;
        carrier_phase += (uint32_t) carrier_phase_rate;
    }
    }
    if (!__any(any_ready  ||  restarted))
        break;
    // ---- phase C: the baud, for every lane that completed one in this round ----------------------------------
    if (baud_done)
    {
        carrier_phase -= (uint32_t) carrier_phase_rate;
                {
                    // symbol_sync(), v27ter_rx.c:486-528
                    // eq_buf[(eq_step - 1, -2, -3) & 31] = the three newest entries of the delay line
                    float p = xre[EQN - 3] - xre[EQN - 1];
                    p *= xre[EQN - 2];
                    float q = xim[EQN - 3] - xim[EQN - 1];
                    q *= xim[EQN - 2];
                    gardner_integrate += (p + q > 0.0f)  ?  gardner_step  :  -gardner_step;
                    if (abs(gardner_integrate) >= 128)
                    {
                        eq_put_step += gardner_integrate/128;
                        total_corr += gardner_integrate/128;
                        qam_report(1, gardner_integrate, 0.0f, 0.0f, 0.0f, 0.0f);      // v27ter_rx.c:517-518
                        gardner_integrate = 0;
                    }
                }
#define LANE_PART LANE_EQ_DOT
#include "modem_lane.inc"

                do_track = false;
                do_tune = false;
                do_save = false;
                float rep_re = 0.0f;                        // `target` of process_half_baud(), for the qam report
                float rep_im = 0.0f;
                if (stage == V27_NORMAL  ||  stage == V27_TEST_ONES)
                    decode_baud(zre, zim);
                switch (stage)
                {
                case V27_NORMAL:
                    if constexpr (QAM)
                        target_of(fast  ?  constellation_state  :  (constellation_state << 1), rep_re, rep_im);
                    break;
                case V27_SYMBOL_ACQUISITION:
                    if (++training_count >= 30)
                    {
                        gardner_step = 32;
                        stage = V27_LOG_PHASE;
                        for (int k = 0;  k < 16;  k++)
                            diff_st(k, 0);
                        last_angle0 = v29_arctan2(zim, zre);
                    }
                    break;
                case V27_LOG_PHASE:
                    last_angle1 = v29_arctan2(zim, zre);
                    training_count = 1;
                    stage = V27_WAIT_FOR_HOP;
                    break;
                case V27_WAIT_FOR_HOP:
                {
                    int32_t angle = v29_arctan2(zim, zre);
                    int i = training_count + 1;
                    const int32_t prev = (i & 1)  ?  last_angle1  :  last_angle0;
                    int32_t ang = (int32_t) ((uint32_t) angle - (uint32_t) prev);
                    if (i & 1)
                        last_angle1 = angle;
                    else
                        last_angle0 = angle;
                    diff_st(i, (int32_t) ((uint32_t) diff_ld(i - 2) + (uint32_t) (ang >> 4)));
                    if ((ang > 0x20000000  ||  ang < (int32_t) 0xE0000000u)  &&  training_count >= 13)
                    {
                        i = (training_count - 8) & ~1;
                        if (i > 1)
                        {
                            const int jj = i & 0xF;
                            ang = (int32_t) ((uint32_t) diff_ld(jj) + (uint32_t) diff_ld(jj | 1))/(i - 1);
                            if (fast)
                                carrier_phase_rate += 16*(ang/10);
                            else
                                carrier_phase_rate += 3*16*(ang/40);
                        }
                        if (carrier_phase_rate < v29_f2i((1800.0f - 20.0f)*65536.0f*65536.0f/8000)
                            ||  carrier_phase_rate > v29_f2i((1800.0f + 20.0f)*65536.0f*65536.0f/8000))
                        {
                            park();
                            break;
                        }
                        angle = (int32_t) ((uint32_t) angle + 0x80000000u);
                        const float p = ((uint32_t) angle)*2.0f*3.1415926f/(65536.0f*65536.0f);
                        const float zc = spg_sincosf(p, true);
                        const float zs = -spg_sincosf(p, false);
#pragma unroll
                        for (int k = 0;  k < EQN;  k++)
                        {
                            const float xr = xre[k];
                            const float xi = xim[k];
                            xre[k] = xr*zc - xi*zs;
                            xim[k] = xr*zs + xi*zc;
                        }
                        carrier_phase += (uint32_t) angle;
                        gardner_step = 2;
                        training_bc = 1;
                        training_bc ^= descramble(1);
                        descramble(1);
                        descramble(1);
                        constellation_state = training_bc  ?  4  :  0;
                        rep_re = training_bc  ?  -1.414f  :  1.414f;
                        training_count = 1;
                        stage = V27_TRAIN_ON_ABAB;
                        emit(-3);                           // SIG_STATUS_TRAINING_IN_PROGRESS
                    }
                    else if (++training_count > 50)
                    {
                        park();
                    }
                    break;
                }
                case V27_TRAIN_ON_ABAB:
                {
                    training_bc ^= descramble(1);
                    descramble(1);
                    descramble(1);
                    constellation_state = training_bc  ?  4  :  0;
                    const float tre = training_bc  ?  -1.414f  :  1.414f;
                    rep_re = tre;
                    track_carrier(tre, 0.0f);
                    tune_equalizer(tre, 0.0f);
                    carrier_track_i = 400.0f + (200000.0f - 400.0f)*(float) (1074 - training_count)/(float) 1074;
                    carrier_track_p = 1000000.0f + (10000000.0f - 1000000.0f)*(float) (1074 - training_count)/(float) 1074;
                    if (++training_count >= 1074)
                    {
                        constellation_state = fast  ?  4  :  2;
                        training_count = 0;
                        stage = V27_TEST_ONES;
                    }
                    break;
                }
                case V27_TEST_ONES:
                {
                    float tre;
                    float tim;
                    target_of(fast  ?  constellation_state  :  (constellation_state << 1), tre, tim);
                    rep_re = tre;
                    rep_im = tim;
                    const float dre2 = zre - tre;
                    const float dim2 = zim - tim;
                    training_error += (dre2*dre2 + dim2*dim2);
                    if (++training_count >= 8)
                    {
                        if (training_error < (fast  ?  8.0f*0.25f  :  8.0f*0.5f))
                        {
                            emit(-4);                       // SIG_STATUS_TRAINING_SUCCEEDED
                            signal_present = fast  ?  90  :  120;
                            stage = V27_NORMAL;
                            do_save = true;                 // taps and carrier rate, once this baud's updates are in
                            agc_scaling_save = agc_scaling;
                        }
                        else
                        {
                            park();
                        }
                    }
                    break;
                }
                default:
                    break;
                }
                qam_report(0, constellation_state, zre, zim, rep_re, rep_im);      // v27ter_rx.c:765-777
#define LANE_PART LANE_CARRY_OUT
#include "modem_lane.inc"
        carrier_phase += (uint32_t) carrier_phase_rate;     // dds_advancef() with the rate the baud left behind
    }
    }
    }

    stf(WF_AGC, agc_scaling);
    stf(WF_AGC_SAVE, agc_scaling_save);
    stf(WF_TRAIN_ERR, training_error);
    stf(WF_TRACK_P, carrier_track_p);
    stf(WF_TRACK_I, carrier_track_i);
#define LANE_PART LANE_LINES_STORE
#include "modem_lane.inc"
#define LANE_PART LANE_EQ_CLEAR
#include "modem_lane.inc"
#define LANE_PART LANE_EQ_STORE
#include "modem_lane.inc"
    sti(WI_RRC_STEP, rrc_step);
    sti(WI_SCRAMBLE, (int32_t) scramble_reg);
    sti(WI_PATTERN_COUNT, pattern_count);
    sti(WI_TRAINING_BC, training_bc);
    sti(WI_STAGE, stage);
    sti(WI_TRAIN_COUNT, training_count);
    sti(WI_LAST_SAMPLE, last_sample);
    sti(WI_SIGNAL_PRESENT, signal_present);
    sti(WI_DROP_PENDING, drop_pending);
    sti(WI_LOW_SAMPLES, low_samples);
    sti(WI_HIGH_SAMPLE, high_sample);
    sti(WI_CONSTEL, constellation_state);
    sti(WI_CARRIER_PHASE, (int32_t) carrier_phase);
    sti(WI_PHASE_RATE, carrier_phase_rate);
    sti(WI_PHASE_RATE_SAVE, carrier_phase_rate_save);
    sti(WI_POWER, power_reading);
    sti(WI_EQ_STEP, eq_step);
    sti(WI_EQ_PUT_STEP, eq_put_step);
    sti(WI_EQ_SKIP, eq_skip);
    sti(WI_BAUD_HALF, baud_half);
    sti(WI_GARDNER_INT, gardner_integrate);
    sti(WI_GARDNER_STEP, gardner_step);
    sti(WI_TOTAL_CORR, total_corr);
    sti(WI_LAST_ANGLES, last_angle0);
    sti(WI_LAST_ANGLES + 1, last_angle1);
    L.ev_count[ch] = n_ev;
    if constexpr (QAM)
        L.qam_count[ch] = n_q;
#undef TAP
}

#define LANE_PART LANE_END
#include "modem_lane.inc"

}   // namespace spg
