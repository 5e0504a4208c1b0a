// modem_lane.inc -- the lane frame of the one-channel-per-lane modem receivers, part by part (see modem_lane.hpp for what the
// parts are and why they are text).  Included inside v29_bank_kernel / v27ter_bank_kernel / v17_bank_kernel with
//     #define LANE_PART LANE_xxx
// in front; each part works on the kernel's state under the reference's names.
#if !defined(LANE_PART)  ||  !defined(LF_FLOATS)  ||  !defined(LF_TILE)  ||  !defined(LF_EQLEN)  ||  !defined(LF_PARKED)  ||  !defined(LF_DELTA)  ||  !defined(LF_F)  ||  !defined(LF_I)
#error "modem_lane.inc: LANE_PART and the LF_ constants of the including kernel (modem_lane.hpp)"
#endif

#if LANE_PART == LANE_STATE
    // ---- state word accessors; this lane's RRC delay line and its wave's PCM tile --------------------------------------------
    auto ldf = [&](int w) { return __uint_as_float(L.state[(size_t) w*N + ch]); };
    auto ldi = [&](int w) { return (int32_t) L.state[(size_t) (LF_FLOATS + w)*N + ch]; };
    // A float word goes back as its bits -- except a NaN (a receiver whose equaliser has run away is full of them), which
    // goes back as x86's: there an invalid operation makes the negative quiet NaN and arithmetic hands an operand's NaN on
    // sign and all, while here the negated operand of a subtraction flips it.  Nothing ever depends on a NaN's sign.
    auto stf = [&](int w, float v) { L.state[(size_t) w*N + ch] = (v != v)  ?  0xFFC00000u  :  __float_as_uint(v); };
    auto sti = [&](int w, int32_t v) { L.state[(size_t) (LF_FLOATS + w)*N + ch] = (uint32_t) v; };

    // The delay line, index-major [pair][CPW]: lane l always uses the banks of (l mod 32) whatever its position.  It is stored
    // as 2*27 zero padded pairs: pair k < 27 is {x[k], 0}, pair 27 + k is {0, x[k]} -- the window of 27 pairs starting at the
    // circular position then holds, in .x, the head part of vec_circular_dot_prodf()'s sum padded with zeros and, in .y, zeros
    // followed by its wrapped part, so that one packed multiply-add per tap forms both partial sums of the circular inner
    // product (rrc_dot, modem_lane.hpp).  PK16: pair k = x[k] | 0 << 16, pair 27 + k = 0 | x[k] << 16.
    float2 *rrc2 = &lanes[PK16  ?  0  :  (wv*CPW*2*kRrcLen + lane)];           // [2*27] pairs, stride CPW
    uint32_t *rrc16 = &lanes16[PK16  ?  (wv*CPW*2*kRrcLen + lane)  :  0];
    uint32_t *pcmw = &pcm[wv*CPW*(LF_TILE/2)];
    // delay line element k <- v (both of its pairs); the element back as a float
    auto rrc_put = [&](int k, float v)
    {
        if (PK16)
        {
            const uint32_t h = (uint32_t) (int) v & 0xFFFFu;
            rrc16[k*CPW] = h;
            rrc16[(kRrcLen + k)*CPW] = h << 16;
        }
        else
        {
            rrc2[k*CPW].x = v;
            rrc2[(kRrcLen + k)*CPW].y = v;
        }
    };
    auto rrc_at = [&](int k) -> float
    {
        if (PK16)
            return (float) (int) (short) (rrc16[k*CPW] & 0xFFFFu);
        return rrc2[k*CPW].x;
    };

#elif LANE_PART == LANE_RRC_LOAD
    // ---- rrc_filter[27] of the state into the delay line -------------------------------------------------------------------
    for (int i = 0;  i < kRrcLen;  i++)
    {
        const float v = ldf(LF_F(RRC) + i);
        if (!PK16)
        {
            rrc2[i*CPW] = make_float2(v, 0.0f);
            rrc2[(kRrcLen + i)*CPW] = make_float2(0.0f, v);
        }
        rrc_put(i, v);
    }

#elif LANE_PART == LANE_EQ_LOAD
    // ---- equaliser taps into LDS (TAP(i), [tap][lane]); the equaliser delay line into registers, in age order ---------------
    // xre[i] = eq_buf[(eq_step + i) mod LF_EQLEN] (i = 0 oldest): a shift of the whole line per T/2 instant, so that every
    // access has a compile-time index; the reference's circular position survives only as the per-lane split point of the
    // summation and as the order in which state is stored.
    for (int i = 0;  i < LF_EQLEN;  i++)
        TAP(i) = make_float2(ldf(LF_F(EQ_COEFF) + 2*i), ldf(LF_F(EQ_COEFF) + 2*i + 1));
    float xre[LF_EQLEN];
    float xim[LF_EQLEN];
    bool eq_clear_pending = false;
    bool restart_pending = false;
    {
        const int es = ldi(LF_I(EQ_STEP));
#pragma unroll
        for (int i = 0;  i < LF_EQLEN;  i++)
        {
            int k = es + i;
            k = LF_EQ_WRAP(k);
            xre[i] = ldf(LF_F(EQ_BUF) + 2*k);
            xim[i] = ldf(LF_F(EQ_BUF) + 2*k + 1);
        }
    }

#elif LANE_PART == LANE_RECORDS
    // ---- records: put_bit() / put_status of the reference as events, qam_report() calls --------------------------------------
    int8_t *evp = L.events + (size_t) ch*L.ev_cap;
    int n_ev = 0;
    auto emit = [&](int v)
    {
        if (n_ev < L.ev_cap)
            evp[n_ev] = (int8_t) v;
        n_ev++;
    };

    // qam_report(user, constel, target, symbol) calls, for the kernel variant a caller's tap asks for: one record per
    // call = {events emitted before it in this launch, 1 if the pointers were NULL, symbol, constel re / im, target re / im}
    int n_q = 0;
    auto qam_report = [&](uint32_t null_ptrs, int symbol, float cre, float cim, float tre, float tim)
    {
        if constexpr (QAM)
        {
            if (n_q < L.qam_cap)
            {
                uint32_t *r = L.qam + ((size_t) ch*L.qam_cap + n_q)*7;
                r[0] = (uint32_t) n_ev;
                r[1] = null_ptrs;
                r[2] = (uint32_t) symbol;
                r[3] = __float_as_uint(cre);
                r[4] = __float_as_uint(cim);
                r[5] = __float_as_uint(tre);
                r[6] = __float_as_uint(tim);
            }
            n_q++;
        }
    };

#elif LANE_PART == LANE_RRC_CLEAR
        // ---- *_rx_restart(): the delay line ------------------------------------------------------------------------------
        for (int i = 0;  i < 2*kRrcLen;  i++)
        {
            if (PK16)
                rrc16[i*CPW] = 0;
            else
                rrc2[i*CPW] = make_float2(0.0f, 0.0f);
        }

#elif LANE_PART == LANE_REQUESTS
    // ---- track_carrier() and tune_equalizer() (v29rx.c:281-331) are requested by the stage logic and carried out once, after
    // it (LANE_CARRY_OUT), with the loop gains -- and, where the training changes it, the step size -- as they were when the
    // reference would have called them.
    bool do_track = false;
    bool do_tune = false;
    bool do_save = false;
    float tgt_re = 0.0f;
    float tgt_im = 0.0f;
    float use_track_i = 0.0f;
    float use_track_p = 0.0f;
#ifdef LF_DELTA_MOVES
    float use_delta = 0.0f;
#endif
    auto track_carrier = [&](float tre, float tim)
    {
        do_track = true;
        tgt_re = tre;
        tgt_im = tim;
        use_track_i = carrier_track_i;
        use_track_p = carrier_track_p;
    };
    auto tune_equalizer = [&](float tre, float tim)
    {
        do_tune = true;
        tgt_re = tre;
        tgt_im = tim;
#ifdef LF_DELTA_MOVES
        use_delta = eq_delta;
#endif
    };

#elif LANE_PART == LANE_STAGE_PCM
    // ---- stage this lane's stretch of PCM: pcm[k][lane] = samples 2k, 2k+1 of the tile ----------------------
    {
        static_assert(LF_TILE%8 == 0  &&  LF_TILE >= 8, "the PCM tile is staged in 16-byte pieces");
        const int16_t *row = src + tile;
        const bool wide = ((((uintptr_t) row) & 15) == 0)  &&  (tn == LF_TILE);
        if (wide)
        {
#pragma unroll
            for (int k = 0;  k < LF_TILE/8;  k++)
            {
                const int4 v = ((const int4 *) row)[k];
                pcmw[(4*k + 0)*CPW + lane] = (uint32_t) v.x;
                pcmw[(4*k + 1)*CPW + lane] = (uint32_t) v.y;
                pcmw[(4*k + 2)*CPW + lane] = (uint32_t) v.z;
                pcmw[(4*k + 3)*CPW + lane] = (uint32_t) v.w;
            }
        }
        else
        {
            for (int k = 0;  k < (tn + 1)/2;  k++)
            {
                const uint32_t lo = (uint16_t) row[2*k];
                const uint32_t hi = (2*k + 1 < tn)  ?  (uint16_t) row[2*k + 1]  :  0u;
                pcmw[k*CPW + lane] = lo | (hi << 16);
            }
        }
    }

#elif LANE_PART == LANE_SAMPLE
        // ---- the sample step of phase A, inside the kernel's do { } while (0): the lane's next sample into the delay line
        // and through carrier detection; `break` when it goes no further.  Leaves `power`.
        const uint32_t pw = pcmw[(pos >> 1)*CPW + lane];
        const int amp = (int) (short) ((pos & 1)  ?  (pw >> 16)  :  (pw & 0xFFFF));
        pos++;
        rrc_put(rrc_step, (float) amp);
        if (++rrc_step >= kRrcLen)
            rrc_step = 0;

        // signal_detect() (with the IAXMODEM_STUFF the reference snapshot #defines): v29rx.c:788-865, v27ter_rx.c:779-861,
        // v17rx.c:1133-1210 -- the same text three times
        {
            const int x = amp >> 1;
            int d = (int) (short) (x - last_sample);
            last_sample = x;
            power_reading += ((d*d - power_reading) >> 4);
            power = power_reading;
            d = (int) (short) abs(d);
            if (10*d < high_sample)
            {
                if (++low_samples > 120)
                {
                    power_reading = 0;
                    high_sample = 0;
                    low_samples = 0;
                }
            }
            else
            {
                low_samples = 0;
                if (d > high_sample)
                    high_sample = d;
            }
            if (signal_present > 0)
            {
                if (drop_pending  ||  power < carrier_off_power)
                {
                    if (--signal_present <= 0)
                    {
                        // *_rx_restart() rewrites some forty state variables: done right after the sample loop (the lane
                        // takes no further sample until then), because with it inline every iteration of the loop
                        // paid for the register copies at its merge points
                        restart_pending = true;
                        emit(-1);                           // SIG_STATUS_CARRIER_DOWN
                        power = 0;
                        break;
                    }
                    else
                    {
                        drop_pending = 1;
                    }
                }
            }
            else
            {
                if (power < carrier_on_power)
                {
                    power = 0;
                }
                else
                {
                    signal_present = 1;
                    drop_pending = 0;
                    emit(-2);                               // SIG_STATUS_CARRIER_UP
                }
            }
        }
        if (power == 0  ||  stage == LF_PARKED)
            break;

#elif LANE_PART == LANE_EQ_CLEAR
    // ---- *_rx_restart() clears the equaliser delay line -- but that is register state, and the restart is rare: clearing it
    // there, inside the sample loop, made every iteration of that loop pay ~450 register moves at the merge points.  It is
    // cleared where it is next looked at instead (start of the T/2 phase, write-back).
    if (__any(eq_clear_pending))
    {
        if (eq_clear_pending)
        {
#pragma unroll
            for (int i = 0;  i < LF_EQLEN;  i++)
            {
                xre[i] = 0.0f;
                xim[i] = 0.0f;
            }
            eq_clear_pending = false;
        }
    }

#elif LANE_PART == LANE_ROOT_POWER
                // ---- root_power = fixed_sqrt32(power), math_fixed.c:158-169, never 0 ----
                int root_power;
                {
                    uint32_t xx = (uint32_t) power;
                    const int top = 31 - __builtin_clz(xx);
                    const int shift = 30 - (top & ~1);
                    xx <<= shift;
                    root_power = t_sqrt[((xx >> 24) & 0xFF) - 64] >> (shift >> 1);
                }
                if (root_power == 0)
                    root_power = 1;

#elif LANE_PART == LANE_EQ_PUSH
            // ---- a T/2 instant's {hre, him} into the equaliser delay line ----
#pragma unroll
            for (int i = 0;  i < LF_EQLEN - 1;  i++)
            {
                xre[i] = xre[i + 1];
                xim[i] = xim[i + 1];
            }
            xre[LF_EQLEN - 1] = hre;
            xim[LF_EQLEN - 1] = him;
            if (++eq_step >= LF_EQLEN)
                eq_step = 0;

#elif LANE_PART == LANE_EQ_DOT
                // ---- {zre, zim} = equalizer_get(): cvec_circular_dot_prodf (complex_vector_float.c:137-196), ascending
                // coefficient index, the circular split summed separately and added last -- by snapshotting the accumulator
                // at the per-lane split point instead of branching
                {
                    const int split = LF_EQLEN - eq_step;
                    float2 cs_[LF_EQLEN];
#pragma unroll
                    for (int i = 0;  i < LF_EQLEN;  i++)
                        cs_[i] = TAP(i);
                    f32x2v acc = f32x2v{0.0f, 0.0f};
                    f32x2v fst = f32x2v{0.0f, 0.0f};
#pragma unroll
                    for (int i = 0;  i < LF_EQLEN;  i++)
                    {
                        if (i == split)
                        {
                            fst = acc;
                            acc = f32x2v{0.0f, 0.0f};
                        }
                        // {xr*c.x - xi*c.y, xr*c.y + xi*c.x}: two packed products, a packed add with one negated half
                        const f32x2v t1 = f32x2v{xre[i], xre[i]}*f32x2v{cs_[i].x, cs_[i].y};
                        const f32x2v t2 = f32x2v{xim[i], xim[i]}*f32x2v{cs_[i].y, cs_[i].x};
                        acc += t1 + f32x2v{-t2.x, t2.y};
                    }
                    zre = fst.x + acc.x;
                    zim = fst.y + acc.y;
                }

#elif LANE_PART == LANE_CARRY_OUT
                // ---- what the baud's stage logic asked for (LANE_REQUESTS) ----
                if (do_track)
                {
                    const float error = zim*tgt_re - zre*tgt_im;
                    carrier_phase_rate += v29_f2i(use_track_i*error);
                    carrier_phase += (uint32_t) v29_f2i(use_track_p*error);
                }
                if (do_tune)
                {
                    // cvec_circular_lmsf (complex_vector_float.c:201-219)
                    const float ere = (tgt_re - zre)*LF_DELTA;
                    const float eim = (tgt_im - zim)*LF_DELTA;
#pragma unroll
                    for (int i = 0;  i < LF_EQLEN;  i++)
                    {
                        const float2 c0 = TAP(i);
                        // {xi*eim + xr*ere, xr*eim - xi*ere}
                        const f32x2v u = f32x2v{xim[i], xre[i]}*f32x2v{eim, eim};
                        const f32x2v w = f32x2v{xre[i], xim[i]}*f32x2v{ere, ere};
                        const f32x2v c = f32x2v{c0.x, c0.y}*f32x2v{0.9999f, 0.9999f} + (u + f32x2v{w.x, -w.y});
                        TAP(i) = make_float2(c.x, c.y);
                    }
                }
                if (do_save)
                {
                    carrier_phase_rate_save = carrier_phase_rate;
                    for (int k = 0;  k < LF_EQLEN;  k++)
                    {
                        const float2 c = TAP(k);
                        stf(LF_F(EQ_SAVE) + 2*k, c.x);
                        stf(LF_F(EQ_SAVE) + 2*k + 1, c.y);
                    }
                }

#elif LANE_PART == LANE_LINES_STORE
        // ---- write-back of the RRC delay line and the equaliser taps ----
        for (int i = 0;  i < kRrcLen;  i++)
            stf(LF_F(RRC) + i, rrc_at(i));
        for (int i = 0;  i < LF_EQLEN;  i++)
        {
            const float2 c = TAP(i);
            stf(LF_F(EQ_COEFF) + 2*i, c.x);
            stf(LF_F(EQ_COEFF) + 2*i + 1, c.y);
        }

#elif LANE_PART == LANE_EQ_STORE
        // ---- ... and of the equaliser delay line, in eq_buf's order (after a LANE_EQ_CLEAR) ----
#pragma unroll
        for (int i = 0;  i < LF_EQLEN;  i++)
        {
            int k = eq_step + i;
            k = LF_EQ_WRAP(k);
            stf(LF_F(EQ_BUF) + 2*k, xre[i]);
            stf(LF_F(EQ_BUF) + 2*k + 1, xim[i]);
        }

#elif LANE_PART == LANE_END
    // ---- the end of the kernel: its constants go ----
#undef LF_FLOATS
#undef LF_TILE
#undef LF_EQLEN
#undef LF_PARKED
#undef LF_DELTA
#undef LF_DELTA_MOVES
#undef LF_F
#undef LF_I

#else
#error "modem_lane.inc: unknown LANE_PART"
#endif
#undef LANE_PART
