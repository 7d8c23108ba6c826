// vigo_solver_optimize.inc — the text of one whole solve, included as a function body (vigo_solver.hip): of k_optimize
// (VIGO_OPTIMIZE_ENTRY 1: finds its trajectory, loads it and decides whether this launch solves it), and of
// optimize_loaded (0: b, Q, x, K and KL come from the caller, k_optimize_fused, which has done all that).  The
// including function provides T, GROUP, PPL, FAST, OBS, D, RH, MIXED, SOLO and A.
    static_assert(!MIXED || (D == 3 && OBS && PPL == 1), "mixed counts: the general kernel, one point per lane");
    static_assert(PPL == 1 ? (RH >= 1 && RH <= 6) : RH == 0, "register-held history only with one point per lane");
    // AXIS (D == 1): a level trajectory on a whole wave, one COORDINATE per lane — lane l < 32 holds coordinate 0 of
    // control point l, lane l + 32 coordinate 1 of the same point (GROUP = 32 is then the lanes of one axis).  Every
    // loop-carried vector is one double per lane, an axpy one instruction, a history record {s, y} of one axis; a
    // dot product is one product, the xor-32 exchange (the add dot3<.., 2> does) and the 32-lane tree, so both halves
    // hold the same bits in every scalar and nothing diverges inside the wave.  fp64 reference order, no obstacles.
    constexpr bool AXIS = D == 1;
    static_assert(!AXIS || (std::is_same<T, double>::value && GROUP == 32 && PPL == 1 && !FAST && !OBS),
                  "the axis-per-lane layout: fp64 reference order, N <= 32, no obstacles");
    static_assert(!SOLO || (D == 3 && GROUP == 32 && PPL == 1 && !OBS && !MIXED && kMaxMem <= GROUP),
                  "one trajectory alone on half a wave: the general no-obstacle body of 32 x 1");
#if VIGO_OPTIMIZE_ENTRY
    const DevConst& K = *Kp;  // uniform address: scalar loads at the use sites, not 100+ live SGPRs
#endif
    constexpr int TPB = (AXIS || SOLO) ? 1 : kWave / GROUP;   // trajectories per wave
    constexpr int COLS = SOLO ? 1 : kWave / GROUP;  // history columns per free control point index: trajectories, or axes
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int N = A.N, NI = N - 6;
    const int ROW = COLS * NI;
    // one more column per slot that holds zeros for good: the history of every control point that is NOT free (the
    // three fixed points at either end, lanes beyond N).  Their s and y are identically zero, so the two-loop needs
    // no per-step select to keep their d at zero (two v_cndmask on the dependent chain of each of its 32 steps).
    const int ROWP = ROW + 1;
    using YS = YSv<FAST>;
    // A history slot = its ROWP records followed by the slot's {ys, 1/ys} per trajectory, so the steady-state ring
    // walks ONE byte offset for both (slot stride in bytes, a multiple of 16 for the ds_read_b128s)
    constexpr int kYsSlotBytes = (TPB * (int)sizeof(YS) + 15) & ~15;
    const int slotB = ROWP * (int)sizeof(HPair<T, D>) + kYsSlotBytes;
    const int m = K.mem_size;
#if VIGO_OPTIMIZE_ENTRY
    const LoopConst<AXIS> KL(K);   // what the iteration loop reads: K itself, or (AXIS) its fields held in registers
#endif
    // REG1 (one control point per lane): the two newest history pairs (ages 0 and 1) stay in
    // registers, LDS holds the older m - 2 — at N = 64, m = 16 that is 38.3 KB instead of 43.8 KB
    // per wave, i.e. four resident waves per CU (one per SIMD) instead of three.
    constexpr bool REG1 = (PPL == 1);
    const int ms = REG1 ? (m > RH + 1 ? m - (RH + 1) : 0) : m;   // history slots in LDS
    HPair<T, D>* hist = reinterpret_cast<HPair<T, D>*>(lds_raw);
    double* ys_tab = reinterpret_cast<double*>(lds_raw + (size_t)ms * slotB);   // alphas, obstacle table

    const int lane = threadIdx.x;
    const int grp = lane / GROUP;            // the lane's trajectory within the wave; AXIS: its axis; SOLO: 0
    const int tg = AXIS ? 0 : grp;           // the lane's trajectory within the wave
#if VIGO_OPTIMIZE_ENTRY
    int b = blockIdx.x * TPB + tg;
    if (A.active_idx) {                       // vigo_rebound_rounds: the compacted active set
        if (b >= *A.active_count) return;
        b = A.active_idx[b];
    } else if (b >= A.B) {
        return;
    }

    LaneProblem<T, PPL> Q;
    const bool valid_n = load_problem<T, GROUP, PPL, MIXED>(A, K, b, lane % GROUP, Q);
    // x holds this lane's control points: free variables where interior, fixed boundary points
    // elsewhere (their g, d, s, y are identically zero so they never move).
    T x[PPL][3];
    load_points<T, PPL>(A, b, Q, x);
    set_level<T, GROUP, PPL>(K, Q, x);       // (AXIS: both halves hold the point's z and get the same answer)
    if constexpr (AXIS) {
        if (!Q.level) return;                // solved by the general kernel, which follows
        x[0][0] = grp ? x[0][1] : x[0][0];
        axis_guides(Q, grp);
    } else {
        // A solve is launched as ONE general kernel (D = 3), or — calls without obstacles, one point per lane — as the
        // D = 2 instantiation, which carries only x and y through the recursion (two thirds of the history in LDS, of
        // the dot products and of the stencils), followed by the general kernel: a wave whose trajectories are ALL
        // level is solved by the first launch and skipped by the second, every other wave the other way round.  A
        // level trajectory that shares a wave with one that is not is solved here with its z terms masked: the same
        // bits either way, so a result never depends on which trajectory it was paired with.
        const bool wave_level = __all(Q.level);
        if (D == 2 && !wave_level) return;
        if (D == 3 && A.level_waves_elsewhere && wave_level) return;
    }
#endif  // VIGO_OPTIMIZE_ENTRY
    // level_waves_elsewhere == 2: EVERY level trajectory has been solved by the axis-per-lane launch, also one that
    // shares this wave with a trajectory that is not level.  Its group leaves below, once the zero column is written
    // (the lanes that write it may be its own), and the other group goes on alone — as it already does whenever its
    // line search takes more evaluations than its partner's.  Every wave-wide operation from there on acts on the
    // active lanes only and is used that way: the DPP rows and v_permlane16_swap of the reductions stay inside a
    // group; readfirstlane(bound) and readfirstlane(last) read the first ACTIVE lane, and the __any over `last` and
    // over the two-loop's range flag see the remaining group alone, as they see one trajectory in the last wave of
    // an odd batch; the single-wave __syncthreads does not wait for lanes that have returned.
    const bool solved_elsewhere = D == 3 && !SOLO && A.level_waves_elsewhere == 2 && Q.level;
#if VIGO_PROFILE_SECTIONS
    long long tick_ = (long long)__builtin_readcyclecounter();
    double t_eval = 0, t_ls = 0, t_upd = 0, t_two = 0, t_tail = 0, t_pre = 0, t_trial = 0, t_cal = 0;
#endif
    // history column of each owned point; points that are not free read the zero column and never write
    HPair<T, D>* hl[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        const int p = Q.p0 + q;
        hl[q] = Q.interior[q] ? hist + (grp * NI + (p - 3)) : hist + ROW;
    }
    for (int slot = lane; slot < ms; slot += kWave) {
        HPair<T, D> zero;
#pragma unroll
        for (int a = 0; a < D; ++a) zero.s[a] = zero.y[a] = T(0);
        *reinterpret_cast<HPair<T, D>*>(lds_raw + (size_t)slot * slotB + (size_t)ROW * sizeof(HPair<T, D>)) = zero;
    }
    __syncthreads();   // one wave per workgroup: orders the zero column before the first history read
    if (solved_elsewhere) return;
    if (MIXED && !valid_n) {   // a bad count: LBFGSERR_INVALID_N (LB:36) and nothing else; its group leaves as above
        if (lane % GROUP == 0 && A.out_status) A.out_status[(size_t)b * (A.status_stride ? A.status_stride : 1)] = LBERR_INVALID_N;
        return;
    }
    YS* ys_l = reinterpret_cast<YS*>(lds_raw + (size_t)ROWP * sizeof(HPair<T, D>)) + tg;   // slot 0; slot k at + k * slotB bytes
    double* al_l = ys_tab + tg;
    auto hist_at = [&](int q, int slot) -> HPair<T, D>& {
        return *reinterpret_cast<HPair<T, D>*>(reinterpret_cast<char*>(hl[q]) + (size_t)slot * slotB);
    };
    auto ys_at = [&](int slot) -> YS& { return *reinterpret_cast<YS*>(reinterpret_cast<char*>(ys_l) + (size_t)slot * slotB); };
    if (!OBS) { Q.obs = nullptr; Q.o_begin = Q.o_end = 0; }
    if (OBS && A.obs) {
        // stage this trajectory's obstacles once: the predicted positions and thresholds of
        // BT.cpp:1011-1020 by the expressions of obstacle_term(), sizes in T arithmetic
        constexpr int kEnt = kObsTabEntries<GROUP>;
        double* tab = ys_tab + (size_t)m * TPB + (size_t)grp * kObsTabDoubles<GROUP>;
        const int cnt = Q.o_end - Q.o_begin;
        const int steps = K.pred_num / 2 + 1;
        int fit = kEnt / steps;
        if (fit > kObsTabObs) fit = kObsTabObs;
        Q.o_tab = cnt < fit ? cnt : fit;
        Q.o_steps = steps;
        Q.obs_tab = tab;
        Q.obs_size = tab + 3 * kEnt;
        for (int e = lane % GROUP; e < Q.o_tab * steps; e += GROUP) {
            const int j = e / steps, n = 2 * (e - j * steps);
            const double* o = A.obs + 9 * (size_t)(Q.o_begin + j);
            const T tn = (T)((double)n * K.ts);
            tab[3 * e + 0] = (double)((T)o[0] + tn * (T)o[3]);
            tab[3 * e + 1] = (double)((T)o[1] + tn * (T)o[4]);
            tab[3 * e + 2] = (double)((T(1) - (T)(n / K.pred_num) * T(0.2)) * (T)K.thr_dyn);
        }
        for (int j = lane % GROUP; j < Q.o_tab; j += GROUP) {
            const double* o = A.obs + 9 * (size_t)(Q.o_begin + j);
            const T hx = (T)o[6] / 2, hy = (T)o[7] / 2;
            tab[3 * kEnt + j] = (double)(T)sqrt(hx * hx + hy * hy);
        }
        __syncthreads();  // one wave per workgroup: orders the staging writes before the lanes' reads
    }

    T g[PPL][3], xp[PPL][3], gp[PPL][3], d[PPL][3];
#pragma unroll
    for (int q = 0; q < PPL; ++q)
#pragma unroll
        for (int a = 0; a < 3; ++a) g[q][a] = xp[q][a] = gp[q][a] = d[q][a] = T(0);
    constexpr int kRH = RH > 0 ? RH : 1;
    T sR[kRH][PPL][3], yR[kRH][PPL][3];   // REG1: the pairs of ages 1 .. RH of the next two-loop (sR[j] = age j + 1)
    YS ysR[kRH]{};
#pragma unroll
    for (int q = 0; q < PPL; ++q)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int j = 0; j < kRH; ++j) sR[j][q][a] = yR[j][q][a] = T(0);
    // AXIS: the z coordinate.  Under the level rule its g, s and y are exact zeros and its d is -0 through every step of a
    // two-loop whose coefficients are finite, so z + step * d is z: nothing to carry.  A coefficient that is NOT finite
    // (ys = 0, see below) makes that d a NaN (0 * inf) in the general kernel and in the oracle, and the next trial point's
    // z with it.  The d of a control point that is not free goes through the same operations on the same zeros: dz is
    // lane 0's, taken once per iteration, and the trial point's z is formed from it as the general kernel forms it.
    T dz = T(-0.0);
    double sums[7];
    int evals = 0;
    int ret = LBERR_UNKNOWN;
    int k = 0, end = 0, last = 0;
    double fx = 0.0, step = 0.0;
    bool first = true;

    for (;;) {  // one trip per L-BFGS iteration; trip 0 only evaluates the start point (LB:1132)
        // ---------------- line_search_morethuente, LB:716-937 ----------------
        int ls = 0;
        if constexpr (AXIS && (VIGO_AXIS_LS_FIRST_TESTS || VIGO_AXIS_LS_FIRST_SETUP)) {
            // The search of vigo_linesearch.hpp, the same statements as the else arm's, with the set-up of a trial moved
            // to the end of the trial before it (still ONE evaluation site): the first trial's set-up, ahead of the loop,
            // is then the two clamps and stmax.  Behind switches that are off (measured and rejected), a first-trial path
            // after the evaluation — every scalar is the same in every lane, so __any() of a lane's condition is that
            // condition and the branch the wave's.  FIRST_TESTS: the first trial's exits are the four that need no bracket.
            // FIRST_SETUP = 1: interval ends, widths and the bracket's six doubles are formed by ls_first_reject, from the
            // step kept as it was before the clamps.
            constexpr bool kTests = VIGO_AXIS_LS_FIRST_TESTS, kDefer = VIGO_AXIS_LS_FIRST_SETUP == 1;
            const LsParams P{KL.min_step, KL.max_step, KL.ftol, KL.gtol, KL.xtol, KL.max_linesearch};
            LsState S;   // (fresh: 17 values would otherwise stay live across the two-loop, 35 more registers and AGPR copies)
            fresh_reg(S.dginit); fresh_reg(S.finit); fresh_reg(S.dgtest); fresh_reg(S.width); fresh_reg(S.prev_width);
            fresh_reg(S.xt); fresh_reg(S.xf); fresh_reg(S.xd); fresh_reg(S.yt); fresh_reg(S.yf); fresh_reg(S.yd);
            fresh_reg(S.stmin); fresh_reg(S.stmax);
            fresh_reg(S.count); fresh_reg(S.brackt); fresh_reg(S.stage1); fresh_reg(S.uinfo);
            double step0 = step;
            auto move_x = [&]() {   // x <- xp + step * d  (LB:824-825)
                x[0][0] = xp[0][0] + step * d[0][0];
                x[0][2] = xp[0][2] + step * (Q.interior[0] ? dz : 0.0);
            };
            bool run = true;
            if (!first) {
                xp[0][0] = x[0][0]; gp[0][0] = g[0][0];  // LB:1172-1173
                xp[0][2] = x[0][2];
                // sums[4]: g.d for the d just built (reduced at the end of the two-loop below)
                ls = kDefer ? ls_first_begin(P, S, step, fx, sums[4]) : ls_begin(P, S, step, fx, sums[4]);
                run = ls == 0;
                if (run) {
                    if constexpr (kDefer) ls_first_setup(P, step);
                    else ls_setup(P, S, step);   // (brackt = 0, xt = 0 are constants here: the clamps and stmax are left)
                    move_x();
                }
            }
            while (run) {
                VIGO_TICK(t_pre);
                fx = eval_cost_grad_axis(KL, Q, grp, x, d, g, sums);   // the only evaluation site (LB:828, :1132)
                VIGO_TICK(t_eval);
                ++evals;
                if (first) break;

                const double dg = sums[4];
                const double ftest1 = ls_ftest1(S, step);
                ++S.count;
                if ((kTests || kDefer) && S.count == 1) {   // a scalar branch
                    if constexpr (kTests) {
                        const int code = ls_first_exit_code(P, S, step, fx, dg, ftest1);
                        if (__any(code != 0)) { ls = code; break; }
                    }
                    if constexpr (kDefer) {
                        hold_in_reg(step0);   // keeps the state behind the branch
                        ls_first_reject(P, S, step0);
                        // (... and its copies out of the block the accepted trial leaves through)
                        hold_in_reg(S.xt); hold_in_reg(S.xf); hold_in_reg(S.xd); hold_in_reg(S.yt); hold_in_reg(S.yf); hold_in_reg(S.yd);
                        hold_in_reg(S.width); hold_in_reg(S.prev_width); hold_in_reg(S.stmin); hold_in_reg(S.stmax);
                        hold_in_reg(S.brackt); hold_in_reg(S.stage1); hold_in_reg(S.uinfo);
                    }
                }
                if (!kTests || S.count != 1) {
                    const int code = ls_exit_code(P, S, step, fx, dg, ftest1);
                    if (code != 0) { ls = code; break; }
                }
                VIGO_TICK(t_ls);
                ls_update(P, S, step, fx, dg, ftest1);
                VIGO_TICK(t_trial);
                ls_setup(P, S, step);
                move_x();
            }
        } else {
            int count = 0, brackt = 0, stage1 = 1, uinfo = 0;
            double dginit = 0.0, finit = 0.0, dgtest = 0.0, width = 0.0, prev_width = 0.0;
            double xt = 0., xf = 0., xd = 0., yt = 0., yf = 0., yd = 0.;
            const double stpmin = KL.min_step, stpmax = KL.max_step;
            bool run = true;
            if (!first) {
#pragma unroll
                for (int q = 0; q < PPL; ++q)
#pragma unroll
                    for (int a = 0; a < D; ++a) { xp[q][a] = x[q][a]; gp[q][a] = g[q][a]; }  // LB:1172-1173
                if constexpr (AXIS) xp[0][2] = x[0][2];
                dginit = sums[4];  // g.d for the d just built (reduced at the end of the two-loop below)
                if (step <= 0.) { ls = LBERR_INVALIDPARAMETERS; run = false; }
                else if (0 < dginit) { ls = LBERR_INCREASEGRADIENT; run = false; }
                finit = fx;
                dgtest = KL.ftol * dginit;
                width = stpmax - stpmin;
                prev_width = 2.0 * width;
                xt = yt = 0.;
                xf = yf = finit;
                xd = yd = dginit;
            }
            while (run) {
                double stmin = 0., stmax = 0.;
                if (!first) {
                    if (brackt) {
                        stmin = xt <= yt ? xt : yt;
                        stmax = xt >= yt ? xt : yt;
                    } else {
                        stmin = xt;
                        stmax = step + 4.0 * (step - xt);
                    }
                    if (step < stpmin) step = stpmin;
                    if (stpmax < step) step = stpmax;
                    if ((brackt && ((step <= stmin || stmax <= step) || KL.max_linesearch <= count + 1 || uinfo != 0)) ||
                        (brackt && (stmax - stmin <= KL.xtol * stmax))) {
                        step = xt;
                    }
                    // x <- xp + step * d  (LB:824-825)
#pragma unroll
                    for (int q = 0; q < PPL; ++q)
#pragma unroll
                        for (int a = 0; a < D; ++a)
                            x[q][a] = FAST ? fmaT((T)step, d[q][a], xp[q][a]) : xp[q][a] + (T)step * d[q][a];
                    if constexpr (AXIS) x[0][2] = xp[0][2] + (T)step * (Q.interior[0] ? dz : T(0));
                }

                VIGO_TICK(t_pre);
                // the only evaluation site (LB:828, :1132)
                if constexpr (AXIS) fx = eval_cost_grad_axis(KL, Q, grp, x, d, g, sums);
                else fx = eval_cost_grad<T, GROUP, PPL, FAST, OBS, D>(KL, Q, x, d, g, sums);
                VIGO_TICK(t_eval);
                ++evals;
                if (first) break;

                const double dg = sums[4];
                const double ftest1 = finit + step * dgtest;
                ++count;

                // LB:832-866: six exits tested in order, the first that holds wins.  Evaluated as one select chain
                // in reverse order and ONE branch (six exec-mask branches cost more issue slots than the compares)
                {
                    int code = 0;
                    if (fx <= ftest1 && fabs(dg) <= KL.gtol * (-dginit)) code = count;                      // LB:862-866 (count >= 1)
                    if (KL.max_linesearch <= count) code = LBERR_MAXIMUMLINESEARCH;                         // LB:857-860
                    if (brackt && (stmax - stmin) <= KL.xtol * stmax) code = LBERR_WIDTHTOOSMALL;           // LB:852-855
                    if (step == stpmin && (ftest1 < fx || dgtest <= dg)) code = LBERR_MINIMUMSTEP;         // LB:847-850
                    if (step == stpmax && fx <= ftest1 && dg <= dgtest) code = LBERR_MAXIMUMSTEP;          // LB:842-845
                    if (brackt && ((step <= stmin || stmax <= step) || uinfo != 0)) code = LBERR_ROUNDING_ERROR;   // LB:837-840
                    if (code != 0) { ls = code; break; }
                }

                const double cmin = KL.ftol <= KL.gtol ? KL.ftol : KL.gtol;
                if (stage1 && fx <= ftest1 && cmin * dginit <= dg) stage1 = 0;

                // LB:883-920: the interval update runs on the modified function while stage1 holds and
                // the decrease is insufficient; one call site, operands selected here.
                const bool mod = stage1 && ftest1 < fx && fx <= xf;
                double axf = mod ? xf - xt * dgtest : xf, axd = mod ? xd - dgtest : xd;
                double ayf = mod ? yf - yt * dgtest : yf, ayd = mod ? yd - dgtest : yd;
                const double atf = mod ? fx - step * dgtest : fx, atd = mod ? dg - dgtest : dg;
                VIGO_TICK(t_ls);
                uinfo = trial_interval(xt, axf, axd, yt, ayf, ayd, step, atf, atd, stmin, stmax, brackt);
                VIGO_TICK(t_trial);
                xf = mod ? axf + xt * dgtest : axf;
                yf = mod ? ayf + yt * dgtest : ayf;
                xd = mod ? axd + dgtest : axd;
                yd = mod ? ayd + dgtest : ayd;

                if (brackt) {
                    if (0.66 * prev_width <= fabs(yt - xt)) step = xt + 0.5 * (yt - xt);
                    prev_width = width;
                    width = fabs(yt - xt);
                }
            }
        }

        VIGO_TICK(t_ls);
        double xnorm = sqrt(sums[5]), gnorm = sqrt(sums[6]);   // (AXIS: axis_converged() takes the roots, where it needs them)
        if (first) {
            first = false;
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int a = 0; a < D; ++a) d[q][a] = -g[q][a];  // LB:1144
            if constexpr (AXIS && VIGO_AXIS_CONV_FILTER) {
                if (axis_converged(KL, sums[6], sums[5])) { ret = LB_ALREADY_MINIMIZED; break; }
            } else {
                if (xnorm < 1.0) xnorm = 1.0;
                if (gnorm / xnorm <= KL.g_epsilon) { ret = LB_ALREADY_MINIMIZED; break; }  // LB:1154-1157
            }
            // d = -g: d.d = g.g and g.d = -(g.g) exactly (negation commutes with every rounding)
            step = 1.0 / sqrt(sums[6]);  // LB:1163
            sums[4] = -sums[6];
            k = 1;
            end = 0;
            continue;
        }

        if (ls < 0) {
            // LB:1189-1197.  optData_.controlPoints keeps the last trial (BT.cpp:803): write it
            // out now, then revert x like the reference does.
            // (AXIS: a control point that is not free is stored as it was.  The reference never writes it; here it has
            // been through xp + step * 0, which a step that is not finite turns into NaN — a failed search can end on
            // one, tests/test_gpu_solver_axis_params.py.  The other instantiations still store that NaN.)
            if constexpr (AXIS) store_point_axis(A, b, Q, grp, Q.interior[0] ? x[0][0] : xp[0][0], Q.interior[0] ? x[0][2] : xp[0][2]);
            else store_points<T, PPL>(A, b, Q, x);
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int a = 0; a < D; ++a) { x[q][a] = xp[q][a]; g[q][a] = gp[q][a]; }
            if constexpr (AXIS) x[0][2] = xp[0][2];
            ret = ls;
            break;
        }

        // convergence test, LB:1200-1225 (norms came with the last evaluation)
        if constexpr (AXIS && VIGO_AXIS_CONV_FILTER) {
            if (axis_converged(KL, sums[6], sums[5])) { ret = LB_CONVERGENCE; break; }
        } else {
            if (xnorm < 1.0) xnorm = 1.0;
            if (gnorm / xnorm <= KL.g_epsilon) { ret = LB_CONVERGENCE; break; }
        }
        if (KL.max_iterations != 0 && KL.max_iterations < k + 1) { ret = LBERR_MAXIMUMITERATION; break; }

        // s, y, ys, yy — LB:1264-1276
        T sv[PPL][3], yv[PPL][3];
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
#pragma unroll
            for (int a = 0; a < D; ++a) { sv[q][a] = x[q][a] - xp[q][a]; yv[q][a] = g[q][a] - gp[q][a]; }
            if (!REG1 && Q.interior[q]) {
                HPair<T, D> hp;
#pragma unroll
                for (int a = 0; a < D; ++a) { hp.s[a] = sv[q][a]; hp.y[a] = yv[q][a]; }
                hist_at(q, end) = hp;
            }
        }
        double ysyy[2];
        if constexpr (AXIS && VIGO_AXIS_PAIR_UPDATE) {
            ys_yy_axis(yv[0][0], sv[0][0], ysyy[0], ysyy[1]);   // the same two sums, one per half of the wave in one tree
        } else {
            ysyy[0] = dot_lane<FAST, T, PPL, D>(yv, sv);
            ysyy[1] = dot_lane<FAST, T, PPL, D>(yv, yv);
            // (level trajectory: the z product the general kernel adds here is (+0) * (+0); it turns a lane partial of -0 into
            // +0, and the sign of a zero ys decides the sign of the infinities the reference then divides into being)
            if (D <= 2) ysyy[0] += 0.0;    // (AXIS: after the exchange add, where the D = 2 kernel has it)
            group_sum<GROUP, 2>(ysyy);
        }
        const double ys = ysyy[0], yy = ysyy[1];
        // the two-loop divides by ys of each pair (LB:1300, :1312); FAST keeps its reciprocal instead
        const YS ys_div = make_ys(ys, static_cast<YS*>(nullptr));
        if (!REG1) ys_at(end) = ys_div;
        const bool haveR = REG1 && k >= RH + 1;   // sR[RH - 1] holds a pair (age RH now): it moves to the LDS ring below

        // two-loop recursion, LB:1286-1316, fully unrolled over the pair's age with a register
        // window of kWin pairs (static index age % kWin): the pair needed kWin steps ahead is
        // fetched from LDS into the window slot the current step has just consumed, so the
        // dependent chain never waits for LDS and does no address arithmetic or copies.
        const int bound = (m <= k) ? m : k;
        // !REG1: slot of the pair just stored (age 0); REG1: slot of the pair of age RH + 1 (the last one written)
        const int newest = REG1 ? last : end;
        if (!REG1) end = (end + 1 == m) ? 0 : end + 1;
        ++k;
#pragma unroll
        for (int q = 0; q < PPL; ++q)
#pragma unroll
            for (int a = 0; a < D; ++a) d[q][a] = -g[q][a];

        constexpr int kWin = 2;
        T Ps[kWin][PPL][3], Py[kWin][PPL][3];
        YS Pys[kWin];
        auto fetch = [&](int age, T (&s_)[PPL][3], T (&y_)[PPL][3], YS& ys_) {
            // (age is a literal after unrolling: the register cases fold away)
            if (REG1 && age == 0) {
#pragma unroll
                for (int q = 0; q < PPL; ++q)
#pragma unroll
                    for (int a = 0; a < D; ++a) { s_[q][a] = sv[q][a]; y_[q][a] = yv[q][a]; }
                ys_ = ys_div;
                return;
            }
            if (REG1 && age >= 1 && age <= RH) {
                const int j = (age - 1 < kRH && age >= 1) ? age - 1 : 0;
#pragma unroll
                for (int q = 0; q < PPL; ++q)
#pragma unroll
                    for (int a = 0; a < D; ++a) { s_[q][a] = sR[j][q][a]; y_[q][a] = yR[j][q][a]; }
                ys_ = ysR[j];
                return;
            }
            int slot = REG1 ? newest - (age - (RH + 1)) : newest - age;
            if (slot < 0) slot += ms;
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const HPair<T, D> h = hist_at(q, slot);
#pragma unroll
                for (int a = 0; a < D; ++a) { s_[q][a] = h.s[a]; y_[q][a] = h.y[a]; }
            }
            ys_ = ys_at(slot);
        };
        // STEADY: the history is full (bound == kMaxMem, every iteration after the 16th): `age <
        // bound` is true at compile time, so the 32 steps are straight-line code — no exec-mask
        // blocks, no merge copies of the window registers, LDS fetches hoisted freely — and the
        // alphas stay in registers.  Same operations in the same order as the general path.
        // MARK: the divisions by ys are Markstein's sequence on the stored reciprocal (over_ys); the result says whether
        // the recursion has to be repeated with true divisions (a dividend outside 2^+-500, a NaN reciprocal or a NaN in d).
        // A plain std::true_type / std::false_type tag: the steady-state recursion alone divides that way, unless FAST.
        // A TwoLoopTag (AXIS) names both.
        auto two_loop = [&](auto steady_tag) -> bool {
            constexpr bool STEADY = decltype(steady_tag)::value;
            constexpr bool MARK = two_loop_mark<FAST>(decltype(steady_tag){});
            double amin = 1.0, amax = 1.0;
            // (general path: every live lane of the wave is in the same iteration, so the number of pairs is taken
            // through an SGPR — `age < bnd` becomes a scalar branch instead of a compare + exec-mask block per step)
            const int bnd = STEADY ? kMaxMem : __builtin_amdgcn_readfirstlane(bound);
            // the alphas stay in registers: STEADY, and (AXIS) the general path as well — the indices are literals after
            // unrolling, the two paths are never live together, and al_l goes unused (the LDS layout keeps its place).
            // (Measured and left off, profiles/README.md, round 6: the AXIS general path walking the ring by running byte
            // offsets as the steady path does, wrapping at ms slots — 52 v_mul_lo_u32 fewer, and slower.)
            constexpr bool REGAL = STEADY || AXIS;
            double al_reg[REGAL ? kMaxMem : 1];
            // STEADY: the LDS ring (kMaxMem - RH - 1 slots) is walked with running byte offsets — one
            // add and a wrap per fetch instead of slot arithmetic and two quarter-rate multiplies
            constexpr int kRing = kMaxMem - (RH + 1);
            constexpr int kFirstRing = RH + 1;    // the youngest age that lives in the ring
            const int stepB = slotB;
            // (the slot index is the same in every live lane — all trajectories of a wave are in the
            // same iteration — and is taken through an SGPR so the ring walk is scalar work; the caller
            // checks the uniformity)
            const int lastU = STEADY ? __builtin_amdgcn_readfirstlane(last) : 0;
            int curB = lastU * stepB;   // slot of the pair of age RH + 1
            auto ring_fetch = [&](T (&s_)[PPL][3], T (&y_)[PPL][3], YS& ys_) {
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    const HPair<T, D> h = *reinterpret_cast<const HPair<T, D>*>(reinterpret_cast<const char*>(hl[q]) + curB);
#pragma unroll
                    for (int a = 0; a < D; ++a) { s_[q][a] = h.s[a]; y_[q][a] = h.y[a]; }
                }
                ys_ = *reinterpret_cast<const YS*>(reinterpret_cast<const char*>(ys_l) + curB);
            };
            auto ring_older = [&]() {   // towards higher ages: one slot down, wrapping
                curB -= stepB;
                if (curB < 0) curB += kRing * stepB;
            };
            auto ring_newer = [&]() {
                curB += stepB;
                if (curB >= kRing * stepB) curB -= kRing * stepB;
            };
            // the pair of age `age` (a literal after unrolling) into a window slot; the running offset relies on the two
            // loops asking for the ages in ring order.  (Measured and left off, profiles/README.md, round 3: the byte
            // offsets of the 14 ring slots by AGE worked out once per two-loop, pinned in SGPRs, and each of the 28
            // fetches taking its offset from that table by a static index, instead of this running offset stepped and
            // wrapped before every fetch (4 SALU instructions per fetch).  The step loses its 4 SALU instructions and
            // gains 4 s_nop: they had been sitting in the wait states the DPP moves of the butterfly need after the add
            // that feeds them.  +2 % at B = 1024, +3 % on the full-chip batches.)
            auto ring_fetch_age = [&](int age, bool newer_next, T (&s_)[PPL][3], T (&y_)[PPL][3], YS& ys_) {
                ring_fetch(s_, y_, ys_);
                if (newer_next) ring_newer(); else ring_older();
            };
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int a = 0; a < D; ++a) { Ps[0][q][a] = sv[q][a]; Py[0][q][a] = yv[q][a]; }
            Pys[0] = ys_div;
#pragma unroll
            for (int age = 1; age < kWin; ++age)
                if (age < bnd) {
                    // (a window of more than two pairs starts with ring slots in it: the ring pointer moves with them)
                    if (STEADY && age >= kFirstRing) ring_fetch_age(age, false, Ps[age], Py[age], Pys[age]);
                    else fetch(age, Ps[age], Py[age], Pys[age]);
                }
#pragma unroll
            for (int age = 0; age < kMaxMem; ++age) {      // newest -> oldest, LB:1294-1303
                if (age < bnd) {
                    const int w = age % kWin;
                    double al = group_sum1<GROUP>(dot_lane<FAST, T, PPL, D>(Ps[w], d));
                    al = over_ys<MARK>(al, Pys[w], amin, amax);
                    if (REGAL) al_reg[REGAL ? age : 0] = al;
                    else al_l[age * TPB] = al;         // alpha_j parks in LDS at a static offset
                    {
                        const T na = (T)(-al);     // (points that are not free hold y = 0: no select, see ROWP)
#pragma unroll
                        for (int q = 0; q < PPL; ++q)
#pragma unroll
                            for (int a = 0; a < D; ++a) d[q][a] = FAST ? fmaT(na, Py[w][q][a], d[q][a]) : d[q][a] + na * Py[w][q][a];
                    }
                    if (age + kWin < kMaxMem && age + kWin < bnd) {
                        if (STEADY && age + kWin >= kFirstRing) ring_fetch_age(age + kWin, false, Ps[w], Py[w], Pys[w]);
                        else fetch(age + kWin, Ps[w], Py[w], Pys[w]);
                    }
                }
            }
            if (STEADY) {
                // the ring pointer has gone once around (age kMaxMem == the slot of age RH + 1); the second
                // loop starts fetching at age kMaxMem - 1 - kWin.  The compiler must not keep the
                // first loop's 14 pairs alive in AGPRs for it (24 register moves per pair cost more
                // VALU slots than three ds_read_b128): LDS is declared clobbered here.
#pragma unroll
                for (int i = 0; i < kWin + 1; ++i) ring_newer();
                asm volatile("" ::: "memory");
            }
            {
                const T sc = (T)(ys / yy);  // LB:1305
#pragma unroll
                for (int q = 0; q < PPL; ++q)
#pragma unroll
                    for (int a = 0; a < D; ++a) d[q][a] *= sc;
            }
            // the window now holds the ages [max(0, bound - kWin), bound)
#pragma unroll
            for (int age = kMaxMem - 1; age >= 0; --age) {  // oldest -> newest, LB:1307-1316
                if (age < bnd) {
                    const int w = age % kWin;
                    double beta = group_sum1<GROUP>(dot_lane<FAST, T, PPL, D>(Py[w], d));
                    beta = over_ys<MARK>(beta, Pys[w], amin, amax);
                    const double cod = (REGAL ? al_reg[REGAL ? age : 0] : al_l[age * TPB]) - beta;
                    {
                        const T co = (T)cod;
#pragma unroll
                        for (int q = 0; q < PPL; ++q)
#pragma unroll
                            for (int a = 0; a < D; ++a) d[q][a] = FAST ? fmaT(co, Ps[w][q][a], d[q][a]) : d[q][a] + co * Ps[w][q][a];
                    }
                    if (age - kWin >= 0) {
                        if (STEADY && age - kWin >= kFirstRing) ring_fetch_age(age - kWin, true, Ps[w], Py[w], Pys[w]);
                        else fetch(age - kWin, Ps[w], Py[w], Pys[w]);
                    }
                }
            }
            if (!MARK) return false;
            bool bad = !(amin >= 0x1p-500) || !(amax <= 0x1p500);
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int a = 0; a < D; ++a) bad |= !(d[q][a] == d[q][a]);
            return bad;
        };
        VIGO_TICK(t_upd);
        if constexpr (AXIS) {
            // Both recursions divide with Markstein's sequence — the warm-up iterations (history not yet full) on the
            // general path — and share ONE true-division recursion, the general one, for the two-loops that report `bad`.
            bool bad;
            if (bound == kMaxMem && !__any(last != __builtin_amdgcn_readfirstlane(last))) bad = two_loop(TwoLoopTag<true, true>{});
            else bad = two_loop(TwoLoopTag<false, true>{});
            if (__any(bad)) {
                asm volatile("" ::: "memory");
                d[0][0] = -g[0][0];
                two_loop(TwoLoopTag<false, false>{});
            }
        } else if (PPL == 1 && bound == kMaxMem && !__any(last != __builtin_amdgcn_readfirstlane(last))) {
            if (__any(two_loop(std::true_type{}))) {
                // a dividend outside the range Markstein's sequence is proven for (or a NaN): the same
                // recursion again from d = -g on the general path, which divides for real
                asm volatile("" ::: "memory");
#pragma unroll
                for (int q = 0; q < PPL; ++q)
#pragma unroll
                    for (int a = 0; a < D; ++a) d[q][a] = -g[q][a];
                two_loop(std::false_type{});
            }
        } else {
            two_loop(std::false_type{});
        }
        // A coefficient that is not finite (ys = 0: the reference has no ys > 0 guard, LB:1300) turns the zero d of the
        // points that are not free into NaN (0 * inf) — and through their lanes' partials every later dot product of
        // that two-loop, which oracle/vigo_oracle.c's emulation mirrors.  Those points never move: their d is reset
        // here, once per iteration instead of in every step.
        if constexpr (AXIS)   // (lane 0 holds control point 0, which is never free; every lane of the wave is active here)
            dz = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(d[0][0])),
                                  __builtin_amdgcn_readfirstlane(__double2loint(d[0][0])));
#pragma unroll
        for (int q = 0; q < PPL; ++q)
#pragma unroll
            for (int a = 0; a < D; ++a) d[q][a] = Q.interior[q] ? d[q][a] : T(0);
        VIGO_TICK(t_two);
        if (REG1) {
            // the pair of age RH turns age RH + 1 for the next two-loop: it leaves the registers for the LDS
            // ring (overwriting the pair that would be age m); the younger ones move up by one, the new pair is age 1
            if (haveR && ms > 0) {
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    if (Q.interior[q]) {
                        HPair<T, D> hp;
#pragma unroll
                        for (int a = 0; a < D; ++a) { hp.s[a] = sR[kRH - 1][q][a]; hp.y[a] = yR[kRH - 1][q][a]; }
                        hist_at(q, end) = hp;
                    }
                }
                ys_at(end) = ysR[kRH - 1];
                last = end;
                end = (end + 1 == ms) ? 0 : end + 1;
            }
#pragma unroll
            for (int j = kRH - 1; j > 0; --j) {
#pragma unroll
                for (int q = 0; q < PPL; ++q)
#pragma unroll
                    for (int a = 0; a < D; ++a) { sR[j][q][a] = sR[j - 1][q][a]; yR[j][q][a] = yR[j - 1][q][a]; }
                ysR[j] = ysR[j - 1];
            }
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int a = 0; a < D; ++a) { sR[0][q][a] = sv[q][a]; yR[0][q][a] = yv[q][a]; }
            ysR[0] = ys_div;
        }
        sums[4] = group_sum1<GROUP>(dot_lane<FAST, T, PPL, D>(g, d));  // dginit of the next line search (LB:746)
        step = 1.0;  // LB:1321
        VIGO_TICK(t_tail);
        VIGO_TICK(t_cal);    // back-to-back: the cost of one probe
    }

    // results.  On success / convergence / iteration cap the last evaluated point is x itself.
    if (ret >= 0 || ret == LBERR_MAXIMUMITERATION) {
        if constexpr (AXIS) store_point_axis(A, b, Q, grp, x[0][0], x[0][2]);
        else store_points<T, PPL>(A, b, Q, x);
    }
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        if (Q.interior[q] && A.out_x) {
            double* dst = A.out_x + ((size_t)b * NI + (Q.p0 + q - 3)) * 3;
            if constexpr (AXIS) {   // each lane its coordinate; z as loaded, by the lane of coordinate 0
                dst[grp] = (double)x[q][0];
                if (grp == 0) dst[2] = (double)x[q][2];
            } else {
                dst[0] = (double)x[q][0]; dst[1] = (double)x[q][1]; dst[2] = (double)x[q][2];
            }
        }
    }
#if VIGO_PROFILE_SECTIONS
    if (lane % GROUP == 0 && A.out_x) {
        double* o = A.out_x + (size_t)b * NI * 3;
        o[0] = t_eval; o[1] = t_ls; o[2] = t_upd; o[3] = t_two; o[4] = t_tail; o[5] = (double)k; o[6] = (double)evals;
        o[7] = t_pre; o[8] = t_trial; o[9] = t_cal;
    }
#endif
    if (lane % (kWave / TPB) == 0) {   // the first lane of each trajectory
        if (A.out_status) A.out_status[(size_t)b * (A.status_stride ? A.status_stride : 1)] = ret;
        if (A.out_fx) A.out_fx[b] = fx;
        if (A.out_iters) A.out_iters[b] = k;
        if (A.out_evals) A.out_evals[b] = evals;
    }
