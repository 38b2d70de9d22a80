// sng_step_general.h -- the general step kernel (step_kernel): every station size (a runtime N too), one, two
// or four lanes per env, the per-step diagnostics, NumPy < 2 promotion and any dt; what a plan falls back to
// when neither the lean nor the wide kernel covers it (sng_step_plan.h).
// Needs sng_dev_util.h (buffer access, TileStage, copy_out, wave_lds_fence), sng_dev_sums.h and
// sng_dev_env.h (charger_step, env_tail, step_constant, ...).  Included by sng_kernels.hip only.
#pragma once

namespace sng {

// Workgroup size of the step kernel: 256 threads (4 wavefronts, 4x fewer workgroups to
// dispatch) while the LDS staging fits, one wavefront for wide stations (N > 16 or runtime N)
// so the [ENVS][O] observation tile stays well inside the 160 KB LDS.
__host__ __device__ constexpr int step_block(int NC) { return (NC > 0 && NC <= 16) ? 256 : 64; }

// LDS carve-up of the step kernel, one slice per wavefront (every region 16-byte aligned):
//   act [WENVS][A] f32 | obs [WENVS][O] f32 | (kRows) rcp [256] f64 | (kRows) cst [16] f64
//   | pos [WENVS][NC] f64 | neg [WENVS][NC] f64 | (L > 1) pw [WENVS][NC] f64
// With L > 1 the penalty rows q [WENVS][NC] f64 share the first region with the actions tile:
// a lane's chargers are one batch, whose action reads all precede the first q write in the
// wavefront's program order (the BESS action is read before the loop).
// Each wavefront stages, computes and writes back its own 64/L envs: no workgroup barrier, so
// the waves of a CU drift apart and one wave's loads overlap another's arithmetic and stores.
template <int NC, int L>
struct StepLds {
    static constexpr int BLOCK = step_block(NC);
    static constexpr int WAVES = BLOCK / kWave;
    static constexpr int WENVS = kWave / L;              // envs per wavefront
    static constexpr int ENVS = WAVES * WENVS;           // envs per workgroup
    static constexpr bool kRows = NC > 0 && NC <= 16;   // compacted power rows (else PairwiseSum)
    __host__ __device__ static int act_floats(int A) { return round4(WENVS * A); }
    __host__ __device__ static int obs_floats(int O) { return round4(WENVS * O); }
    // wide stations (!kRows) keep no 1/c table and no step constants in LDS: at N = 50 the act
    // and obs tiles alone are 40 KB per wavefront, and 40 KB is what lets 4 wavefronts (one per
    // SIMD) share a CU's 160 KB
    __host__ __device__ static size_t first_bytes(int A) {   // actions tile, or the q rows aliasing it
        const size_t a = (size_t)act_floats(A) * 4, q = L > 1 ? (size_t)WENVS * NC * 8 : 0;
        return a > q ? a : q;
    }
    __host__ __device__ static size_t wave_bytes(int A, int O) {
        size_t b = first_bytes(A) + (size_t)obs_floats(O) * 4;
        if (kRows) b += (size_t)(256 + 16) * 8 + (size_t)2 * WENVS * NC * 8;
        if (L > 1) b += (size_t)WENVS * NC * 8;
        return b;
    }
    __host__ __device__ static size_t bytes(int A, int O) { return WAVES * wave_bytes(A, O); }
};

// Chargers per batch of the one-lane step kernel: all of them up to 16; for wider stations the
// largest divisor of N in [10, 16] (no ragged last batch), else 8 -- each batch's loads are issued
// together and then consumed.  Measured at N = 50 (config 5): batches of 10 33.1 us per step, 17
// 33.5, 25 34.5, 13 36.8, 8 39.1.
__host__ __device__ constexpr int wide_batch(int NC) {
    if (NC > 0 && NC <= 16) return NC;
    for (int d = 16; d >= 10; --d)
        if (NC > 0 && NC % d == 0) return d;
    return 8;
}

// ---------------------------------------------------------------------------------
// The fused step: SmartNanogridEnv.step(actions) for BLOCK/L envs per workgroup.
// NC   = compile-time charger count (0: runtime p.n, L must be 1);
// L    = lanes per env;
// DIAG = also write the per-step diagnostics (SngInfo arrays).
// Every per-charger load of a lane's batch is issued before any of it is used, and the first
// batch before the action staging wait, so one lane keeps 3*CH + 2 requests in flight.
// ---------------------------------------------------------------------------------
// One wavefront per SIMD at the bench's population (1,024 waves), so the kernel may use the whole register
// file: amdgpu_waves_per_eu(1, 1) lets the wide stations' prefetched batch live in registers (at the
// default two waves per SIMD the compiler spilled it to scratch).
template <int NC, int L, bool DIAG, bool FAST, bool PK>
__global__ __launch_bounds__(step_block(NC)) __attribute__((amdgpu_waves_per_eu(1, 1))) void step_kernel(
    Params p, DeviceState s, InfoPtrs info,
                                                              const float *__restrict__ act, float *__restrict__ obs,
                                                              double *__restrict__ reward, uint8_t *__restrict__ done,
                                                              int64_t E, int t, int vec_io) {
    static_assert(L == 1 || NC > 0, "multi-lane envs need a compile-time charger count");
    using Lay = StepLds<NC, L>;
    constexpr int WENVS = Lay::WENVS;
    constexpr bool kRows = Lay::kRows;
    constexpr int CH = (L > 1) ? (NC + L - 1) / L : wide_batch(NC);
    // actions tile in one round: K float4 per lane covers WENVS * A floats for A <= NC + 1
    constexpr int KT = NC > 0 ? ((NC + 1) * WENVS + 4 * kWave - 1) / (4 * kWave) : 8;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int n = NC ? NC : p.n;
    const int A = p.act_dim, O = p.obs_dim;
    // the wavefront index is wave-uniform: readfirstlane keeps e0 and the row offsets scalar
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
    const int le = lane / L, part = lane % L;
    const int64_t e0 = (int64_t)blockIdx.x * Lay::ENVS + (int64_t)wave * WENVS;   // this wave's first env
    if (e0 >= E) return;                                                           // wave-uniform
    const int nw = (int)((E - e0) < WENVS ? (E - e0) : WENVS);
    const int64_t e = e0 + le;
    const bool live = le < nw;
    const bool leader = part == 0;
    float *s_act = reinterpret_cast<float *>(reinterpret_cast<char *>(lds) + wave * Lay::wave_bytes(A, O));
    float *s_obs = reinterpret_cast<float *>(reinterpret_cast<char *>(s_act) + Lay::first_bytes(A));
    double *s_rcp = reinterpret_cast<double *>(s_obs + Lay::obs_floats(O));   // [256] 1/c (kRows)
    double *s_cst = s_rcp + (kRows ? 256 : 0);                    // [16] per-step constants (kRows)
    double *s_pos = s_cst + (kRows ? 16 : 0);                     // [WENVS][NC] compacted positive powers
    double *s_neg = s_pos + (kRows ? WENVS * NC : 0);             // [WENVS][NC] compacted negative powers
    double *s_pw = s_neg + (kRows ? WENVS * NC : 0);              // [WENVS][NC] per-charger powers (L > 1)
    double *s_q = reinterpret_cast<double *>(s_act);              // [WENVS][NC] penalty terms (L > 1)
    const uint32_t *__restrict__ word = s.word;
    const double *__restrict__ auxv = s.aux;
    const double *__restrict__ reqv = s.req;
    double *__restrict__ socv = s.soc;
    const size_t tbase = (size_t)t * n;
    const int cbeg = (L > 1) ? part * CH : 0;
    const int cend = (L > 1) ? ((cbeg + CH) < n ? (cbeg + CH) : n) : n;

    // Loads are issued oldest-needed-last: everything the LDS commits wait for (tables, actions
    // tile) is issued after the conditional loads and before the per-charger state, and no
    // branch separates it from the per-charger loads, so the wait before the commits is
    // vmcnt(#per-charger loads) and charger c's update starts as soon as its own loads land.
    // Non-live lanes load a valid env (E - 1) and discard it.
    const int64_t el = live ? e : E - 1;
    const uint32_t lo = (uint32_t)(el - e0);   // lane offset from the wave's first env
    const uint32_t el1 = (uint32_t)el, el4 = el1 * 4u, el8 = el1 * 8u;   // byte offsets of the env
    const uint32_t *__restrict__ word_t = word + tbase * (size_t)E;   // this step's timeline planes
    const double *__restrict__ aux_t = auxv + tbase * (size_t)E;
    // a packed day's records: plane t + 1 (sng_layout.h)
    const uint16_t *__restrict__ rec_t = packed_records(s) + (tbase + n) * (size_t)E;
    const double *__restrict__ req_t = reqv + tbase * (size_t)E;
    uint32_t w[CH];
    double aux[CH], run[CH], req[CH];
    auto load_state = [&](int c0) {
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int c = c0 + j;
            if (c < cend) {
                const uint32_t r4 = (uint32_t)c * (uint32_t)E * 4u, r8 = 2u * r4;   // charger row
                if (PK) {   // packed device-day record (sng_layout.h)
                    const RecOff ro = rec_off(c, n, E, el1);
                    w[j] = bld16(rec_t, ro.v, ro.s);
                } else {
                    w[j] = bld(word_t, el4, r4);
                    aux[j] = bld(aux_t, el8, r8);
                }
                const SocOff so = soc_off(c, n, E, el8);   // the SoC state in charger pairs
                run[j] = bld(socv, so.v, so.s);
            } else {
                w[j] = 0u;
                aux[j] = run[j] = 0.0;
            }
        }
    };
    auto load_req = [&](int c0) {
        if (p.req_stream && !p.req_zero) {
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                const int c = c0 + j;
                req[j] = (c < cend) ? bld(req_t, el8, (uint32_t)c * (uint32_t)E * 8u) : 1.0;
            }
        } else {
            const double rq = req_default(p);
#pragma unroll
            for (int j = 0; j < CH; ++j) req[j] = rq;
        }
    };
    auto load_batch = [&](int c0) {
        load_req(c0);
        load_state(c0);
    };
    // Wide single-lane stations (several batches): batch b + 1's loads are issued before batch b is
    // computed, so they land while it computes instead of after it (the loop is not unrolled: the
    // prefetched registers are copied into the batch's at the top of the next iteration).
    constexpr bool kPF = (L == 1) && !kRows && (NC > 0) && (CH < NC) && (NC % CH == 0);
    constexpr int PFN = kPF ? CH : 1;
    uint32_t wn[PFN];
    double auxn[PFN], runn[PFN], reqn[PFN];
    auto load_next = [&](int c0) {
        if constexpr (kPF) {
            const bool rq_live = p.req_stream && !p.req_zero;
            const double rq = req_default(p);
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                const int c = c0 + j;
                const uint32_t r4 = (uint32_t)c * (uint32_t)E * 4u, r8 = 2u * r4;   // charger row
                if (PK) {
                    const RecOff ro = rec_off(c, n, E, el1);
                    wn[j] = bld16(rec_t, ro.v, ro.s);
                } else {
                    wn[j] = bld(word_t, el4, r4);
                    auxn[j] = bld(aux_t, el8, r8);
                }
                const SocOff so = soc_off(c, n, E, el8);
                runn[j] = bld(socv, so.v, so.s);
                reqn[j] = rq_live ? bld(req_t, el8, r8) : rq;
            }
        }
    };

    // 1. per-env values: pointer selects rather than branches (a disabled stream re-reads ratio)
    const double ratio = bld(s.ratio, el8);
    const double bess_l = bld(p.bess ? s.bess : s.ratio, el8);
    const double pen0_l = bld(t == 0 ? s.pen0 : s.ratio, el8);
    const double ret_l = bld(info.episode_return ? info.episode_return : s.ratio, el8);
    const double bess0 = DIAG ? bld((p.bess && t > 0 && info.bess_initial) ? s.bess0 : s.ratio, el8) : 0.0;
    const double bess = p.bess ? bess_l : 0.0;
    const double pen0 = (t == 0) ? pen0_l : 0.0;
    const double ret_prev = info.episode_return ? ret_l : 0.0;
    // 2. requested SoC of the first batch and the day's profile factors for t..t+3 (uniform
    //    branches, ahead of the tile)
    load_req(cbeg);
    double fpv[4] = {1.0, 1.0, 1.0, 1.0}, fpr[4] = {1.0, 1.0, 1.0, 1.0};
    if (p.noise) profile_factors(p, s, el8, t, fpv, fpr);
    // 3. tables and the wave's actions tile
    //    (wide stations: no 1/c table, the step constants in scalar registers -- see StepLds)
    constexpr int RCP_PER_LANE = kRows ? 256 / kWave : 0;
    double rcp_v[RCP_PER_LANE > 0 ? RCP_PER_LANE : 1];
#pragma unroll
    for (int k = 0; k < RCP_PER_LANE; ++k) rcp_v[k] = s.tables->recip[k * kWave + lane];
    const double cst_v = (kRows && lane < CST_COUNT) ? step_constant(s.tables, t, lane) : 0.0;
    double cst_r[CST_COUNT];
    if (!kRows) {
#pragma unroll
        for (int i = 0; i < CST_COUNT; ++i) cst_r[i] = step_constant(s.tables, t, i);   // uniform: s_load
    }
    TileStage<KT, kWave> act_tile;
    act_tile.issue(act + e0 * A, nw * A, vec_io != 0, lane);
    // 4. per-charger state of the first batch
    load_state(cbeg);
#pragma unroll
    for (int k = 0; k < RCP_PER_LANE; ++k) s_rcp[k * kWave + lane] = rcp_v[k];
    if (kRows && lane < CST_COUNT) s_cst[lane] = cst_v;
    const double *cst = kRows ? s_cst : cst_r;
    act_tile.commit(s_act, lane);
    wave_lds_fence();

    const float *a_row = s_act + le * A;
    float *o_row = s_obs + le * O;
    const float bess_action = p.bess ? a_row[n] : 0.0f;   // before the q rows reuse the tile
    const int k_soc = (p.pv ? 8 : 4);
    // the observation header needs only the PV ratio and this step's constants: written here,
    // while the chargers' loads are still in flight, instead of at the end of the env tail
    if (live && leader) write_obs_header(o_row, p, cst + CST_IRR, cst + CST_PN, ratio, fpv, fpr);
    PairwiseSum pos, neg;
    double seq_pos = 0.0, seq_neg = 0.0;
    int n_pos = 0, n_neg = 0;
    double *row_pos = s_pos + le * NC, *row_neg = s_neg + le * NC;
    if (!kRows) {
        pos.init();
        neg.init();
    }
    // one power into the pairwise-sum state (numpy order: compacted array of positives/negatives).
    // Rows: unconditional LDS stores at the current count (a slot is overwritten until its element
    // is kept) and select-based counters, so nothing here is addressed through a pointer select.
    auto add_power = [&](double pw) {
        if (kRows) {
            const bool ip = pw > 0.0, in = pw < 0.0;
            row_pos[n_pos] = pw;
            row_neg[n_neg] = pw;
            // + max(pw, 0) / + min(pw, 0): adds the kept element, or a zero that leaves the running
            // sum exactly unchanged (v_max/v_min return the non-NaN operand: a NaN power is
            // dropped, as numpy's P[P > 0] drops it)
            seq_pos += __builtin_fmax(pw, 0.0);
            seq_neg += __builtin_fmin(pw, 0.0);
            n_pos += ip ? 1 : 0;
            n_neg += in ? 1 : 0;
        } else {
            if (pw > 0.0) pos.push(pw);
            if (pw < 0.0) neg.push(pw);
        }
    };
    double pen_v = 0.0;
    uint32_t n_nonexist = 0;
    uint32_t fl = 0;
    if (live) {
        for (int c0 = cbeg; c0 < cend; c0 += CH) {
            if constexpr (kPF) {   // NC % CH == 0: every batch is full
                if (c0 != cbeg) {
#pragma unroll
                    for (int j = 0; j < CH; ++j) {
                        w[j] = wn[j];
                        if (!PK) aux[j] = auxn[j];
                        run[j] = runn[j];
                        req[j] = reqn[j];
                    }
                }
                if (c0 + CH < cend) load_next(c0 + CH);
            } else if (c0 != cbeg) {
                load_batch(c0);
            }
            // the batch's actions ahead of the LDS writes below (they issue back to back)
            float av[CH];
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                const int c = c0 + j;
                av[j] = (c < cend) ? a_row[c] : 0.0f;
            }
            if (L > 1) wave_lds_fence();   // the q rows below reuse the actions tile
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                const int c = c0 + j;
                if (c >= cend) break;
                // 1/cap from the LDS table here, not ahead with the actions: it needs charger j's
                // record, and reading every record's up front waited for all of them
                // (wide stations: recip_cap instead of the LDS table, exact all the same -- div_by_cap)
                const ChargerVisit<PK> v =
                    visit_charger<FAST, false, PK, kRows>(p, w[j], aux[j], run[j], req[j], av[j], t, s_rcp);
                const ChargerResult &r = v.r;
                const SocOff so = soc_off(c, n, E, el8);
                bst<kNT>(socv, so.v, v.soc, so.s);
                if (DIAG) {   // 'Charger power values' and the SOC[c, t] the day record holds
                    if (info.charger_power) info.charger_power[(size_t)e * n + c] = r.pw;
                    if (info.vehicle_soc) info.vehicle_soc[(size_t)e * n + c] = r.soc;
                }
                o_row[k_soc + c] = v.obs_soc();
                o_row[k_soc + n + c] = v.obs_dep();
                n_nonexist += r.nx;
                fl |= r.fl;
                if (L == 1) {
                    pen_v += r.q;
                    add_power(r.pw);
                } else {
                    s_pw[le * NC + c] = r.pw;
                    s_q[le * NC + c] = r.q;
                }
                // chargers in order: charger j's arithmetic waits only for its own loads
                // (vmcnt counts down charger by charger) and overlaps the later chargers' loads;
                // left to interleave them, the scheduler hoisted work that waited for all loads
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if (L > 1) {
        // gather the env's lanes (same wavefront): counts and flag bits, then in-order
        // penalty / power sums by the leader from LDS
#pragma unroll
        for (int off = 1; off < L; off <<= 1) {
            n_nonexist += (uint32_t)__shfl_down((int)n_nonexist, off, L);
            fl |= (uint32_t)__shfl_down((int)fl, off, L);
        }
        wave_lds_fence();
        if (live && leader) {
            if (kRows) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    pen_v += s_q[le * NC + c];
                    add_power(s_pw[le * NC + c]);
                }
            } else {
                // wide stations: compact in place -- positives into the power row, negatives into
                // the penalty row; slot k <= c has been read before it is rewritten at step c
                double *pw_row = s_pw + le * NC, *q_row = s_q + le * NC;
#pragma unroll 10
                for (int c = 0; c < NC; ++c) {
                    const double qv = q_row[c], v = pw_row[c];
                    pen_v += qv;
                    pw_row[n_pos] = v;
                    q_row[n_neg] = v;
                    seq_pos += __builtin_fmax(v, 0.0);
                    seq_neg += __builtin_fmin(v, 0.0);
                    n_pos += (v > 0.0) ? 1 : 0;
                    n_neg += (v < 0.0) ? 1 : 0;
                }
            }
        }
    }
    if (live && leader) {
        // t = 0 reads the python index -1 slot (pen0); every per-charger term is 0 there, and
        // adding +0.0 / adding to +0.0 is exact, so this equals the reference's choice of sum
        pen_v += pen0;
        double p_ch, p_dis;
        if (kRows) {
            constexpr int W = (NC > 0 && NC <= 16) ? NC : 1;   // kRows: NC in [1, 16]
            p_ch = pairwise_row_c<W>(row_pos, n_pos, seq_pos);
            p_dis = pairwise_row_c<W>(row_neg, n_neg, seq_neg);
        } else if (L > 1) {
            p_ch = pairwise_row(s_pw + le * NC, n_pos, seq_pos);
            p_dis = pairwise_row(s_q + le * NC, n_neg, seq_neg);
        } else {
            p_ch = pos.result();
            p_dis = neg.result();
        }
        env_tail<DIAG>(p, s, info, e0, lo, el1, el8, t, ratio, bess, bess_action, p_ch, p_dis, pen_v,
                       100.0 * (double)n_nonexist, fl,
                       o_row, cst, fpv, fpr, ret_prev, bess0, reward, done);
    }
    wave_lds_fence();
    copy_out<kWave>(obs + e0 * O, s_obs, nw * O, vec_io != 0, lane);
    // a device-RNG day's first step advances the day counter its reset read (generate_kernel);
    // nothing in this launch reads it (done last: at the top it perturbed the prologue's schedule).
    // A replayed day (bump_day = 0) drew no counter value of its own.
    bump_day_counter<PK>(p, s, t);
}

}  // namespace sng
