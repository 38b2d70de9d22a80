// sng_step_lean.h -- the lean step kernel (step_lean_kernel): one lane per env, N <= 16 chargers.
// Needs sng_dev_util.h (buffer access, TileStage, copy_out, wave_lds_fence), sng_dev_sums.h (pairwise_row_c)
// and sng_dev_env.h (charger_step, env_tail, StepConst, ...).  Included by sng_kernels.hip only.
#pragma once

namespace sng {

// ---------------------------------------------------------------------------------
// The lean step kernel: the one-lane, no-diagnostics, NumPy-2 / power-of-two-dt step of a station of
// N <= 16 chargers without stochastic profiles (every configuration the bench and a training loop
// run), one wavefront per 64 envs and one wavefront per workgroup (kLeanBlock), its LDS tiles its own.
// Against the general step_kernel (sng_step_general.h):
//   - the prologue is one kernarg round trip: no early exit (a wavefront past E loads env E - 1 and
//     stores nothing), no runtime branch before the loads (the requested-SoC stream is the template
//     argument REQ), and this step's table constants arrive by value (StepConst) instead of through
//     the tables pointer, so every vector load issues right after the kernel arguments land;
//   - nothing but the actions and observation tiles lives in LDS: 1/cap comes from recip_cap (no
//     per-wavefront table staging, no LDS round trip per charger);
//   - the charging / discharging totals are the running sums the lane keeps anyway whenever those
//     equal numpy's pairwise sum of the compacted arrays (charging_station.py:289-293) exactly:
//       * fewer than 8 terms: numpy sums them sequentially (loops_utils.h.src), and the skipped +0.0
//         terms leave a sum unchanged;
//       * positive powers are float32 values (the NEP 50 product pc, charger.py:92-94, when
//         charging); when the smallest of them, pmin, satisfies sum <= pmin * 2^28, every partial sum
//         is a multiple of pmin's float32 ulp below 2^53 such ulps, so every addition is exact in any
//         order.
//     Only a lane with 8 or more negative powers, or 8 or more positive ones whose sum is not
//     provably exact, compacts its powers into its LDS rows and runs the pairwise sum (rare; skipped
//     wave-uniformly otherwise).
// ---------------------------------------------------------------------------------
// Threads per workgroup of the lean step kernel: one wavefront (1,024 workgroups at E = 65,536).
// A/B on one box (day of 65,536 x 10): 64 threads 6.33-6.38 us per step, 256 threads 6.47-6.55,
// 128 threads 7.13-7.14 (library A/B: tools/diag/variant.sh builds, tools/gpu_session.sh ablib runs them).
constexpr int kLeanBlock = 64;

template <int NC>
struct LeanLds {
    static constexpr int A = NC + 1;   // actions per env with a BESS (one fewer without)
    static constexpr int O = 2 * NC + 9;
    static constexpr int ACT = round4(kWave * A), OBS = round4(kWave * O);
    static constexpr size_t WAVE_BYTES = (size_t)(ACT + OBS) * 4 + (size_t)2 * kWave * NC * 8;
    static constexpr size_t BYTES = (kLeanBlock / kWave) * WAVE_BYTES;
};

// The 64 envs of a wavefront, one per lane: their loads (issue), then their step (run), split as WideGroup
// (sng_step_wide.h) splits the wide step.  step_lean_kernel issues the state and the step's inputs together and
// runs the step; day_lean_kernel (sng_step_day.h) issues the state once a day and each step's inputs ahead of
// the step before (issue_step_inputs / take_step_inputs), runs the same step with KEEP and stores the state
// after the last one (store_state).
template <int NC, bool PK, bool REQ>
struct LeanGroup {
    using Lay = LeanLds<NC>;
    static constexpr int KT = (Lay::A * kWave + 4 * kWave - 1) / (4 * kWave);
    int64_t e0, ew;
    int nw;
    bool live;
    uint32_t el1, el4, el8;
    TileStage<KT, kWave> act_tile;
    double ratio, bess_l, pen0_l, ret_l;
    uint32_t w[NC];
    double aux[PK ? 1 : NC], run_[NC], req[NC];
    SNG_WSTAMP_DECL;   // diagnostic builds: 0 issue, 1 actions tile staged, 2 chargers, 3 env tail, 4 obs stores issued

    // the lane's env and its byte offsets: the same for every step of a day
    __device__ __forceinline__ void place(int64_t e0_, int64_t E, int lane) {
        e0 = e0_;
        const int64_t rem_e = E - e0;
        nw = rem_e <= 0 ? 0 : (rem_e < kWave ? (int)rem_e : kWave);
        live = lane < nw;
        const int64_t el = live ? e0 + lane : E - 1;   // idle lanes load a valid env and discard it
        ew = nw > 0 ? e0 : E - 1;                       // a wavefront past E stages env E - 1's row
        el1 = (uint32_t)el;
        el4 = el1 * 4u;
        el8 = el1 * 8u;
    }
    __device__ __forceinline__ void issue_tile(const float *act, int vec_io, const Params &p, int lane) {
        act_tile.issue(act + ew * p.act_dim, (nw > 0 ? nw : 1) * p.act_dim, vec_io != 0, lane);
    }
    // the SoC state's 16 B slot of the charger pair c0, c0 + 1 (sng_layout.h), or the last odd charger's 8 B
    __device__ __forceinline__ void issue_soc(int c0, int64_t E, const DeviceState &s) {
        if (c0 + 1 < NC)
            bld2(s.soc, 2u * el8, (uint32_t)c0 * (uint32_t)E * 8u, run_[c0], run_[c0 + 1]);
        else
            run_[c0] = bld(s.soc, el8, (uint32_t)c0 * (uint32_t)E * 8u);
    }
    // ... and charger c's store, with the same pairing (v: the chargers' values): the pair's 16 B slot once both
    // chargers are stepped
    __device__ __forceinline__ void store_soc(int c, int64_t E, const DeviceState &s, const double *v) {
        if (c & 1)
            bst2<kNT>(s.soc, 2u * el8, v[c - 1], v[c], (uint32_t)(c - 1) * (uint32_t)E * 8u);
        else if (c == NC - 1)
            bst<kNT>(s.soc, el8, v[c], (uint32_t)c * (uint32_t)E * 8u);
    }
    // the day kernel's state back to memory after the day's last step: every charger's SoC, the BESS SoC and
    // the day return
    __device__ __forceinline__ void store_state(int64_t E, const Params &p, const DeviceState &s, const InfoPtrs &info) {
        if (live) {
#pragma unroll
            for (int c = 0; c < NC; ++c) store_soc(c, E, s, run_);
            if (p.bess) bst<kNT>(s.bess, el8, bess_l);
            if (info.episode_return) bst<kNT>(info.episode_return, el8, ret_l);
        }
    }
    // loads oldest-needed-first, all behind the one kernarg wait: the wave's actions tile and the per-env values
    // (the LDS commit and the observation header wait for them, before any charger), then the per-charger
    // state, which charger c waits for in order.
    // STEP: what one step reads (its actions tile, records or word / aux, requested SoC); STATE: what passes
    // from step to step (PV ratio, BESS SoC, the t = 0 penalty, the day return and every charger's SoC).
    template <bool STATE = true, bool STEP = true>
    __device__ __forceinline__ void issue(int64_t e0_, const float *act, int64_t E, int t, int vec_io, const Params &p,
                                          const DeviceState &s, const InfoPtrs &info, int lane) {
        SNG_WSTAMP(0);
        place(e0_, E, lane);
        [[maybe_unused]] const size_t plane = (size_t)t * NC * (size_t)E;   // this step's timeline planes
        if constexpr (STEP) issue_tile(act, vec_io, p, lane);
        if constexpr (STATE) {
            ratio = bld(s.ratio, el8);   // pointer selects rather than branches: a disabled
            bess_l = bld(p.bess ? s.bess : s.ratio, el8);   // stream re-reads ratio
            pen0_l = bld(t == 0 ? s.pen0 : s.ratio, el8);
            ret_l = bld(info.episode_return ? info.episode_return : s.ratio, el8);
        }
        [[maybe_unused]] const uint16_t *rec_t = packed_records(s) + plane + (size_t)NC * (size_t)E;   // t + 1
#pragma unroll
        for (int c0 = 0; c0 < NC; c0 += 2) {   // charger pairs: the SoC state's 16 B slots (sng_layout.h)
            if constexpr (STEP) {
                if (PK && (c0 & 3) == 0) {   // packed device-day records (sng_layout.h), plane t + 1: a quad per 8 B
                    if (c0 + 4 <= NC) {
                        unpack_quad(bld(reinterpret_cast<const uint64_t *>(rec_t), el1 * 8u, (uint32_t)c0 * (uint32_t)E * 2u), w + c0);
                    } else {
#pragma unroll
                        for (int c = c0; c < NC; ++c) {
                            const RecOff ro = rec_off(c, NC, E, el1);
                            w[c] = bld16(rec_t, ro.v, ro.s);
                        }
                    }
                }
#pragma unroll
                for (int c = c0; c < c0 + 2 && c < NC; ++c) {
                    const uint32_t r4 = (uint32_t)c * (uint32_t)E * 4u, r8 = 2u * r4;   // charger row
                    if (!PK) {
                        w[c] = bld(s.word + plane, el4, r4);
                        aux[PK ? 0 : c] = bld(s.aux + plane, el8, r8);
                    }
                }
            }
            if constexpr (STATE) issue_soc(c0, E, s);
            // the requested SoC at python index t-1, or its default without the stream
            if constexpr (STEP) {
#pragma unroll
                for (int c = c0; c < c0 + 2 && c < NC; ++c)
                    req[c] = REQ ? bld(s.req + plane, el8, (uint32_t)c * (uint32_t)E * 8u) : req_default(p);
            }
        }
    }
    // One step's inputs, for the day kernel: the actions tile into act_tile, the step's records as they lie in
    // memory (whole quads and the partial quad's u16s: rq, rl) or its word and aux planes, the requested SoC,
    // and the step's table constants (uniform loads through s.tables: a per-launch StepConst cannot carry T
    // steps).  They wait in registers of their own until take_step_inputs, once the step before has read its.
    static constexpr int NQ = PK ? NC / 4 : 0, NR = PK ? NC % 4 : 0;
    uint64_t rq[NQ ? NQ : 1];
    uint32_t rl[NR ? NR : 1];
    uint32_t wn[PK ? 1 : NC];
    double auxn[PK ? 1 : NC], reqn[REQ ? NC : 1];
    StepConst kn;
    __device__ __forceinline__ void issue_step_inputs(const float *act, int64_t E, int t, int vec_io, const Params &p,
                                                      const DeviceState &s, int lane) {
        const size_t plane = (size_t)t * NC * (size_t)E;
        [[maybe_unused]] const uint16_t *rec_t = packed_records(s) + plane + (size_t)NC * (size_t)E;   // t + 1, as issue()
#pragma unroll
        for (int i = 0; i < CST_COUNT; ++i) kn.v[i] = step_constant(s.tables, t, i);
        issue_tile(act, vec_io, p, lane);
        if constexpr (PK) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                rq[q] = bld(reinterpret_cast<const uint64_t *>(rec_t), el1 * 8u, (uint32_t)(4 * q) * (uint32_t)E * 2u);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const RecOff ro = rec_off(4 * NQ + r, NC, E, el1);
                rl[r] = bld16(rec_t, ro.v, ro.s);
            }
        } else {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const uint32_t r4 = (uint32_t)c * (uint32_t)E * 4u, r8 = 2u * r4;
                wn[c] = bld(s.word + plane, el4, r4);
                auxn[c] = bld(s.aux + plane, el8, r8);
            }
        }
        if constexpr (REQ) {
#pragma unroll
            for (int c = 0; c < NC; ++c) reqn[c] = bld(s.req + plane, el8, (uint32_t)c * (uint32_t)E * 8u);
        }
    }
    __device__ __forceinline__ void take_step_inputs(const Params &p) {
        if constexpr (PK) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) unpack_quad(rq[q], w + 4 * q);
#pragma unroll
            for (int r = 0; r < NR; ++r) w[4 * NQ + r] = rl[r];
        } else {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                w[c] = wn[c];
                aux[PK ? 0 : c] = auxn[PK ? 0 : c];
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) req[c] = REQ ? reqn[REQ ? c : 0] : req_default(p);
    }

    // the wavefront's step; s_act holds its actions tile (committed), s_obs is its observation tile, s_pos /
    // s_neg its rows for the slow sums.  KEEP (the day kernel): what the next step of the same env would load
    // straight back stays in registers -- every charger's new SoC in run_[], the BESS SoC in bess_l, the day
    // return in ret_l -- and the caller stores it after the day's last step (store_state); every other output
    // is stored as always.
    template <bool KEEP = false>
    __device__ __forceinline__ void run(const float *s_act, float *s_obs, double *s_pos, double *s_neg, float *obs,
                                        double *reward, uint8_t *done, int64_t E, int t, int vec_io, const StepConst &k,
                                        const Params &p, const DeviceState &s, const InfoPtrs &info, int lane) {
        SNG_WSTAMP(1);
        const int Ad = p.act_dim, O = p.obs_dim;
        const float *a_row = s_act + lane * Ad;
        float *o_row = s_obs + lane * O;
        float av[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) av[c] = a_row[c];
        const float bess_action = p.bess ? a_row[NC] : 0.0f;
        const int k_soc = p.pv ? 8 : 4;
        const double one4[4] = {1.0, 1.0, 1.0, 1.0};
        // the header needs only the PV ratio and the constants: written while the chargers' loads fly
        if (live) write_obs_header(o_row, p, k.v + CST_IRR, k.v + CST_PN, ratio, one4, one4);
        // KEEP: the BESS step needs only per-env values too, and its new SoC stays with the caller
        [[maybe_unused]] BessStep bs{};
        if constexpr (KEEP) {
            if (live) {
                bs = bess_step<false>(p, s, el8, t, p.bess ? bess_l : 0.0, bess_action);
                if (p.bess) o_row[O - 1] = (float)bs.bess;
            }
        }

        double pwv[NC], sv[NC];
        double pen_v = 0.0, seq_pos = 0.0, seq_neg = 0.0, pmin = __builtin_inf();
        int n_pos = 0, n_neg = 0;
        uint32_t n_nonexist = 0, fl = 0;
        bool pos_other = false;   // a positive power that is not the float32 charging product
        if (live) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const ChargerVisit<PK> v = visit_charger<true, false, PK>(p, w[c], aux[PK ? 0 : c], run_[c], req[c], av[c], t);
                const ChargerResult &r = v.r;
                sv[c] = v.soc;
                if constexpr (KEEP) run_[c] = sv[c];
                else store_soc(c, E, s, sv);   // the pair's 16 B slot once both chargers are stepped
                o_row[k_soc + c] = v.obs_soc();
                o_row[k_soc + NC + c] = v.obs_dep();
                n_nonexist += r.nx;
                fl |= r.fl;
                pen_v += r.q;
                const double pw = r.pw;
                pwv[c] = pw;
                const bool ip = pw > 0.0;
                seq_pos += __builtin_fmax(pw, 0.0);   // v_max/v_min drop a NaN power, as P[P > 0] does
                seq_neg += __builtin_fmin(pw, 0.0);
                n_pos += ip ? 1 : 0;
                n_neg += (pw < 0.0) ? 1 : 0;
                pmin = __builtin_fmin(pmin, ip ? pw : __builtin_inf());
                pos_other |= ip && !(av[c] > 0.0f);
                // chargers in order: charger c waits only for its own loads (vmcnt counts down charger
                // by charger) while the later chargers' loads are in flight
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        SNG_WSTAMP(2);
        double p_ch = seq_pos, p_dis = seq_neg;
        if constexpr (NC >= 8) {
            const bool pos_slow = n_pos >= 8 && (pos_other || !(seq_pos <= pmin * 0x1.0p28));
            const bool slow = live && (pos_slow || n_neg >= 8);
            if (__builtin_amdgcn_ballot_w64(slow)) {   // wave-uniform: rare
                if (slow) {
                    double *row_pos = s_pos + lane * NC, *row_neg = s_neg + lane * NC;
                    int kp = 0, kn_ = 0;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        row_pos[kp] = pwv[c];
                        row_neg[kn_] = pwv[c];
                        kp += (pwv[c] > 0.0) ? 1 : 0;
                        kn_ += (pwv[c] < 0.0) ? 1 : 0;
                    }
                    p_ch = pairwise_row_c<NC>(row_pos, n_pos, seq_pos);
                    p_dis = pairwise_row_c<NC>(row_neg, n_neg, seq_neg);
                }
            }
        }
        if (live) {
            // t = 0 reads the python index -1 slot (pen0); the per-charger terms are all 0 there
            pen_v += (t == 0) ? pen0_l : 0.0;
            if constexpr (KEEP) {
                env_tail<false, true, true>(p, s, info, e0, (uint32_t)lane, el1, el8, t, ratio, p.bess ? bess_l : 0.0,
                                            bess_action, p_ch, p_dis, pen_v, 100.0 * (double)n_nonexist, fl, o_row, k.v,
                                            one4, one4, info.episode_return ? ret_l : 0.0, 0.0, reward, done, &bs, &ret_l);
                bess_l = bs.bess;
            } else {
                env_tail<false>(p, s, info, e0, (uint32_t)lane, el1, el8, t, ratio, p.bess ? bess_l : 0.0, bess_action,
                                p_ch, p_dis, pen_v, 100.0 * (double)n_nonexist, fl, o_row, k.v, one4, one4,
                                info.episode_return ? ret_l : 0.0, 0.0, reward, done);
            }
        }
        wave_lds_fence();
        SNG_WSTAMP(3);
        if (nw > 0) copy_out<kWave>(obs + e0 * O, s_obs, nw * O, vec_io != 0, lane);
        SNG_WSTAMP(4);
    }
};

// The wavefront's LDS: its actions tile, its observation tile and its two rows per lane for the slow sums.
template <int NC>
struct LeanTiles {
    float *s_act, *s_obs;
    double *s_pos, *s_neg;
    __device__ __forceinline__ LeanTiles(float *lds, int wave) {
        using Lay = LeanLds<NC>;
        s_act = reinterpret_cast<float *>(reinterpret_cast<char *>(lds) + wave * Lay::WAVE_BYTES);
        s_obs = s_act + Lay::ACT;
        s_pos = reinterpret_cast<double *>(s_obs + Lay::OBS);
        s_neg = s_pos + kWave * NC;
    }
};

template <int NC, bool PK, bool REQ>
__global__ __launch_bounds__(kLeanBlock) void step_lean_kernel(const float *__restrict__ act, float *__restrict__ obs,
                                                        double *__restrict__ reward, uint8_t *__restrict__ done,
                                                        int64_t E, int t, int vec_io, StepConst k, Params p,
                                                        DeviceState s, InfoPtrs info) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
    const LeanTiles<NC> tl(lds, wave);
    LeanGroup<NC, PK, REQ> g;
    g.issue((int64_t)blockIdx.x * kLeanBlock + (int64_t)wave * kWave, act, E, t, vec_io, p, s, info, lane);
    g.act_tile.commit(tl.s_act, lane);
    wave_lds_fence();
    g.run(tl.s_act, tl.s_obs, tl.s_pos, tl.s_neg, obs, reward, done, E, t, vec_io, k, p, s, info, lane);
    SNG_WSTAMP_FLUSH(g.stamp_, 5);
    // a device-RNG day's first step advances the day counter its reset read (generate_kernel); no-return
    // atomic, so nothing waits for it.  A replayed day (bump_day = 0) drew no counter value of its own.
    bump_day_counter<PK>(p, s, t);
}

}  // namespace sng
