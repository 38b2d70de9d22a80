// sng_step_wide.h -- the wide lean step kernel (step_wide_kernel): two lanes per env, every charger's state in
// registers; the headline station (N = 10) and config 5 (N = 50).
// Needs sng_dev_util.h (buffer access, TileStage, copy_out, wave_lds_fence), sng_dev_sums.h
// (PairwiseSum) and sng_dev_env.h (charger_step, bess_step, env_tail, StepConst, ...).  Included by
// sng_kernels.hip only.
#pragma once

namespace sng {

// ---------------------------------------------------------------------------------
// The wide lean step kernel: step_lean_kernel's recipe for stations wider than 16 chargers (BASELINE
// config 5: N = 50, 15-minute steps, stochastic PV / price profiles), one wavefront per 64 envs, one
// wavefront per workgroup, one wavefront per SIMD at E = 65,536 (so the whole 512-entry register file:
// every charger's state is loaded up front).  What makes it lean at N = 50:
//   - the charging total is the running sum whenever that equals numpy's pairwise sum of the compacted
//     positive powers exactly (step_lean_kernel's argument: fewer than 8 terms, or float32 powers whose
//     sum stays below 2^28 times the smallest), instead of numpy's 8-accumulator schedule fed one
//     power at a time (PairwiseSum: ~40 VALU per power, two per charger);
//   - the discharging total is exactly 0.0 (numpy's sum of an empty array) when no action of the wave is
//     negative: a negative power needs a negative action (charger.py:37-56, 108-140), and then no power
//     is positive other than a charging product.  A wavefront with a negative action (V2X) takes the
//     general order, PairwiseSum over both signs, in a rolled loop that re-reads each charger's inputs
//     (rare: nothing in the fast loop indexes the register arrays at run time);
//   - a lane whose positive sum is not provably exact rebuilds its compacted positive powers from what
//     the step leaves unchanged -- the records (occupancy) and the actions tile (the float32 product
//     charger.py:92-94) -- and sums them in numpy's order (rare);
//   - constants by value, one kernarg round trip before the loads, 1/cap by recip_cap, no LDS but the
//     actions and observation tiles (40 KB per wavefront: four per CU).
// ---------------------------------------------------------------------------------

// What day_station_kernel hands its step besides the StepConst (WideGroup::run<KEEP, STATION>).
struct StationStep {
    float pnf[4];            // (float)price_norm[t .. t + 3]: the observation's four price entries, the same for every env
    const uint16_t *rec_t;   // record plane t + 1
};

template <int NC, int L>
struct WideLds {
    static constexpr int WENVS = kWave / L;   // envs per wavefront
    static constexpr int A = NC + 1;          // actions per env with a BESS (one fewer without)
    static constexpr int O = 2 * NC + 9;
    static constexpr int ACT = round4(WENVS * A), OBS = round4(WENVS * O);
    static constexpr size_t BYTES = (size_t)(ACT + OBS) * 4;
};

// Lane `part` K's value of an env's two adjacent lanes, for the env's first lane, by DPP quad permutation (a
// quad holds two envs: lanes 0-1 and 2-3).
template <int K>
__device__ __forceinline__ uint32_t from_part(uint32_t x) {
    constexpr int ctrl = K | (K << 2) | ((K + 2) << 4) | ((K + 2) << 6);
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, ctrl, 0xF, 0xF, false);
}
template <int K>
__device__ __forceinline__ double from_part(double x) {
    const uint64_t b = __builtin_bit_cast(uint64_t, x);
    const uint64_t lo = from_part<K>((uint32_t)b), hi = from_part<K>((uint32_t)(b >> 32));
    return __builtin_bit_cast(double, lo | (hi << 32));
}

// The WENVS = 32 envs of a wavefront: their loads (issue), then their step (run).  step_wide_kernel, below,
// says how the two lanes of an env share its chargers.
template <int NC, int L, bool PK, bool REQ, bool NOISE>
struct WideGroup {
    using Lay = WideLds<NC, L>;
    // The one supported shape: two lanes per env and N = 2 mod 8 (the headline's 10, config 5's 50).  Lane
    // `part` steps the chargers [part H, part H + H) (H = (N - 2) / 2, a multiple of 4) and charger
    // N - 2 + part of the last pair, so its SoC state moves as whole 16 B charger pairs and its records as whole
    // 8 B quads (sng_layout.h) but for that last charger: 8 B of the last pair, 2 B of the partial quad.
    static_assert(L == 2 && NC % 8 == 2, "two lanes per env, each with whole charger pairs and record quads");
    static constexpr int WENVS = Lay::WENVS, H = (NC - 2) / 2, CPL = H + 1;
    static constexpr int KT = (Lay::A * WENVS + 4 * kWave - 1) / (4 * kWave);
    // the fast loop's charger step without the discharge branch (charger_step NONNEG) for the headline's
    // station (step 6.60-6.66 -> 6.53-6.56 us, profiles/r04_ab_nonneg.txt).  At N = 50 the compiler merges
    // several chargers' select masks ahead of the per-charger scheduling barriers and spills them (332
    // v_readlane); with each charger's inputs pinned to its block it compiles to 5.5 % fewer VALU, and
    // config 5 ran 22.62-22.69 against 22.47-22.54 us (profiles/r04_ab_config5_nonneg.txt): its step is
    // bound by its bytes, so config 5 keeps the general form
    static constexpr bool kNonneg = NC <= 16;
    static __device__ __forceinline__ int charger(int part, int j) { return j < H ? part * H + j : NC - 2 + part; }
    int64_t e0;
    int nw;
    bool live;
    uint32_t el1, el4, el8, row4, row4_last, soc_a, soc_b, rec_a, rec_b;
    TileStage<KT, kWave> act_tile;
    double ratio, bess_l, pen0_l, ret_l;
    double fpv[4], fpr[4];
    uint32_t w[CPL];
    double aux[PK ? 1 : CPL], run_[CPL], req[REQ ? CPL : 1];
    SNG_WSTAMP_DECL;   // diagnostic builds: 0 issue, 1 actions tile staged, 2 chargers, 3 env tail, 4 obs stores issued
    // the day kernels' stamp 0: the top of a step of their loop (each step overwrites the stamps: the last one's stay)
    __device__ __forceinline__ void stamp_step_top() { SNG_WSTAMP(0); }

    // the (per-lane, uniform) byte offsets of charger j of the lane in a [N][E] u32 plane: the lane's first row
    // (or its last-pair charger's) in the per-lane part, j * E (or (N - 2) * E) in the uniform part
    static __device__ __forceinline__ uint32_t r4_of(int j, int64_t E) {
        return (uint32_t)(j < H ? j : NC - 2) * (uint32_t)E * 4u;
    }
    __device__ __forceinline__ uint32_t row_of(int j) const { return j < H ? row4 : row4_last; }
    // the lane's env and its byte offsets: the same for every step of a day
    __device__ __forceinline__ void place(int64_t e0_, int64_t E, int lane) {
        const int le = lane / L, part = lane % L;
        e0 = e0_;
        nw = (E - e0) < WENVS ? (int)(E - e0) : WENVS;
        live = le < nw;
        const int64_t el = live ? e0 + le : E - 1;   // idle lanes load a valid env and discard it
        el1 = (uint32_t)el;
        el4 = el1 * 4u;
        el8 = el1 * 8u;
        row4 = el4 + (uint32_t)(part * H) * (uint32_t)E * 4u;     // charger part H + j, j < H: + j E (uniform)
        row4_last = el4 + (uint32_t)part * (uint32_t)E * 4u;      // charger N - 2 + part: + (N - 2) E (uniform)
        soc_a = 2u * el8 + (uint32_t)(part * H) * (uint32_t)E * 8u;   // pair row part H + j: + j E 8 (uniform)
        soc_b = 2u * el8 + (uint32_t)part * 8u;                      // the last pair's row: + (N - 2) E 8
        rec_a = el1 * 8u + (uint32_t)(part * H) * (uint32_t)E * 2u;   // quad row part H + j: + j E 2 (uniform)
        rec_b = el1 * 4u + (uint32_t)part * 2u;                      // the partial quad (N - 2, N - 1): + (N - 2) E 2
    }
    // charger j of the lane: its SoC load -- a pair's 16 B with the pair's second charger, the last pair's 8 B
    __device__ __forceinline__ void issue_soc(int j, int64_t E, const DeviceState &s) {
        if (j < H && (j & 1)) bld2(s.soc, soc_a, (uint32_t)(j - 1) * (uint32_t)E * 8u, run_[j - 1], run_[j]);
        if (j == H) run_[j] = bld(s.soc, soc_b, (uint32_t)(NC - 2) * (uint32_t)E * 8u);
    }
    // ... and its SoC store, with the same pairing (v: the lane's chargers' values): a pair's 16 B once both its
    // chargers are stepped, the last pair's 8 B
    __device__ __forceinline__ void store_soc(int j, int64_t E, const DeviceState &s, const double *v) {
        if (j < H && (j & 1)) bst2<kNT>(s.soc, soc_a, v[j - 1], v[j], (uint32_t)(j - 1) * (uint32_t)E * 8u);
        if (j == H) bst<kNT>(s.soc, soc_b, v[j], (uint32_t)(NC - 2) * (uint32_t)E * 8u);
    }
    // the day kernel's state back to memory: every charger's SoC (a live lane's own chargers), and after the
    // day's last step the BESS SoC and the day return too
    __device__ __forceinline__ void store_state_soc(int64_t E, const DeviceState &s) {
        if (live) {
#pragma unroll
            for (int j = 0; j < CPL; ++j) store_soc(j, E, s, run_);
        }
    }
    __device__ __forceinline__ void store_state(int64_t E, const Params &p, const DeviceState &s, const InfoPtrs &info,
                                                int lane) {
        store_state_soc(E, s);
        if (live && lane % L == 0) {
            if (p.bess) bst<kNT>(s.bess, el8, bess_l);
            if (info.episode_return) bst<kNT>(info.episode_return, el8, ret_l);
        }
    }
    // loads oldest-needed-first: the actions tile and the per-env values, then every charger's state.
    // STEP: what one step reads (its actions tile, records, requested SoC and profile factors); STATE: what
    // passes from step to step (PV ratio, BESS SoC, the t = 0 penalty, the day return and every charger's
    // SoC).  step_wide_kernel issues both, interleaved as below; the day kernel (sng_step_day.h) issues the
    // state once a day and each step's inputs with issue_step_inputs.
    template <bool STATE = true, bool STEP = true>
    __device__ __forceinline__ void issue(int64_t e0_, const float *act, int64_t E, int t, int vec_io, const Params &p,
                                          const DeviceState &s, const InfoPtrs &info, int lane) {
        SNG_WSTAMP(0);
        place(e0_, E, lane);
        [[maybe_unused]] const size_t plane = (size_t)t * NC * (size_t)E;   // this step's timeline planes
        [[maybe_unused]] const uint16_t *rec_t = packed_records(s) + plane + (size_t)NC * (size_t)E;   // t + 1
        [[maybe_unused]] const int Ad = p.act_dim;
        if constexpr (STEP) act_tile.issue(act + e0 * Ad, nw * Ad, vec_io != 0, lane);
        if constexpr (STATE) {
            ratio = bld(s.ratio, el8);
            bess_l = bld(p.bess ? s.bess : s.ratio, el8);
        }
        if constexpr (STEP) {
#pragma unroll
            for (int j = 0; j < 4; ++j) fpv[j] = fpr[j] = 1.0;
            if constexpr (NOISE) profile_factors(p, s, el8, t, fpv, fpr);   // the day's profile factors of t..t+3
        }
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            // charger `charger(part, j)`
            const uint32_t v4 = row_of(j), r4 = r4_of(j, E), v8 = 2u * v4, r8 = 2u * r4;
            if constexpr (STEP) {
                if (PK) {   // 2 B records in charger quads: the lane's whole quads as 8 B, its last-pair charger as 2 B
                    if (j < H && (j & 3) == 0)
                        unpack_quad(bld(reinterpret_cast<const uint64_t *>(rec_t), rec_a, (uint32_t)j * (uint32_t)E * 2u),
                                    w + j);
                    if (j == H) w[j] = bld16(rec_t, rec_b, (uint32_t)(NC - 2) * (uint32_t)E * 2u);
                } else {
                    w[j] = bld(s.word + plane, v4, r4);
                    aux[PK ? 0 : j] = bld(s.aux + plane, v8, r8);
                }
            }
            // a pair's 16 B once both its records are issued; the last pair's 8 B
            if constexpr (STATE) issue_soc(j, E, s);
            if constexpr (STEP)
                if (REQ) req[REQ ? j : 0] = bld(s.req + plane, v8, r8);
        }
        // the t = 0 penalty and the day return are read only by the env tail: issued behind every charger's
        // loads, so the waits before the chargers (the header's PV ratio, the BESS step's SoC) do not count them
        // (round 6, A/B in the day graph: 6.36 -> 6.25-6.29 us per step, profiles/r06_ab_step_tail_order.txt).
        // Stores issued earlier or in bursts measured slower there: the observation tile stored before the env
        // tail +0.33 us, its copy-out unrolled (every LDS read, then every 16 B store) +0.6 us, the SoC pairs
        // stored after the charger loop +0.3 us -- paced stores leave the other wavefronts' loads alone.
        if constexpr (STATE) {
            pen0_l = bld(t == 0 ? s.pen0 : s.ratio, el8);
            ret_l = bld(info.episode_return ? info.episode_return : s.ratio, el8);
        }
    }
    // One step's inputs of a packed day, for the day kernel: the actions tile into day_tile, the step's records
    // as they lie in memory (the lane's quads and its last-pair record: rq, rl; take_step_inputs unpacks them
    // into w[] once the step before has read its own) and the requested SoC.  The step's table constants are
    // not among them: the day kernel reads them by scalar loads at the top of their own step
    // (step_constant_scalar; a per-launch StepConst cannot carry T steps).
    static constexpr int NQ = H / 4;
    TileStage<KT, kWave, true> day_tile;   // issued a step ahead of its commit: TileStage, VEC_ONLY
    uint64_t rq[NQ];
    uint32_t rl;
    double reqn[REQ ? CPL : 1];
    __device__ __forceinline__ void issue_step_inputs(const float *act, int64_t E, int t, int vec_io, const Params &p,
                                                      const DeviceState &s, int lane) {
        static_assert(PK, "the day kernel steps packed days");
        const size_t plane = (size_t)t * NC * (size_t)E;
        const uint16_t *rec_t = packed_records(s) + plane + (size_t)NC * (size_t)E;   // t + 1, as issue()
        day_tile.issue(act + e0 * p.act_dim, nw * p.act_dim, vec_io != 0, lane);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            rq[q] = bld(reinterpret_cast<const uint64_t *>(rec_t), rec_a, (uint32_t)(4 * q) * (uint32_t)E * 2u);
        rl = bld16(rec_t, rec_b, (uint32_t)(NC - 2) * (uint32_t)E * 2u);
        if constexpr (REQ) {
#pragma unroll
            for (int j = 0; j < CPL; ++j) reqn[j] = bld(s.req + plane, 2u * row_of(j), 2u * r4_of(j, E));
        }
    }
    // The same for day_station_kernel, whose loop carries the step's actions block and record plane (t + 1) as
    // pointers it advances, instead of rebuilding both from E, t and t0 by 64-bit scalar multiplies on every step.
    __device__ __forceinline__ void issue_step_inputs_at(const float *act_t, const uint16_t *rec_t, int64_t E, int vec_io,
                                                         int lane) {
        static_assert(PK && !REQ, "the default station's packed days");
        day_tile.issue(act_t + e0 * Lay::A, nw * Lay::A, vec_io != 0, lane);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            rq[q] = bld(reinterpret_cast<const uint64_t *>(rec_t), rec_a, (uint32_t)(4 * q) * (uint32_t)E * 2u);
        rl = bld16(rec_t, rec_b, (uint32_t)(NC - 2) * (uint32_t)E * 2u);
    }
    __device__ __forceinline__ void take_step_inputs() {
#pragma unroll
        for (int q = 0; q < NQ; ++q) unpack_quad(rq[q], w + 4 * q);
        w[H] = rl;
        if constexpr (REQ) {
#pragma unroll
            for (int j = 0; j < CPL; ++j) req[j] = reqn[j];
        }
    }
    // the requested SoC at python index t-1 of charger j of the lane, or its default without the stream
    __device__ __forceinline__ double req_of(int j, const Params &p) const {
        return REQ ? req[REQ ? j : 0] : req_default(p);
    }

    // the group's step; s_act holds its actions tile (committed), s_obs is the wavefront's observation tile.
    // KEEP (the day kernel): what the next step of the same env would load straight back stays in registers --
    // every charger's new SoC in run_[], the BESS SoC in bess_l, the day return in ret_l -- and the caller
    // stores it after the day's last step (store_state); every other output is stored as always.
    // STATION (day_station_kernel, with KEEP): the leaner forms of that kernel's step, each behind this switch so
    // that every other kernel's step is the code it was.  `st` carries what its caller has per step; k holds the
    // irradiance entries and the env tail's two constants (its price_norm entries are not read).
    template <bool KEEP = false, bool STATION = false>
    __device__ __forceinline__ void run(const float *s_act, float *s_obs, float *obs, double *reward, uint8_t *done,
                                        int64_t E, int t, int vec_io, const StepConst &k, const Params &p,
                                        const DeviceState &s, const InfoPtrs &info, int lane,
                                        const StationStep *st = nullptr) {
        static_assert(!STATION || (KEEP && PK && !REQ && !NOISE && kNonneg), "the default station's day kernel");
        SNG_WSTAMP(1);
        const int Ad = p.act_dim, O = p.obs_dim;
        const int le = lane / L, part = lane % L;
        const bool leader = part == 0;
        const size_t plane = (size_t)t * NC * (size_t)E;
        const uint16_t *rec_t = packed_records(s) + plane + (size_t)NC * (size_t)E;
        if constexpr (STATION) rec_t = st->rec_t;   // carried by the day's loop, not rebuilt from E and t
        const float *a_row = s_act + le * Ad;
        float *o_row = s_obs + le * O;
        float av[CPL];
        // the largest action bit pattern: above +inf's (0x7f800000) when some action is negative (-0.0 too) or
        // NaN, and such a wavefront takes the general order below (an integer max keeps no per-charger lane
        // masks alive into the charger loop)
        uint32_t amax_bits = 0u;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            av[j] = a_row[charger(part, j)];
            amax_bits = __builtin_elementwise_max(amax_bits, __builtin_bit_cast(uint32_t, av[j]));
        }
        const bool not_nonneg = amax_bits > 0x7f800000u;
        const float bess_action = p.bess ? a_row[NC] : 0.0f;
        const int k_soc = p.pv ? 8 : 4;
        // the observation header and the BESS step need only per-env values: both run here, while the
        // chargers' loads are still in flight (the BESS's division no longer trails the charger sums)
        BessStep bs{};
        if (live && leader) {
            if constexpr (STATION) write_obs_header_station(o_row, k.v + CST_IRR, st->pnf, ratio);
            else write_obs_header(o_row, p, k.v + CST_IRR, k.v + CST_PN, ratio, fpv, fpr);
            bs = bess_step<!KEEP>(p, s, el8, t, p.bess ? bess_l : 0.0, bess_action);
            if (p.bess) o_row[O - 1] = (float)bs.bess;
        }

        double pen_v = 0.0, p_ch = 0.0, p_dis = 0.0;
        uint32_t n_nonexist = 0, fl = 0;
        if (__builtin_amdgcn_ballot_w64(live && not_nonneg) == 0) {
            // the fast loop: every action of the wave is >= 0, so no negative power (p_dis stays 0.0) and no
            // charger discharges (charger_step<..., NONNEG>)
            double seq_pos = 0.0, pmin = __builtin_inf();
            int n_pos = 0;
            // STATION: the exact-sum test on the terms' high words instead of the count, the minimum and the
            // comparison in f64 (sng_exact_sum.h)
            uint32_t bmax = kExactSumBmax0, bmin = kExactSumBmin0;
            double qv[CPL], sv[CPL];
            if (live) {
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
                    const int c = charger(part, j);
                    // visit_charger's conventions by hand: with the helper here the day kernel spills more SGPRs
                    // than tests/test_day_kernel_resources.py allows (profiles/charger_visit_ab.txt)
                    const uint32_t capi = cap_field<PK>(w[j]);
                    const bool occ = (w[j] & W_OCC) != 0;
                    const ChargerResult r = charger_step<true, kNonneg, PK>(p, PK ? (w[j] & ~W_STATIC) : w[j],
                                                                           PK ? 0.0 : aux[PK ? 0 : j], run_[j], req_of(j, p),
                                                                           av[j], t, recip_cap((double)capi));
                    sv[j] = (PK && !occ) ? (double)rec_soc(w[j]) : r.soc;
                    if constexpr (KEEP) run_[j] = sv[j];
                    else store_soc(j, E, s, sv);
                    o_row[k_soc + c] = (float)r.soc;
                    o_row[k_soc + NC + c] = departure_obs<PK>((PK && !occ) ? 0u : w[j]);
                    n_nonexist += r.nx;
                    fl |= r.fl;
                    qv[j] = r.q;
                    // the lane's own penalties in charger order; the last pair's come after the other lane's
                    // whole pairs (below)
                    if (j < H) pen_v += r.q;
                    if constexpr (STATION) {
                        seq_pos += r.pw;
                        exact_sum_track(exact_sum_hi(r.pw), bmax, bmin);
                    } else {
                        const bool ip = r.pw > 0.0;
                        seq_pos += r.pw;   // >= 0 here (the float32 product of a >= 0, or 0.0): adding it is exact
                        n_pos += ip ? 1 : 0;
                        pmin = __builtin_fmin(pmin, ip ? r.pw : __builtin_inf());
                    }
                    // chargers in order: charger j waits only for its own loads.  A/B of scheduling groups
                    // (profiles/r03_ab_wide_sched_groups.txt): config 5 22.6-22.7 us with one or two chargers
                    // per group, 22.8 with five, 27.1 with no barrier in a lane's 25 chargers; the headline
                    // within noise.  The barrier and the in-order walk answer the step kernel's load arrival; the
                    // day kernel (KEEP) has every charger's inputs in registers before the loop and could overlap
                    // the five chains.  Measured there, with the header and the BESS step in the same block and
                    // every choice a select: 114.9-115.2 us per day against 114.5-114.6 (240 VGPRs), so it keeps
                    // this form: its step was not waiting on these chains (profiles/day_kernel_chain_ab.txt)
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // numpy sums fewer than 8 positive powers in order: one lane's running sum is that sum; two lanes'
            // partial sums combined are that sum only when one of them is empty or the sum is exact
            // the other lane's totals (exact combinations), and its penalties after the first lane's own, in
            // charger order (adding a +0.0 term is exact)
            const double seq_own = seq_pos, pmin_own = pmin;
            const int n_own = n_pos;
            const uint32_t nx_own = n_nonexist, fl_own = fl;
            int with_pos = n_own > 0 ? 1 : 0;
            const uint32_t bmax_own = bmax, bmin_own = bmin;
            auto gather = [&] {
                if constexpr (STATION) {
                    bmax = __builtin_elementwise_max(bmax, from_part<1>(bmax_own));
                    bmin = __builtin_elementwise_min(bmin, from_part<1>(bmin_own));
                    seq_pos += from_part<1>(seq_own);
                } else {
                    const int nk = (int)from_part<1>((uint32_t)n_own);
                    with_pos += nk > 0 ? 1 : 0;
                    n_pos += nk;
                    seq_pos += from_part<1>(seq_own);
                    pmin = __builtin_fmin(pmin, from_part<1>(pmin_own));
                }
                n_nonexist += from_part<1>(nx_own);
                fl |= from_part<1>(fl_own);
#pragma unroll
                for (int j = 0; j < H; ++j) {
                    const double qk = from_part<1>(qv[j]);
                    // only the leader's pen_v is read (the env tail): STATION adds on both lanes, no select
                    pen_v = (STATION || leader) ? pen_v + qk : pen_v;
                }
            };
            gather();
            {   // the last pair: charger N - 2 (this lane), then N - 1 (the other)
                const double qk = from_part<1>(qv[H]);
                pen_v = (STATION || leader) ? (pen_v + qv[H]) + qk : pen_v;
            }
            const bool split = with_pos > 1;
            p_ch = seq_pos;
            bool pos_slow;
            if constexpr (STATION) pos_slow = live && leader && exact_sum_rebuild(bmax, bmin);
            else pos_slow = live && leader && (n_pos >= 8 || split) && !(seq_pos <= pmin * 0x1.0p28);
            if (__builtin_amdgcn_ballot_w64(pos_slow)) {   // wave-uniform: rare
                if (pos_slow) {
                    // the compacted positive powers again, in charger order: an occupied charger charging with
                    // a > 0 under bounded charging bills pc (charger.py:58-94); nothing else is positive here
                    PairwiseSum pos;
                    pos.init();
#pragma unroll 1
                    for (int c = 0; c < NC; ++c) {
                        const RecOff ro = rec_off(c, NC, E, el1);
                        const uint32_t wc = PK ? bld16(rec_t, ro.v, ro.s)
                                               : bld(s.word + plane, el4, (uint32_t)c * (uint32_t)E * 4u);
                        const float a = a_row[c];
                        const double pc = charging_power(p, a);
                        if ((wc & W_OCC) && p.bounded && a > 0.0f && pc > 0.0) pos.push(pc);
                    }
                    p_ch = pos.result();
                }
            }
        } else {
            // a wave with a discharging action: numpy's pairwise order for both signs (PairwiseSum), one
            // charger at a time on the env's first lane, its inputs re-read from memory and the actions tile
            PairwiseSum pos, neg;
            pos.init();
            neg.init();
            // KEEP: this path keeps memory as its SoC state (the first lane steps the other lanes' chargers
            // too), so the wavefront's SoC registers go to memory before it and come back after it; the
            // wavefront's own stores and loads of an address stay in order (one L1 for the whole wavefront)
            if constexpr (KEEP) {
                store_state_soc(E, s);
                wave_mem_fence();
            }
            if (live && leader) {
#pragma unroll 1
                for (int c = 0; c < NC; ++c) {
                    const uint32_t r4 = (uint32_t)c * (uint32_t)E * 4u, r8 = 2u * r4;
                    const SocOff so = soc_off(c, NC, E, el8);
                    const RecOff ro = rec_off(c, NC, E, el1);
                    const uint32_t wc = PK ? bld16(rec_t, ro.v, ro.s) : bld(s.word + plane, el4, r4);
                    const double auxc = PK ? 0.0 : bld(s.aux + plane, el8, r8);
                    const double runc = bld(s.soc, so.v, so.s);
                    const double reqc = REQ ? bld(s.req + plane, el8, r8) : req_default(p);
                    const ChargerVisit<PK> v = visit_charger<true, false, PK>(p, wc, auxc, runc, reqc, a_row[c], t);
                    const ChargerResult &r = v.r;
                    bst<kNT>(s.soc, so.v, v.soc, so.s);
                    o_row[k_soc + c] = v.obs_soc();
                    o_row[k_soc + NC + c] = v.obs_dep();
                    n_nonexist += r.nx;
                    fl |= r.fl;
                    pen_v += r.q;
                    if (r.pw > 0.0) pos.push(r.pw);
                    if (r.pw < 0.0) neg.push(r.pw);
                }
            }
            p_ch = pos.result();
            p_dis = neg.result();
            if constexpr (KEEP) {
                wave_mem_fence();
#pragma unroll
                for (int j = 0; j < CPL; ++j) issue_soc(j, E, s);
                // landed here, on the rare path: the fast path writes the same registers, and a load the compiler
                // sees pending on any way to there makes its wavefronts wait for all they have in flight
                wave_vmem_drain();
            }
        }
        SNG_WSTAMP(2);
        // The day kernel (KEEP) issued the next step's loads before this step, and the step's stores start here.
        // Those loads are drained now, ahead of the stores and outside every branch: they have had the header,
        // the BESS step and the chargers to land.  Left to their first use at the top of the next step they
        // wait there for this step's stores too (wave_vmem_drain, sng_dev_util.h; day_wide_kernel drains the
        // first step's before its loop), which was 1.8 of the step's 4.1 us (profiles/day_kernel_chain_ab.txt)
        if constexpr (KEEP) wave_vmem_drain();
        if (live && leader) {
            pen_v += (t == 0) ? pen0_l : 0.0;   // python index -1 slot; every per-charger term is 0 at t = 0
            env_tail<false, true, KEEP>(p, s, info, e0, (uint32_t)le, el1, el8, t, ratio, p.bess ? bess_l : 0.0,
                                        bess_action, p_ch, p_dis, pen_v, 100.0 * (double)n_nonexist, fl, o_row, k.v, fpv,
                                        fpr, info.episode_return ? ret_l : 0.0, 0.0, reward, done, &bs, &ret_l);
            if constexpr (KEEP) bess_l = bs.bess;
        }
        SNG_WSTAMP(3);
        wave_lds_fence();
        copy_out<kWave>(obs + e0 * O, s_obs, nw * O, vec_io != 0, lane);
        SNG_WSTAMP(4);
    }
};

// Two lanes per env (L = 2, the only layout compiled; the template parameter names the kernels): lane `part` of
// an env steps chargers [part * H, (part + 1) * H), H = (NC - 2) / 2, and charger NC - 2 + part of the last pair
// (WideGroup, above).  The env's lanes are adjacent (half a DPP quad); the partial charging sums, counts and
// minima combine exactly on the first lane (a sum the exactness test accepts is exact in any order, and
// fewer than 8 powers are numpy's in-order sum when one lane holds them all), the first lane adds the
// other lane's vehicle penalties after its own in charger order (Python's sum, penaliser.py:55), and the
// rare exact-order paths run on the first lane over all chargers.  One group of 32 envs per wavefront;
// the register budget is sized for two waves per SIMD (every wave of the E = 65,536 grid resident at once).
// Measured and reverted (A/B on one box):
//   - two groups of 32 envs per wavefront at N = 10 (1,024 wavefronts, each group's loads issued before the
//     first group is stepped): 8.62-8.64 us per step in the graph against 6.68-6.71 us
//     (profiles/r04_ab_groups.txt);
//   - config 5 with four lanes per env and a 3-wave budget (166 VGPRs, no spills, 3 of the 4,096 waves per
//     SIMD resident): 29.6-29.8 us against 23.4 us with two lanes (profiles/r03_ab_config5_four_lanes.txt);
//   - round 5: two or four such wavefronts per workgroup (each with its own envs and LDS tiles, no barrier;
//     512 / 1,024 workgroups instead of 2,048): 6.79-6.80 / 6.99-7.03 us per step in the graph against
//     6.31-6.34 us with one (profiles/r05_ab_waves_per_workgroup.txt).
template <int NC, int L, bool PK, bool REQ, bool NOISE>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(L, L))) void
step_wide_kernel(const float *__restrict__ act, float *__restrict__ obs, double *__restrict__ reward,
                 uint8_t *__restrict__ done, int64_t E, int t, int vec_io, StepConst k, Params p, DeviceState s,
                 InfoPtrs info) {
    using Grp = WideGroup<NC, L, PK, REQ, NOISE>;
    using Lay = WideLds<NC, L>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    float *s_obs = lds + Lay::ACT;   // the actions tile, then the observation tile
    Grp g;
    const int64_t e0 = (int64_t)blockIdx.x * Grp::WENVS;   // the grid covers E: the wavefront has an env
    g.issue(e0, act, E, t, vec_io, p, s, info, lane);
    g.act_tile.commit(lds, lane);
    wave_lds_fence();
    g.run(lds, s_obs, obs, reward, done, E, t, vec_io, k, p, s, info, lane);
    SNG_WSTAMP_FLUSH(g.stamp_, 5);
    bump_day_counter<PK>(p, s, t);
}

}  // namespace sng
