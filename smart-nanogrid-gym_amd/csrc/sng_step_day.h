// sng_step_day.h -- the day kernels: the steps t0 .. t0 + nt - 1 of a loaded day in one launch.  sng_graph_create
// captures one in place of the day's T dependent step nodes: it is given every step's actions at capture, and envs
// never interact, so a wavefront can step its envs through the whole day on its own -- no grid-wide synchronisation,
// no node boundary (1.6-1.9 us each, the end-of-kernel write-back the next node waits for included) and no state
// round trip.
//   day_wide_kernel  packed (device-RNG) days of the wide family's 10-charger station, 64 / L envs per wavefront;
//   day_station_kernel  the same for the default station, its switches fixed at compile time and its arguments
//                    one small struct (sng_step_plan.h day_station_fixed);
//   day_lean_kernel  the lean family's stations, packed and unpacked days, 64 envs per wavefront; it can keep every
//                    step's outputs (per-step strides).
// Which plan has which is decided in sng_step_plan.h (day_kernel_of).
// Needs sng_step_wide.h and sng_step_lean.h (WideGroup, LeanGroup: a step's arithmetic is their run<KEEP = true>(),
// nothing is restated here).  Included by sng_kernels.hip only.
#pragma once

namespace sng {

// Step t + 1's loads (its actions tile, records and requested SoC) are issued before step t's first store.  A
// store counts in vmcnt ahead of every later load, so a load issued behind step t's stores waits for them; issued
// ahead of them it costs registers for the whole step (the raw records, the tile's registers and, with the
// stream, the requested SoC).  Issuing them early is half of it: the wait for them has to come before step t's
// stores too.  The compiler puts a loaded register's wait at its first use -- the top of step t + 1 -- with the
// count that is safe on the loop's entry, where no store lies between the load and the use; on the back edge that
// count drains step t's stores as well (1.8 us of a 4.1 us step, profiles/day_kernel_chain_ab.txt).  So the
// loads are drained explicitly where nothing younger is in flight (wave_vmem_drain: before the loop, and in
// WideGroup::run<KEEP> between the chargers and the env tail's first store), the actions tile has only its
// aligned form in registers (TileStage, VEC_ONLY) and the rare general path drains its SoC reloads: no path into
// the loop's top, real or only in the control-flow graph, leaves a load pending there.
// Geometry as step_wide_kernel's: one wavefront per workgroup, WideLds<NC, L>::WENVS envs per wavefront, the
// same LDS tiles.  `act` is step t0's [E][act_dim] block, the later steps' blocks follow it.
//   once a day:  the PV ratio, BESS SoC, t = 0 penalty, day return, profile keys and every charger's SoC are
//                loaded before the first step and live in registers; SoC, BESS SoC and the day return are
//                stored after the last step, as the same f64 values memory would have carried from step to
//                step.  bess0 is written at t = 0 and the day counter advanced once, as by the step kernel.
//   every step:  the actions tile, record plane t + 1 (and the requested-SoC plane) are read, the table
//                constants come from s.tables by scalar loads at the step's own top, and the observation rows,
//                reward, done, flags and the flag summary are stored exactly as step_wide_kernel stores them.
// Per env-step it reads 4 (N + 1) + 2 N bytes and writes 4 (2 N + 9) + 9; per env-day the state moves
// 8 N + 32 bytes each way, plus bess0.
template <int NC, int L, bool REQ, bool NOISE>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(L, L))) void
day_wide_kernel(const float *__restrict__ act, float *__restrict__ obs, double *__restrict__ reward,
                uint8_t *__restrict__ done, int64_t E, int t0, int nt, int vec_io, Params p, DeviceState s,
                InfoPtrs info) {
    using Grp = WideGroup<NC, L, true, REQ, NOISE>;
    using Lay = WideLds<NC, L>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    float *s_obs = lds + Lay::ACT;   // the actions tile, then the observation tile
    Grp g;
    const int64_t e0 = (int64_t)blockIdx.x * Grp::WENVS;   // the grid covers E: the wavefront has an env
    const size_t block = (size_t)E * (size_t)p.act_dim;    // one step's actions
    g.template issue<true, false>(e0, act, E, t0, vec_io, p, s, info, lane);   // the day's state
    v2u keys = {0u, 0u};
    if constexpr (NOISE) keys = profile_keys(s, g.el8);
#pragma unroll
    for (int j = 0; j < 4; ++j) g.fpv[j] = g.fpr[j] = 1.0;
    g.issue_step_inputs(act, E, t0, vec_io, p, s, lane);
    // the day's state and the first step's inputs landed before the loop, as every later step's are before the
    // stores of the step ahead of it (WideGroup::run): nothing the loop's top uses is still in flight on either
    // way into it, so no wait there stands behind a store
    wave_vmem_drain();
    // Which of a step's ten table constants go to vector registers (bit i: constant i, CST_*): all of them in the
    // headline's instantiation; with the requested-SoC stream or the profile factors the first two and the env
    // tail's two.  Chosen by what the register allocator makes of each instantiation, against the SGPR-spill
    // ceilings of tests/test_day_kernel_resources.py (all ten there: 157 spills with the factors, and a stack
    // slot with the stream)
    constexpr unsigned kPinned = (REQ || NOISE) ? 0x303u : 0x3ffu;
    const int t1 = t0 + nt;
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        g.stamp_step_top();
        g.take_step_inputs();
        g.day_tile.commit(lds, lane);
        wave_lds_fence();
        if constexpr (NOISE) expand_profile_factors(p, keys, t, g.fpv, g.fpr);
        if (t + 1 < t1)   // ahead of this step's stores
            g.issue_step_inputs(act + (size_t)(t + 1 - t0) * block, E, t + 1, vec_io, p, s, lane);
        // this step's table constants: scalar loads, which wait on lgkmcnt and never behind a store, so they need
        // no step of prefetch.  The pinned ones are copied to vector registers once loaded (an empty asm with a
        // "v" operand): the kernel has vector registers to spare and none of the scalar ones
        StepConst k;
#pragma unroll
        for (int i = 0; i < CST_COUNT; ++i) {
            k.v[i] = step_constant_scalar(s.tables, t, i);
            if (kPinned & (1u << i)) asm("" : "+v"(k.v[i]));
        }
        g.template run<true>(lds, s_obs, obs, reward, done, E, t, vec_io, k, p, s, info, lane);
        wave_lds_fence();   // the next step's tile writes stay behind this step's reads of both tiles
    }
    SNG_WSTAMP_FLUSH(g.stamp_, 5);   // diagnostic builds: the last step's phases (tools/stamps.py --day)
    g.store_state(E, p, s, info, lane);
    bump_day_counter<true>(p, s, t0);
}

// day_station_kernel: day_wide_kernel<NC, L, false, false> for the one station whose switches are all known when the
// day is captured (sng_step_plan.h day_station_fixed: the default station of SmartNanogridVecEnv -- PV, BESS, bounded
// charging, no V2X, NumPy-2 promotion, a power-of-two dt, T = kDayStationT steps, no requested-SoC stream, not a
// replayed day).  A station's switches never change over the life of a handle, yet the generic kernel holds each in a
// scalar register through the day (spilled to a VGPR lane and read back: its by-value Params, DeviceState and
// InfoPtrs are 500-odd bytes) and decides the same select or branch with it on every step.  Here the body's Params
// is built in the kernel with those switches as constants, which fold through the force-inlined step, and the
// arguments are one struct of what this path reads: the physical constants of the charger, BESS and cost formulas
// and the state, record, table and output pointers.  The loop and the geometry are day_wide_kernel's.
// The per-env flag store, the flag summary and the day return stay run-time pointers (null: not written), as in the
// generic kernel: every handle of the station takes this kernel, whatever SngInfo it passes.
// t0 and nt are arguments because they are launch_day's and day_wide_kernel's; launch_day's one caller (a capture,
// sng_graph.cpp) passes 0 and T, so no part of a day has been run or tested through this kernel.  They were not
// made constants: that form was not measured.
struct DayStationArgs {
    const float *act;
    float *obs;
    double *reward;
    uint8_t *done;
    int64_t E;
    int32_t t0, nt, vec_io, bump_day;
    float dt_f, ev_power_f, ev_eff_f;
    double dt, rdt;
    double bess_cap, bess_pmax_ch, bess_pmax_dis, bess_eff_ch, bess_eff_dis, bess_dod;
    double grid_w, bat_pen_w, sell_coef;
    double *soc, *bess, *bess0, *ratio, *pen0, *rec;   // rec: the packed records (DeviceState::aux)
    uint32_t *flags;
    uint64_t *episode;
    const Tables *tables;
    uint32_t *info_flags, *flag_any;   // InfoPtrs::flags, flag_any
    double *episode_return;
};
// The day's table rows in the wavefront's LDS, behind its two tiles (launch_day asks for the room): entries
// t = 0 .. T + 2, what the steps of any part of the day read (step t: irr_norm and price_norm t .. t + 3, pv_power
// and price t).  Staged once, ahead of the loop; a step reads its ten values by LDS reads at a uniform address
// (the irradiance as two pairs, the env tail's pv_power and price as one pair, the four price entries as float32).
// The generic kernel reads them by ten scalar loads in three dependent round trips at the top of every step and
// copies each to a vector register (profiles/day_station_step_ab.txt).
struct StationRows {
    static constexpr int N = kDayStationT + 3;
    double irr[N];
    double env[N][2];   // pv_power[t], price[t]
    float pnf[N + 1];   // (float)price_norm[t]
};
template <int NC, int L>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(L, L))) void day_station_kernel(DayStationArgs a) {
    Params p{};
    p.n = NC;
    p.T = kDayStationT;
    p.act_dim = NC + 1;
    p.obs_dim = 2 * NC + 9;
    p.pv = p.bess = p.bounded = p.dt_pow2 = p.packed = 1;   // v2x, legacy, req_stream, req_zero, noise: 0
    p.lanes = 1;
    p.bump_day = a.bump_day;
    p.dt = a.dt;
    p.rdt = a.rdt;
    p.dt_f = a.dt_f;
    p.ev_power_f = a.ev_power_f;
    p.ev_eff_f = a.ev_eff_f;
    p.bess_cap = a.bess_cap;
    p.bess_pmax_ch = a.bess_pmax_ch;
    p.bess_pmax_dis = a.bess_pmax_dis;
    p.bess_eff_ch = a.bess_eff_ch;
    p.bess_eff_dis = a.bess_eff_dis;
    p.bess_dod = a.bess_dod;
    p.grid_w = a.grid_w;
    p.bat_pen_w = a.bat_pen_w;
    p.sell_coef = a.sell_coef;
    DeviceState s{};
    s.soc = a.soc;
    s.bess = a.bess;
    s.bess0 = a.bess0;
    s.ratio = a.ratio;
    s.pen0 = a.pen0;
    s.aux = a.rec;
    s.flags = a.flags;
    s.episode = a.episode;
    s.tables = a.tables;
    InfoPtrs info{};
    info.flags = a.info_flags;
    info.flag_any = a.flag_any;
    info.episode_return = a.episode_return;
    // day_wide_kernel's loop without the stream and the profile factors, in the station's leaner form: the table
    // rows staged in LDS, the two input pointers carried from step to step, and run<KEEP, STATION>.  (As one inlined
    // function shared with that kernel, its four instantiations allocate differently -- 138 SGPR spills for 121 in the
    // headline's -- and tests/test_day_kernel_resources.py pins them: profiles/day_station_kernel_ab.txt.)
    using Grp = WideGroup<NC, L, true, false, false>;
    using Lay = WideLds<NC, L>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    float *s_obs = lds + Lay::ACT;
    Grp g;
    const int64_t E = a.E;
    const int t0 = a.t0, vec_io = a.vec_io;
    const float *__restrict__ act = a.act;
    float *__restrict__ obs = a.obs;
    double *__restrict__ reward = a.reward;
    uint8_t *__restrict__ done = a.done;
    const int64_t e0 = (int64_t)blockIdx.x * Grp::WENVS;
    // one step's actions and one record plane: what the loop's two input pointers advance by
    const size_t block = (size_t)E * (size_t)p.act_dim, plane = (size_t)NC * (size_t)E;
    const float *act_t = act;
    const uint16_t *rec_t = packed_records(s) + (size_t)(t0 + 1) * plane;   // step t reads record plane t + 1
    // the day's table rows, one entry a lane (the lanes past the last entry load and write it again)
    StationRows *rows = reinterpret_cast<StationRows *>(lds + Lay::ACT + Lay::OBS);
    const int row_i = lane < StationRows::N ? lane : StationRows::N - 1;
    const Tables *tb = a.tables;
    const double row_irr = tb->irr_norm[row_i], row_pn = tb->price_norm[row_i], row_pv = tb->pv_power[row_i],
                 row_price = tb->price[row_i];
    g.template issue<true, false>(e0, act, E, t0, vec_io, p, s, info, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) g.fpv[j] = g.fpr[j] = 1.0;
    g.issue_step_inputs_at(act_t, rec_t, E, vec_io, lane);
    wave_vmem_drain();
    rows->irr[row_i] = row_irr;
    rows->pnf[row_i] = (float)row_pn;
    rows->env[row_i][0] = row_pv;
    rows->env[row_i][1] = row_price;
    wave_lds_fence();
    const int t1 = t0 + a.nt;
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        g.stamp_step_top();
        // this step's ten table values from the staged rows, straight into vector registers: issued here, ahead of
        // the tile commit, and waited for (lgkmcnt) where the header and the env tail read them.  No scalar load, no
        // wait on one and no copy from scalar registers in the loop
        StepConst k;
        StationStep st;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            k.v[CST_IRR + j] = rows->irr[t + j];
            k.v[CST_PN + j] = 0.0;   // not read: the header takes st.pnf
            st.pnf[j] = rows->pnf[t + j];
        }
        k.v[CST_PV] = rows->env[t][0];
        k.v[CST_PRICE] = rows->env[t][1];
        st.rec_t = rec_t;
        g.take_step_inputs();
        g.day_tile.commit(lds, lane);
        wave_lds_fence();
        act_t += block;
        rec_t += plane;
        if (t + 1 < t1) g.issue_step_inputs_at(act_t, rec_t, E, vec_io, lane);
        g.template run<true, true>(lds, s_obs, obs, reward, done, E, t, vec_io, k, p, s, info, lane, &st);
        wave_lds_fence();
    }
    SNG_WSTAMP_FLUSH(g.stamp_, 5);
    g.store_state(E, p, s, info, lane);
    bump_day_counter<true>(p, s, t0);
}

// day_lean_kernel: the same for the lean family's stations (step_lean_kernel's: N <= 16, one lane per env), for
// both timeline encodings -- packed device-RNG days (PK) and the word / aux planes of reference-RNG, injected and
// replayed days.  Geometry as step_lean_kernel's: one wavefront per workgroup, 64 envs per wavefront, LeanLds<NC>
// and the same idle-lane convention.  The step is LeanGroup::run<KEEP = true>(), nothing is restated here; with the
// SoC in registers a step's first store is the reward store of the env tail, and step t + 1's inputs are issued
// ahead of it.
//   once a day:  the PV ratio, BESS SoC, t = 0 penalty, day return and every charger's SoC (the 16 B pairs of
//                sng_layout.h) are loaded before the first step; SoC, BESS SoC and the day return are stored after
//                the last, bess0 is written at t = 0 and the day counter advanced once (bump_day_counter<PK>).
//   every step:  the actions tile, record plane t + 1 (PK) or the word and aux planes of t, the requested-SoC
//                plane (REQ) and the ten table constants are read; observation rows, reward, done, flags and the
//                flag summary are stored as step_lean_kernel stores them.
// obs_step / out_step: floats between two steps' observation blocks and elements between two steps' reward and
// done blocks (SNG_GRAPH_TRAJECTORY: every step's outputs are kept), 0 when every step overwrites the same block.
// vec_io promises 16 B alignment of every step's block, so the caller clears it when obs_step is no multiple of 4.
//
// Registers.  At 65,536 envs the grid is 1,024 wavefronts, one per SIMD, so a wavefront may take the whole
// 512-entry file; smaller populations leave SIMDs empty.  Occupancy buys nothing here, and a spill would put
// scratch traffic on the path this kernel exists to shorten: the kernel asks for one wavefront per SIMD at least
// and bounds nothing above it (kDayLeanWaves), which leaves the allocator free to use what the prefetch needs
// (N = 16 unpacked with the requested SoC: 16 + 32 + 32 VGPRs of step t + 1's inputs next to run_[]'s 32).
// tests/test_day_lean_kernel_resources.py holds every instantiation to zero scratch and zero VGPR spills.
constexpr int kDayLeanWaves = 1;
template <int NC, bool PK, bool REQ>
__global__ __launch_bounds__(kLeanBlock) __attribute__((amdgpu_waves_per_eu(kDayLeanWaves))) void
day_lean_kernel(const float *__restrict__ act, float *__restrict__ obs, double *__restrict__ reward,
                uint8_t *__restrict__ done, int64_t E, int t0, int nt, int vec_io, int64_t obs_step, int64_t out_step,
                Params p, DeviceState s, InfoPtrs info) {
    static_assert(kLeanBlock == kWave, "one wavefront per workgroup");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    const LeanTiles<NC> tl(lds, 0);
    LeanGroup<NC, PK, REQ> g;
    const size_t block = (size_t)E * (size_t)p.act_dim;    // one step's actions
    g.template issue<true, false>((int64_t)blockIdx.x * kLeanBlock, act, E, t0, vec_io, p, s, info, lane);   // the day's state
    g.issue_step_inputs(act, E, t0, vec_io, p, s, lane);
    const int t1 = t0 + nt;
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        g.take_step_inputs(p);
        g.act_tile.commit(tl.s_act, lane);
        wave_lds_fence();
        const StepConst k = g.kn;
        if (t + 1 < t1)   // ahead of this step's stores
            g.issue_step_inputs(act + (size_t)(t + 1 - t0) * block, E, t + 1, vec_io, p, s, lane);
        g.template run<true>(tl.s_act, tl.s_obs, tl.s_pos, tl.s_neg, obs, reward, done, E, t, vec_io, k, p, s, info, lane);
        wave_lds_fence();   // the next step's tile writes stay behind this step's reads of both tiles
        obs += obs_step;
        reward += out_step;
        done += out_step;
    }
    g.store_state(E, p, s, info);
    bump_day_counter<PK>(p, s, t0);
}

}  // namespace sng
