// sng_step_day.h -- the day kernel (day_wide_kernel): the steps t0 .. t0 + nt - 1 of a packed (device-RNG) day in
// one launch, for the wide family's stations.  sng_graph_create captures it in place of the day's T dependent
// step_wide_kernel nodes: it is given every step's actions at capture, and envs never interact, so a wavefront
// can step its 64 / L envs through the whole day on its own -- no grid-wide synchronisation, no node boundary
// (1.6-1.9 us each, the end-of-kernel write-back the next node waits for included) and no state round trip.
// Needs sng_step_wide.h (WideGroup: the step's arithmetic is run<KEEP = true>(), nothing is restated here).
// Included by sng_kernels.hip only.
#pragma once

namespace sng {

// Step t + 1's loads (its actions tile, records, requested SoC and table constants) are issued before step t's
// first store.  A store counts in vmcnt ahead of every later load, so a load issued behind step t's stores waits
// for them; issued ahead of them it costs registers for the whole step (the raw records, the tile's registers
// and, with the stream, the requested SoC).
// Geometry as step_wide_kernel's: one wavefront per workgroup, WideLds<NC, L>::WENVS envs per wavefront, the
// same LDS tiles.  `act` is step t0's [E][act_dim] block, the later steps' blocks follow it.
//   once a day:  the PV ratio, BESS SoC, t = 0 penalty, day return, profile keys and every charger's SoC are
//                loaded before the first step and live in registers; SoC, BESS SoC and the day return are
//                stored after the last step, as the same f64 values memory would have carried from step to
//                step.  bess0 is written at t = 0 and the day counter advanced once, as by the step kernel.
//   every step:  the actions tile, record plane t + 1 (and the requested-SoC plane) are read, the table
//                constants come from s.tables by uniform loads, and the observation rows, reward, done, flags
//                and the flag summary are stored exactly as step_wide_kernel stores them.
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
    const int t1 = t0 + nt;
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        const StepConst k = g.kn;
        g.take_step_inputs();
        g.act_tile.commit(lds, lane);
        wave_lds_fence();
        if constexpr (NOISE) expand_profile_factors(p, keys, t, g.fpv, g.fpr);
        if (t + 1 < t1)   // ahead of this step's stores
            g.issue_step_inputs(act + (size_t)(t + 1 - t0) * block, E, t + 1, vec_io, p, s, lane);
        g.template run<true>(lds, s_obs, obs, reward, done, E, t, vec_io, k, p, s, info, lane);
        wave_lds_fence();   // the next step's tile writes stay behind this step's reads of both tiles
    }
    g.store_state(E, p, s, info, lane);
    bump_day_counter<true>(p, s, t0);
}

}  // namespace sng
