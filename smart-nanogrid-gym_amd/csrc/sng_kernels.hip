// sng_kernels.hip -- HIP kernels of the batched SmartNanogridEnv hot path (gfx950).
//
// The single device translation unit: the kernels live in the topical headers included below, in the order
// the code object has always had them, and this file holds the bandwidth probe and every launch wrapper
// (sng_launch.h).
//
// Step kernel mapping: a wavefront steps 64 / L environments, L lanes per environment (L = 1, 2 or 4), and
// keeps its own LDS tiles (no workgroup barrier).  The lean and the wide kernel run one wavefront per
// workgroup; the general kernel four (256 threads) while a station's tiles fit (N <= 16), else one.  Lane
// `part` of an env owns a range of chargers; the env's first lane (the leader) finishes the env (sums, BESS,
// cost, reward).
//
// Per-env state is SoA with the env index fastest (sng_layout.h), so every per-charger
// load/store of a wavefront is a contiguous run.  The policy-facing row-major actions
// [E][A] and observations [E][O] are staged through LDS so their HBM side is a contiguous,
// 16-byte-per-lane stream.
//
// Arithmetic follows the reference operation for operation (built with -ffp-contract=off;
// the two explicit fma-based divisions of sng_dev_env.h are exact, see their comments).  Sums over
// chargers use the reference's order: numpy's pairwise sum for the charging powers
// (charging_station.py:293-294) and Python's left-to-right sum() for the vehicle penalties
// (penaliser.py:55).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

#include "sng.h"
#include "sng_graph_form.h"
#include "sng_launch.h"
#include "sng_layout.h"
#include "sng_step_plan.h"

#include "sng_dev_util.h"       // buffer access, LDS tile stagers, the diagnostic hooks
#include "sng_dev_sums.h"       // numpy's pairwise sum
#include "sng_exact_sum.h"      // when a running sum of positive powers is that sum (day_station_kernel)
#include "sng_dev_env.h"        // one env's step arithmetic: charger, BESS, env tail
#include "sng_step_lean.h"      // step_lean_kernel
#include "sng_step_wide.h"      // step_wide_kernel
#include "sng_step_day.h"       // day_wide_kernel, day_station_kernel, day_lean_kernel
#include "sng_step_general.h"   // step_kernel
#include "sng_generate.h"       // observe0_kernel, profile_kernel, generate_kernel
#include "sng_policy.h"         // mlp_actor_tile, policy_kernel
#include "sng_policy_net.h"     // policy_net_kernel
#include "sng_ppo.h"            // rollout_gae_kernel
#include "sng_ppo_net.h"        // value_net_kernel, gae_scan_kernel
#include "sng_noise.h"          // action_noise_kernel
#include "sng_ddpg.h"           // replay_push_kernel, replay_sample_kernel, q_net_kernel
#include "sng_ddpg_learn.h"     // learn_concat_kernel, learn_gemm_kernel, learn_loss_kernel, learn_step_kernel

namespace sng {

// ---------------------------------------------------------------------------------
// Bandwidth probe (diagnostics, sng_bandwidth_probe): the measured ceiling the step kernel's roofline is
// quoted against.  One float4 per thread: thread i reads in[i] when i < nr and writes out[i] when
// i < nw (nontemporal, the step's store policy), so one dispatch moves 16 (nr + nw) bytes.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void probe_copy_kernel(const float4 *__restrict__ in, float4 *__restrict__ out,
                                                         int64_t nr, int64_t nw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    typedef float v4f __attribute__((ext_vector_type(4)));
    v4f v = {0.f, 0.f, 0.f, 0.f};
    if (i < nr) v = reinterpret_cast<const v4f *>(in)[i];
    if (i < nw) __builtin_nontemporal_store(v, reinterpret_cast<v4f *>(out) + i);
}

// ---------------------------------------------------------------------------------
// launch wrappers (called from sng_api.cpp, sng_state.cpp and sng_graph.cpp, declared in sng_launch.h)
// ---------------------------------------------------------------------------------
// One launch, with optional start/stop events (both or neither): hipExtLaunchKernel stamps them with the
// dispatch's own begin/end timestamps, i.e. the kernel's device time.
template <class Kernel, class... Args>
static hipError_t launch_kernel(Kernel kern, dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                                hipEvent_t ev_start, hipEvent_t ev_stop, Args... args) {
    if (ev_start && ev_stop)
        hipExtLaunchKernelGGL(kern, grid, block, (uint32_t)lds, stream, ev_start, ev_stop, 0u, args...);
    else
        hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
    return hipGetLastError();
}

hipError_t launch_probe_copy(const void *in, void *out, int64_t nr, int64_t nw, hipStream_t stream, hipEvent_t a,
                             hipEvent_t b) {
    const int64_t n = nr > nw ? nr : nw;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    return launch_kernel(probe_copy_kernel, grid, block, 0, stream, a, b, (const float4 *)in, (float4 *)out, nr, nw);
}

SNG_DIAG_SET_STAMPS   // diagnostic builds: sng_debug_set_stamps

// A plan's kernel and launch geometry.  The lean and the wide kernel share one signature (this step's table
// constants by value, StepConst); the general kernel reads them through the tables pointer.
typedef void (*ConstStepKernel)(const float *, float *, double *, uint8_t *, int64_t, int, int, StepConst, Params,
                                DeviceState, InfoPtrs);
typedef void (*GeneralStepKernel)(Params, DeviceState, InfoPtrs, const float *, float *, double *, uint8_t *, int64_t,
                                  int, int);
struct StepLaunch {
    ConstStepKernel by_const = nullptr;   // STEP_LEAN, STEP_WIDE
    GeneralStepKernel general = nullptr;   // STEP_GENERAL
    dim3 grid, block;
    size_t lds = 0;
};

static dim3 blocks_for(int64_t E, int envs_per_block) { return dim3((unsigned)((E + envs_per_block - 1) / envs_per_block)); }

template <int NC>
static StepLaunch lean_launch(const StepPlan &pl, int64_t E) {
    static constexpr ConstStepKernel k[2][2] = {{step_lean_kernel<NC, false, false>, step_lean_kernel<NC, false, true>},
                                                {step_lean_kernel<NC, true, false>, step_lean_kernel<NC, true, true>}};
    return {k[pl.pk][pl.req], nullptr, blocks_for(E, kLeanBlock), dim3(kLeanBlock), LeanLds<NC>::BYTES};
}

template <int NC>
static StepLaunch wide_launch(const StepPlan &pl, int64_t E) {
    constexpr int L = kWideLanes;
    static constexpr ConstStepKernel k[2][2][2] = {
        {{step_wide_kernel<NC, L, false, false, false>, step_wide_kernel<NC, L, false, false, true>},
         {step_wide_kernel<NC, L, false, true, false>, step_wide_kernel<NC, L, false, true, true>}},
        {{step_wide_kernel<NC, L, true, false, false>, step_wide_kernel<NC, L, true, false, true>},
         {step_wide_kernel<NC, L, true, true, false>, step_wide_kernel<NC, L, true, true, true>}}};
    using Lay = WideLds<NC, L>;   // one wavefront of WENVS envs per workgroup
    return {k[pl.pk][pl.req][pl.noise], nullptr, blocks_for(E, Lay::WENVS), dim3(kWave), Lay::BYTES};
}

template <int NC, int L>
static StepLaunch general_launch(const StepPlan &pl, const Params &p, int64_t E) {
    static constexpr GeneralStepKernel k[2][2][2] = {
        {{step_kernel<NC, L, false, false, false>, step_kernel<NC, L, false, false, true>},
         {step_kernel<NC, L, false, true, false>, step_kernel<NC, L, false, true, true>}},
        {{step_kernel<NC, L, true, false, false>, step_kernel<NC, L, true, false, true>},
         {step_kernel<NC, L, true, true, false>, step_kernel<NC, L, true, true, true>}}};
    using Lay = StepLds<NC, L>;
    return {nullptr, k[pl.diag][pl.fast][pl.pk], blocks_for(E, Lay::ENVS), dim3(Lay::BLOCK),
            Lay::bytes(p.act_dim, p.obs_dim)};
}

template <int NC>
static StepLaunch general_launch_lanes(const StepPlan &pl, const Params &p, int64_t E) {
    return pl.lanes == 4   ? general_launch<NC, 4>(pl, p, E)
           : pl.lanes == 2 ? general_launch<NC, 2>(pl, p, E)
                           : general_launch<NC, 1>(pl, p, E);
}

// Calls f with the run-time value `nc` (a station size, mostly) as a compile-time constant (an integral_constant) where
// it is one of Ns; false, and no call, for any other value.  with_lean_size: the lean sizes of kStationSizes (sng_step_plan.h).
template <int... Ns, class F>
static bool with_size(int nc, F f) {
    return ((nc == Ns && (f(std::integral_constant<int, Ns>{}), true)) || ...);
}
template <class F>
static bool with_lean_size(int nc, F f) {
    return with_size<1, 2, 4, 8, 10, 16>(nc, f);
}

// The map from a plan to its kernel: one case per compiled station size of kStationSizes (sng_step_plan.h).  A
// plan without a case here has no kernel (launch_step fails; tests/test_step_plan_cpu.py holds every name a
// plan can give against the code object's symbols).
static StepLaunch step_launch(const StepPlan &pl, const Params &p, int64_t E) {
    StepLaunch l;
    switch (pl.family) {
        case STEP_LEAN: with_lean_size(pl.nc, [&](auto n) { l = lean_launch<decltype(n)::value>(pl, E); }); break;
        case STEP_WIDE: with_size<10, 50>(pl.nc, [&](auto n) { l = wide_launch<decltype(n)::value>(pl, E); }); break;
        case STEP_GENERAL:   // a runtime N and one charger run one lane per env only
            if (!with_size<0, 1>(pl.nc, [&](auto n) { l = general_launch<decltype(n)::value, 1>(pl, p, E); }))
                with_size<2, 4, 8, 10, 16, 50>(pl.nc, [&](auto n) { l = general_launch_lanes<decltype(n)::value>(pl, p, E); });
            break;
    }
    return l;
}

hipError_t launch_step(const Params &p, const DeviceState &s, const InfoPtrs &info, const Tables &tab,
                       const float *act, float *obs, double *reward, uint8_t *done, int64_t E, int t, int vec_io,
                       hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop) {
    const StepLaunch l = step_launch(step_plan(p, info_diag(info)), p, E);
    if (l.general)
        return launch_kernel(l.general, l.grid, l.block, l.lds, stream, ev_start, ev_stop, p, s, info, act, obs, reward,
                             done, E, t, vec_io);
    if (!l.by_const) return hipErrorInvalidDeviceFunction;   // a plan without a compiled kernel
    StepConst k;
    for (int i = 0; i < CST_COUNT; ++i) k.v[i] = step_constant(&tab, t, i);
    return launch_kernel(l.by_const, l.grid, l.block, l.lds, stream, ev_start, ev_stop, act, obs, reward, done, E, t,
                         vec_io, k, p, s, info);
}

// The day kernels (sng_step_day.h): day_wide_kernel and day_station_kernel for the packed days of the wide family's
// 10-charger station, day_lean_kernel for the lean family's plans; every other plan has none.  Which of them a
// captured day runs is decided before launch_day is called (sng_graph_form.h graph_form).  N = 50 is not compiled:
// with every charger's SoC kept next to the step's 239 VGPRs it spills (325-423 VGPR spills, 0.8-1 KB of scratch),
// so config 5's days stay T step nodes.
typedef void (*DayKernel)(const float *, float *, double *, uint8_t *, int64_t, int, int, int, Params, DeviceState,
                          InfoPtrs);
typedef void (*DayLeanKernel)(const float *, float *, double *, uint8_t *, int64_t, int, int, int, int64_t, int64_t,
                              Params, DeviceState, InfoPtrs);
template <int NC>
static StepLaunch day_launch(const StepPlan &pl, int64_t E, DayKernel &kern) {
    constexpr int L = kWideLanes;
    static constexpr DayKernel k[2][2] = {{day_wide_kernel<NC, L, false, false>, day_wide_kernel<NC, L, false, true>},
                                          {day_wide_kernel<NC, L, true, false>, day_wide_kernel<NC, L, true, true>}};
    using Lay = WideLds<NC, L>;
    kern = k[pl.req][pl.noise];
    return {nullptr, nullptr, blocks_for(E, Lay::WENVS), dim3(kWave), Lay::BYTES};
}
// an instantiation day_lean_compiled (sng_step_plan.h) leaves out is not instantiated
template <int NC, bool PK, bool REQ>
static DayLeanKernel day_lean_entry() {
    if constexpr (day_lean_compiled(NC, PK, REQ)) return day_lean_kernel<NC, PK, REQ>;
    else return nullptr;
}
template <int NC>
static StepLaunch day_lean_launch(const StepPlan &pl, int64_t E, DayLeanKernel &kern) {
    const DayLeanKernel k[2][2] = {{day_lean_entry<NC, false, false>(), day_lean_entry<NC, false, true>()},
                                   {day_lean_entry<NC, true, false>(), day_lean_entry<NC, true, true>()}};
    kern = k[pl.pk][pl.req];
    return {nullptr, nullptr, blocks_for(E, kLeanBlock), dim3(kLeanBlock), LeanLds<NC>::BYTES};
}

hipError_t launch_day(DayNode node, const Params &p, const DeviceState &s, const InfoPtrs &info, const float *act,
                      float *obs, double *reward, uint8_t *done, int64_t E, int t0, int nt, int vec_io, hipStream_t stream,
                      int64_t obs_step, int64_t out_step) {
    const StepPlan pl = step_plan(p, info_diag(info));
    // the node graph_form decided is one of the plan's family (and the station kernel only its own station's)
    const DayFamily fam = day_kernel_of(pl, obs_step != 0 || out_step != 0);
    const bool wide = node == DAY_KERNEL_WIDE || node == DAY_KERNEL_STATION;
    if (fam == DAY_NONE || (fam == DAY_WIDE) != wide || (fam == DAY_LEAN) != (node == DAY_KERNEL_LEAN) ||
        (node == DAY_KERNEL_STATION && !day_station_fixed(pl, p)))
        return hipErrorNotSupported;
    if (t0 < 0 || nt < 1 || t0 + nt > p.T) return hipErrorInvalidValue;
    if (wide) {
        DayKernel kern = nullptr;
        const StepLaunch l = day_launch<10>(pl, E, kern);
        if (node == DAY_KERNEL_STATION) {
            static_assert(kDayStationN == 10 && kWideLanes == 2, "day_launch<10>'s geometry");
            const DayStationArgs a{act, obs, reward, done, E, t0, nt, vec_io, p.bump_day, p.dt_f, p.ev_power_f, p.ev_eff_f,
                                   p.dt, p.rdt, p.bess_cap, p.bess_pmax_ch, p.bess_pmax_dis, p.bess_eff_ch,
                                   p.bess_eff_dis, p.bess_dod, p.grid_w, p.bat_pen_w, p.sell_coef, s.soc, s.bess,
                                   s.bess0, s.ratio, s.pen0, s.aux, s.flags, s.episode, s.tables, info.flags,
                                   info.flag_any, info.episode_return};
            // the two tiles and, behind them, the day's table rows (this kernel alone)
            return launch_kernel(day_station_kernel<kDayStationN, kWideLanes>, l.grid, l.block,
                                 l.lds + sizeof(StationRows), stream, nullptr, nullptr, a);
        }
        return launch_kernel(kern, l.grid, l.block, l.lds, stream, nullptr, nullptr, act, obs, reward, done, E, t0, nt,
                             vec_io, p, s, info);
    }
    DayLeanKernel kern = nullptr;
    StepLaunch l;
    with_lean_size(pl.nc, [&](auto n) { l = day_lean_launch<decltype(n)::value>(pl, E, kern); });
    if (!kern) return hipErrorInvalidDeviceFunction;   // a plan without a compiled kernel
    // every step's observation block 16 B aligned, or none is promised to be
    if (obs_step % 4 != 0) vec_io = 0;
    return launch_kernel(kern, l.grid, l.block, l.lds, stream, nullptr, nullptr, act, obs, reward, done, E, t0, nt,
                         vec_io, obs_step, out_step, p, s, info);
}

hipError_t launch_observe0(const Params &p, const DeviceState &s, float *obs, double *ep_return, int64_t E,
                           int vec_io, hipStream_t stream, int mode, int64_t replay, const RefStreams *ps, int py) {
    const RefStreams no_streams{nullptr, nullptr};
    const RefStreams &pss = (py && ps) ? *ps : no_streams;
    if (!ps) py = 0;
    // 256 envs per workgroup while their [256][obs_dim] LDS tile fits 64 KB, else one wavefront's
    const bool big = (size_t)round4(256 * p.obs_dim) * 4 <= 64 * 1024;
    const int envs = big ? 256 : kWave;
    auto kern = big ? (p.packed ? observe0_kernel<256, true> : observe0_kernel<256, false>)
                    : (p.packed ? observe0_kernel<kWave, true> : observe0_kernel<kWave, false>);
    return launch_kernel(kern, blocks_for(E, envs), dim3(envs), (size_t)round4(envs * p.obs_dim) * 4, stream, nullptr,
                         nullptr, p, s, obs, ep_return, E, vec_io, mode, replay, pss, py);
}

// A whole device-RNG reset.  The t = 0 observation runs as extra blocks of the generator's grid
// while its [256][obs_dim] LDS tile stays small next to the vehicle lists (N <= 16: at most 42 KB,
// a few generator workgroups per CU still fit); wider stations keep profile_kernel and
// observe0_kernel as separate launches behind the generator.
// day_delta != 0 or obs == nullptr: an overlapped reset graph's generator (sng_graph_form.h reset_overlapped), the
// one-launch form only.
hipError_t launch_generate(const Params &p, const DeviceState &s, uint64_t seed, int64_t E, int i4, int i10, int i1,
                           float *obs, double *ep_return, int vec_io, hipStream_t stream, hipEvent_t ev_start,
                           hipEvent_t ev_stop, int day_delta, size_t min_lds) {
    const size_t veh = generate_lds_bytes(p.req_enabled != 0), tile = (size_t)round4(kObsEnvs * p.obs_dim) * 4;
    const bool fused = generator_fused(p);   // up to 60 chargers (config 5's 50: 27.9 KB)
    if (!fused && (day_delta != 0 || !obs)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((E + kGenBlock - 1) / kGenBlock), (unsigned)(gen_rows(p.n) + (fused ? kObsBlocks : 0))),
        block(kGenBlock);
    size_t lds = (fused && obs && tile > veh) ? tile : veh;   // no row, no tile
    if (min_lds > lds) lds = min_lds;   // fewer workgroups per CU (overlapped_generator_lds)
    const bool req = p.req_enabled != 0;
    auto kern = p.T == 24 ? (req ? generate_kernel<24, true> : generate_kernel<24, false>)
                : (p.T == 96 && !req) ? generate_kernel<96, false>   // config 5's 15-minute day
                : (req ? generate_kernel<0, true> : generate_kernel<0, false>);
    if (fused && ev_start && ev_stop)   // the one-launch reset, timed by its own dispatch timestamps
        return launch_kernel(kern, grid, block, lds, stream, ev_start, ev_stop, p, s, seed, E, i4, i10, i1, obs,
                             ep_return, vec_io, day_delta);
    if (ev_start) (void)hipEventRecord(ev_start, stream);
    hipError_t e = launch_kernel(kern, grid, block, lds, stream, nullptr, nullptr, p, s, seed, E, i4, i10, i1, obs,
                                 ep_return, vec_io, day_delta);
    if (!fused) {
        if (e == hipSuccess) e = launch_profiles(p, s, E, stream);
        // the PV ratio and pen0 of the day, from the streams, as the fused t = 0 blocks do
        if (e == hipSuccess) e = launch_observe0(p, s, obs, ep_return, E, vec_io, stream, OBS0_DEVICE, -1);
    }
    if (e == hipSuccess && ev_stop) e = hipEventRecord(ev_stop, stream);
    return e;
}

}  // namespace sng

// the MT19937 kernels and ref_day2_kernel: here, behind probe_copy_kernel, as the code object has them
#include "sng_ref_day.h"

namespace sng {

// Envs per workgroup of ref_day2_kernel: each drawing wavefront's day is one serial chain (an env's stream
// is consumed charger after charger), so small populations spread over more, thinner workgroups.
static int ref_day2_envs(int64_t E) {
    return E >= 65536 ? 64 : E >= 16384 ? 32 : E >= 4096 ? 16 : 8;
}

// more than 64 KB of dynamic LDS (four groups of 64 envs: up to 144 KB) is allowed once per kernel; a
// refusal surfaces as the launch's error
template <int TT, bool REQ, int ENVS>
static void launch_ref_day2_envs(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Params &p,
                                 const DeviceState &s, const RefStreams &rs, int64_t E, int i4, int i10, int i1) {
    static const hipError_t set = hipFuncSetAttribute(reinterpret_cast<const void *>(ref_day2_kernel<TT, REQ, ENVS>),
                                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                                      (int)ref_day2_lds_bytes(REQ, ENVS));
    (void)set;
    hipLaunchKernelGGL((ref_day2_kernel<TT, REQ, ENVS>), grid, block, lds, stream, p, s, rs, E, i4, i10, i1);
}

template <int TT, bool REQ>
static void launch_ref_day2(const Params &p, const DeviceState &s, const RefStreams &rs, int64_t E, int i4, int i10,
                            int i1, hipStream_t stream) {
    const int envs = ref_day2_envs(E);
    const int64_t per = (int64_t)envs * kRefGroups;   // envs per workgroup
    const dim3 grid((unsigned)((E + per - 1) / per)), block(kRefBlock);
    const size_t lds = ref_day2_lds_bytes(REQ, envs);
    with_size<8, 16, 32, 64>(envs, [&](auto n) {
        launch_ref_day2_envs<TT, REQ, decltype(n)::value>(grid, block, lds, stream, p, s, rs, E, i4, i10, i1);
    });
}

hipError_t launch_ref_seed(const RefStreams &rs, uint64_t seed0, int64_t E, hipStream_t stream) {
    hipLaunchKernelGGL(mt_seed_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, stream, rs, seed0, E);
    return hipGetLastError();
}

hipError_t launch_mt_prepare(const RefStreams &rs, int64_t E, hipStream_t stream) {
    hipLaunchKernelGGL(mt_prepare_kernel, dim3((unsigned)((E + 3) / 4)), dim3(256), 0, stream, rs, E);
    return hipGetLastError();
}

// One reference-RNG day of every env into the word / aux (/ req) planes; ratio, pen0 and the t = 0
// observation are the caller's (launch_observe0, which draws the Python streams).
// prepare = false: the streams' blocks were prepared for this day already (sng_reset prepares the next
// day's on a side stream while a day is stepped)
hipError_t launch_ref_day(const Params &p, const DeviceState &s, const RefStreams &rs, int64_t E, int i4, int i10,
                          int i1, bool prepare, hipStream_t stream) {
    if (prepare) {
        hipError_t e = launch_mt_prepare(rs, E, stream);
        if (e != hipSuccess) return e;
    }
    const bool req = p.req_stream != 0;
    auto launch = p.T == 24 ? (req ? launch_ref_day2<24, true> : launch_ref_day2<24, false>)
                            : (req ? launch_ref_day2<0, true> : launch_ref_day2<0, false>);
    launch(p, s, rs, E, i4, i10, i1, stream);
    return hipGetLastError();
}

// Atomic, as the first step's own advance is (bump_day_counter): in an overlapped reset graph the bump node
// behind the last generator and the last day's first step are not ordered, and nothing reads the counter then.
__global__ void bump_day_kernel(DeviceState s, uint64_t amount) {
    __hip_atomic_fetch_add(s.episode, amount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t launch_bump_day(const DeviceState &s, hipStream_t stream, uint64_t amount) {
    hipLaunchKernelGGL(bump_day_kernel, dim3(1), dim3(1), 0, stream, s, amount);
    return hipGetLastError();
}

typedef void (*PolicyDayKernel)(const float *, PolicyImage, const float *, int64_t, int, const float *, float *, float *,
                                double *, uint8_t *, int64_t, int, int, int, int, int64_t, int64_t, int64_t, Params,
                                DeviceState, InfoPtrs);
// an instantiation policy_day_compiled (sng_step_plan.h) leaves out is not instantiated
template <int NC, bool PK, bool REQ>
static PolicyDayKernel policy_day_entry() {
    if constexpr (policy_day_compiled(NC, PK, REQ)) return day_lean_policy_kernel<NC, PK, REQ>;
    else return nullptr;
}
template <int NC>
static StepLaunch policy_day_launch(const StepPlan &pl, int64_t E, PolicyDayKernel &kern) {
    const PolicyDayKernel k[2][2] = {{policy_day_entry<NC, false, false>(), policy_day_entry<NC, false, true>()},
                                     {policy_day_entry<NC, true, false>(), policy_day_entry<NC, true, true>()}};
    kern = k[pl.pk][pl.req];
    return {nullptr, nullptr, blocks_for(E, kLeanBlock), dim3(kLeanBlock), PolicyDayLds<NC>::BYTES};
}

hipError_t launch_policy_day(const Params &p, const DeviceState &s, const InfoPtrs &info, const float *img,
                             const PolicyImage &m, const float *noise, const float *obs0, float *obs,
                             float *actions_out, double *reward, uint8_t *done, int64_t E, int vec_io,
                             hipStream_t stream, int64_t obs_step, int64_t out_step, int64_t act_step) {
    const StepPlan pl = step_plan(p, info_diag(info));
    if (m.O != p.obs_dim || m.A != p.act_dim) return hipErrorInvalidValue;
    PolicyDayKernel kern = nullptr;
    StepLaunch l;
    if (pl.family == STEP_LEAN)
        with_lean_size(pl.nc, [&](auto n) { l = policy_day_launch<decltype(n)::value>(pl, E, kern); });
    if (!kern) return hipErrorInvalidDeviceFunction;   // a plan without a compiled kernel
    // every step's block 16 B aligned, or none is promised to be
    const int64_t noise_step = noise ? E * (int64_t)p.act_dim : 0;
    if (obs_step % 4 != 0 || !aligned16(obs0) || !aligned16(noise) || noise_step % 4 != 0) vec_io = 0;
    const int vec_act = (aligned16(actions_out) && act_step % 4 == 0) ? 1 : 0;
    // without noise the prefetch reads step 0's block of a, which is never used
    return launch_kernel(kern, l.grid, l.block, l.lds, stream, nullptr, nullptr, img, m, noise ? noise : actions_out,
                         noise_step, noise ? 1 : 0, obs0, obs, actions_out, reward, done, E, 0, p.T, vec_io, vec_act,
                         obs_step, out_step, act_step, p, s, info);
}

// One workgroup's tiles are more than 64 KB of dynamic LDS from 46 chargers on (150,528 B at 128): allowed once
// per kernel, up to the CU's 160 KB, and asked for when the first policy is created -- outside any stream capture.
// raise_lds_limit asks for every kernel of its list and returns the first refusal; the *_kernels_init functions
// keep its answer.
template <class... Kernels>
static hipError_t raise_lds_limit(int bytes, Kernels... kernels) {
    hipError_t first = hipSuccess;
    for (const void *k : {reinterpret_cast<const void *>(kernels)...}) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (first == hipSuccess) first = e;
    }
    return first;
}
constexpr int kPolicyMaxLds = 160 * 1024;
hipError_t policy_kernels_init() {
    static const hipError_t set = raise_lds_limit(kPolicyMaxLds, policy_kernel<false>, policy_kernel<true>,
                                                  policy_net_kernel<false>, policy_net_kernel<true>);
    return set;
}

template <bool TANH>
static hipError_t launch_policy_kernel(const float *img, const PolicyImage &m, const float *obs, const float *noise,
                                       float *actions, float *env_actions, int64_t E, hipStream_t stream) {
    const size_t lds = policy_lds_bytes(m.O, m.A);
    if (lds > (size_t)kPolicyMaxLds) return hipErrorInvalidValue;
    if (lds > 64u * 1024u && policy_kernels_init() != hipSuccess) return policy_kernels_init();
    const int vec = (aligned16(obs) && aligned16(noise) && aligned16(actions) && aligned16(env_actions)) ? 1 : 0;
    return launch_kernel(policy_kernel<TANH>, blocks_for(E, kWave), dim3(kPolicyBlock), lds, stream, nullptr, nullptr, img, m,
                         obs, noise, actions, env_actions, E, vec);
}

hipError_t launch_policy(const float *img, const PolicyImage &m, const float *obs, const float *noise, float *actions,
                         float *env_actions, int64_t E, hipStream_t stream) {
    return m.activation == POLICY_RELU ? launch_policy_kernel<false>(img, m, obs, noise, actions, env_actions, E, stream)
                                       : launch_policy_kernel<true>(img, m, obs, noise, actions, env_actions, E, stream);
}

// policy_net_kernel: 64 rows a workgroup; its LDS (hidden1's rows and the shared region) is above 64 KB from a
// hidden1 of 224 on.
hipError_t launch_policy_net(const float *img, const NetImage &m, const float *obs, const float *noise, float *actions,
                             float *env_actions, int64_t E, hipStream_t stream) {
    static_assert(kNetMaxLds == (size_t)kPolicyMaxLds, "one limit for the policy kernels");
    const size_t lds = net_lds_bytes(m);
    if (lds > kNetMaxLds || m.N3 > kNetMaxAct) return hipErrorInvalidValue;   // what net_spec_check refuses
    if (lds > 64u * 1024u && policy_kernels_init() != hipSuccess) return policy_kernels_init();
    const dim3 grid = blocks_for(E, kNetRows), block(kNetBlock);
    auto kern = m.activation == POLICY_RELU ? policy_net_kernel<false> : policy_net_kernel<true>;
    return launch_kernel(kern, grid, block, lds, stream, nullptr, nullptr, img, m, obs, noise, actions, env_actions, E);
}

// rollout_gae_kernel's dynamic-LDS limit, raised once as policy_kernels_init raises the policy kernels': two observation
// tiles, the hidden rows and the noise tile are more than 64 KB from 35 chargers on.
hipError_t ppo_kernels_init() {
    static const hipError_t set = raise_lds_limit(kPpoMaxLds, rollout_gae_kernel<false>, rollout_gae_kernel<true>);
    return set;
}

// Two observation tiles (the step before's is prefetched beside the layers) where they fit a compute unit's LDS with
// the hidden rows and the noise tile, else one.
hipError_t launch_rollout_gae(const float *img, const PpoImage &m, const SngPpoRollout &r, int64_t E, int T,
                              hipStream_t stream) {
    const float *noise = r.logp ? r.noise : nullptr;   // no log-probability stage without both
    const bool two = ppo_lds_bytes(m.v.O, m.head.A, true, noise != nullptr) <= (size_t)kPpoMaxLds;
    const size_t lds = ppo_lds_bytes(m.v.O, m.head.A, two, noise != nullptr);
    if (lds > (size_t)kPpoMaxLds || T < 1 || E < 1 || r.days < 1 || r.days > kPpoMaxLaunchDays) return hipErrorInvalidValue;
    if (lds > 64u * 1024u && ppo_kernels_init() != hipSuccess) return ppo_kernels_init();
    // every step's block 16 B aligned, or none is promised to be
    const int vec_obs = (aligned16(r.obs) && (E * (int64_t)m.v.O) % 4 == 0) ? 1 : 0;
    const int vec_noise = (aligned16(noise) && (E * (int64_t)m.head.A) % 4 == 0) ? 1 : 0;
    const dim3 grid((unsigned)((E + kWave - 1) / kWave), (unsigned)r.days), block(kPolicyBlock);
    const float g = ppo_gamma_f32(r.gamma), gl = ppo_gamma_lambda_f32(r.gamma, r.gae_lambda);
    auto kern = m.v.activation == POLICY_RELU ? rollout_gae_kernel<false> : rollout_gae_kernel<true>;
    return launch_kernel(kern, grid, block, lds, stream, nullptr, nullptr, img, m, r.obs, r.reward, r.done, noise, r.values,
                         r.advantages, r.returns, r.logp, E, T, g, gl, two ? 1 : 0, vec_obs, vec_noise);
}

// value_net_kernel's dynamic-LDS limit, raised once as policy_kernels_init raises policy_net_kernel's: the same tiles,
// above 64 KB from a hidden1 of 224 on.
hipError_t ppo_net_kernels_init() {
    static const hipError_t set = raise_lds_limit((int)kNetMaxLds, value_net_kernel<false>, value_net_kernel<true>);
    return set;
}

// The two launches of a net head's sng_ppo_finish: value_net_kernel over the trajectory's rows as one flat batch, then
// gae_scan_kernel, whose grid rows are the days and, with the log-probability stage, the T steps.
hipError_t launch_ppo_net(const float *img, const PpoNetImage &m, const SngPpoRollout &r, int64_t E, int T,
                          hipStream_t stream) {
    const float *noise = r.logp ? r.noise : nullptr;   // no log-probability stage without both
    const size_t lds = net_lds_bytes(m.v);
    if (T < 1 || E < 1 || r.days < 1) return hipErrorInvalidValue;
    const int64_t rows = ppo_net_rows(r.days, T, E), scan_rows = (int64_t)r.days + (noise ? T : 0);
    // what ppo_net_spec_check and sng_ppo_finish refuse
    if (lds > kNetMaxLds || m.v.N3 != kNetTile || gae_scan_lds_bytes(m.head.A) > 64u * 1024u ||
        ppo_net_blocks(rows) > kPpoNetMaxBlocks || scan_rows > kPpoMaxLaunchDays)
        return hipErrorInvalidValue;
    if (lds > 64u * 1024u && ppo_net_kernels_init() != hipSuccess) return ppo_net_kernels_init();
    const dim3 grid((unsigned)ppo_net_blocks(rows)), block(kNetBlock);
    auto kern = m.v.activation == POLICY_RELU ? value_net_kernel<false> : value_net_kernel<true>;
    const hipError_t e = launch_kernel(kern, grid, block, lds, stream, nullptr, nullptr, img, m.v, r.obs, r.values, rows);
    if (e != hipSuccess) return e;
    const dim3 sgrid((unsigned)((E + kScanBlock - 1) / kScanBlock), (unsigned)scan_rows), sblock(kScanBlock);
    const float g = ppo_gamma_f32(r.gamma), gl = ppo_gamma_lambda_f32(r.gamma, r.gae_lambda);
    const float *values = r.values;
    const GaussHead &h = m.head;
    auto scan = noise ? gae_scan_kernel<true> : gae_scan_kernel<false>;
    return launch_kernel(scan, sgrid, sblock, noise ? gae_scan_lds_bytes(h.A) : 0, stream, nullptr, nullptr, img, h.log_std,
                         h.inv_std, (int)h.A, r.reward, r.done, noise, values, r.advantages, r.returns, r.logp, E, T,
                         (int)r.days, g, gl);
}

// A source's fill and, behind it, its counter's bump: grid x over the row's groups of four elements, y over the blocks.
hipError_t launch_noise_fill(const SngNoiseSpec &spec, const float *params, uint64_t *counter, int64_t env_offset,
                             float *out, int32_t days, int T, int64_t E, hipStream_t stream) {
    const int A = spec.act_dim;
    if (days < 1 || T < 1 || E < 1 || A < 1 || A > kNoiseMaxAct || !params || !counter || !out) return hipErrorInvalidValue;
    const int64_t row = E * (int64_t)A, per = (int64_t)kNoiseBlock * kNoisePer;
    const int64_t blocks = (row + per - 1) / per;
    if (blocks > 2147483647ll) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks, (unsigned)(days < kNoiseMaxGridDays ? days : kNoiseMaxGridDays)), block(kNoiseBlock);
    const int vec = (aligned16(out) && row % 4 == 0) ? 1 : 0;
    const float theta = (float)spec.theta, dt = (float)spec.dt;
    auto kern = spec.kind == SNG_NOISE_OU ? action_noise_kernel<SNG_NOISE_OU> : action_noise_kernel<SNG_NOISE_GAUSSIAN>;
    const hipError_t e = launch_kernel(kern, grid, block, 0, stream, nullptr, nullptr, params, (const uint64_t *)counter,
                                       spec.seed, env_offset, theta, dt, out, (int)days, T, E, A, vec);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(noise_bump_kernel, dim3(1), dim3(1), 0, stream, counter, (uint64_t)days);
    return hipGetLastError();
}

// grid x over the longest segment's 16-byte groups, kPushPer a thread (the others' threads run out of work sooner), y
// over the segments
hipError_t launch_replay_push(const PushArgs &a, hipStream_t stream) {
    if (a.count < 1 || a.count > kPushSegments || a.longest < 1) return hipErrorInvalidValue;
    for (int i = 0; i < a.count; ++i)
        if (!a.seg[i].src || !a.seg[i].dst || a.seg[i].n < 1) return hipErrorInvalidValue;
    const int64_t per = (int64_t)kPushBlock * kPushPer * 4;   // elements of a workgroup, at 4-byte elements
    int64_t blocks = (a.longest + per - 1) / per;
    blocks = blocks < 1 ? 1 : blocks > (1 << 20) ? (1 << 20) : blocks;
    return launch_kernel(replay_push_kernel, dim3((unsigned)blocks, (unsigned)a.count), dim3(kPushBlock), 0, stream,
                         nullptr, nullptr, a);
}

hipError_t launch_replay_sample(const ReplayStorage &ring, const SngReplayBatch &out, uint32_t key, uint64_t n, int T,
                                int64_t E, int O, int A, int64_t batch, hipStream_t stream) {
    if (batch < 1 || n < 1 || T < 1 || E < 1 || O < 1 || A < 1 || !ring.obs || !ring.actions || !ring.reward ||
        !ring.done || !out.obs || !out.actions || !out.next_obs || !out.reward || !out.done)
        return hipErrorInvalidValue;
    const int64_t blocks = (batch + kSampleRows - 1) / kSampleRows;
    if (blocks > 2147483647ll || (int64_t)kSampleRows * (O > A ? O : A) > 2147483647ll) return hipErrorInvalidValue;
    return launch_kernel(replay_sample_kernel, dim3((unsigned)blocks), dim3(kSampleBlock), 0, stream, nullptr, nullptr,
                         ring, out, key, n, (uint64_t)T * (uint64_t)E, (uint64_t)E, O, A, batch);
}

// q_net_kernel's dynamic-LDS limit, raised once as ppo_net_kernels_init raises value_net_kernel's: the same tiles.
hipError_t critic_kernels_init() {
    static const hipError_t set =
        raise_lds_limit((int)kNetMaxLds, q_net_kernel<false, false>, q_net_kernel<false, true>,
                        q_net_kernel<true, false>, q_net_kernel<true, true>);
    return set;
}

hipError_t launch_q_net(const float *img, const NetImage &m, int O, const float *obs, const float *actions,
                        const float *reward, const float *done, float g, float *out, int64_t rows, hipStream_t stream) {
    const size_t lds = net_lds_bytes(m);
    const bool target = reward != nullptr;
    // what critic_spec_check and the entry points refuse
    if (rows < 1 || O < 1 || O >= m.O || lds > kNetMaxLds || m.N3 != kNetTile || critic_blocks(rows) > kCriticMaxBlocks ||
        !img || !obs || !actions || !out || (target && !done))
        return hipErrorInvalidValue;
    if (lds > 64u * 1024u && critic_kernels_init() != hipSuccess) return critic_kernels_init();
    const dim3 grid((unsigned)critic_blocks(rows)), block(kNetBlock);
    auto kern = m.activation == POLICY_RELU ? (target ? q_net_kernel<false, true> : q_net_kernel<false, false>)
                                            : (target ? q_net_kernel<true, true> : q_net_kernel<true, false>);
    return launch_kernel(kern, grid, block, lds, stream, nullptr, nullptr, img, m, obs, actions, O, reward, done, g, out,
                         rows);
}

// x = [obs | actions] over `rows` rows (learn_concat_kernel)
hipError_t launch_learn_concat(const float *obs, const float *actions, float *x, int64_t rows, int O, int A,
                               hipStream_t stream) {
    if (rows < 1 || rows > kLearnMaxRows || O < 1 || A < 1 || !obs || !actions || !x) return hipErrorInvalidValue;
    const int64_t n = rows * ((int64_t)O + A);
    int64_t blocks = (n + kLearnBlock - 1) / kLearnBlock;
    blocks = blocks > (1 << 16) ? (1 << 16) : blocks;
    return launch_kernel(learn_concat_kernel, dim3((unsigned)blocks), dim3(kLearnBlock), 0, stream, nullptr, nullptr, obs,
                         actions, x, rows, O, A);
}

// One product of an update (learn_gemm_kernel): grid x over C's column tiles, y over groups of four row tiles, z over
// the segments of the reduction.
hipError_t launch_learn_gemm(const LearnGemm &g, int epilogue, hipStream_t stream) {
    if (g.M < 1 || g.N < 1 || g.K < 1 || g.S < 1 || !g.a || !g.b || !g.c) return hipErrorInvalidValue;
    if ((epilogue == LEARN_EPI_MASK || epilogue == LEARN_EPI_DTANH) && !g.aux) return hipErrorInvalidValue;
    if (epilogue == LEARN_EPI_TANH && !g.c2) return hipErrorInvalidValue;
    const int per = kNetTile * (kLearnBlock / kWave);
    const int64_t segs = ((int64_t)g.K + g.S - 1) / g.S;
    const dim3 grid((unsigned)((g.N + kNetTile - 1) / kNetTile), (unsigned)((g.M + per - 1) / per), (unsigned)segs);
    if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
    const dim3 block(kLearnBlock);
    hipError_t e = hipErrorInvalidValue;   // no such epilogue
    with_size<LEARN_EPI_NONE, LEARN_EPI_RELU, LEARN_EPI_MASK, LEARN_EPI_TANH, LEARN_EPI_DTANH>(epilogue, [&](auto epi) {
        e = launch_kernel(learn_gemm_kernel<decltype(epi)::value>, grid, block, 0, stream, nullptr, nullptr, g);
    });
    return e;
}

// dq [rows] and the loss (learn_loss_kernel); y is the critic's, null with `actor`
hipError_t launch_learn_loss(bool actor, const float *q, const float *y, float *dq, float *loss, int64_t rows,
                             hipStream_t stream) {
    if (rows < 1 || rows > kLearnMaxRows || !q || (!actor && !y) || !dq || !loss) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((rows + kLearnBlock - 1) / kLearnBlock + 1)), block(kLearnBlock);
    return actor ? launch_kernel(learn_loss_kernel<true>, grid, block, 0, stream, nullptr, nullptr, q, y, dq, loss, rows)
                 : launch_kernel(learn_loss_kernel<false>, grid, block, 0, stream, nullptr, nullptr, q, y, dq, loss, rows);
}

// A net's Adam step, polyak blend and repack (learn_step_kernel), or with adam = false the repack alone
hipError_t launch_learn_step(const LearnStep &s, bool adam, hipStream_t stream) {
    if (s.total < 1 || s.nseg < 1 || !s.img || !s.img_target) return hipErrorInvalidValue;
    uint64_t blocks = (s.total + kLearnBlock - 1) / kLearnBlock;
    blocks = blocks > (1u << 16) ? (1u << 16) : blocks;
    const dim3 grid((unsigned)blocks), block(kLearnBlock);
    return adam ? launch_kernel(learn_step_kernel<true>, grid, block, 0, stream, nullptr, nullptr, s)
                : launch_kernel(learn_step_kernel<false>, grid, block, 0, stream, nullptr, nullptr, s);
}

hipError_t launch_profiles(const Params &p, const DeviceState &s, int64_t E, hipStream_t stream) {
    if (!p.noise) return hipSuccess;
    const dim3 grid((unsigned)((E + 255) / 256)), block(256);
    hipLaunchKernelGGL(profile_kernel, grid, block, 0, stream, p, s, E);
    return hipGetLastError();
}

}  // namespace sng
