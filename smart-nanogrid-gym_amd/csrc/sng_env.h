// sng_env.h -- the handle behind the C ABI (include/sng.h) and what the library's host translation units
// share around it: sng_api.cpp (create, resets, steps, accessors), sng_state.cpp (checkpoints) and
// sng_graph.cpp (day graphs, timed days, the bandwidth probe).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "sng.h"
#include "sng_device_scope.h"
#include "sng_host_tables.h"
#include "sng_launch.h"
#include "sng_layout.h"
#include "sng_state_format.h"

// The second day slot of an overlapped reset graph (sng_graph.cpp; sng_graph_form.h reset_overlapped): buffers of
// its own for everything the device generator writes for a day -- the packed record timeline (`aux`, sized for a
// packed day), the SoC seed the steps then run on, the PV ratio, the t = 0 penalty, the profile keys (where
// Params::noise) and the requested-SoC plane (where enabled) -- and a day-return row [E] for graphs created
// without day_returns.  Everything else of a DeviceState (bess, bess0, flags, the day counter, the tables) is
// shared with the handle's own.  Allocated by the first graph that needs it, freed with the handle; never
// exported, checkpointed or loaded: a graph's last day is always in the handle's own buffers.
struct DaySlot {
    double *soc = nullptr, *ratio = nullptr, *pen0 = nullptr, *aux = nullptr, *req = nullptr;
    uint32_t *prof_key = nullptr;
    double *day_return = nullptr;
};

struct SngEnv {
    SngConfig cfg{};
    sng::Params p{};
    sng::HostTables tables;
    sng::Tables host_tab{};           // what d_tables holds
    uint64_t cfg_hash = 0;            // configuration fingerprint (scalars + tables), checked by sng_set_state
    std::vector<double> irradiance;   // owned copy
    int device = 0;
    int64_t E = 0;
    uint64_t seed = 0;
    int t = -1;                       // -1: never reset; T: day finished
    bool day_finished = false;        // the reference's end-of-day Python draw (:181) is still owed
    sng::DaySpans spans{0, 0, 0, sng::kSlots};   // 4 h, 10 h, 1 h in steps; per-charger array length of scenarios
    // the day reset(generate_new_initial_values=False) replays: the last day sng_reset generated
    // (the reference's initial_values.json, charging_station.py:185-186 / :119-136)
    int gen_mode = -1;                // -1: none yet; else the SngRngMode that generated it
    bool gen_loaded = false;          // its timeline is still the loaded one (no injected day since)
    uint64_t replays = 0;             // device-RNG replays so far: the replay ratio stream's counter
    sng::DeviceState ds{};
    DaySlot shadow{};                 // ensure_shadow
    sng::Tables *d_tables = nullptr;
    // host staging (pinned) for days built on the CPU
    uint32_t *h_word = nullptr;
    double *h_aux = nullptr, *h_req = nullptr, *h_ratio = nullptr, *h_pen0 = nullptr;
    hipEvent_t staging_done = nullptr;
    // reference RNG streams of every env (allocated on first use), both on the device: numpy's (rs, drawn by
    // ref_day2_kernel) and Python's (ps below: two or three draws a day, seeded on host threads)
    sng::RefStreams rs{};
    bool np_seeded = false;
    // the next day's stream blocks are prepared (mt_prepare_kernel) on a side stream while a day is stepped;
    // every access to rs on a caller's stream first waits for prep_done
    hipStream_t prep_stream = nullptr;
    hipEvent_t prep_done = nullptr, day_drawn = nullptr;
    bool prep_launched = false;   // prep_done marks a prepare launched on prep_stream

    bool prepared = false;        // the next day's blocks are (being) prepared: no inline prepare
    sng::RefStreams ps{};             // Python's `random` stream of every env, on the device (py_ratio_lane in observe0_kernel)
    bool py_seeded = false;
    // sng_step_host's I/O block: the step kernel reads its actions from and writes its outputs to host memory
    // (mapped, coherent), so a host-driven step is one dispatch and one wait.  A/B (profiles/r06_single_env.log,
    // SmartNanogridEnv.step at N = 10): 21.7 us per call against 25.4 us staged through a device block with a
    // copy each way, and 34.2 us for round 5's torch copies; tools/io_latency.hip: 13.0 / 17.2 us in C
    char *hio = nullptr, *hio_dev = nullptr;
    size_t hio_bytes = 0;
    std::string err;

    size_t timeline() const { return (size_t)p.T * p.n * (size_t)E; }
};

// A device image with its pinned host mirror and the event of its last upload: what a handle keeps whose parameters
// are packed on the host and uploaded on a caller's stream (SngPolicy, SngPpo, SngNoise).
struct UploadedImage {
    float *d = nullptr, *h = nullptr;
    size_t bytes = 0;
    hipEvent_t uploaded = nullptr;   // the last upload has read h

    hipError_t create(size_t n) {
        bytes = n;
        hipError_t e = hipMalloc((void **)&d, n);
        if (e == hipSuccess) e = hipHostMalloc((void **)&h, n, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&uploaded, hipEventDisableTiming);
        return e;
    }
    // pack(h) fills the mirror once the upload before this one has read it; then the copy and its event on `st`
    template <class Pack>
    hipError_t upload(hipStream_t st, Pack pack) {
        hipError_t e = hipEventSynchronize(uploaded);
        if (e != hipSuccess) return e;
        pack(h);
        e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st);
        return e != hipSuccess ? e : hipEventRecord(uploaded, st);
    }
    // a new handle's first image: uploaded, and on the device when this returns
    template <class Pack>
    hipError_t upload_now(Pack pack) {
        const hipError_t e = upload(nullptr, pack);
        return e != hipSuccess ? e : hipEventSynchronize(uploaded);
    }
    void destroy() {
        if (uploaded) {
            (void)hipEventSynchronize(uploaded);
            (void)hipEventDestroy(uploaded);
        }
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        d = h = nullptr;
        uploaded = nullptr;
    }
};

// An MLP actor of a handle's envs (sng_policy.cpp): the device image the policy kernels and the graphs captured with
// it read, which sng_policy_set_weights packs and uploads, and the clipped actions a captured step node reads.  It has
// one of two forms: sng_policy_create's 64-64 actor (spec, image: sng_policy_host.h) or, with `net`,
// sng_policy_create_net's actor of any width (net_spec, net_image: sng_policy_net_host.h).  What depends on the form
// is decided in policy_weights_ok, policy_pack_image, launch_actor and policy_kind below, and nowhere else.
struct SngPolicy {
    SngEnv *env = nullptr;
    bool net = false;
    int O = 0, A = 0, H1 = 0, H2 = 0;   // the dims, whichever the form
    size_t floats = 0;                  // of the image
    SngMlpSpec spec{};
    sng::PolicyImage image{};
    SngMlpNetSpec net_spec{};
    sng::NetImage net_image{};
    std::vector<float> clip_low, clip_high;   // owned copies behind the spec's bounds
    UploadedImage img;
    float *d_env_actions = nullptr;           // [E][act_dim]
};

// A critic of a handle's envs (sng_ddpg.cpp): its spec, the NetImage of (obs_dim + act_dim, 1, hidden1, hidden2) and
// the device image q_net_kernel reads, which sng_critic_set_weights packs and uploads and a learner
// (sng_ddpg_learn.cpp) rewrites on the device.
struct SngCritic {
    SngEnv *env = nullptr;
    SngCriticSpec spec{};
    sng::NetImage image{};
    UploadedImage img;
};

// An action-noise source of a handle's envs (sng_noise.cpp): the spec, the per-action parameters' device image
// (sng_noise_host.h, noise_pack_params: mu [A], sd [A]), and the counter of the next block, on the device, which only
// the kernel behind a fill advances.
struct SngNoise {
    SngEnv *env = nullptr;
    SngNoiseSpec spec{};
    UploadedImage params;
    uint64_t *d_counter = nullptr;
};

struct SngGraph {
    SngEnv *env = nullptr;
    bool with_reset = false;
    // from the graph's form (sng_graph_form.h graph_form)
    int nodes_per_day = 0;     // the nodes that step a day (sng_graph_step_nodes): 1, T or 2 T
    std::string day_kernel_name;   // a day-kernel node's kernel as rocprofv3 names it (not a policy graph's); else empty
    bool overlapped = false;   // day d + 1 is generated beside day d's steps (reset_overlapped)
    sng::DayKey key{};   // the loaded-day encoding the graph's steps were captured for
    // the stream keys baked into the captured kernels' arguments: the device days a reset graph draws
    // and the PV-ratio / profile streams are those of this seed and env offset
    uint64_t seed = 0;
    int64_t env_offset = 0;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

// Shared by the library's translation units, not exported by it.
#pragma GCC visibility push(hidden)
namespace sng {

// The error text of a call without a handle (sng_create, the bandwidth probe), per thread; defined in sng_api.cpp.
extern thread_local std::string g_create_error;

inline int fail(SngEnv *env, int code, const std::string &msg) {
    if (env) env->err = msg; else g_create_error = msg;
    return code;
}

// The device generator keeps the day's vehicles of a charger plus an end sentinel in 8 LDS slots
// (sng_kernels.hip, kDayVehicles): a vehicle stays >= 4/dt steps and leaves one step empty, so a
// day has at most T / (4/dt + 1) + 1 vehicles, which must leave the sentinel's slot free.
inline bool device_rng_ok(const SngEnv *env) { return env->spans.i4 >= 2 && env->p.T / (env->spans.i4 + 1) + 1 <= 7; }

inline int hip_fail(SngEnv *env, hipError_t e, const char *what) {
    return fail(env, SNG_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// a handle's buffers could not be made: "<what> buffers" where the memory ran out, else HIP's own text
inline int create_fail(SngEnv *env, hipError_t e, const std::string &what) {
    return e == hipErrorOutOfMemory ? fail(env, SNG_ERR_OUT_OF_MEMORY, what + " buffers")
                                    : hip_fail(env, e, (what + " create").c_str());
}

#define HIP_TRY(env, expr)                                   \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return hip_fail(env, _e, #expr); \
    } while (0)
// ... and of a helper that returns an SNG_* code and has set the handle's error itself
#define SNG_TRY(expr)                     \
    do {                                  \
        if (int _rc = (expr)) return _rc; \
    } while (0)

// An entry point's prologue, after its argument checks: the rest of the call runs on the handle's device (DeviceScope).
// A declaration and a statement that may return: once per function, at block scope, never under a brace-less `if`.
#define ON_DEVICE_OF(env)               \
    DeviceScope dev_((env)->device);    \
    HIP_TRY(env, dev_.err)

// --- the loaded day (DayKey, t, day_finished, gen_mode, gen_loaded) ---
inline void load_day(SngEnv *env, const DayKey &k) { env->p = with_day(env->p, k); }
// a day begins: its t = 0 observation is queued
inline void begin_day(SngEnv *env) {
    env->t = 0;
    env->day_finished = false;
}
// a generated day is now the one reset(generate_new_initial_values=False) replays
inline void generated_day_loaded(SngEnv *env, int rng_mode) {
    env->gen_mode = rng_mode;
    env->gen_loaded = true;
}
// whole days ran (a day graph, the timed days): the last one is over
inline void days_ran(SngEnv *env) {
    env->t = env->p.T;
    env->day_finished = true;
}
// A device day is counted by its first step (step_kernel advances the day counter); one that was reset but
// never stepped is counted here, before what follows it, so the next device day drawn is a new one.
inline hipError_t count_unstepped_device_day(SngEnv *env, hipStream_t st) {
    return DayKey::of(env->p).unstepped_device_day(env->t) ? launch_bump_day(env->ds, st) : hipSuccess;
}

inline InfoPtrs info_ptrs(const SngInfo *i) {
    InfoPtrs o{};
    if (!i) return o;
    o.grid_power = i->grid_power;
    o.p_charge = i->total_charging_power;
    o.p_discharge = i->total_discharging_power;
    o.bess_soc = i->battery_state_of_charge;
    o.pen_vehicle = i->total_vehicle_penalty;
    o.pen_battery = i->total_battery_penalty;
    o.grid_cost = i->grid_energy_cost;
    o.total_cost = i->total_cost;
    o.solar = i->utilized_solar_energy;
    o.bess_power = i->battery_power_value;
    o.bess_calc_power = i->battery_calculated_power;
    o.nonexistent = i->nonexistent_vehicle_penalty;
    o.bess_initial = i->initial_battery_soc;
    o.flags = i->flags;
    o.episode_return = i->episode_return;
    o.charger_power = i->charger_power;
    o.vehicle_soc = i->vehicle_soc;
    o.flag_any = i->flag_summary;
    return o;
}

// --- what depends on a policy's form ---
inline int policy_weights_ok(const SngPolicy *pol, const SngMlpWeights *w, std::string *why) {
    return pol->net ? net_weights_check(pol->net_spec, w, why) : policy_weights_check(pol->spec, w, why);
}
inline void policy_pack_image(const SngPolicy *pol, const SngMlpWeights &w, float *img) {
    if (pol->net) net_pack(pol->net_image, pol->net_spec, w, img);
    else policy_pack(pol->image, pol->spec, w, img);
}
// One actor launch over the env's rows, by the policy's own kernel.
inline hipError_t launch_actor(const SngPolicy *pol, const float *obs, const float *noise, float *actions,
                               float *env_actions, int64_t E, hipStream_t stream) {
    return pol->net ? launch_policy_net(pol->img.d, pol->net_image, obs, noise, actions, env_actions, E, stream)
                    : launch_policy(pol->img.d, pol->image, obs, noise, actions, env_actions, E, stream);
}
// What graph_form (sng_graph_form.h) asks about a graph's policy; null: the caller's actions.
inline PolicyKind policy_kind(const SngPolicy *pol) { return !pol ? POLICY_NONE : pol->net ? POLICY_NET : POLICY_MLP; }

inline hipStream_t as_stream(void *s) { return (hipStream_t)s; }

// Defined in sng_api.cpp, called from sng_state.cpp and sng_graph.cpp too.
// the requested-SoC plane, on first use
int ensure_req(SngEnv *env);
// the second day slot, on first use; `out`: the handle's DeviceState with the slot's buffers in place of its own
int ensure_shadow(SngEnv *env, DeviceState *out);
// Orders `st` after the side stream's preparation of the streams (sng_reset), before st touches them.
int await_prepare(SngEnv *env, hipStream_t st);
// one stream set's device blocks ([E][2][624] words and the positions), on first use
int alloc_streams(SngEnv *env, RefStreams &r);
// numpy's streams of every env, seeded on the device (mt_seed_kernel) if they are not yet, queued on `st`
int ensure_np_streams(SngEnv *env, hipStream_t st);

}  // namespace sng
#pragma GCC visibility pop
