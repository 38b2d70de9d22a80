// sng_graph.cpp -- whole days in one call: days captured into a hipGraph (sng_graph_create / launch / destroy),
// days timed kernel by kernel (sng_time_step_kernels), and the bandwidth probe bench.py's memory floor uses.
#include <algorithm>

#include "sng_env.h"

using namespace sng;

// sng_graph_create and sng_graph_create_policy.  Without a policy, `actions` holds the day's T action blocks.  With
// one (sng_policy.cpp), every step's actions are the actor's answer to the observation before it: `noise` (T
// blocks, may be null) takes the place of the actions stream, `actions_out` receives a, and the step nodes read the
// policy's clipped actions.
// With a noise source (sng_graph_create_policy_noise), `noise` is the [days][T][E][A] buffer the graph's first node fills
// and day d's actor reads block d of; without one it is the caller's one block, read every day.
static int capture_days(SngEnv *env, SngPolicy *policy, const float *actions, const float *noise, float *actions_out,
                        float *obs, double *reward, uint8_t *done, const SngInfo *info, int flags, int32_t days,
                        double *day_returns, SngGraph **out, SngNoise *noise_source = nullptr) {
    const bool with_reset = (flags & SNG_GRAPH_RESET) != 0;
    if (policy) actions = policy->d_env_actions;
    if (!env || !actions || !obs || !reward || !done || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    if (days < 1 || (days > 1 && !with_reset))
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "days must be >= 1 (more than one needs SNG_GRAPH_RESET)");
    if (with_reset && !device_rng_ok(env))
        return fail(env, SNG_ERR_UNSUPPORTED, "device RNG needs time_interval <= 2h");
    ON_DEVICE_OF(env);
    if (env->p.req_enabled) SNG_TRY(ensure_req(env));
    hipStream_t cs;
    HIP_TRY(env, hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    SngGraph *g = new SngGraph();
    g->env = env;
    g->policy = policy;
    // with a reset: every day a freshly generated device day (sng_reset(SNG_RNG_DEVICE)); else the loaded day
    g->with_reset = with_reset;
    g->key = with_reset ? DayKey::device_day(env->p) : DayKey::of(env->p);
    const Params p = with_day(env->p, g->key);
    g->seed = env->seed;
    g->env_offset = p.env_offset;
    const InfoPtrs ip = info_ptrs(info);
    const DaySpans &sp = env->spans;
    const int64_t E = env->E;
    const int A = p.act_dim;
    const int vec = (aligned16(actions) && aligned16(obs)) ? 1 : 0;
    // SNG_GRAPH_TRAJECTORY: every step of every day keeps its outputs -- obs [days][T + 1][E][obs_dim] (block 0 of a
    // day is the reset's observation), reward and done [days][T][E]; else every step overwrites one block
    const bool traj = (flags & SNG_GRAPH_TRAJECTORY) != 0;
    const size_t obs_block = (size_t)E * (size_t)p.obs_dim;
    const int64_t obs_step = traj ? (int64_t)obs_block : 0, out_step = traj ? E : 0;
    // a day's T steps as one day-kernel node where the plan has one (sng_step_plan.h day_kernel_of), else -- or
    // with SNG_GRAPH_STEP_NODES -- as T dependent step nodes
    // with a policy: one fused node where the plan has that form (sng_step_plan.h policy_day_form), else T x (policy
    // node, step node)
    // (a net policy's days are always nodes: policy_net_day_form)
    g->day_kernel = policy ? policy_graph_fused(policy, p, ip, traj, (flags & SNG_GRAPH_STEP_NODES) != 0,
                                                (flags & SNG_GRAPH_POLICY_FUSED) != 0)
                           : !(flags & SNG_GRAPH_STEP_NODES) && day_kernel_available(p, ip, traj) != 0;
    // the wide plan's day kernel: the station-fixed one where the plan selects it (sng_step_plan.h
    // day_station_selected), unless SNG_GRAPH_GENERIC_DAY keeps the generic one
    const bool generic_day = (flags & SNG_GRAPH_GENERIC_DAY) != 0;
    if (g->day_kernel && !policy) {
        char name[128];
        if (day_kernel_name(p, ip, traj, generic_day, name, (int)sizeof name) > 0) g->day_kernel_name = name;
    }
    // Overlapped (sng_step_plan.h reset_overlapped, day_shape): the generators are captured on a second stream, day
    // d + 1's into the day slot that day d does not use, so it runs beside day d's steps.  The edges are gen(d) ->
    // day(d), day(d - 1) -> day(d) and day(d - 1) -> gen(d + 1) (the slot is free again); the generators follow
    // one another on their stream, and the node that advances the day counter for all days but the last follows
    // the last of them, when no generator reads the counter any more.
    // Both kernels become ready at the same join, and a generator that fills the CUs first delays the day's steps by
    // more than it hides: its workgroups ask for generator_lds of dynamic LDS so that fewer of them fit a CU.
    size_t generator_lds = 0;
    g->overlapped = !policy && with_reset && reset_graph_overlapped(p, ip, days, traj, (flags & SNG_GRAPH_SERIAL_RESET) != 0,
                                                         (flags & SNG_GRAPH_OVERLAPPED_RESET) != 0, &generator_lds,
                                                         g->day_kernel && !policy, generic_day) != 0;
    DeviceState slots[2] = {env->ds, env->ds};
    hipStream_t gs = nullptr;                      // the generators' stream
    std::vector<hipEvent_t> generated, stepped;   // day d's generator / steps are captured
    hipError_t e = hipSuccess;
    if (g->overlapped) {
        if (int rc = ensure_shadow(env, &slots[1])) {
            (void)hipStreamDestroy(cs);
            delete g;
            return rc;
        }
        generated.assign((size_t)days, nullptr);
        stepped.assign((size_t)days, nullptr);
        e = hipStreamCreateWithFlags(&gs, hipStreamNonBlocking);
        for (int d = 0; d < days; ++d) {
            if (e == hipSuccess) e = hipEventCreateWithFlags(&generated[(size_t)d], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&stepped[(size_t)d], hipEventDisableTiming);
        }
    }
    auto row = [&](int d, const DayShape &sh) {   // day d's returns (the generator zeroes the row, every step adds)
        InfoPtrs ipd = ip;
        if (day_returns) ipd.episode_return = day_returns + (size_t)d * E;   // into row d
        else if (sh.slot && ip.episode_return) ipd.episode_return = env->shadow.day_return;
        return ipd;
    };
    // an overlapped graph's generator of day d, on `gs`
    auto capture_generator = [&](int d) {
        const DayShape sh = day_shape(true, days, d);
        if (d >= 2) e = hipStreamWaitEvent(gs, stepped[(size_t)d - 2], 0);
        if (e == hipSuccess)
            e = launch_generate(p, slots[sh.slot], env->seed, E, sp.i4, sp.i10, sp.i1, nullptr, row(d, sh).episode_return,
                                0, gs, nullptr, nullptr, sh.day_delta, generator_lds);
        if (e == hipSuccess) e = hipEventRecord(generated[(size_t)d], gs);
        if (e == hipSuccess && sh.bump_node) e = launch_bump_day(env->ds, gs, (uint64_t)sh.bump_node);
    };
    if (e == hipSuccess) e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    const bool capturing = e == hipSuccess;
    // a source's fill of every day's block and its counter's bump: the chain's first nodes
    const size_t noise_day = noise_source ? (size_t)p.T * (size_t)E * (size_t)A : 0;
    if (noise_source && e == hipSuccess)
        e = launch_noise_fill(noise_source->spec, noise_source->params.d, noise_source->d_counter, p.env_offset,
                              const_cast<float *>(noise), days, p.T, E, cs);
    if (g->overlapped && e == hipSuccess) {   // fork
        e = hipEventRecord(stepped[0], cs);
        if (e == hipSuccess) e = hipStreamWaitEvent(gs, stepped[0], 0);
        if (e == hipSuccess) capture_generator(0);
    }
    for (int d = 0; e == hipSuccess && d < days; ++d) {
        const DayShape sh = day_shape(g->overlapped, days, d);
        const InfoPtrs ipd = row(d, sh);
        const DeviceState &ds = slots[sh.slot];
        Params pd = p;
        if (g->overlapped) pd.bump_day = sh.bump_day;
        // day d's blocks: the reset's observation, then step 0's outputs
        float *obs0 = obs + (traj ? (size_t)d * (size_t)(p.T + 1) * obs_block : 0);
        float *obs_d = obs0 + obs_step;
        double *reward_d = reward + (traj ? (size_t)d * (size_t)p.T * (size_t)E : 0);
        uint8_t *done_d = done + (traj ? (size_t)d * (size_t)p.T * (size_t)E : 0);
        if (g->overlapped) {
            e = hipStreamWaitEvent(cs, generated[(size_t)d], 0);
        } else if (with_reset) {
            e = launch_generate(p, ds, env->seed, E, sp.i4, sp.i10, sp.i1, obs0, ipd.episode_return,
                                (vec && aligned16(obs0)) ? 1 : 0, cs);
        }
        if (policy) {
            // step t answers the observation in block t of the day (the reset's, then step t - 1's)
            const size_t act_block = (size_t)E * (size_t)A;
            float *a_d = actions_out + (traj ? (size_t)d * (size_t)p.T * act_block : 0);
            const float *noise_d = noise ? noise + (size_t)d * noise_day : nullptr;
            if (e == hipSuccess && g->day_kernel)
                e = launch_policy_day(pd, ds, ipd, policy->img.d, policy->image, noise_d, obs0, obs_d, a_d, reward_d, done_d,
                                      E, (vec && aligned16(obs_d)) ? 1 : 0, cs, obs_step, out_step,
                                      traj ? (int64_t)act_block : 0);
            for (int t = 0; e == hipSuccess && !g->day_kernel && t < p.T; ++t) {
                float *obs_t = obs_d + (size_t)t * (size_t)obs_step;
                e = launch_actor(policy, obs0 + (size_t)t * (size_t)obs_step,
                                 noise_d ? noise_d + (size_t)t * act_block : nullptr, a_d + (traj ? (size_t)t * act_block : 0),
                                 policy->d_env_actions, E, cs);
                if (e == hipSuccess)
                    e = launch_step(pd, ds, ipd, env->host_tab, policy->d_env_actions, obs_t,
                                    reward_d + (size_t)t * (size_t)out_step, done_d + (size_t)t * (size_t)out_step, E, t,
                                    (vec && aligned16(obs_t)) ? 1 : 0, cs);
            }
        } else if (g->day_kernel) {
            if (e == hipSuccess)
                e = launch_day(pd, ds, ipd, actions, obs_d, reward_d, done_d, E, 0, p.T,
                               (vec && aligned16(obs_d)) ? 1 : 0, cs, obs_step, out_step, generic_day);
        } else {
            for (int t = 0; e == hipSuccess && t < p.T; ++t) {
                float *obs_t = obs_d + (size_t)t * (size_t)obs_step;
                e = launch_step(pd, ds, ipd, env->host_tab, actions + (size_t)t * E * A, obs_t,
                                reward_d + (size_t)t * (size_t)out_step, done_d + (size_t)t * (size_t)out_step, E, t,
                                (vec && aligned16(obs_t)) ? 1 : 0, cs);
            }
        }
        if (g->overlapped) {
            if (e == hipSuccess) e = hipEventRecord(stepped[(size_t)d], cs);
            // behind day d's steps in capture order (ahead of them measured the same, profiles/overlapped_reset_ab.txt)
            if (e == hipSuccess && d + 1 < days) capture_generator(d + 1);
        }
    }
    if (g->overlapped && capturing) {   // join: the bump node is the generators' stream's last
        hipError_t ej = hipEventRecord(generated[0], gs);
        if (ej == hipSuccess) ej = hipStreamWaitEvent(cs, generated[0], 0);
        if (e == hipSuccess) e = ej;
    }
    hipGraph_t graph = nullptr;
    hipError_t e2 = capturing ? hipStreamEndCapture(cs, &graph) : hipSuccess;
    if (e == hipSuccess) e = e2;
    if (e == hipSuccess) e = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
    (void)hipStreamDestroy(cs);
    if (gs) (void)hipStreamDestroy(gs);
    for (hipEvent_t x : generated)
        if (x) (void)hipEventDestroy(x);
    for (hipEvent_t x : stepped)
        if (x) (void)hipEventDestroy(x);
    if (e != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        delete g;
        return hip_fail(env, e, "graph capture");
    }
    g->graph = graph;
    *out = g;
    return SNG_OK;
}

extern "C" {

int sng_graph_create(SngEnv *env, const float *actions, float *obs, double *reward, uint8_t *done,
                     const SngInfo *info, int flags, int32_t days, double *day_returns, SngGraph **out) {
    return capture_days(env, nullptr, actions, nullptr, nullptr, obs, reward, done, info, flags, days, day_returns, out);
}

int sng_graph_create_policy(SngEnv *env, SngPolicy *policy, const float *noise, float *obs, float *actions_out,
                            double *reward, uint8_t *done, const SngInfo *info, int flags, int32_t days,
                            double *day_returns, SngGraph **out) {
    if (!env || !policy || !actions_out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    if (policy->env != env) return fail(env, SNG_ERR_INVALID_ARGUMENT, "the policy was created for another env");
    return capture_days(env, policy, nullptr, noise, actions_out, obs, reward, done, info, flags, days, day_returns, out);
}

int sng_graph_create_policy_noise(SngEnv *env, SngPolicy *policy, SngNoise *noise_source, float *noise_out, float *obs,
                                  float *actions_out, double *reward, uint8_t *done, const SngInfo *info, int flags,
                                  int32_t days, double *day_returns, SngGraph **out) {
    if (!env || !policy || !actions_out || !noise_source || !noise_out)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    if (policy->env != env) return fail(env, SNG_ERR_INVALID_ARGUMENT, "the policy was created for another env");
    if (noise_source->env != env) return fail(env, SNG_ERR_INVALID_ARGUMENT, "the noise source was created for another env");
    return capture_days(env, policy, nullptr, noise_out, actions_out, obs, reward, done, info, flags, days, day_returns, out,
                        noise_source);
}

int sng_graph_launch(SngGraph *g, void *stream) {
    if (!g) return SNG_ERR_INVALID_ARGUMENT;
    SngEnv *env = g->env;
    if (!g->with_reset) {
        // a steps-only graph steps the loaded day from t = 0 with the Params it was captured with
        if (!(g->key == DayKey::of(env->p)))
            return fail(env, SNG_ERR_STATE,
                        "graph captured for a day of another encoding (RNG mode, requested-SoC stream or replay): "
                        "recapture it after this reset");
        if (env->t != 0) return fail(env, SNG_ERR_STATE, "a steps-only graph starts at t = 0: reset first");
    }
    // sng_set_seed / sng_set_state / sng_set_env_offset since the capture: the graph's kernels would
    // still draw the old streams
    if (g->seed != env->seed || g->env_offset != env->p.env_offset)
        return fail(env, SNG_ERR_STATE, "seed or env offset changed since the graph was captured: recapture it");
    ON_DEVICE_OF(env);
    // the graph's first reset must not redraw a device day that was reset but never stepped
    if (g->with_reset) HIP_TRY(env, count_unstepped_device_day(env, as_stream(stream)));
    HIP_TRY(env, hipGraphLaunch(g->exec, as_stream(stream)));
    if (g->with_reset) {
        load_day(env, g->key);
        generated_day_loaded(env, SNG_RNG_DEVICE);
    }
    days_ran(env);
    return SNG_OK;
}

int sng_graph_step_nodes(const SngGraph *g) {
    if (!g) return -1;
    return g->day_kernel ? 1 : g->policy ? 2 * g->env->p.T : g->env->p.T;
}

int sng_graph_day_kernel_name(const SngGraph *g, char *buf, int32_t len) {
    if (!g || !buf || len < 1) return SNG_ERR_INVALID_ARGUMENT;
    if ((size_t)len <= g->day_kernel_name.size()) return SNG_ERR_INVALID_ARGUMENT;
    snprintf(buf, (size_t)len, "%s", g->day_kernel_name.c_str());
    return SNG_OK;
}

int sng_graph_reset_overlapped(const SngGraph *g) {
    if (!g) return -1;
    return g->overlapped ? 1 : 0;
}

void sng_graph_destroy(SngGraph *g) {
    if (!g) return;
    DeviceScope scope(g->env->device);
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
}

int sng_time_step_kernels(SngEnv *env, const float *actions, float *obs, double *reward, uint8_t *done,
                          const SngInfo *info, int32_t days, float *ms, float *reset_ms, void *stream) {
    if (!env || !actions || !obs || !reward || !done || days < 1)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    if (!device_rng_ok(env)) return fail(env, SNG_ERR_UNSUPPORTED, "device RNG needs time_interval <= 2h");
    ON_DEVICE_OF(env);
    hipStream_t st = as_stream(stream);
    const DayKey key = DayKey::device_day(env->p);
    const Params p = with_day(env->p, key);
    if (p.req_stream) SNG_TRY(ensure_req(env));
    const InfoPtrs ip = info_ptrs(info);
    const DaySpans &sp = env->spans;
    const int64_t E = env->E;
    const int T = p.T, A = p.act_dim;
    const int vec = (aligned16(actions) && aligned16(obs)) ? 1 : 0;
    std::vector<hipEvent_t> ev(ms ? 2 * (size_t)T * days : 0, nullptr), rev(reset_ms ? 2 * (size_t)days : 0, nullptr);
    hipError_t e = count_unstepped_device_day(env, st);   // as in sng_reset
    for (auto &x : ev)
        if (e == hipSuccess) e = hipEventCreate(&x);
    for (auto &x : rev)
        if (e == hipSuccess) e = hipEventCreate(&x);
    for (int d = 0; e == hipSuccess && d < days; ++d) {
        e = launch_generate(p, env->ds, env->seed, E, sp.i4, sp.i10, sp.i1, obs, ip.episode_return, vec, st,
                            reset_ms ? rev[2 * (size_t)d] : nullptr, reset_ms ? rev[2 * (size_t)d + 1] : nullptr);
        for (int t = 0; e == hipSuccess && t < T; ++t) {
            hipEvent_t a = ms ? ev[2 * ((size_t)d * T + t)] : nullptr, b = ms ? ev[2 * ((size_t)d * T + t) + 1] : nullptr;
            e = launch_step(p, env->ds, ip, env->host_tab, actions + (size_t)t * E * A, obs, reward, done, E, t, vec, st, a, b);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    for (int k = 0; e == hipSuccess && ms && k < T * days; ++k) e = hipEventElapsedTime(&ms[k], ev[2 * k], ev[2 * k + 1]);
    for (int d = 0; e == hipSuccess && reset_ms && d < days; ++d)
        e = hipEventElapsedTime(&reset_ms[d], rev[2 * (size_t)d], rev[2 * (size_t)d + 1]);
    for (auto x : ev)
        if (x) (void)hipEventDestroy(x);
    for (auto x : rev)
        if (x) (void)hipEventDestroy(x);
    if (e != hipSuccess) return hip_fail(env, e, "timed day");
    load_day(env, key);
    generated_day_loaded(env, SNG_RNG_DEVICE);
    days_ran(env);
    return SNG_OK;
}

int sng_bandwidth_probe(int device, int64_t read_bytes, int64_t write_bytes, int32_t reps, float *dispatch_us,
                        float *back_to_back_us, void *stream) {
    if (read_bytes < 0 || write_bytes < 0 || read_bytes + write_bytes < 16 || reps < 1)
        return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "sng_bandwidth_probe: bad sizes");
    DeviceScope scope(device);
    if (scope.err != hipSuccess) return fail(nullptr, SNG_ERR_HIP, "sng_bandwidth_probe: hipSetDevice");
    hipStream_t st = as_stream(stream);
    const int64_t nr = read_bytes / 16, nw = write_bytes / 16;
    void *in = nullptr, *out = nullptr;
    std::vector<hipEvent_t> ev(2 * (size_t)reps + 2, nullptr);
    hipError_t e = hipMalloc(&in, (size_t)std::max<int64_t>(nr, 1) * 16);
    if (e == hipSuccess) e = hipMalloc(&out, (size_t)std::max<int64_t>(nw, 1) * 16);
    if (e == hipSuccess) e = hipMemsetAsync(in, 0, (size_t)std::max<int64_t>(nr, 1) * 16, st);
    for (auto &x : ev)
        if (e == hipSuccess) e = hipEventCreate(&x);
    // warm-up, then `reps` dispatches each between its own start/stop events (the dispatch's device time),
    // then `reps` back to back between two events (start to start, as a graph runs kernels)
    for (int k = 0; e == hipSuccess && k < 3; ++k) e = launch_probe_copy(in, out, nr, nw, st, nullptr, nullptr);
    for (int k = 0; e == hipSuccess && k < reps; ++k)
        e = launch_probe_copy(in, out, nr, nw, st, ev[2 * (size_t)k], ev[2 * (size_t)k + 1]);
    if (e == hipSuccess) e = hipEventRecord(ev[2 * (size_t)reps], st);
    for (int k = 0; e == hipSuccess && k < reps; ++k) e = launch_probe_copy(in, out, nr, nw, st, nullptr, nullptr);
    if (e == hipSuccess) e = hipEventRecord(ev[2 * (size_t)reps + 1], st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    float sum = 0.f, ms = 0.f;
    for (int k = 0; e == hipSuccess && k < reps; ++k) {
        e = hipEventElapsedTime(&ms, ev[2 * (size_t)k], ev[2 * (size_t)k + 1]);
        sum += ms;
    }
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[2 * (size_t)reps], ev[2 * (size_t)reps + 1]);
    for (auto x : ev)
        if (x) (void)hipEventDestroy(x);
    if (in) (void)hipFree(in);
    if (out) (void)hipFree(out);
    if (e != hipSuccess) return fail(nullptr, SNG_ERR_HIP, std::string("sng_bandwidth_probe: ") + hipGetErrorString(e));
    if (dispatch_us) *dispatch_us = sum / reps * 1e3f;
    if (back_to_back_us) *back_to_back_us = ms / reps * 1e3f;
    return SNG_OK;
}

}  // extern "C"
