// sng_graph.cpp -- whole days in one call: days captured into a hipGraph (sng_graph_create / launch / destroy),
// days timed kernel by kernel (sng_time_step_kernels), and the bandwidth probe bench.py's memory floor uses.
#include <algorithm>

#include "sng_env.h"

using namespace sng;

namespace {

// Events created with one set of flags, destroyed with the list.
struct EventList {
    std::vector<hipEvent_t> ev;
    EventList() = default;
    EventList(const EventList &) = delete;
    ~EventList() {
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
    }
    hipError_t create(size_t n, unsigned flags) {
        ev.assign(n, nullptr);
        hipError_t e = hipSuccess;
        for (auto &x : ev)
            if (e == hipSuccess) e = hipEventCreateWithFlags(&x, flags);
        return e;
    }
    hipEvent_t operator[](size_t i) const { return ev[i]; }
};

// What sng_graph_create, sng_graph_create_policy and sng_graph_create_policy_noise capture: first what all three take,
// in sng_graph_create's order, then what only some do.  Without a policy, `actions` holds the day's T action blocks.
// With one (sng_policy.cpp), every step's actions are the actor's answer to the observation before it: `actions` is the
// policy's block of clipped actions, which the step nodes read, `noise` (T blocks, may be null) takes the place of the
// actions stream and `actions_out` receives a.  With a noise source, `noise` is the [days][T][E][A] buffer the graph's
// first node fills and day d's actor reads block d of; without one it is the caller's one block, read every day.
struct CaptureArgs {
    SngEnv *env;
    float *obs;
    double *reward;
    uint8_t *done;
    const SngInfo *info;
    int flags, days;
    double *day_returns;
    const float *actions = nullptr, *noise = nullptr;
    float *actions_out = nullptr;
    SngPolicy *policy = nullptr;
    SngNoise *noise_source = nullptr;
};

// A capture in progress.  `cs` is the capturing stream.  Overlapped (sng_graph_form.h reset_overlapped, day_shape): the
// generators are captured on a second stream `gs`, day d + 1's into the day slot that day d does not use, so it runs
// beside day d's steps.  The edges are gen(d) -> day(d), day(d - 1) -> day(d) and day(d - 1) -> gen(d + 1) (the slot is
// free again); the generators follow one another on their stream, and the node that advances the day counter for all
// days but the last follows the last of them, when no generator reads the counter any more.
// Both kernels become ready at the same join, and a generator that fills the CUs first delays the day's steps by more
// than it hides: its workgroups ask for form.generator_lds of dynamic LDS so that fewer of them fit a CU.
struct Capture {
    const CaptureArgs &a;
    SngEnv *env;
    GraphForm form;
    Params p;   // of the day the graph steps
    InfoPtrs ip;
    int64_t E;
    int vec;
    DeviceState slots[2];
    hipStream_t cs = nullptr, gs = nullptr;
    EventList generated, stepped;   // day d's generator / steps are captured
    hipError_t e = hipSuccess;      // the first call that failed; nothing is captured behind it

    ~Capture() {
        if (cs) (void)hipStreamDestroy(cs);
        if (gs) (void)hipStreamDestroy(gs);
    }
    // day d's returns (the generator zeroes the row, every step adds)
    InfoPtrs row(int d, const DayShape &sh) const {
        InfoPtrs ipd = ip;
        if (a.day_returns) ipd.episode_return = a.day_returns + (size_t)d * E;   // into row d
        else if (sh.slot && ip.episode_return) ipd.episode_return = env->shadow.day_return;
        return ipd;
    }
    int vec_for(const void *block) const { return (vec && aligned16(block)) ? 1 : 0; }

    // an overlapped graph's generator of day d, on `gs`
    void capture_generator(int d) {
        const DayShape sh = day_shape(true, a.days, d);
        const DaySpans &sp = env->spans;
        if (d >= 2) e = hipStreamWaitEvent(gs, stepped[(size_t)d - 2], 0);
        if (e == hipSuccess)
            e = launch_generate(p, slots[sh.slot], env->seed, E, sp.i4, sp.i10, sp.i1, nullptr, row(d, sh).episode_return,
                                0, gs, nullptr, nullptr, sh.day_delta, form.generator_lds);
        if (e == hipSuccess) e = hipEventRecord(generated[(size_t)d], gs);
        if (e == hipSuccess && sh.bump_node) e = launch_bump_day(env->ds, gs, (uint64_t)sh.bump_node);
    }
    void fork() {
        if (e == hipSuccess) e = hipEventRecord(stepped[0], cs);
        if (e == hipSuccess) e = hipStreamWaitEvent(gs, stepped[0], 0);
        if (e == hipSuccess) capture_generator(0);
    }
    // the bump node is the generators' stream's last; joined also behind a failed launch, so that the capture can end
    void join() {
        hipError_t ej = hipEventRecord(generated[0], gs);
        if (ej == hipSuccess) ej = hipStreamWaitEvent(cs, generated[0], 0);
        if (e == hipSuccess) e = ej;
    }

    // day d on `cs`: its reset (or the wait for its generator), then the nodes form.day names
    void capture_day(int d) {
        const DayShape sh = day_shape(form.overlapped, a.days, d);
        const DaySpans &sp = env->spans;
        const DeviceState &ds = slots[sh.slot];
        const InfoPtrs ipd = row(d, sh);
        Params pd = p;
        if (form.overlapped) pd.bump_day = sh.bump_day;
        // day d's blocks: the reset's observation, then step 0's outputs
        const DayBlocks b = day_blocks(form.trajectory, d, p.T, E, p.obs_dim, p.act_dim);
        const size_t act_block = (size_t)E * (size_t)p.act_dim;
        float *obs0 = a.obs + b.obs0, *obs_d = obs0 + b.obs_step, *a_d = a.policy ? a.actions_out + b.actions : nullptr;
        double *reward_d = a.reward + b.out;
        uint8_t *done_d = a.done + b.out;
        const float *noise_d = a.noise ? a.noise + (a.noise_source ? b.noise_day : 0) : nullptr;
        if (form.overlapped) {
            e = hipStreamWaitEvent(cs, generated[(size_t)d], 0);
        } else if (form.with_reset) {
            e = launch_generate(p, ds, env->seed, E, sp.i4, sp.i10, sp.i1, obs0, ipd.episode_return, vec_for(obs0), cs);
        }
        if (e != hipSuccess) return;
        switch (form.day) {
            case DAY_STEP_NODES:
            case DAY_POLICY_NODES:
                // step t, behind its actor node where a policy is in the loop, answers the observation in block t of
                // the day (the reset's, then step t - 1's)
                for (int t = 0; e == hipSuccess && t < p.T; ++t) {
                    float *obs_t = obs_d + (size_t)t * (size_t)b.obs_step;
                    if (a.policy)
                        e = launch_actor(a.policy, obs0 + (size_t)t * (size_t)b.obs_step,
                                         noise_d ? noise_d + (size_t)t * act_block : nullptr,
                                         a_d + (size_t)t * (size_t)b.act_step, a.policy->d_env_actions, E, cs);
                    if (e == hipSuccess)
                        e = launch_step(pd, ds, ipd, env->host_tab, a.policy ? a.actions : a.actions + (size_t)t * act_block,
                                        obs_t, reward_d + (size_t)t * (size_t)b.out_step,
                                        done_d + (size_t)t * (size_t)b.out_step, E, t, vec_for(obs_t), cs);
                }
                break;
            case DAY_POLICY_FUSED:
                e = launch_policy_day(pd, ds, ipd, a.policy->img.d, a.policy->image, noise_d, obs0, obs_d, a_d, reward_d,
                                      done_d, E, vec_for(obs_d), cs, b.obs_step, b.out_step, b.act_step);
                break;
            default:   // a day kernel
                e = launch_day(form.day, pd, ds, ipd, a.actions, obs_d, reward_d, done_d, E, 0, p.T, vec_for(obs_d), cs,
                               b.obs_step, b.out_step);
        }
        if (form.overlapped) {
            if (e == hipSuccess) e = hipEventRecord(stepped[(size_t)d], cs);
            // behind day d's steps in capture order (ahead of them measured the same, profiles/overlapped_reset_ab.txt)
            if (e == hipSuccess && d + 1 < a.days) capture_generator(d + 1);
        }
    }

};

int capture_days(const CaptureArgs &a, SngGraph **out) {
    SngEnv *env = a.env;
    const bool with_reset = (a.flags & SNG_GRAPH_RESET) != 0;
    if (!env || !a.actions || !a.obs || !a.reward || !a.done || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    if (a.days < 1 || (a.days > 1 && !with_reset))
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "days must be >= 1 (more than one needs SNG_GRAPH_RESET)");
    if (with_reset && !device_rng_ok(env))
        return fail(env, SNG_ERR_UNSUPPORTED, "device RNG needs time_interval <= 2h");
    ON_DEVICE_OF(env);
    if (env->p.req_enabled) SNG_TRY(ensure_req(env));
    // with a reset: every day a freshly generated device day (sng_reset(SNG_RNG_DEVICE)); else the loaded day
    const DayKey key = with_reset ? DayKey::device_day(env->p) : DayKey::of(env->p);
    const Params p = with_day(env->p, key);
    const InfoPtrs ip = info_ptrs(a.info);
    Capture c{a, env, graph_form(p, info_diag(ip), a.flags, a.days, policy_kind(a.policy)), p, ip, env->E,
              (aligned16(a.actions) && aligned16(a.obs)) ? 1 : 0, {env->ds, env->ds}};
    HIP_TRY(env, hipStreamCreateWithFlags(&c.cs, hipStreamNonBlocking));
    if (c.form.overlapped) {
        SNG_TRY(ensure_shadow(env, &c.slots[1]));
        c.e = hipStreamCreateWithFlags(&c.gs, hipStreamNonBlocking);
        if (c.e == hipSuccess) c.e = c.generated.create((size_t)a.days, hipEventDisableTiming);
        if (c.e == hipSuccess) c.e = c.stepped.create((size_t)a.days, hipEventDisableTiming);
    }
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    if (c.e == hipSuccess) c.e = hipStreamBeginCapture(c.cs, hipStreamCaptureModeThreadLocal);
    const bool capturing = c.e == hipSuccess;
    // a source's fill of every day's block and its counter's bump: the chain's first nodes
    if (a.noise_source && c.e == hipSuccess)
        c.e = launch_noise_fill(a.noise_source->spec, a.noise_source->params.d, a.noise_source->d_counter, p.env_offset,
                                const_cast<float *>(a.noise), a.days, p.T, env->E, c.cs);
    if (c.form.overlapped) c.fork();
    for (int d = 0; c.e == hipSuccess && d < a.days; ++d) c.capture_day(d);
    if (c.form.overlapped && capturing) c.join();
    // a failed launch still ends the capture on `cs`, before the streams and events are destroyed
    const hipError_t end = capturing ? hipStreamEndCapture(c.cs, &graph) : hipSuccess;
    if (c.e == hipSuccess) c.e = end;
    if (c.e == hipSuccess) c.e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (c.e != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        return hip_fail(env, c.e, "graph capture");
    }
    *out = new SngGraph{env, with_reset, c.form.nodes_per_day, c.form.day_kernel_name, c.form.overlapped, key,
                        env->seed, p.env_offset, graph, exec};
    return SNG_OK;
}

}  // namespace

extern "C" {

int sng_graph_create(SngEnv *env, const float *actions, float *obs, double *reward, uint8_t *done,
                     const SngInfo *info, int flags, int32_t days, double *day_returns, SngGraph **out) {
    return capture_days({env, obs, reward, done, info, flags, days, day_returns, actions}, out);
}

// what both policy entry points check before they capture
static int capture_policy_days(CaptureArgs a, SngGraph **out) {
    if (!a.env || !a.policy || !a.actions_out) return fail(a.env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    if (a.policy->env != a.env) return fail(a.env, SNG_ERR_INVALID_ARGUMENT, "the policy was created for another env");
    a.actions = a.policy->d_env_actions;
    return capture_days(a, out);
}

int sng_graph_create_policy(SngEnv *env, SngPolicy *policy, const float *noise, float *obs, float *actions_out,
                            double *reward, uint8_t *done, const SngInfo *info, int flags, int32_t days,
                            double *day_returns, SngGraph **out) {
    return capture_policy_days({env, obs, reward, done, info, flags, days, day_returns, nullptr, noise, actions_out, policy}, out);
}

int sng_graph_create_policy_noise(SngEnv *env, SngPolicy *policy, SngNoise *noise_source, float *noise_out, float *obs,
                                  float *actions_out, double *reward, uint8_t *done, const SngInfo *info, int flags,
                                  int32_t days, double *day_returns, SngGraph **out) {
    if (!noise_source || !noise_out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    if (noise_source->env != env) return fail(env, SNG_ERR_INVALID_ARGUMENT, "the noise source was created for another env");
    return capture_policy_days({env, obs, reward, done, info, flags, days, day_returns, nullptr, noise_out, actions_out, policy,
                                noise_source}, out);
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
    return g->nodes_per_day;
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

int sng_graph_describe(const SngGraph *g, char *buf, int64_t len) {
    if (!g || !g->graph || len < 0 || (len > 0 && !buf)) return SNG_ERR_INVALID_ARGUMENT;
    SngEnv *env = g->env;
    ON_DEVICE_OF(env);
    static const char *const type_names[] = {"kernel", "memcpy", "memset", "host", "graph", "empty", "wait_event", "event_record"};
    static_assert(hipGraphNodeTypeKernel == 0 && hipGraphNodeTypeEventRecord == 7, "type_names follows hipGraphNodeType");
    size_t n = 0, nd = 0;
    HIP_TRY(env, hipGraphGetNodes(g->graph, nullptr, &n));
    std::vector<hipGraphNode_t> nodes(n), deps;
    if (n) HIP_TRY(env, hipGraphGetNodes(g->graph, nodes.data(), &n));
    std::string text;
    char geometry[96];
    for (size_t i = 0; i < n; ++i) {
        hipGraphNodeType type;
        HIP_TRY(env, hipGraphNodeGetType(nodes[i], &type));
        text += std::to_string(i) + " " + ((unsigned)type < 8u ? type_names[type] : "other");
        if (type == hipGraphNodeTypeKernel) {
            hipKernelNodeParams kp{};
            HIP_TRY(env, hipGraphKernelNodeGetParams(nodes[i], &kp));
            const char *name = hipKernelNameRefByPtr(kp.func, nullptr);
            snprintf(geometry, sizeof geometry, " grid=(%u,%u,%u) block=(%u,%u,%u) lds=%u", kp.gridDim.x, kp.gridDim.y,
                     kp.gridDim.z, kp.blockDim.x, kp.blockDim.y, kp.blockDim.z, kp.sharedMemBytes);
            text += std::string(" ") + (name ? name : "?") + geometry;
        }
        HIP_TRY(env, hipGraphNodeGetDependencies(nodes[i], nullptr, &nd));
        deps.resize(nd);
        if (nd) HIP_TRY(env, hipGraphNodeGetDependencies(nodes[i], deps.data(), &nd));
        std::vector<size_t> idx;   // of the nodes it depends on, ascending
        for (hipGraphNode_t dep : deps) idx.push_back((size_t)(std::find(nodes.begin(), nodes.end(), dep) - nodes.begin()));
        std::sort(idx.begin(), idx.end());
        text += " deps=[";
        for (size_t k = 0; k < idx.size(); ++k) text += (k ? "," : "") + std::to_string(idx[k]);
        text += "]\n";
    }
    if (text.size() > 0x7fffffffu) return fail(env, SNG_ERR_UNSUPPORTED, "sng_graph_describe: the text is longer than an int");
    if ((int64_t)text.size() < len) snprintf(buf, (size_t)len, "%s", text.c_str());
    return (int)text.size();
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
    EventList ev, rev;
    hipError_t e = count_unstepped_device_day(env, st);   // as in sng_reset
    if (e == hipSuccess) e = ev.create(ms ? 2 * (size_t)T * days : 0, hipEventDefault);
    if (e == hipSuccess) e = rev.create(reset_ms ? 2 * (size_t)days : 0, hipEventDefault);
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
    EventList ev;
    hipError_t e = hipMalloc(&in, (size_t)std::max<int64_t>(nr, 1) * 16);
    if (e == hipSuccess) e = hipMalloc(&out, (size_t)std::max<int64_t>(nw, 1) * 16);
    if (e == hipSuccess) e = hipMemsetAsync(in, 0, (size_t)std::max<int64_t>(nr, 1) * 16, st);
    if (e == hipSuccess) e = ev.create(2 * (size_t)reps + 2, hipEventDefault);
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
    if (in) (void)hipFree(in);
    if (out) (void)hipFree(out);
    if (e != hipSuccess) return fail(nullptr, SNG_ERR_HIP, std::string("sng_bandwidth_probe: ") + hipGetErrorString(e));
    if (dispatch_us) *dispatch_us = sum / reps * 1e3f;
    if (back_to_back_us) *back_to_back_us = ms / reps * 1e3f;
    return SNG_OK;
}

}  // extern "C"
