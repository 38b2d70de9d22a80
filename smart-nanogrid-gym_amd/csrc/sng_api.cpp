// sng_api.cpp -- host side of libsng.so: the C ABI declared in include/sng.h, but for checkpoints (sng_state.cpp)
// and day graphs (sng_graph.cpp).
//
// Owns the per-handle device state, uploads the constant tables (sng_host_tables.h), turns days in the
// reference's own layout into the packed per-charger-step words the step kernel reads (sng_host_day.h),
// queues the device kernels that generate a day (the device generator, or the reference's numpy and Python
// MT19937 streams drawn on the device: host threads only seed Python's streams and encode injected days),
// replays the last generated day and steps it.
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>

#include "sng_env.h"
#include "sng_host_day.h"
#include "sng_host_pool.h"
#include "sng_mt.h"

using namespace sng;

namespace sng {

thread_local std::string g_create_error;

int ensure_req(SngEnv *env) {
    if (!env->ds.req) HIP_TRY(env, hipMalloc(&env->ds.req, env->timeline() * sizeof(double)));
    return SNG_OK;
}

int ensure_shadow(SngEnv *env, DeviceState *out) {
    DaySlot &sh = env->shadow;
    const Params &p = env->p;
    const size_t E = (size_t)env->E;
    // a packed day's T + 1 record planes (sng_layout.h), and a spare one: the kernels address the planes through
    // unbounded buffer descriptors, idle lanes of a last wavefront included
    const size_t rec_bytes = (size_t)(p.T + 2) * (size_t)p.n * ((E + 255) / 256 * 256) * sizeof(uint16_t);
    struct {
        void **ptr;
        size_t bytes;
    } const arrays[] = {
        {(void **)&sh.soc, E * p.n * sizeof(double)},
        {(void **)&sh.ratio, E * sizeof(double)},
        {(void **)&sh.pen0, E * sizeof(double)},
        {(void **)&sh.aux, rec_bytes},
        {(void **)&sh.day_return, E * sizeof(double)},
        {(void **)&sh.req, env->ds.req ? env->timeline() * sizeof(double) : 0},
        {(void **)&sh.prof_key, p.noise ? 2 * E * sizeof(uint32_t) : 0},
    };
    for (const auto &a : arrays) {
        if (*a.ptr || !a.bytes) continue;
        HIP_TRY(env, hipMalloc(a.ptr, a.bytes));
        HIP_TRY(env, hipMemset(*a.ptr, 0, a.bytes));
    }
    *out = env->ds;
    out->soc = sh.soc;
    out->ratio = sh.ratio;
    out->pen0 = sh.pen0;
    out->aux = sh.aux;
    out->req = sh.req;
    out->prof_key = sh.prof_key;   // (`word`: a packed day has no word plane)
    return SNG_OK;
}

int await_prepare(SngEnv *env, hipStream_t st) {
    if (env->prep_launched) HIP_TRY(env, hipStreamWaitEvent(st, env->prep_done, 0));
    return SNG_OK;
}

int alloc_streams(SngEnv *env, RefStreams &r) {
    if (r.mt) return SNG_OK;
    HIP_TRY(env, hipMalloc(&r.mt, (size_t)env->E * 2 * kMtN * sizeof(uint32_t)));
    HIP_TRY(env, hipMalloc(&r.pos, (size_t)env->E * sizeof(int32_t)));
    return SNG_OK;
}

// The reference's global RNG streams of every env, np.random.seed(s) and random.seed(s) with
// s = seed + global env index (SngRngMode SNG_RNG_REFERENCE), both on the device.  Python's is seeded on
// the host threads (CPython's init_by_array, sng_mt.h) and uploaded once into the RefStreams layout
// (block 0, position N: the first draw twists), then drawn by observe0_kernel (py_ratio_lane): random.randint(0, 180)
// for a reset's PV ratio, after the day-end draw the last step owes (smart_nanogrid_environment.py:181, 349).
// numpy's np.random.seed takes seeds in [0, 2^32): env i of a reference-RNG population is seeded
// seed + env offset + i, so the last env's seed must stay below 2^32 (mt_seed_kernel would wrap it).
static int check_reference_seed(SngEnv *env) {
    const uint64_t last = env->seed + (uint64_t)env->p.env_offset + (uint64_t)(env->E - 1);
    if (env->seed >= (1ull << 32) || last >= (1ull << 32) || last < env->seed)
        return fail(env, SNG_ERR_INVALID_ARGUMENT,
                    "the reference's RNG streams (a reference-RNG day, or a PV ratio drawn for an injected or replayed "
                    "day): seed + env offset + env index must be < 2^32 (np.random.seed's range)");
    return SNG_OK;
}

// ... and numpy's on the device (mt_seed_kernel), queued on `st`.
int ensure_np_streams(SngEnv *env, hipStream_t st) {
    SNG_TRY(check_reference_seed(env));
    SNG_TRY(alloc_streams(env, env->rs));
    if (!env->np_seeded) {
        SNG_TRY(await_prepare(env, st));
        HIP_TRY(env, launch_ref_seed(env->rs, env->seed + (uint64_t)env->p.env_offset, env->E, st));
        env->np_seeded = true;
        env->prepared = false;   // fresh streams: the first day prepares its blocks inline
    }
    return SNG_OK;
}

}  // namespace sng

namespace {

int ensure_staging(SngEnv *env, bool with_req) {
    const size_t n = env->timeline();
    if (!env->h_word) {
        HIP_TRY(env, hipHostMalloc(&env->h_word, n * sizeof(uint32_t), hipHostMallocDefault));
        HIP_TRY(env, hipHostMalloc(&env->h_aux, n * sizeof(double), hipHostMallocDefault));
        HIP_TRY(env, hipHostMalloc(&env->h_ratio, env->E * sizeof(double), hipHostMallocDefault));
        HIP_TRY(env, hipHostMalloc(&env->h_pen0, env->E * sizeof(double), hipHostMallocDefault));
        HIP_TRY(env, hipEventCreateWithFlags(&env->staging_done, hipEventDisableTiming));
    }
    if (with_req && !env->h_req) HIP_TRY(env, hipHostMalloc(&env->h_req, n * sizeof(double), hipHostMallocDefault));
    // the previous upload must have drained before the staging buffers are rewritten
    HIP_TRY(env, hipEventSynchronize(env->staging_done));
    return SNG_OK;
}

int ensure_py_streams(SngEnv *env, hipStream_t st) {
    const size_t E = (size_t)env->E;
    SNG_TRY(check_reference_seed(env));
    SNG_TRY(alloc_streams(env, env->ps));
    if (env->py_seeded) return SNG_OK;
    SNG_TRY(await_prepare(env, st));   // no preparation may still be writing the streams
    std::vector<uint32_t> words(E * kMtN);
    std::vector<int32_t> pos(E);
    const uint64_t s0 = env->seed + (uint64_t)env->p.env_offset;
    parallel_ranges(env->E, 1024, [&](int64_t b, int64_t en) {
        MT19937 m;
        uint32_t st_words[MT19937::kStateWords];
        for (int64_t i = b; i < en; ++i) {
            m.seed_python(s0 + (uint64_t)i);
            m.save(st_words);
            (void)saved_to_stream(st_words, &words[(size_t)i * kMtN], &pos[i]);   // block 0, mti = N
        }
    });
    HIP_TRY(env, hipMemcpy2DAsync(env->ps.mt, 2 * kMtN * sizeof(uint32_t), words.data(), kMtN * sizeof(uint32_t),
                                  kMtN * sizeof(uint32_t), E, hipMemcpyHostToDevice, st));
    HIP_TRY(env, hipMemcpyAsync(env->ps.pos, pos.data(), E * sizeof(int32_t), hipMemcpyHostToDevice, st));
    // the first twist by a wavefront per env now, not by py_ratio_lane at the first draw
    HIP_TRY(env, launch_mt_prepare(env->ps, env->E, st));
    HIP_TRY(env, hipStreamSynchronize(st));   // the host vectors go out of scope
    env->py_seeded = true;
    return SNG_OK;
}

// Build every env's day on host threads and upload it while the rest is still being built:
// workers take chunks of envs and encode them into the pinned [T][N][E] staging planes; as soon as
// chunk k (in order) is encoded, this thread enqueues its columns of the planes as one 2D copy per
// plane.  build(i, need_req, err) builds env i.  req_upload: the requested-SoC plane goes
// up with the chunks (1), after the last chunk if any env needs it (-1: decided by need_req), or
// not at all (0).  Returns SNG_OK or an error; *need_req_out reports whether any env needed it.
template <class Build>
int build_and_upload(SngEnv *env, int req_upload, hipStream_t st, bool *need_req_out, Build &&build) {
    const int64_t E = env->E;
    const int N = env->p.n, T = env->p.T;
    const size_t rows = (size_t)T * N;
    const int nt = (int)std::min<int64_t>(host_threads(), std::max<int64_t>(1, E / 256));
    const int64_t chunk = std::max<int64_t>(256, (E + 4 * nt - 1) / (4 * nt));   // ~4 chunks per thread
    const int64_t nchunks = (E + chunk - 1) / chunk;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<int> state((size_t)nchunks, 0);   // 0 pending, 1 encoded, 2 failed
    std::vector<std::string> errs((size_t)nchunks);
    std::atomic<int64_t> next{0};
    std::atomic<bool> stop{false}, need_req{false};
    auto worker = [&]() {
        for (;;) {
            const int64_t k = next.fetch_add(1);
            if (k >= nchunks) return;
            int st_k = 1;
            std::string e;
            bool nr = false;
            if (stop.load()) {
                st_k = 2;
                e = "cancelled";
            } else {
                const int64_t b = k * chunk, en = std::min(E, b + chunk);
                for (int64_t i = b; i < en; ++i)
                    if (!build(i, &nr, e)) {
                        st_k = 2;
                        stop.store(true);
                        break;
                    }
            }
            if (nr) need_req.store(true);
            {
                std::lock_guard<std::mutex> lk(mu);
                state[(size_t)k] = st_k;
                errs[(size_t)k] = e;
            }
            cv.notify_one();
        }
    };
    std::vector<std::thread> th;
    for (int w = 0; w < nt; ++w) th.emplace_back(worker);
    int rc = SNG_OK;
    std::string msg;
    for (int64_t k = 0; k < nchunks && rc == SNG_OK; ++k) {
        int st_k;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return state[(size_t)k] != 0; });
            st_k = state[(size_t)k];
            msg = errs[(size_t)k];
        }
        if (st_k != 1) {
            rc = SNG_ERR_INVALID_ARGUMENT;
            break;
        }
        const int64_t b = k * chunk, w = std::min(E, b + chunk) - b;
        hipError_t e = hipMemcpy2DAsync(env->ds.word + b, E * sizeof(uint32_t), env->h_word + b, E * sizeof(uint32_t),
                                        w * sizeof(uint32_t), rows, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipMemcpy2DAsync(env->ds.aux + b, E * sizeof(double), env->h_aux + b, E * sizeof(double),
                                 w * sizeof(double), rows, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && req_upload == 1)
            e = hipMemcpy2DAsync(env->ds.req + b, E * sizeof(double), env->h_req + b, E * sizeof(double),
                                 w * sizeof(double), rows, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) {
            rc = SNG_ERR_HIP;
            msg = std::string("staged upload: ") + hipGetErrorString(e);
        }
    }
    stop.store(rc != SNG_OK);
    for (auto &x : th) x.join();
    if (rc != SNG_OK) return fail(env, rc, msg);
    *need_req_out = need_req.load();
    if (req_upload == -1 && *need_req_out) {
        int r = ensure_req(env);
        if (r) return r;
        HIP_TRY(env, hipMemcpyAsync(env->ds.req, env->h_req, env->timeline() * sizeof(double),
                                    hipMemcpyHostToDevice, st));
    }
    return SNG_OK;
}

// After the day's planes: the PV ratios and t = 0 penalties, then the t = 0 observation.  py_end / py_draw:
// the Python streams' owed day-end draw / the ratio drawn on the device (in observe0_kernel) over the upload.
int finish_host_day(SngEnv *env, bool req_stream, float *obs, hipStream_t st, int py_end, int py_draw) {
    HIP_TRY(env, hipMemcpyAsync(env->ds.ratio, env->h_ratio, env->E * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(env, hipMemcpyAsync(env->ds.pen0, env->h_pen0, env->E * sizeof(double), hipMemcpyHostToDevice, st));
    if (py_end || py_draw) SNG_TRY(await_prepare(env, st));   // the draws themselves run inside observe0_kernel below
    HIP_TRY(env, hipEventRecord(env->staging_done, st));
    load_day(env, DayKey::host_day(req_stream));
    HIP_TRY(env, sng::launch_profiles(env->p, env->ds, env->E, st));
    HIP_TRY(env, sng::launch_observe0(env->p, env->ds, obs, nullptr, env->E, aligned16(obs) ? 1 : 0, st, OBS0_HOST, -1,
                                      &env->ps, (py_draw ? 1 : 0) | (py_end ? 2 : 0)));
    begin_day(env);
    return SNG_OK;
}

// sng_step / sng_step_host: the loaded day has a step left; and that step was queued
int step_begin(SngEnv *env) {
    if (env->t < 0) return fail(env, SNG_ERR_STATE, "step() before reset()");
    if (env->t >= env->p.T) return fail(env, SNG_ERR_STATE, "the day is over: call reset()");
    return SNG_OK;
}
void step_queued(SngEnv *env) {
    env->t += 1;
    if (env->t == env->p.T) env->day_finished = true;
}

}  // namespace

extern "C" {

int32_t sng_abi_version(void) { return SNG_ABI_VERSION; }
#ifndef SNG_BUILD_ID
#define SNG_BUILD_ID "unversioned"   // built outside csrc/Makefile
#endif
const char *sng_build_id(void) { return SNG_BUILD_ID; }

void sng_config_defaults(SngConfig *c) {
    std::memset(c, 0, sizeof *c);
    c->abi_version = SNG_ABI_VERSION;
    c->number_of_chargers = 8;                 // smart_nanogrid_environment.py:32
    c->time_interval_hours = 1.0;              // :138
    c->price_model = 0;
    c->pv_system_available = 1;
    c->battery_system_available = 1;
    c->vehicle_to_everything = 0;
    c->different_vehicle_capacities = 1;
    c->requested_state_of_charge = 0;
    c->charging_mode_bounded = 1;
    c->penalty_mode = SNG_PENALTY_SPARSE;
    c->numpy_legacy_promotion = 0;
    c->grid_cost_weight = 0.75;                // accountant.py:35
    c->battery_penalty_weight = 0.8;           // penaliser.py:181
    c->selling_price_coefficient = 0.8;        // accountant.py:6
    c->bess_capacity_kwh = 80;                 // central_management_system.py:35
    c->bess_initial_soc = 0.5;
    c->bess_max_charging_kw = 44;
    c->bess_max_discharging_kw = 44;
    c->bess_charging_efficiency = 0.95;
    c->bess_discharging_efficiency = 0.95;
    c->bess_depth_of_discharge = 0.15;
    c->ev_max_power_kw = 22;                   // charger.py:20-23
    c->ev_efficiency = 0.95;
}

const char *sng_last_error(const SngEnv *env) { return env ? env->err.c_str() : g_create_error.c_str(); }

int sng_create(const SngConfig *cfg, int device, int64_t num_envs, uint64_t seed, SngEnv **out) {
    if (!out) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    int T = 0;
    std::string err;
    int rc = validate(cfg, &T, err);
    if (rc) return fail(nullptr, rc, err);
    if (num_envs < 1) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "num_envs must be >= 1");
    // the step kernel addresses a charger-major plane ([N][E] f64: the SoC state, one timestep of
    // the timeline) as one raw buffer with 32-bit byte offsets
    if ((uint64_t)num_envs * (uint64_t)cfg->number_of_chargers * sizeof(double) >= (1ull << 32))
        return fail(nullptr, SNG_ERR_INVALID_ARGUMENT,
                    "num_envs * number_of_chargers must be < 2^29 per handle (shard larger populations)");

    SngEnv *env = new SngEnv();
    env->cfg = *cfg;
    env->irradiance.assign(cfg->irradiance_per_minute, cfg->irradiance_per_minute + cfg->irradiance_minutes);
    env->cfg.irradiance_per_minute = env->irradiance.data();
    env->device = device;
    env->E = num_envs;
    env->seed = seed;
    if (!build_tables(env->cfg, T, env->tables, err)) {
        delete env;
        return fail(nullptr, SNG_ERR_UNSUPPORTED, err);
    }
    const SngConfig &c = env->cfg;
    Params &p = env->p;
    if (!fill_params(c, T, seed, p, env->spans)) {
        delete env;
        return fail(nullptr, SNG_ERR_UNSUPPORTED, "step_lanes_per_env not available for this charger count");
    }
    load_day(env, DayKey::host_day(p.req_enabled != 0));   // before the first reset: no day is loaded

    // host copy of the device tables
    Tables &ht = env->host_tab;
    fill_tables(env->tables, ht);
    // checkpoint fingerprint: every configuration scalar that changes the simulation, and the tables
    env->cfg_hash = fnv1a(&ht, sizeof ht, config_fingerprint(c));

    DeviceScope dev(device);
    if (dev.err != hipSuccess) {
        delete env;
        return fail(nullptr, SNG_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(dev.err));
    }
    const size_t E = (size_t)num_envs, tl = env->timeline();
    DeviceState &ds = env->ds;
    const std::vector<double> b(E, c.bess_initial_soc), ones(E, 1.0);
    // the handle's device arrays, in allocation order: where, bytes (0: not for this configuration), and what
    // they start as (host bytes to upload; else zeros if `zero`; else nothing: a day writes it before it is read)
    struct {
        void **ptr;
        size_t bytes;
        const void *host;
        bool zero;
    } const arrays[] = {
        {(void **)&ds.soc, E * p.n * sizeof(double), nullptr, true},
        {(void **)&ds.bess, E * sizeof(double), b.data(), false},
        {(void **)&ds.bess0, E * sizeof(double), b.data(), false},
        {(void **)&ds.ratio, E * sizeof(double), ones.data(), false},
        {(void **)&ds.pen0, E * sizeof(double), nullptr, true},
        {(void **)&ds.word, tl * sizeof(uint32_t), nullptr, true},
        {(void **)&ds.aux, tl * sizeof(double), nullptr, true},
        {(void **)&ds.flags, E * sizeof(uint32_t), nullptr, true},
        {(void **)&ds.episode, sizeof(uint64_t), nullptr, true},
        {(void **)&env->d_tables, sizeof(Tables), &ht, false},
        {(void **)&ds.req, p.req_enabled ? tl * sizeof(double) : 0, nullptr, false},
        {(void **)&ds.prof_key, p.noise ? 2 * E * sizeof(uint32_t) : 0, nullptr, false},
    };
    for (const auto &a : arrays) {
        const hipError_t r = a.bytes ? hipMalloc(a.ptr, a.bytes) : hipSuccess;
        if (r != hipSuccess) {
            sng_destroy(env);
            return fail(nullptr, SNG_ERR_OUT_OF_MEMORY, std::string("hipMalloc: ") + hipGetErrorString(r));
        }
    }
    ds.tables = env->d_tables;
    hipError_t init = hipSuccess;
    for (const auto &a : arrays) {
        if (init != hipSuccess || !a.bytes) continue;
        if (a.host) init = hipMemcpy(*a.ptr, a.host, a.bytes, hipMemcpyHostToDevice);
        else if (a.zero) init = hipMemset(*a.ptr, 0, a.bytes);
    }
    if (init != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        sng_destroy(env);
        return fail(nullptr, SNG_ERR_HIP, "device initialisation failed");
    }
    *out = env;
    return SNG_OK;
}

void sng_destroy(SngEnv *env) {
    if (!env) return;
    DeviceScope scope(env->device);
    if (env->prep_stream) {
        (void)hipStreamSynchronize(env->prep_stream);
        (void)hipStreamDestroy(env->prep_stream);
        (void)hipEventDestroy(env->prep_done);
        (void)hipEventDestroy(env->day_drawn);
    }
    DeviceState &ds = env->ds;
    void *dev[] = {ds.soc, ds.bess, ds.bess0, ds.ratio, ds.pen0, ds.word, ds.aux, ds.req, ds.flags, ds.prof_key,
                   ds.episode, env->d_tables, env->rs.mt, env->rs.pos, env->ps.mt, env->ps.pos,
                   env->shadow.soc, env->shadow.ratio, env->shadow.pen0, env->shadow.aux, env->shadow.req,
                   env->shadow.prof_key, env->shadow.day_return};
    for (void *x : dev)
        if (x) (void)hipFree(x);
    void *host[] = {env->h_word, env->h_aux, env->h_req, env->h_ratio, env->h_pen0};
    for (void *x : host)
        if (x) (void)hipHostFree(x);
    if (env->staging_done) (void)hipEventDestroy(env->staging_done);
    if (env->hio) (void)hipHostFree(env->hio);
    delete env;
}

int sng_get_dims(const SngEnv *env, SngDims *out) {
    if (!env || !out) return SNG_ERR_INVALID_ARGUMENT;
    out->obs_dim = env->p.obs_dim;
    out->act_dim = env->p.act_dim;
    out->timesteps = env->p.T;
    out->number_of_chargers = env->p.n;
    out->num_envs = env->E;
    out->step_lanes_per_env = env->p.lanes;
    out->slots = env->spans.slots;
    return SNG_OK;
}

int sng_get_timestep(const SngEnv *env) { return env ? env->t : -1; }

int sng_set_env_offset(SngEnv *env, int64_t offset) {
    if (!env || offset < 0) return fail(env, SNG_ERR_INVALID_ARGUMENT, "bad env offset");
    env->p.env_offset = offset;
    env->np_seeded = false;   // reference streams are re-seeded (seed + offset + i) at the next reset
    env->py_seeded = false;
    env->day_finished = false;
    return SNG_OK;
}

int sng_set_seed(SngEnv *env, uint64_t seed, void *stream) {
    if (!env) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null handle");
    ON_DEVICE_OF(env);
    env->seed = seed;
    env->p.seed = seed;
    env->np_seeded = false;   // re-seeded (seed + offset + i) at the next reset
    env->py_seeded = false;
    env->day_finished = false;
    env->replays = 0;
    // device days restart at day 0 of the new streams; the loaded day stays loaded
    HIP_TRY(env, hipMemsetAsync(env->ds.episode, 0, sizeof(uint64_t), as_stream(stream)));
    if (DayKey::of(env->p).unstepped_device_day(env->t)) load_day(env, DayKey::of(env->p).disowned());
    HIP_TRY(env, hipStreamSynchronize(as_stream(stream)));
    return SNG_OK;
}

int sng_reset(SngEnv *env, int rng_mode, float *obs, void *stream) {
    if (!env || !obs) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    ON_DEVICE_OF(env);
    hipStream_t st = as_stream(stream);
    const DaySpans &sp = env->spans;
    if (rng_mode == SNG_RNG_DEVICE) {
        if (!device_rng_ok(env)) return fail(env, SNG_ERR_UNSUPPORTED, "device RNG needs time_interval <= 2h");
        if (env->p.req_enabled) SNG_TRY(ensure_req(env));
        // a second device reset with no step in between still draws a new day
        HIP_TRY(env, count_unstepped_device_day(env, st));
        load_day(env, DayKey::device_day(env->p));
        HIP_TRY(env, launch_generate(env->p, env->ds, env->seed, env->E, sp.i4, sp.i10, sp.i1, obs, nullptr,
                                     aligned16(obs) ? 1 : 0, st));
        begin_day(env);
        generated_day_loaded(env, SNG_RNG_DEVICE);
        return SNG_OK;
    }
    if (rng_mode != SNG_RNG_REFERENCE) return fail(env, SNG_ERR_INVALID_ARGUMENT, "unknown rng_mode");

    // the day on the device (ref_day2_kernel: numpy's stream, draw for draw), then the PV ratio from each
    // env's Python stream on the device, after the day-end draw the last step still owes
    // (smart_nanogrid_environment.py:181, 349)
    SNG_TRY(ensure_np_streams(env, st));
    SNG_TRY(ensure_py_streams(env, st));
    const bool with_req = env->p.req_enabled != 0;
    if (with_req) SNG_TRY(ensure_req(env));
    SNG_TRY(await_prepare(env, st));
    if (!env->prep_stream) {
        HIP_TRY(env, hipStreamCreateWithFlags(&env->prep_stream, hipStreamNonBlocking));
        HIP_TRY(env, hipEventCreateWithFlags(&env->prep_done, hipEventDisableTiming));
        HIP_TRY(env, hipEventCreateWithFlags(&env->day_drawn, hipEventDisableTiming));
    }
    load_day(env, DayKey::host_day(with_req));
    HIP_TRY(env, launch_ref_day(env->p, env->ds, env->rs, env->E, sp.i4, sp.i10, sp.i1, !env->prepared, st));
    HIP_TRY(env, sng::launch_profiles(env->p, env->ds, env->E, st));
    // (the t = 0 penalty of a generated day is 0: observe0 writes it)
    // (the PV ratio from each env's Python stream, after the owed day-end draw, inside observe0_kernel)
    HIP_TRY(env, sng::launch_observe0(env->p, env->ds, obs, nullptr, env->E, aligned16(obs) ? 1 : 0, st, OBS0_GENERATED,
                                      -1, &env->ps, 1 | (env->day_finished ? 2 : 0)));
    // the next day's blocks of both streams, on the side stream, while this day is stepped
    // (mt_prepare_kernel: about every other day twists a numpy block, ~0.1 ms at 65,536 envs, off the next
    // reset's critical path); queued behind the t = 0 observation, which it would otherwise slow down
    HIP_TRY(env, hipEventRecord(env->day_drawn, st));
    HIP_TRY(env, hipStreamWaitEvent(env->prep_stream, env->day_drawn, 0));
    HIP_TRY(env, launch_mt_prepare(env->rs, env->E, env->prep_stream));
    HIP_TRY(env, launch_mt_prepare(env->ps, env->E, env->prep_stream));
    HIP_TRY(env, hipEventRecord(env->prep_done, env->prep_stream));
    env->prep_launched = true;
    env->prepared = true;
    begin_day(env);
    generated_day_loaded(env, SNG_RNG_REFERENCE);
    return SNG_OK;
}

int sng_reset_replay(SngEnv *env, float *obs, void *stream) {
    if (!env || !obs) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    if (env->gen_mode < 0 || !env->gen_loaded)
        return fail(env, SNG_ERR_STATE,
                    env->gen_mode < 0 ? "reset(generate_new_initial_values=False) replays the last generated day "
                                        "(initial_values.json, charging_station.py:185-186): none was generated yet"
                                      : "reset(generate_new_initial_values=False) replays the last generated day; an "
                                        "injected day (sng_reset_from_scenario) has replaced it since");
    ON_DEVICE_OF(env);
    hipStream_t st = as_stream(stream);
    const int vec = aligned16(obs) ? 1 : 0;
    // a device day replayed before any step was never counted, and the replay's steps do not count it
    // (DayKey::replayed), so count it here: the next device reset then draws a new day
    HIP_TRY(env, count_unstepped_device_day(env, st));
    if (env->gen_mode == SNG_RNG_REFERENCE) {
        // a new random_pv_shift_ratio from each env's Python stream (smart_nanogrid_environment.py:349),
        // after the day-end draw the last step still owes (:181); the numpy stream is not touched
        SNG_TRY(ensure_py_streams(env, st));
        SNG_TRY(await_prepare(env, st));
        load_day(env, DayKey::of(env->p).replayed());
        HIP_TRY(env, sng::launch_observe0(env->p, env->ds, obs, nullptr, env->E, vec, st, OBS0_REPLAY, -1, &env->ps,
                                          1 | (env->day_finished ? 2 : 0)));
    } else {
        load_day(env, DayKey::of(env->p).replayed());
        HIP_TRY(env, sng::launch_observe0(env->p, env->ds, obs, nullptr, env->E, vec, st, OBS0_REPLAY,
                                          (int64_t)env->replays));
        env->replays += 1;
    }
    begin_day(env);
    return SNG_OK;
}

int sng_reset_from_scenario(SngEnv *env, const SngScenario *sc, float *obs, void *stream) {
    if (!env || !sc || !obs) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    if (sc->slots != env->spans.slots)
        return fail(env, SNG_ERR_INVALID_ARGUMENT,
                    "scenario slots must be " + std::to_string(env->spans.slots) + " (25; T+1 with extended_day)");
    if (!sc->soc || !sc->occupancy || !sc->capacity || !sc->requested_soc || !sc->arrivals || !sc->departures ||
        sc->max_vehicles < 1)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "incomplete scenario");
    ON_DEVICE_OF(env);
    SNG_TRY(ensure_staging(env, true));
    // Python-stream accounting (env i == the reference seeded seed + i): the day-end draw the last
    // step still owes (smart_nanogrid_environment.py:181), and, when no ratio is given, the reset's own
    // draw (:349) -- what reset(generate_new_initial_values=False) consumes
    const bool draw_ratio = sc->pv_ratio == nullptr;
    if (draw_ratio) SNG_TRY(ensure_py_streams(env, as_stream(stream)));
    const bool end_draw = env->day_finished && env->py_seeded;
    const int N = env->p.n, V = sc->max_vehicles, S = env->spans.slots;
    // the requested-SoC plane goes up with the chunks when the config enables it (the step reads it
    // then), else only if some penalised slot of the given days is not 1.0
    const bool req_enabled = env->p.req_enabled != 0;
    if (req_enabled) SNG_TRY(ensure_req(env));
    bool need = false;
    int rc = build_and_upload(env, req_enabled ? 1 : -1, as_stream(stream), &need,
                          [&](int64_t i, bool *nr, std::string &e) -> bool {
                              const size_t o = (size_t)i * N * S, ol = (size_t)i * N * V;
                              DayView d{const_cast<double *>(sc->soc + o), const_cast<double *>(sc->occupancy + o),
                                        const_cast<double *>(sc->capacity + o),
                                        const_cast<double *>(sc->requested_soc + o),
                                        const_cast<int32_t *>(sc->arrivals + ol),
                                        const_cast<int32_t *>(sc->departures + ol), V, S};
                              env->h_ratio[i] = draw_ratio ? 1.0 : sc->pv_ratio[i];   // (drawn on the device)
                              if (!encode_day(env->p, env->E, i, d, env->h_word, env->h_aux, env->h_req,
                                              &env->h_pen0[i], nr, e)) {
                                  e = "env " + std::to_string(i) + ": " + e;
                                  return false;
                              }
                              return true;
                          });
    if (rc) {
        // chunks before the failing env are already uploaded over the loaded day's planes: the loaded
        // day is no longer valid, so step, replay and steps-only graphs refuse until the next reset (no
        // Python-stream draw was made)
        env->t = -1;
        env->gen_loaded = false;
        env->day_finished = false;
        env->err += " (the loaded day was partly overwritten: reset again)";
        return rc;
    }
    SNG_TRY(finish_host_day(env, req_enabled || need, obs, as_stream(stream), end_draw ? 1 : 0, draw_ratio ? 1 : 0));
    env->gen_loaded = false;   // the generated day a replay restores is no longer loaded
    return SNG_OK;
}

int sng_step(SngEnv *env, const float *actions, float *obs, double *reward, uint8_t *done, const SngInfo *info,
             void *stream) {
    if (!env || !actions || !obs || !reward || !done) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    SNG_TRY(step_begin(env));
    ON_DEVICE_OF(env);
    const int vec = (aligned16(actions) && aligned16(obs)) ? 1 : 0;
    HIP_TRY(env, launch_step(env->p, env->ds, info_ptrs(info), env->host_tab, actions, obs, reward, done, env->E, env->t, vec,
                             as_stream(stream)));
    step_queued(env);
    return SNG_OK;
}

int sng_step_host(SngEnv *env, const float *actions, float *obs, double *reward, uint8_t *done, uint32_t *step_flags,
                  const SngInfo *info, void *stream) {
    if (!env || !actions || !obs || !reward || !done || !step_flags)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    SNG_TRY(step_begin(env));
    if (info && info->flags)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "sng_step_host returns the step's flags itself: SngInfo.flags must be null");
    ON_DEVICE_OF(env);
    hipStream_t st = as_stream(stream);
    const size_t E = (size_t)env->E, A = (size_t)env->p.act_dim, O = (size_t)env->p.obs_dim;
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    // [actions E x A f32 | obs E x O f32 | reward E f64 | done E u8 | flags E u32], sections 256 B aligned
    const size_t o_obs = al(E * A * 4), o_rew = o_obs + al(E * O * 4), o_done = o_rew + al(E * 8),
                 o_fl = o_done + al(E), bytes = o_fl + al(E * 4);
    if (env->hio_bytes < bytes) {
        if (env->hio) (void)hipHostFree(env->hio);
        env->hio = env->hio_dev = nullptr;
        env->hio_bytes = 0;
        HIP_TRY(env, hipHostMalloc((void **)&env->hio, bytes, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(env, hipHostGetDevicePointer((void **)&env->hio_dev, env->hio, 0));
        env->hio_bytes = bytes;
    }
    char *h = env->hio, *d = env->hio_dev;
    std::memcpy(h, actions, E * A * 4);
    InfoPtrs ip = info_ptrs(info);
    ip.flags = reinterpret_cast<uint32_t *>(d + o_fl);   // this step's flags of every env (the sticky ones stay)
    HIP_TRY(env, launch_step(env->p, env->ds, ip, env->host_tab, reinterpret_cast<const float *>(d),
                             reinterpret_cast<float *>(d + o_obs), reinterpret_cast<double *>(d + o_rew),
                             reinterpret_cast<uint8_t *>(d + o_done), env->E, env->t, 1, st));
    step_queued(env);
    HIP_TRY(env, hipStreamSynchronize(st));
    std::memcpy(obs, h + o_obs, E * O * 4);
    std::memcpy(reward, h + o_rew, E * 8);
    std::memcpy(done, h + o_done, E);
    std::memcpy(step_flags, h + o_fl, E * 4);
    return SNG_OK;
}

int sng_step_kernel_name(const SngEnv *env, const SngInfo *info, char *buf, int32_t len) {
    if (!env || !buf || len < 1) return SNG_ERR_INVALID_ARGUMENT;
    const int n = step_plan_name(step_plan(env->p, info_diag(info_ptrs(info))), buf, len);
    return (n > 0 && n < len) ? SNG_OK : SNG_ERR_INVALID_ARGUMENT;
}

int sng_read_errors(SngEnv *env, uint32_t *host_flags, int clear, void *stream) {
    if (!env || !host_flags) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    ON_DEVICE_OF(env);
    hipStream_t st = as_stream(stream);
    HIP_TRY(env, hipMemcpyAsync(host_flags, env->ds.flags, env->E * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (clear) HIP_TRY(env, hipMemsetAsync(env->ds.flags, 0, env->E * sizeof(uint32_t), st));
    HIP_TRY(env, hipStreamSynchronize(st));
    return SNG_OK;
}

// One per-env f64 array between the device and the host, ordered on `stream` (the caller's work on it
// completes first); synchronises that stream only.
static int copy_env_array(SngEnv *env, double *dev, double *host, bool to_host, void *stream, const char *what) {
    if (!env) return SNG_ERR_INVALID_ARGUMENT;
    if (!host) return fail(env, SNG_ERR_INVALID_ARGUMENT, std::string(what) + ": null host array");
    ON_DEVICE_OF(env);
    hipStream_t st = as_stream(stream);
    if (to_host)
        HIP_TRY(env, hipMemcpyAsync(host, dev, env->E * sizeof(double), hipMemcpyDeviceToHost, st));
    else
        HIP_TRY(env, hipMemcpyAsync(dev, host, env->E * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(env, hipStreamSynchronize(st));
    return SNG_OK;
}

int sng_get_battery_soc(SngEnv *env, double *h, void *stream) {
    return env ? copy_env_array(env, env->ds.bess, h, true, stream, "sng_get_battery_soc") : SNG_ERR_INVALID_ARGUMENT;
}

int sng_set_battery_soc(SngEnv *env, const double *h, void *stream) {
    return env ? copy_env_array(env, env->ds.bess, const_cast<double *>(h), false, stream, "sng_set_battery_soc")
               : SNG_ERR_INVALID_ARGUMENT;
}

int sng_get_pv_ratio(SngEnv *env, double *h, void *stream) {
    return env ? copy_env_array(env, env->ds.ratio, h, true, stream, "sng_get_pv_ratio") : SNG_ERR_INVALID_ARGUMENT;
}

// The SoC state on the host (charger pairs, sng_layout.h soc_index) and, on a packed day past t = 0, the records
// of the last stepped step t - 1 (plane t, charger quads: rec_index): there an empty charger's running SoC
// carries the next arrival's (sng_layout.h) while SOC[c, t] shows 0, and the record's OCC bit is the step's
// occupancy.  rec stays empty on any other day; the SoC is pulled then only if the caller asks (`soc_always`).
static int pull_vehicle_soc(SngEnv *env, hipStream_t st, bool soc_always, std::vector<double> &soc,
                            std::vector<uint16_t> &rec) {
    const bool packed_mid = env->p.packed && env->t >= 1;
    soc.resize((size_t)env->p.n * env->E);
    if (!soc_always && !packed_mid) return SNG_OK;
    HIP_TRY(env, hipMemcpyAsync(soc.data(), env->ds.soc, soc.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (packed_mid) {
        rec.resize(soc.size());
        HIP_TRY(env, hipMemcpyAsync(rec.data(), reinterpret_cast<const uint16_t *>(env->ds.aux) + (size_t)env->t * rec.size(),
                                    rec.size() * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(env, hipStreamSynchronize(st));
    return SNG_OK;
}

int sng_get_vehicle_soc(SngEnv *env, double *h, void *stream) {
    if (!env) return SNG_ERR_INVALID_ARGUMENT;
    if (!h) return fail(env, SNG_ERR_INVALID_ARGUMENT, "sng_get_vehicle_soc: null host array");
    ON_DEVICE_OF(env);
    const int N = env->p.n;
    std::vector<double> tmp;
    std::vector<uint16_t> rec;
    SNG_TRY(pull_vehicle_soc(env, as_stream(stream), true, tmp, rec));
    for (int64_t e = 0; e < env->E; ++e)
        for (int c = 0; c < N; ++c)   // -> [E][N] on the host; an empty charger of a packed day shows 0
            h[e * N + c] = (!rec.empty() && !(rec[rec_index(c, e, N, env->E)] & W_OCC)) ? 0.0 : tmp[soc_index(c, e, N, env->E)];
    return SNG_OK;
}

int sng_set_vehicle_soc(SngEnv *env, const double *h, void *stream) {
    if (!env) return SNG_ERR_INVALID_ARGUMENT;
    if (!h) return fail(env, SNG_ERR_INVALID_ARGUMENT, "sng_set_vehicle_soc: null host array");
    ON_DEVICE_OF(env);
    const int N = env->p.n;
    hipStream_t st = as_stream(stream);
    std::vector<double> tmp;
    std::vector<uint16_t> rec;
    SNG_TRY(pull_vehicle_soc(env, st, false, tmp, rec));
    for (int64_t e = 0; e < env->E; ++e)
        for (int c = 0; c < N; ++c)   // a packed day mid-day: empty chargers keep the arrival SoC they carry
            if (rec.empty() || (rec[rec_index(c, e, N, env->E)] & W_OCC)) tmp[soc_index(c, e, N, env->E)] = h[e * N + c];
    HIP_TRY(env, hipMemcpyAsync(env->ds.soc, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(env, hipStreamSynchronize(st));
    return SNG_OK;
}

// The loaded day of envs [first, first + count) in the reference's layout (decode_day, sng_host_day.h).  The
// env range's columns of each plane come over in one 2D copy.
int sng_get_scenario(SngEnv *env, int64_t first, int64_t count, int32_t V, double *soc, double *occupancy,
                     double *capacity, double *requested_soc, int32_t *arrivals, int32_t *departures,
                     int32_t *n_vehicles, double *pv_ratio, void *stream) {
    if (!env || !soc || !occupancy || !capacity || !requested_soc || !arrivals || !departures || !n_vehicles ||
        !pv_ratio)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    if (first < 0 || count < 1 || first + count > env->E || V < 1)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "env range or max_vehicles out of range");
    if (env->t < 0) return fail(env, SNG_ERR_STATE, "no day yet: call reset()");
    ON_DEVICE_OF(env);
    hipStream_t st = as_stream(stream);
    const int N = env->p.n, T = env->p.T, S = env->spans.slots;
    const size_t rows = (size_t)T * N, pitch = (size_t)env->E, cnt = (size_t)count;
    std::vector<uint32_t> w(rows * cnt);
    std::vector<double> aux(rows * cnt), rq;
    std::vector<uint16_t> rec;
    if (env->p.packed) {   // device-RNG day: 2 B packed records in charger quads (sng_layout.h), T + 1 planes
        // rec[plane][c][k] for the env range, one 2D copy (over the planes) per quad row: the range's slots
        // of quad row c0 are one run of count * width records
        rec.resize(rows * cnt + (size_t)N * cnt);
        std::vector<uint16_t> q((size_t)(T + 1) * 4 * cnt);
        for (int c0 = 0; c0 < N; c0 += 4) {
            const int wq = N - c0 < 4 ? N - c0 : 4;
            HIP_TRY(env, hipMemcpy2DAsync(q.data(), cnt * wq * sizeof(uint16_t),
                                          reinterpret_cast<const uint16_t *>(env->ds.aux) + (size_t)c0 * pitch + first * wq,
                                          (size_t)N * pitch * sizeof(uint16_t), cnt * wq * sizeof(uint16_t), (size_t)T + 1,
                                          hipMemcpyDeviceToHost, st));
            HIP_TRY(env, hipStreamSynchronize(st));
            for (int tp = 0; tp <= T; ++tp)
                for (int cc = 0; cc < wq; ++cc)
                    for (size_t k = 0; k < cnt; ++k)
                        rec[((size_t)tp * N + c0 + cc) * cnt + k] = q[(size_t)tp * cnt * wq + k * wq + cc];
        }
    } else {
        HIP_TRY(env, hipMemcpy2DAsync(w.data(), cnt * sizeof(uint32_t), env->ds.word + first, pitch * sizeof(uint32_t),
                                      cnt * sizeof(uint32_t), rows, hipMemcpyDeviceToHost, st));
        HIP_TRY(env, hipMemcpy2DAsync(aux.data(), cnt * sizeof(double), env->ds.aux + first, pitch * sizeof(double),
                                      cnt * sizeof(double), rows, hipMemcpyDeviceToHost, st));
    }
    const bool have_req = env->p.req_stream && !env->p.req_zero && env->ds.req;
    if (have_req) {
        rq.resize(rows * cnt);
        HIP_TRY(env, hipMemcpy2DAsync(rq.data(), cnt * sizeof(double), env->ds.req + first, pitch * sizeof(double),
                                      cnt * sizeof(double), rows, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(env, hipMemcpyAsync(pv_ratio, env->ds.ratio + first, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(env, hipStreamSynchronize(st));
    if (env->p.packed) records_to_words(rec.data(), (size_t)N * cnt, T, w.data(), aux.data());
    for (size_t k = 0; k < cnt; ++k) {
        const DayView d{soc + k * N * S, occupancy + k * N * S, capacity + k * N * S, requested_soc + k * N * S,
                        arrivals + k * N * V, departures + k * N * V, V, S};
        decode_day(env->p, cnt, k, w.data(), aux.data(), have_req ? rq.data() : nullptr, d, n_vehicles + k * N);
    }
    return SNG_OK;
}

int sng_get_tables(const SngEnv *env, double *irr, double *irr_max, double *pv_power, double *price,
                   double *price_max, int32_t *n) {
    if (!env) return SNG_ERR_INVALID_ARGUMENT;
    const auto &tb = env->tables;
    if (irr) std::memcpy(irr, tb.irr.data(), tb.irr.size() * sizeof(double));
    if (pv_power) std::memcpy(pv_power, tb.pv_power.data(), tb.pv_power.size() * sizeof(double));
    if (price) std::memcpy(price, tb.price.data(), tb.price.size() * sizeof(double));
    if (irr_max) *irr_max = tb.irr_max;
    if (price_max) *price_max = tb.price_max;
    if (n) *n = (int32_t)tb.irr.size();
    return SNG_OK;
}

int sng_host_generate_scenarios(const SngConfig *cfg, int64_t num_envs, uint64_t seed, int32_t episodes, double *soc,
                                double *occupancy, double *capacity, double *requested_soc, int32_t *arrivals,
                                int32_t *departures, int32_t max_vehicles, double *pv_ratio) {
    int T = 0;
    std::string err;
    int rc = validate(cfg, &T, err);
    if (rc) return fail(nullptr, rc, err);
    if (num_envs < 1 || episodes < 1 || max_vehicles < 1)
        return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "bad sizes");
    const DayView out{soc, occupancy, capacity, requested_soc, arrivals, departures, max_vehicles, day_slots(*cfg, T)};
    if (!generate_scenarios(*cfg, T, num_envs, seed, episodes, out, pv_ratio))
        return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "max_vehicles too small");
    return SNG_OK;
}

int32_t sng_host_threads(void) { return host_threads(); }

int sng_get_day_counter(SngEnv *env, uint64_t *out, void *stream) {
    if (!env) return SNG_ERR_INVALID_ARGUMENT;
    if (!out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "sng_get_day_counter: null output");
    ON_DEVICE_OF(env);
    HIP_TRY(env, hipMemcpyAsync(out, env->ds.episode, sizeof(uint64_t), hipMemcpyDeviceToHost, as_stream(stream)));
    HIP_TRY(env, hipStreamSynchronize(as_stream(stream)));
    return SNG_OK;
}

}  // extern "C"
