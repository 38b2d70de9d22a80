// sng_state.cpp -- checkpoint / resume of a handle (sng_state_size, sng_get_state, sng_set_state): the blob
// that sng_state_format.h lays out, pulled from and pushed to the handle's device arrays.
#include <cstring>

#include "sng_env.h"

using namespace sng;

namespace {

// The blob's device sections behind the header, in blob order, for this handle and the header's section flags:
// sng_get_state pulls them, sng_set_state pushes them (the RNG streams follow, converted on the host).
struct StateSection {
    void *dev;
    size_t bytes;
};
std::vector<StateSection> state_sections(const SngEnv *env, const StateHeader &h, const double *ep_return) {
    const size_t E = (size_t)env->E, tl = env->timeline();
    const DeviceState &ds = env->ds;
    std::vector<StateSection> s = {{ds.soc, (size_t)env->p.n * E * 8}, {ds.bess, E * 8}, {ds.bess0, E * 8},
                                   {ds.ratio, E * 8}, {ds.pen0, E * 8}, {ds.flags, E * 4}};
    if (h.has_word) s.push_back({ds.word, tl * 4});
    s.push_back({ds.aux, tl * 8});
    if (h.has_req) s.push_back({ds.req, tl * 8});
    if (h.has_prof) s.push_back({ds.prof_key, 2 * E * 4});
    if (h.has_return) s.push_back({const_cast<double *>(ep_return), E * 8});
    return s;
}

uint64_t state_bytes(const SngEnv *env, const StateHeader &h) {
    size_t b = sizeof(StateHeader) + (h.has_streams ? (size_t)env->E * 2 * MT19937::kStateWords * 4 : 0);
    for (const StateSection &s : state_sections(env, h, nullptr)) b += s.bytes;
    return b;
}

StateHeader state_layout(const SngEnv *env, bool with_return) {
    StateHeader h{};
    std::memcpy(h.magic, kStateMagic, sizeof h.magic);
    h.abi = SNG_ABI_VERSION;
    h.header_bytes = (int32_t)sizeof(StateHeader);
    h.num_envs = env->E;
    h.n = env->p.n;
    h.T = env->p.T;
    h.slots = env->spans.slots;
    h.obs_dim = env->p.obs_dim;
    h.config_hash = env->cfg_hash;
    h.seed = env->seed;
    h.env_offset = env->p.env_offset;
    h.t = env->t;
    h.day_finished = env->day_finished ? 1 : 0;
    h.day = DayKey::of(env->p);
    h.gen_mode = env->gen_mode;
    h.gen_loaded = env->gen_loaded ? 1 : 0;
    h.replays = env->replays;
    h.has_word = env->p.packed ? 0 : 1;
    h.has_req = (env->ds.req && env->p.req_stream) ? 1 : 0;
    h.has_prof = env->ds.prof_key ? 1 : 0;
    h.has_return = with_return ? 1 : 0;
    h.has_streams = env->py_seeded ? 1 : 0;
    h.total_bytes = state_bytes(env, h);
    return h;
}

}  // namespace

extern "C" {

int sng_state_size(const SngEnv *env, int with_return, size_t *bytes) {
    if (!env || !bytes) return SNG_ERR_INVALID_ARGUMENT;
    *bytes = (size_t)state_layout(env, with_return != 0).total_bytes;
    return SNG_OK;
}

int sng_get_state(SngEnv *env, void *buf, size_t bytes, const double *episode_return, void *stream) {
    if (!env || !buf) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    ON_DEVICE_OF(env);
    hipStream_t st = as_stream(stream);
    StateHeader h = state_layout(env, episode_return != nullptr);
    if (bytes < h.total_bytes) return fail(env, SNG_ERR_INVALID_ARGUMENT, "state buffer too small (sng_state_size)");
    const size_t E = (size_t)env->E;
    char *out = static_cast<char *>(buf) + sizeof(StateHeader);
    auto pull = [&](const void *dev, size_t n) -> hipError_t {
        hipError_t e = hipMemcpyAsync(out, dev, n, hipMemcpyDeviceToHost, st);
        out += n;
        return e;
    };
    // the numpy streams live on the device: seeded here if no reference day drew from them yet
    std::vector<uint32_t> np_words, py_words;
    std::vector<int32_t> np_pos, py_pos;
    if (h.has_streams) {
        SNG_TRY(ensure_np_streams(env, st));
        SNG_TRY(await_prepare(env, st));
        np_words.resize(E * 2 * kMtN);
        py_words.resize(E * 2 * kMtN);
        np_pos.resize(E);
        py_pos.resize(E);
        HIP_TRY(env, hipMemcpyAsync(np_words.data(), env->rs.mt, np_words.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(env, hipMemcpyAsync(np_pos.data(), env->rs.pos, E * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(env, hipMemcpyAsync(py_words.data(), env->ps.mt, py_words.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(env, hipMemcpyAsync(py_pos.data(), env->ps.pos, E * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(env, hipMemcpyAsync(&h.day_counter, env->ds.episode, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    for (const StateSection &x : state_sections(env, h, episode_return)) HIP_TRY(env, pull(x.dev, x.bytes));
    HIP_TRY(env, hipStreamSynchronize(st));
    if (h.has_streams) {
        uint32_t *w = reinterpret_cast<uint32_t *>(out);
        for (size_t i = 0; i < E; ++i) {   // numpy's RandomState, then Python's random
            stream_to_saved(&np_words[i * 2 * kMtN], np_pos[i], w + (2 * i) * MT19937::kStateWords);
            stream_to_saved(&py_words[i * 2 * kMtN], py_pos[i], w + (2 * i + 1) * MT19937::kStateWords);
        }
    }
    std::memcpy(buf, &h, sizeof h);
    return SNG_OK;
}

int sng_set_state(SngEnv *env, const void *buf, size_t bytes, double *episode_return, void *stream) {
    if (!env || !buf) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    if (bytes < sizeof(StateHeader)) return fail(env, SNG_ERR_INVALID_ARGUMENT, "not an sng state");
    StateHeader h;
    std::memcpy(&h, buf, sizeof h);
    if (std::memcmp(h.magic, kStateMagic, sizeof h.magic - 1) == 0 && h.magic[7] != kStateMagic[7])
        return fail(env, SNG_ERR_INVALID_ARGUMENT,
                    std::string("unsupported checkpoint version ") + h.magic[7] + " (this library reads version " +
                        kStateMagic[7] + ")");
    if (std::memcmp(h.magic, kStateMagic, sizeof h.magic) != 0 || h.abi != SNG_ABI_VERSION ||
        h.header_bytes != (int32_t)sizeof(StateHeader))
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "not an sng state of this ABI version");
    if (h.num_envs != env->E || h.n != env->p.n || h.T != env->p.T || h.slots != env->spans.slots ||
        h.obs_dim != env->p.obs_dim || h.config_hash != env->cfg_hash)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "state of a handle with another configuration or size");
    // the sections the header announces must be self-consistent before any of them is read
    auto flag = [](int32_t v) { return v == 0 || v == 1; };
    if (!flag(h.has_word) || !flag(h.has_req) || !flag(h.has_prof) || !flag(h.has_return) || !flag(h.has_streams) ||
        !flag(h.day.packed) || h.has_word != 1 - h.day.packed || state_bytes(env, h) != h.total_bytes)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "corrupt state header (inconsistent sections or size)");
    if (h.total_bytes > bytes) return fail(env, SNG_ERR_INVALID_ARGUMENT, "truncated state");
    if (h.has_return && !episode_return)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "the state holds day returns: pass an episode_return array");
    if ((h.has_prof != 0) != (env->ds.prof_key != nullptr)) return fail(env, SNG_ERR_INVALID_ARGUMENT, "profile mismatch");
    if (h.t < -1 || h.t > env->p.T) return fail(env, SNG_ERR_INVALID_ARGUMENT, "bad timestep in state");
    ON_DEVICE_OF(env);
    hipStream_t st = as_stream(stream);
    if (h.has_req) SNG_TRY(ensure_req(env));
    const size_t E = (size_t)env->E;
    const char *in = static_cast<const char *>(buf) + sizeof(StateHeader);
    auto push = [&](void *dev, size_t n) -> hipError_t {
        hipError_t e = hipMemcpyAsync(dev, in, n, hipMemcpyHostToDevice, st);
        in += n;
        return e;
    };
    // the restored streams, checked before anything is changed: both into block 0 of the device streams
    // (position = mti)
    std::vector<uint32_t> np_words, py_words;
    std::vector<int32_t> np_pos, py_pos;
    if (h.has_streams) {
        const size_t off = h.total_bytes - E * 2 * MT19937::kStateWords * 4;
        const uint32_t *w = reinterpret_cast<const uint32_t *>(static_cast<const char *>(buf) + off);
        np_words.resize(E * kMtN);
        py_words.resize(E * kMtN);
        np_pos.resize(E);
        py_pos.resize(E);
        for (size_t i = 0; i < E; ++i)
            if (!saved_to_stream(w + (2 * i) * MT19937::kStateWords, &np_words[i * kMtN], &np_pos[i]) ||
                !saved_to_stream(w + (2 * i + 1) * MT19937::kStateWords, &py_words[i * kMtN], &py_pos[i]))
                return fail(env, SNG_ERR_INVALID_ARGUMENT, "corrupt RNG stream state");
        SNG_TRY(alloc_streams(env, env->rs));
        SNG_TRY(alloc_streams(env, env->ps));
        SNG_TRY(await_prepare(env, st));   // no preparation may still be writing the streams
    }
    HIP_TRY(env, hipMemcpyAsync(env->ds.episode, &h.day_counter, sizeof(uint64_t), hipMemcpyHostToDevice, st));
    for (const StateSection &x : state_sections(env, h, episode_return)) HIP_TRY(env, push(x.dev, x.bytes));
    if (h.has_streams) {
        HIP_TRY(env, hipMemcpy2DAsync(env->rs.mt, 2 * kMtN * sizeof(uint32_t), np_words.data(), kMtN * sizeof(uint32_t),
                                      kMtN * sizeof(uint32_t), E, hipMemcpyHostToDevice, st));
        HIP_TRY(env, hipMemcpyAsync(env->rs.pos, np_pos.data(), E * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(env, hipMemcpy2DAsync(env->ps.mt, 2 * kMtN * sizeof(uint32_t), py_words.data(), kMtN * sizeof(uint32_t),
                                      kMtN * sizeof(uint32_t), E, hipMemcpyHostToDevice, st));
        HIP_TRY(env, hipMemcpyAsync(env->ps.pos, py_pos.data(), E * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(env, hipStreamSynchronize(st));
    env->seed = h.seed;
    env->p.seed = h.seed;
    env->p.env_offset = h.env_offset;
    env->t = h.t;
    env->day_finished = h.day_finished != 0;
    load_day(env, h.day);
    env->gen_mode = h.gen_mode;
    env->gen_loaded = h.gen_loaded != 0;
    env->replays = h.replays;
    env->np_seeded = h.has_streams != 0;
    env->py_seeded = h.has_streams != 0;
    env->prepared = false;   // the restored position says what the next day still has to prepare
    return SNG_OK;
}

}  // extern "C"
