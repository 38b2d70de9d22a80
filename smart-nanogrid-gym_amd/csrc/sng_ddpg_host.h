// sng_ddpg_host.h -- the off-policy side of a DDPG / TD3 iteration in host form (include/sng.h, sng_replay_create and
// sng_critic_create): the replay ring's bookkeeping, the sampling law, the critic's validation, image and arithmetic,
// and the TD target.  The sampling law and the target are written once as host-and-device functions, as
// sng_noise_host.h writes the noise, so that replay_sample_kernel and q_net_kernel (sng_ddpg.h) compile from the same
// text as the host models and agree bit for bit.  Nothing of the critic's forward pass is stated here that another
// header does not state already: Q(s, a) is mlp_net_host (sng_policy_net_host.h) on a NetImage packed by net_pack for
// (obs_dim + act_dim, 1, hidden1, hidden2), over rows [obs row | action row].  No HIP: it compiles with plain g++
// (tests/native/ddpg_host_check.cpp); build with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sng.h"
#include "sng_noise_host.h"
#include "sng_policy_net_host.h"

namespace sng {

// ------------------------------------------------------------------------------------------------- the replay ring
// The ring's host state: `head` is the slot the next pushed day goes to, `filled` the slots that hold a day.
struct ReplayRing {
    int32_t capacity = 0, head = 0, filled = 0;
};

inline int replay_spec_check(const SngReplaySpec *s, std::string *why) {
    auto no = [&](const std::string &msg) {
        if (why) *why = msg;
        return (int)SNG_ERR_INVALID_ARGUMENT;
    };
    if (!s) return no("null replay spec");
    if (s->capacity_days < 1) return no("replay capacity_days " + std::to_string(s->capacity_days) + " must be >= 1");
    if (!s->obs || !s->actions || !s->reward || !s->done) return no("null replay storage");
    return SNG_OK;
}

// SNG_OK, or why a push of `days` days is refused.
inline int replay_push_check(const ReplayRing &r, int32_t days, std::string *why) {
    auto no = [&](const std::string &msg) {
        if (why) *why = msg;
        return (int)SNG_ERR_INVALID_ARGUMENT;
    };
    if (days < 1) return no("replay push: days must be >= 1");
    if (days > r.capacity)
        return no("replay push: " + std::to_string(days) + " days are more than the ring's capacity_days " +
                  std::to_string(r.capacity));
    return SNG_OK;
}

// The slot day d of a push goes to; the ring's state after the push.
inline int32_t replay_slot(const ReplayRing &r, int32_t d) { return (int32_t)(((int64_t)r.head + d) % r.capacity); }
inline ReplayRing replay_pushed(const ReplayRing &r, int32_t days) {
    ReplayRing n = r;
    n.head = replay_slot(r, days);
    n.filled = r.filled + days < r.capacity ? r.filled + days : r.capacity;
    return n;
}
// transitions a sample draws from: filled * T * E
inline uint64_t replay_size(const ReplayRing &r, int32_t T, int64_t E) {
    return (uint64_t)r.filled * (uint64_t)T * (uint64_t)E;
}

// A push is at most two runs of consecutive days into consecutive slots (the second behind the wrap-around); each run
// is one contiguous copy per array.
struct ReplayRun {
    int32_t day0 = 0, slot0 = 0, days = 0;
};
inline int replay_runs(const ReplayRing &r, int32_t days, ReplayRun (&runs)[2]) {
    const int32_t first = days < r.capacity - r.head ? days : r.capacity - r.head;
    runs[0] = {0, r.head, first};
    runs[1] = {first, 0, days - first};
    return days > first ? 2 : 1;
}

// The ring's storage (SngReplaySpec's pointers) and a push's sources.
struct ReplayStorage {
    float *obs = nullptr, *actions = nullptr, *reward = nullptr;
    uint8_t *done = nullptr;
};
struct ReplaySource {
    const float *obs = nullptr, *actions = nullptr;
    const double *reward = nullptr;
    const uint8_t *done = nullptr;
};

// What replay_push_kernel is given: one segment per run and array, `n` elements from src to dst.
enum PushKind : int32_t { PUSH_F32 = 0, PUSH_F64_F32 = 1, PUSH_U8 = 2 };
struct PushSegment {
    const void *src = nullptr;
    void *dst = nullptr;
    int64_t n = 0;
    int32_t kind = PUSH_F32;
};
constexpr int kPushSegments = 8;
struct PushArgs {
    PushSegment seg[kPushSegments];
    int32_t count = 0;
    int64_t longest = 0;   // the most elements of a segment
};
inline PushArgs replay_push_args(const ReplayRing &r, int32_t days, const ReplayStorage &ring, const ReplaySource &src,
                                 int32_t T, int64_t E, int32_t O, int32_t A) {
    PushArgs a;
    ReplayRun runs[2];
    const int nruns = replay_runs(r, days, runs);
    const size_t step = (size_t)T * (size_t)E, obs_day = (size_t)(T + 1) * (size_t)E * (size_t)O,
                 act_day = step * (size_t)A;
    for (int i = 0; i < nruns; ++i) {
        const size_t d0 = (size_t)runs[i].day0, s0 = (size_t)runs[i].slot0, nd = (size_t)runs[i].days;
        const PushSegment segs[4] = {
            {src.obs + d0 * obs_day, ring.obs + s0 * obs_day, (int64_t)(nd * obs_day), PUSH_F32},
            {src.actions + d0 * act_day, ring.actions + s0 * act_day, (int64_t)(nd * act_day), PUSH_F32},
            {src.reward + d0 * step, ring.reward + s0 * step, (int64_t)(nd * step), PUSH_F64_F32},
            {src.done + d0 * step, ring.done + s0 * step, (int64_t)(nd * step), PUSH_U8}};
        for (const PushSegment &s : segs) {
            a.seg[a.count++] = s;
            if (s.n > a.longest) a.longest = s.n;
        }
    }
    return a;
}

// ------------------------------------------------------------------------------------------------ the sampling law
constexpr uint32_t kDomainSample = 0x72730000u;   // apart from kDomainNoise / PV / Price / Ratio / Replay

// What (seed, env offset, counter) give every row of a sample: noise_key's mixes, under the sampler's own domain tag.
SNG_NOISE_HD uint32_t replay_sample_key(uint64_t seed, uint64_t env_offset, uint64_t c) {
    const uint32_t k1 = noise_mix32(noise_day_key(seed, c) ^ (uint32_t)env_offset);
    return noise_mix32(k1 ^ ((uint32_t)(env_offset >> 32) * 0x85ebca6bu + kDomainSample * 0xc2b2ae35u + 0x27d4eb2fu));
}
// Row b's 64 bits: two hashes of the row's own key, in which all 64 bits of b take part.
SNG_NOISE_HD uint64_t replay_sample_bits(uint32_t key, uint64_t b) {
    const uint32_t k1 = noise_mix32(key ^ (uint32_t)b);
    const uint32_t kb = noise_mix32(k1 ^ ((uint32_t)(b >> 32) * 0x85ebca6bu + 0x165667b1u));
    return ((uint64_t)noise_hash(kb, 1u) << 32) | (uint64_t)noise_hash(kb, 2u);
}
// (h * n) >> 64: an index below n, with a bias below n / 2^64
SNG_NOISE_HD uint64_t replay_sample_index(uint64_t h, uint64_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(h, n);
#else
    return (uint64_t)(((unsigned __int128)h * (unsigned __int128)n) >> 64);
#endif
}

inline void replay_host_indices(uint64_t seed, int64_t env_offset, uint64_t counter, uint64_t n, int64_t batch,
                                int64_t *out) {
    const uint32_t key = replay_sample_key(seed, (uint64_t)env_offset, counter);
    for (int64_t b = 0; b < batch; ++b) out[b] = (int64_t)replay_sample_index(replay_sample_bits(key, (uint64_t)b), n);
}

// Transition i of a ring of days of T steps of E envs (TE = T * E): the row of obs [capacity][T + 1][E] that holds its
// observation, i + slot * E (the next observation is E rows further); i itself is its row of actions / reward / done.
SNG_NOISE_HD uint64_t replay_obs_row(uint64_t i, uint64_t TE, uint64_t E) { return i + (i / TE) * E; }

// ------------------------------------------------------------------------------------------------------ the critic
inline SngMlpNetSpec critic_net_spec(int O, int A, const SngCriticSpec &s) {
    return SngMlpNetSpec{O + A, 1, s.hidden1, s.hidden2, s.activation, SNG_MLP_OUT_MEAN, nullptr, nullptr};
}
inline NetImage critic_image(int O, int A, const SngCriticSpec &s) {
    return net_image(O + A, 1, s.hidden1, s.hidden2, s.activation, SNG_MLP_OUT_MEAN, false);
}

// SNG_OK, or the status sng_critic_create and the host entry points return with `why`: net_spec_check's refusals for
// the input width obs_dim + act_dim and one output.
inline int critic_spec_check(const SngCriticSpec *s, int O, int A, std::string *why) {
    auto no = [&](int code, const std::string &msg) {
        if (why) *why = msg;
        return code;
    };
    if (!s) return no(SNG_ERR_INVALID_ARGUMENT, "null critic spec");
    if (O < 1 || A < 1) return no(SNG_ERR_INVALID_ARGUMENT, "critic obs_dim and act_dim must be >= 1");
    if ((int64_t)O + (int64_t)A > 2147483647ll) return no(SNG_ERR_INVALID_ARGUMENT, "critic obs_dim + act_dim overflows");
    const SngMlpNetSpec v = critic_net_spec(O, A, *s);
    std::string inner;
    if (int rc = net_spec_check(&v, 0, 0, &inner))
        return no(rc, "critic Q(s, a), input width obs_dim + act_dim = " + std::to_string(O) + " + " + std::to_string(A) +
                          ": " + inner);
    return SNG_OK;
}
inline int critic_weights_check(int O, int A, const SngCriticSpec &s, const SngMlpWeights *w, std::string *why) {
    return mlp_weights_check(O + A, s.hidden1, s.hidden2, 1, "critic", w, why);
}
inline void critic_pack(const NetImage &m, int O, int A, const SngCriticSpec &s, const SngMlpWeights &w, float *img) {
    net_pack(m, critic_net_spec(O, A, s), w, img);
}

// gamma of a target call: finite and in [0, 1]
inline int critic_gamma_check(double gamma, std::string *why) {
    if (!(gamma >= 0.0 && gamma <= 1.0)) {   // NaN fails both
        if (why) *why = "critic targets: gamma " + std::to_string(gamma) + " must be in [0, 1]";
        return SNG_ERR_INVALID_ARGUMENT;
    }
    return SNG_OK;
}

// Q over `rows` rows: obs [rows][O], actions [rows][A] -> q [rows], mlp_net_host on the concatenated rows, a block of
// rows at a time.
inline void critic_q_host(const NetImage &m, const float *img, int O, int A, int64_t rows, const float *obs,
                          const float *actions, float *q) {
    constexpr int64_t kBlock = 256;
    const size_t K = (size_t)O + (size_t)A;
    std::vector<float> x((size_t)kBlock * K);
    for (int64_t r0 = 0; r0 < rows; r0 += kBlock) {
        const int64_t n = rows - r0 < kBlock ? rows - r0 : kBlock;
        for (int64_t r = 0; r < n; ++r) {
            float *row = x.data() + (size_t)r * K;
            for (int k = 0; k < O; ++k) row[k] = obs[(size_t)(r0 + r) * (size_t)O + (size_t)k];
            for (int k = 0; k < A; ++k) row[O + k] = actions[(size_t)(r0 + r) * (size_t)A + (size_t)k];
        }
        mlp_net_host(m, img, n, x.data(), nullptr, q + r0, nullptr);
    }
}

// SB3's TD3.train target with one critic, in float32, each operation rounded on its own:
//     nn = 1.0f - done;   y = reward + ((nn * g) * q'),   g = (float)gamma
SNG_NOISE_HD float critic_td_target(float reward, float done, float g, float q_next) {
    const float nn = noise_sub(1.0f, done);
    return noise_add(reward, noise_mul(noise_mul(nn, g), q_next));
}

// y [rows] from the target critic's image, next_obs [rows][O], next_actions [rows][A], reward and done [rows]
inline void critic_targets_host(const NetImage &m, const float *img, int O, int A, int64_t rows, const float *next_obs,
                                const float *next_actions, const float *reward, const float *done, double gamma,
                                float *y) {
    critic_q_host(m, img, O, A, rows, next_obs, next_actions, y);
    const float g = (float)gamma;
    for (int64_t r = 0; r < rows; ++r) y[r] = critic_td_target(reward[r], done[r], g, y[r]);
}

// the rows of a launch in workgroups of kNetRows; a grid's x dimension holds 2^31 - 1
constexpr int64_t kCriticMaxBlocks = 2147483647;
inline int64_t critic_blocks(int64_t rows) { return (rows + kNetRows - 1) / kNetRows; }

}  // namespace sng
