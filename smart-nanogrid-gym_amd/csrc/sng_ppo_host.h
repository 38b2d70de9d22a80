// sng_ppo_host.h -- what finishes a PPO rollout, in host form: the device image of the value net and the Gaussian
// head's log_std (PpoImage), the checks of the sng_ppo_* calls, and the contract's arithmetic on the CPU
// (ppo_values_host, ppo_gae_host, ppo_logp_host), which rollout_gae_kernel (sng_ppo.h) reproduces bit for bit with
// relu and up to the device's tanhf with tanh.  Host only, no HIP: it compiles with plain g++
// (tests/native/ppo_host_check.cpp runs it against naive loops).
//
// The contract (include/sng.h, sng_ppo_create).  The value net is SngMlpSpec's arithmetic with act_dim = 1, no noise
// and no clip: its host model is mlp_actor_host on policy_image(O, 1, activation, false), and V is the output
// layer's one chain.  The advantages are numpy's float32 evaluation of SB3's compute_returns_and_advantage and the
// log-probability is DiagGaussianDistribution's of the noise the actor added; every operation of both is rounded on
// its own (this header must be compiled with -ffp-contract=off, as the library and its tests are).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "sng.h"
#include "sng_policy_host.h"

namespace sng {

constexpr float kHalfLog2Pi = 0.91893853f;   // 0.5 log(2 pi), float32
constexpr int32_t kPpoMaxLaunchDays = 65535;   // sng_ppo_finish: the days are the y dimension of one launch's grid

// The Gaussian head's part of a head's device image: log_std and inv_std = 1 / exp(log_std), each padded to a
// multiple of kPolicyOutChunk with zeros, behind the value net's image.  inv_std is computed once, on the host, when the
// image is packed: the device never calls expf, and host and device read the same words.
struct GaussHead {
    int32_t A = 0, AP = 0;
    size_t log_std = 0, inv_std = 0;
};

// the head laid out from float `at` of an image on; *floats: the image's size with it
inline GaussHead gauss_head(int A, size_t at, size_t *floats) {
    GaussHead h;
    h.A = A;
    h.AP = (A + kPolicyOutChunk - 1) / kPolicyOutChunk * kPolicyOutChunk;
    h.log_std = at;
    h.inv_std = h.log_std + (size_t)h.AP;
    *floats = h.inv_std + (size_t)h.AP;
    return h;
}

// The device image, in floats: the value net's PolicyImage (A = 1), then the Gaussian head.
struct PpoImage {
    PolicyImage v;
    GaussHead head;
    size_t floats = 0;
};

inline PpoImage ppo_image(int O, int A, int activation) {
    PpoImage m;
    m.v = policy_image(O, 1, activation, false);
    m.head = gauss_head(A, m.v.floats, &m.floats);
    return m;
}

inline SngMlpSpec ppo_value_spec(int O, int activation) { return SngMlpSpec{O, 1, kPolicyHidden, activation, nullptr, nullptr}; }

// SNG_OK, or SNG_ERR_INVALID_ARGUMENT with `why`: the dims and the activation of a head.
inline int ppo_dims_check(int O, int A, int activation, std::string *why) {
    auto no = [&](const char *msg) {
        if (why) *why = msg;
        return (int)SNG_ERR_INVALID_ARGUMENT;
    };
    if (O < 1 || A < 1) return no("ppo obs_dim and act_dim must be >= 1");
    if (activation != POLICY_TANH && activation != POLICY_RELU) return no("ppo activation must be 0 (tanh) or 1 (relu)");
    return SNG_OK;
}

// A non-finite log_std is refused (null: zeros).
inline int ppo_log_std_check(int A, const float *log_std, std::string *why) {
    if (log_std)
        for (int j = 0; j < A; ++j)
            if (!std::isfinite(log_std[j])) {
                if (why) *why = "non-finite log_std";
                return SNG_ERR_INVALID_ARGUMENT;
            }
    return SNG_OK;
}

// The value net's weights as mlp_weights_check refuses them, and log_std.
inline int ppo_weights_check(int O, int A, int /*activation*/, const SngMlpWeights *w, const float *log_std, std::string *why) {
    if (int rc = mlp_weights_check(O, kPolicyHidden, kPolicyHidden, 1, "value net", w, why)) return rc;
    return ppo_log_std_check(A, log_std, why);
}

// The image of a head without a value net (zero weights), `floats` floats: for a caller that brings its own values.
inline void ppo_pack_log_std(const GaussHead &m, size_t floats, const float *log_std, float *img) {
    for (size_t i = 0; i < floats; ++i) img[i] = 0.f;
    for (int j = 0; j < m.A; ++j) {
        const float ls = log_std ? log_std[j] : 0.f;
        img[m.log_std + j] = ls;
        img[m.inv_std + j] = 1.0f / std::exp(ls);
    }
}

// The value net and log_std (null: zeros, SB3's log_std_init) into `img` (PpoImage::floats floats).
inline void ppo_pack(const PpoImage &m, const SngMlpWeights &w, const float *log_std, float *img) {
    ppo_pack_log_std(m.head, m.floats, log_std, img);
    policy_pack(m.v, ppo_value_spec(m.v.O, m.v.activation), w, img);
}

// What sng_ppo_finish and sng_ppo_host_finish refuse in a rollout, whatever memory its pointers name.
// need_obs: the values are computed (from obs), not given.
inline int ppo_rollout_check(const SngPpoRollout *r, bool need_obs, std::string *why) {
    auto no = [&](const char *msg) {
        if (why) *why = msg;
        return (int)SNG_ERR_INVALID_ARGUMENT;
    };
    if (!r) return no("null ppo rollout");
    if (r->days < 1) return no("ppo rollout: days must be >= 1");
    if (!(r->gamma >= 0.0 && r->gamma <= 1.0)) return no("ppo rollout: gamma must be in [0, 1]");
    if (!(r->gae_lambda >= 0.0 && r->gae_lambda <= 1.0)) return no("ppo rollout: gae_lambda must be in [0, 1]");
    if (!r->reward || !r->done || !r->values || !r->advantages || !r->returns || (need_obs && !r->obs))
        return no("ppo rollout: null obs, reward, done, values, advantages or returns");
    return SNG_OK;
}

// gamma and gamma * lambda as the recurrence takes them: float32, the product formed in double
inline float ppo_gamma_f32(double gamma) { return (float)gamma; }
inline float ppo_gamma_lambda_f32(double gamma, double gae_lambda) { return (float)(gamma * gae_lambda); }

// One step of the recurrence: `gae` in, the step's advantage out (the new gae); *ret = advantage + v.
inline float ppo_gae_step(float g, float gl, float r, float nn, float v, float v_next, float gae, float *ret) {
    const float delta = (r + ((g * v_next) * nn)) - v;
    const float a = delta + ((gl * nn) * gae);
    *ret = a + v;
    return a;
}

// values [days][T + 1][E] -> advantages, returns [days][T][E], per env and per day, walking t = T - 1 .. 0.
inline void ppo_gae_host(int32_t days, int32_t T, int64_t E, double gamma, double gae_lambda, const double *reward,
                         const uint8_t *done, const float *values, float *advantages, float *returns) {
    const float g = ppo_gamma_f32(gamma), gl = ppo_gamma_lambda_f32(gamma, gae_lambda);
    for (int32_t d = 0; d < days; ++d)
        for (int64_t e = 0; e < E; ++e) {
            float gae = 0.0f;
            for (int32_t t = T - 1; t >= 0; --t) {
                const size_t at = ((size_t)d * (size_t)T + (size_t)t) * (size_t)E + (size_t)e;
                const size_t vt = ((size_t)d * (size_t)(T + 1) + (size_t)t) * (size_t)E + (size_t)e;
                const float nn = 1.0f - (float)done[at];
                gae = ppo_gae_step(g, gl, (float)reward[at], nn, values[vt], values[vt + (size_t)E], gae, &returns[at]);
                advantages[at] = gae;
            }
        }
}

// One row's log-probability: `noise` [A] under N(0, exp(log_std)), in j order.
inline float ppo_logp_row(const GaussHead &m, const float *img, const float *noise) {
    float lp = 0.0f;
    for (int j = 0; j < m.A; ++j) {
        const float z = noise[j] * img[m.inv_std + j];
        const float term = (((-0.5f * z) * z) - img[m.log_std + j]) - kHalfLog2Pi;
        lp = lp + term;
    }
    return lp;
}

// noise [T][E][A], reused every day -> logp [days][T][E]
inline void ppo_logp_host(const GaussHead &m, const float *img, int32_t days, int32_t T, int64_t E, const float *noise,
                          float *logp) {
    const size_t rows = (size_t)T * (size_t)E;
    for (int32_t d = 0; d < days; ++d)
        for (size_t r = 0; r < rows; ++r) logp[(size_t)d * rows + r] = ppo_logp_row(m, img, noise + r * (size_t)m.A);
}

// obs [days][T + 1][E][O] -> values [days][T + 1][E]: mlp_actor_host with one action, no noise and no clip
inline void ppo_values_host(const PpoImage &m, const float *img, int32_t days, int32_t T, int64_t E, const float *obs,
                            float *values) {
    mlp_actor_host(m.v, img, (int64_t)days * (int64_t)(T + 1) * E, obs, nullptr, values, nullptr);
}

}  // namespace sng
