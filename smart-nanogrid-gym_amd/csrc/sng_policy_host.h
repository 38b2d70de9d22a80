// sng_policy_host.h -- the MLP actor in host form: the validation of an SngMlpSpec, the packing of its weights
// into the device image the policy kernels read (sng_policy.h), and the actor's arithmetic contract on the CPU
// (mlp_actor_host), which the kernels reproduce bit for bit with relu and up to the device's tanhf with tanh.
// Host only, no HIP: it compiles with plain g++ (tests/native/policy_host_check.cpp runs it against a naive loop).
//
// The contract (include/sng.h, sng_policy_create).  x is an env's observation row, weights are in torch's
// nn.Linear layout [out][in], and every layer's output j is the k-ordered f32 fmaf chain started from the bias:
//     h = b[j];  for k = 0 .. K-1:  h = fmaf(in[k], W[j][k], h)
// Two hidden layers of kPolicyHidden units with tanh or relu (relu(h) = h > 0 ? h : 0), an output layer without
// activation (the mean), a = mean + noise (one f32 add) when noise is given, and the env is stepped with
// min(max(a, low), high) when the spec has clip bounds, else with a.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sng.h"

namespace sng {

constexpr int kPolicyHidden = 64;
constexpr int kPolicyOutChunk = 16;   // the output layer's accumulators per pass (sng_policy.h): A is padded to it
enum PolicyActivation : int { POLICY_TANH = 0, POLICY_RELU = 1 };

// The device image, in floats.  The weights are stored transposed ([in][out]): the kernels walk k in the outer
// loop and read one k's row of weights as a wave-uniform run.  The output layer's width is padded to a multiple
// of kPolicyOutChunk with zero weights, zero biases and zero bounds; a padded output is computed and never stored.
//     w1t [O][64] | b1 [64] | w2t [64][64] | b2 [64] | w3t [64][AP] | b3 [AP] | low [AP] | high [AP]
struct PolicyImage {
    int32_t O = 0, A = 0, AP = 0;
    int32_t activation = POLICY_TANH, clip = 0;
    size_t w1t = 0, b1 = 0, w2t = 0, b2 = 0, w3t = 0, b3 = 0, low = 0, high = 0, floats = 0;
};

inline PolicyImage policy_image(int O, int A, int activation, bool clip) {
    constexpr size_t H = kPolicyHidden;
    PolicyImage m;
    m.O = O;
    m.A = A;
    m.AP = (A + kPolicyOutChunk - 1) / kPolicyOutChunk * kPolicyOutChunk;
    m.activation = activation;
    m.clip = clip ? 1 : 0;
    size_t at = 0;
    auto take = [&](size_t n) {
        const size_t o = at;
        at += n;
        return o;
    };
    m.w1t = take((size_t)O * H);
    m.b1 = take(H);
    m.w2t = take(H * H);
    m.b2 = take(H);
    m.w3t = take(H * (size_t)m.AP);
    m.b3 = take((size_t)m.AP);
    m.low = take((size_t)m.AP);
    m.high = take((size_t)m.AP);
    m.floats = at;
    return m;
}

// SNG_OK, or the status sng_policy_create returns with `why`: other widths than 64 are unsupported (the depth is
// fixed by SngMlpWeights), everything else that is off is an invalid argument.  obs_dim / act_dim: the env's, or
// 0 for a host-only call that has no env to match.
inline int policy_spec_check(const SngMlpSpec *s, int obs_dim, int act_dim, std::string *why) {
    auto no = [&](int code, const char *msg) {
        if (why) *why = msg;
        return code;
    };
    if (!s) return no(SNG_ERR_INVALID_ARGUMENT, "null policy spec");
    if (s->obs_dim < 1 || s->act_dim < 1) return no(SNG_ERR_INVALID_ARGUMENT, "policy obs_dim and act_dim must be >= 1");
    if ((obs_dim && s->obs_dim != obs_dim) || (act_dim && s->act_dim != act_dim))
        return no(SNG_ERR_INVALID_ARGUMENT, "policy obs_dim / act_dim differ from the env's");
    if (s->hidden != kPolicyHidden) return no(SNG_ERR_UNSUPPORTED, "the MLP actor has two hidden layers of 64 units");
    if (s->activation != POLICY_TANH && s->activation != POLICY_RELU)
        return no(SNG_ERR_INVALID_ARGUMENT, "policy activation must be 0 (tanh) or 1 (relu)");
    if ((s->clip_low == nullptr) != (s->clip_high == nullptr))
        return no(SNG_ERR_INVALID_ARGUMENT, "policy clip bounds: give both or neither");
    if (s->clip_low)
        for (int j = 0; j < s->act_dim; ++j)
            if (std::isnan(s->clip_low[j]) || std::isnan(s->clip_high[j]) || s->clip_low[j] > s->clip_high[j])
                return no(SNG_ERR_INVALID_ARGUMENT, "policy clip bounds must be ordered numbers");
    return SNG_OK;
}

// Non-finite weights are refused at upload: the six arrays of a net of O inputs, hidden widths H1 and H2 and A outputs.
// `what` names them in the message: "policy", or "value net" for a PPO head's (sng_ppo_host.h).
inline int mlp_weights_check(int O, int H1, int H2, int A, const char *what, const SngMlpWeights *w, std::string *why) {
    auto no = [&](const std::string &msg) {
        if (why) *why = msg;
        return (int)SNG_ERR_INVALID_ARGUMENT;
    };
    if (!w || !w->w1 || !w->b1 || !w->w2 || !w->b2 || !w->w3 || !w->b3) return no(std::string("null ") + what + " weights");
    const size_t n1 = (size_t)H1, n2 = (size_t)H2, n3 = (size_t)A;
    const struct {
        const float *v;
        size_t n;
    } parts[] = {{w->w1, n1 * (size_t)O}, {w->b1, n1}, {w->w2, n2 * n1}, {w->b2, n2}, {w->w3, n3 * n2}, {w->b3, n3}};
    for (const auto &part : parts)
        for (size_t i = 0; i < part.n; ++i)
            if (!std::isfinite(part.v[i])) return no(std::string("non-finite ") + what + " weight");
    return SNG_OK;
}
inline int policy_weights_check(const SngMlpSpec &s, const SngMlpWeights *w, std::string *why) {
    return mlp_weights_check(s.obs_dim, kPolicyHidden, kPolicyHidden, s.act_dim, "policy", w, why);
}

// The weights and the spec's clip bounds into `img` (PolicyImage::floats floats).
inline void policy_pack(const PolicyImage &m, const SngMlpSpec &s, const SngMlpWeights &w, float *img) {
    constexpr int H = kPolicyHidden;
    for (size_t i = 0; i < m.floats; ++i) img[i] = 0.f;
    for (int k = 0; k < m.O; ++k)
        for (int j = 0; j < H; ++j) img[m.w1t + (size_t)k * H + j] = w.w1[(size_t)j * m.O + k];
    for (int k = 0; k < H; ++k)
        for (int j = 0; j < H; ++j) img[m.w2t + (size_t)k * H + j] = w.w2[(size_t)j * H + k];
    for (int k = 0; k < H; ++k)
        for (int j = 0; j < m.A; ++j) img[m.w3t + (size_t)k * m.AP + j] = w.w3[(size_t)j * H + k];
    for (int j = 0; j < H; ++j) {
        img[m.b1 + j] = w.b1[j];
        img[m.b2 + j] = w.b2[j];
    }
    for (int j = 0; j < m.A; ++j) {
        img[m.b3 + j] = w.b3[j];
        if (m.clip) {
            img[m.low + j] = s.clip_low[j];
            img[m.high + j] = s.clip_high[j];
        }
    }
}

inline float policy_activate(int activation, float h) {
    return activation == POLICY_RELU ? (h > 0.f ? h : 0.f) : std::tanh(h);
}

// min(max(a, low), high), spelt as the kernels spell it
inline float policy_clip(float a, float low, float high) {
    const float c = a < low ? low : a;
    return high < c ? high : c;
}

// The contract's three layers over `rows` observation rows [rows][O], on a packed image: every output is the chain
// from its bias over the layer's k = 0 .. K-1 in order, one fmaf and so one rounding a term.  bias[l]: where layer
// l's biases begin in img; at(l, j, k): where its W[j][k] is (the two images differ in nothing else).  Row r's output
// layer goes to out(r, j, mean).
template <class WeightAt, class Output>
inline void mlp_forward_host(int O, int H1, int H2, int A, int activation, const float *img, const size_t (&bias)[3],
                             WeightAt at, int64_t rows, const float *obs, Output out) {
    std::vector<float> h1((size_t)H1), h2((size_t)H2);
    for (int64_t r = 0; r < rows; ++r) {
        const float *x = obs + (size_t)r * (size_t)O;
        for (int j = 0; j < H1; ++j) {
            float h = img[bias[0] + j];
            for (int k = 0; k < O; ++k) h = std::fmaf(x[k], img[at(0, j, k)], h);
            h1[j] = policy_activate(activation, h);
        }
        for (int j = 0; j < H2; ++j) {
            float h = img[bias[1] + j];
            for (int k = 0; k < H1; ++k) h = std::fmaf(h1[k], img[at(1, j, k)], h);
            h2[j] = policy_activate(activation, h);
        }
        for (int j = 0; j < A; ++j) {
            float h = img[bias[2] + j];
            for (int k = 0; k < H2; ++k) h = std::fmaf(h2[k], img[at(2, j, k)], h);
            out(r, j, h);
        }
    }
}

// The contract, on the packed image: `rows` observation rows [rows][O] -> actions [rows][A] (a) and, where
// env_actions is given, the actions the env is stepped with.  noise [rows][A] may be null.
inline void mlp_actor_host(const PolicyImage &m, const float *img, int64_t rows, const float *obs, const float *noise,
                           float *actions, float *env_actions) {
    constexpr int H = kPolicyHidden;
    const size_t w[3] = {m.w1t, m.w2t, m.w3t}, ld[3] = {(size_t)H, (size_t)H, (size_t)m.AP};   // [in][out]
    mlp_forward_host(
        m.O, H, H, m.A, m.activation, img, {m.b1, m.b2, m.b3}, [&](int l, int j, int k) { return w[l] + (size_t)k * ld[l] + j; },
        rows, obs, [&](int64_t r, int j, float mean) {
            const size_t at = (size_t)r * (size_t)m.A + (size_t)j;
            const float a = noise ? mean + noise[at] : mean;
            actions[at] = a;
            if (env_actions) env_actions[at] = m.clip ? policy_clip(a, img[m.low + j], img[m.high + j]) : a;
        });
}

}  // namespace sng
