// sng_policy_net_host.h -- the MLP actor of any width in host form (include/sng.h, sng_policy_create_net): the
// validation of an SngMlpNetSpec, the packing of its weights into the device image policy_net_kernel reads
// (sng_policy_net.h), the size of that kernel's LDS, and the arithmetic contract on the CPU (mlp_net_host).
// Host only, no HIP: it compiles with plain g++ (tests/native/policy_net_host_check.cpp runs it against a naive
// loop over the unpacked arrays).  Build with -ffp-contract=off, as the library is: the squash stage rounds its
// product and its sum separately.
//
// The contract.  x is an env's observation row, weights are in torch's nn.Linear layout [out][in], and every
// layer's output j is the k-ordered f32 fmaf chain started from the bias, over the layer's real K:
//     h = b[j];  for k = 0 .. K-1:  h = fmaf(in[k], W[j][k], h)
// Hidden layers of hidden1 and hidden2 units with tanh or relu (relu(h) = h > 0 ? h : 0); the output layer gives the
// mean.  SNG_MLP_OUT_MEAN: a = mean (+ noise), env = min(max(a, low), high) where the spec has bounds, else a.
// SNG_MLP_OUT_SQUASH: s = tanh(mean), with noise s = min(max(s + noise, -1), 1), a = s, and
//     env = low[j] + ((0.5f * (s + 1.0f)) * d[j]),  d[j] = high[j] - low[j] computed in f32 when the image is packed,
// which is numpy's float32 evaluation of SB3's unscale_action.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "sng_policy_host.h"

namespace sng {

constexpr int kNetMinWidth = 8, kNetMaxWidth = 512;
constexpr int kNetRows = 64;      // rows of a workgroup: two 32-row tiles
constexpr int kNetTile = 32;      // the MFMA tile: 32 rows x 32 outputs
constexpr int kNetKGroup = 8;     // k's of one weight group: a lane's four dwords are four MFMAs' B operands
constexpr int kNetChunk = 64;     // hidden2 outputs per round: the output layer advances chunk by chunk, in k order
constexpr size_t kNetMaxLds = 160u * 1024u;   // a compute unit's LDS
constexpr int kNetMaxAct = 2 * kNetTile;      // the output layer's width at most: one output tile per wavefront slot

constexpr int net_round_up(int v, int to) { return (v + to - 1) / to * to; }

// The device image, in floats.  A layer with K inputs and N outputs is stored for the MFMA's B operand: KP = K
// rounded up to kNetKGroup and NP = N rounded up to a tile (hidden2: to a chunk), zero-filled, as
//     [tile t < NP / 32][group g < KP / 8][lane l < 64][i < 4]  =  W[j = 32 t + (l & 31)][k = 8 g + 2 i + (l >> 5)]
// so the 64 lanes of a wavefront read one group of a tile as 1 KB in a row, 16 B a lane, and dword i of it is the
// operand B[k = l >> 5][j = l & 31] of the MFMA that takes the chain from k = 8 g + 2 i to 8 g + 2 i + 2.  The padded
// k's follow the real ones (a chain's trailing zero terms); the padded outputs have zero weights and zero biases.
//     w1 | b1 [N1] | w2 | b2 [N2] | w3 | b3 [N3] | low [N3] | high [N3] | span [N3] (high - low)
struct NetImage {
    int32_t O = 0, A = 0, H1 = 0, H2 = 0;
    int32_t K1 = 0, N1 = 0, K2 = 0, N2 = 0, K3 = 0, N3 = 0;
    int32_t activation = POLICY_TANH, output = SNG_MLP_OUT_MEAN, clip = 0;
    size_t w1 = 0, b1 = 0, w2 = 0, b2 = 0, w3 = 0, b3 = 0, low = 0, high = 0, span = 0, floats = 0;
};

// where W[j][k] of a layer padded to KP inputs sits in the layer's block
inline size_t net_weight_at(int KP, int j, int k) {
    const size_t t = (size_t)(j / kNetTile), g = (size_t)(k / kNetKGroup);
    const size_t lane = (size_t)((k & 1) * 32 + (j & 31)), i = (size_t)((k & 7) >> 1);
    return ((t * (size_t)(KP / kNetKGroup) + g) * 64 + lane) * 4 + i;
}

inline NetImage net_image(int O, int A, int H1, int H2, int activation, int output, bool clip) {
    NetImage m;
    m.O = O;
    m.A = A;
    m.H1 = H1;
    m.H2 = H2;
    m.K1 = net_round_up(O, kNetKGroup);
    m.N1 = net_round_up(H1, kNetTile);
    m.K2 = net_round_up(H1, kNetKGroup);
    m.N2 = net_round_up(H2, kNetChunk);
    m.K3 = net_round_up(H2, kNetKGroup);
    m.N3 = net_round_up(A, kNetTile);
    m.activation = activation;
    m.output = output;
    m.clip = clip ? 1 : 0;
    size_t at = 0;
    auto take = [&](size_t n) {
        const size_t o = at;
        at += n;
        return o;
    };
    m.w1 = take((size_t)m.K1 * (size_t)m.N1);
    m.b1 = take((size_t)m.N1);
    m.w2 = take((size_t)m.K2 * (size_t)m.N2);
    m.b2 = take((size_t)m.N2);
    m.w3 = take((size_t)m.K3 * (size_t)m.N3);
    m.b3 = take((size_t)m.N3);
    m.low = take((size_t)m.N3);
    m.high = take((size_t)m.N3);
    m.span = take((size_t)m.N3);
    m.floats = at;
    return m;
}

// policy_net_kernel's LDS, in floats: hidden1's rows [64][N1 + 1], and one region that holds the observation rows
// [64][K1 + 1] first and a chunk of hidden2's rows [64][kNetChunk + 1] afterwards.  The row strides are odd, so the
// 32 rows an MFMA's A operand reads at one k differ in bank.
constexpr int net_lds_h1_stride(int N1) { return N1 + 1; }
constexpr int net_lds_obs_stride(int K1) { return K1 + 1; }
constexpr int net_lds_chunk_stride() { return kNetChunk + 1; }
inline int net_lds_h1(const NetImage &m) { return kNetRows * net_lds_h1_stride(m.N1); }
inline int net_lds_shared(const NetImage &m) {
    const int a = net_lds_obs_stride(m.K1), b = net_lds_chunk_stride();
    return kNetRows * (a > b ? a : b);
}
inline size_t net_lds_bytes(const NetImage &m) { return (size_t)(net_lds_h1(m) + net_lds_shared(m)) * sizeof(float); }

// SNG_OK, or the status sng_policy_create_net returns with `why`.  obs_dim / act_dim: the env's, or 0 for a
// host-only call that has no env to match.
inline int net_spec_check(const SngMlpNetSpec *s, int obs_dim, int act_dim, std::string *why) {
    auto no = [&](int code, const std::string &msg) {
        if (why) *why = msg;
        return code;
    };
    if (!s) return no(SNG_ERR_INVALID_ARGUMENT, "null policy spec");
    if (s->obs_dim < 1 || s->act_dim < 1) return no(SNG_ERR_INVALID_ARGUMENT, "policy obs_dim and act_dim must be >= 1");
    if ((obs_dim && s->obs_dim != obs_dim) || (act_dim && s->act_dim != act_dim))
        return no(SNG_ERR_INVALID_ARGUMENT, "policy obs_dim / act_dim differ from the env's");
    if (s->hidden1 < kNetMinWidth || s->hidden1 > kNetMaxWidth || s->hidden2 < kNetMinWidth || s->hidden2 > kNetMaxWidth)
        return no(SNG_ERR_UNSUPPORTED, "the MLP actor's hidden widths must be 8 .. 512");
    if (s->activation != POLICY_TANH && s->activation != POLICY_RELU)
        return no(SNG_ERR_INVALID_ARGUMENT, "policy activation must be 0 (tanh) or 1 (relu)");
    if (s->output != SNG_MLP_OUT_MEAN && s->output != SNG_MLP_OUT_SQUASH)
        return no(SNG_ERR_INVALID_ARGUMENT, "policy output must be SNG_MLP_OUT_MEAN or SNG_MLP_OUT_SQUASH");
    if ((s->low == nullptr) != (s->high == nullptr))
        return no(SNG_ERR_INVALID_ARGUMENT, "policy bounds: give both or neither");
    if (s->output == SNG_MLP_OUT_SQUASH && !s->low)
        return no(SNG_ERR_INVALID_ARGUMENT, "a squashed output needs the action Box (low, high)");
    if (s->low)
        for (int j = 0; j < s->act_dim; ++j) {
            if (std::isnan(s->low[j]) || std::isnan(s->high[j]) || s->low[j] > s->high[j])
                return no(SNG_ERR_INVALID_ARGUMENT, "policy bounds must be ordered numbers");
            if (s->output == SNG_MLP_OUT_SQUASH && (!std::isfinite(s->low[j]) || !std::isfinite(s->high[j])))
                return no(SNG_ERR_INVALID_ARGUMENT, "a squashed output needs a finite action Box");
        }
    // policy_net_kernel keeps one output tile per wavefront slot, two tiles in all: stations of up to 63 chargers with
    // a BESS, 64 without.  The host model is held to the same limit, so that the two accept the same specs.
    if (s->act_dim > kNetMaxAct)
        return no(SNG_ERR_UNSUPPORTED, "the MLP actor's act_dim " + std::to_string(s->act_dim) + " is above " +
                                           std::to_string(kNetMaxAct) + ", the two output tiles of policy_net_kernel");
    // obs_dim is bounded by the LDS check below; this keeps its arithmetic in range
    if ((size_t)s->obs_dim > kNetMaxLds / (kNetRows * sizeof(float)))
        return no(SNG_ERR_UNSUPPORTED, "the MLP actor's LDS tiles do not fit a compute unit: obs_dim " +
                                           std::to_string(s->obs_dim) + " alone needs more than " +
                                           std::to_string(kNetMaxLds) + " B");
    const NetImage m = net_image(s->obs_dim, s->act_dim, s->hidden1, s->hidden2, s->activation, s->output, s->low != nullptr);
    if (net_lds_bytes(m) > kNetMaxLds)
        return no(SNG_ERR_UNSUPPORTED,
                  "the MLP actor's LDS tiles do not fit a compute unit: obs_dim " + std::to_string(s->obs_dim) +
                      ", hidden " + std::to_string(s->hidden1) + "-" + std::to_string(s->hidden2) + " need " +
                      std::to_string(net_lds_bytes(m)) + " B of " + std::to_string(kNetMaxLds));
    return SNG_OK;
}

// Non-finite weights are refused at upload.
inline int net_weights_check(const SngMlpNetSpec &s, const SngMlpWeights *w, std::string *why) {
    return mlp_weights_check(s.obs_dim, s.hidden1, s.hidden2, s.act_dim, "policy", w, why);
}

// The weights and the spec's bounds into `img` (NetImage::floats floats).
inline void net_pack(const NetImage &m, const SngMlpNetSpec &s, const SngMlpWeights &w, float *img) {
    for (size_t i = 0; i < m.floats; ++i) img[i] = 0.f;
    for (int j = 0; j < m.H1; ++j)
        for (int k = 0; k < m.O; ++k) img[m.w1 + net_weight_at(m.K1, j, k)] = w.w1[(size_t)j * m.O + k];
    for (int j = 0; j < m.H2; ++j)
        for (int k = 0; k < m.H1; ++k) img[m.w2 + net_weight_at(m.K2, j, k)] = w.w2[(size_t)j * m.H1 + k];
    for (int j = 0; j < m.A; ++j)
        for (int k = 0; k < m.H2; ++k) img[m.w3 + net_weight_at(m.K3, j, k)] = w.w3[(size_t)j * m.H2 + k];
    for (int j = 0; j < m.H1; ++j) img[m.b1 + j] = w.b1[j];
    for (int j = 0; j < m.H2; ++j) img[m.b2 + j] = w.b2[j];
    for (int j = 0; j < m.A; ++j) {
        img[m.b3 + j] = w.b3[j];
        if (s.low) {
            img[m.low + j] = s.low[j];
            img[m.high + j] = s.high[j];
            img[m.span + j] = s.high[j] - s.low[j];
        }
    }
}

// SB3's unscale_action in float32, as numpy evaluates low + (0.5 * (s + 1.0) * (high - low)): span = high - low
inline float net_unscale(float s, float low, float span) {
    const float half = 0.5f * (s + 1.0f);
    const float prod = half * span;
    return low + prod;
}

// One row's output stage: the mean (and the noise, where has_noise) to a and the env action.
inline void net_output(const NetImage &m, const float *img, int j, float mean, bool has_noise, float noise, float *a,
                       float *env) {
    if (m.output == SNG_MLP_OUT_SQUASH) {
        float s = std::tanh(mean);
        if (has_noise) s = policy_clip(s + noise, -1.f, 1.f);
        *a = s;
        *env = net_unscale(s, img[m.low + j], img[m.span + j]);
    } else {
        const float v = has_noise ? mean + noise : mean;
        *a = v;
        *env = m.clip ? policy_clip(v, img[m.low + j], img[m.high + j]) : v;
    }
}

// The contract, on the packed image and over the real K of every chain: `rows` observation rows [rows][O] ->
// actions [rows][A] (a) and, where env_actions is given, the actions the env is stepped with.  noise [rows][A] may
// be null.
inline void mlp_net_host(const NetImage &m, const float *img, int64_t rows, const float *obs, const float *noise,
                         float *actions, float *env_actions) {
    const size_t w[3] = {m.w1, m.w2, m.w3};
    const int KP[3] = {m.K1, m.K2, m.K3};
    mlp_forward_host(
        m.O, m.H1, m.H2, m.A, m.activation, img, {m.b1, m.b2, m.b3},
        [&](int l, int j, int k) { return w[l] + net_weight_at(KP[l], j, k); }, rows, obs, [&](int64_t r, int j, float mean) {
            const size_t at = (size_t)r * (size_t)m.A + (size_t)j;
            float a, env;
            net_output(m, img, j, mean, noise != nullptr, noise ? noise[at] : 0.f, &a, &env);
            actions[at] = a;
            if (env_actions) env_actions[at] = env;
        });
}

}  // namespace sng
