// The PPO head's host model (csrc/sng_ppo_host.h) against naive evaluations written here, bitwise
// (tests/test_ppo_rollout_cpu.py builds this with plain g++, -ffp-contract=off, -Wall -Werror and no ROCm on the
// include path).  The naive GAE walks one env at a time over plain arrays with every intermediate in a volatile
// float, the naive log-probability reads log_std and recomputes 1 / exp itself, and the value path is held against
// mlp_actor_host on an image packed for act_dim = 1 and against a naive chain over the unpacked arrays.
// Cases: O in {5, 25, 109} x A in {2, 9, 51} x relu / tanh x T in {12, 24} x E = 7 x days = 2.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sng_ppo_host.h"

using namespace sng;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform01() {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}
static float uniform(float lo, float hi) { return (float)(lo + (hi - lo) * uniform01()); }
static std::vector<float> fill(size_t n, float bound) {
    std::vector<float> v(n);
    for (float &x : v) x = uniform(-bound, bound);
    return v;
}
static float act(int activation, float h) { return activation == 1 ? (h > 0.f ? h : 0.f) : std::tanh(h); }
static float chain(const float *in, const float *w_row, int K, float bias) {
    float h = bias;
    for (int k = 0; k < K; ++k) h = std::fmaf(in[k], w_row[k], h);
    return h;
}
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main() {
    const int Os[] = {5, 25, 109}, As[] = {2, 9, 51}, Ts[] = {12, 24};
    const int H = 64, days = 2;
    const int64_t E = 7;
    const double gamma = 0.99, lambda = 0.95;
    long checked = 0;
    for (int O : Os)
        for (int A : As)
            for (int activation = 0; activation < 2; ++activation)
                for (int T : Ts) {
                    const auto w1 = fill((size_t)H * O, 1.f / std::sqrt((float)O)), b1 = fill(H, 0.3f);
                    const auto w2 = fill((size_t)H * H, 0.125f), b2 = fill(H, 0.3f);
                    const auto w3 = fill(H, 0.5f), b3 = fill(1, 0.3f);
                    const auto log_std = fill(A, 1.2f);
                    const size_t rows = (size_t)days * (T + 1) * E, steps = (size_t)days * T * E;
                    const auto obs = fill(rows * O, 1.f), noise = fill((size_t)T * E * A, 1.5f);
                    std::vector<double> reward(steps);
                    std::vector<uint8_t> done(steps);
                    for (size_t i = 0; i < steps; ++i) {
                        reward[i] = -30.0 * uniform01();
                        done[i] = uniform01() < 0.25 ? 1 : 0;
                    }
                    const SngMlpWeights w{w1.data(), b1.data(), w2.data(), b2.data(), w3.data(), b3.data()};
                    std::string why;
                    if (ppo_dims_check(O, A, activation, &why) != SNG_OK ||
                        ppo_weights_check(O, A, activation, &w, log_std.data(), &why) != SNG_OK) {
                        printf("refused: %s\n", why.c_str());
                        return 1;
                    }
                    const PpoImage m = ppo_image(O, A, activation);
                    std::vector<float> img(m.floats), values(rows), adv(steps), ret(steps), logp(steps);
                    ppo_pack(m, w, log_std.data(), img.data());
                    ppo_values_host(m, img.data(), days, T, E, obs.data(), values.data());
                    ppo_gae_host(days, T, E, gamma, lambda, reward.data(), done.data(), values.data(), adv.data(), ret.data());
                    ppo_logp_host(m.head, img.data(), days, T, E, noise.data(), logp.data());
                    // the value path: mlp_actor_host with A = 1 on an image of its own, and a naive chain
                    {
                        const SngMlpSpec spec{O, 1, H, activation, nullptr, nullptr};
                        const PolicyImage pm = policy_image(O, 1, activation, false);
                        std::vector<float> pimg(pm.floats), v2(rows);
                        policy_pack(pm, spec, w, pimg.data());
                        mlp_actor_host(pm, pimg.data(), (int64_t)rows, obs.data(), nullptr, v2.data(), nullptr);
                        for (size_t r = 0; r < rows; ++r) {
                            float h1[64], h2[64];
                            for (int j = 0; j < H; ++j) h1[j] = act(activation, chain(&obs[r * O], &w1[(size_t)j * O], O, b1[j]));
                            for (int j = 0; j < H; ++j) h2[j] = act(activation, chain(h1, &w2[(size_t)j * H], H, b2[j]));
                            const float want = chain(h2, w3.data(), H, b3[0]);
                            if (!same(values[r], v2[r]) || !same(values[r], want)) {
                                printf("value mismatch O=%d act=%d row %zu: %a %a %a\n", O, activation, r, values[r], v2[r], want);
                                return 1;
                            }
                            ++checked;
                        }
                    }
                    // GAE, one env at a time
                    const float g = (float)gamma, gl = (float)(gamma * lambda);
                    for (int d = 0; d < days; ++d)
                        for (int64_t e = 0; e < E; ++e) {
                            volatile float gae = 0.0f;
                            for (int t = T - 1; t >= 0; --t) {
                                const size_t at = ((size_t)d * T + t) * E + e, vt = ((size_t)d * (T + 1) + t) * E + e;
                                volatile float nn = 1.0f - (float)done[at];
                                volatile float x = g * values[vt + E];
                                x = x * nn;
                                x = (float)reward[at] + x;
                                volatile float delta = x - values[vt];
                                volatile float y = gl * nn;
                                y = y * gae;
                                gae = delta + y;
                                volatile float rr = gae + values[vt];
                                if (!same(adv[at], gae) || !same(ret[at], rr)) {
                                    printf("gae mismatch T=%d d=%d t=%d e=%d: %a %a, want %a %a\n", T, d, t, (int)e, adv[at],
                                           ret[at], (float)gae, (float)rr);
                                    return 1;
                                }
                                checked += 2;
                            }
                        }
                    // log-probability, from log_std itself
                    for (int d = 0; d < days; ++d)
                        for (size_t r = 0; r < (size_t)T * E; ++r) {
                            volatile float lp = 0.0f;
                            for (int j = 0; j < A; ++j) {
                                volatile float inv = 1.0f / std::exp(log_std[j]);
                                volatile float z = noise[r * A + j] * inv;
                                volatile float q = -0.5f * z;
                                q = q * z;
                                q = q - log_std[j];
                                q = q - 0.91893853f;
                                lp = lp + q;
                            }
                            if (!same(logp[(size_t)d * T * E + r], lp)) {
                                printf("logp mismatch A=%d d=%d row %zu: %a, want %a\n", A, d, r, logp[(size_t)d * T * E + r], (float)lp);
                                return 1;
                            }
                            ++checked;
                        }
                    // the image's padding is zero
                    for (int j = A; j < m.head.AP; ++j)
                        if (img[m.head.log_std + j] != 0.f || img[m.head.inv_std + j] != 0.f) return 2;
                }
    // validation
    {
        auto w1 = fill(64 * 11, 1.f), b = fill(64, 1.f), w2 = fill(64 * 64, 1.f), w3 = fill(64, 1.f);
        SngMlpWeights w{w1.data(), b.data(), w2.data(), b.data(), w3.data(), b.data()};
        float ls[3] = {0.f, -1.f, 0.5f};
        std::string why;
        if (ppo_weights_check(11, 3, 0, &w, ls, &why) != SNG_OK) return 3;
        if (ppo_weights_check(11, 3, 0, &w, nullptr, &why) != SNG_OK) return 4;
        ls[1] = INFINITY;
        if (ppo_weights_check(11, 3, 0, &w, ls, &why) != SNG_ERR_INVALID_ARGUMENT || why != "non-finite log_std") return 5;
        ls[1] = 0.f;
        w3[63] = NAN;
        if (ppo_weights_check(11, 3, 0, &w, ls, &why) != SNG_ERR_INVALID_ARGUMENT || why != "non-finite value net weight") return 6;
        if (ppo_weights_check(11, 3, 0, nullptr, ls, &why) != SNG_ERR_INVALID_ARGUMENT) return 7;
        if (ppo_dims_check(11, 3, 2, &why) != SNG_ERR_INVALID_ARGUMENT || ppo_dims_check(0, 3, 0, &why) != SNG_ERR_INVALID_ARGUMENT) return 8;
        float x = 0.f;
        double r = 0.0;
        uint8_t dn = 0;
        SngPpoRollout ro{1, 0.99, 0.95, &x, &r, &dn, nullptr, &x, &x, &x, nullptr};
        if (ppo_rollout_check(&ro, true, &why) != SNG_OK) return 9;
        ro.days = 0;
        if (ppo_rollout_check(&ro, true, &why) != SNG_ERR_INVALID_ARGUMENT) return 10;
        ro.days = 1;
        ro.gamma = 1.0000001;
        if (ppo_rollout_check(&ro, true, &why) != SNG_ERR_INVALID_ARGUMENT) return 11;
        ro.gamma = NAN;
        if (ppo_rollout_check(&ro, true, &why) != SNG_ERR_INVALID_ARGUMENT) return 12;
        ro.gamma = 0.0;
        ro.gae_lambda = -0.1;
        if (ppo_rollout_check(&ro, true, &why) != SNG_ERR_INVALID_ARGUMENT) return 13;
        ro.gae_lambda = 1.0;
        ro.obs = nullptr;
        if (ppo_rollout_check(&ro, true, &why) != SNG_ERR_INVALID_ARGUMENT || ppo_rollout_check(&ro, false, &why) != SNG_OK) return 14;
        ro.returns = nullptr;
        if (ppo_rollout_check(&ro, false, &why) != SNG_ERR_INVALID_ARGUMENT) return 15;
    }
    printf("ppo host ok: %ld outputs\n", checked);
    return 0;
}
