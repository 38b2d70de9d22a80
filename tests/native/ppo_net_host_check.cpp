// The net PPO head's host model (csrc/sng_ppo_net_host.h) against naive evaluations written here, bitwise
// (tests/test_ppo_net_rollout_cpu.py builds this with plain g++, -ffp-contract=off, -Wall -Werror and no ROCm on the
// include path).  The value path is held against a naive chain over the unpacked arrays, the GAE against a walk of
// one env at a time with every intermediate in a volatile float, and the log-probability against a loop that reads
// log_std and recomputes 1 / exp itself; the image's tail must be log_std | inv_std behind the NetImage, zero padded.
// Cases: (H1, H2) in {(8, 8), (33, 65), (64, 64), (400, 300), (512, 512)} x O in {11, 29} x A in {2, 9, 129} (one A
// per O and net, in rotation) x relu / tanh x T = 12 x E = 5 x days = 2.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "sng_ppo_net_host.h"

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
    const int nets[][2] = {{8, 8}, {33, 65}, {64, 64}, {400, 300}, {512, 512}};
    const int Os[] = {11, 29}, As[] = {2, 9, 129};
    const int days = 2, T = 12;
    const int64_t E = 5;
    const double gamma = 0.99, lambda = 0.95;
    long checked = 0;
    int rotation = 0;
    for (const auto &net : nets)
        for (int O : Os)
            for (int activation = 0; activation < 2; ++activation) {
                const int H1 = net[0], H2 = net[1], A = As[rotation++ % 3];
                const SngPpoNetSpec spec{H1, H2, activation};
                const auto w1 = fill((size_t)H1 * O, 1.f / std::sqrt((float)O)), b1 = fill(H1, 0.3f);
                const auto w2 = fill((size_t)H2 * H1, 1.f / std::sqrt((float)H1)), b2 = fill(H2, 0.3f);
                const auto w3 = fill(H2, 4.f / std::sqrt((float)H2)), b3 = fill(1, 0.3f);
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
                if (ppo_net_spec_check(&spec, O, A, &why) != SNG_OK ||
                    ppo_net_weights_check(O, A, spec, &w, log_std.data(), &why) != SNG_OK) {
                    printf("refused: %s\n", why.c_str());
                    return 1;
                }
                const PpoNetImage m = ppo_net_image(O, A, spec);
                if (m.head.log_std != m.v.floats || m.head.inv_std != m.v.floats + (size_t)m.head.AP ||
                    m.floats != m.v.floats + 2 * (size_t)m.head.AP || m.head.AP < A || m.head.AP % kPolicyOutChunk)
                    return 2;
                std::vector<float> img(m.floats, 7.f), values(rows), adv(steps), ret(steps), logp(steps);
                ppo_net_pack(m, spec, w, log_std.data(), img.data());
                ppo_net_values_host(m, img.data(), days, T, E, obs.data(), values.data());
                ppo_gae_host(days, T, E, gamma, lambda, reward.data(), done.data(), values.data(), adv.data(), ret.data());
                ppo_logp_host(m.head, img.data(), days, T, E, noise.data(), logp.data());
                // the value path: a naive chain over the unpacked arrays
                std::vector<float> h1(H1), h2(H2);
                for (size_t r = 0; r < rows; ++r) {
                    for (int j = 0; j < H1; ++j) h1[j] = act(activation, chain(&obs[r * O], &w1[(size_t)j * O], O, b1[j]));
                    for (int j = 0; j < H2; ++j) h2[j] = act(activation, chain(h1.data(), &w2[(size_t)j * H1], H1, b2[j]));
                    const float want = chain(h2.data(), w3.data(), H2, b3[0]);
                    if (!same(values[r], want)) {
                        printf("value mismatch %d-%d O=%d act=%d row %zu: %a %a\n", H1, H2, O, activation, r, values[r], want);
                        return 1;
                    }
                    ++checked;
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
                                printf("gae mismatch d=%d t=%d e=%d: %a %a, want %a %a\n", d, t, (int)e, adv[at], ret[at],
                                       (float)gae, (float)rr);
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
                // the tail: log_std | inv_std, zero padded; a head without a value net has a zero NetImage
                for (int j = 0; j < m.head.AP; ++j) {
                    const float ls = j < A ? log_std[j] : 0.f, is = j < A ? 1.0f / std::exp(log_std[j]) : 0.f;
                    if (!same(img[m.head.log_std + j], ls) || !same(img[m.head.inv_std + j], is)) return 3;
                }
                std::vector<float> bare(m.floats, 7.f);
                ppo_net_pack_log_std(m, log_std.data(), bare.data());
                for (size_t i = 0; i < m.v.floats; ++i)
                    if (bare[i] != 0.f) return 4;
                if (std::memcmp(&bare[m.v.floats], &img[m.v.floats], (m.floats - m.v.floats) * sizeof(float)) != 0) return 5;
            }
    // validation
    {
        std::string why;
        const SngPpoNetSpec ok{33, 65, 1};
        if (ppo_net_spec_check(&ok, 29, 11, &why) != SNG_OK) return 10;
        if (ppo_net_spec_check(nullptr, 29, 11, &why) != SNG_ERR_INVALID_ARGUMENT) return 11;
        for (int bad : {7, 513, 0, -1}) {
            const SngPpoNetSpec a{bad, 64, 1}, b{64, bad, 1};
            if (ppo_net_spec_check(&a, 29, 11, &why) != SNG_ERR_UNSUPPORTED || why.find("8 .. 512") == std::string::npos) return 12;
            if (ppo_net_spec_check(&b, 29, 11, &why) != SNG_ERR_UNSUPPORTED) return 13;
        }
        const SngPpoNetSpec act{64, 64, 2}, wide{512, 512, 0};
        if (ppo_net_spec_check(&act, 29, 11, &why) != SNG_ERR_INVALID_ARGUMENT) return 14;
        if (ppo_net_spec_check(&ok, 0, 11, &why) != SNG_ERR_INVALID_ARGUMENT) return 15;
        if (ppo_net_spec_check(&wide, 109, 51, &why) != SNG_OK) return 16;
        if (ppo_net_spec_check(&wide, 121, 57, &why) != SNG_ERR_UNSUPPORTED || why.find("164352") == std::string::npos ||
            why.find("163840") == std::string::npos || why.find("512-512") == std::string::npos)
            return 17;
        if (ppo_net_spec_check(&ok, 29, 129, &why) != SNG_OK) return 18;
        if (ppo_net_spec_check(&ok, 29, kPpoNetMaxAct + 1, &why) != SNG_ERR_UNSUPPORTED) return 19;
        auto w1 = fill(33 * 11, 1.f), b1 = fill(33, 1.f), w2 = fill(65 * 33, 1.f), b2 = fill(65, 1.f), w3 = fill(65, 1.f);
        SngMlpWeights w{w1.data(), b1.data(), w2.data(), b2.data(), w3.data(), b1.data()};
        float ls[3] = {0.f, -1.f, 0.5f};
        if (ppo_net_weights_check(11, 3, ok, &w, ls, &why) != SNG_OK) return 20;
        if (ppo_net_weights_check(11, 3, ok, &w, nullptr, &why) != SNG_OK) return 21;
        ls[1] = INFINITY;
        if (ppo_net_weights_check(11, 3, ok, &w, ls, &why) != SNG_ERR_INVALID_ARGUMENT || why != "non-finite log_std") return 22;
        ls[1] = 0.f;
        w3[64] = NAN;
        if (ppo_net_weights_check(11, 3, ok, &w, ls, &why) != SNG_ERR_INVALID_ARGUMENT || why != "non-finite value net weight") return 23;
        if (ppo_net_weights_check(11, 3, ok, nullptr, ls, &why) != SNG_ERR_INVALID_ARGUMENT || why != "null value net weights") return 24;
        // 65,536 envs x 97 rows x days: 64-bit rows and blocks
        if (ppo_net_rows(65535, 96, 65536) != (int64_t)65535 * 97 * 65536 || ppo_net_blocks(65) != 2) return 25;
        if (ppo_net_blocks(ppo_net_rows(65535, 96, 65536)) <= kPpoNetMaxBlocks) return 26;
    }
    printf("ppo net host ok: %ld outputs\n", checked);
    return 0;
}
