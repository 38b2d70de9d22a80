// The MLP actor's host model (csrc/sng_policy_host.h) against a second, naive evaluation written here, bitwise
// (tests/test_policy_cpu.py builds this with plain g++, -ffp-contract=off, -Wall -Werror and no ROCm on the include
// path).  The naive one reads torch's [out][in] arrays directly and never sees the packed image, so a wrong
// transpose, a wrong pad or a wrong offset in the packing shows as a mismatch.
// Cases: O in {11, 25, 41, 109} x A in {2, 9, 17, 51} (odd K, A above one and two output chunks) x relu / tanh x
// clip / no clip x noise / none, 37 random rows each.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sng_policy_host.h"

using namespace sng;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static float uniform(float lo, float hi) {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    const double u = (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
    return (float)(lo + (hi - lo) * u);
}

static std::vector<float> fill(size_t n, float bound) {
    std::vector<float> v(n);
    for (float &x : v) x = uniform(-bound, bound);
    return v;
}

static float act(int activation, float h) { return activation == 1 ? (h > 0.f ? h : 0.f) : std::tanh(h); }

// one layer, one output: the k-ordered fmaf chain from the bias
static float chain(const float *in, const float *w_row, int K, float bias) {
    float h = bias;
    for (int k = 0; k < K; ++k) h = std::fmaf(in[k], w_row[k], h);
    return h;
}

int main() {
    const int Os[] = {11, 25, 41, 109}, As[] = {2, 9, 17, 51};
    const int rows = 37, H = 64;
    long checked = 0;
    for (int O : Os)
        for (int A : As)
            for (int activation = 0; activation < 2; ++activation)
                for (int clip = 0; clip < 2; ++clip)
                    for (int with_noise = 0; with_noise < 2; ++with_noise) {
                        const auto w1 = fill((size_t)H * O, 1.f / std::sqrt((float)O)), b1 = fill(H, 0.3f);
                        const auto w2 = fill((size_t)H * H, 0.125f), b2 = fill(H, 0.3f);
                        const auto w3 = fill((size_t)A * H, 0.5f), b3 = fill(A, 0.3f);
                        const auto obs = fill((size_t)rows * O, 1.f), noise = fill((size_t)rows * A, 0.4f);
                        std::vector<float> low(A), high(A);
                        for (int j = 0; j < A; ++j) {
                            low[j] = (j % 3 == 0) ? -1.f : 0.f;
                            high[j] = 1.f;
                        }
                        SngMlpSpec spec{O, A, H, activation, clip ? low.data() : nullptr, clip ? high.data() : nullptr};
                        const SngMlpWeights w{w1.data(), b1.data(), w2.data(), b2.data(), w3.data(), b3.data()};
                        std::string why;
                        if (policy_spec_check(&spec, O, A, &why) != SNG_OK || policy_weights_check(spec, &w, &why) != SNG_OK) {
                            printf("refused: %s\n", why.c_str());
                            return 1;
                        }
                        const PolicyImage m = policy_image(O, A, activation, clip != 0);
                        std::vector<float> img(m.floats), a((size_t)rows * A), env((size_t)rows * A);
                        policy_pack(m, spec, w, img.data());
                        mlp_actor_host(m, img.data(), rows, obs.data(), with_noise ? noise.data() : nullptr, a.data(),
                                       env.data());
                        for (int r = 0; r < rows; ++r) {
                            float h1[64], h2[64];
                            for (int j = 0; j < H; ++j) h1[j] = act(activation, chain(&obs[(size_t)r * O], &w1[(size_t)j * O], O, b1[j]));
                            for (int j = 0; j < H; ++j) h2[j] = act(activation, chain(h1, &w2[(size_t)j * H], H, b2[j]));
                            for (int j = 0; j < A; ++j) {
                                const float mean = chain(h2, &w3[(size_t)j * H], H, b3[j]);
                                const float want = with_noise ? mean + noise[(size_t)r * A + j] : mean;
                                float stepped = want;
                                if (clip) stepped = std::fmin(std::fmax(want, low[j]), high[j]);
                                const float got = a[(size_t)r * A + j], got_env = env[(size_t)r * A + j];
                                if (std::memcmp(&got, &want, 4) != 0 || std::memcmp(&got_env, &stepped, 4) != 0) {
                                    printf("mismatch O=%d A=%d act=%d clip=%d noise=%d row %d out %d: %a %a, want %a %a\n", O,
                                           A, activation, clip, with_noise, r, j, got, got_env, want, stepped);
                                    return 1;
                                }
                                ++checked;
                            }
                        }
                    }
    // validation: another width is unsupported, the rest is an invalid argument
    {
        const float lo[2] = {0.f, 0.f}, hi[2] = {1.f, 1.f};
        SngMlpSpec spec{11, 2, 64, 0, lo, hi};
        if (policy_spec_check(&spec, 11, 2, nullptr) != SNG_OK) return 2;
        if (policy_spec_check(&spec, 13, 2, nullptr) != SNG_ERR_INVALID_ARGUMENT) return 3;
        spec.hidden = 32;
        if (policy_spec_check(&spec, 11, 2, nullptr) != SNG_ERR_UNSUPPORTED) return 4;
        spec.hidden = 64;
        spec.activation = 2;
        if (policy_spec_check(&spec, 11, 2, nullptr) != SNG_ERR_INVALID_ARGUMENT) return 5;
        spec.activation = 1;
        spec.clip_high = nullptr;
        if (policy_spec_check(&spec, 11, 2, nullptr) != SNG_ERR_INVALID_ARGUMENT) return 6;
        spec.clip_high = hi;
        auto w1 = fill(64 * 11, 1.f), b = fill(64, 1.f), w2 = fill(64 * 64, 1.f), w3 = fill(2 * 64, 1.f);
        SngMlpWeights w{w1.data(), b.data(), w2.data(), b.data(), w3.data(), b.data()};
        if (policy_weights_check(spec, &w, nullptr) != SNG_OK) return 7;
        w3[77] = NAN;
        if (policy_weights_check(spec, &w, nullptr) != SNG_ERR_INVALID_ARGUMENT) return 8;
        w3[77] = INFINITY;
        if (policy_weights_check(spec, &w, nullptr) != SNG_ERR_INVALID_ARGUMENT) return 9;
    }
    printf("policy host ok: %ld outputs\n", checked);
    return 0;
}
