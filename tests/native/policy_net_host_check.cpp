// The any-width MLP actor's host model (csrc/sng_policy_net_host.h) against a second, naive evaluation written
// here, bitwise (tests/test_policy_net_cpu.py builds this with plain g++, -ffp-contract=off, -Wall -Werror and no
// ROCm on the include path, and once more with -fsanitize=address,undefined).  The naive one reads torch's
// [out][in] arrays directly and never sees the packed image, so a wrong tile, group, lane or pad in the MFMA
// B-operand packing shows as a mismatch.
// Cases: nets (400, 300), (64, 64), (8, 8), (33, 65), (512, 512) x obs_dim {11, 109} x act_dim {2, 51} x relu / tanh
// x {mean, mean with clip, squash} x noise / none, 5 random rows each.  Then: the 64-64 mean net equals
// mlp_actor_host (csrc/sng_policy_host.h) bitwise; every padded entry of an image is zero; every refusal of
// net_spec_check / net_weights_check; the LDS sizes that must fit and one that must not; and policy_net_day_form
// gives nodes for every plan (listed on stdout).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sng_policy_net_host.h"
#include "sng_graph_form.h"

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

static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

struct Net {
    int O, A, H1, H2;
    std::vector<float> w1, b1, w2, b2, w3, b3, low, high;
    Net(int O_, int A_, int H1_, int H2_) : O(O_), A(A_), H1(H1_), H2(H2_) {
        w1 = fill((size_t)H1 * O, 1.f / std::sqrt((float)O));
        b1 = fill(H1, 0.3f);
        w2 = fill((size_t)H2 * H1, 1.f / std::sqrt((float)H1));
        b2 = fill(H2, 0.3f);
        w3 = fill((size_t)A * H2, 3.f / std::sqrt((float)H2));
        b3 = fill(A, 0.3f);
        low.resize(A);
        high.resize(A);
        for (int j = 0; j < A; ++j) {   // the Boxes of the stations: with V2X [-1, 1], without [0, 1]
            low[j] = (j % 3 == 0) ? -1.f : 0.f;
            high[j] = 1.f;
        }
    }
    SngMlpWeights weights() const { return {w1.data(), b1.data(), w2.data(), b2.data(), w3.data(), b3.data()}; }
};

int main() {
    const int nets[][2] = {{400, 300}, {64, 64}, {8, 8}, {33, 65}, {512, 512}};
    const int Os[] = {11, 109}, As[] = {2, 51};
    const int rows = 5;
    long checked = 0;
    for (const auto &hw : nets)
        for (int O : Os)
            for (int A : As) {
                const Net n(O, A, hw[0], hw[1]);
                const SngMlpWeights w = n.weights();
                const auto obs = fill((size_t)rows * O, 1.f), noise = fill((size_t)rows * A, 0.8f);
                for (int activation = 0; activation < 2; ++activation)
                    for (int mode = 0; mode < 3; ++mode)   // mean, mean + clip, squash
                        for (int with_noise = 0; with_noise < 2; ++with_noise) {
                            const int output = mode == 2 ? SNG_MLP_OUT_SQUASH : SNG_MLP_OUT_MEAN;
                            const bool bounds = mode != 0;
                            const SngMlpNetSpec spec{O, A, n.H1, n.H2, activation, output,
                                                     bounds ? n.low.data() : nullptr, bounds ? n.high.data() : nullptr};
                            std::string why;
                            if (net_spec_check(&spec, O, A, &why) != SNG_OK || net_weights_check(spec, &w, &why) != SNG_OK) {
                                printf("refused: %s\n", why.c_str());
                                return 1;
                            }
                            const NetImage m = net_image(O, A, n.H1, n.H2, activation, output, bounds);
                            std::vector<float> img(m.floats), a((size_t)rows * A), env((size_t)rows * A);
                            net_pack(m, spec, w, img.data());
                            // every entry the packing did not write is zero: as many non-zeros as real values at most
                            if (activation == 0 && mode == 0 && with_noise == 0) {
                                size_t nz = 0;
                                for (float v : img) nz += v != 0.f;
                                const size_t real = (size_t)n.H1 * O + n.H1 + (size_t)n.H2 * n.H1 + n.H2 + (size_t)A * n.H2 + A;
                                if (nz > real || nz + 64 < real) {
                                    printf("image of %d-%d O=%d A=%d: %zu non-zero entries for %zu values\n", n.H1, n.H2, O, A, nz, real);
                                    return 1;
                                }
                            }
                            mlp_net_host(m, img.data(), rows, obs.data(), with_noise ? noise.data() : nullptr, a.data(),
                                         env.data());
                            std::vector<float> h1(n.H1), h2(n.H2);
                            for (int r = 0; r < rows; ++r) {
                                for (int j = 0; j < n.H1; ++j)
                                    h1[j] = act(activation, chain(&obs[(size_t)r * O], &n.w1[(size_t)j * O], O, n.b1[j]));
                                for (int j = 0; j < n.H2; ++j)
                                    h2[j] = act(activation, chain(h1.data(), &n.w2[(size_t)j * n.H1], n.H1, n.b2[j]));
                                for (int j = 0; j < A; ++j) {
                                    const float mean = chain(h2.data(), &n.w3[(size_t)j * n.H2], n.H2, n.b3[j]);
                                    const float nz = noise[(size_t)r * A + j];
                                    float want, stepped;
                                    if (mode == 2) {
                                        want = std::tanh(mean);
                                        if (with_noise) want = std::fmin(std::fmax(want + nz, -1.f), 1.f);
                                        const float d = n.high[j] - n.low[j];
                                        const float half = 0.5f * (want + 1.0f);
                                        const float prod = half * d;
                                        stepped = n.low[j] + prod;
                                    } else {
                                        want = with_noise ? mean + nz : mean;
                                        stepped = mode == 1 ? std::fmin(std::fmax(want, n.low[j]), n.high[j]) : want;
                                    }
                                    const float got = a[(size_t)r * A + j], got_env = env[(size_t)r * A + j];
                                    if (!same(got, want) || !same(got_env, stepped)) {
                                        printf("mismatch %d-%d O=%d A=%d act=%d mode=%d noise=%d row %d out %d: %a %a, want %a %a\n",
                                               n.H1, n.H2, O, A, activation, mode, with_noise, r, j, got, got_env, want, stepped);
                                        return 1;
                                    }
                                    ++checked;
                                }
                            }
                            // the 64-64 mean net is the existing actor's contract, bit for bit
                            if (n.H1 == 64 && n.H2 == 64 && mode != 2) {
                                const SngMlpSpec old{O, A, 64, activation, spec.low, spec.high};
                                const PolicyImage pm = policy_image(O, A, activation, bounds);
                                std::vector<float> pimg(pm.floats), pa((size_t)rows * A), penv((size_t)rows * A);
                                policy_pack(pm, old, w, pimg.data());
                                mlp_actor_host(pm, pimg.data(), rows, obs.data(), with_noise ? noise.data() : nullptr,
                                               pa.data(), penv.data());
                                if (std::memcmp(pa.data(), a.data(), a.size() * 4) != 0 ||
                                    std::memcmp(penv.data(), env.data(), env.size() * 4) != 0) {
                                    printf("64-64 differs from mlp_actor_host: O=%d A=%d act=%d mode=%d noise=%d\n", O, A,
                                           activation, mode, with_noise);
                                    return 1;
                                }
                            }
                        }
            }
    // validation
    {
        const float lo[2] = {0.f, -1.f}, hi[2] = {1.f, 1.f}, inf[2] = {1.f, INFINITY}, rev[2] = {-1.f, -2.f};
        const SngMlpNetSpec ok{11, 2, 400, 300, 1, SNG_MLP_OUT_SQUASH, lo, hi};
        std::string why;
        auto rc = [&](SngMlpNetSpec s, int O = 11, int A = 2) { return net_spec_check(&s, O, A, &why); };
        auto with = [&](auto edit) {
            SngMlpNetSpec s = ok;
            edit(s);
            return s;
        };
        if (rc(ok) != SNG_OK) return 2;
        if (net_spec_check(nullptr, 0, 0, &why) != SNG_ERR_INVALID_ARGUMENT) return 3;
        if (rc(ok, 13, 2) != SNG_ERR_INVALID_ARGUMENT || rc(ok, 11, 3) != SNG_ERR_INVALID_ARGUMENT) return 4;
        if (rc(with([](SngMlpNetSpec &s) { s.obs_dim = 0; }), 0, 0) != SNG_ERR_INVALID_ARGUMENT) return 5;
        for (int bad : {7, 513, 0, -4}) {
            if (rc(with([&](SngMlpNetSpec &s) { s.hidden1 = bad; })) != SNG_ERR_UNSUPPORTED) return 6;
            if (rc(with([&](SngMlpNetSpec &s) { s.hidden2 = bad; })) != SNG_ERR_UNSUPPORTED) return 7;
        }
        for (int fine : {8, 512, 33})
            if (rc(with([&](SngMlpNetSpec &s) { s.hidden1 = s.hidden2 = fine; })) != SNG_OK) return 8;
        if (rc(with([](SngMlpNetSpec &s) { s.activation = 2; })) != SNG_ERR_INVALID_ARGUMENT) return 9;
        if (rc(with([](SngMlpNetSpec &s) { s.output = 2; })) != SNG_ERR_INVALID_ARGUMENT) return 10;
        if (rc(with([](SngMlpNetSpec &s) { s.high = nullptr; })) != SNG_ERR_INVALID_ARGUMENT) return 11;
        if (rc(with([](SngMlpNetSpec &s) { s.low = s.high = nullptr; })) != SNG_ERR_INVALID_ARGUMENT) return 12;   // squash
        if (rc(with([](SngMlpNetSpec &s) { s.low = s.high = nullptr; s.output = SNG_MLP_OUT_MEAN; })) != SNG_OK) return 13;
        if (rc(with([&](SngMlpNetSpec &s) { s.high = inf; })) != SNG_ERR_INVALID_ARGUMENT) return 14;   // squash: finite
        if (rc(with([&](SngMlpNetSpec &s) { s.high = inf; s.output = SNG_MLP_OUT_MEAN; })) != SNG_OK) return 15;
        if (rc(with([&](SngMlpNetSpec &s) { s.high = rev; })) != SNG_ERR_INVALID_ARGUMENT) return 16;
        // LDS: every pair up to 512 at 16 chargers (obs_dim 41), the named nets at 50 (obs_dim 109)
        for (int h1 = 8; h1 <= 512; h1 += 8)
            if (rc(with([&](SngMlpNetSpec &s) { s.obs_dim = 41; s.hidden1 = h1; s.hidden2 = 512; }), 41, 2) != SNG_OK) return 17;
        for (const auto &hw : {std::pair<int, int>{400, 300}, {256, 256}, {64, 64}, {512, 512}})
            if (rc(with([&](SngMlpNetSpec &s) { s.obs_dim = 109; s.hidden1 = hw.first; s.hidden2 = hw.second; }), 109, 2) != SNG_OK)
                return 18;
        if (rc(with([](SngMlpNetSpec &s) { s.obs_dim = 409; s.hidden1 = 512; }), 409, 2) != SNG_ERR_UNSUPPORTED) return 19;
        if (why.find("409") == std::string::npos || why.find("512-300") == std::string::npos) return 20;
        // two output tiles: 64 actions at most, on the host as on the device
        if (rc(with([](SngMlpNetSpec &s) { s.act_dim = 64; s.low = s.high = nullptr; s.output = SNG_MLP_OUT_MEAN; }), 11, 64) != SNG_OK)
            return 25;
        if (rc(with([](SngMlpNetSpec &s) { s.act_dim = 65; s.low = s.high = nullptr; s.output = SNG_MLP_OUT_MEAN; }), 11, 65) !=
            SNG_ERR_UNSUPPORTED)
            return 26;
        if (why.find("act_dim 65") == std::string::npos) return 27;
        if (rc(with([](SngMlpNetSpec &s) { s.obs_dim = 1 << 30; }), 1 << 30, 2) != SNG_ERR_UNSUPPORTED) return 28;
        const NetImage ddpg50 = net_image(109, 51, 400, 300, 1, SNG_MLP_OUT_SQUASH, true);
        printf("lds 400-300 obs 109: %zu B of %zu\n", net_lds_bytes(ddpg50), kNetMaxLds);
        // weights
        const Net n(11, 2, 33, 65);
        const SngMlpNetSpec s33{11, 2, 33, 65, 1, SNG_MLP_OUT_MEAN, nullptr, nullptr};
        SngMlpWeights w = n.weights();
        if (net_weights_check(s33, &w, nullptr) != SNG_OK) return 21;
        std::vector<float> w2 = n.w2;
        w.w2 = w2.data();
        w2[w2.size() - 1] = NAN;
        if (net_weights_check(s33, &w, nullptr) != SNG_ERR_INVALID_ARGUMENT) return 22;
        w2[w2.size() - 1] = -INFINITY;
        if (net_weights_check(s33, &w, nullptr) != SNG_ERR_INVALID_ARGUMENT) return 23;
        w.w2 = nullptr;
        if (net_weights_check(s33, &w, nullptr) != SNG_ERR_INVALID_ARGUMENT) return 24;
    }
    // the form of a net policy's captured day: nodes for every family, station and flag
    {
        int listed = 0;
        for (int family = STEP_LEAN; family <= STEP_GENERAL; ++family)
            for (const StationSize &sz : kStationSizes)
                for (int bits = 0; bits < 64; ++bits) {
                    const StepPlan pl{(StepFamily)family, sz.n, family == STEP_WIDE ? kWideLanes : 1, (bits & 1) != 0,
                                      (bits & 2) != 0, false, (bits & 4) != 0, true};
                    const bool traj = bits & 8, nodes = bits & 16, force = bits & 32;
                    const PolicyDayForm form = policy_net_day_form(pl, traj, nodes, force);
                    char name[128];
                    step_plan_name(pl, name, sizeof name);
                    printf("net plan | %s | traj %d step_nodes %d force %d | %s\n", name, traj, nodes, force,
                           form == POLICY_NODES ? "nodes" : "fused");
                    if (form != POLICY_NODES) return 30;
                    ++listed;
                }
        if (listed != 3 * 7 * 64) return 31;
    }
    printf("policy net host ok: %ld outputs\n", checked);
    return 0;
}
