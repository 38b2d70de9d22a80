// The action noise's host model (csrc/sng_noise_host.h) on its own: tests/test_action_noise_cpu.py builds this with
// plain g++, -ffp-contract=off, -Wall -Werror and no ROCm on the include path, so the header the kernel compiles is
// also a host header.
//   noise_host_check                      self-checks, prints "noise host ok"
//   noise_host_check <in.u32> <out.f32>   ... and the variate of every 32-bit hash in the first file into the second
// Self-checks: the variate is odd in the sign bit, never 0 and finite at the ends of every segment and for h = 0; the
// segment index and fraction are what a bit-by-bit walk gives; noise_host_fill is the naive loop over noise_key /
// noise_hash / noise_z_host for both kinds (the OU recurrence with every intermediate in a volatile float); every
// refusal gives SNG_ERR_INVALID_ARGUMENT and names the value.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "sng_noise_host.h"

using namespace sng;

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                              \
        }                                                            \
    } while (0)

static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static void check_variate() {
    CHECK(noise_z_host(0u) > 6.0f && noise_z_host(0x80000000u) < -6.0f);   // u = max(0, 1)
    CHECK(same(noise_z_host(0u), noise_z_host(1u)));
    for (int msb = 0; msb <= 30; ++msb) {
        const uint32_t lo = 1u << msb, hi = msb == 30 ? 0x7fffffffu : (2u << msb) - 1u;
        for (uint32_t u : {lo, hi, lo + (hi - lo) / 4, lo + (hi - lo) / 2, lo + (hi - lo) / 4 * 3}) {
            const float z = noise_z_host(u), m = noise_z_host(u | 0x80000000u);
            CHECK(z > 0.f && std::isfinite(z) && same(m, -z));
            float x;
            const int seg = noise_segment(u, &x);
            // bit by bit: the octave, then two bits, then 24
            int top = 30;
            while (!((u >> top) & 1u)) --top;
            CHECK(top == msb && seg / kNoiseSubs == 30 - msb);
            uint32_t sub = 0, frac = 0;
            for (int b = 0; b < 26; ++b) {
                const int at = msb - 1 - b;
                const uint32_t bit = at >= 0 ? (u >> at) & 1u : 0u;
                if (b < 2) sub = 2 * sub + bit;
                else frac = 2 * frac + bit;
            }
            CHECK(seg % kNoiseSubs == (int)sub && x == (float)frac * 0x1.0p-24f && x < 1.0f);
        }
    }
    // decreasing in u (towards p = 0.5) across a segment's and an octave's border, up to the fit's error
    for (int msb = 3; msb <= 30; ++msb)
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t u = (1u << msb) + q * (1u << (msb - 2));
            CHECK(std::fabs(noise_z_host(u) - noise_z_host(u - 1)) < 2.5e-1f);
            if (msb >= 12) CHECK(std::fabs(noise_z_host(u) - noise_z_host(u - 1)) < 1e-3f);
        }
}

static void check_fill() {
    const int A = 5, T = 7, days = 3;
    const int64_t E = 6, off = (int64_t)((1ull << 33) + 5);
    const uint64_t seed = 0x123456789abcdef0ull, c = (1ull << 40) + 3;
    const float mu[A] = {0.f, 0.25f, -1.5f, 3.f, 0.125f}, scale[A] = {1.f, 0.5f, 2.f, 0.f, 0.3f};
    for (int kind : {SNG_NOISE_GAUSSIAN, SNG_NOISE_OU}) {
        const SngNoiseSpec spec{kind, A, seed, 0.15, 1e-2};
        std::string why;
        CHECK(noise_spec_check(&spec, A, &why) == SNG_OK && noise_params_check(A, mu, scale, &why) == SNG_OK);
        std::vector<float> params(2 * A), out((size_t)days * T * E * A, -7.f);
        noise_pack_params(spec, mu, scale, params.data());
        noise_host_fill(spec, params.data(), T, E, off, c, days, out.data());
        const float theta = (float)spec.theta, dt = (float)spec.dt;
        for (int d = 0; d < days; ++d)
            for (int64_t e = 0; e < E; ++e)
                for (int j = 0; j < A; ++j) {
                    const uint32_t key = noise_key(seed, (uint64_t)(off + e), (uint32_t)j, c + (uint64_t)d);
                    const float sd = kind == SNG_NOISE_OU ? (float)((double)scale[j] * std::sqrt(1e-2)) : scale[j];
                    CHECK(same(sd, params[A + j]) && same(mu[j], params[j]));
                    volatile float x = 0.f;
                    for (int t = 0; t < T; ++t) {
                        const float z = noise_z_host(noise_mix32(key + (uint32_t)t * 0x9e3779b9u));
                        if (kind == SNG_NOISE_OU) {
                            volatile float a = mu[j] - x;
                            volatile float b = theta * a;
                            volatile float g = b * dt;
                            volatile float h = x + g;
                            volatile float s = sd * z;
                            x = h + s;
                        } else {
                            volatile float s = sd * z;
                            x = mu[j] + s;
                        }
                        CHECK(same(x, out[(((size_t)d * T + t) * E + e) * A + j]));
                    }
                }
    }
    // the key takes all 64 bits of the env and of the counter, and the action
    const uint32_t k = noise_key(1, 2, 3, 4);
    CHECK(k != noise_key(1, 2 + (1ull << 32), 3, 4) && k != noise_key(1, 2, 3, 4 + (1ull << 32)));
    CHECK(k != noise_key(1 + (1ull << 32), 2, 3, 4) && k != noise_key(1, 2, 4, 4) && k != noise_key(1, 3, 3, 4));
    CHECK(kDomainNoise != 0x50560000u && kDomainNoise != 0x50520000u && kDomainNoise != 0x7a710000u &&
          kDomainNoise != 0x7a720000u && (kDomainNoise & 0xffu) == 0);
}

static void check_refusals() {
    std::string why;
    const float inf = INFINITY, nan = NAN;
    SngNoiseSpec ok{SNG_NOISE_OU, 5, 0, 0.15, 1e-2};
    CHECK(noise_spec_check(nullptr, 0, &why) == SNG_ERR_INVALID_ARGUMENT);
    for (int a : {0, -1, 256}) {
        SngNoiseSpec s = ok;
        s.act_dim = a;
        CHECK(noise_spec_check(&s, 0, &why) == SNG_ERR_INVALID_ARGUMENT && why.find(std::to_string(a)) != std::string::npos);
    }
    CHECK(noise_spec_check(&ok, 6, &why) == SNG_ERR_INVALID_ARGUMENT && why.find("6") != std::string::npos);
    CHECK(noise_spec_check(&ok, 5, &why) == SNG_OK && noise_spec_check(&ok, 0, &why) == SNG_OK);
    SngNoiseSpec s = ok;
    s.kind = 2;
    CHECK(noise_spec_check(&s, 0, &why) == SNG_ERR_INVALID_ARGUMENT && why.find("kind 2") != std::string::npos);
    s = ok;
    s.theta = inf;
    CHECK(noise_spec_check(&s, 0, &why) == SNG_ERR_INVALID_ARGUMENT && why.find("theta") != std::string::npos);
    s = ok;
    s.dt = nan;
    CHECK(noise_spec_check(&s, 0, &why) == SNG_ERR_INVALID_ARGUMENT && why.find("dt") != std::string::npos);
    s = ok;
    s.dt = -1.0;
    CHECK(noise_spec_check(&s, 0, &why) == SNG_ERR_INVALID_ARGUMENT && why.find("negative") != std::string::npos);
    float mu[5] = {0, 0, 0, 0, 0}, scale[5] = {1, 1, 1, 1, 1};
    CHECK(noise_params_check(5, mu, scale, &why) == SNG_OK && noise_params_check(5, nullptr, scale, &why) == SNG_OK);
    CHECK(noise_params_check(5, mu, nullptr, &why) == SNG_ERR_INVALID_ARGUMENT);
    mu[3] = nan;
    CHECK(noise_params_check(5, mu, scale, &why) == SNG_ERR_INVALID_ARGUMENT && why.find("mu[3]") != std::string::npos);
    mu[3] = 0.f;
    scale[2] = inf;
    CHECK(noise_params_check(5, mu, scale, &why) == SNG_ERR_INVALID_ARGUMENT && why.find("scale[2]") != std::string::npos);
    scale[2] = -0.5f;
    CHECK(noise_params_check(5, mu, scale, &why) == SNG_ERR_INVALID_ARGUMENT && why.find("scale[2]") != std::string::npos &&
          why.find("negative") != std::string::npos);
}

int main(int argc, char **argv) {
    check_variate();
    check_fill();
    check_refusals();
    size_t n = 0;
    if (argc == 3) {
        std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
        if (!in || !out) {
            std::printf("cannot open %s or %s\n", argv[1], argv[2]);
            return 2;
        }
        std::vector<uint32_t> h(1 << 16);
        std::vector<float> z(h.size());
        size_t got;
        while ((got = std::fread(h.data(), 4, h.size(), in)) > 0) {
            for (size_t i = 0; i < got; ++i) z[i] = noise_z_host(h[i]);
            if (std::fwrite(z.data(), 4, got, out) != got) return 2;
            n += got;
        }
        std::fclose(in);
        std::fclose(out);
    }
    if (failures) return 1;
    std::printf("noise host ok %zu variates\n", n);
    return 0;
}
