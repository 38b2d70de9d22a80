// The replay ring's and the critic's host models (csrc/sng_ddpg_host.h) against naive evaluations written here
// (tests/test_ddpg_cpu.py builds this with plain g++, -ffp-contract=off, -Wall -Werror and no ROCm on the include
// path).  The sampling law is held against its definition restated with the 128-bit product written out in 32-bit
// limbs; the ring's bookkeeping against a slot -> day map kept here; a push's segments by carrying them out with
// plain loops and comparing the storage with that map; Q against a naive chain over concatenated rows and the
// unpacked arrays, bitwise; the targets against the formula with every intermediate in a volatile float.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "sng_ddpg_host.h"

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

// the high 64 bits of h * n from 32-bit limbs
static uint64_t mulhi_limbs(uint64_t h, uint64_t n) {
    const uint64_t h0 = (uint32_t)h, h1 = h >> 32, n0 = (uint32_t)n, n1 = n >> 32;
    const uint64_t p00 = h0 * n0, p01 = h0 * n1, p10 = h1 * n0, p11 = h1 * n1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

static int check_sampling(long &checked) {
    const uint64_t ns[] = {1, 2, 5040, (1ull << 31) + 7, (1ull << 40) + 1};
    for (uint64_t n : ns)
        for (uint64_t c : {0ull, 1ull, (1ull << 32) + 5})
            for (int64_t off : {(int64_t)0, (int64_t)65536, (int64_t)((1ll << 33) + 3)}) {
                const int64_t B = 300;
                std::vector<int64_t> got(B);
                replay_host_indices(0x1234abcd5678ull, off, c, n, B, got.data());
                const uint32_t k1 = noise_mix32(noise_day_key(0x1234abcd5678ull, c) ^ (uint32_t)off);
                const uint32_t key = noise_mix32(
                    k1 ^ ((uint32_t)((uint64_t)off >> 32) * 0x85ebca6bu + 0x72730000u * 0xc2b2ae35u + 0x27d4eb2fu));
                for (int64_t b = 0; b < B; ++b) {
                    const uint32_t a = noise_mix32(key ^ (uint32_t)b);
                    const uint32_t kb = noise_mix32(a ^ ((uint32_t)((uint64_t)b >> 32) * 0x85ebca6bu + 0x165667b1u));
                    const uint64_t h = ((uint64_t)noise_mix32(kb + 0x9e3779b9u) << 32) | noise_mix32(kb + 2u * 0x9e3779b9u);
                    const uint64_t want = mulhi_limbs(h, n);
                    if ((uint64_t)got[b] != want || want >= n) {
                        printf("index mismatch n=%llu c=%llu b=%lld: %lld, want %llu\n", (unsigned long long)n,
                               (unsigned long long)c, (long long)b, (long long)got[b], (unsigned long long)want);
                        return 1;
                    }
                    ++checked;
                }
            }
    // rows past 2^32 take their high word into the key
    if (replay_sample_bits(7u, 5ull) == replay_sample_bits(7u, 5ull + (1ull << 32))) return 2;
    // the obs row of a transition: slot (T + 1) E + t E + e
    const uint64_t T = 24, E = 70;
    for (uint64_t slot = 0; slot < 3; ++slot)
        for (uint64_t t = 0; t < T; ++t)
            for (uint64_t e = 0; e < E; e += 23) {
                const uint64_t i = (slot * T + t) * E + e;
                if (replay_obs_row(i, T * E, E) != (slot * (T + 1) + t) * E + e) return 3;
                ++checked;
            }
    return 0;
}

// capacity 3; pushes of 2, 2, 1, 3 days: the slot -> day map, filled and head after each, and the storage a push's
// segments leave
static int check_ring(long &checked) {
    const int32_t cap = 3, T = 5, O = 7, A = 3;
    const int64_t E = 6;
    ReplayRing r;
    r.capacity = cap;
    const size_t step = (size_t)T * E, obs_day = (size_t)(T + 1) * E * O, act_day = step * A;
    std::vector<float> s_obs(cap * obs_day, -1.f), s_act(cap * act_day, -1.f), s_rew(cap * step, -1.f);
    std::vector<uint8_t> s_done(cap * step, 9);
    const ReplayStorage ring{s_obs.data(), s_act.data(), s_rew.data(), s_done.data()};
    int slot_day[3] = {-1, -1, -1};
    const int want_head[] = {2, 1, 2, 2}, want_filled[] = {2, 3, 3, 3};
    const int want_map[][3] = {{0, 1, -1}, {3, 1, 2}, {3, 4, 2}, {6, 7, 5}};
    const int pushes[] = {2, 2, 1, 3};
    int day = 0;   // global number of the next pushed day
    std::string why;
    for (int p = 0; p < 4; ++p) {
        const int32_t days = pushes[p];
        if (replay_push_check(r, days, &why) != SNG_OK) return 10;
        // day d of this push: every value encodes the global day and the element
        std::vector<float> obs(days * obs_day), actv(days * act_day);
        std::vector<double> rew(days * step);
        std::vector<uint8_t> done(days * step);
        for (int d = 0; d < days; ++d) {
            for (size_t i = 0; i < obs_day; ++i) obs[d * obs_day + i] = (float)((day + d) * 100000 + (int)i);
            for (size_t i = 0; i < act_day; ++i) actv[d * act_day + i] = (float)(-(day + d) * 100000 - (int)i);
            for (size_t i = 0; i < step; ++i) {
                rew[d * step + i] = -1.0 / 3.0 * (double)((day + d) * 1000 + (int)i);   // not a float32
                done[d * step + i] = (uint8_t)(((day + d) + i) % 2);
            }
        }
        const ReplaySource src{obs.data(), actv.data(), rew.data(), done.data()};
        const PushArgs a = replay_push_args(r, days, ring, src, T, E, O, A);
        if (a.count != 4 && a.count != 8) return 11;
        int64_t longest = 0;
        for (int s = 0; s < a.count; ++s) {
            const PushSegment &g = a.seg[s];
            longest = g.n > longest ? g.n : longest;
            for (int64_t i = 0; i < g.n; ++i) {
                if (g.kind == PUSH_F32) ((float *)g.dst)[i] = ((const float *)g.src)[i];
                else if (g.kind == PUSH_F64_F32) ((float *)g.dst)[i] = (float)((const double *)g.src)[i];
                else ((uint8_t *)g.dst)[i] = ((const uint8_t *)g.src)[i];
            }
        }
        if (longest != a.longest) return 12;
        for (int d = 0; d < days; ++d) slot_day[replay_slot(r, d)] = day + d;
        r = replay_pushed(r, days);
        day += days;
        if (r.head != want_head[p] || r.filled != want_filled[p]) {
            printf("push %d: head %d filled %d\n", p, r.head, r.filled);
            return 13;
        }
        if (replay_size(r, T, E) != (uint64_t)r.filled * T * E) return 14;
        for (int s = 0; s < cap; ++s) {
            if (slot_day[s] != want_map[p][s]) return 15;
            const int g = slot_day[s];
            for (size_t i = 0; i < obs_day; ++i) {
                const float want = g < 0 ? -1.f : (float)(g * 100000 + (int)i);
                if (!same(s_obs[s * obs_day + i], want)) return 16;
            }
            for (size_t i = 0; i < act_day; ++i) {
                const float want = g < 0 ? -1.f : (float)(-g * 100000 - (int)i);
                if (!same(s_act[s * act_day + i], want)) return 17;
            }
            for (size_t i = 0; i < step; ++i) {
                const float want = g < 0 ? -1.f : (float)(-1.0 / 3.0 * (double)(g * 1000 + (int)i));
                if (!same(s_rew[s * step + i], want)) return 18;
                if (s_done[s * step + i] != (g < 0 ? 9 : (uint8_t)((g + i) % 2))) return 19;
            }
            ++checked;
        }
    }
    if (replay_push_check(r, 4, &why) != SNG_ERR_INVALID_ARGUMENT || why.find("capacity_days 3") == std::string::npos) return 20;
    if (replay_push_check(r, 0, &why) != SNG_ERR_INVALID_ARGUMENT) return 21;
    float f;
    uint8_t u;
    SngReplaySpec spec{0, 1, &f, &f, &f, &u};
    if (replay_spec_check(&spec, &why) != SNG_ERR_INVALID_ARGUMENT || why.find("capacity_days 0") == std::string::npos) return 22;
    spec.capacity_days = -2;
    if (replay_spec_check(&spec, &why) != SNG_ERR_INVALID_ARGUMENT) return 23;
    spec.capacity_days = 1;
    if (replay_spec_check(&spec, &why) != SNG_OK) return 24;
    spec.done = nullptr;
    if (replay_spec_check(&spec, &why) != SNG_ERR_INVALID_ARGUMENT || replay_spec_check(nullptr, &why) != SNG_ERR_INVALID_ARGUMENT)
        return 25;
    return 0;
}

static int check_critic(long &checked) {
    const int nets[][2] = {{8, 8}, {33, 65}, {400, 300}, {512, 512}};
    const int dims[][2] = {{11, 2}, {29, 11}, {109, 51}};
    const int64_t rows = 37;
    int rotation = 0;
    for (const auto &net : nets)
        for (int activation = 0; activation < 2; ++activation) {
            const int H1 = net[0], H2 = net[1];
            const int O = dims[rotation % 3][0], A = dims[rotation % 3][1], K = O + A;
            ++rotation;
            const SngCriticSpec spec{H1, H2, activation};
            std::string why;
            if (H1 == 512 && O == 109) {   // the one combination that does not fit: checked below
                if (critic_spec_check(&spec, O, A, &why) != SNG_ERR_UNSUPPORTED) return 30;
                continue;
            }
            const auto w1 = fill((size_t)H1 * K, 1.f / std::sqrt((float)K)), b1 = fill(H1, 0.3f);
            const auto w2 = fill((size_t)H2 * H1, 1.f / std::sqrt((float)H1)), b2 = fill(H2, 0.3f);
            const auto w3 = fill(H2, 4.f / std::sqrt((float)H2)), b3 = fill(1, 0.3f);
            const SngMlpWeights w{w1.data(), b1.data(), w2.data(), b2.data(), w3.data(), b3.data()};
            if (critic_spec_check(&spec, O, A, &why) != SNG_OK || critic_weights_check(O, A, spec, &w, &why) != SNG_OK) {
                printf("refused: %s\n", why.c_str());
                return 31;
            }
            const NetImage m = critic_image(O, A, spec);
            if (m.O != K || m.A != 1 || m.K1 != net_round_up(K, 8) || m.N3 != 32) return 32;
            std::vector<float> img(m.floats, 7.f), q(rows), y(rows);
            critic_pack(m, O, A, spec, w, img.data());
            const auto obs = fill(rows * O, 1.f), actions = fill(rows * A, 1.f), reward = fill(rows, 40.f);
            std::vector<float> done(rows);
            for (auto &d : done) d = uniform01() < 0.4 ? 1.f : 0.f;
            critic_q_host(m, img.data(), O, A, rows, obs.data(), actions.data(), q.data());
            std::vector<float> x(K), h1(H1), h2(H2);
            for (int64_t r = 0; r < rows; ++r) {
                for (int k = 0; k < O; ++k) x[k] = obs[r * O + k];
                for (int k = 0; k < A; ++k) x[O + k] = actions[r * A + k];
                for (int j = 0; j < H1; ++j) h1[j] = act(activation, chain(x.data(), &w1[(size_t)j * K], K, b1[j]));
                for (int j = 0; j < H2; ++j) h2[j] = act(activation, chain(h1.data(), &w2[(size_t)j * H1], H1, b2[j]));
                const float want = chain(h2.data(), w3.data(), H2, b3[0]);
                if (!same(q[r], want)) {
                    printf("q mismatch %d-%d O=%d act=%d row %lld: %a %a\n", H1, H2, O, activation, (long long)r, q[r], want);
                    return 33;
                }
                ++checked;
            }
            for (double gamma : {0.99, 0.9, 0.0, 1.0}) {
                critic_targets_host(m, img.data(), O, A, rows, obs.data(), actions.data(), reward.data(), done.data(),
                                    gamma, y.data());
                const float g = (float)gamma;
                for (int64_t r = 0; r < rows; ++r) {
                    volatile float nn = 1.0f - done[r];
                    volatile float t = nn * g;
                    t = t * q[r];
                    volatile float want = reward[r] + t;
                    if (!same(y[r], want)) return 34;
                    ++checked;
                }
            }
        }
    // refusals
    std::string why;
    const SngCriticSpec ok{400, 300, 1}, wide{512, 512, 1};
    if (critic_spec_check(&ok, 109, 51, &why) != SNG_OK) return 40;
    if (net_lds_bytes(critic_image(109, 51, ok)) != 147968) return 41;
    if (critic_spec_check(&wide, 109, 51, &why) != SNG_ERR_UNSUPPORTED || why.find("172544") == std::string::npos ||
        why.find("163840") == std::string::npos || why.find("512-512") == std::string::npos ||
        why.find("109 + 51") == std::string::npos)
        return 42;
    if (critic_spec_check(&wide, 29, 11, &why) != SNG_OK) return 43;
    for (int bad : {7, 513}) {
        const SngCriticSpec a{bad, 64, 1}, b{64, bad, 1};
        if (critic_spec_check(&a, 29, 11, &why) != SNG_ERR_UNSUPPORTED || why.find("8 .. 512") == std::string::npos) return 44;
        if (critic_spec_check(&b, 29, 11, &why) != SNG_ERR_UNSUPPORTED || why.find("8 .. 512") == std::string::npos) return 45;
    }
    const SngCriticSpec badact{64, 64, 2};
    if (critic_spec_check(&badact, 29, 11, &why) != SNG_ERR_INVALID_ARGUMENT) return 46;
    if (critic_spec_check(nullptr, 29, 11, &why) != SNG_ERR_INVALID_ARGUMENT) return 47;
    if (critic_spec_check(&ok, 0, 11, &why) != SNG_ERR_INVALID_ARGUMENT || critic_spec_check(&ok, 29, 0, &why) != SNG_ERR_INVALID_ARGUMENT)
        return 48;
    for (double bad : {1.5, -0.01, (double)NAN, (double)INFINITY})
        if (critic_gamma_check(bad, &why) != SNG_ERR_INVALID_ARGUMENT || why.find("gamma") == std::string::npos) return 49;
    if (critic_gamma_check(0.0, &why) != SNG_OK || critic_gamma_check(1.0, &why) != SNG_OK) return 50;
    const SngCriticSpec small{8, 8, 1};
    auto w1 = fill(8 * 5, 1.f), b = fill(8, 1.f), w2 = fill(64, 1.f), w3 = fill(8, 1.f);
    SngMlpWeights w{w1.data(), b.data(), w2.data(), b.data(), w3.data(), b.data()};
    if (critic_weights_check(3, 2, small, &w, &why) != SNG_OK) return 51;
    w1[39] = NAN;
    if (critic_weights_check(3, 2, small, &w, &why) != SNG_ERR_INVALID_ARGUMENT || why != "non-finite critic weight") return 52;
    if (critic_weights_check(3, 2, small, nullptr, &why) != SNG_ERR_INVALID_ARGUMENT) return 53;
    if (critic_blocks(65) != 2 || critic_blocks((int64_t)1 << 40) != (int64_t)1 << 34) return 54;
    return 0;
}

int main() {
    long checked = 0;
    if (int rc = check_sampling(checked)) return rc;
    if (int rc = check_ring(checked)) return rc;
    if (int rc = check_critic(checked)) return rc;
    printf("ddpg host ok: %ld checks\n", checked);
    return 0;
}
