// CPU check of the exact-sum criterion (csrc/sng_exact_sum.h) that day_station_kernel's fast loop decides its rebuild
// path with (tests/test_exact_sum_criterion_cpu.py).
//   exact_sum_check <oracle library>
// Sets of 1 to 10 float32-valued doubles >= +0.0, as charger_step<..., NONNEG> returns them: random and adversarial
// significands, exponent spreads of 0, 24, 25, 26 and 60 between the largest and the smallest positive term, zeros
// mixed in, float32 subnormals, +inf alone and beside finite terms.  Per set:
//   - the criterion answers "rebuild" exactly when two positive terms' binary exponents differ by more than 25 (+inf
//     counts as an exponent above every finite one), and never for a set without two distinct positive exponents;
//   - where it answers "exact", the in-order sum, the reversed sum, every split of the terms into two groups (each
//     summed in order, then added: 2^n splits, the two lanes' among them) and the oracle's pairwise_sum of the
//     positive terms are bit-equal.
// Prints one line per class, "<class> <sets> <exact> <rebuild>", and returns 1 after the first failures.
#include <dlfcn.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "sng_exact_sum.h"

using namespace sng;

typedef double (*PairwiseSum)(const double *, long);
static PairwiseSum oracle_sum;
static int failures;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static int below(int n) { return (int)(rnd() % (uint64_t)n); }

static uint64_t bits(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}
// the float32 value with significand m (24 bits, the top one set) and exponent e in [-126, 127], or for e = -127
// the subnormal m * 2^-149 with m below 2^23; through float, so what comes out is a float32 value by construction
static double f32_value(uint32_t m, int e) {
    const float f = e == -127 ? std::ldexp((float)(m & 0x7fffffu ? m & 0x7fffffu : 1u), -149)
                              : std::ldexp((float)((m & 0x7fffffu) | 0x800000u), e - 23);
    return (double)f;
}

struct Counts {
    long sets = 0, exact = 0, rebuild = 0;
};

static void fail(const char *what, const std::vector<double> &v) {
    if (++failures > 10) return;
    fprintf(stderr, "FAIL %s:", what);
    for (double x : v) fprintf(stderr, " %a", x);
    fprintf(stderr, "\n");
}

// want: 1 the criterion must say rebuild, 0 it must say exact, -1 derive it from the exponents
static void check(const std::vector<double> &v, Counts &c, int want = -1) {
    const int n = (int)v.size();
    uint32_t bmax = kExactSumBmax0, bmin = kExactSumBmin0;
    // as the kernel keeps them: two lanes' own pairs (chargers 0-3 and 8; 4-7 and 9), combined by max and min
    uint32_t lmax[2] = {kExactSumBmax0, kExactSumBmax0}, lmin[2] = {kExactSumBmin0, kExactSumBmin0};
    int emax = 0, emin = 0, npos = 0;
    bool inf = false, finite_pos = false;
    for (int i = 0; i < n; ++i) {
        exact_sum_track(exact_sum_hi(v[i]), bmax, bmin);
        const int lane = (i < 8 ? i / 4 : i - 8) & 1;
        exact_sum_track(exact_sum_hi(v[i]), lmax[lane], lmin[lane]);
        if (!(v[i] > 0.0)) continue;
        if (std::isinf(v[i])) {
            inf = true;
            continue;
        }
        const int e = std::ilogb(v[i]);
        emax = npos ? (e > emax ? e : emax) : e;
        emin = npos ? (e < emin ? e : emin) : e;
        ++npos;
        finite_pos = true;
    }
    const bool rebuild = exact_sum_rebuild(bmax, bmin);
    const uint32_t cmax = lmax[0] > lmax[1] ? lmax[0] : lmax[1], cmin = lmin[0] < lmin[1] ? lmin[0] : lmin[1];
    if (exact_sum_rebuild(cmax, cmin) != rebuild) fail("two lanes' pairs combined differ from one walk", v);
    const bool expect = (inf && finite_pos) || (finite_pos && emax - emin > (int)kExactSumSpread);
    if (rebuild != expect) fail(expect ? "must rebuild, says exact" : "must be exact, says rebuild", v);
    if (want >= 0 && rebuild != (want != 0)) fail("the class's answer", v);
    ++c.sets;
    if (rebuild) {
        ++c.rebuild;
        return;
    }
    ++c.exact;
    double fwd = 0.0, rev = 0.0;
    for (int i = 0; i < n; ++i) fwd += v[i];
    for (int i = n - 1; i >= 0; --i) rev += v[i];
    if (bits(fwd) != bits(rev)) fail("reversed sum", v);
    for (unsigned mask = 0; mask < (1u << n); ++mask) {
        double a = 0.0, b = 0.0;
        for (int i = 0; i < n; ++i) {
            if (mask & (1u << i)) a += v[i];
            else b += v[i];
        }
        if (bits(a + b) != bits(fwd)) {
            fail("a split into two partial sums", v);
            break;
        }
    }
    double pos[10];
    int np = 0;
    for (int i = 0; i < n; ++i)
        if (v[i] > 0.0) pos[np++] = v[i];
    if (bits(oracle_sum(pos, np)) != bits(fwd)) fail("the oracle's pairwise_sum of the positive terms", v);
}

// n terms whose positive exponents span exactly `spread` (two or more positive terms; one: spread 0), lowest
// exponent e0 (-127: float32 subnormals at the bottom); style 0 random significands, 1 all ones, 2 the top term all
// ones and the others with only their lowest bit set besides the leading one, 3 powers of two
static std::vector<double> make_set(int n, int spread, int e0, int style, int zeros_per_8) {
    std::vector<double> v(n);
    const int hi = below(n);
    int lo = below(n);
    if (n > 1 && lo == hi) lo = (hi + 1) % n;
    for (int i = 0; i < n; ++i) {
        int e = e0 + (spread ? below(spread + 1) : 0);
        if (i == hi) e = e0 + spread;
        if (i == lo && n > 1) e = e0;
        if (n == 1) e = e0;
        uint32_t m = (uint32_t)rnd() & 0x7fffffu;
        if (style == 1) m = 0x7fffffu;
        if (style == 2) m = i == hi ? 0x7fffffu : 1u;
        if (style == 3) m = 0u;
        if (e == -127 && (m & 0x7fffffu) == 0u) m = 1u;
        v[i] = f32_value(m, e);
        if (i != hi && i != lo && below(8) < zeros_per_8) v[i] = 0.0;
    }
    return v;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    void *h = dlopen(argv[1], RTLD_NOW);
    if (!h) {
        fprintf(stderr, "%s\n", dlerror());
        return 2;
    }
    oracle_sum = (PairwiseSum)dlsym(h, "orc_pairwise_sum");
    if (!oracle_sum) return 2;
    const int spreads[] = {0, 24, 25, 26, 60};
    for (int spread : spreads) {
        Counts c, sub;
        for (int n = 1; n <= 10; ++n) {
            const int sp = n == 1 ? 0 : spread;
            const int want = sp > (int)kExactSumSpread ? 1 : 0;
            for (int style = 0; style < 4; ++style)
                for (int rep = 0; rep < (style == 0 ? 40 : 8); ++rep) {
                    const int e0 = -126 + below(127 + 126 - sp + 1);   // the top exponent stays at 127 or below
                    check(make_set(n, sp, e0, style, rep % 3 == 0 ? 0 : 3), c, want);
                    // the same with float32 subnormals as the smallest terms (a subnormal's exponent is below -126)
                    const std::vector<double> s = make_set(n, sp, -127, style, rep % 3 == 0 ? 0 : 3);
                    check(s, sub);
                }
        }
        printf("spread%d %ld %ld %ld\n", spread, c.sets, c.exact, c.rebuild);
        printf("subnormal_spread%d %ld %ld %ld\n", spread, sub.sets, sub.exact, sub.rebuild);
    }
    {   // subnormals whose own exponents span 0 .. 22, and the smallest one beside a normal 25 and 26 above it
        Counts c;
        for (int n = 1; n <= 10; ++n)
            for (int rep = 0; rep < 40; ++rep) {
                std::vector<double> v(n);
                for (double &x : v) x = below(4) ? f32_value(1u + ((uint32_t)rnd() % 0x7fffffu), -127) : 0.0;
                check(v, c, 0);
            }
        const double tiny = f32_value(1u, -127);   // 2^-149
        check({tiny, std::ldexp(1.0, -149 + 25)}, c, 0);
        check({tiny, std::ldexp(1.0, -149 + 25) * (2.0 - 0x1p-23), tiny, tiny, tiny, tiny, tiny, tiny, tiny, tiny}, c, 0);
        check({std::ldexp(1.0, -149 + 26), tiny}, c, 1);
        printf("subnormal_only %ld %ld %ld\n", c.sets, c.exact, c.rebuild);
    }
    {   // the largest sums the bound allows: ten all-ones terms at the top exponent and a lowest-bit term 25 below
        Counts c;
        for (int e0 = -126; e0 + 25 <= 127; e0 += 7) {
            std::vector<double> v(10, f32_value(0x7fffffu, e0 + 25));
            for (int i = 0; i < 10; ++i) {
                std::vector<double> w = v;
                w[i] = f32_value(1u, e0);
                check(w, c, 0);
                w[i] = f32_value(1u, e0 - 1 < -126 ? -126 : e0 - 1);
                check(w, c, e0 - 1 < -126 ? 0 : 1);
            }
        }
        printf("adversarial %ld %ld %ld\n", c.sets, c.exact, c.rebuild);
    }
    {   // no positive term; +inf alone, with zeros, twice; +inf beside finite terms
        Counts c;
        const double inf = std::numeric_limits<double>::infinity();
        for (int n = 1; n <= 10; ++n) {
            check(std::vector<double>(n, 0.0), c, 0);
            for (int i = 0; i < n; ++i) {
                std::vector<double> v(n, 0.0);
                v[i] = inf;
                check(v, c, 0);
                if (n > 1) {
                    v[(i + 1) % n] = inf;
                    check(v, c, 0);
                    v[(i + 1) % n] = f32_value((uint32_t)rnd(), -126 + below(254));
                    check(v, c, 1);
                    v[(i + 1) % n] = f32_value(0x7fffffu, 127);   // the largest float32
                    check(v, c, 1);
                    v[(i + 1) % n] = f32_value(1u, -127);
                    check(v, c, 1);
                }
            }
        }
        printf("inf %ld %ld %ld\n", c.sets, c.exact, c.rebuild);
    }
    return failures ? 1 : 0;
}
