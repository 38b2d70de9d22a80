/* Exhaustive check of the two fma-based divisions in the step kernels (csrc/sng_dev_env.h).
 *
 * 1. div_by_cap: for float32-valued x and integer c in [1, 255], r = fl(1/c),
 *        q = x*r;  q' = fma(min(fma(-q, c, x), q), r, q)   ==   x / c   (IEEE float64)
 *    Every operation scales exactly by 2^k (a float32-valued x neither underflows nor overflows in
 *    float64), so checking every float32 mantissa in the binade [1, 2) against every c covers every
 *    finite float32 x >= 0; the kernel divides magnitudes and gives the quotient its sign after.
 *    2^23 * 255 = 2.1e9 cases.  The min passes every finite remainder (it is far below q) and makes the
 *    quotient of x = +inf (an action whose float32 charging product overflows) +inf, where the plain
 *    form gives inf - inf = NaN; +0, the largest and the smallest float32, +inf and NaN are checked for
 *    every c as well.
 * 2. departure_obs: d in [0, 255], float32 q = d*(1/24); fmaf(fmaf(-q, 24, d), 1/24, q)
 *    == (float)((double)d / 24)  (the reference's float64 quotient rounded to float32).
 *
 *    gcc -O2 -ffp-contract=off -fopenmp tools/check_division.c -o /tmp/check_division -lm && /tmp/check_division
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

int main(void) {
    long long bad = 0, total = 0;
    for (int c = 1; c < 256; ++c) {
        const double cd = (double)c, r = 1.0 / cd;
        long long bad_c = 0;
#pragma omp parallel for reduction(+ : bad_c)
        for (uint32_t m = 0; m < (1u << 23); ++m) {
            const uint32_t bits = 0x3f800000u | m;
            float xf;
            memcpy(&xf, &bits, 4);
            const double x = (double)xf;
            const double q = x * r;
            const double qq = fma(fmin(fma(-q, cd, x), q), r, q);
            if (qq != x / cd) ++bad_c;
        }
        const double edge[5] = {0.0, (double)FLT_MAX, (double)(FLT_MIN * FLT_EPSILON), INFINITY, NAN};
        for (int k = 0; k < 5; ++k) {
            const double x = edge[k], q = x * r;
            const double qq = fma(fmin(fma(-q, cd, x), q), r, q);
            if (isnan(x) ? !isnan(qq) : (qq != x / cd || signbit(qq) != signbit(x / cd))) ++bad_c;
        }
        bad += bad_c;
        total += 1ll << 23;
    }
    printf("div_by_cap: %lld cases, %lld mismatches\n", total, bad);

    int bad_d = 0;
    const float r24 = 1.0f / 24.0f;
    for (int d = 0; d < 256; ++d) {
        const float df = (float)d;
        const float q = df * r24;
        const float qq = fmaf(fmaf(-q, 24.0f, df), r24, q);
        if (qq != (float)((double)d / 24.0)) ++bad_d;
    }
    printf("departure_obs: 256 cases, %d mismatches\n", bad_d);
    return (bad || bad_d) ? 1 : 0;
}
