// sng_exact_sum.h -- when a sum of an env-step's positive charging powers is exact, decided on the terms' bits.
// HIP-free: day_station_kernel's fast loop (sng_step_wide.h) and tests/native/exact_sum_check.cpp both use it.
//
// Every term is a float32-valued double >= +0.0 (charger_step NONNEG: the float32 product charger.py:92-94, or 0.0),
// at most ten of them.  With e_max and e_min the binary exponents of the largest and the smallest positive term:
//   - every term is a multiple of 2^(e_min - 23): a float32 value has 24 significant bits, a subnormal one fewer;
//   - every sum of some of the terms is below 10 * 2^(e_max + 1) < 2^(e_max + 5);
//   - a double holds every multiple of 2^q below 2^(q + 53).
// So while e_max + 5 <= e_min - 23 + 53, that is e_max - e_min <= 25, every partial sum in every order is exact, and
// an exact sum is numpy's pairwise sum whatever the count of the terms and whichever lane holds them.
// The exponents are read from the terms' high words (float32-valued: the low 29 bits of a double are zero, and the
// float32 subnormals are normal doubles).  A caller keeps
//     bmax = max(bmax, hi)         from 0
//     bmin = min(bmin, hi - 1)     from 0xffffffff: a zero term's hi - 1 wraps to 0xffffffff and drops out
// over the high words `hi` of its terms, combines two lanes' pairs by max and min, and asks exact_sum_rebuild.
// +inf (an overflowed product) has the exponent field 0x7ff, 897 or more above any float32-valued finite term's:
// beside a finite positive term it asks for the rebuild; alone, or with other infinities, the sum is +inf in any
// order.  No positive term at all: bmax = 0, bmin + 1 = 0, no rebuild, and the sum is +0.0.
#pragma once
#include <stdint.h>

#include "sng_layout.h"   // SNG_HD

namespace sng {

constexpr uint32_t kExactSumBmax0 = 0u, kExactSumBmin0 = 0xffffffffu;
constexpr uint32_t kExactSumSpread = 25u;   // e_max - e_min up to which ten terms sum exactly

SNG_HD inline uint32_t exact_sum_hi(double term) {
    uint64_t b;
    __builtin_memcpy(&b, &term, 8);
    return (uint32_t)(b >> 32);
}
SNG_HD inline void exact_sum_track(uint32_t hi, uint32_t &bmax, uint32_t &bmin) {
    bmax = bmax > hi ? bmax : hi;
    bmin = bmin < hi - 1u ? bmin : hi - 1u;
}
// true: the running sum is not known to be exact, sum the positive terms again in numpy's order
SNG_HD inline bool exact_sum_rebuild(uint32_t bmax, uint32_t bmin) {
    return (bmax >> 20) > ((bmin + 1u) >> 20) + kExactSumSpread;
}

}  // namespace sng
