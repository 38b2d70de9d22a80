#!/usr/bin/env python3
"""Fits the inverse-CDF table of the action noise (csrc/sng_noise_host.h, kNoiseIcdf) and prints it as C.

The variate of a 32-bit hash h (include/sng.h, "Action noise"): u = max(h & 0x7fffffff, 1), p = (u + 0.5) 2^-32 in
(0, 0.5); octave k = 30 - msb(u); the bits below u's leading one, left-aligned, give a 2-bit sub-segment s and a 24-bit
fraction x in [0, 1).  Segment (k, s) therefore covers u = 2^(30 - k) (1 + (s + x) / 4), and the table holds, per segment,
the cubic r(x) ~ -ndtri(p) in float32 (c0, c1, c2, c3), evaluated as fmaf(fmaf(fmaf(c3, x, c2), x, c1), x, c0).

Fit: least squares against float64 scipy.special.ndtri on 64 Chebyshev nodes per segment, coefficients rounded to
float32.  `--check` evaluates the rounded table exactly as the library does (float32 fmaf emulated in float64, which
is exact for one fma of float32 operands up to the final rounding) over every u < 65,536, 2^14 evenly spaced u per
octave and 2^22 random h, and prints the largest |z - ndtri(p)|.

    python tools/fit_noise_table.py            # the C initialiser, on stdout
    python tools/fit_noise_table.py --check    # and the measured error, on stderr
"""
import sys

import numpy as np
from scipy.special import ndtri

OCTAVES, SUBS, NODES = 31, 4, 64


def segment_p(k, s, x):
    """p of fraction x (float64, [0, 1)) in sub-segment s of octave k."""
    u = np.ldexp(1.0 + (s + x) / 4.0, 30 - k)
    return (u + 0.5) * 2.0 ** -32


def fit():
    i = np.arange(NODES)
    x = 0.5 - 0.5 * np.cos((2 * i + 1) * np.pi / (2 * NODES))   # Chebyshev nodes of [0, 1]
    V = np.vander(x, 4, increasing=True)
    tab = np.zeros((OCTAVES, SUBS, 4), np.float32)
    for k in range(OCTAVES):
        for s in range(SUBS):
            r = -ndtri(segment_p(k, s, x))
            c, *_ = np.linalg.lstsq(V, r, rcond=None)
            tab[k, s] = c.astype(np.float32)
    return tab


def fma32(a, b, c):
    """float32 fmaf of float32 arrays: the product of two float32 is exact in float64 and the sum of it and a float32
    is rounded once to float64, then to float32 -- double rounding could differ from fmaf in rare ties, so this is the
    script's estimate; tests/test_action_noise_cpu.py measures the library itself."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def variate(tab, h):
    h = h.astype(np.uint32)
    u = np.maximum(h & np.uint32(0x7fffffff), np.uint32(1)).astype(np.uint64)
    msb = np.floor(np.log2(u.astype(np.float64))).astype(np.int64)
    msb = np.where((np.uint64(1) << msb.astype(np.uint64)) > u, msb - 1, msb)
    k = 30 - msb
    w = ((u << (32 - msb).astype(np.uint64)) & np.uint64(0xffffffff)).astype(np.uint64)   # below the leading one
    s = (w >> np.uint64(30)).astype(np.int64)
    x = ((w >> np.uint64(6)) & np.uint64(0xffffff)).astype(np.float32) * np.float32(2.0 ** -24)
    c = tab[k, s]
    r = fma32(fma32(fma32(c[:, 3], x, c[:, 2]), x, c[:, 1]), x, c[:, 0])
    r = np.maximum(r, np.float32(2.0 ** -32))
    z = np.where(h >> np.uint32(31), -r, r)
    p = (u.astype(np.float64) + 0.5) * 2.0 ** -32
    want = np.where(h >> np.uint32(31), ndtri(p), -ndtri(p))
    return z, want


def check(tab):
    rng = np.random.default_rng(0)
    worst = 0.0
    sets = [np.arange(65536, dtype=np.uint32), rng.integers(0, 2 ** 32, 1 << 22, dtype=np.uint64).astype(np.uint32)]
    for k in range(OCTAVES):
        lo = 1 << (30 - k)
        sets.append(np.unique((lo + np.arange(1 << 14) * (lo / float(1 << 14))).astype(np.uint32)))
    zmax = 0.0
    for h in sets:
        for sign in (0, 0x80000000):
            z, want = variate(tab, h | np.uint32(sign))
            worst = max(worst, float(np.max(np.abs(z.astype(np.float64) - want))))
            zmax = max(zmax, float(np.max(np.abs(z))))
    print(f"max |z - ndtri(p)| = {worst:.3e} (bound 2^-18 = {2.0 ** -18:.3e}), max |z| = {zmax:.4f}", file=sys.stderr)


def hexf(v):
    mant, exp = float(v).hex().split("p")
    mant = mant.rstrip("0")
    return f"{mant}{'0' if mant.endswith('.') else ''}p{exp}f,"


def main():
    tab = fit()
    print("// [octave][sub-segment][c0 c1 c2 c3]: tools/fit_noise_table.py")
    print("constexpr float kNoiseIcdf[kNoiseOctaves * kNoiseSubs * 4] = {")
    for k in range(OCTAVES):
        for s in range(SUBS):
            print("    " + " ".join(hexf(v) for v in tab[k, s]) + ("   // octave %d" % k if s == 0 else ""))
    print("};")
    if "--check" in sys.argv:
        check(tab)


if __name__ == "__main__":
    main()
