"""The day kernel's register and scratch budgets (csrc/sng_step_day.h), read from the gfx950 code object that
libsng.so ships, as tests/test_kernel_resources.py reads the step kernels'.

day_wide_kernel keeps a day's state in registers next to one step's working set, so what the register allocator
does with it decides whether the kernel is worth having: scratch or a VGPR spill puts memory traffic back on the
path the kernel exists to shorten, and fewer than L wavefronts per SIMD (L lanes per env, two) leaves part of the
65,536-env grid waiting for a slot.  The VGPR and SGPR-spill counts of this build are recorded as ceilings (SGPR
spills go to VGPR lanes, not to scratch): a compiler upgrade that moves them fails here, on the CPU.
"""
import os

import pytest

from test_kernel_resources import LIB, LLVM, _mangled, kernel_resources, waves_per_simd

LANES = 2   # kWideLanes

# (REQ, NOISE) -> (VGPRs at most, SGPR spills at most) of this build
CEILINGS = {
    ("false", "false"): (216, 122),
    ("false", "true"): (223, 153),
    ("true", "false"): (238, 130),
    ("true", "true"): (245, 159),
}


@pytest.fixture(scope="module")
def day_kernels(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm-readelf not installed")
    assert os.path.exists(LIB), "build libsng.so first (make -C smart-nanogrid-gym_amd/csrc)"
    res = kernel_resources(LIB, str(tmp_path_factory.mktemp("co")))
    return {n: k for n, k in res.items() if n.startswith("_ZN3sng15day_wide_kernel")}


def test_day_kernel_instantiations(day_kernels):
    """The 10-charger station, with and without the requested-SoC stream and the stochastic profiles."""
    for req, noise in CEILINGS:
        prefix = _mangled("day_wide_kernel", 10, LANES, req, noise)
        assert sum(n.startswith(prefix) for n in day_kernels) == 1, prefix
    assert len(day_kernels) == len(CEILINGS), sorted(day_kernels)


def test_no_day_kernel_spills_and_each_fits_its_wavefronts(day_kernels):
    assert day_kernels
    bad = []
    for n, k in day_kernels.items():
        if k[".private_segment_fixed_size"] != 0 or k.get(".vgpr_spill_count", 0) != 0:
            bad.append(f"{n}: scratch {k['.private_segment_fixed_size']} B, {k.get('.vgpr_spill_count', 0)} VGPR spills")
        w = waves_per_simd(k[".vgpr_count"], k.get(".agpr_count", 0))
        if w < LANES:
            bad.append(f"{n}: {k['.vgpr_count']} VGPRs -> {w} wavefronts per SIMD, at least {LANES}")
    assert not bad, "; ".join(bad)


def test_day_kernel_register_ceilings(day_kernels):
    bad = []
    for (req, noise), (vgprs, sgpr_spills) in CEILINGS.items():
        prefix = _mangled("day_wide_kernel", 10, LANES, req, noise)
        k = next(v for n, v in day_kernels.items() if n.startswith(prefix))
        if k[".vgpr_count"] + k.get(".agpr_count", 0) > vgprs:
            bad.append(f"<10, 2, {req}, {noise}>: {k['.vgpr_count']} VGPRs, at most {vgprs}")
        if k.get(".sgpr_spill_count", 0) > sgpr_spills:
            bad.append(f"<10, 2, {req}, {noise}>: {k['.sgpr_spill_count']} SGPR spills, at most {sgpr_spills}")
    assert not bad, "; ".join(bad)
