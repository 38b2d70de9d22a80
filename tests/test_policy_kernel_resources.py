"""The policy kernels (csrc/sng_policy.h): policy_kernel<TANH> and day_lean_policy_kernel<NC, PK, REQ>, their
register and scratch budgets read from the gfx950 code object that libsng.so ships, as
tests/test_day_lean_kernel_resources.py reads day_lean_kernel's.

policy_kernel keeps a wavefront's 16 chains of a layer in registers and takes its weights as scalar operands; the
fused day keeps a hidden layer's 64 chains next to day_lean_kernel's working set.  Scratch or a VGPR spill would put
memory traffic into the inner loops: an instantiation that had either would be left out of policy_day_compiled
(csrc/sng_step_plan.h) and its plan would keep nodes.  None has; the fused day is compiled exactly where
day_lean_kernel is.  SGPR spills go to VGPR lanes, not to scratch.  The VGPR counts of this build are recorded as
ceilings: a compiler upgrade that moves them fails here, on the CPU.
"""
import os

import pytest

from test_day_lean_kernel_resources import CEILINGS as DAY_LEAN
from test_kernel_resources import LIB, LLVM, _mangled, kernel_resources, waves_per_simd

# TANH -> .vgpr_count + .agpr_count at most: this build's counts
POLICY = {"false": 67, "true": 67}

# (NC, PK, REQ) -> the unified file's total (.vgpr_count, AGPRs included) at most: this build's counts
FUSED = {
    (1, "false", "false"): 162, (1, "false", "true"): 162, (1, "true", "false"): 161,
    (2, "false", "false"): 168, (2, "false", "true"): 174, (2, "true", "false"): 165, (2, "true", "true"): 167,
    (4, "false", "false"): 194, (4, "false", "true"): 208, (4, "true", "false"): 179, (4, "true", "true"): 189,
    (8, "false", "false"): 238, (8, "false", "true"): 258, (8, "true", "false"): 205, (8, "true", "true"): 230,
    (10, "false", "false"): 254, (10, "false", "true"): 286, (10, "true", "false"): 211, (10, "true", "true"): 245,
    (16, "false", "false"): 330, (16, "false", "true"): 394, (16, "true", "false"): 255, (16, "true", "true"): 325,
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm-readelf not installed")
    assert os.path.exists(LIB), "build libsng.so first (make -C smart-nanogrid-gym_amd/csrc)"
    res = kernel_resources(LIB, str(tmp_path_factory.mktemp("co")))
    return ({n: k for n, k in res.items() if n.startswith("_ZN3sng13policy_kernel")},
            {n: k for n, k in res.items() if n.startswith("_ZN3sng22day_lean_policy_kernel")})


def test_instantiations(kernels):
    """policy_kernel for tanh and relu; the fused day for exactly the plans that have day_lean_kernel."""
    policy, fused = kernels
    for tanh in POLICY:
        assert sum(n.startswith(_mangled("policy_kernel", tanh)) for n in policy) == 1, tanh
    assert len(policy) == len(POLICY), sorted(policy)
    assert set(FUSED) == set(DAY_LEAN)
    for key in FUSED:
        assert sum(n.startswith(_mangled("day_lean_policy_kernel", *key)) for n in fused) == 1, key
    assert len(fused) == len(FUSED), sorted(fused)


def test_no_scratch_no_spills_and_each_fits_a_wavefront_per_simd(kernels):
    policy, fused = kernels
    assert policy and fused
    bad = []
    for n, k in {**policy, **fused}.items():
        if k[".private_segment_fixed_size"] != 0 or k.get(".vgpr_spill_count", 0) != 0:
            bad.append(f"{n}: scratch {k['.private_segment_fixed_size']} B, {k.get('.vgpr_spill_count', 0)} VGPR spills")
        # .vgpr_count is the unified file's total, AGPRs included (tests/test_day_lean_kernel_resources.py)
        if waves_per_simd(k[".vgpr_count"]) < 1:
            bad.append(f"{n}: {k['.vgpr_count']} registers ({k.get('.agpr_count', 0)} of them AGPRs) do not fit a SIMD")
    assert not bad, "; ".join(bad)


def test_register_ceilings(kernels):
    policy, fused = kernels
    bad = []
    for tanh, vgprs in POLICY.items():
        k = next(v for n, v in policy.items() if n.startswith(_mangled("policy_kernel", tanh)))
        if k[".vgpr_count"] > vgprs:
            bad.append(f"policy_kernel<{tanh}>: {k['.vgpr_count']} VGPRs + {k.get('.agpr_count', 0)} AGPRs, at most {vgprs}")
    for key, vgprs in FUSED.items():
        k = next(v for n, v in fused.items() if n.startswith(_mangled("day_lean_policy_kernel", *key)))
        if k[".vgpr_count"] > vgprs:
            bad.append(f"day_lean_policy_kernel<{key}>: {k['.vgpr_count']} VGPRs ({k.get('.agpr_count', 0)} of them "
                       f"AGPRs), at most {vgprs}")
    assert not bad, "; ".join(bad)
