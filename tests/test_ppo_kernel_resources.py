"""rollout_gae_kernel<TANH> (csrc/sng_ppo.h): its register and scratch budgets read from the gfx950 code object that
libsng.so ships, as tests/test_policy_kernel_resources.py reads the policy kernels'.

The kernel keeps a wavefront's 16 chains of a hidden layer, the prefetched observation tile of the step before (up to
8 float4 a thread) and the step's noise tile (2) in registers, and takes its weights as scalar operands.  Scratch or a
VGPR spill would put memory traffic into the chains.  SGPR spills go to VGPR lanes, not to scratch.  At most 128
registers keep four wavefronts on a SIMD, which is what the LDS of a station of up to 10 chargers admits (four
workgroups of four wavefronts a compute unit).  The VGPR counts of this build are recorded as ceilings: a compiler
upgrade that moves them fails here, on the CPU.
"""
import os

import pytest

from test_kernel_resources import LIB, LLVM, _mangled, kernel_resources, waves_per_simd

# TANH -> .vgpr_count (the unified file's total, AGPRs included) at most: this build's counts
ROLLOUT = {"false": 122, "true": 124}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm-readelf not installed")
    assert os.path.exists(LIB), "build libsng.so first (make -C smart-nanogrid-gym_amd/csrc)"
    res = kernel_resources(LIB, str(tmp_path_factory.mktemp("co")))
    return {n: k for n, k in res.items() if n.startswith("_ZN3sng18rollout_gae_kernel")}


def test_exactly_two_instantiations(kernels):
    for tanh in ROLLOUT:
        assert sum(n.startswith(_mangled("rollout_gae_kernel", tanh)) for n in kernels) == 1, tanh
    assert len(kernels) == len(ROLLOUT) == 2, sorted(kernels)


def test_no_scratch_no_spills_and_four_wavefronts_per_simd(kernels):
    assert kernels
    bad = []
    for n, k in kernels.items():
        if k[".private_segment_fixed_size"] != 0 or k.get(".vgpr_spill_count", 0) != 0:
            bad.append(f"{n}: scratch {k['.private_segment_fixed_size']} B, {k.get('.vgpr_spill_count', 0)} VGPR spills")
        if waves_per_simd(k[".vgpr_count"]) < 4:
            bad.append(f"{n}: {k['.vgpr_count']} registers ({k.get('.agpr_count', 0)} of them AGPRs): fewer than four "
                       "wavefronts per SIMD")
    assert not bad, "; ".join(bad)


def test_register_ceilings(kernels):
    bad = []
    for tanh, vgprs in ROLLOUT.items():
        k = next(v for n, v in kernels.items() if n.startswith(_mangled("rollout_gae_kernel", tanh)))
        if k[".vgpr_count"] > vgprs:
            bad.append(f"rollout_gae_kernel<{tanh}>: {k['.vgpr_count']} VGPRs ({k.get('.agpr_count', 0)} of them AGPRs), "
                       f"at most {vgprs}")
    assert not bad, "; ".join(bad)
