"""learn_gemm_kernel<EPI>, learn_loss_kernel<ACTOR>, learn_step_kernel<ADAM> and learn_concat_kernel
(csrc/sng_ddpg_learn.h): their register and scratch budgets read from the gfx950 code object that libsng.so ships, as
tests/test_ddpg_kernel_resources.py reads q_net_kernel's.

learn_gemm_kernel keeps one 16-register accumulator and two batches of eight operands in flight: scratch or a VGPR
spill would put memory traffic between its MFMAs.  The other three are elementwise.  The ceilings are this build's
counts (.vgpr_count, AGPRs included)."""
import os

import pytest

from test_kernel_resources import LIB, LLVM, kernel_resources, waves_per_simd

LOSS_VGPRS, LOSS_LDS = 26, (64 * 65 + 64) * 4   # 64 segments' tiles of 64 rows in rows of 65 floats, and the partials
# mangled prefix -> (what it is, register ceiling, static LDS in bytes)
KERNELS = {
    **{f"_ZN3sng17learn_gemm_kernelILi{e}EEE": (f"learn_gemm_kernel<{e}>", 64, 0) for e in range(5)},
    "_ZN3sng17learn_loss_kernelILb0EEE": ("learn_loss_kernel<false>", LOSS_VGPRS, LOSS_LDS),
    "_ZN3sng17learn_loss_kernelILb1EEE": ("learn_loss_kernel<true>", LOSS_VGPRS, LOSS_LDS),
    "_ZN3sng17learn_step_kernelILb0EEE": ("learn_step_kernel<false>", 24, 0),
    "_ZN3sng17learn_step_kernelILb1EEE": ("learn_step_kernel<true>", 34, 0),
    "_ZN3sng19learn_concat_kernelE": ("learn_concat_kernel", 19, 0),
}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm-readelf not installed")
    assert os.path.exists(LIB), "build libsng.so first (make -C smart-nanogrid-gym_amd/csrc)"
    return kernel_resources(LIB, str(tmp_path_factory.mktemp("co")))


def test_every_instantiation_is_found_once(resources):
    for prefix, (name, _, _) in KERNELS.items():
        assert sum(n.startswith(prefix) for n in resources) == 1, name
    # and the library has no other kernel of these stems
    for stem, count in (("_ZN3sng17learn_gemm_kernel", 5), ("_ZN3sng17learn_loss_kernel", 2),
                        ("_ZN3sng17learn_step_kernel", 2), ("_ZN3sng19learn_concat_kernel", 1)):
        assert sum(n.startswith(stem) for n in resources) == count, stem
    assert sum("learn_" in n for n in resources) == len(KERNELS)


def test_no_scratch_no_spills_and_register_ceilings(resources):
    bad = []
    for prefix, (name, vgprs, lds) in KERNELS.items():
        k = next(v for n, v in resources.items() if n.startswith(prefix))
        if k[".private_segment_fixed_size"] != 0 or k.get(".vgpr_spill_count", 0) != 0:
            bad.append(f"{name}: scratch {k['.private_segment_fixed_size']} B, {k.get('.vgpr_spill_count', 0)} VGPR spills")
        if k[".vgpr_count"] > vgprs:
            bad.append(f"{name}: {k['.vgpr_count']} registers ({k.get('.agpr_count', 0)} of them AGPRs), at most {vgprs}")
        if waves_per_simd(k[".vgpr_count"]) < 1:
            bad.append(f"{name}: {k['.vgpr_count']} registers do not fit a SIMD")
        if k[".group_segment_fixed_size"] != lds:
            bad.append(f"{name}: {k['.group_segment_fixed_size']} B of static LDS, not {lds}")
        if k[".max_flat_workgroup_size"] != 256:
            bad.append(f"{name}: workgroups of {k['.max_flat_workgroup_size']}, not four wavefronts")
    assert not bad, "; ".join(bad)


def test_the_trunk_kernels_are_what_they_were(resources):
    """The learner adds no instantiation of the kernels whose images it rewrites."""
    for stem, count in (("_ZN3sng12q_net_kernel", 4), ("_ZN3sng17policy_net_kernel", 2), ("_ZN3sng16value_net_kernel", 2)):
        assert sum(n.startswith(stem) for n in resources) == count, stem
