"""action_noise_kernel<KIND> (csrc/sng_noise.h): its register, scratch and LDS budgets read from the gfx950 code object
that libsng.so ships, as tests/test_ppo_net_kernel_resources.py reads the net head's kernels'.

The kernel is a stream of stores behind a little arithmetic: per element and step a hash, one 16-byte LDS read and a
few VALU operations, four elements a thread.  Scratch or a VGPR spill would put memory traffic between them; its LDS is
the coefficient table alone (1,984 B, static), far below what would limit the workgroups of a compute unit; and it wants
the hardware's eight wavefronts per SIMD to hide the store stream's latency: at most 64 registers.  The VGPR counts of
this build are recorded as ceilings: a compiler upgrade that moves them fails here, on the CPU."""
import os

import pytest

from test_kernel_resources import LIB, LLVM, _mangled, kernel_resources, waves_per_simd

# template argument (SNG_NOISE_GAUSSIAN 0, SNG_NOISE_OU 1) -> .vgpr_count at most: this build's counts
NOISE = {"0": 46, "1": 54}
TABLE_BYTES = 31 * 4 * 4 * 4


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm-readelf not installed")
    assert os.path.exists(LIB), "build libsng.so first (make -C smart-nanogrid-gym_amd/csrc)"
    return kernel_resources(LIB, str(tmp_path_factory.mktemp("co")))


def named(kernels, name):
    return {n: k for n, k in kernels.items() if n.startswith(f"_ZN3sng{len(name)}{name}")}


def test_instantiations(kernels):
    mine = named(kernels, "action_noise_kernel")
    for arg in NOISE:
        assert sum(n.startswith(_mangled("action_noise_kernel", arg)) for n in mine) == 1, arg
    assert len(mine) == len(NOISE) == 2, sorted(mine)
    assert len(named(kernels, "noise_bump_kernel")) == 1


def test_no_scratch_no_spills_small_lds(kernels):
    bad = []
    for n, k in named(kernels, "action_noise_kernel").items():
        if k[".private_segment_fixed_size"] != 0 or k.get(".vgpr_spill_count", 0) != 0:
            bad.append(f"{n}: scratch {k['.private_segment_fixed_size']} B, {k.get('.vgpr_spill_count', 0)} VGPR spills")
        if k.get(".sgpr_spill_count", 0) != 0:
            bad.append(f"{n}: {k['.sgpr_spill_count']} SGPR spills")
        if k[".group_segment_fixed_size"] != TABLE_BYTES or k[".group_segment_fixed_size"] >= 4096:
            bad.append(f"{n}: {k['.group_segment_fixed_size']} B of static LDS, not the table's {TABLE_BYTES}")
        if k[".max_flat_workgroup_size"] != 256:
            bad.append(f"{n}: workgroups of {k['.max_flat_workgroup_size']}, not 256")
    assert not bad, "; ".join(bad)


def test_occupancy_and_register_ceilings(kernels):
    bad = []
    for arg, vgprs in NOISE.items():
        k = next(v for n, v in kernels.items() if n.startswith(_mangled("action_noise_kernel", arg)))
        if waves_per_simd(k[".vgpr_count"], k.get(".agpr_count", 0)) < 8:
            bad.append(f"action_noise_kernel<{arg}>: {k['.vgpr_count']} registers: fewer than 8 wavefronts per SIMD")
        if k[".vgpr_count"] > vgprs:
            bad.append(f"action_noise_kernel<{arg}>: {k['.vgpr_count']} registers, at most {vgprs}")
    assert not bad, "; ".join(bad)
