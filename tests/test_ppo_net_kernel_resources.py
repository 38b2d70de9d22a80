"""value_net_kernel<TANH> and gae_scan_kernel<LOGP> (csrc/sng_ppo_net.h): their register, scratch and LDS budgets read
from the gfx950 code object that libsng.so ships, as tests/test_ppo_kernel_resources.py reads rollout_gae_kernel's.

value_net_kernel is policy_net_kernel's structure with another output stage: two 16-register accumulators and a ring
of six 16-byte weight groups in flight, one workgroup of four wavefronts per compute unit (its dynamic LDS sets that),
so scratch or a VGPR spill would put memory traffic between the MFMAs and a wavefront per SIMD must fit.
gae_scan_kernel is one wavefront a workgroup; it keeps kScanAhead = 8 steps' reward, done and V in registers ahead of
the recurrence, and is latency bound, so it wants many wavefronts on a SIMD: at most 64 registers keep eight.  The
VGPR counts of this build are recorded as ceilings: a compiler upgrade that moves them fails here, on the CPU."""
import os

import pytest

from test_kernel_resources import LIB, LLVM, _mangled, kernel_resources, waves_per_simd

# template argument -> .vgpr_count (the unified file's total, AGPRs included) at most: this build's counts
VALUE = {"false": 112, "true": 112}
SCAN = {"false": 44, "true": 44}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm-readelf not installed")
    assert os.path.exists(LIB), "build libsng.so first (make -C smart-nanogrid-gym_amd/csrc)"
    return kernel_resources(LIB, str(tmp_path_factory.mktemp("co")))


def named(kernels, name):
    return {n: k for n, k in kernels.items() if n.startswith(f"_ZN3sng{len(name)}{name}")}


def test_instantiations(kernels):
    for name, table in (("value_net_kernel", VALUE), ("gae_scan_kernel", SCAN)):
        mine = named(kernels, name)
        for arg in table:
            assert sum(n.startswith(_mangled(name, arg)) for n in mine) == 1, (name, arg)
        assert len(mine) == len(table) == 2, sorted(mine)


def test_no_scratch_no_spills(kernels):
    bad = []
    for name, block in (("value_net_kernel", 256), ("gae_scan_kernel", 64)):
        mine = named(kernels, name)
        assert mine
        for n, k in mine.items():
            if k[".private_segment_fixed_size"] != 0 or k.get(".vgpr_spill_count", 0) != 0:
                bad.append(f"{n}: scratch {k['.private_segment_fixed_size']} B, {k.get('.vgpr_spill_count', 0)} VGPR spills")
            if k[".group_segment_fixed_size"] != 0:
                bad.append(f"{n}: {k['.group_segment_fixed_size']} B of static LDS: the tiles are dynamic")
            if k[".max_flat_workgroup_size"] != block:
                bad.append(f"{n}: workgroups of {k['.max_flat_workgroup_size']}, not {block}")
    assert not bad, "; ".join(bad)


def test_occupancy(kernels):
    for n, k in named(kernels, "value_net_kernel").items():
        assert waves_per_simd(k[".vgpr_count"]) >= 1, n
    for n, k in named(kernels, "gae_scan_kernel").items():
        assert waves_per_simd(k[".vgpr_count"]) >= 8, (n, k[".vgpr_count"])


def test_register_ceilings(kernels):
    bad = []
    for name, table in (("value_net_kernel", VALUE), ("gae_scan_kernel", SCAN)):
        for arg, vgprs in table.items():
            k = next(v for n, v in kernels.items() if n.startswith(_mangled(name, arg)))
            if k[".vgpr_count"] > vgprs:
                bad.append(f"{name}<{arg}>: {k['.vgpr_count']} registers ({k.get('.agpr_count', 0)} of them AGPRs), "
                           f"at most {vgprs}")
    assert not bad, "; ".join(bad)
