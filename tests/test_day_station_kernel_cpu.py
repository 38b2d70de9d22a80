"""day_station_kernel (csrc/sng_step_day.h) on the CPU: which handles it is selected for, and its register and scratch
budgets, read from the gfx950 code object that libsng.so ships as tests/test_day_kernel_resources.py reads
day_wide_kernel's.

The selection is one host-only predicate (csrc/sng_step_plan.h, day_station_fixed).  tests/native/
day_station_check.cpp, built with g++, makes the library's own Params of a configuration and a loaded day and asks it:
true for the headline station's generated days, false with any one fixed fact flipped, and over the station matrix
true for the one row that is that station.  A 2 h or a 15 min day keeps a power-of-two dt but has T = 12 or 96: the
kernel fixes T = 24 (its `done` compares with the constant), and only the 1 h day was measured, so those days keep
the generic kernel.

The kernel exists to hold less in scalar registers than day_wide_kernel<10, 2, false, false>, so its SGPR spills must
stay strictly below that instantiation's in the same code object; the counts of this build are recorded as ceilings.
"""
import os
import shutil
import subprocess

import pytest

from station_matrix_cases import ROWS, UNBOUNDED
from test_kernel_resources import LIB, LLVM, _mangled, kernel_resources, waves_per_simd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smart-nanogrid-gym_amd", "csrc")
SYMBOL = "_ZN3sng18day_station_kernel"
LANES = 2   # kWideLanes
VGPRS_AT_MOST, SGPR_SPILLS_AT_MOST = 181, 73   # this build's

FLIPPED = ["unbounded", "v2x", "no_pv", "no_bess", "legacy", "requested_soc", "noise", "replayed",
           "replayed_requested_soc", "host_day", "day_2h", "day_15min", "day_20min", "diagnostics", "two_lanes",
           "n1", "n2", "n4", "n8", "n9", "n11", "n16", "n50"]
HOURS = {"15min": 0.25, "20min": 1 / 3, "30min": 0.5, "1h": 1.0, "2h": 2.0, "4h": 4.0}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    path = str(tmp_path_factory.mktemp("station") / "day_station_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "day_station_check.cpp"), "-o", path], check=True)
    return path


def test_headline_is_fixed_and_every_flipped_fact_is_not(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    rows = {name: tuple(int(x) for x in rest) for name, *rest in (line.split() for line in out.stdout.splitlines())}
    assert rows.pop("headline") == (1, 1, 0)   # fixed, selected by default, not under generic_day
    assert sorted(rows) == sorted(FLIPPED)
    for name, got in rows.items():
        assert got == (0, 0, 0), (name, got)


def station_args(row):
    kw = row.kw
    return [str(kw["number_of_chargers"]), repr(HOURS[kw["time_interval"]]),
            *(str(int(bool(x))) for x in (
                kw["pv_system_available_in_model"], kw["battery_system_available_in_model"],
                kw["charging_mode"] == "bounded", kw.get("vehicle_to_everything", False),
                kw.get("numpy_legacy_promotion", False), kw.get("enable_requested_state_of_charge", False),
                kw.get("pv_noise", 0) > 0 or kw.get("price_noise", 0) > 0, row.rng == "device", False))]


def test_station_matrix_rows(exe):
    """Of the matrix, the 1 h station with PV and a BESS is the kernel's (its penalty mode and cost weight are not
    among the fixed facts); every other row, the unbounded station included, keeps its kernel."""
    got = {}
    for row in ROWS + [UNBOUNDED]:
        out = subprocess.run([exe, *station_args(row)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (row.name, out.returncode, out.stderr)
        got[row.name] = int(out.stdout)
    assert [n for n, v in got.items() if v] == ["day10_nopen_gridw"], got


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm llvm-readelf not installed")
    assert os.path.exists(LIB), "build libsng.so first (make -C smart-nanogrid-gym_amd/csrc)"
    return kernel_resources(LIB, str(tmp_path_factory.mktemp("co")))


def test_station_kernel_budgets(resources):
    names = [n for n in resources if n.startswith(SYMBOL)]
    assert names == [n for n in names if n.startswith(_mangled("day_station_kernel", 10, LANES))] and len(names) == 1, names
    k = resources[names[0]]
    assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, k
    vgprs = k[".vgpr_count"] + k.get(".agpr_count", 0)
    assert waves_per_simd(k[".vgpr_count"], k.get(".agpr_count", 0)) >= LANES, vgprs
    assert vgprs <= VGPRS_AT_MOST, vgprs
    spills = k.get(".sgpr_spill_count", 0)
    assert spills <= SGPR_SPILLS_AT_MOST, spills
    generic = [v for n, v in resources.items() if n.startswith(_mangled("day_wide_kernel", 10, LANES, "false", "false"))]
    assert len(generic) == 1
    assert spills < generic[0].get(".sgpr_spill_count", 0), (spills, generic[0].get(".sgpr_spill_count", 0))
    # the compact arguments: less than half the generic kernel's kernarg segment
    assert 2 * k[".kernarg_segment_size"] < generic[0][".kernarg_segment_size"]
