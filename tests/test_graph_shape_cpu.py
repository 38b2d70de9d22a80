"""The shape of a captured reset graph (csrc/sng_step_plan.h: reset_overlapped, day_shape), listed on the CPU by
tests/native/graph_shape_check.cpp for every configuration of the step-plan table.

Which graphs generate day d + 1 beside day d's steps is one host-only decision: two days or more, no kept
trajectory, no SNG_GRAPH_SERIAL_RESET, a device reset that is one launch (the t = 0 observation tile of the
generator's extra blocks within 32 KB), and a plan whose day measured shorter that way or
SNG_GRAPH_OVERLAPPED_RESET.  The day slots rotate so that the last day of a replay is always in the
handle's own buffers (slot 0), and the day counter advances by `days` per replay in both forms, with the same day
indices drawn.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smart-nanogrid-gym_amd", "csrc")
DAYS = range(1, 6)
OVERLAPPING = ("void sng::step_wide_kernel<10,",)


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    assert shutil.which("g++"), "g++ builds the host-only check"
    exe = str(tmp_path_factory.mktemp("shape") / "graph_shape_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "graph_shape_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr)
    plans, shapes = [], {}
    for line in out.stdout.splitlines():
        parts = [x.strip() for x in line.split("|")]
        head = parts[0].split()
        if head[0] == "plan":
            fused, lds = (int(x) for x in parts[2].split())
            plans.append((tuple(int(x) for x in head[1:]), parts[1], fused, lds, parts[3].split()))
        else:
            assert head[0] == "shape"
            shapes[tuple(int(x) for x in head[1:])] = tuple(int(x) for x in parts[1].split())
    return plans, shapes


def test_overlap_decision_for_every_plan(listing):
    plans, _ = listing
    assert len(plans) > 2000 and len({p[1] for p in plans}) > 50   # the whole table, many kernels
    fused_n, overlapping = set(), set()
    for key, kernel, fused, lds, flags in plans:
        n = key[0]
        assert fused == int((64 * (2 * n + 9) + 3) // 4 * 4 * 4 <= 32 * 1024), key
        if fused:
            fused_n.add(n)
        # the plans whose day measured shorter overlapped: the wide 10-charger station
        faster = kernel.startswith(OVERLAPPING)
        # a capped generator beside the wide family's day: two 56 KB workgroups and the day's 40 KB of tiles fill
        # a CU's 160 KB, and a workgroup may ask for 64 KB at most without an attribute
        assert lds == (56 * 1024 if "step_wide_kernel" in kernel else 0), key
        assert 2 * lds + 40 * 1024 <= 160 * 1024 < 3 * lds + 40 * 1024 or lds == 0
        assert len(flags) == len(DAYS)
        for days, eight in zip(DAYS, flags):
            # (trajectory, serial) = (0, 0), (0, 1), (1, 0), (1, 1): only the first can overlap; by default where
            # it measured faster, with SNG_GRAPH_OVERLAPPED_RESET (the last four) wherever the reset is one launch
            can = fused and days >= 2
            assert eight == ("1000" if can and faster else "0000") + ("1000" if can else "0000"), (key, kernel, days)
            if eight[0] == "1":
                overlapping.add(kernel)
    assert fused_n == {1, 2, 3, 4, 5, 8, 10, 16, 17, 50}   # config 5's 50 chargers included, 128 not
    assert "void sng::step_wide_kernel<10, 2, true, false, false>" in overlapping   # the headline's plan
    assert all(k.startswith(OVERLAPPING) for k in overlapping)


@pytest.mark.parametrize("days", DAYS)
def test_slot_rotation_and_counter_amounts(listing, days):
    _, shapes = listing
    serial = [shapes[(0, days, d)] for d in range(days)]
    assert serial == [(0, 0, 1, 0)] * days   # slot, day_delta, bump_day, bump_node
    over = [shapes[(1, days, d)] for d in range(days)]
    slots = [s[0] for s in over]
    assert slots[-1] == 0 and all(a != b for a, b in zip(slots, slots[1:])) and set(slots) <= {0, 1}
    for form in (serial, over):
        assert sum(s[2] + s[3] for s in form) == days
    # the overlapped generators read the counter before anything advances it: day d draws counter + d, the
    # index the serial chain's day d draws after d first steps
    assert [s[1] for s in over] == list(range(days))
    assert [s[2] for s in over] == [0] * (days - 1) + [1]
    assert [s[3] for s in over] == [0] * (days - 1) + [days - 1]
