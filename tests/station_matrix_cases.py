"""The station matrix shared by its CPU check (test_station_matrix_cpu.py) and its GPU test
(test_gpu_station_matrix.py): the configuration surface the lean, wide and day kernels step for every caller without
diagnostics, one row per station, each pinned to the CPU oracle bit for bit.

A row is a station's env kwargs, its RNG mode, the step kernel it exists for (by the name step_plan() gives it:
csrc/sng_step_plan.h), whether that station has a day kernel, and the coverage conditions its days and actions must
meet (Coverage below) -- asserted on the CPU from the oracle's model of the device days, so a row is known to be
meaningful before it reaches a GPU, and again on the GPU from the days actually stepped.

E = 70 envs (ragged at 64 and at 32 envs per wavefront), two consecutive days, one handle seed.  The actions are one
[T, E, A] array for both days (a captured graph reuses its actions every day), drawn inside the station's Box: a
fifth exact zeros, a twentieth exactly the upper bound, one env in eight with every charger idle at half of its steps
(the sell branch of a station without BESS), and with a BESS a quarter of the envs at -1 on the BESS most steps (the
over-discharge clamp and the depth-of-discharge penalty).  No NaN, nothing outside the Box.
"""
import collections

import numpy as np

import oracle as O
from smart_nanogrid_gym.settings import EnvSettings
from smart_nanogrid_gym.spaces import make_spaces

E, DAYS, SEED = 70, 2, 4242
MIN_COUNT = 10   # of every condition: the GPU's day may differ from the model's at an ambiguous wait, and no
#                  condition may hang on one vehicle

BASE = dict(charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
            battery_system_available_in_model=True)
NO_PV = dict(pv_system_available_in_model=False)
NO_BESS = dict(battery_system_available_in_model=False)

Row = collections.namedtuple("Row", "name kw rng kernel day_kernel graph_step_nodes conditions")


def _conditions(kw):
    """The coverage conditions a station can produce (Coverage.counts' keys)."""
    c = {"empty", "arrival", "departure", "present_last"}
    bounded = kw["charging_mode"] == "bounded"
    pv, bess = kw["pv_system_available_in_model"], kw["battery_system_available_in_model"]
    v2x = kw.get("vehicle_to_everything", False)
    if kw["vehicle_uncharged_penalty_mode"] != "no_penalty":
        c.add("pen_vehicle")
    if bess and bounded:   # an unbounded station's BESS never moves: every BESS action raises the flag instead
        c |= {"pen_battery", "bess_clamp"}
    if pv:
        c.add("solar")
    if pv or v2x:
        c.add("sell")
    if v2x:
        c.add("discharge")
    return frozenset(c)


def _row(name, N, interval, kernel, rng="device", day_kernel=False, graph_step_nodes=False, **station):
    kw = dict(BASE, number_of_chargers=N, time_interval=interval, **station)
    if "min" in interval:
        kw["extended_day"] = True
    return Row(name, kw, rng, "void sng::" + kernel, day_kernel, graph_step_nodes, _conditions(kw))


WIDE10 = "step_wide_kernel<10, 2, true, false, false>"
ROWS = [
    # device-RNG days (packed records): the N = 10 wide kernel and its day kernel
    _row("day10_2h", 10, "2h", WIDE10, day_kernel=True),
    _row("day10_30min_req_dense", 10, "30min", "step_wide_kernel<10, 2, true, true, false>", day_kernel=True,
         enable_requested_state_of_charge=True, vehicle_uncharged_penalty_mode="dense"),
    _row("day10_15min", 10, "15min", WIDE10, day_kernel=True),
    _row("day10_nopv_nobess", 10, "1h", WIDE10, day_kernel=True, **NO_PV, **NO_BESS),
    _row("day10_nobess_ondep", 10, "1h", WIDE10, day_kernel=True, **NO_BESS,
         vehicle_uncharged_penalty_mode="on_departure"),
    _row("day10_nopv_price2_samecap", 10, "1h", WIDE10, day_kernel=True, **NO_PV, price_model=2,
         enable_different_vehicle_battery_capacities=False),
    _row("day10_nopen_gridw", 10, "1h", WIDE10, day_kernel=True, vehicle_uncharged_penalty_mode="no_penalty",
         grid_cost_weight=0.8),
    # the lean kernels
    _row("lean4_2h_nopv", 4, "2h", "step_lean_kernel<4, true, false>", **NO_PV),
    _row("lean16_30min_nobess_dense", 16, "30min", "step_lean_kernel<16, true, false>", **NO_BESS,
         vehicle_uncharged_penalty_mode="dense"),
    _row("lean10_v2x_15min", 10, "15min", "step_lean_kernel<10, true, false>", vehicle_to_everything=True),
    _row("lean1_bare_nopen", 1, "1h", "step_lean_kernel<1, true, false>", **NO_PV, **NO_BESS,
         vehicle_uncharged_penalty_mode="no_penalty"),
    # the N = 50 wide kernel (no day kernel: its graph keeps T step nodes)
    _row("wide50_2h_nopv_req", 50, "2h", "step_wide_kernel<50, 2, true, true, false>", graph_step_nodes=True,
         **NO_PV, enable_requested_state_of_charge=True),
    # the general kernel without diagnostics and FAST = false: a dt that is no power of two, legacy promotion;
    # V2X, so the inverted-flag discharge divides by dt on the charger side too
    _row("general10_20min_v2x", 10, "20min", "step_kernel<10, 1, false, false, true>", vehicle_to_everything=True),
    _row("general8_legacy_v2x", 8, "1h", "step_kernel<8, 1, false, false, true>", vehicle_to_everything=True,
         numpy_legacy_promotion=True),
    # reference-RNG days (unpacked records), the oracle's envs seeded seed + i
    _row("ref_wide10_2h_nobess", 10, "2h", "step_wide_kernel<10, 2, false, false, false>", rng="reference",
         **NO_BESS),
    _row("ref_lean8_4h", 8, "4h", "step_lean_kernel<8, false, false>", rng="reference"),
    _row("ref_lean16_30min_req", 16, "30min", "step_lean_kernel<16, false, true>", rng="reference",
         enable_requested_state_of_charge=True),
    _row("ref_wide50_2h_nopv", 50, "2h", "step_wide_kernel<50, 2, false, false, false>", rng="reference", **NO_PV),
]
IDS = [r.name for r in ROWS]

# Not a row of the matrix: `charging_mode != "bounded"` (N = 10, 1 h).  The reference raises at the first moved
# charger (charger.py:88) and defines no state after that; the kernels raise a sticky flag, bill no power and hold
# the SoC, whereas the oracle leaves the step's SoC slot as the day's arrays had it.  The oracle lacks the
# behaviour, so the station is not compared with it under moving actions: test_gpu_station_matrix.py compares it
# with the diagnostics kernel and the day kernel, and pins the held SoC to the oracle through a handle that idles.
UNBOUNDED = _row("day10_unbounded", 10, "1h", WIDE10, day_kernel=True, charging_mode="")


def action_space(row):
    return make_spaces(EnvSettings(**row.kw))[1]


def row_actions(row, space, T):
    """[T, E, A] float32 inside the Box `space` (the handle's action_space, or action_space(row) on the CPU)."""
    lo, hi = np.asarray(space.low, np.float32), np.asarray(space.high, np.float32)
    A = lo.shape[0]
    assert A == row.kw["number_of_chargers"] + int(row.kw["battery_system_available_in_model"])
    rng = np.random.default_rng(1000 * A + T)
    a = (lo + (hi - lo) * rng.random((T, E, A))).astype(np.float32)
    r = rng.random(a.shape)
    a[r < 0.2] = 0.0
    top = (r >= 0.2) & (r < 0.25)
    a[top] = hi[np.nonzero(top)[2]]
    # one env in eight leaves every charger idle at half of its steps: without a BESS and without V2X the station
    # sells only when the PV output exceeds the whole station's charging demand, which Box-uniform actions on 10
    # or more chargers reach at a handful of env-steps only (1 and 7 in two of the rows below without this)
    idle = ((np.arange(E) % 8) == 5)[None, :] & (rng.random((T, E)) < 0.5)
    a[..., :row.kw["number_of_chargers"]][idle] = 0.0
    if row.kw["battery_system_available_in_model"]:
        heavy = ((np.arange(E) % 4) == 0)[None, :] & (rng.random((T, E)) < 0.7)
        a[..., -1][heavy] = -1.0
    assert not np.isnan(a).any() and (a >= lo).all() and (a <= hi).all()
    return a


def load_model_day(env, d):
    """A model day (oracle.device_day) or an exported one in its layout, loaded into an oracle env; returns obs."""
    return env.load(d["soc"], d["occ"], d["cap"], d["req"], d["arrivals"], d["departures"], d["ratio"])


class Coverage:
    """Counts of a row's coverage conditions over the days and steps an oracle env batch went through."""

    def __init__(self, row, T):
        self.row, self.T = row, T
        self.counts = collections.Counter()

    def add_day(self, occ, arrivals, departures):
        """occ [E][N][slots], arrivals / departures [E][N][V] padded with -1: one day of every env."""
        occ = np.asarray(occ)[:, :, :self.T]
        arrivals, departures = np.asarray(arrivals), np.asarray(departures)
        self.counts["empty"] += int((occ == 0).sum())
        self.counts["arrival"] += int((arrivals > 0).sum())
        self.counts["departure"] += int(((departures >= 0) & (departures < self.T)).sum())
        self.counts["present_last"] += int((occ[:, :, self.T - 1] == 1).sum())

    def add_step(self, infos):
        """The oracle's info of every env at one step."""
        c = self.counts
        for inf in infos:
            c["pen_vehicle"] += inf["pen_vehicle"] > 0
            c["pen_battery"] += inf["pen_battery"] > 0
            c["bess_clamp"] += inf["bess_power"] < 0 and inf["bess_soc"] == 0.0
            c["solar"] += inf["solar_power"] > 0
            c["sell"] += inf["grid_power"] < 0
            c["discharge"] += inf["p_discharge"] < 0
            c["error"] += inf["error"] != 0

    def check(self):
        name = self.row.name
        for k in sorted(self.row.conditions):
            assert self.counts[k] >= MIN_COUNT, (name, k, dict(self.counts))
        if "pen_vehicle" not in self.row.conditions:
            assert self.counts["pen_vehicle"] == 0, (name, dict(self.counts))
        assert self.counts["error"] == 0, (name, dict(self.counts))   # nothing here is about illegal input


def padded(lists, V=8):
    """Ragged per-charger lists as an [N][V] int32 array padded with -1."""
    out = np.full((len(lists), V), -1, np.int32)
    for c, row in enumerate(lists):
        out[c, :len(row)] = row
    return out


def square_mode(on):
    import ctypes
    O.lib().orc_set_square_mode.argtypes = [ctypes.c_int]
    O.lib().orc_set_square_mode(1 if on else 0)
