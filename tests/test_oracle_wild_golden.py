"""The CPU oracle against the reference under actions outside the Box and non-finite actions
(tests/golden/wild_*.npz, made by `make_golden.py wild`; the classes are wild_action_cases.CLASSES).

The reference never clips: above the Box, 1e30, 1e37, the values whose float32 charging product overflows, +-inf,
NaN (a quiet one, and one with a sign and a payload), -0.0, subnormals and values below -1 go straight into
charger.py and battery_energy_storage_system.py.  At every recorded step the oracle's observation, reward and
scalars equal the reference's; NaN counts as equal to NaN (assert_array_equal), and a NaN's sign and payload are
not part of the contract (x86 and the GPU produce different default NaNs).  Where the reference raises, the
oracle reports the error code of that exception at that step; where it stops in breakpoint(), the oracle's
`breakpoint`.
"""
import json
import os

import numpy as np
import pytest

import oracle as O
import wild_action_cases as W
from golden_util import GOLDEN

SCALARS = ["grid_power", "p_charge", "p_discharge", "bess_soc", "pen_vehicle", "pen_battery", "grid_cost",
           "total_cost", "solar_power", "bess_power", "bess_calc_power", "nonexistent", "bess_initial_soc"]
NEGATIVE_DEMAND = "Error: If V2X mode is not enabled, then power_demand cannot be less than 0!"


def wild_cases():
    with open(os.path.join(GOLDEN, "wild_cases.json")) as fp:
        return json.load(fp)


CASES = {m["name"]: m for m in wild_cases()}
RUN = [n for n, m in CASES.items() if m["setup_error"] is None]


def same(a, b):
    """Equal, NaN equal to NaN."""
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    return True


@pytest.mark.parametrize("name", RUN)
def test_oracle_matches_reference_under_wild_actions(name):
    meta = CASES[name]
    d = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    cfg = O.OracleConfig(**meta["kwargs"])
    raises = {r["day"]: r for r in meta["raises"]}
    env = None
    for day in range(meta["n_days"]):
        if env is None or meta["fresh_env_per_day"]:
            env = O.OracleEnv(cfg, meta["seed"] + (day if meta["fresh_env_per_day"] else 0))
        assert env.bess_soc == d["bess_soc_reset"][day]
        obs = env.reset()
        np.testing.assert_array_equal(obs, d["obs_reset"][day])
        assert env.ratio == d["ratio"][day]
        sc = env.scenario()
        for k, key in (("soc", "soc0"), ("occ", "occ"), ("cap", "cap"), ("req", "req"), ("arrivals", "arrivals"),
                       ("departures", "departures")):
            np.testing.assert_array_equal(sc[k], d[key][day])
        n = int(d["n_steps"][day])
        assert (n < meta["T"]) == (day in raises)
        for t in range(n):
            obs, r, done, info = env.step(d["actions"][day][t])
            what = (name, day, t, d["actions"][day][t])
            np.testing.assert_array_equal(obs, d["obs"][day][t], err_msg=str(what))
            assert same(r, d["reward"][day][t]), what
            assert done == bool(d["done"][day][t])
            assert info["breakpoint"] == int(d["breakpoint"][day][t] > 0), what
            assert info["error"] == 0, what
            for k in SCALARS:
                np.testing.assert_array_equal(info[k], d[k][day][t], err_msg=str((k,) + what))
        if day in raises:   # the step the reference left by an exception: the oracle's error code for it
            assert raises[day]["step"] == n
            assert (raises[day]["type"], raises[day]["message"]) == ("ValueError", NEGATIVE_DEMAND)
            _, _, _, info = env.step(d["actions"][day][n])
            assert info["error"] == 1, (name, day, n)


def test_fixtures_hold_every_class():
    """Every class met an occupied charger, an empty one ("nonexistent vehicle", a != 0: true for NaN) and the BESS
    in the V2X cases; without V2X the chargers got the non-negative classes and NaN, the BESS every class; the
    negative-action case raised on every day."""
    hits = {n: CASES[n]["class_hits_occupied_empty_bess"] for n in RUN}
    for name in ("wild_v2x_bpv_n10", "wild_v2x_bess_2h_n10"):
        assert not CASES[name]["raises"]
        for k in W.NAMES:
            occupied, empty, bess = hits[name][k]
            assert occupied >= 1 and bess >= 1, (name, k, hits[name][k])
            assert empty >= 1 or name != "wild_v2x_bpv_n10", (name, k)
    h = hits["wild_bpv_n10"]
    for k in W.NAMES:
        assert h[k][2] >= 1, k
        assert (h[k][0] >= 1) == (k in W.NONNEG + W.NANS), (k, h[k])
    neg = CASES["wild_neg_n4"]
    assert neg["fresh_env_per_day"] and sorted(r["day"] for r in neg["raises"]) == list(range(neg["n_days"]))
    # a NaN charger action and a NaN BESS action were recorded with a finite grid power: the reference's flags are
    # NaN there and true (charger.py:122-132, battery_energy_storage_system.py:82-94)
    d = np.load(os.path.join(GOLDEN, "wild_v2x_bpv_n10.npz"))
    N = CASES["wild_v2x_bpv_n10"]["N"]
    nan_c = np.isnan(d["actions"][:, :, :N]) & (d["occ"][:, :, :24].transpose(0, 2, 1) == 1)
    assert nan_c.sum() >= 10 and np.isfinite(d["charger_power"][nan_c]).all()
    nan_b = np.isnan(d["actions"][:, :, N])
    assert nan_b.sum() >= 1 and np.isfinite(d["bess_power"][nan_b]).all() and np.isnan(d["bess_calc_power"][nan_b]).all()


def test_a_quarter_hour_day_is_beyond_the_reference():
    """V2X + BESS at 15 min, N = 4: the reference's 25-slot arrays (charger.py:16-19) do not hold a 96-step day,
    and the fixture records what it does instead of a trajectory.  The oracle refuses the same station unless
    extended_day (this build's longer arrays) is asked for; the 2 h case stands in for a dt other than 1 h."""
    meta = CASES["wild_v2x_bess_15min_n4"]
    assert meta["setup_error"]["type"] == "IndexError" and not os.path.exists(
        os.path.join(GOLDEN, "wild_v2x_bess_15min_n4.npz"))
    with pytest.raises(IndexError):
        O.OracleEnv(O.OracleConfig(**meta["kwargs"]), meta["seed"])
