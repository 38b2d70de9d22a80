"""GPU: device-RNG days (generate_kernel, its fused t = 0 blocks observe_day0, the unfused observe0_kernel) pinned
exactly to the oracle's CPU model of their streams (oracle.device_day), at every shape of
the generator's grid and every instantiation of the kernel (the case table, device_day_cases.py).

Per row, over three consecutive days (the day number read from day_counter() before each reset):
  - the export of all E envs (get_scenarios: SOC, occupancy, capacity, requested SoC, arrivals, departures) and
    pv_ratio() equal the model's day bit for bit.  The geometric wait is the one value the GPU takes from a
    hardware approximation (__log2f): where the float64 wait has an integer within the model's margin (1e-5,
    sng_oracle.c) the model takes the GPU's arrival if it is one of the two candidate waits.  Such vehicles are
    the only ones excused, their count is printed, and their share stays at or below 1e-3 (the share the model
    alone meets is held to the same bound on the CPU, test_device_day_model_cpu.py);
  - the reset's observation equals OracleEnv.load(<the model's arrays>, <the model's ratio>): the fused t = 0
    blocks draw from the streams on their own;
  - oracle envs loaded from the MODEL's arrays -- not from the export, as test_gpu_bench_kernel.py and
    test_gpu_wide_kernel.py load them -- step the day with that file's action recipe: observations and rewards
    bit-exact (x*x squares), the BESS SoC at each day end.  This carries what the export does not hold: the
    records' PEN and STATIC bits, the carried arrival SoC and the requested-SoC plane.
One row also replays its last day and compares the replay stream's PV ratios.
"""
import ctypes

import numpy as np
import pytest

import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smart_nanogrid_gym import SmartNanogridVecEnv  # noqa: E402
from device_day_cases import AMBIGUOUS_SHARE_MAX, CASES, DAYS, IDS, env_kwargs, model_days, padded  # noqa: E402
from test_gpu_bench_kernel import actions  # noqa: E402

EXPORT = (("soc", "SOC"), ("occ", "Charger_occupancy"), ("cap", "Vehicle_capacities"), ("req", "Requested_SOC"))


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    O.lib().orc_set_square_mode.argtypes = [ctypes.c_int]
    O.lib().orc_set_square_mode(1)
    yield
    O.lib().orc_set_square_mode(0)


def _exact_day(case, cfg, venv, day):
    """The export of every env against the model's day; returns (model days, vehicles, excused, off the floor)."""
    ivs, ratios = venv.get_scenarios()
    model = model_days(case, day, [padded(iv["Arrivals"]) for iv in ivs], cfg)
    excused = off_floor = 0
    for e, (iv, m) in enumerate(zip(ivs, model)):
        where = f"{case.name} day {day} env {e}"
        np.testing.assert_array_equal(padded(iv["Arrivals"]), m["arrivals"], err_msg=f"{where} arrivals")
        np.testing.assert_array_equal(padded(iv["Departures"]), m["departures"], err_msg=f"{where} departures")
        for ours, theirs in EXPORT:
            np.testing.assert_array_equal(np.asarray(iv[theirs]), m[ours], err_msg=f"{where} {theirs}")
        if m["followed"]:
            excused += m["followed"]
            floor = O.device_day(cfg, case.seed, case.env_offset + e, day)
            off_floor += int(not np.array_equal(floor["arrivals"], m["arrivals"]))
    want = np.array([m["ratio"] for m in model])
    np.testing.assert_array_equal(ratios, want, err_msg=f"{case.name} day {day} exported ratio")
    np.testing.assert_array_equal(venv.pv_ratio(), want, err_msg=f"{case.name} day {day} pv_ratio()")
    return model, sum(m["vehicles"] for m in model), excused, off_floor


def _load(env, m, req=None):
    return env.load(m["soc"], m["occ"], m["cap"], m["req"] if req is None else req, m["arrivals"], m["departures"],
                    m["ratio"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_days_equal_the_model(case):
    kw = env_kwargs(case)
    E, A = case.E, case.N + 1
    # (sng_set_env_offset takes any non-negative 64-bit offset, so the row above 2^32 runs like the others)
    venv = SmartNanogridVecEnv(E, seed=case.seed, rng="device", env_offset=case.env_offset, **kw)
    cfg = O.OracleConfig(**kw)
    # oracle env i is seeded like global env i (its profile-noise key); its own generator is never used
    envs = [O.OracleEnv(cfg, case.seed + case.env_offset + e) for e in range(E)]
    rng = np.random.default_rng(case.seed % 2 ** 32)
    heavy = (np.arange(E) % 4) == 0
    vehicles = excused = off_floor = 0
    for _ in range(DAYS):
        day = venv.day_counter()
        obs = venv.reset_tensors().cpu().numpy()
        model, n_veh, n_exc, n_off = _exact_day(case, cfg, venv, day)
        vehicles, excused, off_floor = vehicles + n_veh, excused + n_exc, off_floor + n_off
        ref0 = np.stack([_load(env, m) for env, m in zip(envs, model)])
        np.testing.assert_array_equal(obs, ref0, err_msg=f"{case.name} day {day} reset observation")
        for t in range(venv.timesteps):
            a = actions(rng, E, A, heavy)
            o, r, d = venv.step_tensors(torch.from_numpy(a).to(venv.device))
            outs = [env.step(a[i]) for i, env in enumerate(envs)]
            np.testing.assert_array_equal(o.cpu().numpy(), np.stack([x[0] for x in outs]),
                                          err_msg=f"{case.name} day {day} t {t} observation")
            np.testing.assert_array_equal(r.cpu().numpy(), np.array([x[1] for x in outs]),
                                          err_msg=f"{case.name} day {day} t {t} reward")
            assert bool(d.cpu().numpy().all()) == (t == venv.timesteps - 1)
        np.testing.assert_array_equal(venv.battery_state_of_charge(), np.array([env.bess_soc for env in envs]),
                                      err_msg=f"{case.name} day {day} BESS SoC")
    venv.close()
    print(f"{case.name}: excused {excused} of {vehicles} vehicles ({off_floor} env-days off the float64 floor)")
    assert vehicles > 0 and excused <= AMBIGUOUS_SHARE_MAX * vehicles, (excused, vehicles)


def test_replayed_device_day_ratios():
    """reset(generate_new_initial_values=False) of a device day redraws the PV ratio from the replay stream
    (replay_ratio_draw): replay number k of the handle gives the model's ratio k, and the replayed day's t = 0
    observation is the model's day under that ratio, its requested SoC left at the zeros that
    clear_initialisation_variables wrote (load_initial_values does not restore it, charging_station.py:119-150)."""
    case = next(c for c in CASES if c.name == "quads7")._replace(E=77)
    kw = env_kwargs(case)
    venv = SmartNanogridVecEnv(case.E, seed=case.seed, rng="device", **kw)
    cfg = O.OracleConfig(**kw)
    envs = [O.OracleEnv(cfg, case.seed + e) for e in range(case.E)]
    day = venv.day_counter()
    venv.reset_tensors()
    model = _exact_day(case, cfg, venv, day)[0]
    zeros = torch.zeros((case.E, venv.act_dim), device=venv.device)
    for t in range(venv.timesteps):
        venv.step_tensors(zeros)
    bess = venv.battery_state_of_charge()
    for k in range(3):
        obs = venv.replay_tensors().cpu().numpy()
        want = np.array([O.device_replay_ratio(case.seed, e, k) for e in range(case.E)])
        np.testing.assert_array_equal(venv.pv_ratio(), want, err_msg=f"replay {k}")
        assert want.min() >= 0.0 and want.max() <= 1.8 and np.unique(want).size > 20
        ref0 = []
        for env, m, b, ratio in zip(envs, model, bess, want):
            env.bess_soc = b
            ref0.append(_load(env, dict(m, ratio=ratio), req=np.zeros_like(m["req"])))
        np.testing.assert_array_equal(obs, np.stack(ref0), err_msg=f"replay {k} observation")
    venv.close()
