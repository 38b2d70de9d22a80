"""GPU: the station matrix (station_matrix_cases.py) -- the lean, the wide and the day kernel, and the general kernel
without diagnostics, at the day lengths, station shapes, charging and penalty modes they step for every caller
without diagnostics but were never compared with the oracle at: T = 6, 12, 48, 72 and 96, stations without PV or
without BESS, no_penalty and on_departure, fixed capacities, another price model, a grid cost weight, legacy
promotion and a dt that is no power of two.  An unbounded charging mode has a test of its own, below.

One test per row.  A handle without diagnostics (`fast`: the row asserts the step kernel it exists for by name) and
a twin with info=True (the general kernel with DIAG) start from the same seed and step two consecutive days with
one [T, E, A] action array.  At every step the observations and rewards of all 70 envs are equal bit for bit to
the twin's and to the CPU oracle's (device-RNG days are exported with get_scenarios and loaded into oracle envs;
reference-RNG days are the oracle's own, seeded seed + i); after each day so are the BESS SoC, the vehicles' SoC,
the sticky flags and the day return.  The row's coverage conditions are counted again on the days actually stepped.

Rows whose station has a day kernel capture both days in one EpisodeGraph on a third handle of the same seed: one
step node per day, and after one launch the handle equals `fast` after its two eager days in everything
test_gpu_day_kernel.assert_same compares; day_returns' rows equal the oracle's day returns.
"""
import numpy as np
import pytest

import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smart_nanogrid_gym import SmartNanogridVecEnv, _native  # noqa: E402
from smart_nanogrid_gym.vec_env import EpisodeGraph  # noqa: E402
from station_matrix_cases import (DAYS, E, IDS, ROWS, SEED, UNBOUNDED, Coverage, padded, row_actions,  # noqa: E402
                                  square_mode)
from test_gpu_day_kernel import assert_same, flags_of  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    square_mode(True)   # x*x squares, as on the GPU
    yield
    square_mode(False)


def load_exported_day(env, iv, ratio):
    V = max(1, max(len(x) for x in iv["Arrivals"]))
    return env.load(iv["SOC"], iv["Charger_occupancy"], iv["Vehicle_capacities"], iv["Requested_SOC"],
                    padded(iv["Arrivals"], V), padded(iv["Departures"], V), ratio)


@pytest.mark.parametrize("name", IDS)
def test_station_row_vs_general_kernel_and_oracle(name):
    row = ROWS[IDS.index(name)]
    kw, device = row.kw, row.rng == "device"
    bess = kw["battery_system_available_in_model"]
    fast = SmartNanogridVecEnv(E, seed=SEED, rng=row.rng, **kw)
    diag = SmartNanogridVecEnv(E, seed=SEED, rng=row.rng, info=True, **kw)
    cfg = O.OracleConfig(**kw)
    T = fast.timesteps
    assert T == cfg.T and fast.obs_dim == cfg.obs_dim and fast.act_dim == cfg.act_dim
    acts = row_actions(row, fast.action_space, T)
    acts_d = torch.from_numpy(acts).to(fast.device)
    envs = [O.OracleEnv(cfg, 0 if device else SEED + e) for e in range(E)]
    cov = Coverage(row, T)
    day_returns = []
    for day in range(DAYS):
        obs = fast.reset_tensors().cpu().numpy()
        np.testing.assert_array_equal(obs, diag.reset_tensors().cpu().numpy(), err_msg=f"{name} day {day}: reset")
        assert fast.step_kernel_name() == row.kernel, (name, fast.step_kernel_name())
        parts = diag.step_kernel_name().rstrip(">").split("<")
        assert parts[0] == "void sng::step_kernel" and parts[1].split(", ")[2] == "true", diag.step_kernel_name()
        if device:   # the day, independently of any step kernel: into the oracle
            ivs, ratios = fast.get_scenarios(0, E)
            ref0 = np.stack([load_exported_day(e, iv, r) for e, iv, r in zip(envs, ivs, ratios)])
            cov.add_day(np.array([iv["Charger_occupancy"] for iv in ivs]),
                        np.stack([padded(iv["Arrivals"], 32) for iv in ivs]),
                        np.stack([padded(iv["Departures"], 32) for iv in ivs]))
        else:
            ref0 = np.stack([e.reset() for e in envs])
            days = [e.scenario(vmax=32) for e in envs]
            cov.add_day(*(np.stack([d[k] for d in days]) for k in ("occ", "arrivals", "departures")))
        np.testing.assert_array_equal(obs, ref0, err_msg=f"{name} day {day}: reset vs oracle")
        ret = np.zeros(E)
        for t in range(T):
            what = f"{name} day {day} t {t}"
            o, r, d = fast.step_tensors(acts_d[t])
            ot, rt, dt = diag.step_tensors(acts_d[t])
            o, r, d = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()
            np.testing.assert_array_equal(o, ot.cpu().numpy(), err_msg=what + ": obs vs general kernel")
            np.testing.assert_array_equal(r, rt.cpu().numpy(), err_msg=what + ": reward vs general kernel")
            outs = [e.step(acts[t, i]) for i, e in enumerate(envs)]
            np.testing.assert_array_equal(o, np.stack([x[0] for x in outs]), err_msg=what + ": obs vs oracle")
            np.testing.assert_array_equal(r, np.array([x[1] for x in outs]), err_msg=what + ": reward vs oracle")
            assert bool(d.all()) == bool(d.any()) == (t == T - 1), what
            np.testing.assert_array_equal(d, dt.cpu().numpy(), err_msg=what)
            ret = ret + r
            cov.add_step([x[3] for x in outs])
        what = f"{name} after day {day}"
        if bess:
            b = fast.battery_state_of_charge()
            np.testing.assert_array_equal(b, diag.battery_state_of_charge(), err_msg=what)
            np.testing.assert_array_equal(b, np.array([e.bess_soc for e in envs]), err_msg=what)
        np.testing.assert_array_equal(fast.vehicle_state_of_charge(), diag.vehicle_state_of_charge(), err_msg=what)
        np.testing.assert_array_equal(flags_of(fast), flags_of(diag), err_msg=what)
        np.testing.assert_array_equal(fast.return_d.cpu().numpy(), ret, err_msg=what + ": day return vs oracle")
        day_returns.append(ret)
    cov.check()
    if row.day_kernel or row.graph_step_nodes:
        captured_days_vs_eager(row, acts_d, fast, day_returns)
    fast.close()
    diag.close()


def captured_days_vs_eager(row, acts_d, fast, day_returns):
    """Both days as one EpisodeGraph launch on a fresh handle of the same seed, against `fast` after its eager days
    and the day returns found there."""
    h = SmartNanogridVecEnv(E, seed=SEED, rng="device", **row.kw)
    rets = torch.zeros((DAYS, E), dtype=torch.float64, device=h.device)
    g = EpisodeGraph(h, acts_d, days=DAYS, day_returns=rets)
    assert g.step_nodes_per_day == (1 if row.day_kernel else h.timesteps), (row.name, g.step_nodes_per_day)
    g.launch()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rets.cpu().numpy(), np.stack(day_returns), err_msg=f"{row.name}: day_returns")
    # the graph's returns went into day_returns' rows, not into return_d: the last day's row is what the eager
    # handle's return_d holds (and what its checkpoint saves)
    h.return_d.copy_(rets[DAYS - 1])
    assert_same(h, fast, f"{row.name}: {DAYS} captured days vs eager days")
    g.close()
    h.close()


def test_unbounded_station_holds_soc_and_raises_the_flag():
    """charging_mode != "bounded" on the wide N = 10 kernel and its day kernel (station_matrix_cases.UNBOUNDED says
    why this is no row of the matrix): every moved charger and every BESS action raises the sticky flag, no power
    is billed and nothing moves -- in the day kernel the SoC that stays put lives in registers all day.  Against
    the diagnostics twin at every step; the observations equal those of a third handle that idles (zero actions,
    which the reference defines: SoC carried over), and that handle equals the oracle bit for bit."""
    row = UNBOUNDED
    kw = row.kw
    fast = SmartNanogridVecEnv(E, seed=SEED, rng="device", **kw)
    diag = SmartNanogridVecEnv(E, seed=SEED, rng="device", info=True, **kw)
    idle = SmartNanogridVecEnv(E, seed=SEED, rng="device", **kw)
    cfg = O.OracleConfig(**kw)
    T = fast.timesteps
    acts = row_actions(row, fast.action_space, T)
    acts_d = torch.from_numpy(acts).to(fast.device)
    zeros = np.zeros(fast.act_dim, np.float32)
    zeros_d = torch.zeros((E, fast.act_dim), device=fast.device)
    envs = [O.OracleEnv(cfg, 0) for _ in range(E)]
    moved = np.zeros(E, bool)
    day_returns = []
    for day in range(DAYS):
        obs = fast.reset_tensors().cpu().numpy()
        np.testing.assert_array_equal(obs, diag.reset_tensors().cpu().numpy())
        np.testing.assert_array_equal(obs, idle.reset_tensors().cpu().numpy())
        assert fast.step_kernel_name() == idle.step_kernel_name() == row.kernel, fast.step_kernel_name()
        ivs, ratios = fast.get_scenarios(0, E)
        ref0 = np.stack([load_exported_day(e, iv, r) for e, iv, r in zip(envs, ivs, ratios)])
        np.testing.assert_array_equal(obs, ref0, err_msg=f"day {day}: reset vs oracle")
        occ = np.array([iv["Charger_occupancy"] for iv in ivs])
        ret = np.zeros(E)
        for t in range(T):
            what = f"unbounded day {day} t {t}"
            o, r, d = fast.step_tensors(acts_d[t])
            ot, rt, _ = diag.step_tensors(acts_d[t])
            oi, ri, _ = idle.step_tensors(zeros_d)
            o, r, oi = o.cpu().numpy(), r.cpu().numpy(), oi.cpu().numpy()
            np.testing.assert_array_equal(o, ot.cpu().numpy(), err_msg=what + ": obs vs general kernel")
            np.testing.assert_array_equal(r, rt.cpu().numpy(), err_msg=what + ": reward vs general kernel")
            outs = [e.step(zeros) for e in envs]
            np.testing.assert_array_equal(oi, np.stack([x[0] for x in outs]), err_msg=what + ": idle vs oracle")
            np.testing.assert_array_equal(ri.cpu().numpy(), np.array([x[1] for x in outs]), err_msg=what)
            np.testing.assert_array_equal(o, oi, err_msg=what + ": nothing moved")
            assert bool(d.cpu().numpy().all()) == (t == T - 1), what
            ret = ret + r
            moved |= ((occ[:, :, t] == 1) & (acts[t, :, :10] != 0)).any(axis=1) | (acts[t, :, 10] != 0)
        for other in (diag, idle):
            np.testing.assert_array_equal(fast.battery_state_of_charge(), other.battery_state_of_charge())
            np.testing.assert_array_equal(fast.vehicle_state_of_charge(), other.vehicle_state_of_charge())
        np.testing.assert_array_equal(fast.return_d.cpu().numpy(), ret)
        day_returns.append(ret)
    flags = flags_of(fast)
    np.testing.assert_array_equal(flags, flags_of(diag))
    assert moved.all() and (flags == _native.FLAG_CHARGING_MODE).all(), flags
    assert not flags_of(idle).any()
    captured_days_vs_eager(row, acts_d, fast, day_returns)
    for v in (fast, diag, idle):
        v.close()
