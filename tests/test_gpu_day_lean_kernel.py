"""GPU: the lean day kernel (day_lean_kernel, csrc/sng_step_day.h) -- a captured day's T steps of a lean-family
station as one graph node, with SoC, BESS SoC and the day return in registers, for packed device-RNG days and for
the word / aux planes of reference-RNG, injected and replayed days.

  1. Twin graphs: the default form (one node per day) against EpisodeGraph(step_nodes=True), three replays, with
     test_gpu_day_kernel's twin_replays / assert_same: outputs, day returns, BESS SoC, day counter, sticky flags and
     the whole checkpoint.
  2. Every step against the CPU oracle, through the trajectory buffers (EpisodeGraph(trajectory=True)), for the
     lean rows of the station matrix: a wrong observation at step 3 of a day shows at step 3.
  3. Replayed days at N = 8 with the requested SoC enabled (the replay clears the requests, so the plan drops REQ).
  4. The recorded N = 4 PPO day, injected and replayed as one launch.
  5. The slow sums (8 or more powers whose running sum is not numpy's) inside the day kernel, on the inputs of
     test_gpu_lean_sums.py, which asserts for exactly these inputs that the branch was needed and changed sums.
"""
import numpy as np
import pytest

import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from golden_util import kat  # noqa: E402
from smart_nanogrid_gym import SmartNanogridVecEnv, _native  # noqa: E402
from smart_nanogrid_gym.vec_env import EpisodeGraph  # noqa: E402
from station_matrix_cases import DAYS, E as ME, ROWS, SEED, row_actions, square_mode  # noqa: E402
from test_gpu_day_kernel import assert_same, flags_of, make_actions, twin_replays  # noqa: E402
from test_gpu_lean_sums import _actions as sums_actions  # noqa: E402
from test_gpu_station_matrix import load_exported_day  # noqa: E402

BASE = dict(charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
            battery_system_available_in_model=True)


def station(N, interval, **kw):
    out = dict(BASE, number_of_chargers=N, time_interval=interval, **kw)
    if "min" in interval:
        out["extended_day"] = True
    return out


STEPS = {"30min": 48, "1h": 24, "2h": 12}


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    square_mode(True)   # x*x squares, as on the GPU
    yield
    square_mode(False)


# ---------------------------------------------------------------------------------------------------- 1. twin graphs
@pytest.mark.parametrize("E", [1, 64, 70])   # one lane, one full wavefront, a full one and a ragged one of 6 lanes
def test_default_station_matches_step_nodes(E):
    twin_replays(E, station(8, "1h"), make_actions(24, E, 9, seed=E))


@pytest.mark.parametrize("N,interval", [(4, "2h"), (1, "30min"), (2, "30min"), (16, "30min")])
def test_station_sizes_and_day_lengths_match_step_nodes(N, interval):
    twin_replays(70, station(N, interval), make_actions(STEPS[interval], 70, N + 1, seed=N))


def test_v2x_station_with_negative_actions_raises_flags():
    fl = twin_replays(70, station(10, "1h", vehicle_to_everything=True), make_actions(24, 70, 11, seed=21, low=-1.0))
    assert fl.any()


def test_requested_soc_stream():
    kw = station(8, "1h", enable_requested_state_of_charge=True)
    v = SmartNanogridVecEnv(1, seed=5, rng="device", **kw)
    v.reset_tensors()
    assert v.step_kernel_name() == "void sng::step_lean_kernel<8, true, true>"
    v.close()
    twin_replays(70, kw, make_actions(24, 70, 9, seed=22))


def test_two_days_with_day_returns():
    twin_replays(70, station(8, "1h"), make_actions(24, 70, 9, seed=23), days=2, with_returns=True)


def test_actions_at_a_4_byte_aligned_address():
    twin_replays(70, station(8, "1h"), make_actions(24, 70, 9, seed=24, offset_floats=1))


# ------------------------------------------------------------------------------ 2. every step against the oracle
LEAN_ROWS = [r for r in ROWS if "step_lean_kernel" in r.kernel]
ND, BP = _native.FLAG_NEGATIVE_DEMAND, _native.FLAG_V2X_BREAKPOINT


def oracle_flags(infos):
    return np.array([(ND if i["error"] == 1 else 0) | (BP if i["breakpoint"] else 0) for i in infos], np.uint32)


def compare_day(name, day, envs, acts, obs_traj, reward_traj, done_traj, flags):
    """One day of the oracle envs (their t = 0 observation taken already) against one day of trajectory buffers
    [T + 1, E, O], [T, E], [T, E]; returns the day's returns, ORs the oracle's flags into `flags`."""
    T = acts.shape[0]
    ret = np.zeros(len(envs))
    for t in range(T):
        what = f"{name} day {day} t {t}"
        outs = [e.step(acts[t, i]) for i, e in enumerate(envs)]
        np.testing.assert_array_equal(obs_traj[t + 1], np.stack([x[0] for x in outs]), err_msg=what + ": obs")
        r = np.array([x[1] for x in outs])
        np.testing.assert_array_equal(reward_traj[t], r, err_msg=what + ": reward")
        np.testing.assert_array_equal(done_traj[t], np.full(len(envs), int(t == T - 1), np.uint8), err_msg=what)
        assert all(x[3]["error"] in (0, 1) for x in outs), what
        flags |= oracle_flags([x[3] for x in outs])
        ret = ret + r
    return ret


def final_vehicle_soc(envs, T):
    """SOC[c, T - 1] of every env's day as the oracle holds it after the last step."""
    return np.stack([e.scenario(vmax=32)["soc"][:, T - 1] for e in envs])


@pytest.mark.parametrize("name", [r.name for r in LEAN_ROWS])
def test_every_step_of_a_captured_day_vs_oracle(name):
    row = next(r for r in LEAN_ROWS if r.name == name)
    kw, device = row.kw, row.rng == "device"
    h = SmartNanogridVecEnv(ME, seed=SEED, rng=row.rng, **kw)
    cfg = O.OracleConfig(**kw)
    T = h.timesteps
    acts = row_actions(row, h.action_space, T)
    acts_d = torch.from_numpy(acts).to(h.device)
    envs = [O.OracleEnv(cfg, 0 if device else SEED + e) for e in range(ME)]
    flags = np.zeros(ME, np.uint32)
    if device:
        # the days the graph's resets will draw, from a handle of the same seed that only resets (a day that was
        # reset but never stepped is counted by the next reset)
        src = SmartNanogridVecEnv(ME, seed=SEED, rng="device", **kw)
        exported = []
        for _ in range(DAYS):
            src.reset_tensors()
            exported.append(src.get_scenarios(0, ME))
        src.close()
        rets = torch.zeros((DAYS, ME), dtype=torch.float64, device=h.device)
        g = EpisodeGraph(h, acts_d, days=DAYS, day_returns=rets, trajectory=True)
        assert g.step_nodes_per_day == 1, (name, g.step_nodes_per_day)
        g.launch()
        torch.cuda.synchronize()
        obs, rew, done = g.obs_traj.cpu().numpy(), g.reward_traj.cpu().numpy(), g.done_traj.cpu().numpy()
        for day, (ivs, ratios) in enumerate(exported):
            ref0 = np.stack([load_exported_day(e, iv, r) for e, iv, r in zip(envs, ivs, ratios)])
            np.testing.assert_array_equal(obs[day, 0], ref0, err_msg=f"{name} day {day}: reset vs oracle")
            ret = compare_day(name, day, envs, acts, obs[day], rew[day], done[day], flags)
            np.testing.assert_array_equal(rets[day].cpu().numpy(), ret, err_msg=f"{name} day {day}: day return")
        g.close()
    else:
        for day in range(DAYS):
            h.reset_tensors()
            assert h.step_kernel_name() == row.kernel, (name, h.step_kernel_name())
            g = EpisodeGraph(h, acts_d, with_reset=False, trajectory=True)
            assert g.step_nodes_per_day == 1, (name, g.step_nodes_per_day)
            g.launch()
            torch.cuda.synchronize()
            obs, rew, done = (x.cpu().numpy()[0] for x in (g.obs_traj, g.reward_traj, g.done_traj))
            np.testing.assert_array_equal(obs[0], np.stack([e.reset() for e in envs]), err_msg=f"{name} day {day}: reset")
            ret = compare_day(name, day, envs, acts, obs, rew, done, flags)
            np.testing.assert_array_equal(h.return_d.cpu().numpy(), ret, err_msg=f"{name} day {day}: day return")
            g.close()
    assert h.step_kernel_name() == row.kernel, (name, h.step_kernel_name())
    if kw["battery_system_available_in_model"]:
        np.testing.assert_array_equal(h.battery_state_of_charge(), np.array([e.bess_soc for e in envs]))
    np.testing.assert_array_equal(flags_of(h), flags)
    # the vehicles' SoC after the last day: the oracle's SOC[:, T - 1] where a vehicle stood at the last step (an
    # empty charger's slot is the kernels' own bookkeeping: the arrival SoC a packed record carries)
    occ = np.stack([e.scenario(vmax=32)["occ"][:, T - 1] for e in envs]) == 1
    assert occ.any()
    np.testing.assert_array_equal(h.vehicle_state_of_charge()[occ], final_vehicle_soc(envs, T)[occ])
    h.close()


# --------------------------------------------------------------------------------------------- 3. replayed days
@pytest.mark.parametrize("rng", ["device", "reference"])
def test_generated_day_then_its_replay_with_a_requested_soc_plane(rng):
    """The generated day runs <8, PK, true>; its replay clears the requests (req_zero) and owns no day-counter
    value, so the plan drops REQ on a day whose req plane exists."""
    E = 70
    kw = station(8, "1h", enable_requested_state_of_charge=True)
    pk = "true" if rng == "device" else "false"
    acts = make_actions(24, E, 9, seed=31)
    v = SmartNanogridVecEnv(E, seed=32, rng=rng, **kw)
    w = SmartNanogridVecEnv(E, seed=32, rng=rng, **kw)
    for new_day, req in ((lambda x: x.reset_tensors(), "true"), (lambda x: x.replay_tensors(), "false")):
        new_day(v)
        new_day(w)
        assert v.step_kernel_name() == w.step_kernel_name() == f"void sng::step_lean_kernel<8, {pk}, {req}>"
        g = EpisodeGraph(v, acts, with_reset=False)
        assert g.step_nodes_per_day == 1
        g.launch()
        for t in range(24):
            w.step_tensors(acts[t])
        assert_same(v, w, f"steps-only graph, {rng} day, REQ = {req}")
        assert bool((v.return_d != 0).any())
        g.close()
    v.close()
    w.close()


# ------------------------------------------------------------------------------------------- 4. the recorded day
def test_recorded_ppo_day_injected_and_replayed_as_one_launch():
    k = kat("single_prediction_files")
    kw = dict(number_of_chargers=k["N"], time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse", grid_cost_weight=0.8)
    acts = torch.from_numpy(k["actions"][:, None, :].copy()).to("cuda:0")   # [24, 1, 5]
    v = SmartNanogridVecEnv(1, **kw)
    w = SmartNanogridVecEnv(1, **kw)
    for x in (v, w):
        x.set_battery_state_of_charge(k["bess_soc0"])
        x.reset_from_initial_values(k["iv"], k["ratio"], restore_requested_soc=True)
        assert x.step_kernel_name().startswith("void sng::step_lean_kernel<4, false, "), x.step_kernel_name()
    obs0 = v.obs_d.clone()
    g = EpisodeGraph(v, acts, with_reset=False, trajectory=True)
    assert g.step_nodes_per_day == 1
    g.launch()
    torch.cuda.synchronize()
    assert torch.equal(g.obs_traj[0, 0], obs0)
    for t in range(24):
        o, r, d = w.step_tensors(acts[t])
        assert torch.equal(g.obs_traj[0, t + 1], o), t
        assert torch.equal(g.reward_traj[0, t], r), t
        assert torch.equal(g.done_traj[0, t], d), t
    assert bool((g.reward_traj != 0).any())
    assert torch.equal(v.return_d, w.return_d)
    np.testing.assert_array_equal(v.vehicle_state_of_charge(), w.vehicle_state_of_charge())
    np.testing.assert_array_equal(v.battery_state_of_charge(), w.battery_state_of_charge())
    g.close()
    v.close()
    w.close()


# ------------------------------------------------------------------------------------------- 5. the slow sums
@pytest.mark.parametrize("N,v2x", [(16, True), (10, True), (16, False)])
def test_slow_sums_inside_the_day_kernel(N, v2x):
    E, seed = 2048, 4242 + N
    kw = dict(BASE, number_of_chargers=N, time_interval="1h", vehicle_to_everything=v2x)
    eager = SmartNanogridVecEnv(E, seed=seed, rng="reference", **kw)
    graphed = SmartNanogridVecEnv(E, seed=seed, rng="reference", **kw)
    for x in (eager, graphed):
        x._info.flags = None   # as test_lean_totals_vs_general_kernel_and_oracle steps its lean handle
    T = eager.timesteps
    rng = np.random.default_rng(N)
    for day in range(2):
        acts = torch.from_numpy(np.stack([sums_actions(rng, E, N, v2x) for _ in range(T)])).to(eager.device)
        assert torch.equal(eager.reset_tensors(), graphed.reset_tensors())
        assert eager.step_kernel_name() == f"void sng::step_lean_kernel<{N}, false, false>"
        g = EpisodeGraph(graphed, acts, with_reset=False, trajectory=True)
        assert g.step_nodes_per_day == 1
        g.launch()
        for t in range(T):
            o, r, _ = eager.step_tensors(acts[t])
            assert torch.equal(g.obs_traj[0, t + 1], o), (day, t)
            # NaN rewards equal NaN rewards: compare the bits
            assert torch.equal(g.reward_traj[0, t].view(torch.int64), r.view(torch.int64)), (day, t)
        torch.cuda.synchronize()
        assert eager.save_state() == graphed.save_state(), day
        g.close()
    eager.close()
    graphed.close()
