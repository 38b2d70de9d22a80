"""GPU: SNG_GRAPH_TRAJECTORY (EpisodeGraph(trajectory=True)) -- a captured day keeps every step's observation,
reward and done instead of the last step's.

The three capture forms write the same trajectory for the same days and actions: the lean day kernel (its per-step
strides are kernel arguments), T step nodes (pointer arithmetic at capture; the only form at N = 50, and what the
wide N = 10 plan falls back to with the flag, because day_wide_kernel takes no stride), and each equals the eager
steps of a twin handle.  Block [d][0] of the observations is day d's t = 0 observation, written by the graph's reset
or copied from venv.obs_d by a steps-only graph's launch.  Without the flag venv.obs_d / reward_d / done_d are written
as before; with it a launch leaves them alone.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smart_nanogrid_gym import SmartNanogridVecEnv  # noqa: E402
from smart_nanogrid_gym.vec_env import EpisodeGraph  # noqa: E402
from test_gpu_day_kernel import make_actions  # noqa: E402

E, SEED, DAYS = 70, 77, 2
BASE = dict(charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
            battery_system_available_in_model=True)
KW8 = dict(BASE, number_of_chargers=8, time_interval="1h")
KW10 = dict(BASE, number_of_chargers=10, time_interval="1h")
KW50 = dict(BASE, number_of_chargers=50, time_interval="2h")
KW4 = dict(BASE, number_of_chargers=4, time_interval="1h")


def eager_days(kw, acts, days=DAYS, e=E):
    """[days, T + 1, E, O], [days, T, E], [days, T, E] of device-RNG days stepped one by one."""
    v = SmartNanogridVecEnv(e, seed=SEED, rng="device", **kw)
    T = v.timesteps
    obs = torch.zeros((days, T + 1, e, v.obs_dim), device=v.device)
    rew = torch.zeros((days, T, e), dtype=torch.float64, device=v.device)
    done = torch.zeros((days, T, e), dtype=torch.uint8, device=v.device)
    for d in range(days):
        obs[d, 0] = v.reset_tensors()
        for t in range(T):
            o, r, dn = v.step_tensors(acts[t])
            obs[d, t + 1], rew[d, t], done[d, t] = o, r, dn
    torch.cuda.synchronize()
    state = v.save_state()
    v.close()
    return obs, rew, done, state


def captured_days(kw, acts, nodes, days=DAYS, e=E, **graph_kw):
    """The same days in one graph with reset; `nodes`: the step nodes per day the form must report."""
    v = SmartNanogridVecEnv(e, seed=SEED, rng="device", **kw)
    before = (v.obs_d.clone(), v.reward_d.clone(), v.done_d.clone())
    g = EpisodeGraph(v, acts, days=days, trajectory=True, **graph_kw)
    assert g.step_nodes_per_day == (1 if nodes == 1 else v.timesteps), g.step_nodes_per_day
    assert tuple(g.obs_traj.shape) == (days, v.timesteps + 1, e, v.obs_dim) and g.obs_traj.dtype == torch.float32
    assert tuple(g.reward_traj.shape) == (days, v.timesteps, e) and g.reward_traj.dtype == torch.float64
    assert tuple(g.done_traj.shape) == (days, v.timesteps, e) and g.done_traj.dtype == torch.uint8
    g.launch()
    torch.cuda.synchronize()
    # the handle's own output tensors are not the graph's
    for a, b in zip(before, (v.obs_d, v.reward_d, v.done_d)):
        assert torch.equal(a, b)
    out = g.obs_traj.clone(), g.reward_traj.clone(), g.done_traj.clone(), v.save_state()
    g.close()
    v.close()
    return out


def assert_trajectories_equal(a, b, what):
    for x, y, name in zip(a[:3], b[:3], ("obs", "reward", "done")):
        assert torch.equal(x, y), f"{what}: {name}"
    assert a[3] == b[3], f"{what}: checkpoint"


@pytest.fixture(scope="module")
def lean8():
    acts = make_actions(24, E, 9, seed=1)
    return acts, eager_days(KW8, acts)


def test_lean_day_kernel_trajectory_equals_eager_days(lean8):
    acts, want = lean8
    assert_trajectories_equal(captured_days(KW8, acts, nodes=1), want, "day_lean_kernel")
    assert bool((want[1] != 0).any()) and bool(want[2][:, -1].all()) and not bool(want[2][:, :-1].any())


def test_step_nodes_trajectory_equals_eager_days(lean8):
    acts, want = lean8
    assert_trajectories_equal(captured_days(KW8, acts, nodes=24, step_nodes=True), want, "step nodes")


def test_config5_station_keeps_step_nodes():
    acts = make_actions(12, E, 51, seed=2)
    assert_trajectories_equal(captured_days(KW50, acts, nodes=12), eager_days(KW50, acts), "N = 50")


def test_wide_plan_falls_back_to_step_nodes_with_the_flag():
    acts = make_actions(24, E, 11, seed=3)
    assert_trajectories_equal(captured_days(KW10, acts, nodes=24), eager_days(KW10, acts), "wide N = 10")
    v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **KW10)
    g = EpisodeGraph(v, acts)   # without the flag: the day kernel, as before
    assert g.step_nodes_per_day == 1
    g.close()
    v.close()


def test_block_alignment_when_an_observation_block_is_8_mod_16():
    """N = 4, E = 70: a block is 70 * 17 * 4 = 4,760 B, so every other step's block starts 8 B past a 16 B line."""
    acts = make_actions(24, E, 5, seed=4)
    want = eager_days(KW4, acts)
    assert (want[0].shape[2] * want[0].shape[3] * 4) % 16 == 8
    assert_trajectories_equal(captured_days(KW4, acts, nodes=1), want, "day_lean_kernel, N = 4")
    assert_trajectories_equal(captured_days(KW4, acts, nodes=24, step_nodes=True), want, "step nodes, N = 4")


@pytest.mark.parametrize("step_nodes", [False, True])
def test_steps_only_graph_copies_the_reset_observation(step_nodes):
    acts = make_actions(24, E, 9, seed=5)
    v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **KW8)
    w = SmartNanogridVecEnv(E, seed=SEED, rng="device", **KW8)
    obs0 = v.reset_tensors().clone()
    w.reset_tensors()
    g = EpisodeGraph(v, acts, with_reset=False, trajectory=True, step_nodes=step_nodes)
    assert g.step_nodes_per_day == (24 if step_nodes else 1)
    g.launch()
    torch.cuda.synchronize()
    assert torch.equal(g.obs_traj[0, 0], obs0) and torch.equal(v.obs_d, obs0)   # obs_d: still the reset's
    for t in range(24):
        o, r, d = w.step_tensors(acts[t])
        assert torch.equal(g.obs_traj[0, t + 1], o) and torch.equal(g.reward_traj[0, t], r), t
        assert torch.equal(g.done_traj[0, t], d), t
    assert torch.equal(v.return_d, w.return_d)
    assert v.save_state() == w.save_state()
    g.close()
    v.close()
    w.close()


def test_without_the_flag_the_handles_tensors_are_written_as_before(lean8):
    acts, want = lean8
    v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **KW8)
    g = EpisodeGraph(v, acts, days=DAYS)
    assert g.obs_traj is None and g.reward_traj is None and g.done_traj is None
    g.launch()
    torch.cuda.synchronize()
    assert torch.equal(v.obs_d, want[0][-1, -1]) and torch.equal(v.reward_d, want[1][-1, -1])
    assert torch.equal(v.done_d, want[2][-1, -1])
    assert v.save_state() == want[3]
    g.close()
    v.close()
    np.testing.assert_array_equal(want[2][:, -1].cpu().numpy(), 1)
