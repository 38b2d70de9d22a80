"""GPU: the policy matrix (policy_matrix_cases.py) -- closed-loop captured days (policy_kernel,
day_lean_policy_kernel, policy_net_kernel, ClosedLoopGraph) and PPO rollouts (rollout_gae_kernel, PpoHead, PpoRollout)
at every row of the station matrix: T = 6, 12, 24, 48, 72 and 96, stations without PV or without BESS, every penalty
mode, the extended 15 min day, the general kernel as the step node (20 min dt, legacy promotion), N = 50, and
reference-RNG days with unpacked records and the requested-SoC stream.

The reference is the independent CPU loop (policy_matrix_cases.cpu_closed_loop): oracle observation -> host actor ->
clip -> oracle step.  It never reads an action, an observation or a reward the device wrote; the days themselves are
exported from a twin handle of the same seed that only resets (device rows) or are the oracle's own (reference rows).
Every step of both days is compared bit for bit: a wrong value at step 3 of day 1 shows there, as the first mismatch.

Device rows run days = 2 in one launch; reference rows run a steps-only graph of one day twice, with a reset_tensors()
before each launch.  E = 70.
"""
import numpy as np
import pytest

import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from policy_matrix_cases import (DAYS, DDPG_ROW, E, GAE_LAMBDA, GAMMA, IDS, LEAN_ROWS, NET_ARCH, NET_ROWS, OUT_SCALE,  # noqa: E402
                                 SEED, Coverage, actor_weights, check_actions, cpu_day, given_actions, log_std, matrix_noise,
                                 net_host_actions, row_of, square_mode, value_weights)
from policy_net_cases import net_f64, random_net_weights, unscale_f32  # noqa: E402
from smart_nanogrid_gym import ClosedLoopGraph, MlpActor, PpoHead, PpoRollout, SmartNanogridVecEnv, policy  # noqa: E402
from station_matrix_cases import padded  # noqa: E402
from test_gpu_day_kernel import flags_of  # noqa: E402
from test_gpu_day_lean_kernel import oracle_flags  # noqa: E402
from test_gpu_policy_net import SQUASH_FACTOR  # noqa: E402
from test_gpu_station_matrix import load_exported_day  # noqa: E402

TRAJ = ("obs", "act", "rew", "done")
PPO = ("values", "advantages", "returns", "log_prob")


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    square_mode(True)   # x*x squares, as on the GPU
    yield
    square_mode(False)


def make_env(row):
    return SmartNanogridVecEnv(E, seed=SEED, rng=row.rng, **row.kw)


_exports = {}


def exported_days(row):
    """The days a device row's graph resets will draw, from a twin handle of the same seed that only resets (a day
    that was reset but never stepped is counted by the next reset); never modified."""
    if row.name not in _exports:
        src = make_env(row)
        days = []
        for _ in range(DAYS):
            src.reset_tensors()
            days.append(src.get_scenarios(0, E))
        src.close()
        _exports[row.name] = days
    return _exports[row.name]


def cpu_reference(row, T, weights, noise, low, high, host_actions, env_actions=None):
    """Both days on the CPU: cpu_day's dicts, the OR of the oracle's flags and the coverage counts.  env_actions
    [DAYS, T, E, A]: the oracle is driven with these instead of the host actor's (the squashed actor's rule)."""
    device = row.rng == "device"
    cfg = O.OracleConfig(**row.kw)
    assert cfg.T == T
    envs = [O.OracleEnv(cfg, 0 if device else SEED + e) for e in range(E)]
    cov = Coverage(row, T)
    flags = np.zeros(E, np.uint32)
    days = []
    for day in range(DAYS):
        if device:
            ivs, ratios = exported_days(row)[day]
            obs0 = np.stack([load_exported_day(e, iv, r) for e, iv, r in zip(envs, ivs, ratios)])
            cov.add_day(np.array([iv["Charger_occupancy"] for iv in ivs]),
                        np.stack([padded(iv["Arrivals"], 32) for iv in ivs]),
                        np.stack([padded(iv["Departures"], 32) for iv in ivs]))
        else:
            obs0 = np.stack([e.reset() for e in envs])
            model = [e.scenario(vmax=32) for e in envs]
            cov.add_day(*(np.stack([d[k] for d in model]) for k in ("occ", "arrivals", "departures")))
        d = cpu_day(envs, obs0, weights, noise, low, high,
                    host_actions if env_actions is None else given_actions(env_actions[day]), cov)
        for step in d["infos"]:
            assert all(i["error"] in (0, 1) for i in step)
            flags |= oracle_flags(step)
        days.append(d)
    return dict(days=days, flags=flags, cov=cov)


def device_days(row, make_actor, noise, rollout=False, step_nodes=False, fused=False, trajectory=True):
    """Both days of a fresh handle of the matrix's seed with the actor in the loop, as a PpoRollout or a plain
    ClosedLoopGraph: what the graph wrote and left."""
    device = row.rng == "device"
    v = make_env(row)
    actor = make_actor(v)
    if not device:
        v.reset_tensors()
    days = DAYS if device else 1
    ro = head = rets = None
    if rollout:
        head = PpoHead(v, "relu").load(value_weights(v.obs_dim), log_std(v.act_dim))
        ro = PpoRollout(v, actor, head, days=days, gamma=GAMMA, gae_lambda=GAE_LAMBDA, with_reset=device)
        ro.noise.copy_(torch.from_numpy(noise))
        g = ro.graph
    else:
        if device:   # a steps-only graph's row is zeroed by nobody: its returns are read from return_d
            rets = torch.zeros((days, E), dtype=torch.float64, device=v.device)
        g = ClosedLoopGraph(v, actor, noise=torch.from_numpy(noise).to(v.device), days=days, with_reset=device,
                            trajectory=trajectory, day_returns=rets, step_nodes=step_nodes, fused=fused)
    out = dict(nodes=g.step_nodes, ret={}, T=v.timesteps, low=np.asarray(v.action_space.low, np.float32),
               high=np.asarray(v.action_space.high, np.float32))
    chunks = []
    for launch in range(DAYS // days):
        if launch:
            v.reset_tensors()
        (ro if rollout else g).launch()
        torch.cuda.synchronize()
        c = {}
        if trajectory:
            c.update(obs=g.obs_traj, act=g.action_traj, rew=g.reward_traj, done=g.done_traj)
        if rollout:
            c.update(starts=ro.episode_starts, values=ro.values, advantages=ro.advantages, returns=ro.returns,
                     log_prob=ro.log_prob)
        chunks.append({k: x.cpu().numpy() for k, x in c.items()})
        if rets is None:
            out["ret"][launch * days + days - 1] = v.return_d.cpu().numpy()
        else:
            out["ret"].update({d: rets[d].cpu().numpy() for d in range(days)})
            v.return_d.copy_(rets[days - 1])   # day_returns' rows took what return_d (and the checkpoint) holds
    for k in chunks[0]:
        out[k] = np.concatenate([c[k] for c in chunks])
    out.update(kernel=v.step_kernel_name(), flags=flags_of(v), state=v.save_state(), head=head,
               last=tuple(x.cpu().numpy() for x in (v.obs_d, g.actions, v.reward_d, v.done_d)))
    g.close()
    if not rollout:
        actor.close()
        v.close()
    else:
        out["close"] = v.close   # the head's host model is still wanted
    return out


def assert_equals_cpu_loop(name, got, ref):
    """Every step of both days, the day returns and the sticky flags against the CPU loop."""
    for day, want in enumerate(ref["days"]):
        for t in range(got["T"]):
            what = f"{name} day {day} t {t}"
            np.testing.assert_array_equal(got["obs"][day, t], want["obs"][t], err_msg=what + ": obs answered")
            np.testing.assert_array_equal(got["act"][day, t], want["act"][t], err_msg=what + ": a")
            np.testing.assert_array_equal(got["rew"][day, t], want["rew"][t], err_msg=what + ": reward")
            np.testing.assert_array_equal(got["done"][day, t], want["done"][t], err_msg=what + ": done")
        np.testing.assert_array_equal(got["obs"][day, -1], want["obs"][-1], err_msg=f"{name} day {day}: last obs")
        if day in got["ret"]:
            np.testing.assert_array_equal(got["ret"][day], want["ret"], err_msg=f"{name} day {day}: day return")
    assert DAYS - 1 in got["ret"]
    np.testing.assert_array_equal(got["flags"], ref["flags"], err_msg=f"{name}: sticky flags")


def assert_same_run(name, got, want, what):
    for k in TRAJ:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name}: {what}: {k}")
    for day, r in got["ret"].items():
        if day in want["ret"]:
            np.testing.assert_array_equal(r, want["ret"][day], err_msg=f"{name}: {what}: day {day} return")
    assert got["state"] == want["state"], f"{name}: {what}: state blob"


# --------------------------------------------------------------------------------- 1. the rollout at every row
@pytest.mark.parametrize("name", IDS)
def test_row_rollout_vs_the_independent_cpu_loop(name):
    row = row_of(name)
    lean = name in LEAN_ROWS
    probe = O.OracleConfig(**row.kw)
    T, A = probe.T, probe.act_dim
    weights = actor_weights(probe.obs_dim, A)
    noise = matrix_noise(row, T, A)

    def make_actor(v):
        return MlpActor(v, "relu").load(weights)
    got = device_days(row, make_actor, noise, rollout=True)
    assert got["kernel"] == row.kernel, (name, got["kernel"])
    assert got["T"] == T and got["obs"].shape == (DAYS, T + 1, E, probe.obs_dim)
    assert got["nodes"] == 2 * T, (name, got["nodes"])   # no plan has the fused day by default
    low, high = got["low"], got["high"]
    ref = cpu_reference(row, T, weights, noise, low, high, policy.host_actions)
    assert_equals_cpu_loop(name, got, ref)
    share = check_actions(row, ref["days"], noise, low, high)
    print(f"{name}: T = {T}, kernel {got['kernel']}, inside the Box {share:.3f}, {dict(ref['cov'].counts)}")
    ref["cov"].check()
    # the PPO half: the host model on the CPU loop's trajectory, not on the device's copy of it
    obs, rew, done = (np.stack([d[k] for d in ref["days"]]) for k in ("obs", "rew", "done"))
    want = got["head"].host_finish(obs, rew, done, noise, GAMMA, GAE_LAMBDA)
    for k, b in zip(PPO, want):
        assert got[k].shape == b.shape and got[k].dtype == b.dtype == np.float32
        np.testing.assert_array_equal(got[k], b, err_msg=f"{name}: {k}")
    assert np.isfinite(got["log_prob"]).all() and got["log_prob"].min() < -1000.0   # the +-100 entries
    assert np.unique(got["values"]).size > got["values"].size // 2
    starts = np.ones((DAYS, T, E), np.uint8)
    starts[:, 1:] = done[:, :-1]
    np.testing.assert_array_equal(got["starts"], starts, err_msg=f"{name}: episode_starts")
    assert starts[:, 0].all() and not starts[:, 1:].any()
    got["close"]()
    # the forms: a fresh handle of the same seed each, the same bytes
    forced = device_days(row, make_actor, noise, step_nodes=True)
    assert forced["nodes"] == 2 * T, (name, forced["nodes"])
    assert_same_run(name, forced, got, "step_nodes=True")
    one = device_days(row, make_actor, noise, fused=True)
    assert one["nodes"] == (1 if lean else 2 * T), (name, one["nodes"])
    assert_same_run(name, one, got, "fused=True")
    np.testing.assert_array_equal(one["flags"], got["flags"])
    if lean:
        last = device_days(row, make_actor, noise, fused=True, trajectory=False)
        assert last["nodes"] == 1
        for x, k in zip(last["last"], TRAJ):
            np.testing.assert_array_equal(x, got[k][-1, -1], err_msg=f"{name}: no trajectory: {k}")
        for day, r in last["ret"].items():
            np.testing.assert_array_equal(r, ref["days"][day]["ret"], err_msg=f"{name}: no trajectory: day {day} return")
        assert last["state"] == got["state"], f"{name}: no trajectory: state blob"


def test_six_rows_have_the_fused_day():
    assert len(LEAN_ROWS) == 6 and len(IDS) == 18


# --------------------------------------------------------------------------------------- 2. the any-width actor
@pytest.mark.parametrize("name", NET_ROWS)
def test_any_width_actor_vs_the_independent_cpu_loop(name):
    """MlpActor(net_arch=(33, 65)) on policy_net_kernel: the mean output with the clip, bitwise through
    host_actions(..., net_arch=(33, 65)); its days are nodes whatever is asked."""
    row = row_of(name)
    probe = O.OracleConfig(**row.kw)
    T, A = probe.T, probe.act_dim
    weights = random_net_weights(probe.obs_dim, A, NET_ARCH, 11, OUT_SCALE)
    noise = matrix_noise(row, T, A)

    def make_actor(v):
        actor = MlpActor(v, "relu", net_arch=NET_ARCH).load(weights)
        assert actor.net
        return actor
    got = device_days(row, make_actor, noise, fused=True)
    assert got["kernel"] == row.kernel and got["nodes"] == 2 * T, (name, got["kernel"], got["nodes"])
    ref = cpu_reference(row, T, weights, noise, got["low"], got["high"], net_host_actions(policy))
    assert_equals_cpu_loop(name, got, ref)
    share = check_actions(row, ref["days"], noise, got["low"], got["high"])
    print(f"{name} {NET_ARCH}: inside the Box {share:.3f}, {dict(ref['cov'].counts)}")
    ref["cov"].check()


# ------------------------------------------------------------------------------------- 3. the squashed DDPG actor
def test_ddpg_actor_on_the_v2x_box():
    """MlpActor.ddpg at general10_20min_v2x, by test_gpu_policy_net.test_closed_loop_ddpg_day's rule: the first Box
    with a lower bound of -1 on the chargers for the squash on the device.  tanhf is not bitwise, so the env actions
    are the host unscale of the device's stored a, bitwise; the env side is the oracle driven by those env actions,
    bitwise at every step of both days; and a against float64 stays within SQUASH_FACTOR of the host model's own
    distance."""
    name = DDPG_ROW
    row = row_of(name)
    probe = O.OracleConfig(**row.kw)
    T, A = probe.T, probe.act_dim
    weights = random_net_weights(probe.obs_dim, A, (400, 300), 11, OUT_SCALE)
    noise = matrix_noise(row, T, A)

    def make_actor(v):
        return MlpActor.ddpg(v).load(weights)
    got = device_days(row, make_actor, noise)
    low, high = got["low"], got["high"]
    assert got["kernel"] == row.kernel and got["nodes"] == 2 * T
    assert (low == -1).all() and (high == 1).all()
    assert (np.abs(got["act"]) <= 1).all()
    # the eager loop: the device's env actions are the host unscale of the stored a
    v = make_env(row)
    actor = make_actor(v)
    noise_d = torch.from_numpy(noise).to(v.device)
    env = np.zeros_like(got["act"])
    for day in range(DAYS):
        obs_t = v.reset_tensors()
        for t in range(T):
            what = f"{name} day {day} t {t}"
            np.testing.assert_array_equal(obs_t.cpu().numpy(), got["obs"][day, t], err_msg=what + ": eager obs")
            a, env_a = actor.actions(obs_t, noise_d[t])
            np.testing.assert_array_equal(a.cpu().numpy(), got["act"][day, t], err_msg=what + ": eager a")
            env[day, t] = env_a.cpu().numpy()
            obs_t, r, _ = v.step_tensors(env_a)
            np.testing.assert_array_equal(r.cpu().numpy(), got["rew"][day, t], err_msg=what + ": eager reward")
    assert v.save_state() == got["state"]
    np.testing.assert_array_equal(env, unscale_f32(got["act"], low, high))
    assert (env >= low).all() and (env <= high).all()
    assert (env[:, noise == np.float32(-100.0)] == -1).all() and (env[:, noise == np.float32(100.0)] == 1).all()
    # a against float64, on the device's own observations
    d_ref = d_dev = 0.0
    for day in range(DAYS):
        for t in range(T):
            o = got["obs"][day, t]
            r64 = net_f64(o, weights, "relu", noise[t], squash=True)
            d_ref = max(d_ref, np.abs(actor.host_actions(o, noise[t])[0].astype(np.float64) - r64).max())
            d_dev = max(d_dev, np.abs(got["act"][day, t].astype(np.float64) - r64).max())
    print(f"{name} ddpg: d_ref {d_ref:.4e}, d_dev {d_dev:.4e}, ratio {d_dev / d_ref:.3f}, factor {SQUASH_FACTOR}")
    assert d_dev <= SQUASH_FACTOR * d_ref
    actor.close()
    v.close()
    # the env side: the oracle driven by those env actions
    ref = cpu_reference(row, T, weights, noise, low, high, None, env_actions=env)
    for day, want in enumerate(ref["days"]):
        for t in range(T + 1):
            np.testing.assert_array_equal(got["obs"][day, t], want["obs"][t], err_msg=f"{name} day {day} t {t}: obs")
        np.testing.assert_array_equal(got["rew"][day], want["rew"], err_msg=f"{name} day {day}: rewards")
        np.testing.assert_array_equal(got["done"][day], want["done"], err_msg=f"{name} day {day}: dones")
        np.testing.assert_array_equal(got["ret"][day], want["ret"], err_msg=f"{name} day {day}: day return")
    np.testing.assert_array_equal(got["flags"], ref["flags"])
    assert ref["flags"].any()   # the breakpoint flag of V2X discharging
    ref["cov"].check()
