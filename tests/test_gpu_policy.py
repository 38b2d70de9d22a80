"""GPU: the MLP actor in the loop (include/sng.h: sng_policy_*, sng_graph_create_policy; policy.py: MlpActor,
ClosedLoopGraph).

With relu the actor is exactly reproducible on the CPU, so everything here but the tanh test is bitwise: the policy
kernel against the host model, and a closed-loop captured day against (i) the same graph with step_nodes=True,
(ii) eager step_tensors fed the clipped stored actions and (iii) the CPU oracle driven with those actions.  Days are
1 h days of T = 24 at E = 70 (one full wavefront and one of 6 live lanes) or E = 1.  Weights are uniform
+-1 / sqrt(fan_in) from a fixed seed with the last layer scaled by OUT_SCALE and Gaussian noise of NOISE_STD, so that
between a tenth and nine tenths of the actions fall strictly inside the Box (asserted: otherwise the clip hides the
network)."""
import ctypes

import numpy as np
import pytest

import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from policy_cases import actor_f64, random_weights  # noqa: E402
from smart_nanogrid_gym import ClosedLoopGraph, MlpActor, SmartNanogridVecEnv, _native, evaluate_models, generate_days  # noqa: E402
from station_matrix_cases import square_mode  # noqa: E402
from test_gpu_station_matrix import load_exported_day  # noqa: E402

SEED, T = 4321, 24
OUT_SCALE, NOISE_STD = 4.0, 0.8
BASE = dict(charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
            battery_system_available_in_model=True, time_interval="1h")

# The factor by which the device's tanh actor may be further from float64 than the host's float32 model is
# (test_tanh_day); chosen after one measurement on an MI355X (ratios 0.99 and 1.09, that test's docstring): 2 leaves
# a different tanhf one more unit in the last place than the host's, and nothing else.  The issue allows at most 8.
TANH_FACTOR = 2.0


def station(N, **kw):
    return dict(BASE, number_of_chargers=N, **kw)


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    square_mode(True)   # x*x squares, as on the GPU
    yield
    square_mode(False)


def make_noise(E, A, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, NOISE_STD, (T, E, A)).astype(np.float32)


def make_actor(venv, activation="relu", clip=True, seed=11, out_scale=OUT_SCALE):
    return MlpActor(venv, activation=activation, clip=clip).load(
        random_weights(venv.obs_dim, venv.act_dim, seed, out_scale))


def clip_to_box(venv, a):
    return np.minimum(np.maximum(a, venv.action_space.low), venv.action_space.high)


# ------------------------------------------------------------------------------------------ 1. policy_kernel, exact
POLICY_STATIONS = {
    "n1": station(1), "n3": station(3), "n8": station(8), "n10": station(10), "n16": station(16), "n50": station(50),
    "n8_no_bess": station(8, battery_system_available_in_model=False),
    "n8_no_pv": station(8, pv_system_available_in_model=False),
}


@pytest.mark.parametrize("name", list(POLICY_STATIONS))
def test_policy_kernel_equals_the_host_model(name):
    kw = POLICY_STATIONS[name]
    E = 70
    v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **kw)
    rng = np.random.default_rng(5)
    recorded = [v.reset_tensors().clone()]
    for _ in range(3):   # observations of a day under way
        a = torch.from_numpy(rng.uniform(v.action_space.low, v.action_space.high, (E, v.act_dim)).astype(np.float32))
        recorded.append(v.step_tensors(a.to(v.device))[0].clone())
    noise = torch.from_numpy(make_noise(E, v.act_dim, 3)[0]).to(v.device)
    checked = clipped = 0
    for clip in (True, False):
        actor = make_actor(v, "relu", clip=clip)
        for obs in (recorded[0], recorded[-1]):
            for nz in (None, noise):
                a, env_a = (x.cpu().numpy() for x in actor.actions(obs, nz))
                want_a, want_env = actor.host_actions(obs, nz)
                np.testing.assert_array_equal(a, want_a, err_msg=f"{name} clip={clip} noise={nz is not None}: a")
                np.testing.assert_array_equal(env_a, want_env, err_msg=f"{name} clip={clip}: env actions")
                if clip:
                    np.testing.assert_array_equal(env_a, clip_to_box(v, a))
                    clipped += int((env_a != a).sum())
                else:
                    np.testing.assert_array_equal(env_a, a)
                checked += a.size
        # the callable: the env actions, rows <= num_envs
        np.testing.assert_array_equal(actor(recorded[0][:7]).cpu().numpy(), actor.host_actions(recorded[0][:7])[1])
        actor.close()
    assert checked == 8 * E * v.act_dim and 0 < clipped < checked // 2   # the clip acts, and not everywhere
    v.close()


def test_create_refuses_what_the_contract_excludes():
    v = SmartNanogridVecEnv(4, seed=SEED, rng="device", **station(8))
    L = _native.lib()

    def create(**kw):
        f = dict(obs_dim=v.obs_dim, act_dim=v.act_dim, hidden=64, activation=0)
        f.update(kw)
        h = ctypes.c_void_p()
        rc = L.sng_policy_create(v._h, ctypes.byref(_native.SngMlpSpec(f["obs_dim"], f["act_dim"], f["hidden"],
                                                                       f["activation"], None, None)), ctypes.byref(h))
        if rc == 0:
            L.sng_policy_destroy(h)
        return rc
    assert create() == 0
    assert create(obs_dim=v.obs_dim + 1) == -1 and create(act_dim=v.act_dim - 1) == -1
    assert create(hidden=32) == -2
    actor = MlpActor(v, "relu")
    bad = random_weights(v.obs_dim, v.act_dim, 1)
    bad[2][5, 5] = np.nan
    with pytest.raises(_native.NativeError, match="non-finite"):
        actor.load(bad)
    actor.close()
    v.close()


# -------------------------------------------------------------------------------------- 2. closed-loop day, exact
DAY_CASES = {
    # name: (station, rng, E, step_nodes of the plan's default form, step_nodes with fused=True): 2 T = the node
    # form, 1 = the fused day (csrc/sng_graph_form.h policy_day_form: the lean plans have it, none has it by default)
    "n1": (station(1), "device", 70, 2 * T, 1),
    "n4": (station(4), "device", 70, 2 * T, 1),
    "n8": (station(8), "device", 70, 2 * T, 1),
    "n8_one_env": (station(8), "device", 1, 2 * T, 1),
    "n16": (station(16), "device", 70, 2 * T, 1),
    "n10_v2x": (station(10, vehicle_to_everything=True), "device", 70, 2 * T, 1),
    "n8_req": (station(8, enable_requested_state_of_charge=True), "device", 70, 2 * T, 1),
    "n8_reference_steps_only": (station(8), "reference", 70, 2 * T, 1),
    "n10_wide": (station(10), "device", 70, 2 * T, 2 * T),
    "n50": (station(50), "device", 70, 2 * T, 2 * T),
}


def closed_loop_day(kw, rng, E, activation="relu", step_nodes=False, trajectory=True, weights_seed=11, launches=1,
                    fused=False, with_noise=True):
    """One captured closed-loop day (the last of `launches`) of a fresh handle: what the graph wrote and left."""
    v = SmartNanogridVecEnv(E, seed=SEED, rng=rng, **kw)
    actor = make_actor(v, activation, seed=weights_seed)
    noise = make_noise(E, v.act_dim, 9)
    with_reset = rng == "device"
    if not with_reset:
        v.reset_tensors()
    if not with_noise:
        noise = np.zeros_like(noise)
    g = ClosedLoopGraph(v, actor, noise=torch.from_numpy(noise).to(v.device) if with_noise else None,
                        with_reset=with_reset, trajectory=trajectory, step_nodes=step_nodes, fused=fused)
    for _ in range(launches):
        g.launch()
    torch.cuda.synchronize()
    out = dict(nodes=g.step_nodes, noise=noise, ret=v.return_d.cpu().numpy(), state=v.save_state(),
               low=v.action_space.low, high=v.action_space.high, kernel=v.step_kernel_name(),
               obs_dim=v.obs_dim, act_dim=v.act_dim,
               last=tuple(x.cpu().numpy() for x in (v.obs_d, g.actions, v.reward_d, v.done_d)))
    if trajectory:
        out.update(obs=g.obs_traj[0].cpu().numpy(), act=g.action_traj[0].cpu().numpy(),
                   rew=g.reward_traj[0].cpu().numpy(), done=g.done_traj[0].cpu().numpy())
        out["host"] = [actor.host_actions(out["obs"][t], noise[t] if with_noise else None) for t in range(T)]
    g.close()
    actor.close()
    v.close()
    return out


_days = {}


def relu_day(name):
    """The relu day of a case, run once and shared by the tests that compare against it (never modified)."""
    if name not in _days:
        kw, rng, E = DAY_CASES[name][:3]
        _days[name] = closed_loop_day(kw, rng, E)
    return _days[name]


def eager_day(kw, rng, E, env_actions):
    """The same day stepped eagerly with given env actions [T, E, A]."""
    v = SmartNanogridVecEnv(E, seed=SEED, rng=rng, **kw)
    obs = [v.reset_tensors().cpu().numpy()]
    rew, done = [], []
    for t in range(T):
        o, r, d = v.step_tensors(torch.from_numpy(env_actions[t]).to(v.device))
        obs.append(o.cpu().numpy())
        rew.append(r.cpu().numpy())
        done.append(d.cpu().numpy())
    torch.cuda.synchronize()
    out = dict(obs=np.stack(obs), rew=np.stack(rew), done=np.stack(done), ret=v.return_d.cpu().numpy(),
               state=v.save_state())
    v.close()
    return out


def assert_env_side_equal(a, b, what):
    for k in ("obs", "rew", "done", "ret"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")
    assert a["state"] == b["state"], f"{what}: state blob"


@pytest.mark.parametrize("name", list(DAY_CASES))
def test_closed_loop_day_relu(name):
    kw, rng, E, nodes, fused_nodes = DAY_CASES[name]
    day = relu_day(name)
    assert day["nodes"] == nodes
    # the actor: every stored action is the host model of the observation it answered, bitwise
    for t in range(T):
        np.testing.assert_array_equal(day["act"][t], day["host"][t][0], err_msg=f"{name} t {t}: actions")
    env_actions = np.stack([h[1] for h in day["host"]])
    np.testing.assert_array_equal(env_actions, np.minimum(np.maximum(day["act"], day["low"]), day["high"]))
    inside = ((day["act"] > day["low"]) & (day["act"] < day["high"])).mean()
    print(f"{name}: {inside:.3f} of the actions strictly inside the Box")
    assert 0.1 < inside < 0.9, inside
    assert (day["rew"] != 0).any() and day["done"][-1].all() and not day["done"][:-1].any()
    # (i) the two forms: step_nodes=True, and fused=True, which is one node exactly where the plan has the fused day
    forced = closed_loop_day(kw, rng, E, step_nodes=True)
    assert forced["nodes"] == 2 * T
    np.testing.assert_array_equal(forced["act"], day["act"], err_msg=f"{name}: step_nodes actions")
    assert_env_side_equal(forced, day, f"{name}: step_nodes=True")
    one = closed_loop_day(kw, rng, E, fused=True)
    assert one["nodes"] == fused_nodes
    np.testing.assert_array_equal(one["act"], day["act"], err_msg=f"{name}: fused actions")
    assert_env_side_equal(one, day, f"{name}: fused=True")
    assert closed_loop_day(kw, rng, E, fused=True, step_nodes=True, trajectory=False)["nodes"] == 2 * T
    # (ii) eager steps fed the clipped stored actions
    assert_env_side_equal(eager_day(kw, rng, E, env_actions), day, f"{name}: eager")
    # (iii) the CPU oracle driven with those actions
    cfg = O.OracleConfig(**kw)
    envs = [O.OracleEnv(cfg, 0 if rng == "device" else SEED + e) for e in range(E)]
    if rng == "device":
        src = SmartNanogridVecEnv(E, seed=SEED, rng="device", **kw)
        src.reset_tensors()
        ivs, ratios = src.get_scenarios(0, E)
        src.close()
        ref0 = np.stack([load_exported_day(e, iv, r) for e, iv, r in zip(envs, ivs, ratios)])
    else:
        ref0 = np.stack([e.reset() for e in envs])
    np.testing.assert_array_equal(day["obs"][0], ref0, err_msg=f"{name}: t = 0 observation vs oracle")
    ret = np.zeros(E)
    for t in range(T):
        outs = [e.step(env_actions[t, i]) for i, e in enumerate(envs)]
        np.testing.assert_array_equal(day["obs"][t + 1], np.stack([x[0] for x in outs]), err_msg=f"{name} t {t}: obs")
        r = np.array([x[1] for x in outs])
        np.testing.assert_array_equal(day["rew"][t], r, err_msg=f"{name} t {t}: reward")
        ret = ret + r
    np.testing.assert_array_equal(day["ret"], ret, err_msg=f"{name}: day return vs oracle")


# ------------------------------------------------------------------------------------------------------- 3. tanh
@pytest.mark.parametrize("N", [8, 16])
def test_tanh_day(N):
    """The env side exactly, against the kernel's own stored actions; the actor against float64.

    d_ref = max |host float32 model - float64| over the day's rows, d_dev the same for the device's stored actions;
    the device may exceed d_ref by TANH_FACTOR, which covers a different tanhf and nothing else.  Measured on an
    MI355X (ROCm 7.2): N = 8: d_ref 7.55e-07, d_dev 7.44e-07 (ratio 0.99); N = 16: d_ref 6.57e-07, d_dev 7.17e-07
    (ratio 1.09); no step's actions were bitwise the host model's.  TANH_FACTOR = 2."""
    kw, E = station(N), 70
    day = closed_loop_day(kw, "device", E, activation="tanh")
    assert day["nodes"] == 2 * T
    one = closed_loop_day(kw, "device", E, activation="tanh", fused=True)   # the same tanhf, the same bits
    assert one["nodes"] == 1
    np.testing.assert_array_equal(one["act"], day["act"])
    assert_env_side_equal(one, day, f"tanh N = {N}: fused")
    env_actions = np.minimum(np.maximum(day["act"], day["low"]), day["high"])
    assert_env_side_equal(eager_day(kw, "device", E, env_actions), day, f"tanh N = {N}: eager")
    weights = random_weights(day["obs"].shape[-1], day["act"].shape[-1], 11, OUT_SCALE)
    d_ref = d_dev = 0.0
    for t in range(T):
        ref = actor_f64(day["obs"][t], weights, "tanh", day["noise"][t])
        d_ref = max(d_ref, np.abs(day["host"][t][0].astype(np.float64) - ref).max())
        d_dev = max(d_dev, np.abs(day["act"][t].astype(np.float64) - ref).max())
    same = np.mean([np.array_equal(day["act"][t], day["host"][t][0]) for t in range(T)])
    print(f"tanh N = {N}: d_ref {d_ref:.4e}, d_dev {d_dev:.4e}, ratio {d_dev / d_ref:.3f}, factor {TANH_FACTOR}, "
          f"{same:.2f} of the steps bitwise equal to the host model")
    inside = ((day["act"] > day["low"]) & (day["act"] < day["high"])).mean()
    assert 0.1 < inside < 0.9, inside
    assert d_dev <= TANH_FACTOR * d_ref


# ------------------------------------------------------------------------------------- 4. without the trajectory
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", ["n8", "n10_wide", "n8_reference_steps_only"])
def test_without_the_trajectory_the_blocks_hold_the_last_step(name, fused):
    kw, rng, E, nodes, fused_nodes = DAY_CASES[name]
    want = relu_day(name)
    got = closed_loop_day(kw, rng, E, trajectory=False, fused=fused)
    assert got["nodes"] == (fused_nodes if fused else nodes)
    obs, act, rew, done = got["last"]
    np.testing.assert_array_equal(obs, want["obs"][-1])
    np.testing.assert_array_equal(act, want["act"][-1])
    np.testing.assert_array_equal(rew, want["rew"][-1])
    np.testing.assert_array_equal(done, want["done"][-1])
    np.testing.assert_array_equal(got["ret"], want["ret"])
    assert got["state"] == want["state"]


@pytest.mark.parametrize("name", ["n8", "n4", "n10_wide"])
def test_without_noise_both_forms(name):
    """No noise block: the mean is the action.  N = 4 at E = 70 has blocks that are not 16 B multiples."""
    kw, rng, E, nodes, fused_nodes = DAY_CASES[name]
    day = closed_loop_day(kw, rng, E, with_noise=False)
    for t in range(T):
        np.testing.assert_array_equal(day["act"][t], day["host"][t][0], err_msg=f"{name} t {t}")
    one = closed_loop_day(kw, rng, E, with_noise=False, fused=True)
    assert one["nodes"] == fused_nodes
    np.testing.assert_array_equal(one["act"], day["act"])
    assert_env_side_equal(one, day, f"{name}: fused, no noise")
    last = closed_loop_day(kw, rng, E, with_noise=False, fused=True, trajectory=False)
    np.testing.assert_array_equal(last["last"][1], day["act"][-1])
    assert last["state"] == day["state"]


# ------------------------------------------------------------------------------------------- 5. weight refresh
@pytest.mark.parametrize("fused", [False, True])
def test_new_weights_take_effect_without_a_recapture(fused):
    kw, E = station(8), 70
    noise = torch.from_numpy(make_noise(E, 9, 9)).to("cuda:0")
    runs = []
    for recapture in (False, True):
        v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **kw)
        actor = make_actor(v, "relu", seed=11)
        g = ClosedLoopGraph(v, actor, noise=noise, trajectory=True, fused=fused)
        g.launch()
        first = g.action_traj.clone()
        actor.load(random_weights(v.obs_dim, v.act_dim, 12, OUT_SCALE))
        if recapture:
            g.close()
            g = ClosedLoopGraph(v, actor, noise=noise, trajectory=True, fused=fused)
        g.launch()
        torch.cuda.synchronize()
        runs.append((first.cpu().numpy(), g.action_traj.cpu().numpy(), g.obs_traj.cpu().numpy(),
                     g.reward_traj.cpu().numpy(), v.save_state()))
        # the second day's actions are the new weights' answers
        want = actor.host_actions(runs[-1][2][0, 5], noise[5].cpu().numpy())[0]
        np.testing.assert_array_equal(runs[-1][1][0, 5], want)
        g.close()
        actor.close()
        v.close()
    for a, b in zip(runs[0][:4], runs[1][:4]):
        np.testing.assert_array_equal(a, b)
    assert runs[0][4] == runs[1][4]
    assert not np.array_equal(runs[0][0], runs[0][1])


# --------------------------------------------------------------------------------------------------- 6. two days
@pytest.mark.parametrize("fused", [False, True])
def test_two_days_in_one_graph_equal_two_launches(fused):
    kw, E = station(8), 70
    noise = torch.from_numpy(make_noise(E, 9, 9)).to("cuda:0")
    v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **kw)
    actor = make_actor(v, "relu")
    rets = torch.zeros((2, E), dtype=torch.float64, device=v.device)
    g = ClosedLoopGraph(v, actor, noise=noise, days=2, day_returns=rets, fused=fused)
    assert g.step_nodes == (1 if fused else 2 * T)
    assert _native.lib().sng_graph_reset_overlapped(g._g) == 0   # policy graphs capture the serial chain
    g.launch()
    torch.cuda.synchronize()
    w = SmartNanogridVecEnv(E, seed=SEED, rng="device", **kw)
    actor_w = make_actor(w, "relu")
    one = torch.zeros((1, E), dtype=torch.float64, device=w.device)
    gw = ClosedLoopGraph(w, actor_w, noise=noise, days=1, day_returns=one)
    for d in range(2):
        gw.launch()
        torch.cuda.synchronize()
        assert torch.equal(rets[d], one[0]), d
    assert bool((rets[0] != rets[1]).any()) and bool((rets != 0).all())
    assert torch.equal(v.obs_d, w.obs_d) and torch.equal(g.actions, gw.actions)
    assert v.save_state() == w.save_state()
    for x in (g, gw, actor, actor_w, v, w):
        x.close()


def test_closing_order():
    """The env batch closes its actors; a graph refuses to launch without its actor."""
    v = SmartNanogridVecEnv(4, seed=SEED, rng="device", **station(8))
    actor = make_actor(v, "relu")
    g = ClosedLoopGraph(v, actor)
    g.launch()
    torch.cuda.synchronize()
    actor.close()
    with pytest.raises(RuntimeError, match="closed"):
        g.launch()
    with pytest.raises(ValueError, match="closed"):
        ClosedLoopGraph(v, actor)
    g.close()
    other = make_actor(v, "relu")
    v.close()
    assert other._p is None


# ------------------------------------------------------------------------------------- 7. callable in the evaluators
def test_actor_as_a_policy_of_evaluate_models():
    kw, episodes = station(8), 6
    days = generate_days(episodes, seed=SEED, rng="reference", **kw)
    v = SmartNanogridVecEnv(episodes, seed=SEED, rng="reference", **kw)
    actor = make_actor(v, "relu")
    final, mean = evaluate_models({"mlp": actor}, seed=SEED, rng="reference", days=days, **kw)
    v.reset_from_initial_values(list(days[0]), days[1], restore_requested_soc=True)
    rets = torch.zeros((1, episodes), dtype=torch.float64, device=v.device)
    g = ClosedLoopGraph(v, actor, with_reset=False, day_returns=rets)
    g.launch()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(final["mlp"], rets[0].cpu().numpy())
    assert mean["mlp"] == float(np.mean(rets[0].cpu().numpy())) and (final["mlp"] != 0).all()
    g.close()
    actor.close()
    v.close()
