"""GPU: the MLP actor of any width on the f32-input MFMA (include/sng.h: sng_policy_create_net; csrc/sng_policy_net.h:
policy_net_kernel; policy.py: MlpActor(net_arch=..., squash=...), MlpActor.ddpg).

With relu hidden layers and the mean output the kernel is exactly reproducible on the CPU (the MFMA's result is the
k-ordered fmaf chain; the kernel's trailing zero terms can only turn a -0 into +0, so the comparisons are by value).
With the squashed output the means are still exact and only tanhf differs.  E = 70: one full 64-row block and one of
6 rows, so a workgroup with both row tiles live and one with a partial first tile and an empty second both run.
Days are 1 h days of T = 24."""
import ctypes

import numpy as np
import pytest

import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from policy_cases import random_weights  # noqa: E402
from policy_net_cases import NETS, net_f64, random_net_weights, unscale_f32  # noqa: E402
from smart_nanogrid_gym import ClosedLoopGraph, MlpActor, SmartNanogridVecEnv, _native, evaluate_models, generate_days  # noqa: E402
from station_matrix_cases import square_mode  # noqa: E402
from test_gpu_station_matrix import load_exported_day  # noqa: E402

SEED, T, E = 4321, 24, 70
OUT_SCALE, NOISE_STD = 4.0, 0.8
BASE = dict(charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
            battery_system_available_in_model=True, time_interval="1h")

# The factor by which the device's actor may be further from float64 than the host's float32 model is, where a tanhf
# is in the way (tests/test_gpu_policy.py test_tanh_day's rule): 2 where the measured ratio d_dev / d_ref is below 1.5,
# else the next power of two, never above 8.  The ratios measured on an MI355X are in the docstrings of the tests.
SQUASH_FACTOR = 2.0
TANH_FACTOR = 2.0


def station(N, **kw):
    return dict(BASE, number_of_chargers=N, **kw)


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    square_mode(True)   # x*x squares, as on the GPU
    yield
    square_mode(False)


def make_noise(A, seed):
    return np.random.default_rng(seed).normal(0.0, NOISE_STD, (T, E, A)).astype(np.float32)


def recorded_observations(v):
    """A reset's observation and one three steps into the day."""
    rng = np.random.default_rng(5)
    first = v.reset_tensors().clone()
    for _ in range(3):
        a = torch.from_numpy(rng.uniform(v.action_space.low, v.action_space.high, (E, v.act_dim)).astype(np.float32))
        last = v.step_tensors(a.to(v.device))[0].clone()
    return first, last


# ------------------------------------------------------------------------------------ 1. policy_net_kernel, exact
# N = 50: A = 51, two output tiles.  N = 63: A = 64, both output tiles full, the widest station the kernel takes
# (test_create_net_refuses_what_the_contract_excludes has N = 64).
EXACT_CASES = ([(n, net) for n in (1, 4, 10) for net in NETS] + [(50, (400, 300)), (50, (64, 64))]
               + [(63, (400, 300)), (63, (64, 64))])


@pytest.mark.parametrize("N,net", EXACT_CASES, ids=[f"n{n}-{a}x{b}" for n, (a, b) in EXACT_CASES])
def test_kernel_equals_the_host_model(N, net):
    v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **station(N))
    weights = random_net_weights(v.obs_dim, v.act_dim, net, 11, OUT_SCALE)
    observations = recorded_observations(v)
    noise = torch.from_numpy(make_noise(v.act_dim, 3)[0]).to(v.device)
    checked = clipped = 0
    for clip in (True, False):
        actor = MlpActor(v, "relu", clip=clip, net_arch=net, net=True).load(weights)
        assert actor.net
        old = MlpActor(v, "relu", clip=clip).load(weights) if net == (64, 64) else None
        for obs in observations:
            for nz in (None, noise):
                a, env_a = (x.cpu().numpy() for x in actor.actions(obs, nz))
                want_a, want_env = actor.host_actions(obs, nz)
                what = f"N={N} {net} clip={clip} noise={nz is not None}"
                np.testing.assert_array_equal(a, want_a, err_msg=what + ": a")
                np.testing.assert_array_equal(env_a, want_env, err_msg=what + ": env actions")
                if old is not None:   # policy_kernel, the VALU form of the same contract
                    old_a, old_env = (x.cpu().numpy() for x in old.actions(obs, nz))
                    np.testing.assert_array_equal(a, old_a, err_msg=what + ": a vs policy_kernel")
                    np.testing.assert_array_equal(env_a, old_env, err_msg=what + ": env actions vs policy_kernel")
                if clip:
                    np.testing.assert_array_equal(env_a, np.minimum(np.maximum(a, v.action_space.low), v.action_space.high))
                    clipped += int((env_a != a).sum())
                else:
                    np.testing.assert_array_equal(env_a, a)
                checked += a.size
        np.testing.assert_array_equal(actor(observations[0][:7]).cpu().numpy(), actor.host_actions(observations[0][:7])[1])
        actor.close()
        if old is not None:
            old.close()
    assert checked == 8 * E * v.act_dim and 0 < clipped < checked // 2   # the clip acts, and not everywhere
    v.close()


# ------------------------------------------------------------------------------------------------------ 2. squash
def distances(actor, weights, activation, observations, noise):
    """d_ref, d_dev: max |host float32 model - float64| and max |device - float64| over the rows, for the squashed
    a; and the device's outputs for the caller's own checks."""
    d_ref = d_dev = 0.0
    outs = []
    for obs in observations:
        for nz in (None, noise):
            a, env_a = (x.cpu().numpy() for x in actor.actions(obs, nz))
            host_a = actor.host_actions(obs, nz)[0]
            ref = net_f64(obs.cpu().numpy(), weights, activation, None if nz is None else nz.cpu().numpy(), squash=True)
            d_ref = max(d_ref, np.abs(host_a.astype(np.float64) - ref).max())
            d_dev = max(d_dev, np.abs(a.astype(np.float64) - ref).max())
            outs.append((a, env_a, host_a, nz))
    return d_ref, d_dev, outs


@pytest.mark.parametrize("N,net", [(4, (400, 300)), (10, (400, 300)), (4, (33, 65)), (50, (400, 300))],
                         ids=["n4-ddpg", "n10-ddpg", "n4-33x65", "n50-ddpg"])
def test_squash_relu(N, net):
    """relu hidden layers: the means are exact, so only tanhf separates device and host.  The stored a lies in
    [-1, 1]; the env actions are the host's unscale arithmetic on the device's a, bitwise; the [-1, 1] clip acts on
    some, fewer than half, of the noisy values; and a against float64 within SQUASH_FACTOR of the host's own distance.
    Measured on an MI355X (ROCm 7.2), d_dev / d_ref: n4-ddpg 1.000 (d_ref 2.53e-07), n10-ddpg 0.948 (3.00e-07),
    n4-33x65 1.000 (2.03e-07), n50-ddpg 0.971 (5.08e-07): all below 1.5, so SQUASH_FACTOR = 2."""
    v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **station(N))
    weights = random_net_weights(v.obs_dim, v.act_dim, net, 11, OUT_SCALE)
    actor = MlpActor(v, "relu", net_arch=net, squash=True).load(weights)
    low, high = v.action_space.low, v.action_space.high
    assert (low[:-1] == 0).all() and low[-1] == -1, "chargers without V2X: the rescale is not the identity"
    noise = torch.from_numpy(make_noise(v.act_dim, 3)[0]).to(v.device)
    d_ref, d_dev, outs = distances(actor, weights, "relu", recorded_observations(v), noise)
    acted = total = 0
    for a, env_a, host_a, nz in outs:
        assert (np.abs(a) <= 1).all()
        np.testing.assert_array_equal(env_a, unscale_f32(a, low, high))
        assert (env_a >= low).all() and (env_a <= high).all()
        if nz is None:
            plain = a   # tanh(mean) of the same observation, ahead of its noisy run
        else:
            want = np.minimum(np.maximum(plain + nz.cpu().numpy(), np.float32(-1)), np.float32(1))
            np.testing.assert_array_equal(a, want)   # one float32 add, then the clip
            acted += int((np.abs(plain + nz.cpu().numpy()) > 1).sum())
            total += a.size
    print(f"squash relu N = {N} {net}: d_ref {d_ref:.4e}, d_dev {d_dev:.4e}, ratio {d_dev / d_ref:.3f}, "
          f"factor {SQUASH_FACTOR}, the [-1, 1] clip acted on {acted} of {total}")
    assert 0 < acted < total // 2
    assert d_dev <= SQUASH_FACTOR * d_ref
    actor.close()
    v.close()


@pytest.mark.parametrize("net", [(64, 64), (400, 300)], ids=["64x64", "400x300"])
def test_squash_tanh_hidden_layers(net):
    """tanh hidden layers too (SAC's and PPO's activation): every layer passes through the device's tanhf.  The same
    rule with TANH_FACTOR.  Measured on an MI355X (ROCm 7.2), d_dev / d_ref at N = 4: 64x64 0.885 (d_ref 3.73e-07),
    400x300 1.102 (5.82e-07): both below 1.5, so TANH_FACTOR = 2."""
    v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **station(4))
    weights = random_net_weights(v.obs_dim, v.act_dim, net, 11, OUT_SCALE)
    actor = MlpActor(v, "tanh", net_arch=net, squash=True).load(weights)
    noise = torch.from_numpy(make_noise(v.act_dim, 3)[0]).to(v.device)
    d_ref, d_dev, outs = distances(actor, weights, "tanh", recorded_observations(v), noise)
    for a, env_a, host_a, nz in outs:
        assert (np.abs(a) <= 1).all()
        np.testing.assert_array_equal(env_a, unscale_f32(a, v.action_space.low, v.action_space.high))
    print(f"squash tanh {net}: d_ref {d_ref:.4e}, d_dev {d_dev:.4e}, ratio {d_dev / d_ref:.3f}, factor {TANH_FACTOR}")
    assert d_dev <= TANH_FACTOR * d_ref
    actor.close()
    v.close()


# -------------------------------------------------------------------------------------------- 3. closed-loop days
def ddpg_actor(v, seed=11):
    return MlpActor.ddpg(v).load(random_net_weights(v.obs_dim, v.act_dim, (400, 300), seed, OUT_SCALE))


def graph_day(kw, fused=False, trajectory=True):
    v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **kw)
    actor = ddpg_actor(v)
    assert actor.net_arch == (400, 300) and actor.squash and actor.activation == "relu"
    noise = make_noise(v.act_dim, 9)
    g = ClosedLoopGraph(v, actor, noise=torch.from_numpy(noise).to(v.device), trajectory=trajectory, fused=fused)
    g.launch()
    torch.cuda.synchronize()
    out = dict(nodes=g.step_nodes, ret=v.return_d.cpu().numpy(), state=v.save_state(),
               last=tuple(x.cpu().numpy() for x in (v.obs_d, g.actions, v.reward_d, v.done_d)))
    if trajectory:
        out.update(obs=g.obs_traj[0].cpu().numpy(), act=g.action_traj[0].cpu().numpy(),
                   rew=g.reward_traj[0].cpu().numpy(), done=g.done_traj[0].cpu().numpy())
    g.close()
    actor.close()
    v.close()
    return out


def eager_day(kw):
    """The same day as an eager loop: actor.actions -> step_tensors."""
    v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **kw)
    actor = ddpg_actor(v)
    noise = torch.from_numpy(make_noise(v.act_dim, 9)).to(v.device)
    obs_t = v.reset_tensors()
    obs, act, env, rew, done = [obs_t.cpu().numpy()], [], [], [], []
    for t in range(T):
        a, env_a = actor.actions(obs_t, noise[t])
        act.append(a.cpu().numpy())
        env.append(env_a.cpu().numpy())
        obs_t, r, d = v.step_tensors(env_a)
        obs.append(obs_t.cpu().numpy())
        rew.append(r.cpu().numpy())
        done.append(d.cpu().numpy())
    torch.cuda.synchronize()
    out = dict(obs=np.stack(obs), act=np.stack(act), env=np.stack(env), rew=np.stack(rew), done=np.stack(done),
               ret=v.return_d.cpu().numpy(), state=v.save_state(), low=v.action_space.low, high=v.action_space.high)
    actor.close()
    v.close()
    return out


@pytest.mark.parametrize("N", [4, 10], ids=["n4_lean", "n10_wide"])
def test_closed_loop_ddpg_day(N):
    kw = station(N)
    day, eager = graph_day(kw), eager_day(kw)
    assert day["nodes"] == 2 * T
    for k in ("obs", "act", "rew", "done", "ret"):
        np.testing.assert_array_equal(day[k], eager[k], err_msg=f"N = {N}: {k} vs the eager loop")
    assert day["state"] == eager["state"]
    assert (day["rew"] != 0).any() and day["done"][-1].all() and not day["done"][:-1].any()
    assert (np.abs(day["act"]) <= 1).all()
    np.testing.assert_array_equal(eager["env"], unscale_f32(day["act"], eager["low"], eager["high"]))
    saturated = (np.abs(day["act"]) == 1).mean()
    print(f"N = {N}: {saturated:.3f} of the stored actions at +-1")
    assert 0.02 < saturated < 0.5
    # fused=True is accepted and gives the same nodes and bytes; so does a graph without the trajectory
    forced = graph_day(kw, fused=True)
    assert forced["nodes"] == 2 * T
    for k in ("obs", "act", "rew", "done", "ret"):
        np.testing.assert_array_equal(forced[k], day[k], err_msg=f"N = {N}: fused=True: {k}")
    assert forced["state"] == day["state"]
    last = graph_day(kw, trajectory=False)
    for got, k in zip(last["last"], ("obs", "act", "rew", "done")):
        np.testing.assert_array_equal(got, day[k][-1])
    assert last["state"] == day["state"]
    # the CPU oracle driven with the recorded env actions
    cfg = O.OracleConfig(**kw)
    envs = [O.OracleEnv(cfg, 0) for _ in range(E)]
    src = SmartNanogridVecEnv(E, seed=SEED, rng="device", **kw)
    src.reset_tensors()
    ivs, ratios = src.get_scenarios(0, E)
    src.close()
    ref0 = np.stack([load_exported_day(e, iv, r) for e, iv, r in zip(envs, ivs, ratios)])
    np.testing.assert_array_equal(day["obs"][0], ref0, err_msg=f"N = {N}: t = 0 observation vs oracle")
    ret = np.zeros(E)
    for t in range(T):
        outs = [e.step(eager["env"][t, i]) for i, e in enumerate(envs)]
        np.testing.assert_array_equal(day["obs"][t + 1], np.stack([x[0] for x in outs]), err_msg=f"N = {N} t {t}: obs")
        r = np.array([x[1] for x in outs])
        np.testing.assert_array_equal(day["rew"][t], r, err_msg=f"N = {N} t {t}: reward")
        ret = ret + r
    np.testing.assert_array_equal(day["ret"], ret, err_msg=f"N = {N}: day return vs oracle")


# ------------------------------------------------------------------------------- 4. weight refresh, two days
def test_new_weights_take_effect_without_a_recapture():
    kw = station(4)
    noise = torch.from_numpy(make_noise(5, 9)).to("cuda:0")
    runs = []
    for recapture in (False, True):
        v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **kw)
        actor = ddpg_actor(v, 11)
        g = ClosedLoopGraph(v, actor, noise=noise, trajectory=True)
        g.launch()
        first = g.action_traj.clone()
        actor.load(random_net_weights(v.obs_dim, v.act_dim, (400, 300), 12, OUT_SCALE))
        if recapture:
            g.close()
            g = ClosedLoopGraph(v, actor, noise=noise, trajectory=True)
        g.launch()
        torch.cuda.synchronize()
        runs.append((first.cpu().numpy(), g.action_traj.cpu().numpy(), g.obs_traj.cpu().numpy(),
                     g.reward_traj.cpu().numpy(), v.save_state()))
        g.close()
        actor.close()
        v.close()
    for a, b in zip(runs[0][:4], runs[1][:4]):
        np.testing.assert_array_equal(a, b)
    assert runs[0][4] == runs[1][4]
    assert not np.array_equal(runs[0][0], runs[0][1])


def test_two_days_in_one_graph_equal_two_launches():
    kw = station(4)
    noise = torch.from_numpy(make_noise(5, 9)).to("cuda:0")
    v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **kw)
    actor = ddpg_actor(v)
    rets = torch.zeros((2, E), dtype=torch.float64, device=v.device)
    g = ClosedLoopGraph(v, actor, noise=noise, days=2, day_returns=rets)
    assert g.step_nodes == 2 * T
    g.launch()
    torch.cuda.synchronize()
    w = SmartNanogridVecEnv(E, seed=SEED, rng="device", **kw)
    actor_w = ddpg_actor(w)
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


# ------------------------------------------------------------------------------------- 5. callable in the evaluators
def test_ddpg_actor_as_a_policy_of_evaluate_models():
    kw, episodes = station(4), 6
    days = generate_days(episodes, seed=SEED, rng="reference", **kw)
    v = SmartNanogridVecEnv(episodes, seed=SEED, rng="reference", **kw)
    actor = ddpg_actor(v)
    final, mean = evaluate_models({"ddpg": actor}, seed=SEED, rng="reference", days=days, **kw)
    v.reset_from_initial_values(list(days[0]), days[1], restore_requested_soc=True)
    rets = torch.zeros((1, episodes), dtype=torch.float64, device=v.device)
    g = ClosedLoopGraph(v, actor, with_reset=False, day_returns=rets)
    g.launch()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(final["ddpg"], rets[0].cpu().numpy())
    assert mean["ddpg"] == float(np.mean(rets[0].cpu().numpy())) and (final["ddpg"] != 0).all()
    # and the eager run of the same days, on a handle of its own (a second day of `v` would start from the
    # battery the first one left)
    w = SmartNanogridVecEnv(episodes, seed=SEED, rng="reference", **kw)
    actor_w = ddpg_actor(w)
    w.reset_from_initial_values(list(days[0]), days[1], restore_requested_soc=True)
    total = torch.zeros(episodes, dtype=torch.float64, device=w.device)
    obs_t = w.obs_d
    for t in range(T):
        obs_t, r, _ = w.step_tensors(actor_w(obs_t))
        total = total + r
    torch.cuda.synchronize()
    np.testing.assert_array_equal(final["ddpg"], total.cpu().numpy())
    for x in (g, actor, actor_w, v, w):
        x.close()


# ------------------------------------------------------------------------------------------------- 6. refusals
def test_create_net_refuses_what_the_contract_excludes():
    v = SmartNanogridVecEnv(4, seed=SEED, rng="device", **station(8))
    L = _native.lib()
    F = _native.c_float_p
    low = np.ascontiguousarray(v.action_space.low, np.float32)
    high = np.ascontiguousarray(v.action_space.high, np.float32)

    def create(bounds=True, **kw):
        f = dict(obs_dim=v.obs_dim, act_dim=v.act_dim, hidden1=400, hidden2=300, activation=1, output=1)
        f.update(kw)
        spec = _native.SngMlpNetSpec(f["obs_dim"], f["act_dim"], f["hidden1"], f["hidden2"], f["activation"], f["output"],
                                     low.ctypes.data_as(F) if bounds else None, high.ctypes.data_as(F) if bounds else None)
        h = ctypes.c_void_p()
        rc = L.sng_policy_create_net(v._h, ctypes.byref(spec), ctypes.byref(h))
        if rc == 0:
            L.sng_policy_destroy(h)
        return rc
    assert create() == 0 and create(hidden1=8, hidden2=512) == 0
    assert create(hidden1=7) == -2 and create(hidden2=513) == -2 and create(hidden1=513) == -2 and create(hidden2=7) == -2
    assert create(obs_dim=v.obs_dim + 1) == -1 and create(act_dim=v.act_dim - 1) == -1
    assert create(bounds=False) == -1 and create(bounds=False, output=0) == 0
    assert create(output=2) == -1 and create(activation=2) == -1
    h = ctypes.c_void_p()
    assert L.sng_policy_create(v._h, ctypes.byref(_native.SngMlpSpec(v.obs_dim, v.act_dim, 32, 0, None, None)),
                               ctypes.byref(h)) == -2
    with pytest.raises(_native.NativeError, match="8 .. 512"):
        MlpActor(v, "relu", net_arch=(600, 300))
    actor = MlpActor.ddpg(v)
    bad = random_net_weights(v.obs_dim, v.act_dim, (400, 300), 1)
    bad[2][5, 5] = np.nan
    with pytest.raises(_native.NativeError, match="non-finite"):
        actor.load(bad)
    with pytest.raises(ValueError, match="shapes"):
        actor.load(random_weights(v.obs_dim, v.act_dim, 1))   # 64-64 weights
    actor.close()
    v.close()


def test_a_station_above_64_actions_is_refused_not_half_computed():
    """64 chargers and a battery: act_dim 65, one more than the kernel's two output tiles.  sng_policy_create_net
    returns SNG_ERR_UNSUPPORTED (no policy exists whose columns from 64 on would stay unwritten); the 64-64 actor of
    sng_policy_create still works there and equals its host model in every column."""
    v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **station(64))
    assert v.act_dim == 65
    L = _native.lib()
    h = ctypes.c_void_p()
    for h1, h2 in ((400, 300), (64, 64)):
        spec = _native.SngMlpNetSpec(v.obs_dim, v.act_dim, h1, h2, 1, 0, None, None)
        assert L.sng_policy_create_net(v._h, ctypes.byref(spec), ctypes.byref(h)) == -2
        assert b"act_dim 65" in L.sng_last_error(v._h)
    with pytest.raises(_native.NativeError, match="act_dim 65"):
        MlpActor.ddpg(v)
    with pytest.raises(_native.NativeError, match="act_dim 65"):
        MlpActor(v, "relu", net=True)
    old = MlpActor(v, "relu").load(random_weights(v.obs_dim, v.act_dim, 11, OUT_SCALE))
    obs = v.reset_tensors()
    a, env_a = (x.cpu().numpy() for x in old.actions(obs))
    want_a, want_env = old.host_actions(obs)
    np.testing.assert_array_equal(a, want_a)
    np.testing.assert_array_equal(env_a, want_env)
    assert (a[:, 64] != 0).any()
    old.close()
    v.close()
