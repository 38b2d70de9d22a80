"""GPU: the action noise source (include/sng.h: sng_noise_create; policy.py: ActionNoise) and the graphs and rollouts
that begin with its fill.

action_noise_kernel has no transcendental in it and compiles from the host model's own text, so a device fill is
compared with sng_noise_host_fill byte for byte.  A thread owns four consecutive floats of a step's row of E A, 1,024 a
workgroup: E = 1 and E = 63 / 64 with A = 2 are a single partial workgroup, A = 129 with E = 200 is 26 of them with a
partial last one; rows whose length is no multiple of four (A = 5, 11, 129 with odd E; E = 1, 63, 70 with odd A) take
the 4-byte stores, the others the 16-byte ones."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from policy_cases import random_weights  # noqa: E402
from policy_net_cases import net_f64, random_net_weights, unscale_f32  # noqa: E402
from smart_nanogrid_gym import (ActionNoise, ClosedLoopGraph, MlpActor, PpoHead, PpoRollout, SmartNanogridVecEnv,  # noqa: E402
                                _native, policy)
from test_gpu_policy_net import SQUASH_FACTOR  # noqa: E402

SEED, DAYS = 4321, 2
OUT_SCALE, VALUE_SCALE = 4.0, 30.0
BASE = dict(charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
            battery_system_available_in_model=True)
BIG_OFFSET = 2 ** 33 + 5


def make_env(N, E, interval="1h", env_offset=0):
    return SmartNanogridVecEnv(E, seed=SEED, rng="device", number_of_chargers=N, time_interval=interval,
                               env_offset=env_offset, **BASE)


def host(x):
    return x.cpu().numpy()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------ 1. fill == host_fill
@pytest.mark.parametrize("E", [1, 63, 64, 70, 200])
@pytest.mark.parametrize("N", [1, 4, 10, 128], ids=lambda n: f"A{n + 1}")
def test_fill_equals_the_host_model_bitwise(N, E):
    for interval, T, offset, c0 in (("1h", 24, 0, 0), ("2h", 12, BIG_OFFSET, 2 ** 32 - 1)):
        v = make_env(N, E, interval, offset)
        A = v.act_dim
        assert A == N + 1 and v.timesteps == T
        mu = np.linspace(-0.5, 0.75, A).astype(np.float32)
        scale = np.linspace(0.1, 1.3, A).astype(np.float32)
        for kind in ("gaussian", "ou"):
            what = f"{kind} A = {A} E = {E} T = {T} offset {offset}"
            src = ActionNoise(v, kind, seed=2 ** 40 + 77, mu=mu, scale=scale, theta=0.3, dt=0.05)
            assert src.counter == 0
            src.counter = c0
            assert src.counter == c0
            first = host(src.fill(DAYS))
            assert first.shape == (DAYS, T, E, A)
            want = policy.noise_host_fill(kind, A, T, E, DAYS, 2 ** 40 + 77, mu, scale, 0.3, 0.05, offset, c0)
            assert same(first, want), what
            assert same(src.host_fill(DAYS, counter=c0), want)
            assert src.counter == c0 + DAYS
            # the second fill continues the counter; new parameters change it without a new object
            second = host(src.fill(DAYS))
            assert same(second, src.host_fill(DAYS, counter=c0 + DAYS)), what
            assert not np.array_equal(second, first)
            src.set(mu[::-1].copy(), 2 * scale)
            third = host(src.fill(DAYS))
            assert src.counter == c0 + 3 * DAYS
            assert same(third, policy.noise_host_fill(kind, A, T, E, DAYS, 2 ** 40 + 77, mu[::-1].copy(), 2 * scale, 0.3,
                                                      0.05, offset, c0 + 2 * DAYS)), what
            # one block of another size from the same source, and a caller's own tensor
            out = torch.empty((1, T, E, A), dtype=torch.float32, device=v.device)
            assert src.fill(1, out=out) is out
            assert same(host(out), src.host_fill(1, counter=c0 + 3 * DAYS))
            assert np.isfinite(third).all() and np.abs(first).max() > 0
            src.close()
        v.close()


def test_refusals_on_the_device():
    v = make_env(4, 8)
    L = _native.lib()
    import ctypes
    h = ctypes.c_void_p()
    for a in (4, 6, 0, 256):
        spec = _native.SngNoiseSpec(0, a, 0, 0.15, 1e-2)
        assert L.sng_noise_create(v._h, ctypes.byref(spec), ctypes.byref(h)) == -1 and not h.value
        assert str(a).encode() in L.sng_last_error(v._h)
    assert L.sng_noise_create(v._h, None, ctypes.byref(h)) == -1
    with pytest.raises(_native.NativeError, match="libsng error -1.*theta"):
        ActionNoise(v, "ou", theta=float("nan"))
    with pytest.raises(_native.NativeError, match=r"libsng error -1.*scale\[0\]"):
        ActionNoise(v, "gaussian", scale=-1.0)
    src = ActionNoise(v, "gaussian", scale=0.5)
    with pytest.raises(_native.NativeError, match=r"libsng error -1.*mu\[2\]"):
        src.set([0, 0, np.inf, 0, 0], 1.0)
    with pytest.raises(_native.NativeError, match="libsng error -1.*days = 0"):
        src.fill(0)
    assert L.sng_noise_fill(src._p, None, 1, None) == -1 and b"null" in L.sng_last_error(v._h)
    assert L.sng_noise_set_params(src._p, None, None, None) == -1 and b"null" in L.sng_last_error(v._h)
    assert src.counter == 0   # nothing was drawn
    other = make_env(4, 8)
    with pytest.raises(ValueError, match="another env batch"):
        ClosedLoopGraph(other, MlpActor(other, "relu"), noise=src)
    with pytest.raises(ValueError, match="gaussian ActionNoise"):
        PpoRollout(v, MlpActor(v, "relu"), PpoHead(v, "relu"), noise=ActionNoise(v, "ou"))
    src.close()
    with pytest.raises(RuntimeError, match="closed"):
        src.fill(1)
    with pytest.raises(ValueError, match="closed"):
        ClosedLoopGraph(v, MlpActor(v, "relu"), noise=src)
    other.close()
    v.close()


# ------------------------------------------------------------------------------ 2. closed-loop graphs with a source
GRAPHS = [(4, (64, 64), False), (10, (64, 64), False), (4, (33, 65), False), (4, (64, 64), True)]


@pytest.mark.parametrize("N,net,fused", GRAPHS, ids=["lean4", "wide10", "lean4-33x65", "lean4-fused"])
def test_closed_loop_graph_draws_its_own_noise(N, net, fused):
    E, c0 = 70, 7
    v = make_env(N, E)
    T, A = v.timesteps, v.act_dim
    weights = random_net_weights(v.obs_dim, A, net, 11, OUT_SCALE)
    actor = MlpActor(v, "relu", net_arch=net).load(weights)
    src = ActionNoise(v, "gaussian", seed=5, mu=0.0, scale=np.linspace(0.2, 0.9, A).astype(np.float32))
    src.counter = c0
    g = ClosedLoopGraph(v, actor, noise=src, days=DAYS, trajectory=True, fused=fused)
    assert g.step_nodes == (1 if fused else 2 * T) and g.noise is None
    assert tuple(g.noise_traj.shape) == (DAYS, T, E, A)
    runs = []
    for launch in range(2):
        g.launch()
        torch.cuda.synchronize()
        nz, obs, act = host(g.noise_traj), host(g.obs_traj), host(g.action_traj)
        assert same(nz, src.host_fill(DAYS, counter=c0 + DAYS * launch)), f"launch {launch}: noise_traj"
        assert not np.array_equal(nz[0], nz[1])
        for d in range(DAYS):
            for t in range(T):
                want = actor.host_actions(obs[d, t], nz[d, t])[0]
                assert same(act[d, t], want), f"launch {launch} day {d} step {t}"
        runs.append((nz, obs, act, host(g.reward_traj)))
    assert src.counter == c0 + 2 * DAYS
    assert not np.array_equal(runs[0][0], runs[1][0]) and (runs[0][3] != 0).any()
    # the tensor path, on a fresh handle (the same device days), given day 0's block: day 0's actions, bitwise
    w = make_env(N, E)
    actor_w = MlpActor(w, "relu", net_arch=net).load(weights)
    plain = ClosedLoopGraph(w, actor_w, noise=torch.from_numpy(runs[0][0][0]).to(w.device), days=1, trajectory=True,
                            fused=fused)
    assert plain.noise_traj is None and plain.noise_source is None
    plain.launch()
    torch.cuda.synchronize()
    assert same(host(plain.action_traj)[0], runs[0][2][0]) and same(host(plain.obs_traj)[0], runs[0][1][0])
    for x in (plain, actor_w, w, g, src, actor, v):
        x.close()


# ----------------------------------------------------------------------------------------- 3. DDPG with an OU source
def test_ddpg_actor_with_an_ou_source():
    """SB3's DDPG("MlpPolicy", env, action_noise=OrnsteinUhlenbeckActionNoise(0, 0.5)) in the loop, N = 4, E = 70.  The
    stored a is the host's clip of tanh(mean) + noise up to the device's tanhf: d_dev <= SQUASH_FACTOR d_ref against
    float64, test_gpu_policy_net's rule; the env actions are the host's unscale of the stored a, bitwise."""
    N, E = 4, 70
    v = make_env(N, E)
    T, A = v.timesteps, v.act_dim
    weights = random_net_weights(v.obs_dim, A, policy.DDPG_NET_ARCH, 11, OUT_SCALE)
    actor = MlpActor.ddpg(v).load(weights)
    src = ActionNoise(v, "ou", seed=9, mu=0.0, scale=0.5)
    g = ClosedLoopGraph(v, actor, noise=src, days=DAYS, trajectory=True)
    g.launch()
    torch.cuda.synchronize()
    nz, obs, act = host(g.noise_traj), host(g.obs_traj), host(g.action_traj)
    assert same(nz, src.host_fill(DAYS, counter=0)) and src.counter == DAYS
    # an OU path: every day starts from 0, so its first step is sd z, far smaller than its later steps' spread
    assert np.abs(nz[:, 0]).max() < 0.5 and nz[:, -1].std() > 2 * nz[:, 0].std()
    low, high = v.action_space.low, v.action_space.high
    d_ref = d_dev = 0.0
    for d in range(DAYS):
        for t in range(T):
            host_a = actor.host_actions(obs[d, t], nz[d, t])[0]
            ref = net_f64(obs[d, t], weights, "relu", nz[d, t], squash=True)
            d_ref = max(d_ref, np.abs(host_a.astype(np.float64) - ref).max())
            d_dev = max(d_dev, np.abs(act[d, t].astype(np.float64) - ref).max())
            # the same kernel on the same rows, eagerly: the stored a again, and what the env was stepped with
            a, env_a = (host(x) for x in actor.actions(g.obs_traj[d, t], g.noise_traj[d, t]))
            assert same(a, act[d, t]) and same(env_a, unscale_f32(act[d, t], low, high)), (d, t)
    print(f"ddpg + OU N = {N}: d_ref {d_ref:.4e}, d_dev {d_dev:.4e}, ratio {d_dev / d_ref:.3f}, factor {SQUASH_FACTOR}")
    assert (np.abs(act) <= 1).all() and d_dev <= SQUASH_FACTOR * d_ref
    for x in (g, src, actor, v):
        x.close()


# ------------------------------------------------------------------------------------- 4. PpoRollout with a source
NAMES = ("values", "advantages", "returns", "log_prob")


def sb3_state_dict(v, actor_arch, value_arch, seed):
    sd = dict(zip(policy.SB3_KEYS, random_net_weights(v.obs_dim, v.act_dim, actor_arch, seed, OUT_SCALE)))
    sd.update(zip(policy.SB3_VALUE_KEYS, random_net_weights(v.obs_dim, 1, value_arch, seed + 1, VALUE_SCALE)))
    sd["log_std"] = np.linspace(-1.0, 0.25, v.act_dim).astype(np.float32)
    return sd


@pytest.mark.parametrize("N,E,arch,net_head", [(8, 72, (64, 64), False), (4, 70, (33, 65), True)],
                         ids=["default-head-n8", "net-head-33x65-n4"])
def test_ppo_rollout_with_a_source(N, E, arch, net_head):
    v = make_env(N, E)
    T, A = v.timesteps, v.act_dim
    sd = sb3_state_dict(v, arch, arch, 31)
    actor, head = MlpActor(v, "relu", net_arch=arch), PpoHead(v, "relu", net_arch=arch if net_head else None)
    src = ActionNoise(v, "gaussian", seed=12)
    ro = PpoRollout(v, actor, head, days=DAYS, gamma=0.98, gae_lambda=0.9, noise=src).load(sd)
    assert tuple(ro.noise.shape) == (DAYS, T, E, A)
    scale = np.exp(sd["log_std"]).astype(np.float32)
    assert same(src.scale, scale)
    for launch in range(2):
        ro.launch()
        torch.cuda.synchronize()
        got = {k: host(getattr(ro, k)) for k in ("obs", "actions", "rewards", "dones", "noise") + NAMES}
        assert same(got["noise"], policy.noise_host_fill("gaussian", A, T, E, DAYS, 12, 0.0, scale, counter=DAYS * launch))
        assert got["values"].shape == (DAYS, T + 1, E) and got["log_prob"].shape == (DAYS, T, E)
        for d in range(DAYS):
            want = head.host_finish(got["obs"][d:d + 1], got["rewards"][d:d + 1], got["dones"][d:d + 1], got["noise"][d],
                                    0.98, 0.9)
            for name, b in zip(NAMES, want):
                np.testing.assert_array_equal(got[name][d:d + 1], b, err_msg=f"launch {launch} day {d}: {name}")
            for t in (0, T - 1):
                assert same(got["actions"][d, t], actor.host_actions(got["obs"][d, t], got["noise"][d, t])[0])
        assert not np.array_equal(got["log_prob"][0], got["log_prob"][1])   # each day's own noise
        assert np.unique(got["values"]).size > got["values"].size // 2
    assert src.counter == 2 * DAYS
    ro.close()
    # noise=None: the object as it was -- the caller's one block, one finish, every day the same log-probabilities
    w = make_env(N, E)
    actor_w, head_w = MlpActor(w, "relu", net_arch=arch), PpoHead(w, "relu", net_arch=arch if net_head else None)
    old = PpoRollout(w, actor_w, head_w, days=DAYS, gamma=0.98, gae_lambda=0.9).load(sd)
    assert old.noise_source is None and tuple(old.noise.shape) == (T, E, A)
    old.noise.copy_(torch.from_numpy(got["noise"][0]))
    old.launch()
    torch.cuda.synchronize()
    assert tuple(old.log_prob.shape) == (DAYS, T, E) and tuple(old.values.shape) == (DAYS, T + 1, E)
    lp = host(old.log_prob)
    assert same(lp[0], lp[1])
    want = head_w.host_finish(host(old.obs), host(old.rewards), host(old.dones), got["noise"][0], 0.98, 0.9)
    for name, b in zip(NAMES, want):
        np.testing.assert_array_equal(host(getattr(old, name)), b, err_msg=f"noise=None: {name}")
    for x in (old, w, v):
        x.close()
    assert src._p is None and head._p is None
