"""GPU: what finishes a PPO rollout (include/sng.h: sng_ppo_*; policy.py: PpoHead, PpoRollout).

With relu the value net is exactly reproducible on the CPU, and the advantages, returns and log-probabilities have no
transcendental in them at all, so everything here but the tanh values is bitwise against the host model
(sng_ppo_host_finish).  E = 70 (one full block of 64 rows and one of 6) is the unaligned form: obs_dim = 2 N + 9 is
odd at every station, so at E = 70 no observation block is a multiple of 16 B, every tile goes through the copy at
the commit point, and only at N = 1 is the noise block aligned.  E = 72 (a block of 64 and one of 8) is the aligned
form, the one a population of 65,536 takes: 16 B loads, and the tiles that fit the prefetch registers (observations
up to N = 59, noise up to N = 31) are staged in them a step ahead.  days = 2."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from policy_cases import actor_f64, random_weights  # noqa: E402
from smart_nanogrid_gym import ClosedLoopGraph, MlpActor, PpoHead, PpoRollout, SmartNanogridVecEnv, _native, policy  # noqa: E402
from test_gpu_policy import TANH_FACTOR  # noqa: E402

SEED, DAYS = 4321, 2
ENVS = (70, 72)   # unaligned blocks, and 16 B aligned blocks with a tail block of 8 rows
VALUE_SCALE = 30.0   # the value output's weights: values of the size of a day's return
BASE = dict(charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
            battery_system_available_in_model=True)


def make_env(N, interval="1h", E=70):
    return SmartNanogridVecEnv(E, seed=SEED, rng="device", number_of_chargers=N, time_interval=interval, **BASE)


def random_done(rng, T, E):
    """Terminal flags with both values at a day's last step and mid-day (tests/test_ppo_rollout_cpu.py)."""
    done = (rng.random((DAYS, T, E)) < 0.2).astype(np.uint8)
    assert set(np.unique(done[:, -1])) == {0, 1} and set(np.unique(done[:, :-1])) == {0, 1}
    assert 0.05 < done.mean() < 0.5
    return done


def synthetic(v, seed):
    """A trajectory of real observation rows (a reset and three stepped observations, tiled over [DAYS][T + 1] with a
    perturbation per block), random float64 rewards, random terminal flags and random noise."""
    rng = np.random.default_rng(seed)
    T, E = v.timesteps, v.num_envs
    recorded = [v.reset_tensors().cpu().numpy()]
    for _ in range(3):
        a = rng.uniform(v.action_space.low, v.action_space.high, (E, v.act_dim)).astype(np.float32)
        recorded.append(v.step_tensors(torch.from_numpy(a).to(v.device))[0].cpu().numpy())
    obs = np.stack([np.stack([recorded[(d + t) % 4] + np.float32(0.003 * (d * (T + 1) + t)) for t in range(T + 1)])
                    for d in range(DAYS)]).astype(np.float32)
    reward = -40.0 * rng.random((DAYS, T, E))
    log_std = rng.uniform(-2.0, 0.5, v.act_dim).astype(np.float32)
    noise = (rng.normal(0, 1, (T, E, v.act_dim)) * np.exp(log_std)).astype(np.float32)
    return obs, reward, random_done(rng, T, E), noise, log_std


def on(v, *arrays):
    return [None if a is None else torch.from_numpy(a).to(v.device) for a in arrays]


def host(x):
    return None if x is None else x.cpu().numpy()


# ------------------------------------------------------------------------------------- 1. finish, relu, synthetic
@pytest.mark.parametrize("E", ENVS)
@pytest.mark.parametrize("interval", ["1h", "2h"])
@pytest.mark.parametrize("N", [1, 4, 8, 10, 50, 128])
def test_finish_equals_the_host_model_relu(N, interval, E):
    """N = 128 with noise is the one-tile LDS fallback (two observation tiles, the hidden rows and the noise tile are
    185,344 B), without noise it has two tiles (152,320 B); N = 50 is above 64 KB of LDS.  At E = 72 the blocks are
    16 B aligned: up to N = 10 the observation and the noise tile are staged in the prefetch registers, at N = 50 the
    observation tile is (6,976 floats) and the noise tile (3,264) is copied with 16 B loads at its commit point, at
    N = 128 both are copied so.  At E = 70 every tile is copied float by float (the noise of N = 1 excepted)."""
    v = make_env(N, interval, E)
    assert (E * v.obs_dim) % 4 == (0 if E == 72 else 2)
    T = v.timesteps
    assert T == (24 if interval == "1h" else 12) and v.obs_dim == 2 * N + 9
    obs, reward, done, noise, log_std = synthetic(v, N)
    head = PpoHead(v, "relu").load(random_weights(v.obs_dim, 1, 17, VALUE_SCALE), log_std)
    obs_d, reward_d, done_d, noise_d = on(v, obs, reward, done, noise)
    for nz_d, nz in ((noise_d, noise), (None, None)):
        for gamma, lam in ((0.99, 0.95), (0.9, 0.8)):
            got = [host(x) for x in head.finish(obs_d, reward_d, done_d, nz_d, gamma, lam)]
            torch.cuda.synchronize()
            want = head.host_finish(obs, reward, done, nz, gamma, lam)
            for name, a, b in zip(("values", "advantages", "returns", "log_prob"), got, want):
                if nz is None and name == "log_prob":
                    assert a is None and b is None
                    continue
                assert a.shape == b.shape and a.dtype == b.dtype == np.float32
                np.testing.assert_array_equal(a, b, err_msg=f"N = {N} T = {T} E = {E} noise = {nz is not None}: {name}")
    values = got[0]
    assert np.unique(values).size > values.size // 2, "degenerate values"
    assert np.unique(got[1]).size > got[1].size // 2
    head.close()
    v.close()


# ------------------------------------------------------------------------------------------------------- 2. tanh
@pytest.mark.parametrize("N,E", [(8, 70), (10, 70), (8, 72)])
def test_finish_tanh(N, E):
    """The values against a float64 critic by test_tanh_day's rule: d_ref = max |host float32 model - float64|, d_dev
    the same for the device's values, and d_dev <= TANH_FACTOR d_ref (the same tanhf in the same chains).  Advantages
    and returns are bitwise the host model's on the device's own stored values, and the log-probabilities, which have
    no tanh in them, bitwise.  Measured on an MI355X (ROCm 7.2): N = 8: d_ref 4.0660e-06, d_dev 3.3615e-06 (ratio
    0.827), 0.221 of the values bitwise the host model's; N = 10: d_ref 2.3370e-06, d_dev 2.2678e-06 (ratio 0.970),
    0.069 bitwise.  E = 72: the aligned, staged form of the same kernel."""
    v = make_env(N, E=E)
    obs, reward, done, noise, log_std = synthetic(v, 100 + N)
    weights = random_weights(v.obs_dim, 1, 17, VALUE_SCALE)
    head = PpoHead(v, "tanh").load(weights, log_std)
    values, adv, ret, lp = (host(x) for x in head.finish(*on(v, obs, reward, done, noise)))
    torch.cuda.synchronize()
    h_values, _, _, h_lp = head.host_finish(obs, reward, done, noise)
    ref = actor_f64(obs.reshape(-1, v.obs_dim), weights, "tanh").reshape(values.shape)
    d_ref = np.abs(h_values.astype(np.float64) - ref).max()
    d_dev = np.abs(values.astype(np.float64) - ref).max()
    print(f"tanh N = {N} E = {E}: d_ref {d_ref:.4e}, d_dev {d_dev:.4e}, ratio {d_dev / d_ref:.3f}, factor {TANH_FACTOR}, "
          f"{np.mean(values == h_values):.3f} of the values bitwise equal to the host model")
    assert np.unique(values).size > values.size // 2
    assert d_dev <= TANH_FACTOR * d_ref
    _, g_adv, g_ret, _ = head.host_finish(obs, reward, done, noise, values=values)
    np.testing.assert_array_equal(adv, g_adv)
    np.testing.assert_array_equal(ret, g_ret)
    np.testing.assert_array_equal(lp, h_lp)
    head.close()
    v.close()


# --------------------------------------------------------------------------------------- 3. PpoRollout end to end
def sb3_state_dict(v, seed, out_scale=4.0):
    sd = dict(zip(policy.SB3_KEYS, random_weights(v.obs_dim, v.act_dim, seed, out_scale)))
    sd.update(zip(policy.SB3_VALUE_KEYS, random_weights(v.obs_dim, 1, seed + 1, VALUE_SCALE)))
    sd["log_std"] = np.linspace(-1.0, 0.25, v.act_dim).astype(np.float32)
    sd["optimizer.state"] = np.zeros(3, np.float32)   # ignored
    return sd


@pytest.mark.parametrize("N,E", [(4, 70), (10, 70), (8, 72), (10, 72)])
def test_rollout_end_to_end_relu(N, E):
    """N = 4 and N = 8 are lean plans, N = 10 the wide one; E = 72 has 16 B aligned blocks (the staged prefetch).  The trajectory is a plain ClosedLoopGraph's; the four new tensors
    are the host model's on it; a second launch with new value weights, and no recapture, gives the new values."""
    rng = np.random.default_rng(N)
    v = make_env(N, E=E)
    T, A = v.timesteps, v.act_dim
    sd = sb3_state_dict(v, 31)
    noise = (rng.normal(0, 1, (T, E, A)) * np.exp(sd["log_std"])).astype(np.float32)
    actor, head = MlpActor(v, "relu"), PpoHead(v, "relu")
    ro = PpoRollout(v, actor, head, days=DAYS, gamma=0.98, gae_lambda=0.9).load(sd)
    ro.noise.copy_(torch.from_numpy(noise))
    ro.launch()
    torch.cuda.synchronize()
    first = {k: host(getattr(ro, k)) for k in ("obs", "actions", "rewards", "dones", "episode_starts", "values",
                                                "advantages", "returns", "log_prob")}
    # the same days from a plain closed-loop graph of a fresh handle
    w = make_env(N, E=E)
    actor_w = MlpActor(w, "relu").load(sd)
    g = ClosedLoopGraph(w, actor_w, noise=torch.from_numpy(noise).to(w.device), days=DAYS, trajectory=True)
    g.launch()
    torch.cuda.synchronize()
    for name, t in (("obs", g.obs_traj), ("actions", g.action_traj), ("rewards", g.reward_traj), ("dones", g.done_traj)):
        np.testing.assert_array_equal(first[name], host(t), err_msg=f"N = {N}: {name}")
    assert first["obs"].shape == (DAYS, T + 1, E, v.obs_dim) and (first["rewards"] != 0).any()
    for x in (g, actor_w, w):
        x.close()
    starts = np.ones((DAYS, T, E), np.uint8)
    starts[:, 1:] = first["dones"][:, :-1]
    np.testing.assert_array_equal(first["episode_starts"], starts)
    assert first["dones"][:, -1].all() and not first["dones"][:, :-1].any() and starts[:, 0].all()

    def check(got, what):
        want = head.host_finish(got["obs"], got["rewards"], got["dones"], noise, 0.98, 0.9)
        for name, b in zip(("values", "advantages", "returns", "log_prob"), want):
            np.testing.assert_array_equal(got[name], b, err_msg=f"N = {N} {what}: {name}")
        assert np.unique(got["values"]).size > got["values"].size // 2
    check(first, "first launch")
    # new value weights between two launches: the second launch's values are theirs, without a recapture
    old = head.weights
    head.load(random_weights(v.obs_dim, 1, 77, VALUE_SCALE), sd["log_std"])
    ro.launch()
    torch.cuda.synchronize()
    second = {k: host(getattr(ro, k)) for k in ("obs", "rewards", "dones", "values", "advantages", "returns", "log_prob")}
    check(second, "second launch")
    stale = policy.ppo_host_finish(second["obs"], second["rewards"], second["dones"], old, sd["log_std"], noise, 0.98,
                                   0.9, "relu")[0]
    assert not np.array_equal(second["values"], stale)
    np.testing.assert_array_equal(second["log_prob"], first["log_prob"])   # the same noise and log_std
    ro.close()
    v.close()
    assert head._p is None and actor._p is None


def test_rollout_refuses_other_actors():
    v = make_env(4)
    head = PpoHead(v, "relu")
    with pytest.raises(ValueError, match="64-64"):
        PpoRollout(v, MlpActor.ddpg(v), head)
    with pytest.raises(ValueError, match="64-64"):
        PpoRollout(v, MlpActor(v, "relu", net_arch=(32, 32)), head)
    v.close()


# ------------------------------------------------------------------------------------------------ 4. closing order
def test_closing_order_and_device_refusals():
    v = make_env(4)
    T = v.timesteps
    head = PpoHead(v, "relu").load(random_weights(v.obs_dim, 1, 3))
    obs, reward, done, noise, _ = synthetic(v, 1)
    tensors = on(v, obs, reward, done, noise)
    head.finish(*tensors)
    with pytest.raises(_native.NativeError, match="gamma"):
        head.finish(*tensors, gamma=1.5)
    with pytest.raises(_native.NativeError, match="gae_lambda"):
        head.finish(*tensors, gae_lambda=float("nan"))
    with pytest.raises(ValueError, match="obs_traj"):
        head.finish(tensors[0][:, :T], *tensors[1:])
    # more days than one launch's grid has rows: refused with a reason before anything is launched or read
    L = _native.lib()
    ptrs = [x.data_ptr() for x in tensors] + [x.data_ptr() for x in head.finish(*tensors)]
    for days, rc in ((65536, -1), (2 ** 31 - 1, -1), (0, -1)):
        r = _native.SngPpoRollout(days, 0.99, 0.95, *ptrs)
        assert L.sng_ppo_finish(head._p, ctypes.byref(r), None) == rc and b"days" in L.sng_last_error(v._h), days
    r = _native.SngPpoRollout(DAYS, 0.99, 0.95, *ptrs)
    assert L.sng_ppo_finish(None, ctypes.byref(r), None) == -1 and b"null ppo handle" in L.sng_last_error(None)
    assert L.sng_ppo_set_weights(None, None, None, None) == -1 and b"null ppo handle" in L.sng_last_error(None)
    assert L.sng_ppo_finish(head._p, None, None) == -1 and b"null" in L.sng_last_error(v._h)
    bad = random_weights(v.obs_dim, 1, 3)
    bad[4][0, 5] = np.inf
    with pytest.raises(_native.NativeError, match="non-finite value net weight"):
        head.load(bad)
    with pytest.raises(_native.NativeError, match="non-finite log_std"):
        head.load(random_weights(v.obs_dim, 1, 3), np.full(v.act_dim, np.nan, np.float32))
    other = PpoHead(v, "tanh")
    other.close()
    with pytest.raises(RuntimeError, match="closed"):
        other.finish(*tensors)
    torch.cuda.synchronize()
    v.close()   # the env batch closes its heads
    assert head._p is None
    with pytest.raises(RuntimeError, match="closed"):
        head.finish(*tensors)
