"""GPU: a PPO rollout's finish for a value net of any two hidden widths (include/sng.h: sng_ppo_create_net; policy.py:
PpoHead(net_arch=...), PpoRollout).

value_net_kernel runs the critic over the trajectory's days (T + 1) E observation rows as one flat batch, 64 rows a
workgroup, so what matters of a shape is its row count: E = 70 with T = 24 and two days is 3,500 rows (54 full blocks
and one of 44), E = 72 is 3,600 (a last block of 16), E = 64 has no partial block, and E = 1 with one day of T = 12 is
13 rows, a single partial block; row blocks straddle steps and days throughout.  With relu the value net is exactly
reproducible on the CPU, and the advantages, returns and log-probabilities have no transcendental in them, so
everything here but the tanh values is compared by value (==) with the host model (sng_ppo_net_host_finish), and given
the device's stored values the advantages and returns are bitwise the host's."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from policy_cases import random_weights  # noqa: E402
from policy_net_cases import net_f64, random_net_weights  # noqa: E402
from smart_nanogrid_gym import ClosedLoopGraph, MlpActor, PpoHead, PpoRollout, SmartNanogridVecEnv, _native, policy  # noqa: E402
from test_gpu_policy import TANH_FACTOR  # noqa: E402

SEED, DAYS = 4321, 2
VALUE_SCALE = 30.0   # the value output's weights: values of the size of a day's return
NETS = [(8, 8), (33, 65), (64, 64), (400, 300), (512, 512)]
PAIRS = ((0.99, 0.95), (0.9, 0.8))   # (gamma, gae_lambda)
NAMES = ("values", "advantages", "returns", "log_prob")
BASE = dict(charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
            battery_system_available_in_model=True)


def make_env(N, interval="1h", E=70):
    return SmartNanogridVecEnv(E, seed=SEED, rng="device", number_of_chargers=N, time_interval=interval, **BASE)


def random_done(rng, days, T, E):
    """Terminal flags with both values at a day's last step and mid-day, where there are envs enough for both."""
    done = (rng.random((days, T, E)) < 0.2).astype(np.uint8)
    if days * E >= 16:
        assert set(np.unique(done[:, -1])) == {0, 1} and set(np.unique(done[:, :-1])) == {0, 1}
        assert 0.05 < done.mean() < 0.5
    return done


def synthetic(v, seed, days=DAYS):
    """A trajectory of real observation rows (a reset and three stepped observations, tiled over [days][T + 1] with a
    perturbation per block), random float64 rewards, random terminal flags and random noise, of which some entries
    are +-100 (far outside any standard deviation here: the log-probability must stay finite)."""
    rng = np.random.default_rng(seed)
    T, E = v.timesteps, v.num_envs
    recorded = [v.reset_tensors().cpu().numpy()]
    for _ in range(3):
        a = rng.uniform(v.action_space.low, v.action_space.high, (E, v.act_dim)).astype(np.float32)
        recorded.append(v.step_tensors(torch.from_numpy(a).to(v.device))[0].cpu().numpy())
    obs = np.stack([np.stack([recorded[(d + t) % 4] + np.float32(0.003 * (d * (T + 1) + t)) for t in range(T + 1)])
                    for d in range(days)]).astype(np.float32)
    reward = -40.0 * rng.random((days, T, E))
    log_std = rng.uniform(-2.0, 0.5, v.act_dim).astype(np.float32)
    noise = (rng.normal(0, 1, (T, E, v.act_dim)) * np.exp(log_std)).astype(np.float32)
    noise[1, 0, 0], noise[T - 1, E - 1, v.act_dim - 1], noise[2, E // 2, :] = 100.0, -100.0, 100.0
    return obs, reward, random_done(rng, days, T, E), noise, log_std


def on(v, *arrays):
    return [None if a is None else torch.from_numpy(a).to(v.device) for a in arrays]


def host(x):
    return None if x is None else x.cpu().numpy()


@pytest.fixture(scope="module")
def stations():
    """One env batch and one synthetic trajectory per (N, interval, E, days), shared by the nets; never changed."""
    made = {}

    def get(N, interval="1h", E=70, days=DAYS):
        key = (N, interval, E, days)
        if key not in made:
            v = make_env(N, interval, E)
            arrays = synthetic(v, 1000 * N + E, days)
            tensors = on(v, *arrays[:4])
            for a in arrays:
                a.setflags(write=False)
            made[key] = (v, arrays, tensors)
        return made[key]
    yield get
    for v, _, _ in made.values():
        v.close()


def check_relu(v, arrays, tensors, net_arch, what):
    """finish against the host model for both (gamma, lambda) pairs, with and without noise.  The host's values are
    computed once; its other runs read them (values_given), which is the same arithmetic on the same values."""
    obs, reward, done, noise, log_std = arrays
    obs_d, reward_d, done_d, noise_d = tensors
    days, T, E = reward.shape
    head = PpoHead(v, "relu", net_arch=net_arch).load(random_net_weights(v.obs_dim, 1, net_arch, 17, VALUE_SCALE), log_std)
    want_values = None
    for nz_d, nz in ((noise_d, noise), (None, None)):
        for gamma, lam in PAIRS:
            got = [host(x) for x in head.finish(obs_d, reward_d, done_d, nz_d, gamma, lam)]
            torch.cuda.synchronize()
            if want_values is None:
                want = head.host_finish(obs, reward, done, nz, gamma, lam)
                want_values = want[0]
            else:
                want = head.host_finish(obs, reward, done, nz, gamma, lam, values=want_values)
            for name, a, b in zip(NAMES, got, want):
                if nz is None and name == "log_prob":
                    assert a is None and b is None
                    continue
                assert a.shape == b.shape and a.dtype == b.dtype == np.float32
                np.testing.assert_array_equal(a, b, err_msg=f"{what} noise = {nz is not None} {gamma}/{lam}: {name}")
            # given the device's own stored values, advantages and returns are the host's bit for bit
            _, g_adv, g_ret, g_lp = head.host_finish(obs, reward, done, nz, gamma, lam, values=got[0])
            assert got[1].tobytes() == g_adv.tobytes() and got[2].tobytes() == g_ret.tobytes(), what
            if nz is not None:
                assert got[3].tobytes() == g_lp.tobytes() and np.isfinite(got[3]).all(), what
                assert (got[3][:, 2, E // 2] < -1000.0).all()   # a row of +100 noise entries
    values = got[0]
    assert values.shape == (days, T + 1, E)
    if values.size >= 64:
        assert np.unique(values).size > values.size // 2, "degenerate values"
        assert np.unique(got[1]).size > got[1].size // 2
    head.close()


# ------------------------------------------------------------------------------------- 1. finish, relu, synthetic
@pytest.mark.parametrize("E", [70, 72])
@pytest.mark.parametrize("N", [1, 4, 10])
@pytest.mark.parametrize("net_arch", NETS, ids=lambda a: f"{a[0]}-{a[1]}")
def test_finish_equals_the_host_model_relu(stations, net_arch, N, E):
    """T = 24: 3,500 rows at E = 70 (54 full blocks and one of 44), 3,600 at E = 72 (a last block of 16)."""
    v, arrays, tensors = stations(N, "1h", E)
    assert v.timesteps == 24 and DAYS * 25 * E == (3500 if E == 70 else 3600)
    check_relu(v, arrays, tensors, net_arch, f"{net_arch} N = {N} E = {E}")


@pytest.mark.parametrize("net_arch,N,interval,E,days", [
    ((33, 65), 4, "2h", 70, DAYS),       # T = 12
    ((400, 300), 50, "1h", 70, DAYS),    # obs_dim 109: 135,680 B of LDS
    ((64, 64), 128, "1h", 70, DAYS),     # obs_dim 265, act_dim 129: the widest log-probability row
    ((33, 65), 4, "2h", 1, 1),           # 13 rows: a single partial block
    ((400, 300), 4, "1h", 64, DAYS),     # 3,200 rows: no partial block
], ids=["T12", "N50", "N128", "E1", "E64"])
def test_finish_further_shapes_relu(stations, net_arch, N, interval, E, days):
    v, arrays, tensors = stations(N, interval, E, days)
    assert v.obs_dim == 2 * N + 9 and v.act_dim == N + 1
    check_relu(v, arrays, tensors, net_arch, f"{net_arch} N = {N} {interval} E = {E} days = {days}")


# ------------------------------------------------------------------------- 2. the (64, 64) net head and the default
def test_a_64_64_net_head_equals_the_default_head(stations):
    v, arrays, tensors = stations(8, "1h", 72)
    obs, reward, done, noise, log_std = arrays
    weights = random_weights(v.obs_dim, 1, 17, VALUE_SCALE)
    default, net = PpoHead(v, "relu").load(weights, log_std), PpoHead(v, "relu", net_arch=(64, 64)).load(weights, log_std)
    assert default.net_arch is None and net.net_arch == (64, 64)
    for gamma, lam in PAIRS:
        a = [host(x) for x in default.finish(*tensors, gamma, lam)]
        b = [host(x) for x in net.finish(*tensors, gamma, lam)]
        torch.cuda.synchronize()
        for name, x, y in zip(NAMES, a, b):
            np.testing.assert_array_equal(x, y, err_msg=name)
    assert np.unique(a[0]).size > a[0].size // 2
    default.close()
    net.close()


# ------------------------------------------------------------------------------------------------------- 3. tanh
@pytest.mark.parametrize("net_arch", [(64, 64), (400, 300)], ids=lambda a: f"{a[0]}-{a[1]}")
def test_finish_tanh(stations, net_arch):
    """The values against a float64 critic by test_tanh_day's rule: d_ref = max |host float32 model - float64|, d_dev
    the same for the device's values, and d_dev <= TANH_FACTOR d_ref (the same tanhf in the same chains).  Advantages
    and returns are bitwise the host model's on the device's own stored values, and the log-probabilities, which have
    no tanh in them, bitwise.  N = 8, E = 72.  Measured on an MI355X (ROCm 7.2): (64, 64): d_ref 4.3236e-06, d_dev
    3.0095e-06 (ratio 0.696), 0.214 of the values bitwise the host model's; (400, 300): d_ref 8.6253e-06, d_dev
    9.7058e-06 (ratio 1.125), 0.155 bitwise."""
    v, arrays, tensors = stations(8, "1h", 72)
    obs, reward, done, noise, log_std = arrays
    weights = random_net_weights(v.obs_dim, 1, net_arch, 17, VALUE_SCALE)
    head = PpoHead(v, "tanh", net_arch=net_arch).load(weights, log_std)
    values, adv, ret, lp = (host(x) for x in head.finish(*tensors))
    torch.cuda.synchronize()
    h_values, _, _, h_lp = head.host_finish(obs, reward, done, noise)
    ref = net_f64(obs.reshape(-1, v.obs_dim), weights, "tanh").reshape(values.shape)
    d_ref = np.abs(h_values.astype(np.float64) - ref).max()
    d_dev = np.abs(values.astype(np.float64) - ref).max()
    print(f"tanh {net_arch} N = 8 E = 72: d_ref {d_ref:.4e}, d_dev {d_dev:.4e}, ratio {d_dev / d_ref:.3f}, factor "
          f"{TANH_FACTOR}, {np.mean(values == h_values):.3f} of the values bitwise equal to the host model")
    assert np.unique(values).size > values.size // 2
    assert d_dev <= TANH_FACTOR * d_ref
    _, g_adv, g_ret, _ = head.host_finish(obs, reward, done, noise, values=values)
    assert adv.tobytes() == g_adv.tobytes() and ret.tobytes() == g_ret.tobytes()
    assert lp.tobytes() == h_lp.tobytes()
    head.close()


# --------------------------------------------------------------------------------------- 4. PpoRollout end to end
def sb3_state_dict(v, actor_arch, value_arch, seed, out_scale=4.0):
    sd = dict(zip(policy.SB3_KEYS, random_net_weights(v.obs_dim, v.act_dim, actor_arch, seed, out_scale)))
    sd.update(zip(policy.SB3_VALUE_KEYS, random_net_weights(v.obs_dim, 1, value_arch, seed + 1, VALUE_SCALE)))
    sd["log_std"] = np.linspace(-1.0, 0.25, v.act_dim).astype(np.float32)
    sd["optimizer.state"] = np.zeros(3, np.float32)   # ignored
    return sd


@pytest.mark.parametrize("N,E,actor_arch,value_arch", [(4, 70, (33, 65), (33, 65)), (10, 72, (64, 64), (400, 300))],
                         ids=["lean4-33-65", "wide10-policy_kernel-400-300"])
def test_rollout_end_to_end_relu(N, E, actor_arch, value_arch):
    """N = 4 is a lean plan, N = 10 the wide one; the second pair is SB3's net_arch=dict(pi=[64, 64], vf=[400, 300])
    with the actor on policy_kernel.  The trajectory is a plain ClosedLoopGraph's; the four new tensors are the host
    model's on it; a second launch with new value weights, and no recapture, gives the new values."""
    rng = np.random.default_rng(N)
    v = make_env(N, E=E)
    T, A = v.timesteps, v.act_dim
    sd = sb3_state_dict(v, actor_arch, value_arch, 31)
    noise = (rng.normal(0, 1, (T, E, A)) * np.exp(sd["log_std"])).astype(np.float32)
    actor, head = MlpActor(v, "relu", net_arch=actor_arch), PpoHead(v, "relu", net_arch=value_arch)
    assert actor.net == (actor_arch != (64, 64))
    ro = PpoRollout(v, actor, head, days=DAYS, gamma=0.98, gae_lambda=0.9).load(sd)
    ro.noise.copy_(torch.from_numpy(noise))
    ro.launch()
    torch.cuda.synchronize()
    first = {k: host(getattr(ro, k)) for k in ("obs", "actions", "rewards", "dones", "episode_starts", "values",
                                                "advantages", "returns", "log_prob")}
    # the same days from a plain closed-loop graph of a fresh handle
    w = make_env(N, E=E)
    actor_w = MlpActor(w, "relu", net_arch=actor_arch).load(sd)
    g = ClosedLoopGraph(w, actor_w, noise=torch.from_numpy(noise).to(w.device), days=DAYS, trajectory=True)
    g.launch()
    torch.cuda.synchronize()
    for name, t in (("obs", g.obs_traj), ("actions", g.action_traj), ("rewards", g.reward_traj), ("dones", g.done_traj)):
        assert first[name].tobytes() == host(t).tobytes(), f"N = {N}: {name}"
    assert first["obs"].shape == (DAYS, T + 1, E, v.obs_dim) and (first["rewards"] != 0).any()
    for x in (g, actor_w, w):
        x.close()
    starts = np.ones((DAYS, T, E), np.uint8)
    starts[:, 1:] = first["dones"][:, :-1]
    np.testing.assert_array_equal(first["episode_starts"], starts)
    assert first["dones"][:, -1].all() and not first["dones"][:, :-1].any() and starts[:, 0].all()

    def check(got, what):
        want = head.host_finish(got["obs"], got["rewards"], got["dones"], noise, 0.98, 0.9)
        for name, b in zip(NAMES, want):
            np.testing.assert_array_equal(got[name], b, err_msg=f"N = {N} {what}: {name}")
        assert np.unique(got["values"]).size > got["values"].size // 2
    check(first, "first launch")
    # new value weights between two launches: the second launch's values are theirs, without a recapture
    old = head.weights
    head.load(random_net_weights(v.obs_dim, 1, value_arch, 77, VALUE_SCALE), sd["log_std"])
    ro.launch()
    torch.cuda.synchronize()
    second = {k: host(getattr(ro, k)) for k in ("obs", "rewards", "dones", "values", "advantages", "returns", "log_prob")}
    check(second, "second launch")
    stale = policy.ppo_host_finish(second["obs"], second["rewards"], second["dones"], old, sd["log_std"], noise, 0.98,
                                   0.9, "relu", net_arch=value_arch)[0]
    assert not np.array_equal(second["values"], stale)
    np.testing.assert_array_equal(second["log_prob"], first["log_prob"])   # the same noise and log_std
    ro.close()
    v.close()
    assert head._p is None and actor._p is None


# ------------------------------------------------------------------------------------------ 5. pairing and refusals
def test_pairing_and_refusals(stations):
    v, arrays, tensors = stations(4, "1h", 70)
    default, net = PpoHead(v, "relu"), PpoHead(v, "relu", net_arch=(33, 65))
    small, ddpg = MlpActor(v, "relu", net_arch=(32, 32)), MlpActor.ddpg(v)
    with pytest.raises(ValueError, match="64-64"):
        PpoRollout(v, small, default)
    with pytest.raises(ValueError, match="64-64"):
        PpoRollout(v, ddpg, default)
    with pytest.raises(ValueError, match="squashed"):
        PpoRollout(v, ddpg, net)
    other = make_env(4, E=8)
    with pytest.raises(ValueError, match="another env batch"):
        PpoRollout(other, MlpActor(other, "relu"), net)
    # unsupported widths and tiles: libsng error -2, with the sizes
    for arch in ((7, 64), (64, 513)):
        with pytest.raises(_native.NativeError, match="libsng error -2.*8 .. 512"):
            PpoHead(v, "relu", net_arch=arch)
    wide = make_env(56, E=8)
    with pytest.raises(_native.NativeError, match="libsng error -2.*obs_dim 121.*512-512 need 164352 B of 163840"):
        PpoHead(wide, "relu", net_arch=(512, 512))
    with pytest.raises(ValueError, match="two hidden widths"):
        PpoHead(v, "relu", net_arch=(64,))
    # the calls of a net head refuse what the default head's refuse
    net.load(random_net_weights(v.obs_dim, 1, (33, 65), 3))
    net.finish(*tensors)
    with pytest.raises(_native.NativeError, match="gamma"):
        net.finish(*tensors, gamma=1.5)
    with pytest.raises(_native.NativeError, match="gae_lambda"):
        net.finish(*tensors, gae_lambda=float("nan"))
    with pytest.raises(ValueError, match="obs_traj"):
        net.finish(tensors[0][:, :v.timesteps], *tensors[1:])
    with pytest.raises(ValueError, match="shapes"):
        net.load(random_weights(v.obs_dim, 1, 3))           # a 64-64 value net
    L = _native.lib()
    outs = net.finish(*tensors)
    ptrs = [x.data_ptr() for x in tensors] + [x.data_ptr() for x in outs]
    T = v.timesteps
    # the days, and with the log-probability stage the T steps, are rows of one launch's grid; nothing is launched
    for days, rc in ((65536 - T, -1), (65536, -1), (2 ** 31 - 1, -1), (0, -1)):
        r = _native.SngPpoRollout(days, 0.99, 0.95, *ptrs)
        assert L.sng_ppo_finish(net._p, ctypes.byref(r), None) == rc and b"days" in L.sng_last_error(v._h), days
    assert L.sng_ppo_finish(net._p, None, None) == -1 and b"null" in L.sng_last_error(v._h)
    bad = random_net_weights(v.obs_dim, 1, (33, 65), 3)
    bad[4][0, 5] = np.inf
    with pytest.raises(_native.NativeError, match="non-finite value net weight"):
        net.load(bad)
    with pytest.raises(_native.NativeError, match="non-finite log_std"):
        net.load(random_net_weights(v.obs_dim, 1, (33, 65), 3), np.full(v.act_dim, np.nan, np.float32))
    torch.cuda.synchronize()
    net.close()
    with pytest.raises(RuntimeError, match="closed"):
        net.finish(*tensors)
    with pytest.raises(ValueError, match="closed"):
        PpoRollout(v, MlpActor(v, "relu"), net)
    for x in (default, small, ddpg, other, wide):
        x.close()
