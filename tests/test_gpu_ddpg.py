"""GPU: the off-policy side of DDPG (include/sng.h: sng_replay_*, sng_critic_*; smart_nanogrid_gym/ddpg.py: ReplayRing,
QCritic, DdpgCollector).

E = 70 with two days into a ring of three, so the second push wraps; stations of 1, 4 and 10 chargers at "1h", 4 at
"2h" (T = 12) and 50 (the critic's input width 160).  Batches of 1, 64 and 200 rows: a single partial block of the
sampler's and the critic's 64 rows, no partial block, three full blocks and one of 8.  The ring and the sampler are
integer work and copies: everything is compared byte for byte with a numpy mirror.  With relu the critic is exactly
reproducible on the CPU: q and y are compared by value (==) with the host model, and given the device's own next
actions and q' the targets are bitwise the formula."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from policy_net_cases import net_f64, random_net_weights  # noqa: E402
from smart_nanogrid_gym import (ActionNoise, ClosedLoopGraph, DdpgCollector, MlpActor, QCritic, ReplayRing,  # noqa: E402
                                SmartNanogridVecEnv, _native, ddpg)
from test_gpu_policy_net import SQUASH_FACTOR  # noqa: E402
from test_gpu_ppo_net_rollout import synthetic  # noqa: E402

SEED, DAYS, CAPACITY, E = 4321, 2, 3, 70
BATCHES = (1, 64, 200)
Q_SCALE, OUT_SCALE = 30.0, 4.0
NETS = [(8, 8), (33, 65), (400, 300), (512, 512)]
CASES = [(1, "1h"), (4, "1h"), (10, "1h"), (4, "2h"), (50, "1h")]
IDS = [f"n{n}-{i}" for n, i in CASES]
BASE = dict(charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
            battery_system_available_in_model=True)


def make_env(N, interval="1h", E=E, env_offset=0):
    return SmartNanogridVecEnv(E, seed=SEED, rng="device", number_of_chargers=N, time_interval=interval,
                               env_offset=env_offset, **BASE)


def host(x):
    return x.cpu().numpy()


def trajectory(v, seed, E=E):
    """test_gpu_ppo_net_rollout's synthetic trajectory with stored actions in [-1, 1] beside it: (obs, actions,
    reward float64, done uint8) of DAYS days."""
    obs, reward, done, _, _ = synthetic(v, seed)
    rng = np.random.default_rng(seed + 100)
    actions = rng.uniform(-1, 1, (DAYS, v.timesteps, E, v.act_dim)).astype(np.float32)
    return obs, actions, reward, done


class Mirror:
    """The ring in numpy: the contract's bookkeeping and layout."""

    def __init__(self, v, capacity, E=E):
        T = v.timesteps
        self.capacity, self.head, self.filled, self.T, self.E = capacity, 0, 0, T, E
        self.obs = np.zeros((capacity, T + 1, E, v.obs_dim), np.float32)
        self.actions = np.zeros((capacity, T, E, v.act_dim), np.float32)
        self.reward = np.zeros((capacity, T, E), np.float32)
        self.done = np.zeros((capacity, T, E), np.uint8)

    def push(self, obs, actions, reward, done):
        for d in range(obs.shape[0]):
            s = (self.head + d) % self.capacity
            self.obs[s], self.actions[s], self.done[s] = obs[d], actions[d], done[d]
            self.reward[s] = reward[d].astype(np.float32)
        self.head = (self.head + obs.shape[0]) % self.capacity
        self.filled = min(self.filled + obs.shape[0], self.capacity)

    def __len__(self):
        return self.filled * self.T * self.E

    def gather(self, idx):
        T, E = self.T, self.E
        slot, t, e = idx // (T * E), (idx // E) % T, idx % E
        return (self.obs[slot, t, e], self.actions[slot, t, e], self.obs[slot, t + 1, e],
                self.done[slot, t, e].astype(np.float32)[:, None], self.reward[slot, t, e][:, None])

    def equals(self, ring):
        return all(host(getattr(ring, n)).tobytes() == getattr(self, n).tobytes()
                   for n in ("obs", "actions", "reward", "done"))


def filled_ring(v, seed=0, E=E):
    """A ring of three slots after two pushes of two days, and its mirror."""
    ring, mirror = ReplayRing(v, CAPACITY, seed=seed), Mirror(v, CAPACITY, E)
    for s in (1, 2):
        traj = trajectory(v, s, E)
        ring.push(*[torch.from_numpy(a).to(v.device) for a in traj])
        mirror.push(*traj)
    return ring, mirror


def seed_with_last_steps(n, T, counters_and_batches):
    """The first sampler seed, found on the CPU, with which every one of these samples holds a last-step row."""
    for seed in range(10000):
        if all((((ddpg.replay_host_indices(seed, 0, c, n, b) // E) % T) == T - 1).any() for c, b in counters_and_batches):
            return seed
    raise AssertionError("no seed found")


# ------------------------------------------------------------------------------------------------- push, wrap, sample
@pytest.mark.parametrize("N,interval", CASES, ids=IDS)
def test_push_wraps_and_samples_equal_the_numpy_mirror(N, interval):
    v = make_env(N, interval)
    T = v.timesteps
    assert T == (12 if interval == "2h" else 24)
    seed = seed_with_last_steps(CAPACITY * T * E, T, list(enumerate(BATCHES)))
    ring, mirror = ReplayRing(v, CAPACITY, seed=seed), Mirror(v, CAPACITY)
    assert len(ring) == 0 and (ring.head, ring.filled) == (0, 0)
    for s, (head, filled) in ((1, (2, 2)), (2, (1, 3))):   # the second push wraps: slots 2, 0
        traj = trajectory(v, s)
        assert ring.push(*[torch.from_numpy(a).to(v.device) for a in traj]) is ring
        mirror.push(*traj)
        torch.cuda.synchronize()
        assert (ring.head, ring.filled) == (head, filled) == (mirror.head, mirror.filled)
        assert len(ring) == len(mirror) == filled * T * E
        assert mirror.equals(ring), f"push {s}"
    for c, B in enumerate(BATCHES):
        assert ring.counter == c
        want_idx = ring.host_indices(B)
        s = ring.sample(B)
        torch.cuda.synchronize()
        idx = host(s.indices)
        assert idx.dtype == np.int64 and np.array_equal(idx, want_idx) and idx.max() < len(ring)
        assert [tuple(x.shape) for x in s] == [(B, v.obs_dim), (B, v.act_dim), (B, v.obs_dim), (B, 1), (B, 1), (B,)]
        for name, got, want in zip(s._fields, s[:5], mirror.gather(idx)):
            assert host(got).tobytes() == want.tobytes(), (B, name)
        last = (idx // E) % T == T - 1
        assert last.any(), B
        slot, e = idx[last] // (T * E), idx[last] % E
        assert host(s.next_observations)[last].tobytes() == mirror.obs[slot, T, e].tobytes()   # block T of its own slot
        assert set(np.unique(host(s.dones))) <= {0.0, 1.0}
    # a second sample differs from the first; the counter set back reproduces the first
    c = ring.counter
    first = [host(x).copy() for x in ring.sample(64)]
    second = [host(x).copy() for x in ring.sample(64)]
    assert ring.counter == c + 2 and not np.array_equal(first[5], second[5]) and first[0].tobytes() != second[0].tobytes()
    ring.counter = c
    again = [host(x) for x in ring.sample(64)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    # days pushed one by one from slices: day 1 and slot 1 lie one day behind a 16-byte boundary alike, which at the
    # stations whose day is no whole number of 16-byte groups (N = 1; the flags at T = 12) is the copy's peeled ends
    ring2, mirror2 = ReplayRing(v, CAPACITY), Mirror(v, CAPACITY)
    traj = trajectory(v, 3)
    on_device = [torch.from_numpy(a).to(v.device) for a in traj]
    for d in range(DAYS):
        ring2.push(*[x[d:d + 1] for x in on_device])
        mirror2.push(*[a[d:d + 1] for a in traj])
    torch.cuda.synchronize()
    assert (ring2.head, ring2.filled) == (2, 2) and mirror2.equals(ring2)
    for x in (ring2, ring, v):
        x.close()


# ------------------------------------------------------------------------------------------------------------ critic
@pytest.mark.parametrize("N,interval", CASES, ids=IDS)
def test_q_relu_equals_the_host_model(N, interval):
    v = make_env(N, interval)
    obs, actions, _, _ = trajectory(v, 3)
    obs = torch.from_numpy(obs[0, :3].reshape(-1, v.obs_dim)).to(v.device)
    actions = torch.from_numpy(actions[0, :3].reshape(-1, v.act_dim)).to(v.device)
    ran = 0
    for net in NETS:
        if N == 50 and net == (512, 512):   # the input width 160: 172,544 B of LDS
            with pytest.raises(_native.NativeError, match=r"libsng error -2.*109 \+ 51.*172544 B of 163840"):
                QCritic(v, net)
            continue
        critic = QCritic(v, net).load(random_net_weights(v.obs_dim + v.act_dim, 1, net, 21, Q_SCALE))
        for B in BATCHES:
            q = host(critic.q(obs[:B].contiguous(), actions[:B].contiguous()))
            want = critic.host_q(obs[:B], actions[:B])
            np.testing.assert_array_equal(q, want, err_msg=f"N={N} {net} B={B}")
            assert B == 1 or np.unique(q).size > q.size // 2
            ran += 1
        critic.close()
    assert ran == (9 if N == 50 else 12)
    v.close()


@pytest.mark.parametrize("N,interval", CASES, ids=IDS)
def test_targets(N, interval):
    """next_actions against the host actor by test_gpu_policy_net's rule for a squashed actor (d_dev <= SQUASH_FACTOR
    d_ref against float64); y == the host targets given the device's own next_actions; given those and the device's
    q', y is bitwise the formula; new target weights change the next call.  Measured on an MI355X (ROCm 7.2),
    d_dev / d_ref: n1 0.955 (d_ref 3.28e-07), n4 0.918 (2.33e-07), n10 0.857 (4.18e-07), n4-2h 1.000 (2.73e-07), n50
    1.018 (4.45e-07)."""
    v = make_env(N, interval)
    ring, _ = filled_ring(v, seed=5)
    arch = ddpg.DDPG_NET_ARCH
    aw = random_net_weights(v.obs_dim, v.act_dim, arch, 11, OUT_SCALE)
    actor_t = MlpActor.ddpg(v).load(aw)
    qw = random_net_weights(v.obs_dim + v.act_dim, 1, arch, 21, Q_SCALE)
    critic_t = QCritic(v).load(qw)
    d_ref = d_dev = 0.0
    for B in (200, 1):
        s = ring.sample(B)
        for gamma in (0.99, 0.0):
            y, na = critic_t.targets(actor_t, s, gamma)
            assert tuple(y.shape) == (B, 1) and tuple(na.shape) == (B, v.act_dim)
            y, na_h = host(y).copy(), host(na).copy()
            nobs = host(s.next_observations)
            host_a = actor_t.host_actions(nobs)[0]
            ref = net_f64(nobs, aw, "relu", squash=True)
            d_ref = max(d_ref, np.abs(host_a.astype(np.float64) - ref).max())
            d_dev = max(d_dev, np.abs(na_h.astype(np.float64) - ref).max())
            assert (np.abs(na_h) <= 1).all()
            want, _ = critic_t.host_targets(s, gamma, next_actions=na_h)
            np.testing.assert_array_equal(y[:, 0], want, err_msg=f"B={B} gamma={gamma}")
            q_next = host(critic_t.q(s.next_observations, na))
            done, reward = host(s.dones)[:, 0], host(s.rewards)[:, 0]
            formula = reward + (((np.float32(1.0) - done) * np.float32(gamma)) * q_next)
            assert formula.dtype == np.float32 and y[:, 0].tobytes() == formula.tobytes(), (B, gamma)
            if B > 1:
                assert set(np.unique(done)) == {0.0, 1.0} and np.unique(y).size > B // 2
                assert np.array_equal(y[done == 1, 0], reward[done == 1])
                assert gamma == 0.0 or (y[done == 0, 0] != reward[done == 0]).all()
    print(f"targets N = {N}: d_ref {d_ref:.4e}, d_dev {d_dev:.4e}, ratio {d_dev / d_ref:.3f}, factor {SQUASH_FACTOR}")
    assert d_dev <= SQUASH_FACTOR * d_ref
    # new target weights between two calls change the next call
    s = ring.sample(64)
    before = host(critic_t.targets(actor_t, s)[0]).copy()
    critic_t.load(random_net_weights(v.obs_dim + v.act_dim, 1, arch, 22, Q_SCALE))
    after, na = (host(x).copy() for x in critic_t.targets(actor_t, s))
    assert (after != before).mean() > 0.5
    np.testing.assert_array_equal(after[:, 0], critic_t.host_targets(s, next_actions=na)[0])
    actor_t.load(random_net_weights(v.obs_dim, v.act_dim, arch, 12, OUT_SCALE))
    assert (host(critic_t.targets(actor_t, s)[0]) != after).mean() > 0.5
    for x in (critic_t, actor_t, ring, v):
        x.close()


# -------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("N", [4, 10])
def test_collector_fills_the_ring_with_the_closed_loop_days(N):
    """Two launches of a DdpgCollector (DDPG's actor, an OU source) into capacity 3: the ring's newest slots are a plain
    ClosedLoopGraph's second launch from a fresh handle with the same seeds."""
    weights = random_net_weights(2 * N + 9, N + 1, ddpg.DDPG_NET_ARCH, 11, OUT_SCALE)

    def parts():
        v = make_env(N)
        return v, MlpActor.ddpg(v).load(weights), ActionNoise(v, "ou", seed=9, mu=0.0, scale=0.5)
    v, actor, noise = parts()
    ring = ReplayRing(v, CAPACITY, seed=1)
    col = DdpgCollector(v, actor, noise, ring, days=DAYS)
    col.launch()
    col.launch()
    w, actor_w, noise_w = parts()
    plain = ClosedLoopGraph(w, actor_w, noise=noise_w, days=DAYS, trajectory=True)
    plain.launch()
    plain.launch()
    torch.cuda.synchronize()
    assert (ring.head, ring.filled) == (1, 3) and len(ring) == 3 * v.timesteps * E
    for d, slot in enumerate((2, 0)):   # the second launch's days
        assert host(ring.obs[slot]).tobytes() == host(plain.obs_traj[d]).tobytes()
        assert host(ring.actions[slot]).tobytes() == host(plain.action_traj[d]).tobytes()
        assert host(ring.reward[slot]).tobytes() == host(plain.reward_traj[d]).astype(np.float32).tobytes()
        assert host(ring.done[slot]).tobytes() == host(plain.done_traj[d]).tobytes()
    assert host(ring.obs[1]).tobytes() != host(ring.obs[2]).tobytes() and host(ring.done[:, -1]).all()
    assert host(col.graph.obs_traj).tobytes() == host(plain.obs_traj).tobytes()
    s = ring.sample(64)
    critic_t = QCritic(v).load(random_net_weights(v.obs_dim + v.act_dim, 1, ddpg.DDPG_NET_ARCH, 21, Q_SCALE))
    y, na = critic_t.targets(actor, s)
    y = host(y)
    assert np.isfinite(y).all() and np.unique(y).size > 32 and (np.abs(host(na)) <= 1).all()
    for x in (col, plain, critic_t, ring, noise, noise_w, actor, actor_w, v, w):
        x.close()


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals_on_the_device_path():
    v, other = make_env(4), make_env(4)
    ring = ReplayRing(v, CAPACITY)
    with pytest.raises(ValueError, match="empty"):
        ring.sample(8)
    out = _native.SngReplayBatch(*[ring.obs.data_ptr()] * 5, None)
    assert _native.lib().sng_replay_sample(ring._p, 8, out, None) == -1    # the library's own refusal
    assert b"empty" in _native.lib().sng_last_error(v._h)
    traj = [torch.from_numpy(a).to(v.device) for a in trajectory(v, 1)]
    ring.push(*traj)
    with pytest.raises(ValueError, match="batch"):
        ring.sample(0)
    with pytest.raises(ValueError, match="obs must be"):
        ring.push(traj[0][:, :-1].contiguous(), *traj[1:])
    with pytest.raises(ValueError, match="reward must be"):
        ring.push(traj[0], traj[1], traj[2].float(), traj[3])
    with pytest.raises(_native.NativeError, match="capacity_days 3"):
        ring.push(*[torch.cat([t, t]) for t in traj])
    with pytest.raises(_native.NativeError, match="capacity_days 0"):
        ReplayRing(v, 0)
    g = ClosedLoopGraph(other, MlpActor(other, "relu"), trajectory=True)
    with pytest.raises(ValueError, match="graph was made for another env batch"):
        ring.push(g)
    with pytest.raises(ValueError, match="ring was made for another env batch"):
        DdpgCollector(other, g.actor, None, ring)
    # targets: a foreign actor, a 64-64 policy_kernel actor, a bad gamma, foreign-shaped samples
    critic = QCritic(v, (33, 65))
    ddpg_actor, ppo_actor, foreign_actor = MlpActor.ddpg(v), MlpActor(v, "relu"), MlpActor.ddpg(other)
    s = ring.sample(8)
    with pytest.raises(ValueError, match="actor_target must run policy_net_kernel"):
        critic.targets(ppo_actor, s)
    assert _native.lib().sng_critic_targets(critic._p, ppo_actor._p, 8, *[s.rewards.data_ptr()] * 3, 0.99,
                                            *[s.rewards.data_ptr()] * 2, None) == -2
    with pytest.raises(ValueError, match="actor_target was made for another env batch"):
        critic.targets(foreign_actor, s)
    with pytest.raises(_native.NativeError, match="gamma"):
        critic.targets(ddpg_actor, s, gamma=1.5)
    with pytest.raises(_native.NativeError, match="gamma"):
        critic.targets(ddpg_actor, s, gamma=float("nan"))
    with pytest.raises(ValueError, match="samples.rewards must be"):
        critic.targets(ddpg_actor, s._replace(rewards=s.rewards[:, 0]))
    with pytest.raises(ValueError, match="actions must be"):
        critic.q(s.observations, s.observations)
    with pytest.raises(_native.NativeError, match="libsng error -2"):
        _native.check(_native.lib().sng_policy_actions_rows(ppo_actor._p, 8, s.observations.data_ptr(), None,
                                                           s.actions.data_ptr(), None, None), v._h)
    # rows through sng_policy_actions_rows are the actor's own rows
    a8 = torch.empty((8, v.act_dim), dtype=torch.float32, device=v.device)
    _native.check(_native.lib().sng_policy_actions_rows(ddpg_actor._p, 8, s.observations.data_ptr(), None, a8.data_ptr(),
                                                        None, None), v._h)
    torch.cuda.synchronize()
    assert not host(a8).any()   # zero weights until load(): tanh(0)
    # closed handles
    ddpg_actor.close()
    with pytest.raises(ValueError, match="actor_target is closed"):
        critic.targets(ddpg_actor, s)
    critic.close()
    with pytest.raises(RuntimeError, match="the critic is closed"):
        critic.q(s.observations, s.actions)
    ring.close()
    with pytest.raises(RuntimeError, match="the replay ring is closed"):
        ring.sample(8)
    with pytest.raises(RuntimeError, match="the replay ring is closed"):
        ring.push(*traj)
    assert len(ring) == 0
    with pytest.raises(ValueError, match="ring is closed"):
        DdpgCollector(v, ppo_actor, None, ring)
    for x in (g, ppo_actor, foreign_actor, v, other):
        x.close()
