"""GPU: DDPG's replay ring, sampler and critic where tests/test_gpu_ddpg.py does not look -- the tanh critic, rings that
are partly filled, of one slot or written across the wrap-around in one push, sampler keys above 2^32, populations
at which a push's copies leave the 16-byte path, and rewards that try the float64 -> float32 conversion.

The ring and the sampler are compared byte for byte with test_gpu_ddpg's numpy mirror and the sampling law's host
model; the tanh critic with the host model by test_gpu_policy_net's rule for tanh hidden layers (its TANH_FACTOR), its
TD targets with the formula bitwise.  The kernel paths (csrc/sng_ddpg.h) each test reaches:

A. q_net_kernel<TANH = true, TARGET = false> (test_q_tanh_...) and <true, true> (test_targets_tanh_...), at the relu
   tests' widths: 8 and 33 / 65 (no multiple of the 32-wide tile or of a weight group), 400-300, input widths 13 to
   160, batches of 1, 64 and 200 rows (a partial block, one whole block, three and one of 8 rows).
B. replay_sample_kernel with n = filled T E below the ring's capacity, with n = T E of a ring of one slot, and with a
   key whose seed, env offset and counter all exceed 2^32 (replay_sample_key's high halves; sng_replay_sample's
   (uint64_t)env_offset against ReplayRing.host_indices' venv.env_offset).
C. replay_push_kernel with two runs in one push (capacity 2, head 1, two days), and push_copy's three paths
   (ddpg_edge_cases.copy_path: "whole" 16-byte groups from the first element, "peeled" ends around them, "element"
   only) for each of its three instances.  With torch's 256-byte-aligned tensors, in PUSH_SEQUENCE's order (two days
   at once; slice 0 into slot 2; slice 1 into slot 0; then a second ring, slice d into slot d):
       E = 1, 3, 67 (N = 1)   obs: whole, element, element, whole, peeled   done: whole, whole, element, whole, peeled
       E = 256 (N = 1)        every copy whole
       E = 3 (N = 4, "2h")    obs as above                                  done: whole, element, element, whole, peeled
       actions and reward     whole at every E: T E A and T E floats are whole numbers of 16-byte groups
   so the float32 and uint8 instances reach all three paths, and the float64 -> float32 one never leaves "whole" on
   such tensors at any E.  Its other two paths need a destination 8 bytes past a boundary, which only storage of the
   caller's own can be (DisplacedRing), or a source 8 bytes past one (a view): DISPLACED's two pushes take reward
   through "peeled" and "element", actions through "element" and "peeled".  tests/test_ddpg_cpu.py asserts this table.
   E = 1 is the smallest population (every row env 0); 3 and 67 are odd; 256 is the aligned one."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ddpg_edge_cases import (DISPLACED, KEY_COUNTER, KEY_OFFSET, KEY_SEED, PUSH_CASES, PUSH_SEQUENCE,  # noqa: E402
                             partly_filled_samples, seed_where, special_rewards, station_dims)
from policy_net_cases import net_f64, random_net_weights  # noqa: E402
from smart_nanogrid_gym import MlpActor, QCritic, ReplayRing, _native, ddpg  # noqa: E402
from test_gpu_ddpg import (CAPACITY, E, OUT_SCALE, Q_SCALE, Mirror, filled_ring, host, make_env,  # noqa: E402
                           trajectory)
from test_gpu_policy_net import TANH_FACTOR  # noqa: E402

BATCHES = (1, 64, 200)
NETS = [(8, 8), (33, 65), (400, 300)]
GUARD, PATTERN = 64, 0x5A   # elements on each side of a displaced array; the byte they are filled with


def on(v, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(v.device) for a in arrays]


def days_of(traj, d0, d1):
    return [a[d0:d1] for a in traj]


def check_sample(ring, mirror, B, T, E_, what):
    """One sample of B rows against the sampling law's host model and the mirror's gather; the indices."""
    want_idx = ring.host_indices(B)
    s = ring.sample(B)
    torch.cuda.synchronize()
    idx = host(s.indices)
    assert np.array_equal(idx, want_idx), what
    assert idx.min() >= 0 and idx.max() < mirror.filled * T * E_ == len(ring), what
    for name, got, want in zip(s._fields, s[:5], mirror.gather(idx)):
        assert host(got).tobytes() == want.tobytes(), (what, name)
    return idx


# ------------------------------------------------------------------------------------------------------ tanh critic
@pytest.mark.parametrize("N", [1, 10, 50])
def test_q_tanh_keeps_the_tanh_rule_against_float64(N):
    """q_net_kernel<true, false>: the device's Q against net_f64 on [obs | a] within TANH_FACTOR of the host model's
    own distance, per (N, net) over the three batches -- the rule of test_gpu_policy_net's tanh tests, which takes both
    distances as maxima over some hundred rows (a single row's ratio is noise: its d_ref can be 0).  The output scale
    30 multiplies both distances alike.  N = 50 (input width 160) with (33, 65) only.
    Measured on an MI355X (ROCm 7.2), d_dev / d_ref (d_ref): n1 8x8 0.708 (1.17e-06), 33x65 0.796 (2.34e-06), 400x300
    1.244 (3.45e-06); n10 8x8 0.942 (1.78e-06), 33x65 1.434 (2.00e-06), 400x300 1.179 (3.54e-06); n50 33x65 0.851
    (4.12e-06): all below 1.5, the range for which that file sets its factor to 2."""
    v = make_env(N)
    obs, actions, _, _ = trajectory(v, 3)
    obs = torch.from_numpy(obs[0, :3].reshape(-1, v.obs_dim)).to(v.device)
    actions = torch.from_numpy(actions[0, :3].reshape(-1, v.act_dim)).to(v.device)
    for net in (NETS if N != 50 else [(33, 65)]):
        weights = random_net_weights(v.obs_dim + v.act_dim, 1, net, 21, Q_SCALE)
        critic = QCritic(v, net, "tanh").load(weights)
        relu = QCritic(v, net, "relu").load(weights)
        d_ref = d_dev = 0.0
        for B in BATCHES:
            o, a = obs[:B].contiguous(), actions[:B].contiguous()
            q = host(critic.q(o, a)).copy()
            assert q.shape == (B,) and np.isfinite(q).all()
            x = np.concatenate([host(o), host(a)], axis=1)
            ref = net_f64(x, weights, "tanh")[:, 0]
            d_ref = max(d_ref, np.abs(critic.host_q(o, a).astype(np.float64) - ref).max())
            d_dev = max(d_dev, np.abs(q.astype(np.float64) - ref).max())
            assert B == 1 or np.unique(q).size > q.size // 2
            assert (q != host(relu.q(o, a))).mean() > 0.5, (net, B)   # not the relu instance on the same weights
        print(f"q tanh N = {N} {net}: d_ref {d_ref:.4e}, d_dev {d_dev:.4e}, ratio {d_dev / d_ref:.3f}, "
              f"factor {TANH_FACTOR}")
        assert d_dev <= TANH_FACTOR * d_ref, (N, net)
        critic.close()
        relu.close()
    v.close()


@pytest.mark.parametrize("N", [4, 10])
def test_targets_tanh_are_the_formula_bitwise(N):
    """q_net_kernel<true, true> at (33, 65) behind a tanh target actor: given the device's own next actions and the
    device's own q' = critic.q(next_obs, next_actions) -- the same trunk, so no tolerance -- y is the float32 formula
    bit for bit, and a finished row's y is its reward.  200 rows and 1, gamma 0.99 and 0."""
    net = (33, 65)
    v = make_env(N)
    ring, _ = filled_ring(v, seed=5)
    actor_t = MlpActor(v, "tanh", net_arch=net, squash=True).load(
        random_net_weights(v.obs_dim, v.act_dim, net, 11, OUT_SCALE))
    critic_t = QCritic(v, net, "tanh").load(random_net_weights(v.obs_dim + v.act_dim, 1, net, 21, Q_SCALE))
    for B in (200, 1):
        s = ring.sample(B)
        for gamma in (0.99, 0.0):
            y, na = critic_t.targets(actor_t, s, gamma)
            y, na_h = host(y).copy(), host(na).copy()
            assert y.shape == (B, 1) and na_h.shape == (B, v.act_dim) and (np.abs(na_h) <= 1).all()
            q_next = host(critic_t.q(s.next_observations, na))
            done, reward = host(s.dones)[:, 0], host(s.rewards)[:, 0]
            formula = reward + (((np.float32(1.0) - done) * np.float32(gamma)) * q_next)
            assert formula.dtype == np.float32 and y[:, 0].tobytes() == formula.tobytes(), (B, gamma)
            assert np.array_equal(y[done == 1, 0], reward[done == 1])
            if B > 1:
                assert set(np.unique(done)) == {0.0, 1.0} and np.unique(y).size > B // 2
                assert gamma == 0.0 or (y[done == 0, 0] != reward[done == 0]).all()
    for x in (critic_t, actor_t, ring, v):
        x.close()


# ------------------------------------------------------------------------------------- partly filled and small rings
def test_a_partly_filled_ring_samples_its_filled_slots_only():
    """Capacity 3 after one day, then after two: n = filled T E in replay_sample_kernel, below the storage's 3 T E.
    The seed is found on the CPU so that each of the four samples holds a last-step row (its next observation is
    block T of its own slot) and, at filled = 2, rows of both slots.  N = 4, E = 70: the smallest setup of the sibling
    test, whose mirror this is."""
    v = make_env(4)
    T = v.timesteps
    samples = partly_filled_samples(T, E)
    ring, mirror = ReplayRing(v, CAPACITY, seed=seed_where(samples, T, E)), Mirror(v, CAPACITY)
    traj = trajectory(v, 1)
    for d, mine in ((0, samples[:2]), (1, samples[2:])):
        day = days_of(traj, d, d + 1)
        ring.push(*on(v, day))
        mirror.push(*day)
        torch.cuda.synchronize()
        assert (ring.head, ring.filled) == (d + 1, d + 1) and mirror.equals(ring)
        for counter, B, n, slots in mine:
            assert ring.counter == counter and len(ring) == n == (d + 1) * T * E
            idx = check_sample(ring, mirror, B, T, E, (d, B))
            assert ((idx // E) % T == T - 1).any() and set(np.unique(idx // (T * E))) == set(range(slots)), (d, B)
    assert not host(ring.obs[2]).any() and not host(ring.reward[2]).any()   # the unfilled slot was never written
    ring.close()
    v.close()


def test_a_ring_of_one_slot_keeps_the_newest_day():
    """Capacity 1: every push is slot 0 (head stays 0, replay_slot's modulus 1), and a sample draws from T E rows."""
    v = make_env(4)
    T = v.timesteps
    ring, mirror = ReplayRing(v, 1, seed=3), Mirror(v, 1)
    traj = trajectory(v, 1)
    for d in range(2):
        day = days_of(traj, d, d + 1)
        ring.push(*on(v, day))
        mirror.push(*day)
        torch.cuda.synchronize()
        assert (ring.head, ring.filled) == (0, 1) and len(ring) == T * E and mirror.equals(ring)
    assert host(ring.obs).tobytes() == traj[0][1:2].tobytes() != traj[0][0:1].tobytes()
    idx = check_sample(ring, mirror, 64, T, E, "capacity 1")
    s = ring._outputs(64)
    assert host(s.observations).tobytes() == traj[0][1, (idx // E) % T, idx % E].tobytes()   # the second day's rows
    ring.close()
    v.close()


def test_one_push_of_two_days_across_the_wrap_around():
    """Capacity 2 at head 1, two days in one push: replay_runs' two runs (day 0 into slot 1, day 1 into slot 0), eight
    segments in one launch, the most a push has."""
    v = make_env(4)
    T = v.timesteps
    ring, mirror = ReplayRing(v, 2, seed=3), Mirror(v, 2)
    first, both = days_of(trajectory(v, 1), 0, 1), trajectory(v, 2)
    for days in (first, both):
        ring.push(*on(v, days))
        mirror.push(*days)
    torch.cuda.synchronize()
    assert (ring.head, ring.filled) == (1, 2) == (mirror.head, mirror.filled) and mirror.equals(ring)
    assert host(ring.obs[1]).tobytes() == both[0][0].tobytes() and host(ring.obs[0]).tobytes() == both[0][1].tobytes()
    check_sample(ring, mirror, 200, T, E, "wrapped")
    ring.close()
    v.close()


# ------------------------------------------------------------------------------------------------------ sampler keys
def test_sampler_keys_above_2_to_32():
    """Env offset 2^33 + 5, ring seed 2^63 + 5, counter 2^32 + 9: the device's key is the host model's, so the env
    offset reaches replay_sample_key whole on both sides.  Against the same ring at env offset 0 the indices differ in
    200 of 200 rows (1.000, ddpg.replay_host_indices on the CPU; asserted above 0.9 in tests/test_ddpg_cpu.py too)."""
    v = make_env(4, env_offset=KEY_OFFSET)
    T = v.timesteps
    assert v.env_offset == KEY_OFFSET
    ring, mirror = filled_ring(v, seed=KEY_SEED)
    ring.counter = KEY_COUNTER
    assert ring.counter == KEY_COUNTER
    want = ring.host_indices(200, counter=KEY_COUNTER)
    assert np.array_equal(want, ddpg.replay_host_indices(KEY_SEED, KEY_OFFSET, KEY_COUNTER, len(ring), 200))
    idx = check_sample(ring, mirror, 200, T, E, "keys")
    assert np.array_equal(idx, want) and ring.counter == KEY_COUNTER + 1
    at_zero = ddpg.replay_host_indices(KEY_SEED, 0, KEY_COUNTER, len(ring), 200)
    assert (idx != at_zero).mean() > 0.9   # measured: 1.000
    ring.close()
    v.close()


# ------------------------------------------------------------------------------------------- the copy's three paths
@pytest.mark.parametrize("N,interval,E_", PUSH_CASES, ids=[f"n{n}-{i}-e{e}" for n, i, e in PUSH_CASES])
def test_pushes_at_populations_that_move_the_copy_off_its_vector_path(N, interval, E_):
    """PUSH_SEQUENCE at one population (the module docstring lists each copy's path): all four arrays equal the mirror
    byte for byte after every push."""
    v = make_env(N, interval, E=E_)
    T = v.timesteps
    assert (T, v.obs_dim, v.act_dim) == station_dims(N, interval) and v.num_envs == E_
    traj = trajectory(v, 1, E_)
    dev = on(v, traj)
    rings = {name: (ReplayRing(v, CAPACITY, seed=2), Mirror(v, CAPACITY, E_)) for name in ("wrap", "slots")}
    for number, (name, days, d0) in enumerate(PUSH_SEQUENCE):
        ring, mirror = rings[name]
        ring.push(*[x[d0:d0 + days] for x in dev])
        mirror.push(*days_of(traj, d0, d0 + days))
        torch.cuda.synchronize()
        assert (ring.head, ring.filled) == (mirror.head, mirror.filled), number
        assert mirror.equals(ring), f"push {number} into {name}"
    ring, mirror = rings["wrap"]
    assert (ring.head, ring.filled) == (1, 3)
    if E_ == 1:   # n = filled T, and every row is env 0
        assert len(ring) == 3 * T
        idx = check_sample(ring, mirror, 64, T, 1, "E = 1")
        assert idx.max() < 3 * T and np.unique(idx).size > 16
    for ring, _ in rings.values():
        ring.close()
    v.close()


class DisplacedRing(ReplayRing):
    """A ReplayRing on storage of the test's own (include/sng.h: SngReplaySpec's device pointers are the caller's):
    each array `displacement[name]` elements past a 256-byte boundary, between two guards of GUARD elements filled
    with PATTERN bytes."""

    def __init__(self, venv, capacity_days, displacement, seed=0):
        self.venv, self.capacity_days, self.seed = venv, int(capacity_days), int(seed)
        self._p = None
        T, n_envs, dev = venv.timesteps, venv.num_envs, venv.device
        shapes = dict(obs=((capacity_days, T + 1, n_envs, venv.obs_dim), torch.float32),
                      actions=((capacity_days, T, n_envs, venv.act_dim), torch.float32),
                      reward=((capacity_days, T, n_envs), torch.float32), done=((capacity_days, T, n_envs), torch.uint8))
        self._raw, self._span = {}, {}
        for name, (shape, dtype) in shapes.items():
            n, lead = int(np.prod(shape)), GUARD + displacement[name]
            size = torch.empty((), dtype=dtype).element_size()
            raw = torch.full(((lead + n + GUARD) * size,), PATTERN, dtype=torch.uint8, device=dev)
            assert raw.data_ptr() % 256 == 0
            view = raw.view(dtype)[lead:lead + n].view(*shape)
            view.zero_()
            assert view.is_contiguous() and view.data_ptr() % 16 == displacement[name] * size % 16
            setattr(self, name, view)
            self._raw[name], self._span[name] = raw, (lead * size, (lead + n) * size)
        spec = _native.SngReplaySpec(self.capacity_days, self.seed, self.obs.data_ptr(), self.actions.data_ptr(),
                                     self.reward.data_ptr(), self.done.data_ptr())
        h = ctypes.c_void_p()
        _native.check(_native.lib().sng_replay_create(venv._h, ctypes.byref(spec), ctypes.byref(h)), venv._h)
        self._own(venv, h)
        self._out = {}

    def guards_intact(self):
        return all(bool((raw[:lo] == PATTERN).all()) and bool((raw[hi:] == PATTERN).all())
                   for raw, (lo, hi) in ((self._raw[n], self._span[n]) for n in self._raw))


def displaced(t, elements):
    """A contiguous copy of tensor t that starts `elements` elements past a 256-byte boundary."""
    buf = torch.empty(t.numel() + elements, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 256 == 0
    out = buf[elements:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == elements * t.element_size() % 16
    return out


def test_pushes_into_displaced_storage_and_from_displaced_sources():
    """DISPLACED: storage and sources off the 16-byte boundaries, which takes the float64 -> float32 copy through its
    peeled and element-only paths (first push: destination 8 bytes past a boundary, source on one, so 2 floats are
    peeled and 70 = 17 groups + 2 follow; second: the source 8 bytes past one) and the float32 copy through a peeled
    one whose head is 1 float.  Every array equals the mirror, and no byte of a guard changes."""
    N, interval, E_, storage, sources = DISPLACED
    v = make_env(N, interval, E=E_)
    T = v.timesteps
    assert (T, v.obs_dim, v.act_dim) == station_dims(N, interval)
    traj = trajectory(v, 1, E_)
    ring, mirror = DisplacedRing(v, CAPACITY, storage, seed=2), Mirror(v, CAPACITY, E_)
    assert ring.guards_intact()
    names = ("obs", "actions", "reward", "done")
    for d, src in enumerate(sources):
        day = days_of(traj, d, d + 1)
        ring.push(*[displaced(t, src[n]) for n, t in zip(names, on(v, day))])
        mirror.push(*day)
        torch.cuda.synchronize()
        assert (ring.head, ring.filled) == (d + 1, d + 1) and mirror.equals(ring), d
        assert ring.guards_intact(), f"push {d} wrote outside the ring's storage"
    check_sample(ring, mirror, 64, T, E_, "displaced")   # the sampler reads from unaligned storage alike
    ring.close()
    v.close()


# -------------------------------------------------------------------------------------------------- reward conversion
@pytest.mark.parametrize("path", ["whole", "peeled", "element"])
def test_reward_conversion_is_round_to_nearest_even_with_subnormals(path):
    """One day at N = 1, E = 67 (1,608 rewards) whose float64 rewards are ddpg_edge_cases.special_rewards repeated over
    the block: exact float32 values, ties between two float32 neighbours with an even and an odd lower neighbour,
    float32 subnormals, -0.0, values beyond float32's range, and float64 neighbours of float32 values.  The ring's
    reward is numpy's reward.astype(float32) (IEEE round to nearest even, gradual underflow, overflow to infinity)
    byte for byte.  "whole": a ReplayRing and torch's tensors, 402 16-byte groups and no ends, the only path such
    tensors take.  "peeled": the storage 2 floats past a boundary, so 2 elements before the 401 groups and 2 behind
    them go through the scalar conversion.  "element": the source one double past a boundary."""
    v = make_env(1, E=67)
    T = v.timesteps
    obs, actions, reward, done = days_of(trajectory(v, 1, 67), 0, 1)
    special, kinds = special_rewards(reward.size)
    reward = special.reshape(reward.shape)
    assert len(kinds) == 7 and reward.size == 1608 > 4 * sum(len(x) for x in kinds.values())
    with np.errstate(over="ignore"):
        want = reward.astype(np.float32)
    assert np.isinf(want).any() and (want == 0).any() and ((want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)).any()
    zero = dict(obs=0, actions=0, reward=0, done=0)
    ring = (ReplayRing(v, CAPACITY) if path == "whole" else
            DisplacedRing(v, CAPACITY, dict(zero, reward=2 if path == "peeled" else 0)))
    dev = on(v, (obs, actions, reward, done))
    if path == "element":
        dev[2] = displaced(dev[2], 1)
    ring.push(*dev)
    torch.cuda.synchronize()
    got = host(ring.reward[0])
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want[0].view(np.uint32).ravel())
    assert bad.size == 0, [(int(i), float(reward.ravel()[i]), float(got.ravel()[i]), float(want.ravel()[i])) for i in bad[:8]]
    assert got.tobytes() == want.tobytes() and not host(ring.reward[1:]).any()
    assert path == "whole" or ring.guards_intact()
    ring.close()
    v.close()
