"""GPU: the action noise source where tests/test_gpu_action_noise.py does not look -- fills of more days than a grid
has rows, outputs that are not 16-byte aligned or sit between guards, graphs with a source in the other
configurations, and a source that changes between two launches of one captured graph.

Every comparison is bitwise against the host model (policy.noise_host_fill / ActionNoise.host_fill, and
MlpActor.host_actions / PpoHead.host_finish for what follows the noise), as in the sibling file.  The kernel paths
(csrc/sng_noise.h, launch_noise_fill) each case reaches:

A. days = 65,537 = kNoiseMaxGridDays + 2: grid.y is capped at 65,535 rows, so the workgroups of blockIdx.y = 0 and 1
   take a *second pass of the day loop* (days 65,535 and 65,536) and rebuild the day key, the stream keys, the OU state
   and the output pointer there.  A = 2, E = 1 (row 2) and A = 5, E = 3 (row 15) run it on the *scalar path by row
   length*, A = 2, E = 2 (row 4, aligned base) on the vector path, and the same row displaced by one float on the
   *scalar path by pointer*.  days = 65,535 is the largest fill with no second pass.
B. rows that are a multiple of four with the base displaced by 0 .. 3 floats from a 16-byte boundary: displacement 0 is
   the vector path, 1 .. 3 the *scalar path by pointer*, and all four give the same bytes.  Rows that are no multiple
   of four (15, 129, 693, 1,161) are the *scalar path by row length* with a *partial last thread*, which owns one to
   three elements past the row's end and stores none of them.  Rows of 2,200 and 1,161 floats are more than one
   workgroup with a partial last one.  Every output lies between two guards of 64 floats that must stay untouched.
C. captured graphs with a source: trajectory=False (one output block, the noise still one block per day), a
   steps-only graph (with_reset=False, days = 1) and a sharded population (env_offset != 0 in the captured fill).
D. one captured graph launched again after set(), after a new counter and after PpoRollout.load(): the fill node
   reads the source's device parameters and counter at every launch.  fill(stream=...) on a side stream."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from policy_net_cases import random_net_weights  # noqa: E402
from smart_nanogrid_gym import (ActionNoise, ClosedLoopGraph, MlpActor, PpoHead, PpoRollout, _native, policy)  # noqa: E402
from test_gpu_action_noise import (BIG_OFFSET, DAYS, GRAPHS, NAMES, OUT_SCALE, host, make_env, same,  # noqa: E402
                                   sb3_state_dict)

GUARD, PATTERN = 64, 0x7FC0BEEF   # floats on each side of a guarded output; a NaN no fill produces
GRID_DAYS = 65535                 # csrc/sng_noise.h kNoiseMaxGridDays
SRC_SEED, THETA, DT = 2 ** 40 + 77, 0.3, 0.05
NET = (64, 64)
GRAPH_IDS = ["lean4", "wide10", "lean4-33x65", "lean4-fused"]


class Guarded:
    """A float32 output [days, T, E, A] inside one flat allocation of the test's own: GUARD floats of PATTERN before
    it (plus `displacement` more, which move its base off a 16-byte boundary) and GUARD after it."""

    def __init__(self, shape, displacement, device):
        assert 0 <= displacement < 4
        n = int(np.prod(shape))
        self.lead, self.n = GUARD + displacement, n
        self.buf = torch.empty(self.lead + n + GUARD, dtype=torch.float32, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.bits = self.buf.view(torch.int32)
        self.bits.fill_(PATTERN)
        self.out = self.buf[self.lead:self.lead + n].view(*shape)
        assert self.out.is_contiguous() and self.out.data_ptr() % 16 == 4 * displacement

    def guards_intact(self):
        before, after = self.bits[:self.lead], self.bits[self.lead + self.n:]
        assert before.numel() == self.lead and after.numel() == GUARD
        return bool((before == PATTERN).all()) and bool((after == PATTERN).all())


def per_action(A):
    return np.linspace(-0.5, 0.75, A).astype(np.float32), np.linspace(0.1, 1.3, A).astype(np.float32)


def make_source(v, kind, c0):
    mu, scale = per_action(v.act_dim)
    src = ActionNoise(v, kind, seed=SRC_SEED, mu=mu, scale=scale, theta=THETA, dt=DT)
    src.counter = c0
    return src


def guarded_fill(src, days, displacement):
    """One fill of `days` blocks into a guarded output: the block on the host, after the guards were checked."""
    v = src.venv
    g = Guarded((days, v.timesteps, v.num_envs, v.act_dim), displacement, v.device)
    assert src.fill(days, out=g.out) is g.out
    torch.cuda.synchronize()
    assert g.guards_intact(), f"a store outside the block: displacement {displacement}"
    return host(g.out)


# ------------------------------------------------------------------- A. more days than the grid has rows
# (N, E, displacement, c0).  c0 = 2^32 - 3: c0 + d carries into the counter's high word at day 3, so all the later days
# -- the second pass's among them -- are keyed with a high word of 1.  c0 = 2^32 - 65,536: the carry falls on day
# 65,536, inside the second pass of the workgroup with blockIdx.y = 1.
MANY_DAYS = [(1, 1, 0, 2 ** 32 - 3), (4, 3, 0, 2 ** 32 - 3), (1, 2, 0, 2 ** 32 - 65536), (1, 2, 1, 2 ** 32 - 3)]


@pytest.mark.parametrize("kind", ["gaussian", "ou"])
@pytest.mark.parametrize("N,E,displacement,c0", MANY_DAYS,
                         ids=["row2-scalar", "row15-scalar", "row4-vector", "row4-displaced"])
def test_fill_with_more_days_than_grid_rows(N, E, displacement, c0, kind):
    """days = 65,537 at T = 12.  The scalar case of the larger row is A = 5, E = 3 (row 15, 47 MB, 11.8 M variates):
    the host model fills it in 0.2 s, so E was not reduced.  The two rows of four floats are additions to the cases
    of A = 2, E = 1, whose row of two floats cannot take the 16-byte stores."""
    days = GRID_DAYS + 2
    v = make_env(N, E, "2h")
    assert v.timesteps == 12 and v.act_dim == N + 1
    src = make_source(v, kind, c0)
    got = guarded_fill(src, days, displacement)
    assert same(got, src.host_fill(days, counter=c0)), f"{kind} row {E * v.act_dim}"
    assert src.counter == c0 + days
    # days 0 and 65,535 are the two passes of the workgroup with blockIdx.y = 0, days 1 and 65,536 those of 1
    picks = (0, 1, GRID_DAYS, GRID_DAYS + 1)
    for i, a in enumerate(picks):
        for b in picks[i + 1:]:
            assert not np.array_equal(got[a], got[b]), (a, b)
    src.close()
    v.close()


@pytest.mark.parametrize("kind", ["gaussian", "ou"])
def test_largest_fill_without_a_second_pass(kind):
    c0 = 2 ** 32 - 3
    v = make_env(1, 1, "2h")
    src = make_source(v, kind, c0)
    got = guarded_fill(src, GRID_DAYS, 0)
    assert same(got, src.host_fill(GRID_DAYS, counter=c0)) and src.counter == c0 + GRID_DAYS
    assert not np.array_equal(got[0], got[-1])
    src.close()
    v.close()


# ------------------------------------------------------------------------------- B. alignment and bounds
# (N, E, interval, env_offset): rows of 128, 4, 280, 504 and 2,200 floats (three workgroups, the last partial) ...
ROWS_OF_FOURS = [(1, 64, "1h", 0), (1, 2, "2h", BIG_OFFSET), (3, 70, "1h", BIG_OFFSET), (7, 63, "2h", 0),
                 (10, 200, "1h", 0)]
# ... and of 15, 129, 693 and 1,161 (two workgroups): the last thread owns 1, 3, 3 and 3 elements past the row's end
OTHER_ROWS = [(4, 3, "1h", BIG_OFFSET), (128, 1, "2h", 0), (10, 63, "2h", BIG_OFFSET), (128, 9, "1h", 0)]


@pytest.mark.parametrize("kind", ["gaussian", "ou"])
@pytest.mark.parametrize("N,E,interval,offset", ROWS_OF_FOURS + OTHER_ROWS, ids=lambda x: str(x))
def test_displaced_and_guarded_outputs(N, E, interval, offset, kind):
    days, c0 = 3, 2 ** 32 - 2
    v = make_env(N, E, interval, offset)
    A, T = v.act_dim, v.timesteps
    assert ((E * A) % 4 == 0) == ((N, E, interval, offset) in ROWS_OF_FOURS) and T == (24 if interval == "1h" else 12)
    mu, scale = per_action(A)
    want = policy.noise_host_fill(kind, A, T, E, days, SRC_SEED, mu, scale, THETA, DT, offset, c0)
    assert np.isfinite(want).all() and not np.array_equal(want[0], want[1])
    src = make_source(v, kind, c0)
    for displacement in range(4):   # 0: 16-byte stores where the row allows them; 1 .. 3: 4-byte stores
        src.counter = c0
        got = guarded_fill(src, days, displacement)
        assert same(got, want), f"{kind} row {E * A} displaced by {displacement} floats"
        assert src.counter == c0 + days
    src.close()
    v.close()


# ------------------------------------------------------- C. graphs with a source, beyond the tested configuration
def relu_actor(v, net, weights=None):
    weights = random_net_weights(v.obs_dim, v.act_dim, net, 11, OUT_SCALE) if weights is None else weights
    return MlpActor(v, "relu", net_arch=net).load(weights)


def graph_source(v, c0, seed=5):
    src = ActionNoise(v, "gaussian", seed=seed, mu=0.0, scale=np.linspace(0.2, 0.9, v.act_dim).astype(np.float32))
    src.counter = c0
    return src


def assert_actions_are_the_host_actors(actor, obs, nz, act, what):
    for d in range(act.shape[0]):
        for t in range(act.shape[1]):
            assert same(act[d, t], actor.host_actions(obs[d, t], nz[d, t])[0]), f"{what} day {d} step {t}"


@pytest.mark.parametrize("N,net,fused", GRAPHS, ids=GRAPH_IDS)
def test_graph_without_a_trajectory_still_draws_a_block_per_day(N, net, fused):
    E, c0 = 70, 7
    v, w = make_env(N, E), make_env(N, E)   # the same seed: the same device days
    T, A = v.timesteps, v.act_dim
    actor, actor_w = relu_actor(v, net), relu_actor(w, net)
    src, src_w = graph_source(v, c0), graph_source(w, c0)
    g = ClosedLoopGraph(v, actor, noise=src, days=DAYS, trajectory=False, fused=fused)
    twin = ClosedLoopGraph(w, actor_w, noise=src_w, days=DAYS, trajectory=True, fused=fused)
    assert g.step_nodes == twin.step_nodes == (1 if fused else 2 * T)
    assert g.obs_traj is None and tuple(g.noise_traj.shape) == (DAYS, T, E, A) and tuple(g.actions.shape) == (E, A)
    blocks = []
    for launch in range(2):
        g.launch()
        twin.launch()
        torch.cuda.synchronize()
        what = f"launch {launch}"
        nz = host(g.noise_traj)
        assert same(nz, host(twin.noise_traj)), what
        assert same(nz, src.host_fill(DAYS, counter=c0 + DAYS * launch)), what
        assert not np.array_equal(nz[0], nz[1])
        assert same(host(v.obs_d), host(twin.obs_traj)[-1, -1]), what
        assert same(host(v.reward_d), host(twin.reward_traj)[-1, -1]), what
        assert same(host(v.done_d), host(twin.done_traj)[-1, -1]), what
        assert same(host(g.actions), host(twin.action_traj)[-1, -1]), what
        assert_actions_are_the_host_actors(actor_w, host(twin.obs_traj), nz, host(twin.action_traj), what)
        blocks.append(nz)
    assert not np.array_equal(blocks[0], blocks[1])
    assert src.counter == c0 + 2 * DAYS and src_w.counter == c0 + 2 * DAYS
    for x in (g, twin, src, src_w, actor, actor_w, v, w):
        x.close()


@pytest.mark.parametrize("N,net,fused", GRAPHS, ids=GRAPH_IDS)
def test_steps_only_graph_with_a_source(N, net, fused):
    E, c0 = 70, 2 ** 32 - 1
    v, w = make_env(N, E), make_env(N, E)
    T, A = v.timesteps, v.act_dim
    actor, actor_w = relu_actor(v, net), relu_actor(w, net)
    src = graph_source(v, c0)
    v.reset_tensors()
    w.reset_tensors()
    with pytest.raises(_native.NativeError, match=r"days must be >= 1 \(more than one needs SNG_GRAPH_RESET\)"):
        ClosedLoopGraph(v, actor, noise=src, days=2, with_reset=False, trajectory=True, fused=fused)
    assert src.counter == c0   # nothing was drawn
    g = ClosedLoopGraph(v, actor, noise=src, days=1, with_reset=False, trajectory=True, fused=fused)
    assert g.step_nodes == (1 if fused else 2 * T) and tuple(g.noise_traj.shape) == (1, T, E, A)
    g.launch()
    torch.cuda.synchronize()
    nz, obs, act = host(g.noise_traj), host(g.obs_traj), host(g.action_traj)
    assert same(nz, src.host_fill(1, counter=c0)) and src.counter == c0 + 1
    assert_actions_are_the_host_actors(actor, obs, nz, act, "steps-only")
    assert (host(g.reward_traj) != 0).any() and host(g.done_traj)[0, -1].all()
    # the tensor path on a twin's same loaded day, given the block the source drew
    plain = ClosedLoopGraph(w, actor_w, noise=g.noise_traj[0].clone(), days=1, with_reset=False, trajectory=True,
                            fused=fused)
    assert plain.noise_source is None
    plain.launch()
    torch.cuda.synchronize()
    for name in ("obs_traj", "action_traj", "reward_traj", "done_traj"):
        assert same(host(getattr(plain, name)), host(getattr(g, name))), name
    for x in (plain, g, src, actor, actor_w, v, w):
        x.close()


@pytest.mark.parametrize("N,fused", [(4, False), (10, False), (4, True)], ids=["lean4", "wide10", "lean4-fused"])
def test_shards_of_a_closed_loop_equal_the_population(N, fused):
    """70 envs at env_offset 2^33 + 5 and their shards of 33 and 37 envs: every trajectory of a shard is the
    population's slice, the envs' own device days included."""
    c0, cut, total = 2 ** 32 - 1, 33, 70
    tensors = ("noise_traj", "obs_traj", "action_traj", "reward_traj", "done_traj")

    def run(E, offset):
        v = make_env(N, E, env_offset=offset)
        actor, src = relu_actor(v, NET), graph_source(v, c0)
        g = ClosedLoopGraph(v, actor, noise=src, days=DAYS, trajectory=True, fused=fused)
        assert g.step_nodes == (1 if fused else 2 * v.timesteps)
        g.launch()
        torch.cuda.synchronize()
        out = {k: host(getattr(g, k)) for k in tensors}
        assert same(out["noise_traj"], src.host_fill(DAYS, counter=c0)) and src.counter == c0 + DAYS
        assert_actions_are_the_host_actors(actor, out["obs_traj"], out["noise_traj"], out["action_traj"], f"E = {E}")
        for x in (g, src, actor, v):
            x.close()
        return out

    whole = run(total, BIG_OFFSET)
    assert not np.array_equal(whole["noise_traj"][:, :, :cut], whole["noise_traj"][:, :, cut:2 * cut])
    for E, offset, part in ((cut, BIG_OFFSET, slice(0, cut)), (total - cut, BIG_OFFSET + cut, slice(cut, total))):
        shard = run(E, offset)
        for k in tensors:
            assert same(shard[k], np.ascontiguousarray(whole[k][:, :, part])), f"shard at {offset - BIG_OFFSET}: {k}"


# ------------------------------------------------------- D. changes between launches of one captured graph
@pytest.mark.parametrize("fused", [False, True], ids=["nodes", "fused"])
def test_new_parameters_and_counter_between_launches(fused):
    N, E, c0, c2 = 4, 70, 7, 2 ** 35 + 1
    v = make_env(N, E)
    T, A = v.timesteps, v.act_dim
    actor = relu_actor(v, NET)
    mu1, scale1 = np.zeros(A, np.float32), np.linspace(0.2, 0.9, A).astype(np.float32)
    mu2, scale2 = np.linspace(0.3, -0.4, A).astype(np.float32), np.linspace(1.1, 0.05, A).astype(np.float32)
    src = ActionNoise(v, "gaussian", seed=5, mu=mu1, scale=scale1)
    src.counter = c0
    g = ClosedLoopGraph(v, actor, noise=src, days=DAYS, trajectory=True, fused=fused)
    assert g.step_nodes == (1 if fused else 2 * T)

    def launch(mu, scale, counter, what):
        g.launch()
        torch.cuda.synchronize()
        nz = host(g.noise_traj)
        assert same(nz, policy.noise_host_fill("gaussian", A, T, E, DAYS, 5, mu, scale, counter=counter)), what
        assert same(nz, src.host_fill(DAYS, counter=counter)), what
        assert_actions_are_the_host_actors(actor, host(g.obs_traj), nz, host(g.action_traj), what)
        assert src.counter == counter + DAYS, what
        return nz

    launch(mu1, scale1, c0, "as captured")
    src.set(mu2, scale2)
    second = launch(mu2, scale2, c0 + DAYS, "after set()")
    assert not np.array_equal(second, policy.noise_host_fill("gaussian", A, T, E, DAYS, 5, mu1, scale1, counter=c0 + DAYS))
    src.counter = c2
    third = launch(mu2, scale2, c2, "after a new counter")
    assert not np.array_equal(third, policy.noise_host_fill("gaussian", A, T, E, DAYS, 5, mu2, scale2,
                                                            counter=c0 + 2 * DAYS))
    for x in (g, src, actor, v):
        x.close()


@pytest.mark.parametrize("N,E,arch,net_head", [(8, 72, (64, 64), False), (4, 70, (33, 65), True)],
                         ids=["default-head-n8", "net-head-33x65-n4"])
def test_ppo_rollout_load_between_launches(N, E, arch, net_head):
    """Noise drawn with one log_std and log-probabilities taken with another is what this would catch."""
    v = make_env(N, E)
    T, A = v.timesteps, v.act_dim
    sd, sd2 = sb3_state_dict(v, arch, arch, 31), sb3_state_dict(v, arch, arch, 57)
    sd2["log_std"] = np.linspace(0.3, -1.4, A).astype(np.float32)
    assert not np.array_equal(sd["log_std"], sd2["log_std"])
    assert all(not np.array_equal(sd[k], sd2[k]) for k in policy.SB3_KEYS + policy.SB3_VALUE_KEYS)
    actor, head = MlpActor(v, "relu", net_arch=arch), PpoHead(v, "relu", net_arch=arch if net_head else None)
    src = ActionNoise(v, "gaussian", seed=12)
    ro = PpoRollout(v, actor, head, days=DAYS, gamma=0.98, gae_lambda=0.9, noise=src).load(sd)
    for launch, state in enumerate((sd, sd2)):
        if launch:
            ro.load(state)
        scale = np.exp(state["log_std"]).astype(np.float32)
        assert same(src.scale, scale) and same(head.log_std.astype(np.float32), state["log_std"])
        ro.launch()
        torch.cuda.synchronize()
        got = {k: host(getattr(ro, k)) for k in ("obs", "actions", "rewards", "dones", "noise") + NAMES}
        want = policy.noise_host_fill("gaussian", A, T, E, DAYS, 12, 0.0, scale, counter=DAYS * launch)
        assert same(got["noise"], want), f"launch {launch}: noise"
        for d in range(DAYS):
            finish = head.host_finish(got["obs"][d:d + 1], got["rewards"][d:d + 1], got["dones"][d:d + 1],
                                      got["noise"][d], 0.98, 0.9)
            for name, b in zip(NAMES, finish):
                np.testing.assert_array_equal(got[name][d:d + 1], b, err_msg=f"launch {launch} day {d}: {name}")
            for t in (0, T - 1):
                assert same(got["actions"][d, t], actor.host_actions(got["obs"][d, t], got["noise"][d, t])[0])
    old = policy.noise_host_fill("gaussian", A, T, E, DAYS, 12, 0.0, np.exp(sd["log_std"]).astype(np.float32), counter=DAYS)
    assert not np.array_equal(got["noise"], old) and src.counter == 2 * DAYS
    ro.close()
    v.close()


def test_fill_on_a_side_stream():
    N, E, c0 = 4, 70, 2 ** 32 - 1
    v = make_env(N, E)
    T, A = v.timesteps, v.act_dim
    for kind in ("gaussian", "ou"):
        src = make_source(v, kind, c0)
        first, second = (torch.empty((DAYS, T, E, A), dtype=torch.float32, device=v.device) for _ in range(2))
        torch.cuda.synchronize()   # set() uploaded on the current stream
        s = torch.cuda.Stream(device=v.device)
        assert s.cuda_stream != torch.cuda.current_stream(v.device).cuda_stream
        assert src.fill(DAYS, out=first, stream=s.cuda_stream) is first
        assert src.fill(DAYS, out=second, stream=s.cuda_stream) is second
        s.synchronize()
        assert same(host(first), src.host_fill(DAYS, counter=c0)), kind
        assert same(host(second), src.host_fill(DAYS, counter=c0 + DAYS)), kind
        assert src.counter == c0 + 2 * DAYS
        src.close()
    v.close()
