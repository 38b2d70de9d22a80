"""GPU: DDPG's gradient step where tests/test_gpu_ddpg_learn.py does not look -- a workspace reused by smaller batches,
the largest update, a resumed learner, gradients that are exactly zero, tau at both ends and a side stream.

Every comparison with the host model (csrc/sng_ddpg_learn_host.h) is by value (==) through the sibling file's
check_update, which gives the host the device's own a_pi; two learners are compared byte for byte.  The invariants of
the zero-gradient tests need no model and are asserted on the device's tensors directly.  The paths (csrc/
sng_ddpg_learn.cpp, sng_ddpg_learn.h) each test reaches:

A. ensure_work's `rows <= w.rows` branch: the partial-sum blocks were carved for more segments than an update now
   writes (learn_step_kernel must add nseg of them, not all), and the row arrays hold an earlier batch's rows behind
   the new M.  2 S + 37, 200, 1, 64, 33, S + 1, 7 rows (S = SNG_LEARNER_SEGMENT): three segments, then one, a single
   row, two whole tiles, one tile and a row, two segments again, less than a tile.
B. 64 segments: 65,536 rows (all 64 segment threads of learn_loss_kernel's last workgroup live, learn_step_kernel adds
   64 partials) and 65,535 (the last segment of 1,023 rows: an odd k and a partial 64-row loss tile), at the narrowest
   net and station, where the host model takes a quarter of a second.
C. sng_learner_set_state with non-zero moments and step, learn_step_kernel<false> rewriting all four packed images,
   and Adam's bias corrections at t = 2, 1000, 10^6 + 1 and 2^40 + 1 (beta^t underflows to 0 in the last two).
D. the epilogues and Adam at zero: LEARN_EPI_DTANH with 1 - a^2 == 0, LEARN_EPI_MASK with every unit dead, dq == 0,
   learn_adam on g == 0 with m = v = 0 (0 / (0 + eps)) and with moments, learn_polyak at tau = 1 and 0.
E. every launch of train() on a stream that is not torch's current one."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from policy_net_cases import net_f64, random_net_weights  # noqa: E402
from smart_nanogrid_gym import DdpgLearner, MlpActor, QCritic, _native, ddpg  # noqa: E402
from test_gpu_ddpg import OUT_SCALE, Q_SCALE, filled_ring, host, make_env  # noqa: E402
from test_gpu_ddpg_learn import HYPER, S, check_update, close, make_nets, same_state  # noqa: E402
from test_gpu_policy_net import SQUASH_FACTOR  # noqa: E402

DESCENDING = (2 * S + 37, 200, 1, 64, 33, S + 1, 7)
ACTOR_KEYS, CRITIC_KEYS = ddpg.net_keys("actor.mu"), ddpg.net_keys("critic.qf0")
ACTOR_T_KEYS, CRITIC_T_KEYS = ddpg.net_keys("actor_target.mu"), ddpg.net_keys("critic_target.qf0")


def four_weights(v, net, seed=0, actor_scale=OUT_SCALE):
    """make_nets' four random nets as arrays: dict(actor=, critic=, actor_target=, critic_target=)."""
    O, A = v.obs_dim, v.act_dim
    return dict(actor=random_net_weights(O, A, net, 11 + seed, actor_scale),
                critic=random_net_weights(O + A, 1, net, 21 + seed, Q_SCALE),
                actor_target=random_net_weights(O, A, net, 12 + seed, actor_scale),
                critic_target=random_net_weights(O + A, 1, net, 22 + seed, Q_SCALE))


def nets_of(v, net, w):
    """(actor, critic, actor_target, critic_target) loaded with four_weights' arrays."""
    return (MlpActor(v, "relu", net_arch=net, squash=True).load(w["actor"]), QCritic(v, net).load(w["critic"]),
            MlpActor(v, "relu", net_arch=net, squash=True).load(w["actor_target"]),
            QCritic(v, net).load(w["critic_target"]))


def copy_state(state):
    return dict(step=state["step"], **{part: {k: a.copy() for k, a in state[part].items()}
                                       for part in ("params", "exp_avg", "exp_avg_sq")})


def dev_bytes(tensors):
    return {k: (host(t).tobytes() if not isinstance(t, tuple) else b"".join(host(x).tobytes() for x in t))
            for k, t in tensors.items()}


def unchanged(learner, before, keys):
    return all(host(learner.params[k]).tobytes() == before["params"][k].tobytes() for k in keys)


def moved(learner, before, keys):
    return all((host(learner.params[k]) != before["params"][k]).any() for k in keys)


def zero(x):
    return not np.asarray(x).any()


def identical(a, b):
    """Two learners after the same steps: every master, target, moment, gradient, the step, the last q and losses."""
    assert a.step == b.step
    for name in ("params", "moments", "grads"):
        x, y = dev_bytes(getattr(a, name)), dev_bytes(getattr(b, name))
        assert x.keys() == y.keys()
        for k in x:
            assert x[k] == y[k], (name, k)
    la, lb = a.last, b.last
    for name in ("q", "dq", "q_pi", "a_pi", "y", "critic_loss", "actor_loss"):
        assert host(la[name]).tobytes() == host(lb[name]).tobytes(), name


# ------------------------------------------------------------------------------------- A. one workspace, any order
@pytest.mark.parametrize("N,net,batches", [(4, (33, 65), DESCENDING), (1, (8, 8), DESCENDING[:3])],
                         ids=["n4-33x65", "n1-8x8"])
def test_smaller_batches_reuse_the_largest_workspace(N, net, batches):
    """Path A.  Each update in full against the host model; the workspace is allocated by the first update and is the
    same block after the last (learner.last's q is its second array)."""
    v = make_env(N)
    ring, _ = filled_ring(v, seed=5)
    nets = make_nets(v, net)
    actor_t, critic_t = nets[2], nets[3]
    learner = DdpgLearner(v, *nets, **HYPER)
    state = learner.host_state()
    q_at = []
    for B in batches:
        s = ring.sample(B)
        y, _ = critic_t.targets(actor_t, s, HYPER["gamma"])
        want = check_update(learner, state, s, y, f"N={N} {net} B={B}")
        last = learner.last
        assert [tuple(last[k].shape) for k in ("q", "dq", "q_pi", "a_pi", "y")] == [(B,)] * 3 + [(B, v.act_dim), (B, 1)]
        assert np.isfinite(want["critic_loss"]) and want["critic_loss"] > 0
        q_at.append(last["q"].data_ptr())
    assert len(set(q_at)) == 1, q_at   # one allocation: no update after the first grew it
    assert learner.step == state["step"] == len(batches)
    close(learner, *nets, ring, v)


# ----------------------------------------------------------------------------------------------- B. 64 segments
def test_the_largest_update_and_a_small_one_behind_it():
    """Path B: LEARNER_MAX_ROWS - 1 rows, then LEARNER_MAX_ROWS, then 64 rows in the 64-segment workspace."""
    N, net = 1, (8, 8)
    M = ddpg.LEARNER_MAX_ROWS
    assert M == 64 * S
    v = make_env(N)
    ring, _ = filled_ring(v, seed=5)
    nets = make_nets(v, net)
    actor_t, critic_t = nets[2], nets[3]
    learner = DdpgLearner(v, *nets, **HYPER)
    state = learner.host_state()
    for B in (M - 1, M, 64):
        s = ring.sample(B)
        y, _ = critic_t.targets(actor_t, s, HYPER["gamma"])
        want = check_update(learner, state, s, y, f"B={B}")
        assert learner.last["q"].shape == (B,) and np.isfinite(want["critic_loss"]) and want["critic_loss"] > 0
        assert all(g.any() for g in want["grads"].values())
    assert learner.step == 3
    close(learner, *nets, ring, v)


# ------------------------------------------------------------------------------------------------------ C. resume
def test_a_resumed_learner_continues_bit_for_bit():
    """Path C.  Learner A takes three train steps; its host_state() goes into learner B, made from four fresh handles
    with other weights in a fresh env (the ring's trajectory is made of the env's own reset observations), whose ring
    has A's contents, seed and counter.  Straight after load_state B's four handles run the state's weights -- critic
    and target critic == their host models, both actors within SQUASH_FACTOR of the host model's distance from
    float64 (measured on an MI355X, d_dev / d_ref: actor 0.987, actor_target 0.841) -- and after two more steps on
    each side everything is byte-identical."""
    N, net, B = 10, (33, 65), 200
    v, w = make_env(N), make_env(N)
    ring_a, _ = filled_ring(v, seed=5)
    ring_b, _ = filled_ring(w, seed=5)
    assert all(host(getattr(ring_a, n)).tobytes() == host(getattr(ring_b, n)).tobytes()
               for n in ("obs", "actions", "reward", "done"))
    nets_a, nets_b = make_nets(v, net), make_nets(w, net, seed=50)
    a = DdpgLearner(v, *nets_a, **HYPER).train(ring_a, B, 3)
    state = a.host_state()
    assert state["step"] == 3 and all(m.any() for m in state["exp_avg"].values())
    b = DdpgLearner(w, *nets_b, **HYPER)
    assert any(host(a.params[k]).tobytes() != host(b.params[k]).tobytes() for k in a.params)
    assert b.load_state(state) is b and b.step == 3
    same_state(b.host_state(), state, "after load_state")
    ring_b.counter = ring_a.counter
    # the four images, before any update
    actor, critic, actor_t, critic_t = nets_b
    s = ring_b.sample(B)
    ring_b.counter = ring_a.counter
    p = state["params"]
    q = host(critic.q(s.observations, s.actions))
    np.testing.assert_array_equal(q, ddpg.host_q(s.observations, s.actions, [p[k] for k in CRITIC_KEYS], net))
    y, na = (host(x).copy() for x in critic_t.targets(actor_t, s, HYPER["gamma"]))
    want_y = ddpg.host_targets(s.next_observations, s.rewards, s.dones, [p[k] for k in CRITIC_T_KEYS],
                               HYPER["gamma"], net, next_actions=na)[0]
    np.testing.assert_array_equal(y[:, 0], want_y)
    obs = host(s.observations)
    for name, handle, keys in (("actor", actor, ACTOR_KEYS), ("actor_target", actor_t, ACTOR_T_KEYS)):
        weights = [p[k] for k in keys]
        dev = torch.empty((B, w.act_dim), dtype=torch.float32, device=w.device)
        _native.check(_native.lib().sng_policy_actions_rows(handle._p, B, s.observations.data_ptr(), None,
                                                            dev.data_ptr(), None, None), w._h)
        torch.cuda.synchronize()
        ref = net_f64(obs, weights, "relu", squash=True)
        handle.weights = weights   # what load_state put on the device, for the handle's host model
        d_ref = np.abs(handle.host_actions(obs)[0].astype(np.float64) - ref).max()
        d_dev = np.abs(host(dev).astype(np.float64) - ref).max()
        print(f"resumed {name}: d_ref {d_ref:.4e}, d_dev {d_dev:.4e}, ratio {d_dev / d_ref:.3f}, factor {SQUASH_FACTOR}")
        assert d_dev <= SQUASH_FACTOR * d_ref
    # two more steps on each side
    a.train(ring_a, B, 2)
    b.train(ring_b, B, 2)
    torch.cuda.synchronize()
    assert a.step == b.step == 5 and ring_a.counter == ring_b.counter
    identical(a, b)
    same_state(b.host_state(), a.host_state(), "after two more steps")
    close(a, b, *nets_a, *nets_b, ring_a, ring_b, v, w)


def random_moments(state, seed):
    """exp_avg ~ N(0, 1e-2) and exp_avg_sq ~ U(0, 1e-3) (a variance of 1e-2: a standard deviation of 0.1) for the
    twelve trained tensors of `state`."""
    rng = np.random.default_rng(seed)
    m = {k: rng.normal(0.0, 0.1, a.shape).astype(np.float32) for k, a in state["exp_avg"].items()}
    vv = {k: rng.uniform(0.0, 1e-3, a.shape).astype(np.float32) for k, a in state["exp_avg_sq"].items()}
    return m, vv


def test_hand_made_states_and_late_steps_and_refused_states():
    """Path C from states no learner produced: random moments and step = 1, 999, 10^6 and 2^40 through load_state, one
    update each against the host model, which stays finite at all four.  A NaN moment and a negative step are refused
    and leave the learner as it was."""
    N, net, B = 4, (33, 65), 64
    v = make_env(N)
    ring, _ = filled_ring(v, seed=5)
    nets = make_nets(v, net)
    actor_t, critic_t = nets[2], nets[3]
    learner = DdpgLearner(v, *nets, **HYPER)
    for i, step in enumerate((1, 999, 10 ** 6, 2 ** 40)):
        sd = {k: a for net_w, prefix in zip(four_weights(v, net, seed=60 + i).values(), ddpg.LEARNER_NETS.values())
              for k, a in zip(ddpg.net_keys(prefix), net_w)}
        blank = ddpg.learner_host_state(sd, v.obs_dim, v.act_dim, net, net)
        m, vv = random_moments(blank, 70 + i)
        state = ddpg.learner_host_state(sd, v.obs_dim, v.act_dim, net, net, exp_avg=m, exp_avg_sq=vv, step=step)
        assert state["step"] == step and all(state["exp_avg"][k].tobytes() == m[k].tobytes() for k in m)
        learner.load_state(state)
        assert learner.step == step
        same_state(learner.host_state(), state, f"loaded step {step}")
        before = copy_state(state)
        s = ring.sample(B)
        y, _ = critic_t.targets(actor_t, s, HYPER["gamma"])
        want = check_update(learner, state, s, y, f"step {step}")
        assert learner.step == state["step"] == step + 1
        assert all(np.isfinite(a).all() for part in ("params", "exp_avg", "exp_avg_sq") for a in state[part].values())
        assert np.isfinite(want["critic_loss"]) and moved(learner, before, ACTOR_KEYS + CRITIC_KEYS)
    # refusals
    good = learner.host_state()
    bad = copy_state(good)
    bad["exp_avg_sq"]["critic.qf0.2.weight"].flat[-1] = np.nan
    with pytest.raises(_native.NativeError, match=r"libsng error -1.*non-finite"):
        learner.load_state(bad)
    bad = copy_state(good)
    bad["exp_avg"]["actor.mu.4.bias"][0] = np.inf
    with pytest.raises(_native.NativeError, match=r"libsng error -1.*non-finite"):
        learner.load_state(bad)
    bad = copy_state(good)
    bad["step"] = -1
    with pytest.raises(_native.NativeError, match=r"libsng error -1.*step must be >= 0"):
        learner.load_state(bad)
    assert learner.step == good["step"] == 2 ** 40 + 1
    same_state(learner.host_state(), good, "after the refusals")
    close(learner, *nets, ring, v)


# ------------------------------------------------------------------------------------------- D. gradients of zero
def zero_gradient_setup(w=None, hyper=HYPER, actor_scale=OUT_SCALE):
    """N = 4, (8, 8), 64 rows: (v, ring, nets, learner, state, sample, y) with `w` (four_weights) changed by the caller."""
    net = (8, 8)
    v = make_env(4)
    ring, _ = filled_ring(v, seed=5)
    weights = four_weights(v, net, actor_scale=actor_scale)
    if w:
        w(weights)
    nets = nets_of(v, net, weights)
    learner = DdpgLearner(v, *nets, **hyper)
    s = ring.sample(64)
    y = nets[3].targets(nets[2], s, HYPER["gamma"])[0].clone()
    return v, ring, weights, nets, learner, learner.host_state(), s, y


@pytest.mark.parametrize("columns", ["all", "even"])
def test_a_saturated_actor_passes_no_gradient_and_stays(columns):
    """Path D, LEARN_EPI_DTANH at 1 - a^2 == 0.  b3 = +-64 with alternating signs on the saturated columns and a last
    layer of scale 1 (|w3 h2| stays far below 48), so that every |mean| >= 16 in float64 and tanhf gives exactly +-1.
    "all": the six actor gradients are zero, Adam on g == 0 with m = v = 0 leaves the masters bit for bit and the
    moments zero, the target still moves towards the unchanged actor, and the critic moves.  "even": only those rows of
    the last layer's weight gradient and entries of its bias gradient are zero."""
    def saturate(weights):
        b3 = weights["actor"][5]
        cols = np.arange(b3.size)[::1 if columns == "all" else 2]
        b3[cols] = 64.0 * np.where(np.arange(cols.size) % 2 == 0, 1.0, -1.0)
    v, ring, weights, nets, learner, state, s, y = zero_gradient_setup(saturate, actor_scale=1.0)
    A = v.act_dim
    cols = np.arange(A)[::1 if columns == "all" else 2]
    rest = np.setdiff1d(np.arange(A), cols)
    sign = np.where(np.arange(cols.size) % 2 == 0, 1.0, -1.0).astype(np.float32)
    mean = net_f64(host(s.observations), weights["actor"], "relu")
    assert (np.abs(mean[:, cols]) >= 16).all() and (np.sign(mean[:, cols]) == sign).all()
    before = copy_state(state)
    want = check_update(learner, state, s, y, f"saturated {columns}")
    a_pi = host(learner.last["a_pi"])
    assert (a_pi[:, cols] == sign).all()                       # exactly +-1
    assert (np.abs(a_pi[:, rest]) < 1).all()
    grads = {k: host(learner.grads[k]) for k in ACTOR_KEYS}
    assert zero(grads["actor.mu.4.weight"][cols]) and zero(grads["actor.mu.4.bias"][cols])
    assert moved(learner, before, CRITIC_KEYS + CRITIC_T_KEYS + ACTOR_T_KEYS)
    assert all(want["grads"][k].any() for k in CRITIC_KEYS)
    if columns == "all":
        assert all(zero(g) for g in grads.values()) and all(zero(want["grads"][k]) for k in ACTOR_KEYS)
        assert unchanged(learner, before, ACTOR_KEYS)
        assert all(zero(host(m)) and zero(host(vv)) for k, (m, vv) in learner.moments.items() if k in ACTOR_KEYS)
    else:
        assert grads["actor.mu.4.weight"][rest].any(axis=1).all() and (grads["actor.mu.4.bias"][rest] != 0).all()
        assert all(grads[k].any() for k in ACTOR_KEYS) and moved(learner, before, ACTOR_KEYS)
    close(learner, *nets, ring, v)


def test_a_dead_critic_layer_stops_both_backward_passes():
    """Path D, LEARN_EPI_MASK with no unit alive.  Critic b1 = -100: h1 == 0 for every row, so the gradients of the
    first layer and of the second layer's weights are zero, nothing reaches the action columns and the six actor
    gradients are zero; those masters stay bit for bit.  The second layer's bias and the last layer still learn (h2 =
    relu(b2)), as the host model says."""
    def kill(weights):
        weights["critic"][1][:] = -100.0
    v, ring, weights, nets, learner, state, s, y = zero_gradient_setup(kill)
    w1, b1, _, b2 = weights["critic"][:4]
    assert (b2 > 0).any()
    x = np.concatenate([host(s.observations), host(s.actions)], axis=1).astype(np.float64)
    assert (x @ w1.astype(np.float64).T + b1 < -50).all()
    before = copy_state(state)
    want = check_update(learner, state, s, y, "dead critic layer")
    x[:, v.obs_dim:] = host(learner.last["a_pi"])
    assert (x @ w1.astype(np.float64).T + b1 < -50).all()
    dead = ["critic.qf0.0.weight", "critic.qf0.0.bias", "critic.qf0.2.weight"] + ACTOR_KEYS
    alive = ["critic.qf0.2.bias", "critic.qf0.4.weight", "critic.qf0.4.bias"]
    assert all(zero(host(learner.grads[k])) and zero(want["grads"][k]) for k in dead)
    assert unchanged(learner, before, dead)
    assert all(zero(host(m)) and zero(host(vv)) for k, (m, vv) in learner.moments.items() if k in dead)
    assert all(host(learner.grads[k]).any() for k in alive) and moved(learner, before, alive)
    assert (host(learner.grads["critic.qf0.2.bias"]) != 0).tolist() == (b2 > 0).tolist()
    assert len(np.unique(host(learner.last["q"]))) == 1   # Q is the same constant for every row
    close(learner, *nets, ring, v)


def test_targets_equal_to_q_leave_the_critic_to_its_moments():
    """Path D, dq == 0.  y = critic.q(s, a) on the current weights: dq and the critic's loss are exactly zero and so are
    its six gradients.  On a first step the critic's masters stay bit for bit (m = v = 0); after two ordinary steps
    the same situation moves them by the moments alone, as the host model says."""
    v, ring, weights, nets, learner, state, s, _ = zero_gradient_setup()
    actor, critic, actor_t, critic_t = nets

    def settled(what):
        before = copy_state(state)
        y = critic.q(s.observations, s.actions).clone()
        want = check_update(learner, state, s, y, what)
        last = learner.last
        assert zero(host(last["dq"])) and float(host(last["critic_loss"])) == 0.0 == float(want["critic_loss"])
        assert np.array_equal(host(last["q"]), host(y))
        assert all(zero(host(learner.grads[k])) and zero(want["grads"][k]) for k in CRITIC_KEYS)
        assert all(want["grads"][k].any() for k in ACTOR_KEYS)
        return before
    before = settled("q == y, first step")
    assert unchanged(learner, before, CRITIC_KEYS) and moved(learner, before, ACTOR_KEYS + CRITIC_T_KEYS)
    assert all(zero(host(m)) and zero(host(vv)) for k, (m, vv) in learner.moments.items() if k in CRITIC_KEYS)
    for i in range(2):
        s2 = ring.sample(64)
        check_update(learner, state, s2, critic_t.targets(actor_t, s2, HYPER["gamma"])[0], f"ordinary step {i}")
    assert s2.observations.data_ptr() == s.observations.data_ptr()   # the ring's 64-row sample, drawn anew: use it
    before = settled("q == y, with moments")
    assert moved(learner, before, CRITIC_KEYS)
    assert learner.step == 4
    close(learner, *nets, ring, v)


def test_tau_at_both_ends():
    """Path D, learn_polyak at tau = 1 (the targets are their masters, bit for bit) and tau = 0 (the targets stay bit
    for bit), each against the host model; the masters and gradients are those of a tau = 0.005 learner."""
    net = (8, 8)
    v = make_env(4)
    ring, _ = filled_ring(v, seed=5)
    weights = four_weights(v, net)
    s = ring.sample(64)
    learners = {}
    for tau in (0.005, 1.0, 0.0):
        nets = nets_of(v, net, weights)
        learner = DdpgLearner(v, *nets, **dict(HYPER, tau=tau))
        state = learner.host_state()
        before = copy_state(state)
        if not learners:
            y = nets[3].targets(nets[2], s, HYPER["gamma"])[0].clone()
        check_update(learner, state, s, y, f"tau {tau}")
        learners[tau] = (learner, nets, before)
    ref = learners[0.005][0]
    for tau in (1.0, 0.0):
        learner, _, before = learners[tau]
        for k in ACTOR_KEYS + CRITIC_KEYS:
            assert host(learner.params[k]).tobytes() == host(ref.params[k]).tobytes(), (tau, k)
            assert host(learner.grads[k]).tobytes() == host(ref.grads[k]).tobytes(), (tau, k)
        for k, kt in zip(ACTOR_KEYS + CRITIC_KEYS, ACTOR_T_KEYS + CRITIC_T_KEYS):
            got = host(learner.params[kt]).tobytes()
            assert got == (host(learner.params[k]).tobytes() if tau == 1.0 else before["params"][kt].tobytes()), (tau, kt)
            assert got != host(ref.params[kt]).tobytes(), (tau, kt)
    assert moved(ref, learners[0.005][2], ACTOR_T_KEYS + CRITIC_T_KEYS)
    for learner, nets, _ in learners.values():
        close(learner, *nets)
    close(ring, v)


# ---------------------------------------------------------------------------------------------- E. a side stream
def test_train_on_a_side_stream_equals_the_default_stream():
    """Path E: two train steps on a stream of the test's own, then its synchronize(), against a twin learner in a fresh
    env with the same seeds on torch's current stream."""
    N, net, B = 4, (33, 65), 64
    v, w = make_env(N), make_env(N)
    ring, _ = filled_ring(v, seed=5)
    ring2, _ = filled_ring(w, seed=5)
    nets, nets2 = make_nets(v, net), make_nets(w, net)
    learner, twin = DdpgLearner(v, *nets, **HYPER), DdpgLearner(w, *nets2, **HYPER)
    torch.cuda.synchronize()   # the pushes and the loads ran on the current stream
    side = torch.cuda.Stream(device=v.device)
    assert side.cuda_stream != torch.cuda.current_stream(v.device).cuda_stream
    assert learner.train(ring, B, 2, stream=side.cuda_stream) is learner
    side.synchronize()
    twin.train(ring2, B, 2)
    torch.cuda.synchronize()
    assert learner.step == 2 and ring.counter == ring2.counter == 2
    identical(learner, twin)
    close(learner, twin, *nets, *nets2, ring, ring2, v, w)
