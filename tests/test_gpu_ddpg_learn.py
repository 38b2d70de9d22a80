"""GPU: DDPG's gradient step on the device (include/sng.h: sng_learner_*; smart_nanogrid_gym/ddpg.py: DdpgLearner).

E = 70 and test_gpu_ddpg's ring of three days.  The host model (csrc/sng_ddpg_learn_host.h) takes the device's own
a_pi = tanhf(mean); everything else of an update is float32 arithmetic in a fixed order on both sides, so q, dq, the
twelve gradients, the masters and moments behind Adam, the targets behind polyak and both losses are compared by value
(==).  Batches of 1, 64 and 200 rows: one partial 32-row MFMA tile (and a weight gradient's chain of a single, odd
k), two whole tiles, and six whole tiles with one of 8 rows, over more than one workgroup of four tiles;
SNG_LEARNER_SEGMENT + 1 and 2 SNG_LEARNER_SEGMENT + 37 rows: two and three segments of the weight gradients' chains,
the last of one row and of an odd 37.  The nets' widths 8, 33, 65, 300 and 400 and the input widths 11 to 160 are no
multiples of the tile or of the MFMA's two k's."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from policy_net_cases import net_f64, random_net_weights  # noqa: E402
from smart_nanogrid_gym import ClosedLoopGraph, DdpgLearner, MlpActor, QCritic, _native, ddpg  # noqa: E402
from test_gpu_ddpg import OUT_SCALE, Q_SCALE, filled_ring, host, make_env  # noqa: E402
from test_gpu_policy_net import SQUASH_FACTOR  # noqa: E402

S = ddpg.LEARNER_SEGMENT
NETS = [(8, 8), (33, 65), (400, 300)]
BATCHES = (1, 64, 200)
CASES = [(N, net) for N in (1, 10) for net in NETS] + [(50, (33, 65))]
HYPER = dict(actor_lr=1e-3, critic_lr=2e-3, tau=0.005, gamma=0.99)


def make_nets(v, net, seed=0):
    """(actor, critic, actor_target, critic_target) of `net`, loaded with four different random nets."""
    O, A = v.obs_dim, v.act_dim
    actor = MlpActor(v, "relu", net_arch=net, squash=True).load(random_net_weights(O, A, net, 11 + seed, OUT_SCALE))
    actor_t = MlpActor(v, "relu", net_arch=net, squash=True).load(random_net_weights(O, A, net, 12 + seed, OUT_SCALE))
    critic = QCritic(v, net).load(random_net_weights(O + A, 1, net, 21 + seed, Q_SCALE))
    critic_t = QCritic(v, net).load(random_net_weights(O + A, 1, net, 22 + seed, Q_SCALE))
    return actor, critic, actor_t, critic_t


def close(*xs):
    for x in xs:
        x.close()


def same_state(got, want, what):
    assert got["step"] == want["step"], what
    for part in ("params", "exp_avg", "exp_avg_sq"):
        assert got[part].keys() == want[part].keys()
        for k in want[part]:
            np.testing.assert_array_equal(got[part][k], want[part][k], err_msg=f"{what} {part} {k}")


def check_update(learner, state, s, y, what):
    """One device update against the host model from `state` (which it advances) with the device's a_pi."""
    learner.update(s, y)
    last = learner.last
    torch.cuda.synchronize()
    want = learner.host_update(state, host(s.observations), host(s.actions), host(y), host(last["a_pi"]))
    for name in ("q", "dq", "q_pi", "critic_loss", "actor_loss"):
        np.testing.assert_array_equal(host(last[name]), want[name], err_msg=f"{what} {name}")
    assert set(learner.grads) == set(want["grads"]) and len(want["grads"]) == 12
    for k, g in want["grads"].items():
        np.testing.assert_array_equal(host(learner.grads[k]), g, err_msg=f"{what} grad {k}")
    same_state(learner.host_state(), state, what)
    for k, p in learner.params.items():   # the device tensors are the arrays get_state reads
        np.testing.assert_array_equal(host(p), state["params"][k], err_msg=f"{what} params {k}")
    for k, (m, vv) in learner.moments.items():
        assert np.array_equal(host(m), state["exp_avg"][k]) and np.array_equal(host(vv), state["exp_avg_sq"][k]), (what, k)
    return want


@pytest.mark.parametrize("N,net", CASES, ids=[f"n{N}-{a}x{b}" for N, (a, b) in CASES])
def test_one_update_equals_the_host_model(N, net):
    v = make_env(N)
    ring, _ = filled_ring(v, seed=5)
    nets = make_nets(v, net)
    actor, critic, actor_t, critic_t = nets
    learner = DdpgLearner(v, *nets, **HYPER)
    state = learner.host_state()
    assert state["step"] == 0 and all(not m.any() for m in state["exp_avg"].values())
    for B in BATCHES + ((S + 1, 2 * S + 37) if net == (8, 8) else ()):
        before = {k: a.copy() for k, a in state["params"].items()}
        s = ring.sample(B)
        y, _ = critic_t.targets(actor_t, s, HYPER["gamma"])
        want = check_update(learner, state, s, y, f"N={N} {net} B={B}")
        # not a comparison of zeros: the gradients are there, every tensor moved and so did its target
        nonzero = {k: float((g != 0).mean()) for k, g in want["grads"].items()}
        assert B < 64 or np.mean(list(nonzero.values())) >= 0.25, nonzero
        for k, a in state["params"].items():
            assert (a != before[k]).any(), (B, k)
        assert np.isfinite(want["critic_loss"]) and want["critic_loss"] > 0 and np.isfinite(want["actor_loss"])
    assert learner.step == state["step"] == (5 if net == (8, 8) else 3)
    assert actor.weights is None and critic_t.weights is None   # stale until pull()
    with pytest.raises(RuntimeError, match="load"):
        critic.host_q(s.observations, s.actions)
    close(learner, *nets, ring, v)


def test_train_steps_equal_the_host_model_in_lockstep_and_repeat():
    """Three train steps (sample -> targets -> update) against the host model on the same samples, drawn by the
    sampling law's host model from the ring's numpy mirror; a second learner with the same inputs, run by one
    train(ring, B, 3), is byte-identical in every master, moment and target."""
    N, net, B = 4, (33, 65), 200
    v = make_env(N)
    ring, mirror = filled_ring(v, seed=5)
    nets = make_nets(v, net)
    actor, critic, actor_t, critic_t = nets
    learner = DdpgLearner(v, *nets, **HYPER)
    state = learner.host_state()
    for step in range(3):
        idx = ring.host_indices(B)
        obs, act, nobs, done, rew = mirror.gather(idx)
        target_w = [state["params"][k] for k in ddpg.net_keys("critic_target.qf0")]
        learner.train(ring, B, 1)
        last = learner.last
        torch.cuda.synchronize()
        na = host(critic_t._outputs(B)[2])   # the device's next actions behind y
        y = ddpg.host_targets(nobs, rew, done, target_w, HYPER["gamma"], net, next_actions=na)[0]
        np.testing.assert_array_equal(host(last["y"])[:, 0], y, err_msg=f"step {step} y")
        want = learner.host_update(state, obs, act, y, host(last["a_pi"]))
        for name in ("q", "dq", "q_pi", "critic_loss", "actor_loss"):
            np.testing.assert_array_equal(host(last[name]), want[name], err_msg=f"step {step} {name}")
        same_state(learner.host_state(), state, f"step {step}")
    assert learner.step == 3 and ring.counter == 3
    # the same three steps in one call, from a fresh env with the same seeds (the ring's trajectory is made of the
    # env's own reset observations)
    w = make_env(N)
    ring2, _ = filled_ring(w, seed=5)
    assert host(ring2.obs).tobytes() == host(ring.obs).tobytes()
    nets2 = make_nets(w, net)
    learner2 = DdpgLearner(w, *nets2, **HYPER).train(ring2, B, 3)
    torch.cuda.synchronize()
    for k in learner.params:
        assert host(learner.params[k]).tobytes() == host(learner2.params[k]).tobytes(), k
    for k in learner.moments:
        for a, b in zip(learner.moments[k], learner2.moments[k]):
            assert host(a).tobytes() == host(b).tobytes(), k
    close(learner, learner2, *nets, *nets2, ring, ring2, v, w)


def test_the_handles_run_the_new_weights():
    """q of the update is critic.q on the weights before it; after the update and pull() the four handles' kernels
    run the learner's weights: critic.q and critic_target.targets equal their host models on the pulled weights, the
    actors their host model up to tanhf.  Measured on an MI355X, d_dev / d_ref of the actors: see the printed line."""
    N, net, B = 10, (400, 300), 200
    v = make_env(N)
    ring, _ = filled_ring(v, seed=5)
    nets = make_nets(v, net)
    actor, critic, actor_t, critic_t = nets
    learner = DdpgLearner(v, *nets, **HYPER)
    s = ring.sample(B)
    q_before = host(critic.q(s.observations, s.actions)).copy()
    y_before = host(critic_t.targets(actor_t, s)[0]).copy()
    learner.update(s)
    np.testing.assert_array_equal(host(learner.last["q"]), q_before)
    np.testing.assert_array_equal(host(learner.last["y"]), y_before)
    sd = learner.pull()
    assert sorted(sd) == sorted(k for p in ddpg.LEARNER_NETS.values() for k in ddpg.net_keys(p))
    q_after = host(critic.q(s.observations, s.actions))
    assert (q_after != q_before).mean() > 0.5
    np.testing.assert_array_equal(q_after, critic.host_q(s.observations, s.actions))
    y, na = (host(x).copy() for x in critic_t.targets(actor_t, s))
    assert (y != y_before).any()
    np.testing.assert_array_equal(y[:, 0], critic_t.host_targets(s, next_actions=na)[0])
    obs = host(s.observations)
    for name, a in (("actor", actor), ("actor_target", actor_t)):
        dev = torch.empty((B, v.act_dim), dtype=torch.float32, device=v.device)
        _native.check(_native.lib().sng_policy_actions_rows(a._p, B, s.observations.data_ptr(), None, dev.data_ptr(),
                                                            None, None), v._h)
        ref = net_f64(obs, a.weights, "relu", squash=True)
        d_ref = np.abs(a.host_actions(obs)[0].astype(np.float64) - ref).max()
        d_dev = np.abs(host(dev).astype(np.float64) - ref).max()
        print(f"{name}: d_ref {d_ref:.4e}, d_dev {d_dev:.4e}, ratio {d_dev / d_ref:.3f}, factor {SQUASH_FACTOR}")
        assert d_dev <= SQUASH_FACTOR * d_ref
    close(learner, *nets, ring, v)


def test_a_captured_graph_acts_with_the_updated_actor():
    N, net, B = 4, (33, 65), 64
    v = make_env(N)
    ring, _ = filled_ring(v, seed=5)
    nets = make_nets(v, net)
    actor = nets[0]
    learner = DdpgLearner(v, *nets, **HYPER)
    g = ClosedLoopGraph(v, actor, days=1, trajectory=True)
    g.launch()
    torch.cuda.synchronize()
    old_w = [w.copy() for w in actor.weights]
    learner.train(ring, B, 3)
    g.launch()
    learner.pull()
    obs, act = host(g.obs_traj)[0], host(g.action_traj)[0]
    d_ref = d_dev = d_old = 0.0
    for t in range(v.timesteps):
        ref = net_f64(obs[t], actor.weights, "relu", squash=True)
        d_ref = max(d_ref, np.abs(actor.host_actions(obs[t])[0].astype(np.float64) - ref).max())
        d_dev = max(d_dev, np.abs(act[t].astype(np.float64) - ref).max())
        d_old = max(d_old, np.abs(act[t].astype(np.float64) - net_f64(obs[t], old_w, "relu", squash=True)).max())
    print(f"graph after update: d_ref {d_ref:.4e}, d_dev {d_dev:.4e}, against the old weights {d_old:.4e}")
    assert d_dev <= SQUASH_FACTOR * d_ref and d_old > 100 * d_ref
    close(g, learner, *nets, ring, v)


def test_refusals_on_the_device_path():
    v, other = make_env(4), make_env(4)
    ring, _ = filled_ring(v, seed=5)
    net = (33, 65)
    nets = make_nets(v, net)
    actor, critic, actor_t, critic_t = nets
    w_a = random_net_weights(v.obs_dim, v.act_dim, net, 1, OUT_SCALE)
    w_c = random_net_weights(v.obs_dim + v.act_dim, 1, net, 2, Q_SCALE)
    lib = _native.lib()

    def create(a, at, c, ct, **kw):
        h = ctypes.c_void_p()
        spec = ddpg._learner_spec(**{**dict(actor_lr=1e-3, critic_lr=1e-3, tau=0.005, betas=(0.9, 0.999), eps=1e-8), **kw})
        rc = lib.sng_learner_create(v._h, a, at, c, ct, ctypes.byref(spec), ctypes.byref(h))
        assert h.value is None or rc == 0
        return rc, lib.sng_last_error(v._h)
    tanh_actor = MlpActor(v, "tanh", net_arch=net, squash=True).load(w_a)
    mean_actor = MlpActor(v, "relu", net_arch=net).load(w_a)
    ppo_actor = MlpActor(v, "relu").load(random_net_weights(v.obs_dim, v.act_dim, (64, 64), 1))
    wide_actor = MlpActor(v, "relu", net_arch=(33, 64), squash=True)
    tanh_critic = QCritic(v, net, "tanh").load(w_c)
    wide_critic = QCritic(v, (32, 65))
    foreign = MlpActor(other, "relu", net_arch=net, squash=True).load(w_a)
    P = [x._p for x in nets]
    assert create(tanh_actor._p, tanh_actor._p, P[1], P[3])[0] == -1            # a net is its own target
    rc, why = create(tanh_actor._p, P[2], P[1], P[3])
    assert rc == -2 and b"relu" in why
    rc, why = create(P[0], P[2], tanh_critic._p, P[3])
    assert rc == -2 and b"relu" in why
    rc, why = create(mean_actor._p, P[2], P[1], P[3])
    assert rc == -2 and b"squash" in why
    rc, why = create(ppo_actor._p, P[2], P[1], P[3])
    assert rc == -2 and b"sng_policy_create_net" in why
    rc, why = create(P[0], wide_actor._p, P[1], P[3])
    assert rc == -1 and b"differ" in why
    rc, why = create(P[0], P[2], P[1], wide_critic._p)
    assert rc == -1 and b"differ" in why
    rc, why = create(foreign._p, P[2], P[1], P[3])
    assert rc == -1 and b"another env" in why
    assert create(None, P[2], P[1], P[3])[0] == -1 and create(P[0], P[2], P[1], None)[0] == -1
    for kw in (dict(tau=1.5), dict(tau=-0.1), dict(actor_lr=0.0), dict(critic_lr=-1.0), dict(eps=float("nan")),
               dict(actor_lr=float("inf")), dict(betas=(1.0, 0.999))):
        assert create(P[0], P[2], P[1], P[3], **kw)[0] == -1, kw
    with pytest.raises(ValueError, match="another env batch"):
        DdpgLearner(v, foreign, critic, actor_t, critic_t)
    with pytest.raises(ValueError, match="load"):
        DdpgLearner(v, actor, wide_critic, actor_t, critic_t)
    with pytest.raises(ValueError, match="must be a QCritic"):
        DdpgLearner(v, actor, actor, actor_t, critic_t)
    learner = DdpgLearner(v, *nets)
    with pytest.raises(_native.NativeError, match="no update yet"):
        learner.last
    s = ring.sample(8)
    p = s.observations.data_ptr()
    assert lib.sng_learner_update(learner._p, 0, p, p, p, None) == -1
    assert lib.sng_learner_update(learner._p, ddpg.LEARNER_MAX_ROWS + 1, p, p, p, None) == -1
    assert b"65536" in lib.sng_last_error(v._h)
    assert lib.sng_learner_update(learner._p, 8, p, None, p, None) == -1
    assert lib.sng_learner_update(None, 8, p, p, p, None) == -1
    with pytest.raises(ValueError, match="y must be"):
        learner.update(s, torch.zeros(7, device=v.device))
    with pytest.raises(ValueError, match="samples.actions must be"):
        learner.update(s._replace(actions=s.observations))
    assert learner.step == 0
    actor_t.close()
    with pytest.raises(RuntimeError, match="actor_target was closed"):
        learner.update(s)
    learner.close()
    with pytest.raises(RuntimeError, match="the learner is closed"):
        learner.update(s)
    close(tanh_actor, mean_actor, ppo_actor, wide_actor, tanh_critic, wide_critic, foreign, actor, critic, critic_t, ring,
          v, other)
