"""The off-policy side of DDPG("MlpPolicy", env) (solvers/RL/ddpg_train.py) on the device: what lies between "a
closed-loop day ended" and "torch holds a minibatch and its TD targets" (include/sng.h, sng_replay_create and
sng_critic_create).

`ReplayRing` keeps whole days of a ClosedLoopGraph's trajectory in device tensors (one copy kernel a push) and samples
transitions from them with a counter-based integer law that has an exact host model, as SB3's ReplayBufferSamples.
`QCritic` is SB3's ContinuousCritic with one Q net, Linear(O + A, h1)-act-Linear(h1, h2)-act-Linear(h2, 1) on
cat([obs, action]), on the f32-input MFMA, and the TD targets y = r + gamma (1 - d) Q'(s', pi'(s')) of a sample from a
target critic and a target MlpActor.  `DdpgCollector` is a closed-loop graph and the push behind it on one stream.
`DdpgLearner` is the gradient step behind them (sng_learner_create): both nets' backward passes, Adam and the polyak
update on master weights the learner owns on the device, and the four handles' images rewritten in place, so that no
weight crosses the host between two collected days; `host_update` is its host model.
"""
import collections
import ctypes

import numpy as np

from . import _native
from ._native import check, lib
from .policy import (ACTIVATIONS, DDPG_NET_ARCH, ActionNoise, ClosedLoopGraph, MlpActor, _as_f32, _Handle, _net_arch,
                     _net_spec, _stream_arg, _want, _weights_struct, actor_weights, prefixed_weights)
from .vec_env import _stream_handle

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

# SB3's ReplayBufferSamples, in its field order, with the sampled transitions' indices behind it
ReplaySamples = collections.namedtuple(
    "ReplaySamples", ("observations", "actions", "next_observations", "dones", "rewards", "indices"))

SB3_CRITIC_PREFIX = "critic.qf0"   # TD3Policy's first Q net: critic.qf0.{0,2,4}.{weight,bias}; critic_target.qf0.*


def replay_host_indices(seed, env_offset, counter, n, batch):
    """The sampling law on the CPU (sng_replay_host_indices): the int64 [batch] transition indices a sample with this
    seed, env offset and counter draws from n transitions.  Needs no GPU."""
    out = np.zeros(max(int(batch), 0), np.int64)
    check(lib().sng_replay_host_indices(int(seed), int(env_offset), int(counter), int(n), int(batch),
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
    return out


def critic_weights(weights, obs_dim, act_dim, net_arch=DDPG_NET_ARCH, prefix=SB3_CRITIC_PREFIX):
    """The critic's six float32 arrays (w1 [h1, obs_dim + act_dim], b1, w2 [h2, h1], b2, w3 [1, h2], b3 [1]) from six
    arrays or tensors in that order, or from a DDPG / TD3 state_dict's `prefix`.{0,2,4}.{weight,bias}."""
    if isinstance(weights, dict):
        weights = prefixed_weights(weights, prefix, "critic weights")
    return actor_weights(weights, obs_dim + act_dim, 1, net_arch)


def _critic_spec(net_arch, activation):
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}")
    h1, h2 = _net_arch(net_arch)
    return _native.SngCriticSpec(h1, h2, ACTIVATIONS[activation])


def host_q(obs, actions, weights, net_arch=DDPG_NET_ARCH, activation="relu"):
    """Q(s, a) on the CPU (sng_critic_host_q): float32 [rows] for obs [rows, obs_dim] and actions [rows, act_dim].
    Needs no GPU."""
    obs, actions = _as_f32(obs), _as_f32(actions)
    if obs.ndim != 2 or actions.ndim != 2 or obs.shape[0] != actions.shape[0]:
        raise ValueError("obs and actions must be [rows, obs_dim] and [rows, act_dim]")
    O, A = obs.shape[1], actions.shape[1]
    spec = _critic_spec(net_arch, activation)
    arrs = critic_weights(weights, O, A, _net_arch(net_arch))
    w = _weights_struct(arrs)
    out = np.zeros(obs.shape[0], np.float32)
    F = _native.c_float_p
    check(lib().sng_critic_host_q(O, A, ctypes.byref(spec), ctypes.byref(w), obs.shape[0], obs.ctypes.data_as(F),
                                  actions.ctypes.data_as(F), out.ctypes.data_as(F)))
    return out


def host_targets(next_obs, rewards, dones, weights, gamma=0.99, net_arch=DDPG_NET_ARCH, activation="relu",
                 next_actions=None, actor=None, act_dim=None):
    """The TD targets on the CPU (sng_critic_host_targets): (y float32 [rows], next_actions [rows, act_dim]).
    next_actions given: they are read; else `actor` = dict(weights=six arrays, net_arch=, activation=, squash=, low=,
    high=) is the target actor's host model.  Needs no GPU."""
    next_obs = _as_f32(next_obs)
    rows, O = next_obs.shape
    rewards, dones = _as_f32(rewards).reshape(-1), _as_f32(dones).reshape(-1)
    if rewards.shape != (rows,) or dones.shape != (rows,):
        raise ValueError(f"rewards and dones must hold {rows} values")
    F = _native.c_float_p
    given = next_actions is not None
    aspec = aw = None
    if given:
        na = _as_f32(next_actions).copy()
        if na.ndim != 2 or na.shape[0] != rows:
            raise ValueError(f"next_actions must have shape ({rows}, act_dim)")
        A = na.shape[1]
    else:
        if actor is None:
            raise ValueError("host_targets needs next_actions or the target actor")
        a_arrs = [_as_f32(x) for x in actor["weights"]]
        A = a_arrs[4].shape[0]
        arch = _net_arch(actor.get("net_arch", DDPG_NET_ARCH))
        a_arrs = actor_weights(a_arrs, O, A, arch)
        low, high = actor.get("low"), actor.get("high")
        if low is not None:
            low, high = (np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float32), (A,))) for x in (low, high))
        s = _net_spec(O, A, actor.get("activation", "relu"), low, high, arch, actor.get("squash", True))
        w_a = _weights_struct(a_arrs)
        aspec, aw = ctypes.byref(s), ctypes.byref(w_a)
        na = np.zeros((rows, A), np.float32)
    spec = _critic_spec(net_arch, activation)
    arrs = critic_weights(weights, O, A, _net_arch(net_arch))
    w = _weights_struct(arrs)
    y = np.zeros(rows, np.float32)
    check(lib().sng_critic_host_targets(O, A, ctypes.byref(spec), ctypes.byref(w), aspec, aw, rows,
                                        next_obs.ctypes.data_as(F), rewards.ctypes.data_as(F),
                                        dones.ctypes.data_as(F), float(gamma), na.ctypes.data_as(F), 1 if given else 0,
                                        y.ctypes.data_as(F)))
    return y, na


class ReplayRing(_Handle):
    """A replay buffer of `venv`'s whole days on the device (include/sng.h, sng_replay_create).

    capacity_days -- slots of one day each: obs [capacity, T + 1, E, obs_dim], actions [capacity, T, E, act_dim] (the
                     stored a: a squashed actor's [-1, 1] action, as SB3 stores it), reward float32 and done uint8
                     [capacity, T, E], device tensors this ring owns (`obs`, `actions`, `reward`, `done`)
    seed          -- of the sampler's streams
    push() writes slots head, head + 1, .. (mod capacity) in one kernel; len(ring) is filled * T * E, the transitions
    a sample draws from; transition i is (slot, t, e) = (i // (T E), (i // E) % T, i % E) and its next observation
    obs[slot, t + 1, e].  sample(batch) draws with the ring's `counter`, a host integer bumped once per sample (set it
    back to repeat a sample); host_indices is the law's host model.  close() frees the handle; the tensors stay the
    ring's."""
    _destroy = "sng_replay_destroy"
    _closed = "the replay ring is closed"
    _sync_first = False   # the handle owns nothing on the device

    def __init__(self, venv, capacity_days, seed=0):
        if venv.closed:
            raise ValueError("venv is closed")
        self.venv, self.capacity_days, self.seed = venv, int(capacity_days), int(seed)
        self._p = None
        T, E, dev = venv.timesteps, venv.num_envs, venv.device
        cap = max(self.capacity_days, 0)
        self.obs = torch.zeros((cap, T + 1, E, venv.obs_dim), dtype=torch.float32, device=dev)
        self.actions = torch.zeros((cap, T, E, venv.act_dim), dtype=torch.float32, device=dev)
        self.reward = torch.zeros((cap, T, E), dtype=torch.float32, device=dev)
        self.done = torch.zeros((cap, T, E), dtype=torch.uint8, device=dev)
        spec = _native.SngReplaySpec(self.capacity_days, self.seed, self.obs.data_ptr(), self.actions.data_ptr(),
                                     self.reward.data_ptr(), self.done.data_ptr())
        h = ctypes.c_void_p()
        check(lib().sng_replay_create(venv._h, ctypes.byref(spec), ctypes.byref(h)), venv._h)
        self._own(venv, h)
        self._out = {}   # batch -> ReplaySamples

    def push(self, obs, actions=None, reward=None, done=None, stream=None):
        """A ClosedLoopGraph(trajectory=True)'s days, or four tensors obs [days, T + 1, E, obs_dim] float32, actions
        [days, T, E, act_dim] float32, reward float64 and done uint8 [days, T, E], into the ring: one launch on
        torch's current stream (or `stream`), no synchronisation."""
        self._check_open()
        venv = self.venv
        if isinstance(obs, ClosedLoopGraph):
            g = obs
            if g.venv is not venv:
                raise ValueError("graph was made for another env batch")
            if not g.trajectory:
                raise ValueError("graph must be a ClosedLoopGraph(trajectory=True)")
            obs, actions, reward, done = g.obs_traj, g.action_traj, g.reward_traj, g.done_traj
        T, E, dev = venv.timesteps, venv.num_envs, venv.device
        days = int(obs.shape[0]) if obs.dim() == 4 else -1
        _want(obs, "obs", (days, T + 1, E, venv.obs_dim), torch.float32, dev)
        if actions is None or reward is None or done is None:
            raise ValueError("actions, reward and done must be given with obs")
        _want(actions, "actions", (days, T, E, venv.act_dim), torch.float32, dev)
        _want(reward, "reward", (days, T, E), torch.float64, dev)
        _want(done, "done", (days, T, E), torch.uint8, dev)
        p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        with torch.cuda.device(dev):
            check(lib().sng_replay_push(self._p, days, p(obs), p(actions), p(reward), p(done), _stream_arg(dev, stream)),
                  venv._h)
        return self

    def __len__(self):
        return 0 if self._p is None else int(lib().sng_replay_size(self._p))

    @property
    def head(self):
        """The slot the next pushed day goes to."""
        return self._state()[0]

    @property
    def filled(self):
        """The slots that hold a day."""
        return self._state()[1]

    def _state(self):
        self._check_open()
        head, filled = ctypes.c_int32(), ctypes.c_int32()
        check(lib().sng_replay_state(self._p, ctypes.byref(head), ctypes.byref(filled)), self.venv._h)
        return int(head.value), int(filled.value)

    @property
    def counter(self):
        self._check_open()
        c = ctypes.c_uint64()
        check(lib().sng_replay_get_counter(self._p, ctypes.byref(c)), self.venv._h)
        return int(c.value)

    @counter.setter
    def counter(self, value):
        self._check_open()
        check(lib().sng_replay_set_counter(self._p, int(value)), self.venv._h)

    def _outputs(self, batch):
        if batch not in self._out:
            dev, f32 = self.venv.device, torch.float32
            O, A = self.venv.obs_dim, self.venv.act_dim
            # empty, not zeros: the kernel writes every element (see PpoHead._outputs)
            self._out[batch] = ReplaySamples(
                torch.empty((batch, O), dtype=f32, device=dev), torch.empty((batch, A), dtype=f32, device=dev),
                torch.empty((batch, O), dtype=f32, device=dev), torch.empty((batch, 1), dtype=f32, device=dev),
                torch.empty((batch, 1), dtype=f32, device=dev), torch.empty((batch,), dtype=torch.int64, device=dev))
        return self._out[batch]

    def sample(self, batch, stream=None):
        """ReplaySamples(observations [B, obs_dim], actions [B, act_dim], next_observations, dones [B, 1], rewards
        [B, 1], indices int64 [B]): device tensors this ring owns, overwritten by the next sample of as many rows.  One
        launch on torch's current stream (or `stream`), no synchronisation."""
        self._check_open()
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch must be >= 1")
        if len(self) == 0:
            raise ValueError("the replay ring is empty: push a day first")
        s = self._outputs(batch)
        p = lambda x: x.data_ptr()   # noqa: E731
        out = _native.SngReplayBatch(p(s.observations), p(s.actions), p(s.next_observations), p(s.rewards), p(s.dones),
                                     p(s.indices))
        dev = self.venv.device
        with torch.cuda.device(dev):
            check(lib().sng_replay_sample(self._p, batch, ctypes.byref(out), _stream_arg(dev, stream)), self.venv._h)
        return s

    def host_indices(self, batch, counter=None):
        """The indices sample(batch) draws with `counter` (None: the ring's current one), from the host model."""
        return replay_host_indices(self.seed, self.venv.env_offset, self.counter if counter is None else counter,
                                   len(self), batch)


class QCritic(_Handle):
    """DDPG's / TD3's Q(s, a) of `venv`'s envs on the device (include/sng.h, sng_critic_create): two hidden layers of
    net_arch widths (each 8 .. 512) on cat([obs, action]), one output, on the f32-input MFMA (q_net_kernel).  Widths
    whose LDS tiles do not fit a compute unit at this station's obs_dim + act_dim are refused (NativeError, libsng
    error -2).  The weights are zero until load().  close() frees the critic's device image."""
    _destroy = "sng_critic_destroy"
    _closed = "the critic is closed"

    def __init__(self, venv, net_arch=DDPG_NET_ARCH, activation="relu"):
        if venv.closed:
            raise ValueError("venv is closed")
        self.venv, self.activation = venv, activation
        self.net_arch = _net_arch(net_arch)
        self.obs_dim, self.act_dim = venv.obs_dim, venv.act_dim
        self.weights = None
        self._p = None
        spec = _critic_spec(self.net_arch, activation)
        h = ctypes.c_void_p()
        with torch.cuda.device(venv.device):
            check(lib().sng_critic_create(venv._h, ctypes.byref(spec), ctypes.byref(h)), venv._h)
        self._own(venv, h)
        self._out = {}   # rows -> (q, y, next_actions)

    def load(self, weights, prefix=SB3_CRITIC_PREFIX):
        """Upload weights: a DDPG / TD3 state_dict as it is (`prefix`.{0,2,4}.{weight,bias}; "critic_target.qf0" for
        the target net; other entries are ignored), or six arrays (w1 [h1, obs_dim + act_dim], b1, w2, b2, w3 [1, h2],
        b3).  They take effect at the next q() or targets()."""
        arrs = critic_weights(weights, self.obs_dim, self.act_dim, self.net_arch, prefix)
        self._check_open()
        w = _weights_struct(arrs)
        with torch.cuda.device(self.venv.device):
            check(lib().sng_critic_set_weights(self._p, ctypes.byref(w), _stream_handle(self.venv.device)), self.venv._h)
        self.weights = arrs
        return self

    def _outputs(self, rows):
        if rows not in self._out:
            dev = self.venv.device
            self._out[rows] = (torch.empty((rows,), dtype=torch.float32, device=dev),
                               torch.empty((rows, 1), dtype=torch.float32, device=dev),
                               torch.empty((rows, self.act_dim), dtype=torch.float32, device=dev))
        return self._out[rows]

    def q(self, obs, actions, stream=None):
        """Q [rows] (a device tensor this critic owns, overwritten by the next q() of as many rows) for obs
        [rows, obs_dim] and actions [rows, act_dim]: one launch on torch's current stream (or `stream`)."""
        self._check_open()
        dev = self.venv.device
        rows = int(obs.shape[0]) if obs.dim() == 2 else -1
        _want(obs, "obs", (rows, self.obs_dim), torch.float32, dev)
        _want(actions, "actions", (rows, self.act_dim), torch.float32, dev)
        if rows < 1:
            raise ValueError("obs must have at least one row")
        out = self._outputs(rows)[0]
        p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        with torch.cuda.device(dev):
            check(lib().sng_critic_q(self._p, rows, p(obs), p(actions), p(out), _stream_arg(dev, stream)), self.venv._h)
        return out

    def targets(self, actor_target, samples, gamma=0.99, stream=None):
        """(y [B, 1], next_actions [B, act_dim]) of a ReplaySamples (or anything with next_observations, rewards and
        dones), with this critic as the target critic and actor_target as the target actor: two launches on torch's
        current stream (or `stream`).  The tensors are this critic's, overwritten by the next call of as many rows."""
        self._check_open()
        if not isinstance(actor_target, MlpActor):
            raise ValueError("actor_target must be an MlpActor")
        if actor_target.venv is not self.venv:
            raise ValueError("actor_target was made for another env batch")
        if actor_target._p is None:
            raise ValueError("actor_target is closed")
        if not actor_target.net:
            raise ValueError("actor_target must run policy_net_kernel (another net_arch, squash=True or net=True): the "
                             "64-64 policy_kernel actor takes no row count")
        dev = self.venv.device
        nobs, rew, done = samples.next_observations, samples.rewards, samples.dones
        rows = int(nobs.shape[0]) if nobs.dim() == 2 else -1
        _want(nobs, "samples.next_observations", (rows, self.obs_dim), torch.float32, dev)
        _want(rew, "samples.rewards", (rows, 1), torch.float32, dev)
        _want(done, "samples.dones", (rows, 1), torch.float32, dev)
        if rows < 1:
            raise ValueError("samples must have at least one row")
        _, y, na = self._outputs(rows)
        p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        with torch.cuda.device(dev):
            check(lib().sng_critic_targets(self._p, actor_target._p, rows, p(nobs), p(rew), p(done), float(gamma), p(na),
                                           p(y), _stream_arg(dev, stream)), self.venv._h)
        return y, na

    def host_q(self, obs, actions):
        """The host model of q() on numpy arrays or tensors."""
        if self.weights is None:
            raise RuntimeError("load() the critic's weights first")
        return host_q(obs, actions, self.weights, self.net_arch, self.activation)

    def host_targets(self, samples, gamma=0.99, next_actions=None, actor_target=None):
        """The host model of targets(): (y [B], next_actions [B, act_dim]) as numpy arrays; next_actions given (e.g.
        the device's own), or computed by actor_target's host model."""
        if self.weights is None:
            raise RuntimeError("load() the critic's weights first")
        actor = None
        if next_actions is None:
            if actor_target is None or actor_target.weights is None:
                raise RuntimeError("host_targets needs next_actions or a loaded actor_target")
            actor = dict(weights=actor_target.weights, net_arch=actor_target.net_arch,
                         activation=actor_target.activation, squash=actor_target.squash, low=actor_target.low,
                         high=actor_target.high)
        return host_targets(samples.next_observations, samples.rewards, samples.dones, self.weights, gamma,
                            self.net_arch, self.activation, next_actions, actor)


# TD3Policy's four nets as SB3's state_dict names them, in sng.h's SNG_LEARNER_* order
LEARNER_NETS = {"actor": "actor.mu", "critic": SB3_CRITIC_PREFIX, "actor_target": "actor_target.mu",
                "critic_target": "critic_target.qf0"}
LEARNER_SEGMENT = _native.LEARNER_SEGMENT
LEARNER_MAX_ROWS = _native.LEARNER_MAX_ROWS


def net_keys(prefix):
    """`prefix`.{0,2,4}.{weight,bias}: a three-layer nn.Sequential's state_dict keys, in (w1, b1, w2, b2, w3, b3) order."""
    return [f"{prefix}.{layer}.{part}" for layer in (0, 2, 4) for part in ("weight", "bias")]


def _net_shapes(k, h1, h2, n):
    return [(h1, k), (h1,), (h2, h1), (h2,), (n, h2), (n,)]


def _learner_shapes(obs_dim, act_dim, actor_arch, critic_arch):
    a, c = _net_shapes(obs_dim, *actor_arch, act_dim), _net_shapes(obs_dim + act_dim, *critic_arch, 1)
    return {"actor": a, "critic": c, "actor_target": a, "critic_target": c}


def _arrays_struct(arrs):
    return _native.SngNetArrays(*[a.ctypes.data for a in arrs])


def _learner_spec(actor_lr, critic_lr, tau, betas, eps):
    return _native.SngLearnerSpec(float(actor_lr), float(critic_lr), float(tau), float(betas[0]), float(betas[1]),
                                  float(eps))


def learner_host_state(params, obs_dim, act_dim, actor_arch=DDPG_NET_ARCH, critic_arch=DDPG_NET_ARCH, exp_avg=None,
                       exp_avg_sq=None, step=0):
    """A learner's state for host_update: dict(params=, exp_avg=, exp_avg_sq=, step=), each a dict of float32 arrays
    under SB3's names -- params the 24 entries of LEARNER_NETS (from a TD3Policy state_dict; other entries are
    ignored), the moments the 12 of actor.mu.* and critic.qf0.* (zeros when not given).  The arrays are copies."""
    shapes = _learner_shapes(obs_dim, act_dim, _net_arch(actor_arch), _net_arch(critic_arch))
    out = dict(params={}, exp_avg={}, exp_avg_sq={}, step=int(step))
    for net, prefix in LEARNER_NETS.items():
        for key, shape in zip(net_keys(prefix), shapes[net]):
            if key not in params:
                raise KeyError(f"learner state: missing {key}")
            arr = _as_f32(params[key]).copy()
            if arr.shape != shape:
                raise ValueError(f"learner state: {key} must have shape {shape}, got {arr.shape}")
            out["params"][key] = arr
            if net in ("actor", "critic"):
                for name, given in (("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
                    out[name][key] = np.zeros(shape, np.float32) if given is None else _as_f32(given[key]).copy()
    return out


def _state_struct(state):
    """(SngLearnerState over the arrays of a learner_host_state dict, which it reads and writes in place)"""
    nets = []
    for net, prefix in LEARNER_NETS.items():
        nets.append(_arrays_struct([state["params"][k] for k in net_keys(prefix)]))
    moments = []
    for net in ("actor", "critic"):
        for name in ("exp_avg", "exp_avg_sq"):
            moments.append(_arrays_struct([state[name][k] for k in net_keys(LEARNER_NETS[net])]))
    return _native.SngLearnerState(*nets, *moments, int(state["step"]))


def host_update(state, obs, actions, y, a_pi, low, high, actor_arch=DDPG_NET_ARCH, critic_arch=DDPG_NET_ARCH,
                actor_lr=1e-3, critic_lr=1e-3, tau=0.005, betas=(0.9, 0.999), eps=1e-8, activation="relu",
                squash=True):
    """The host model of one DdpgLearner.update (sng_learner_host_update) on numpy: `state` (learner_host_state) is
    updated in place; obs [B, obs_dim], actions [B, act_dim], y [B]; a_pi [B, act_dim] stands for tanh(actor(obs)) --
    the device's own for an exact comparison.  low / high: the action Box of the squashed actor.  Returns a dict with q,
    dq, q_pi [B], critic_loss, actor_loss and grads (the 12 gradients under SB3's names).  Needs no GPU."""
    obs, actions, a_pi = _as_f32(obs), _as_f32(actions), _as_f32(a_pi)
    y = _as_f32(y).reshape(-1)
    if obs.ndim != 2 or actions.ndim != 2:
        raise ValueError("obs and actions must be [rows, obs_dim] and [rows, act_dim]")
    rows, O = obs.shape
    A = actions.shape[1]
    if actions.shape[0] != rows or y.shape != (rows,) or a_pi.shape != (rows, A):
        raise ValueError(f"actions, y and a_pi must hold {rows} rows")
    actor_arch, critic_arch = _net_arch(actor_arch), _net_arch(critic_arch)
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}")
    if low is not None:
        low, high = (np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float32), (A,))) for x in (low, high))
    aspec = _net_spec(O, A, activation, low, high, actor_arch, squash)
    cspec = _native.SngCriticSpec(critic_arch[0], critic_arch[1], ACTIVATIONS[activation])
    spec = _learner_spec(actor_lr, critic_lr, tau, betas, eps)
    shapes = _learner_shapes(O, A, actor_arch, critic_arch)
    grads = {k: np.zeros(s, np.float32) for net in ("actor", "critic")
             for k, s in zip(net_keys(LEARNER_NETS[net]), shapes[net])}
    q, dq, q_pi = (np.zeros(max(rows, 1), np.float32) for _ in range(3))
    losses = np.zeros(2, np.float32)
    trace = _native.SngLearnerTrace(
        q.ctypes.data, dq.ctypes.data, q_pi.ctypes.data,
        _arrays_struct([grads[k] for k in net_keys(LEARNER_NETS["critic"])]),
        _arrays_struct([grads[k] for k in net_keys(LEARNER_NETS["actor"])]), losses.ctypes.data,
        losses.ctypes.data + 4)
    st = _state_struct(state)
    F = _native.c_float_p
    check(lib().sng_learner_host_update(ctypes.byref(aspec), ctypes.byref(cspec), ctypes.byref(spec), ctypes.byref(st),
                                        rows, obs.ctypes.data_as(F), actions.ctypes.data_as(F), y.ctypes.data_as(F),
                                        a_pi.ctypes.data_as(F), ctypes.byref(trace)))
    state["step"] = int(st.step)
    return dict(q=q[:rows], dq=dq[:rows], q_pi=q_pi[:rows], critic_loss=losses[0], actor_loss=losses[1], grads=grads)


class _DeviceArray:
    """A float32 array in device memory the library owns, for torch.as_tensor (the CUDA array interface)."""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr="<f4", data=(int(ptr), False), version=2,
                                             strides=None)


class DdpgLearner(_Handle):
    """DDPG's gradient step on the device (include/sng.h, sng_learner_create): one SB3 TD3.train iteration with one
    critic -- the critic's step on mean((Q(s, a) - y)^2), the actor's on -mean(Q(s, pi(s))) with the critic as just
    updated, Adam on both, the polyak update of both targets -- and the four handles' device images rewritten from the
    new weights, as plain launches on one stream without synchronisation.  A ClosedLoopGraph captured with `actor` acts
    with the new weights at its next launch, and critic_target.targets uses the new targets.

    actor, actor_target   -- MlpActors of `venv` with squash=True and relu hidden layers, load()ed
    critic, critic_target -- QCritics of `venv` with relu, load()ed
    Their loaded weights are the initial master weights; Adam's moments start at zero.  `params` (24 entries), `grads`
    (12) and `moments` (12 pairs (exp_avg, exp_avg_sq)) are dicts of device tensors the learner owns, keyed by SB3's
    names: actor.mu.{0,2,4}.{weight,bias}, critic.qf0.*, actor_target.mu.*, critic_target.qf0.*.  update() leaves the
    handles' host `weights` stale and sets them to None; pull() brings the weights back.

    The tensors of `params`, `grads` and `moments` are views of memory the library owns, valid until close() (clone()
    what is to outlive the learner).  While a learner lives its masters are the weights: load() on one of its four nets
    changes that net's device image only until the next update overwrites it from the masters -- give new weights to
    the learner with load_state(learner_host_state(state_dict, ...)) instead."""
    _destroy = "sng_learner_destroy"
    _closed = "the learner is closed"

    def __init__(self, venv, actor, critic, actor_target, critic_target, actor_lr=1e-3, critic_lr=1e-3, tau=0.005,
                 gamma=0.99, betas=(0.9, 0.999), eps=1e-8):
        if venv.closed:
            raise ValueError("venv is closed")
        for name, net, kind in (("actor", actor, MlpActor), ("actor_target", actor_target, MlpActor),
                                ("critic", critic, QCritic), ("critic_target", critic_target, QCritic)):
            if not isinstance(net, kind):
                raise ValueError(f"{name} must be a {kind.__name__}")
            if net.venv is not venv:
                raise ValueError(f"{name} was made for another env batch")
            if net._p is None:
                raise ValueError(f"{name} is closed")
            if net.weights is None:
                raise ValueError(f"load() {name}'s weights first: they are the learner's initial master weights")
        self.venv = venv
        self.actor, self.critic, self.actor_target, self.critic_target = actor, critic, actor_target, critic_target
        self.gamma = float(gamma)
        self.hyper = dict(actor_lr=float(actor_lr), critic_lr=float(critic_lr), tau=float(tau),
                          betas=(float(betas[0]), float(betas[1])), eps=float(eps))
        self._p = None
        spec = _learner_spec(actor_lr, critic_lr, tau, betas, eps)
        h = ctypes.c_void_p()
        with torch.cuda.device(venv.device):
            check(lib().sng_learner_create(venv._h, actor._p, actor_target._p, critic._p, critic_target._p,
                                           ctypes.byref(spec), ctypes.byref(h)), venv._h)
        self._own(venv, h)
        self._shapes = _learner_shapes(venv.obs_dim, venv.act_dim, actor.net_arch, critic.net_arch)
        params = {}
        for name, net in (("actor", actor), ("critic", critic), ("actor_target", actor_target),
                          ("critic_target", critic_target)):
            params.update(zip(net_keys(LEARNER_NETS[name]), net.weights))
        self.load_state(learner_host_state(params, venv.obs_dim, venv.act_dim, actor.net_arch, critic.net_arch))
        dev = {which: self._arrays(which) for which in _native.LEARNER_ARRAYS}
        self.params, self.grads, self.moments = {}, {}, {}
        for net, prefix in LEARNER_NETS.items():
            self.params.update(zip(net_keys(prefix), dev[net]))
        for net in ("actor", "critic"):
            keys = net_keys(LEARNER_NETS[net])
            self.grads.update(zip(keys, dev[net + "_grad"]))
            self.moments.update(zip(keys, zip(dev[net + "_m"], dev[net + "_v"])))

    def _tensor(self, ptr, shape):
        with torch.cuda.device(self.venv.device):
            return torch.as_tensor(_DeviceArray(ptr, shape), device=self.venv.device)

    def _arrays(self, which):
        """The six device tensors of one of _native.LEARNER_ARRAYS."""
        a = _native.SngNetArrays()
        check(lib().sng_learner_arrays(self._p, _native.LEARNER_ARRAYS.index(which), ctypes.byref(a)), self.venv._h)
        net = which.split("_")[0]
        return [self._tensor(getattr(a, f), s) for f, s in zip(("w1", "b1", "w2", "b2", "w3", "b3"), self._shapes[net])]

    @property
    def step(self):
        """Updates so far: Adam's t of the last one."""
        self._check_open()
        t = ctypes.c_int64()
        check(lib().sng_learner_get_step(self._p, ctypes.byref(t)), self.venv._h)
        return int(t.value)

    def load_state(self, state):
        """Masters, targets, moments and step from a learner_host_state dict (sng_learner_set_state); the four
        handles' device images are rewritten from the masters.  Synchronises."""
        self._check_open()
        st = _state_struct(state)
        dev = self.venv.device
        with torch.cuda.device(dev):
            check(lib().sng_learner_set_state(self._p, ctypes.byref(st), _stream_handle(dev)), self.venv._h)
        return self

    def host_state(self):
        """The learner's state on the host, as learner_host_state gives it (sng_learner_get_state).  Synchronises."""
        self._check_open()
        venv = self.venv
        state = dict(params={}, exp_avg={}, exp_avg_sq={}, step=0)
        for net, prefix in LEARNER_NETS.items():
            for key, shape in zip(net_keys(prefix), self._shapes[net]):
                state["params"][key] = np.zeros(shape, np.float32)
                if net in ("actor", "critic"):
                    state["exp_avg"][key] = np.zeros(shape, np.float32)
                    state["exp_avg_sq"][key] = np.zeros(shape, np.float32)
        st = _state_struct(state)
        t = ctypes.c_int64()
        with torch.cuda.device(venv.device):
            check(lib().sng_learner_get_state(self._p, ctypes.byref(st), ctypes.byref(t), _stream_handle(venv.device)),
                  venv._h)
        state["step"] = int(t.value)
        return state

    def pull(self):
        """The 24 weights as a state_dict of numpy arrays under SB3's names, ready for TD3Policy.load_state_dict after
        torch.from_numpy; the four handles' `weights` are refreshed from it, so their host_* methods work again."""
        sd = self.host_state()["params"]
        for name, net in (("actor", self.actor), ("critic", self.critic), ("actor_target", self.actor_target),
                          ("critic_target", self.critic_target)):
            net.weights = [sd[k] for k in net_keys(LEARNER_NETS[name])]
        return sd

    def update(self, samples, y=None, stream=None):
        """One update on a ReplaySamples (or anything with observations and actions, and for y=None what
        QCritic.targets reads).  y [B, 1] or [B]: the TD targets; None: critic_target.targets(actor_target, samples,
        gamma) is called first.  Launches on torch's current stream (or `stream`), no synchronisation."""
        self._check_open()
        for name, net in (("actor", self.actor), ("critic", self.critic), ("actor_target", self.actor_target),
                          ("critic_target", self.critic_target)):
            if net._p is None:
                raise RuntimeError(f"{name} was closed: a DdpgLearner needs its four nets for every update")
        dev = self.venv.device
        obs, act = samples.observations, samples.actions
        rows = int(obs.shape[0]) if obs.dim() == 2 else -1
        _want(obs, "samples.observations", (rows, self.venv.obs_dim), torch.float32, dev)
        _want(act, "samples.actions", (rows, self.venv.act_dim), torch.float32, dev)
        if rows < 1 or rows > LEARNER_MAX_ROWS:
            raise ValueError(f"an update takes 1 .. {LEARNER_MAX_ROWS} rows, got {rows}")
        if y is None:
            y, _ = self.critic_target.targets(self.actor_target, samples, self.gamma, stream)
        if y.numel() != rows or y.dtype != torch.float32 or y.device != dev or not y.is_contiguous():
            raise ValueError(f"y must be a contiguous float32 tensor of {rows} values on {dev}")
        p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        with torch.cuda.device(dev):
            check(lib().sng_learner_update(self._p, rows, p(obs), p(act), p(y), _stream_arg(dev, stream)), self.venv._h)
        self._last_y = y
        for net in (self.actor, self.critic, self.actor_target, self.critic_target):
            net.weights = None   # stale until pull()
        return self

    def train(self, ring, batch, gradient_steps=1, stream=None):
        """SB3's train(gradient_steps, batch_size): sample -> targets -> update, gradient_steps times, on torch's
        current stream (or `stream`) without synchronising."""
        if not isinstance(ring, ReplayRing) or ring.venv is not self.venv:
            raise ValueError("ring must be a ReplayRing of the learner's env batch")
        for _ in range(int(gradient_steps)):
            self.update(ring.sample(batch, stream), stream=stream)
        return self

    @property
    def last(self):
        """The last update's q [B], dq [B], y, a_pi [B, act_dim], q_pi [B], critic_loss and actor_loss (0-dim): device
        tensors the learner owns (y: the caller's or the target critic's), overwritten by the next update.  They are
        views of the learner's workspace, not copies: an update with more rows than any before it frees and reallocates
        that workspace, and close() frees it, after which tensors taken earlier must not be used -- take `last` again
        after such an update, and clone() what is to be kept."""
        self._check_open()
        o = _native.SngLearnerLast()
        check(lib().sng_learner_last(self._p, ctypes.byref(o)), self.venv._h)
        B, A = int(o.rows), self.venv.act_dim
        return dict(q=self._tensor(o.q, (B,)), dq=self._tensor(o.dq, (B,)), y=self._last_y,
                    a_pi=self._tensor(o.a_pi, (B, A)), q_pi=self._tensor(o.q_pi, (B,)),
                    critic_loss=self._tensor(o.critic_loss, (1,)).reshape(()),
                    actor_loss=self._tensor(o.actor_loss, (1,)).reshape(()))

    def host_update(self, state, obs, actions, y, a_pi):
        """The host model of update() with this learner's nets and hyper-parameters (see host_update)."""
        return host_update(state, obs, actions, y, a_pi, self.actor.low, self.actor.high, self.actor.net_arch,
                           self.critic.net_arch, activation=self.actor.activation, squash=self.actor.squash,
                           **self.hyper)


class DdpgCollector:
    """DDPG's collection as one object: `days` closed-loop days of `actor` with `noise` (a ClosedLoopGraph with
    trajectory=True and a device-RNG reset) and the ring's push behind them on the same stream.  launch() runs both,
    without synchronisation; `graph` holds the days just collected."""

    def __init__(self, venv, actor, noise, ring, days=1):
        if not isinstance(ring, ReplayRing):
            raise ValueError("ring must be a ReplayRing")
        if ring.venv is not venv:
            raise ValueError("ring was made for another env batch")
        if ring._p is None:
            raise ValueError("ring is closed")
        if noise is not None and not isinstance(noise, (ActionNoise, torch.Tensor)):
            raise ValueError("noise must be an ActionNoise, a tensor [T, E, act_dim] or None")
        if int(days) < 1 or int(days) > ring.capacity_days:
            raise ValueError(f"days must be 1 .. the ring's capacity_days {ring.capacity_days}")
        self.venv, self.actor, self.noise, self.ring, self.days = venv, actor, noise, ring, int(days)
        self.graph = ClosedLoopGraph(venv, actor, noise=noise, days=self.days, with_reset=True, trajectory=True)

    def launch(self, stream=None):
        if self.ring._p is None:
            raise RuntimeError("the replay ring was closed: a DdpgCollector needs it for every launch")
        self.graph.launch(stream)
        self.ring.push(self.graph, stream=stream)

    def close(self):
        self.graph.close()
