"""The off-policy side of DDPG("MlpPolicy", env) (solvers/RL/ddpg_train.py) on the device: what lies between "a
closed-loop day ended" and "torch holds a minibatch and its TD targets" (include/sng.h, sng_replay_create and
sng_critic_create).

`ReplayRing` keeps whole days of a ClosedLoopGraph's trajectory in device tensors (one copy kernel a push) and samples
transitions from them with a counter-based integer law that has an exact host model, as SB3's ReplayBufferSamples.
`QCritic` is SB3's ContinuousCritic with one Q net, Linear(O + A, h1)-act-Linear(h1, h2)-act-Linear(h2, 1) on
cat([obs, action]), on the f32-input MFMA, and the TD targets y = r + gamma (1 - d) Q'(s', pi'(s')) of a sample from a
target critic and a target MlpActor.  `DdpgCollector` is a closed-loop graph and the push behind it on one stream.
The gradient step and the polyak update stay the caller's torch, which load()s the weights they give.
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
