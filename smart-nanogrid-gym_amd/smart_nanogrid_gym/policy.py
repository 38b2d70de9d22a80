"""The policy in the loop: the MLP actors of the reference's own workloads, PPO("MlpPolicy", env)
(solvers/RL/ppo_train.py:92) and DDPG("MlpPolicy", env) (solvers/RL/ddpg_train.py), evaluated by the library between
steps.

`MlpActor` is the actor as a device kernel: by default the 64-64 tanh (or relu) actor of PPO (include/sng.h,
sng_policy_create); with another `net_arch` or `squash=True` an actor of any two hidden widths up to 512 on the
f32-input MFMA (sng_policy_create_net), whose squashed output is SB3's DDPG / TD3 / SAC actor: tanh, noise clipped in
[-1, 1], rescaled into the action Box.  It is a callable from observations to env actions, and the host model of the
same arithmetic.  `ClosedLoopGraph` captures whole days with the actor between the steps (sng_graph_create_policy),
so a rollout whose every action answers the observation before it is one graph launch, with no torch kernel in it.
"""
import ctypes
import weakref

import numpy as np

from . import _native
from ._native import check, lib
from .vec_env import _stream_handle

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

HIDDEN = 64
ACTIVATIONS = {"tanh": 0, "relu": 1}
# stable-baselines3's ActorCriticPolicy state_dict keys of the actor: policy_net's two Linear layers and action_net
SB3_KEYS = ("mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias",
            "mlp_extractor.policy_net.2.weight", "mlp_extractor.policy_net.2.bias",
            "action_net.weight", "action_net.bias")
# stable-baselines3's TD3Policy (DDPG, TD3) state_dict keys of the actor: mu = Linear, ReLU, Linear, ReLU, Linear, Tanh
SB3_DDPG_KEYS = ("actor.mu.0.weight", "actor.mu.0.bias", "actor.mu.2.weight", "actor.mu.2.bias",
                 "actor.mu.4.weight", "actor.mu.4.bias")
DDPG_NET_ARCH = (400, 300)


def _as_f32(x):
    if torch is not None and isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32)


def _net_arch(net_arch):
    arch = tuple(int(h) for h in net_arch)
    if len(arch) != 2:
        raise ValueError("net_arch must name two hidden widths")
    return arch


def actor_weights(weights, obs_dim, act_dim, net_arch=(HIDDEN, HIDDEN)):
    """Six float32 arrays (w1 [h1, obs_dim], b1, w2 [h2, h1], b2, w3 [act_dim, h2], b3; net_arch = (h1, h2)) from six
    arrays or tensors in that order, or from a dict holding stable-baselines3's actor keys: PPO's (SB3_KEYS) or
    DDPG's / TD3's (SB3_DDPG_KEYS); other entries are ignored."""
    h1, h2 = _net_arch(net_arch)
    if isinstance(weights, dict):
        keys = SB3_DDPG_KEYS if SB3_DDPG_KEYS[0] in weights else SB3_KEYS
        missing = [k for k in keys if k not in weights]
        if missing:
            raise KeyError(f"actor weights: missing {missing}")
        weights = [weights[k] for k in keys]
    arrs = [_as_f32(w) for w in weights]
    shapes = [(h1, obs_dim), (h1,), (h2, h1), (h2,), (act_dim, h2), (act_dim,)]
    if len(arrs) != 6 or any(a.shape != s for a, s in zip(arrs, shapes)):
        raise ValueError(f"actor weights must have shapes {shapes}, got {[a.shape for a in arrs]}")
    return arrs


def _spec(obs_dim, act_dim, activation, low, high, hidden=HIDDEN):
    spec = _native.SngMlpSpec(obs_dim, act_dim, hidden, ACTIVATIONS[activation], None, None)
    if low is not None:
        spec.clip_low = low.ctypes.data_as(_native.c_float_p)
        spec.clip_high = high.ctypes.data_as(_native.c_float_p)
    return spec


def _net_spec(obs_dim, act_dim, activation, low, high, net_arch, squash):
    h1, h2 = net_arch
    spec = _native.SngMlpNetSpec(obs_dim, act_dim, h1, h2, ACTIVATIONS[activation],
                                 _native.MLP_OUT_SQUASH if squash else _native.MLP_OUT_MEAN, None, None)
    if low is not None:
        spec.low = low.ctypes.data_as(_native.c_float_p)
        spec.high = high.ctypes.data_as(_native.c_float_p)
    return spec


def _weights_struct(arrs):
    return _native.SngMlpWeights(*[a.ctypes.data_as(_native.c_float_p) for a in arrs])


def host_actions(obs, weights, activation="tanh", low=None, high=None, noise=None, net_arch=(HIDDEN, HIDDEN),
                 squash=False, net=False):
    """The actor's contract on the CPU: (a, env actions) float32 [rows, act_dim] for observation rows
    [rows, obs_dim].  low / high: the clip bounds, or None for no clip; with squash=True the action Box.  The 64-64
    actor without squash is sng_policy_host_actions; another net_arch, squash=True or net=True (the diagnostic path
    of MlpActor's `net`) is sng_policy_net_host_actions, which accepts what sng_policy_create_net accepts: at most 64
    actions.  Needs no GPU."""
    obs = np.ascontiguousarray(obs, dtype=np.float32)
    rows, obs_dim = obs.shape
    arch = _net_arch(net_arch)
    if isinstance(weights, dict):
        last = weights[SB3_DDPG_KEYS[4]] if SB3_DDPG_KEYS[0] in weights else weights[SB3_KEYS[4]]
    else:
        last = weights[4]
    act_dim = np.shape(last)[0]
    arrs = actor_weights(weights, obs_dim, act_dim, arch)
    if low is not None:
        low, high = (np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float32), (act_dim,))) for x in (low, high))
    w = _weights_struct(arrs)
    a = np.zeros((rows, act_dim), np.float32)
    env_a = np.zeros((rows, act_dim), np.float32)
    nz = None
    if noise is not None:
        nz = np.ascontiguousarray(noise, dtype=np.float32)
        if nz.shape != a.shape:
            raise ValueError(f"noise must have shape {a.shape}")
    F = _native.c_float_p
    args = (rows, obs.ctypes.data_as(F), None if nz is None else nz.ctypes.data_as(F), a.ctypes.data_as(F),
            env_a.ctypes.data_as(F))
    if net or squash or arch != (HIDDEN, HIDDEN):
        spec = _net_spec(obs_dim, act_dim, activation, low, high, arch, squash)
        check(lib().sng_policy_net_host_actions(ctypes.byref(spec), ctypes.byref(w), *args))
    else:
        spec = _spec(obs_dim, act_dim, activation, low, high)
        check(lib().sng_policy_host_actions(ctypes.byref(spec), ctypes.byref(w), *args))
    return a, env_a


class MlpActor:
    """An MLP actor of `venv`'s envs on the device.

    activation -- of the hidden layers: "tanh" (SB3's MlpPolicy) or "relu"
    clip       -- True: the env is stepped with the action clipped to venv.action_space, as SB3 clips a Box
                  action before env.step; False: with the action as it is.  Without meaning with squash=True.
    net_arch   -- the two hidden widths, each 8 .. 512.  (64, 64) without squash is PPO's actor and policy_kernel
                  (sng_policy_create), at every station; anything else runs policy_net_kernel on the f32-input MFMA
                  (sng_policy_create_net), which has two output tiles: venv.act_dim <= 64, i.e. stations of up to 63
                  chargers with a battery and 64 without.  A wider station is refused (NativeError, libsng error -2).
    squash     -- True: SB3's DDPG / TD3 / SAC output: a = tanh(mean), with noise clipped to [-1, 1] after the add,
                  and the env is stepped with a rescaled from [-1, 1] into venv.action_space (unscale_action).
    net        -- True: the 64-64 actor without squash through policy_net_kernel too.  A diagnostic path: the same
                  results, for cross-checking the two kernels, and measured slower than the default (20.2 against
                  17.3 us a launch at 65,536 envs x 8 chargers, profiles/policy_net_ab.txt)

    `actor(obs)` maps a device tensor [rows <= num_envs, obs_dim] to the env actions [rows, act_dim] (one kernel
    launch on torch's current stream), so the actor is a policy for evaluate_models and tools/closed_loop_bench.py
    like any torch callable.  `actions(obs, noise)` returns (a, env actions) for the whole batch.  The weights are
    zero until load()."""

    def __init__(self, venv, activation="tanh", clip=True, net_arch=(HIDDEN, HIDDEN), squash=False, net=False):
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}")
        self.venv = venv
        self.activation = activation
        self.net_arch = _net_arch(net_arch)
        self.squash = bool(squash)
        self.net = bool(net) or self.squash or self.net_arch != (HIDDEN, HIDDEN)
        self.obs_dim, self.act_dim = venv.obs_dim, venv.act_dim
        self.low = self.high = None
        if clip or self.squash:
            self.low = np.ascontiguousarray(venv.action_space.low, dtype=np.float32).reshape(self.act_dim)
            self.high = np.ascontiguousarray(venv.action_space.high, dtype=np.float32).reshape(self.act_dim)
        self.weights = None
        h = ctypes.c_void_p()
        if self.net:
            spec = _net_spec(self.obs_dim, self.act_dim, activation, self.low, self.high, self.net_arch, self.squash)
            check(lib().sng_policy_create_net(venv._h, ctypes.byref(spec), ctypes.byref(h)), venv._h)
        else:
            spec = _spec(self.obs_dim, self.act_dim, activation, self.low, self.high)
            check(lib().sng_policy_create(venv._h, ctypes.byref(spec), ctypes.byref(h)), venv._h)
        self._p = h
        venv._actors.append(weakref.ref(self))   # the env batch closes its actors before itself
        E = venv.num_envs
        self.actions_d = torch.zeros((E, self.act_dim), dtype=torch.float32, device=venv.device)
        self.env_actions_d = torch.zeros((E, self.act_dim), dtype=torch.float32, device=venv.device)
        self._obs_pad = None

    @classmethod
    def ddpg(cls, venv):
        """SB3's DDPG("MlpPolicy", env) actor: 400-300, relu, squashed into venv.action_space."""
        return cls(venv, activation="relu", net_arch=DDPG_NET_ARCH, squash=True)

    def load(self, weights):
        """Upload weights: six arrays or tensors (w1, b1, w2, b2, w3, b3 in torch's [out, in] layout) or a dict with
        SB3's actor keys (PPO's or DDPG's).  Graphs captured with this actor use them from their next launch on."""
        arrs = actor_weights(weights, self.obs_dim, self.act_dim, self.net_arch)
        w = _weights_struct(arrs)
        with torch.cuda.device(self.venv.device):
            check(lib().sng_policy_set_weights(self._p, ctypes.byref(w), _stream_handle(self.venv.device)),
                  self.venv._h)
        self.weights = arrs
        return self

    def actions(self, obs, noise=None):
        """(a, env actions), device tensors [num_envs, act_dim] this object owns, for obs [num_envs, obs_dim] and an
        optional noise tensor [num_envs, act_dim]."""
        venv = self.venv
        E = venv.num_envs
        obs = obs.to(device=venv.device, dtype=torch.float32).contiguous()
        if tuple(obs.shape) != (E, self.obs_dim):
            raise ValueError(f"obs must have shape {(E, self.obs_dim)}")
        nz = None
        if noise is not None:
            noise = noise.to(device=venv.device, dtype=torch.float32).contiguous()
            if tuple(noise.shape) != (E, self.act_dim):
                raise ValueError(f"noise must have shape {(E, self.act_dim)}")
            nz = ctypes.c_void_p(noise.data_ptr())
        with torch.cuda.device(venv.device):
            check(lib().sng_policy_actions(self._p, ctypes.c_void_p(obs.data_ptr()), nz,
                                           ctypes.c_void_p(self.actions_d.data_ptr()),
                                           ctypes.c_void_p(self.env_actions_d.data_ptr()),
                                           _stream_handle(venv.device)), venv._h)
        return self.actions_d, self.env_actions_d

    def __call__(self, obs):
        rows = obs.shape[0]
        E = self.venv.num_envs
        if rows > E:
            raise ValueError(f"the actor was made for {E} envs, got {rows} observation rows")
        if rows < E:   # fewer rows than envs: through a padded batch
            if self._obs_pad is None:
                self._obs_pad = torch.zeros((E, self.obs_dim), dtype=torch.float32, device=self.venv.device)
            self._obs_pad[:rows].copy_(obs)
            obs = self._obs_pad
        return self.actions(obs)[1][:rows].clone()

    def host_actions(self, obs, noise=None):
        """The host model on observation rows (numpy or tensor): (a, env actions) as numpy arrays."""
        if self.weights is None:
            raise RuntimeError("load() the actor's weights first")
        return host_actions(_as_f32(obs), self.weights, self.activation, self.low, self.high,
                            None if noise is None else _as_f32(noise), net_arch=self.net_arch, squash=self.squash,
                            net=self.net)

    def close(self):
        """Frees the actor's device image and buffers.  Closing the env batch closes its actors first (the library
        wants a policy destroyed before its env); graphs captured with the actor must not be launched afterwards."""
        if getattr(self, "_p", None):
            torch.cuda.synchronize(self.venv.device)
            lib().sng_policy_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ClosedLoopGraph:
    """Whole days with the actor in the loop, captured once as a hipGraph and replayed: ([device-RNG reset] + T x
    (actor, step)) x days (include/sng.h, sng_graph_create_policy).

    noise      -- optional device tensor [T, E, act_dim] added to the actor's mean (to tanh(mean) for a squashed
                  actor: DDPG's action noise, e.g. a precomputed Ornstein-Uhlenbeck path), reused every day
    trajectory -- True: keeps every step: obs_traj [days, T + 1, E, obs_dim], action_traj [days, T, E, act_dim] (a,
                  before the clip or the rescale), reward_traj and done_traj [days, T, E]; obs_traj[d, t] is the
                  observation action_traj[d, t] answered.  False: venv.obs_d / reward_d / done_d and `actions`
                  [E, act_dim] hold the last step's values.
    with_reset, days, day_returns, step_nodes -- as EpisodeGraph's.  A steps-only graph steps the loaded day from its
                  t = 0 observation in venv.obs_d.
    fused      -- True: one node a day wherever the station has the fused kernel (the lean stations; sng.h
                  SNG_GRAPH_POLICY_FUSED), also where the node form measured no slower and is the default (the same
                  results; for A/B and tests).  step_nodes wins over it.  An actor on policy_net_kernel (another
                  net_arch, squash) has no fused day: its graphs are nodes whatever is asked.
    New weights loaded into the actor take effect at the next launch, without a recapture."""

    def __init__(self, venv, actor, noise=None, days=1, with_reset=True, trajectory=False, day_returns=None,
                 step_nodes=False, fused=False):
        if actor.venv is not venv:
            raise ValueError("the actor was made for another env batch")
        if actor._p is None or venv.closed:
            raise ValueError("the actor (or its env batch) is closed")
        if with_reset:
            venv._apply_pending_seed()
        elif venv._seeds[0] is not None:
            raise ValueError("seed() waits for the next reset: reset before capturing a steps-only graph")
        self.venv, self.actor = venv, actor
        self.days = int(days)
        self.with_reset = bool(with_reset)
        self.trajectory = bool(trajectory)
        T, E, A = venv.timesteps, venv.num_envs, venv.act_dim
        self.noise = None
        if noise is not None:
            self.noise = noise.to(device=venv.device, dtype=torch.float32).contiguous()
            if tuple(self.noise.shape) != (T, E, A):
                raise ValueError(f"noise must have shape {(T, E, A)}")
        self.day_returns = day_returns
        dr = None
        if day_returns is not None:
            if (tuple(day_returns.shape) != (self.days, E) or day_returns.dtype != torch.float64
                    or day_returns.device != venv.device or not day_returns.is_contiguous()):
                raise ValueError("day_returns must be a contiguous float64 device tensor [days, num_envs]")
            dr = ctypes.c_void_p(day_returns.data_ptr())
        obs, reward, done = venv.obs_d, venv.reward_d, venv.done_d
        self.obs_traj = self.action_traj = self.reward_traj = self.done_traj = None
        if self.trajectory:
            dev = venv.device
            self.obs_traj = obs = torch.zeros((self.days, T + 1, E, venv.obs_dim), dtype=torch.float32, device=dev)
            self.action_traj = torch.zeros((self.days, T, E, A), dtype=torch.float32, device=dev)
            self.reward_traj = reward = torch.zeros((self.days, T, E), dtype=torch.float64, device=dev)
            self.done_traj = done = torch.zeros((self.days, T, E), dtype=torch.uint8, device=dev)
            self.actions = self.action_traj[-1, -1]
        else:
            self.actions = torch.zeros((E, A), dtype=torch.float32, device=venv.device)
        out = self.action_traj if self.trajectory else self.actions
        g = ctypes.c_void_p()
        with torch.cuda.device(venv.device):
            check(lib().sng_graph_create_policy(
                venv._h, actor._p, None if self.noise is None else ctypes.c_void_p(self.noise.data_ptr()),
                ctypes.c_void_p(obs.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(reward.data_ptr()),
                ctypes.c_void_p(done.data_ptr()), ctypes.byref(venv._info),
                (_native.GRAPH_RESET if with_reset else 0) | (_native.GRAPH_STEP_NODES if step_nodes else 0)
                | (_native.GRAPH_TRAJECTORY if self.trajectory else 0)
                | (_native.GRAPH_POLICY_FUSED if fused else 0), self.days, dr, ctypes.byref(g)), venv._h)
        self._g = g

    @property
    def step_nodes(self):
        """Graph nodes that step one day: 1 in the fused form, 2 T in the node form (an actor and a step node per
        step)."""
        return int(lib().sng_graph_step_nodes(self._g))

    def launch(self, stream=None):
        if self.actor._p is None:   # the graph reads the actor's device image and its clipped-actions block
            raise RuntimeError("the actor was closed: a ClosedLoopGraph needs it for every launch")
        s = _stream_handle(self.venv.device) if stream is None else ctypes.c_void_p(stream)
        if self.trajectory and not self.with_reset:   # the loaded day's t = 0 observation, ahead of the graph
            if stream is None:
                self.obs_traj[0, 0].copy_(self.venv.obs_d)
            else:
                with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=self.venv.device)):
                    self.obs_traj[0, 0].copy_(self.venv.obs_d)
        check(lib().sng_graph_launch(self._g, s), self.venv._h)

    def close(self):
        if getattr(self, "_g", None):
            lib().sng_graph_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
