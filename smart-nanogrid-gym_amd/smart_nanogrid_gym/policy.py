"""The policy in the loop: the MLP actors of the reference's own workloads, PPO("MlpPolicy", env)
(solvers/RL/ppo_train.py:92) and DDPG("MlpPolicy", env) (solvers/RL/ddpg_train.py), evaluated by the library between
steps.

`MlpActor` is the actor as a device kernel: by default the 64-64 tanh (or relu) actor of PPO (include/sng.h,
sng_policy_create); with another `net_arch` or `squash=True` an actor of any two hidden widths up to 512 on the
f32-input MFMA (sng_policy_create_net), whose squashed output is SB3's DDPG / TD3 / SAC actor: tanh, noise clipped in
[-1, 1], rescaled into the action Box.  It is a callable from observations to env actions, and the host model of the
same arithmetic.  `ClosedLoopGraph` captures whole days with the actor between the steps (sng_graph_create_policy),
so a rollout whose every action answers the observation before it is one graph launch, with no torch kernel in it.
`PpoHead` is the rest of what a PPO update reads, in one more kernel: the critic's values, the advantages and returns
and the log-probabilities of such a trajectory (sng_ppo_finish); with `net_arch=` its value net has any two hidden
widths up to 512 (sng_ppo_create_net: the value net on the f32-input MFMA over the trajectory's rows as one batch, then
a scan kernel).  `PpoRollout` is the graph and that finish as one object that holds what SB3's RolloutBuffer holds.
`ActionNoise` is the exploration noise those graphs add, drawn by the library (sng_noise_create): Gaussian or
Ornstein-Uhlenbeck blocks from counter-based streams with an exact host model, a new block per day and per launch.
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
# stable-baselines3's ActorCriticPolicy state_dict keys of the critic (value_net's two Linear layers and the value
# output) and of the Gaussian head's log standard deviations
SB3_VALUE_KEYS = ("mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias",
                  "mlp_extractor.value_net.2.weight", "mlp_extractor.value_net.2.bias",
                  "value_net.weight", "value_net.bias")
SB3_LOG_STD_KEY = "log_std"


def _stream_arg(device, stream):
    """The stream a call runs on: torch's current one of `device`, or the caller's raw handle."""
    return _stream_handle(device) if stream is None else ctypes.c_void_p(stream)


def _want(tensor, name, shape, dtype, device, message=None):
    """Refuses a tensor that is not contiguous, of this shape and dtype, on this device."""
    if tuple(tensor.shape) != shape or tensor.dtype != dtype or tensor.device != device or not tensor.is_contiguous():
        raise ValueError(message or f"{name} must be a contiguous {dtype} tensor {shape} on {device}")


class _Handle:
    """A library handle this object owns: close() destroys it once, __del__ closes.  A handle made for an env batch
    (_own) is closed by the batch before the batch itself: the library wants it destroyed before its env."""
    _slot = "_p"          # the attribute that holds the handle, None once closed
    _destroy = None       # the library's destroy call
    _sync_first = True    # kernels still running may read the handle's device buffers
    _closed = None        # what _check_open raises

    def _own(self, venv, handle):
        setattr(self, self._slot, handle)
        venv._actors.append(weakref.ref(self))

    def _check_open(self):
        if getattr(self, self._slot) is None:
            raise RuntimeError(self._closed)

    def close(self):
        if getattr(self, self._slot, None):
            if self._sync_first:
                torch.cuda.synchronize(self.venv.device)
            getattr(lib(), self._destroy)(getattr(self, self._slot))
            setattr(self, self._slot, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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


def prefixed_weights(state_dict, prefix, what="weights"):
    """The six entries `prefix`.{0,2,4}.{weight,bias} of a state_dict, in actor_weights' order: a three-layer
    nn.Sequential as SB3's TD3Policy names its nets (actor.mu, actor_target.mu, critic.qf0, critic_target.qf0)."""
    keys = [f"{prefix}.{layer}.{part}" for layer in (0, 2, 4) for part in ("weight", "bias")]
    missing = [k for k in keys if k not in state_dict]
    if missing:
        raise KeyError(f"{what}: missing {missing}")
    return [state_dict[k] for k in keys]


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


class MlpActor(_Handle):
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
    zero until load().  close() frees the actor's device image and buffers; graphs captured with the actor must not be
    launched afterwards."""
    _destroy = "sng_policy_destroy"

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
        self._own(venv, h)
        E = venv.num_envs
        self.actions_d = torch.zeros((E, self.act_dim), dtype=torch.float32, device=venv.device)
        self.env_actions_d = torch.zeros((E, self.act_dim), dtype=torch.float32, device=venv.device)
        self._obs_pad = None

    @classmethod
    def ddpg(cls, venv):
        """SB3's DDPG("MlpPolicy", env) actor: 400-300, relu, squashed into venv.action_space."""
        return cls(venv, activation="relu", net_arch=DDPG_NET_ARCH, squash=True)

    def load(self, weights, prefix=None):
        """Upload weights: six arrays or tensors (w1, b1, w2, b2, w3, b3 in torch's [out, in] layout) or a dict with
        SB3's actor keys (PPO's or DDPG's).  prefix: with a dict, the net's entries `prefix`.{0,2,4}.{weight,bias}
        instead, e.g. "actor_target.mu" for DDPG's target actor.  Graphs captured with this actor use them from their
        next launch on."""
        if prefix is not None and isinstance(weights, dict):
            weights = prefixed_weights(weights, prefix, "actor weights")
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

def value_weights(weights, obs_dim, net_arch=None):
    """The value net's six float32 arrays (w1 [h1, obs_dim], b1, w2 [h2, h1], b2, w3 [1, h2], b3 [1]; net_arch =
    (h1, h2), None: 64-64) from six arrays or tensors in that order, or from a dict holding stable-baselines3's
    ActorCriticPolicy keys (SB3_VALUE_KEYS, the same for every net_arch); other entries are ignored."""
    if isinstance(weights, dict):
        missing = [k for k in SB3_VALUE_KEYS if k not in weights]
        if missing:
            raise KeyError(f"value net weights: missing {missing}")
        weights = [weights[k] for k in SB3_VALUE_KEYS]
    return actor_weights(weights, obs_dim, 1, (HIDDEN, HIDDEN) if net_arch is None else net_arch)


def head_weights(weights, obs_dim, act_dim, log_std=None, net_arch=None):
    """(value net arrays, log_std float32 [act_dim]) of a PPO head whose value net has the widths net_arch (None:
    64-64).  A dict gives log_std under SB3's `log_std` key unless log_std is passed; with six arrays a log_std of
    None is zeros (SB3's log_std_init)."""
    if log_std is None:
        if isinstance(weights, dict):
            if SB3_LOG_STD_KEY not in weights:
                raise KeyError(f"ppo head: missing ['{SB3_LOG_STD_KEY}']")
            log_std = weights[SB3_LOG_STD_KEY]
        else:
            log_std = np.zeros(act_dim, np.float32)
    log_std = _as_f32(log_std).reshape(-1)
    if log_std.shape != (act_dim,):
        raise ValueError(f"log_std must have shape {(act_dim,)}, got {log_std.shape}")
    return value_weights(weights, obs_dim, net_arch), log_std


def _rollout_struct(days, gamma, gae_lambda, ptr, obs, reward, done, noise, values, advantages, returns, logp):
    p = lambda x: None if x is None else ptr(x)   # noqa: E731
    return _native.SngPpoRollout(int(days), float(gamma), float(gae_lambda), p(obs), p(reward), p(done), p(noise),
                                 p(values), p(advantages), p(returns), p(logp))


def ppo_host_finish(obs, reward, done, weights=None, log_std=None, noise=None, gamma=0.99, gae_lambda=0.95,
                    activation="tanh", values=None, net_arch=None):
    """What finishes a PPO rollout, on the CPU (sng_ppo_host_finish): (values [days, T + 1, E], advantages, returns
    [days, T, E], log_prob [days, T, E] or None without noise) for obs [days, T + 1, E, obs_dim], reward and done
    [days, T, E] and noise [T, E, act_dim].  weights / log_std: as head_weights takes them.  values: given, they are
    read instead of computed (obs and weights may then be None).  net_arch: None is the 64-64 head; a pair of widths
    is the net head's host model (sng_ppo_net_host_finish), which accepts what sng_ppo_create_net accepts.  Needs no
    GPU."""
    arch = None if net_arch is None else _net_arch(net_arch)
    reward = np.ascontiguousarray(reward, dtype=np.float64)
    done = np.ascontiguousarray(done, dtype=np.uint8)
    days, T, E = reward.shape
    if done.shape != reward.shape:
        raise ValueError(f"done must have shape {reward.shape}")
    given = values is not None
    if obs is not None:
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        if obs.ndim != 4 or obs.shape[:3] != (days, T + 1, E):
            raise ValueError(f"obs must have shape {(days, T + 1, E, 'obs_dim')}")
    elif not given:
        raise ValueError("obs is needed where the values are not given")
    if noise is not None:
        noise = np.ascontiguousarray(noise, dtype=np.float32)
        if noise.ndim != 3 or noise.shape[:2] != (T, E):
            raise ValueError(f"noise must have shape {(T, E, 'act_dim')}")
        act_dim = noise.shape[2]
    else:   # no log-probability stage: log_std is not read
        act_dim, log_std = 1, np.zeros(1, np.float32)
    if obs is not None:
        obs_dim = obs.shape[3]
    elif weights is not None:
        obs_dim = np.shape(weights[SB3_VALUE_KEYS[0]] if isinstance(weights, dict) else weights[0])[1]
    else:
        obs_dim = 1
    w = None
    if weights is not None:
        arrs, log_std = head_weights(weights, obs_dim, act_dim, log_std, arch)
        w = ctypes.byref(_weights_struct(arrs))
    else:
        log_std = np.zeros(act_dim, np.float32) if log_std is None else _as_f32(log_std).reshape(act_dim)
    if given:
        vals = np.ascontiguousarray(values, dtype=np.float32).copy()
        if vals.shape != (days, T + 1, E):
            raise ValueError(f"values must have shape {(days, T + 1, E)}")
    else:
        vals = np.zeros((days, T + 1, E), np.float32)
    adv, ret = np.zeros((days, T, E), np.float32), np.zeros((days, T, E), np.float32)
    logp = None if noise is None else np.zeros((days, T, E), np.float32)
    r = _rollout_struct(days, gamma, gae_lambda, lambda x: x.ctypes.data, obs, reward, done, noise, vals, adv, ret, logp)
    ls = None if log_std is None else log_std.ctypes.data_as(_native.c_float_p)
    if arch is None:
        check(lib().sng_ppo_host_finish(obs_dim, act_dim, ACTIVATIONS[activation], T, E, w, ls, ctypes.byref(r),
                                        1 if given else 0))
    else:
        spec = _native.SngPpoNetSpec(arch[0], arch[1], ACTIVATIONS[activation])
        check(lib().sng_ppo_net_host_finish(obs_dim, act_dim, ctypes.byref(spec), T, E, w, ls, ctypes.byref(r),
                                            1 if given else 0))
    return vals, adv, ret, logp


class PpoHead(_Handle):
    """What a PPO update reads beside the trajectory, on the device (include/sng.h, sng_ppo_create): the 64-64 value
    net of SB3's MlpPolicy with the actor's activation, the Gaussian head's log_std, and one kernel
    (rollout_gae_kernel) from a trajectory to critic values, advantages, returns and log-probabilities.  The weights
    are zero until load().

    net_arch -- None: that head.  A pair of hidden widths, each 8 .. 512 (the `vf` of SB3's net_arch): a value net of
                those widths (sng_ppo_create_net), whose finish() is two launches: value_net_kernel on the f32-input
                MFMA over the trajectory's days (T + 1) E rows as one batch, then gae_scan_kernel.  (64, 64) takes
                this path too: the same results by value, for cross-checking the two.  Widths whose LDS tiles do
                not fit a compute unit at this station are refused (NativeError, libsng error -2).
    close() frees the head's device image."""
    _destroy = "sng_ppo_destroy"
    _closed = "the PPO head is closed"

    def __init__(self, venv, activation="tanh", net_arch=None):
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}")
        self.venv = venv
        self.activation = activation
        self.net_arch = None if net_arch is None else _net_arch(net_arch)
        self.obs_dim, self.act_dim = venv.obs_dim, venv.act_dim
        self.weights = self.log_std = None
        h = ctypes.c_void_p()
        if self.net_arch is None:
            check(lib().sng_ppo_create(venv._h, ACTIVATIONS[activation], ctypes.byref(h)), venv._h)
        else:
            spec = _native.SngPpoNetSpec(self.net_arch[0], self.net_arch[1], ACTIVATIONS[activation])
            check(lib().sng_ppo_create_net(venv._h, ctypes.byref(spec), ctypes.byref(h)), venv._h)
        self._own(venv, h)
        self._out = {}   # days -> (values, advantages, returns, log_prob)

    def load(self, weights, log_std=None):
        """Upload the value net and log_std: a dict with SB3's keys (mlp_extractor.value_net.*, value_net.*, log_std;
        the rest is ignored), or six arrays in actor_weights' order with act_dim = 1 (and this head's net_arch) and
        log_std [act_dim] (None: zeros).  They take effect at the next finish()."""
        arrs, ls = head_weights(weights, self.obs_dim, self.act_dim, log_std, self.net_arch)
        self._check_open()
        w = _weights_struct(arrs)
        with torch.cuda.device(self.venv.device):
            check(lib().sng_ppo_set_weights(self._p, ctypes.byref(w), ls.ctypes.data_as(_native.c_float_p),
                                            _stream_handle(self.venv.device)), self.venv._h)
        self.weights, self.log_std = arrs, ls
        return self

    def _outputs(self, days):
        if days not in self._out:
            T, E, dev = self.venv.timesteps, self.venv.num_envs, self.venv.device
            # empty, not zeros: the kernel writes every element, and a fill on torch's current stream would not be
            # ordered against a launch on a caller's stream
            self._out[days] = (torch.empty((days, T + 1, E), dtype=torch.float32, device=dev),) + tuple(
                torch.empty((days, T, E), dtype=torch.float32, device=dev) for _ in range(3))
        return self._out[days]

    def finish(self, obs_traj, reward_traj, done_traj, noise=None, gamma=0.99, gae_lambda=0.95, stream=None):
        """(values [days, T + 1, E], advantages, returns, log_prob [days, T, E]) as device tensors this head owns
        (overwritten by the next finish() of as many days), from obs_traj [days, T + 1, E, obs_dim] float32,
        reward_traj float64 and done_traj uint8 [days, T, E] and the noise [T, E, act_dim] the actor added; without
        noise log_prob is None.  One kernel launch (two for a head with net_arch) on torch's current stream (or
        `stream`), no synchronisation."""
        self._check_open()
        T, E, dev = self.venv.timesteps, self.venv.num_envs, self.venv.device
        days = int(obs_traj.shape[0])
        _want(obs_traj, "obs_traj", (days, T + 1, E, self.obs_dim), torch.float32, dev)
        _want(reward_traj, "reward_traj", (days, T, E), torch.float64, dev)
        _want(done_traj, "done_traj", (days, T, E), torch.uint8, dev)
        if noise is not None:
            _want(noise, "noise", (T, E, self.act_dim), torch.float32, dev)
        values, adv, ret, logp = self._outputs(days)
        if noise is None:
            logp = None
        self._finish_into(days, obs_traj, reward_traj, done_traj, noise, gamma, gae_lambda, values, adv, ret, logp, stream)
        return values, adv, ret, logp

    def _finish_into(self, days, obs, reward, done, noise, gamma, gae_lambda, values, adv, ret, logp, stream):
        """sng_ppo_finish of `days` days into the caller's output rows; nothing is checked here."""
        dev = self.venv.device
        r = _rollout_struct(days, gamma, gae_lambda, lambda x: x.data_ptr(), obs, reward, done, noise, values, adv, ret,
                            logp)
        with torch.cuda.device(dev):
            check(lib().sng_ppo_finish(self._p, ctypes.byref(r), _stream_arg(dev, stream)), self.venv._h)

    def host_finish(self, obs_traj, reward_traj, done_traj, noise=None, gamma=0.99, gae_lambda=0.95, values=None):
        """The host model on numpy arrays or tensors: ppo_host_finish with this head's weights."""
        if self.weights is None:
            raise RuntimeError("load() the head's weights first")
        return ppo_host_finish(_as_f32(obs_traj), _np(reward_traj), _np(done_traj), self.weights, self.log_std,
                               None if noise is None else _as_f32(noise), gamma, gae_lambda, self.activation,
                               None if values is None else _as_f32(values), net_arch=self.net_arch)

def _np(x):
    if torch is not None and isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


NOISE_KINDS = {"gaussian": _native.NOISE_GAUSSIAN, "ou": _native.NOISE_OU}


def _per_action(x, act_dim, name):
    x = _as_f32(x)
    if x.ndim > 1 or (x.ndim == 1 and x.shape[0] not in (1, act_dim)):
        raise ValueError(f"{name} must be a scalar or have shape {(act_dim,)}, got {x.shape}")
    return np.ascontiguousarray(np.broadcast_to(x, (act_dim,)))


def _noise_spec(kind, act_dim, seed, theta, dt):
    if kind not in NOISE_KINDS:
        raise ValueError(f"kind must be one of {sorted(NOISE_KINDS)}")
    return _native.SngNoiseSpec(NOISE_KINDS[kind], int(act_dim), int(seed), float(theta), float(dt))


def noise_host_fill(kind, act_dim, timesteps, num_envs, days=1, seed=0, mu=0.0, scale=1.0, theta=0.15, dt=1e-2,
                    env_offset=0, counter=0):
    """The action noise's host model (sng_noise_host_fill): float32 [days, timesteps, num_envs, act_dim], the blocks
    of counters counter, counter + 1, .. that an ActionNoise with these parameters gives the global envs env_offset ..
    env_offset + num_envs - 1.  mu and scale: scalars or [act_dim].  Needs no GPU."""
    spec = _noise_spec(kind, act_dim, seed, theta, dt)
    A = max(int(act_dim), 1)
    mu, scale = _per_action(mu, A, "mu"), _per_action(scale, A, "scale")
    out = np.zeros((max(int(days), 0), max(int(timesteps), 0), max(int(num_envs), 0), A), np.float32)
    F = _native.c_float_p
    check(lib().sng_noise_host_fill(ctypes.byref(spec), mu.ctypes.data_as(F), scale.ctypes.data_as(F), int(timesteps),
                                    int(num_envs), int(env_offset), int(counter), int(days), out.ctypes.data_as(F)))
    return out


class ActionNoise(_Handle):
    """The exploration noise of `venv`'s envs, drawn on the device (include/sng.h, sng_noise_create): one kernel fills
    whole days' blocks [T, E, act_dim] from counter-based streams keyed by (seed, global env, action, counter, step), so
    a sharded population draws what one population draws, every block has an exact CPU model (host_fill), and a
    captured graph (ClosedLoopGraph(noise=source), PpoRollout(noise=source)) explores with a new sample every day
    and every replay.

    kind  -- "gaussian": n = mu + scale * z, PPO's sample with scale = exp(log_std) and SB3's NormalActionNoise(mean,
             sigma); "ou": SB3's OrnsteinUhlenbeckActionNoise(mean, sigma, theta, dt), restarted from 0 every day
    seed  -- of the streams; the source's own, apart from the env's
    mu, scale -- scalars or [act_dim]; set() replaces them, also between two launches of a captured graph
    theta, dt -- of the OU process (SB3's defaults)
    `counter` is the number of blocks drawn so far: the next fill starts there.  Reading or setting it synchronises.
    close() frees the source's device buffers; graphs captured with the source must not be launched afterwards."""
    _destroy = "sng_noise_destroy"
    _closed = "the noise source is closed"

    def __init__(self, venv, kind="gaussian", seed=0, mu=0.0, scale=1.0, theta=0.15, dt=1e-2):
        self.venv, self.kind, self.seed = venv, kind, int(seed)
        self.theta, self.dt = float(theta), float(dt)
        self.act_dim = venv.act_dim
        self._spec = _noise_spec(kind, self.act_dim, seed, theta, dt)
        self._p = None
        h = ctypes.c_void_p()
        with torch.cuda.device(venv.device):
            check(lib().sng_noise_create(venv._h, ctypes.byref(self._spec), ctypes.byref(h)), venv._h)
        self._own(venv, h)
        self._out = {}   # days -> tensor
        self.mu = self.scale = None
        self.set(mu, scale)

    def set(self, mu, scale):
        """Upload new per-action mu and scale (scalars or [act_dim]); they take effect at the next fill or launch."""
        self._check_open()
        mu, scale = _per_action(mu, self.act_dim, "mu"), _per_action(scale, self.act_dim, "scale")
        F = _native.c_float_p
        with torch.cuda.device(self.venv.device):
            check(lib().sng_noise_set_params(self._p, mu.ctypes.data_as(F), scale.ctypes.data_as(F),
                                             _stream_handle(self.venv.device)), self.venv._h)
        self.mu, self.scale = mu, scale
        return self

    def fill(self, days=1, out=None, stream=None):
        """`days` new blocks as a device tensor [days, T, E, act_dim] this source owns (overwritten by the next fill
        of as many days), or into `out`; two launches on torch's current stream (or `stream`), no synchronisation."""
        self._check_open()
        venv = self.venv
        shape = (int(days), venv.timesteps, venv.num_envs, self.act_dim)
        if out is None:
            if days not in self._out and int(days) >= 1:
                self._out[days] = torch.empty(shape, dtype=torch.float32, device=venv.device)
            out = self._out.get(days)
        else:
            _want(out, "out", shape, torch.float32, venv.device,
                  f"out must be a contiguous float32 tensor {shape} on {venv.device}")
        with torch.cuda.device(venv.device):
            check(lib().sng_noise_fill(self._p, None if out is None else ctypes.c_void_p(out.data_ptr()), int(days),
                                       _stream_arg(venv.device, stream)), venv._h)
        return out

    def host_fill(self, days=1, counter=None):
        """The host model of the blocks a fill of `days` gives from `counter` on (None: the source's current counter)
        with the current mu and scale: numpy float32 [days, T, E, act_dim]."""
        venv = self.venv
        return noise_host_fill(self.kind, self.act_dim, venv.timesteps, venv.num_envs, days, self.seed, self.mu,
                               self.scale, self.theta, self.dt, venv.env_offset,
                               self.counter if counter is None else counter)

    @property
    def counter(self):
        self._check_open()
        c = ctypes.c_uint64()
        with torch.cuda.device(self.venv.device):
            check(lib().sng_noise_get_counter(self._p, ctypes.byref(c), _stream_handle(self.venv.device)), self.venv._h)
        return int(c.value)

    @counter.setter
    def counter(self, value):
        self._check_open()
        with torch.cuda.device(self.venv.device):
            check(lib().sng_noise_set_counter(self._p, int(value), _stream_handle(self.venv.device)), self.venv._h)

class PpoRollout:
    """A PPO iteration's rollout as one object: `days` closed-loop days (a ClosedLoopGraph with trajectory=True) and
    the head's finishing kernel behind them on the same stream.  After launch() it holds what SB3's RolloutBuffer
    holds, as device tensors: obs [days, T + 1, E, obs_dim] (obs[d, T] is the observation last_values answers),
    actions [days, T, E, act_dim], rewards, episode_starts, advantages, returns, log_prob [days, T, E] and values
    [days, T + 1, E].  `noise` [T, E, act_dim] is the Gaussian head's sample, reused every day, which the caller
    fills before a launch (noise.normal_() scaled by exp(log_std)).  With noise=<a gaussian ActionNoise> the library
    draws it instead: `noise` is then [days, T, E, act_dim], one block per day, new at every launch; load() also sets
    the source's scale to exp(log_std) (numpy float32); launch() runs the graph and one finish per day on that day's
    blocks, so log_prob[d] is of day d's own noise.  PPO's Gaussian head is the mean output: a
    squashed actor is refused.  With the default head the actor is 64-64 too; with a head built with net_arch= the
    actor is any mean-output MlpActor, of any widths (SB3's net_arch=dict(pi=..., vf=...) lets the two differ).  New
    weights (load(), or the actor's and the head's own load()) take effect at the next launch, without a recapture."""

    def __init__(self, venv, actor, head, days=1, gamma=0.99, gae_lambda=0.95, with_reset=True, noise=None):
        if noise is not None and (not isinstance(noise, ActionNoise) or noise.kind != "gaussian"):
            raise ValueError("PpoRollout's noise is None (the caller fills `noise`) or a gaussian ActionNoise")
        if head.net_arch is None:
            if actor.squash or actor.net_arch != (HIDDEN, HIDDEN):
                raise ValueError("PpoRollout needs PPO's actor: 64-64 with the mean output (no squash, no other net_arch)")
        elif actor.squash:
            raise ValueError("PpoRollout needs a mean-output actor: the log-probabilities are of a = mean + noise, "
                             "which a squashed actor (tanh, noise clipped in [-1, 1]) does not compute")
        if head.venv is not venv:
            raise ValueError("the head was made for another env batch")
        if head._p is None:
            raise ValueError("the head is closed")
        self.venv, self.actor, self.head = venv, actor, head
        self.days, self.gamma, self.gae_lambda = int(days), float(gamma), float(gae_lambda)
        T, E, A = venv.timesteps, venv.num_envs, venv.act_dim
        self.noise_source = noise
        if noise is None:
            self.noise = torch.zeros((T, E, A), dtype=torch.float32, device=venv.device)
            self.graph = ClosedLoopGraph(venv, actor, noise=self.noise, days=self.days, with_reset=with_reset,
                                         trajectory=True)
            if self.graph.noise.data_ptr() != self.noise.data_ptr():   # the log-probs must be of the noise the actor adds
                raise RuntimeError("the closed-loop graph took a copy of the noise tensor")
        else:   # the source's blocks, one per day: [days, T, E, A]
            self.graph = ClosedLoopGraph(venv, actor, noise=noise, days=self.days, with_reset=with_reset, trajectory=True)
            self.noise = self.graph.noise_traj
        self.values = self.advantages = self.returns = self.log_prob = None

    obs = property(lambda self: self.graph.obs_traj)
    actions = property(lambda self: self.graph.action_traj)
    rewards = property(lambda self: self.graph.reward_traj)
    dones = property(lambda self: self.graph.done_traj)

    @property
    def episode_starts(self):
        """uint8 [days, T, E]: 1 at a day's first step, else the done of the step before."""
        starts = torch.ones_like(self.graph.done_traj)
        starts[:, 1:] = self.graph.done_traj[:, :-1]
        return starts

    def load(self, state_dict):
        """Actor, value net and log_std from one SB3 ActorCriticPolicy state_dict."""
        self.actor.load(state_dict)
        self.head.load(state_dict)
        if self.noise_source is not None:   # the Gaussian head's sample: scale = exp(log_std), in float32
            self.noise_source.set(self.noise_source.mu, np.exp(self.head.log_std.astype(np.float32)).astype(np.float32))
        return self

    def launch(self, stream=None):
        """The graph launch and the finishing kernel, on one stream; no synchronisation."""
        if self.head._p is None:
            raise RuntimeError("the PPO head was closed: a PpoRollout needs it for every launch")
        g = self.graph
        g.launch(stream)
        if self.noise_source is None:
            self.values, self.advantages, self.returns, self.log_prob = self.head.finish(
                g.obs_traj, g.reward_traj, g.done_traj, self.noise, self.gamma, self.gae_lambda, stream=stream)
            return
        # one finish per day (sng_ppo_finish with days = 1), on that day's blocks and that day's noise, straight into
        # day d's rows of the head's [days, ..] outputs
        vals, adv, ret, logp = self.head._outputs(self.days)
        for d in range(self.days):
            self.head._finish_into(1, g.obs_traj[d], g.reward_traj[d], g.done_traj[d], self.noise[d], self.gamma,
                                   self.gae_lambda, vals[d], adv[d], ret[d], logp[d], stream)
        self.values, self.advantages, self.returns, self.log_prob = vals, adv, ret, logp

    def close(self):
        self.graph.close()


class ClosedLoopGraph(_Handle):
    """Whole days with the actor in the loop, captured once as a hipGraph and replayed: ([device-RNG reset] + T x
    (actor, step)) x days (include/sng.h, sng_graph_create_policy).

    noise      -- optional device tensor [T, E, act_dim] added to the actor's mean (to tanh(mean) for a squashed
                  actor: DDPG's action noise, e.g. a precomputed Ornstein-Uhlenbeck path), reused every day; or an
                  ActionNoise: the graph then begins with the source's fill of noise_traj [days, T, E, act_dim]
                  (sng_graph_create_policy_noise), day d's actor reads noise_traj[d], and every launch draws new
                  blocks
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
    _slot, _destroy, _sync_first = "_g", "sng_graph_destroy", False

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
        self.noise = self.noise_source = self.noise_traj = None
        if isinstance(noise, ActionNoise):
            if noise.venv is not venv:
                raise ValueError("the noise source was made for another env batch")
            if noise._p is None:
                raise ValueError("the noise source is closed")
            self.noise_source = noise
            self.noise_traj = torch.zeros((self.days, T, E, A), dtype=torch.float32, device=venv.device)
        elif noise is not None:
            self.noise = noise.to(device=venv.device, dtype=torch.float32).contiguous()
            if tuple(self.noise.shape) != (T, E, A):
                raise ValueError(f"noise must have shape {(T, E, A)}")
        self.day_returns = day_returns
        dr = None
        if day_returns is not None:
            _want(day_returns, "day_returns", (self.days, E), torch.float64, venv.device,
                  "day_returns must be a contiguous float64 device tensor [days, num_envs]")
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
        flags = ((_native.GRAPH_RESET if with_reset else 0) | (_native.GRAPH_STEP_NODES if step_nodes else 0)
                 | (_native.GRAPH_TRAJECTORY if self.trajectory else 0) | (_native.GRAPH_POLICY_FUSED if fused else 0))
        rest = (ctypes.c_void_p(obs.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(reward.data_ptr()),
                ctypes.c_void_p(done.data_ptr()), ctypes.byref(venv._info), flags, self.days, dr, ctypes.byref(g))
        with torch.cuda.device(venv.device):
            if self.noise_source is not None:
                check(lib().sng_graph_create_policy_noise(venv._h, actor._p, self.noise_source._p,
                                                          ctypes.c_void_p(self.noise_traj.data_ptr()), *rest), venv._h)
            else:
                check(lib().sng_graph_create_policy(
                    venv._h, actor._p, None if self.noise is None else ctypes.c_void_p(self.noise.data_ptr()), *rest),
                    venv._h)
        self._g = g

    @property
    def step_nodes(self):
        """Graph nodes that step one day: 1 in the fused form, 2 T in the node form (an actor and a step node per
        step)."""
        return int(lib().sng_graph_step_nodes(self._g))

    def describe(self):
        """The captured graph as text (sng_graph_describe): a line per node with its kernel, geometry and edges."""
        return _native.graph_describe(self._g)

    def launch(self, stream=None):
        if self.actor._p is None:   # the graph reads the actor's device image and its clipped-actions block
            raise RuntimeError("the actor was closed: a ClosedLoopGraph needs it for every launch")
        if self.noise_source is not None and self.noise_source._p is None:   # ... and the source's counter
            raise RuntimeError("the noise source was closed: a ClosedLoopGraph needs it for every launch")
        if self.trajectory and not self.with_reset:   # the loaded day's t = 0 observation, ahead of the graph
            if stream is None:
                self.obs_traj[0, 0].copy_(self.venv.obs_d)
            else:
                with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=self.venv.device)):
                    self.obs_traj[0, 0].copy_(self.venv.obs_d)
        check(lib().sng_graph_launch(self._g, _stream_arg(self.venv.device, stream)), self.venv._h)
