"""Shared by tests/test_policy_net_cpu.py and tests/test_gpu_policy_net.py: random weights for an actor of any two
hidden widths, the actor evaluated in float64 with numpy (mean or squashed output), SB3's unscale_action as numpy
evaluates it in float32, and tests/policy_cases.py's rounding bound generalised to per-layer widths."""
import numpy as np

U = 2.0 ** -24   # float32 unit roundoff

# the nets of the issue: SB3's DDPG / TD3 actor, PPO's, the narrowest, widths that are no multiple of a tile or of a
# weight group, the widest
NETS = [(400, 300), (64, 64), (8, 8), (33, 65), (512, 512)]
DDPG_KEYS = ("actor.mu.0.weight", "actor.mu.0.bias", "actor.mu.2.weight", "actor.mu.2.bias",
             "actor.mu.4.weight", "actor.mu.4.bias")


def random_net_weights(obs_dim, act_dim, net_arch, seed, out_scale=1.0):
    """Uniform +-1 / sqrt(fan_in) weights and biases (torch's nn.Linear default) from a fixed seed, the last layer
    scaled by out_scale; no bias is -0."""
    rng = np.random.default_rng(seed)
    h1, h2 = net_arch

    def layer(out, fan_in, scale=1.0):
        b = scale / np.sqrt(fan_in)
        return (rng.uniform(-b, b, (out, fan_in)).astype(np.float32), rng.uniform(-b, b, out).astype(np.float32))
    w1, b1 = layer(h1, obs_dim)
    w2, b2 = layer(h2, h1)
    w3, b3 = layer(act_dim, h2, out_scale)
    return [w1, b1, w2, b2, w3, b3]


def _act(activation, h):
    return np.tanh(h) if activation == "tanh" else np.where(h > 0, h, 0.0)


def net_layers_f64(obs, weights, activation):
    w1, b1, w2, b2, w3, b3 = [np.asarray(w, np.float64) for w in weights]
    x = np.asarray(obs, np.float64)
    h1 = _act(activation, x @ w1.T + b1)
    h2 = _act(activation, h1 @ w2.T + b2)
    return x, h1, h2


def net_f64(obs, weights, activation, noise=None, squash=False):
    """The network in float64, [rows, act_dim].  squash=False: a = mean (+ noise).  squash=True: a = tanh(mean),
    with noise clip(a + noise, -1, 1)."""
    w3, b3 = np.asarray(weights[4], np.float64), np.asarray(weights[5], np.float64)
    mean = net_layers_f64(obs, weights, activation)[2] @ w3.T + b3
    if not squash:
        return mean if noise is None else mean + np.asarray(noise, np.float64)
    s = np.tanh(mean)
    return s if noise is None else np.clip(s + np.asarray(noise, np.float64), -1.0, 1.0)


def unscale_f32(s, low, high):
    """SB3's unscale_action, low + (0.5 * (scaled_action + 1.0) * (high - low)), in numpy float32: every operation
    rounds on its own."""
    s, low, high = (np.asarray(x, np.float32) for x in (s, low, high))
    return low + (np.float32(0.5) * (s + np.float32(1.0)) * (high - low))


def net_f32_rounding_bound(obs, weights, activation, noise=None, squash=False):
    """An elementwise bound on |float32 fmaf-chain actor - net_f64|, [rows, act_dim]: tests/policy_cases.py's
    f32_rounding_bound with every layer's own K.

    A chain of K fmaf roundings started from the bias is off by at most K u (|b| + sum_k |in_k w_k|) to first order
    (1.01 covers the higher-order terms: K u < 4e-5 at K = 512).  The activations are 1-Lipschitz, so a layer passes
    its input's error on through |W|; a float32 tanh adds at most 4 units in the last place of a value below 1, relu
    adds nothing.  Mean output: the noise add is one more rounding.  Squashed output: tanh is 1-Lipschitz and adds
    its 4 u; the noise add is one more rounding of a value of at most 2 in magnitude before the clip, and the clip
    is 1-Lipschitz."""
    w1, b1, w2, b2, w3, b3 = [np.abs(np.asarray(w, np.float64)) for w in weights]
    f = net_layers_f64(obs, weights, activation)
    x, h1, h2 = np.abs(f[0]), np.abs(f[1]), np.abs(f[2])
    act_err = 4 * U if activation == "tanh" else 0.0
    e1 = 1.01 * w1.shape[1] * U * (x @ w1.T + b1) + act_err
    e2 = e1 @ w2.T + 1.01 * w2.shape[1] * U * (h1 @ w2.T + b2) + act_err
    e3 = e2 @ w3.T + 1.01 * w3.shape[1] * U * (h2 @ w3.T + b3)
    if squash:
        e3 = e3 + 4 * U
        if noise is not None:
            e3 = e3 + U * (1.0 + np.abs(np.asarray(noise, np.float64)) + e3)
    elif noise is not None:
        e3 = e3 + U * (np.abs(net_f64(obs, weights, activation, noise)) + e3)
    return e3
