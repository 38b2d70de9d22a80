"""Shared by tests/test_policy_cpu.py and tests/test_gpu_policy.py: random actor weights, the actor evaluated in
float64 with numpy, and a bound on what float32 rounding may move."""
import numpy as np

HIDDEN = 64
U = 2.0 ** -24   # float32 unit roundoff


def random_weights(obs_dim, act_dim, seed, out_scale=1.0):
    """Uniform +-1 / sqrt(fan_in) weights and biases (torch's nn.Linear default) from a fixed seed, the last layer
    scaled by out_scale; no bias is -0."""
    rng = np.random.default_rng(seed)

    def layer(out, fan_in, scale=1.0):
        b = scale / np.sqrt(fan_in)
        return (rng.uniform(-b, b, (out, fan_in)).astype(np.float32), rng.uniform(-b, b, out).astype(np.float32))
    w1, b1 = layer(HIDDEN, obs_dim)
    w2, b2 = layer(HIDDEN, HIDDEN)
    w3, b3 = layer(act_dim, HIDDEN, out_scale)
    return [w1, b1, w2, b2, w3, b3]


def _act(activation, h):
    return np.tanh(h) if activation == "tanh" else np.where(h > 0, h, 0.0)


def actor_f64(obs, weights, activation, noise=None):
    """The network in float64: a = mean (+ noise), [rows, act_dim]."""
    w1, b1, w2, b2, w3, b3 = [np.asarray(w, np.float64) for w in weights]
    x = np.asarray(obs, np.float64)
    h1 = _act(activation, x @ w1.T + b1)
    h2 = _act(activation, h1 @ w2.T + b2)
    a = h2 @ w3.T + b3
    return a if noise is None else a + np.asarray(noise, np.float64)


def f32_rounding_bound(obs, weights, activation, noise=None):
    """An elementwise bound on |float32 fmaf-chain actor - actor_f64|, [rows, act_dim].

    A chain of K fmaf roundings started from the bias is off by at most K u (|b| + sum_k |in_k w_k|) to first order
    (every partial sum is bounded by that sum of magnitudes; 1.01 covers the higher-order terms, K u < 2e-5).  The
    activations are 1-Lipschitz, so a layer passes its input's error on through |W|; a float32 tanh adds at most 4
    units in the last place of a value below 1 (glibc's and the device library's are documented at 1-2 ulp), relu
    adds nothing.  The noise add is one more rounding."""
    w1, b1, w2, b2, w3, b3 = [np.abs(np.asarray(w, np.float64)) for w in weights]
    f = actor_layers_f64(obs, weights, activation)
    x, h1, h2 = np.abs(f[0]), np.abs(f[1]), np.abs(f[2])
    act_err = 4 * U if activation == "tanh" else 0.0
    e1 = 1.01 * w1.shape[1] * U * (x @ w1.T + b1) + act_err
    e2 = e1 @ w2.T + 1.01 * HIDDEN * U * (h1 @ w2.T + b2) + act_err
    e3 = e2 @ w3.T + 1.01 * HIDDEN * U * (h2 @ w3.T + b3)
    if noise is not None:
        e3 = e3 + U * (np.abs(actor_f64(obs, weights, activation, noise)) + e3)
    return e3


def actor_layers_f64(obs, weights, activation):
    w1, b1, w2, b2, w3, b3 = [np.asarray(w, np.float64) for w in weights]
    x = np.asarray(obs, np.float64)
    h1 = _act(activation, x @ w1.T + b1)
    h2 = _act(activation, h1 @ w2.T + b2)
    return x, h1, h2
