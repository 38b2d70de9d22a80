"""What finishes a PPO rollout (sng_ppo_*, policy.PpoHead / PpoRollout), without a GPU: the host model of
csrc/sng_ppo_host.h against naive loops (a stand-alone g++ program, bitwise; once more under the host sanitizers),
the advantages against a numpy float32 restatement of SB3's compute_returns_and_advantage, the values against the
existing sng_policy_host_actions with act_dim = 1, the log-probabilities against torch.distributions in float64
within a derived bound, every refusal through the host entry point, and the loading of an SB3 state_dict."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from policy_cases import random_weights
from smart_nanogrid_gym import _native, policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smart-nanogrid-gym_amd", "csrc")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", CSRC]
SOURCE = os.path.join(ROOT, "tests", "native", "ppo_host_check.cpp")
# 3 obs_dim x 3 act_dim x 2 activations x (T = 12, 24): 2 days x 7 envs x ((T + 1) values + T x (adv, ret, logp))
OUTPUTS = 3 * 3 * 2 * sum(2 * 7 * ((T + 1) + 3 * T) for T in (12, 24))
U = 2.0 ** -24

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _run_native(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *extra, *INCLUDES, SOURCE, "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ppo host ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    assert int(out.stdout.split()[-2]) == OUTPUTS


@needs_gxx
def test_host_model_equals_naive_loops_bitwise(tmp_path):
    """Plain g++, no ROCm on the include path: ppo_gae_host and ppo_logp_host against naive loops, the value path
    against mlp_actor_host with A = 1 and against a naive chain."""
    _run_native(tmp_path, "ppo_host_check", ["-O2"])


@needs_gxx
def test_host_model_under_the_host_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined, run directly."""
    _run_native(tmp_path, "ppo_host_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


# ------------------------------------------------------------------------------------------------ GAE against numpy
def random_done(rng, days, T, E):
    """Terminal flags with both values at a day's last step and mid-day (what the env itself never gives)."""
    return (rng.random((days, T, E)) < 0.2).astype(np.uint8)


def sb3_gae(rewards, dones, values, last_values, gamma, gae_lambda):
    """RolloutBuffer.compute_returns_and_advantage restated: float32 buffers [steps, E], Python-float gamma and
    gae_lambda, episode_starts[step + 1] = dones[step], `dones` after the last step being the last step's done."""
    rewards = rewards.astype(np.float32)
    steps = rewards.shape[0]
    episode_starts = np.concatenate([np.zeros((1,) + dones.shape[1:], np.float32), dones[:-1].astype(np.float32)])
    advantages = np.zeros_like(rewards)
    last_gae_lam = 0
    for step in reversed(range(steps)):
        if step == steps - 1:
            next_non_terminal = 1.0 - dones[-1].astype(np.float32)
            next_values = last_values
        else:
            next_non_terminal = 1.0 - episode_starts[step + 1]
            next_values = values[step + 1]
        delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
        advantages[step] = last_gae_lam
    assert advantages.dtype == np.float32
    return advantages, advantages + values


def per_day_gae(reward, done, values, gamma, gae_lambda):
    adv, ret = np.zeros(reward.shape, np.float32), np.zeros(reward.shape, np.float32)
    for d in range(reward.shape[0]):
        adv[d], ret[d] = sb3_gae(reward[d], done[d], values[d, :-1], values[d, -1], gamma, gae_lambda)
    return adv, ret


@pytest.mark.parametrize("T", [24, 12])
def test_gae_equals_numpys_float32_sb3_loop_bitwise(T):
    E, days = 70, 2
    rng = np.random.default_rng(T)
    reward = -40.0 * rng.random((days, T, E))
    values = rng.normal(-60, 40, (days, T + 1, E)).astype(np.float32)
    done = random_done(rng, days, T, E)
    assert set(np.unique(done[:, -1])) == {0, 1} and set(np.unique(done[:, :-1])) == {0, 1}
    assert 0.05 < done.mean() < 0.5
    for gamma, lam in ((0.99, 0.95), (0.9, 1.0), (1.0, 0.0)):
        _, adv, ret, logp = policy.ppo_host_finish(None, reward, done, gamma=gamma, gae_lambda=lam, values=values)
        want_adv, want_ret = per_day_gae(reward, done, values, gamma, lam)
        assert logp is None
        assert adv.tobytes() == want_adv.tobytes() and ret.tobytes() == want_ret.tobytes(), (gamma, lam)
    # the env's own pattern: done only at a day's last step; then the days are one SB3 scan over 2 T steps
    env_done = np.zeros((days, T, E), np.uint8)
    env_done[:, -1] = 1
    _, adv, ret, _ = policy.ppo_host_finish(None, reward, env_done, values=values)
    want_adv, want_ret = per_day_gae(reward, env_done, values, 0.99, 0.95)
    assert adv.tobytes() == want_adv.tobytes() and ret.tobytes() == want_ret.tobytes()
    flat = lambda x: x.reshape(days * T, E)   # noqa: E731
    scan_adv, scan_ret = sb3_gae(flat(reward), flat(env_done), flat(values[:, :-1]), values[-1, -1], 0.99, 0.95)
    assert flat(adv).tobytes() == scan_adv.tobytes() and flat(ret).tobytes() == scan_ret.tobytes()
    assert np.unique(adv).size > adv.size // 2


# ---------------------------------------------------------------------------- values against the existing entry point
@pytest.mark.parametrize("activation", ["relu", "tanh"])
@pytest.mark.parametrize("obs_dim", [5, 25, 109])
def test_values_equal_the_actor_entry_point_with_one_action(obs_dim, activation):
    days, T, E = 2, 3, 9
    rng = np.random.default_rng(obs_dim)
    weights = random_weights(obs_dim, 1, seed=21, out_scale=30.0)
    obs = rng.uniform(0, 1, (days, T + 1, E, obs_dim)).astype(np.float32)
    reward, done = -rng.random((days, T, E)), random_done(rng, days, T, E)
    values, adv, ret, _ = policy.ppo_host_finish(obs, reward, done, weights, activation=activation)
    want, _ = policy.host_actions(obs.reshape(-1, obs_dim), weights, activation)
    assert values.tobytes() == want.reshape(days, T + 1, E).tobytes()
    assert np.unique(values).size > values.size // 2
    _, adv2, ret2, _ = policy.ppo_host_finish(None, reward, done, values=values)
    assert adv.tobytes() == adv2.tobytes() and ret.tobytes() == ret2.tobytes()


# ---------------------------------------------------------------------------------------- log-prob against float64
@pytest.mark.parametrize("act_dim", [2, 9, 51])
def test_log_prob_agrees_with_float64_normal(act_dim):
    """|lp - lp64| <= (A + 8) 2^-24 S with S = sum_j (0.5 z_j^2 + |log_std_j| + 0.919): inv_std is within 2 ulp
    (libm's expf <= 1 ulp, plus the divide), which gives 7 ulp on the square term; two subtractions; and A - 1
    additions of partial sums that are each <= S.  Largest observed ratio of the host model's error to the
    bound: 0.206 (A = 2), 0.103 (A = 9), 0.035 (A = 51)."""
    torch = pytest.importorskip("torch")
    days, T, E = 1, 24, 70
    rng = np.random.default_rng(act_dim)
    log_std = rng.uniform(-2.0, 0.5, act_dim).astype(np.float32)
    noise = (rng.normal(0, 1, (T, E, act_dim)) * np.exp(log_std.astype(np.float64))).astype(np.float32)
    reward, done = np.zeros((days, T, E)), np.zeros((days, T, E), np.uint8)
    values = np.zeros((days, T + 1, E), np.float32)
    _, _, _, lp = policy.ppo_host_finish(None, reward, done, log_std=log_std, noise=noise, values=values)
    std64 = torch.from_numpy(log_std.astype(np.float64)).exp()
    lp64 = torch.distributions.Normal(torch.zeros(act_dim, dtype=torch.float64), std64).log_prob(
        torch.from_numpy(noise.astype(np.float64))).sum(-1).numpy()
    z = noise.astype(np.float64) / np.exp(log_std.astype(np.float64))
    S = (0.5 * z * z + np.abs(log_std.astype(np.float64)) + 0.919).sum(-1)
    bound = (act_dim + 8) * U * S
    err = np.abs(lp[0].astype(np.float64) - lp64)
    print(f"A = {act_dim}: max |lp - lp64| {err.max():.3e}, largest ratio to the bound {(err / bound).max():.3f}")
    assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------------------- refusals
def _host_rc(weights, log_std, obs_dim=11, act_dim=3, activation=1, T=4, E=5, given=0, arrays=None, **rollout):
    """sng_ppo_host_finish's return code on zero-filled arrays of the right shapes; `arrays` replaces some of them by
    the caller's own, `rollout` overrides fields of the SngPpoRollout (None: a NULL pointer)."""
    days = max(rollout.get("days", 2), 1)
    F = _native.c_float_p
    bufs = dict(obs=np.zeros((days, T + 1, E, obs_dim), np.float32), reward=np.zeros((days, T, E)),
                done=np.zeros((days, T, E), np.uint8), noise=np.zeros((T, E, act_dim), np.float32),
                values=np.zeros((days, T + 1, E), np.float32), advantages=np.zeros((days, T, E), np.float32),
                returns=np.zeros((days, T, E), np.float32), logp=np.zeros((days, T, E), np.float32))
    bufs.update(arrays or {})
    f = dict(days=2, gamma=0.99, gae_lambda=0.95, **{k: v.ctypes.data for k, v in bufs.items()})
    f.update(rollout)
    r = _native.SngPpoRollout(*[f[name] for name, _ in _native.SngPpoRollout._fields_])
    w = None if weights is None else ctypes.byref(_native.SngMlpWeights(*[x.ctypes.data_as(F) for x in weights]))
    return _native.lib().sng_ppo_host_finish(obs_dim, act_dim, activation, T, E, w,
                                             None if log_std is None else log_std.ctypes.data_as(F), ctypes.byref(r),
                                             given)


def test_refusals_through_the_host_entry_point():
    good = random_weights(11, 1, seed=1)
    ls = np.array([0.0, -1.0, 0.5], np.float32)
    err = lambda: _native.lib().sng_last_error(None)   # noqa: E731
    assert _host_rc(good, ls) == 0 and _host_rc(good, None) == 0
    for part, bad in ((0, np.nan), (2, np.inf), (3, -np.inf), (4, np.nan), (5, np.inf)):
        w = [x.copy() for x in good]
        w[part].flat[w[part].size - 1] = bad
        assert _host_rc(w, ls) == -1 and b"non-finite value net weight" in err(), (part, bad)
    for bad in (np.nan, np.inf, -np.inf):
        assert _host_rc(good, np.array([0.0, bad, 0.0], np.float32)) == -1 and b"non-finite log_std" in err()
        assert _host_rc(None, np.array([0.0, bad, 0.0], np.float32), given=1) == -1
    assert _host_rc(None, ls) == -1 and b"null" in err()              # values to be computed, no value net
    assert _host_rc(None, ls, given=1) == 0
    for bad in (-0.01, 1.01, np.nan, np.inf):
        assert _host_rc(good, ls, gamma=bad) == -1 and b"gamma" in err(), bad
        assert _host_rc(good, ls, gae_lambda=bad) == -1 and b"gae_lambda" in err(), bad
    assert _host_rc(good, ls, gamma=0.0, gae_lambda=1.0) == 0 and _host_rc(good, ls, gamma=1.0, gae_lambda=0.0) == 0
    assert _host_rc(good, ls, days=0) == -1 and b"days" in err()
    assert _host_rc(good, ls, days=-3) == -1
    for name in ("obs", "reward", "done", "values", "advantages", "returns"):
        assert _host_rc(good, ls, **{name: None}) == -1 and b"null" in err(), name
    assert _host_rc(good, ls, obs=None, given=1) == 0                 # given values need no observations
    assert _host_rc(good, ls, noise=None) == 0 and _host_rc(good, ls, logp=None) == 0   # the stage is skipped
    assert _host_rc(good, ls, activation=2) == -1 and _host_rc(good, ls, obs_dim=0) == -1
    assert _host_rc(good, ls, T=0) == -1 and _host_rc(good, ls, E=0) == -1
    assert _native.lib().sng_ppo_host_finish(11, 3, 1, 4, 5, None, None, None, 1) == -1


def test_a_skipped_log_prob_stage_leaves_logp_untouched():
    """A NULL noise skips the stage: a logp buffer that is given all the same keeps its bytes, and the other outputs
    are those of a call with the stage."""
    good = random_weights(11, 1, seed=1)
    ls = np.array([0.0, -1.0, 0.5], np.float32)
    rng = np.random.default_rng(4)
    noise = rng.normal(0, 1, (4, 5, 3)).astype(np.float32)
    obs = rng.uniform(0, 1, (2, 5, 5, 11)).astype(np.float32)
    reward = -rng.random((2, 4, 5))

    def run(**rollout):
        out = dict(logp=np.full((2, 4, 5), 7.25, np.float32), advantages=np.zeros((2, 4, 5), np.float32),
                   values=np.zeros((2, 5, 5), np.float32))
        assert _host_rc(good, ls, arrays=dict(out, noise=noise, obs=obs, reward=reward), **rollout) == 0
        return out
    skipped, with_stage = run(noise=None), run()
    assert (skipped["logp"] == np.float32(7.25)).all()
    assert (with_stage["logp"] != np.float32(7.25)).all()
    for name in ("values", "advantages"):
        assert skipped[name].tobytes() == with_stage[name].tobytes() and skipped[name].any()
    assert run(logp=None)["advantages"].tobytes() == with_stage["advantages"].tobytes()


def test_without_log_std_the_standard_deviations_are_one():
    """log_std = NULL is zeros (SB3's log_std_init): inv_std is exactly 1, and the float32 sum is within the bound of
    test_log_prob_agrees_with_float64_normal of the float64 standard normal's."""
    rng = np.random.default_rng(3)
    reward, done = -rng.random((1, 4, 5)), np.zeros((1, 4, 5), np.uint8)
    values = rng.normal(0, 1, (1, 5, 5)).astype(np.float32)
    noise = rng.normal(0, 1, (4, 5, 3)).astype(np.float32)
    _, _, _, lp = policy.ppo_host_finish(None, reward, done, noise=noise, values=values)
    z = noise.astype(np.float64)
    want = (-0.5 * z ** 2 - 0.5 * np.log(2 * np.pi)).sum(-1)
    assert (np.abs(lp[0] - want) <= (3 + 8) * U * (0.5 * z ** 2 + 0.919).sum(-1)).all()
    zeros = policy.ppo_host_finish(None, reward, done, log_std=np.zeros(3, np.float32), noise=noise, values=values)[3]
    assert lp.tobytes() == zeros.tobytes()


# ------------------------------------------------------------------------------------------------ state-dict loading
def sb3_state_dict(obs_dim, act_dim, seed):
    actor = random_weights(obs_dim, act_dim, seed)
    critic = random_weights(obs_dim, 1, seed + 1)
    sd = dict(zip(policy.SB3_KEYS, actor))
    sd.update(zip(policy.SB3_VALUE_KEYS, critic))
    sd["log_std"] = np.linspace(-1, 0.25, act_dim).astype(np.float32)
    return sd, actor, critic


def test_state_dict_loading_takes_sb3s_keys_and_names_a_missing_one():
    sd, actor, critic = sb3_state_dict(11, 3, 5)
    assert policy.SB3_VALUE_KEYS == ("mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias",
                                     "mlp_extractor.value_net.2.weight", "mlp_extractor.value_net.2.bias",
                                     "value_net.weight", "value_net.bias")
    sd["features_extractor.flatten.weight"] = np.zeros(3, np.float32)   # anything else is ignored
    arrs, ls = policy.head_weights(sd, 11, 3)
    assert all(np.array_equal(a, b) for a, b in zip(arrs, critic)) and np.array_equal(ls, sd["log_std"])
    assert all(np.array_equal(a, b) for a, b in zip(policy.actor_weights(sd, 11, 3), actor))
    six, zeros = policy.head_weights(critic, 11, 3)
    assert all(np.array_equal(a, b) for a, b in zip(six, critic)) and np.array_equal(zeros, np.zeros(3, np.float32))
    assert np.array_equal(policy.head_weights(sd, 11, 3, log_std=np.ones(3))[1], np.ones(3, np.float32))
    for key in policy.SB3_VALUE_KEYS + ("log_std",):
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            policy.head_weights({k: v for k, v in sd.items() if k != key}, 11, 3)
    with pytest.raises(ValueError, match="shapes"):
        policy.head_weights(sd, 12, 3)
    with pytest.raises(ValueError, match="log_std"):
        policy.head_weights(sd, 11, 4)
    # the dict and the arrays give one result
    rng = np.random.default_rng(0)
    obs = rng.uniform(0, 1, (1, 4, 6, 11)).astype(np.float32)
    reward, done = -rng.random((1, 3, 6)), np.zeros((1, 3, 6), np.uint8)
    noise = rng.normal(0, 1, (3, 6, 3)).astype(np.float32)
    a = policy.ppo_host_finish(obs, reward, done, sd, noise=noise)
    b = policy.ppo_host_finish(obs, reward, done, critic, sd["log_std"], noise=noise)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert policy.PpoHead.load.__doc__ and policy.PpoRollout.load.__doc__
