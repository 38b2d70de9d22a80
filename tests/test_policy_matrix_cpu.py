"""CPU: every row of the policy matrix (policy_matrix_cases.py) is meaningful before it reaches a GPU, and the host
model of a PPO rollout's finish is SB3's loop on real rewards.

The closed loop runs on the CPU alone: the oracle's observation, the library's host actor (sng_policy_host_actions,
relu), the clip, the oracle's step.  Device-RNG rows step the oracle's model of the handle's days (oracle.device_day),
reference-RNG rows the oracle's own days of envs seeded SEED + i.  The row's coverage conditions reach MIN_COUNT, the
share of the actions strictly inside the Box lies in (0.1, 0.9), rows without V2X hold exact-zero env actions and
raise no flag, and done is true at step T - 1 only.  Then policy.ppo_host_finish on that trajectory with the recipe's
noise, gamma = 0.98 and lambda = 0.9: advantages and returns bitwise test_ppo_rollout_cpu's numpy float32 restatement
of SB3's compute_returns_and_advantage, at T = 6, 12, 24, 48, 72 and 96, the large penalties of the dense rows
included.
"""
import numpy as np
import pytest

import oracle as O

from policy_matrix_cases import (DAYS, E, GAE_LAMBDA, GAMMA, IDS, ROWS, SEED, Coverage, action_space,  # noqa: E402
                                 actor_weights, check_actions, cpu_day, load_model_day, log_std, matrix_noise,
                                 square_mode, value_weights)
from smart_nanogrid_gym import policy  # noqa: E402
from test_ppo_rollout_cpu import per_day_gae  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    square_mode(True)   # x*x squares, as on the GPU: the arithmetic the GPU test compares with
    yield
    square_mode(False)


def test_the_matrix_covers_every_day_length():
    assert len(ROWS) == 18
    assert {O.OracleConfig(**r.kw).T for r in ROWS} == {6, 12, 24, 48, 72, 96}


@pytest.mark.parametrize("name", IDS)
def test_row_closed_loop_on_the_cpu(name):
    row = ROWS[IDS.index(name)]
    cfg = O.OracleConfig(**row.kw)
    T, A = cfg.T, cfg.act_dim
    space = action_space(row)
    low, high = np.asarray(space.low, np.float32), np.asarray(space.high, np.float32)
    weights = actor_weights(cfg.obs_dim, A)
    noise = matrix_noise(row, T, A)
    assert noise.shape == (T, E, A)
    device = row.rng == "device"
    envs = [O.OracleEnv(cfg, 0 if device else SEED + e) for e in range(E)]
    cov = Coverage(row, T)
    days = []
    for day in range(DAYS):
        if device:
            model = [O.device_day(cfg, SEED, e, day, vmax=16) for e in range(E)]
            obs0 = np.stack([load_model_day(env, d) for env, d in zip(envs, model)])
        else:
            obs0 = np.stack([env.reset() for env in envs])
            model = [env.scenario(vmax=16) for env in envs]
        cov.add_day(*(np.stack([d[k] for d in model]) for k in ("occ", "arrivals", "departures")))
        days.append(cpu_day(envs, obs0, weights, noise, low, high, policy.host_actions, cov))
    share = check_actions(row, days, noise, low, high)
    breakpoints = sum(i["breakpoint"] != 0 for d in days for step in d["infos"] for i in step)
    print(f"{name}: T = {T}, inside the Box {share:.3f}, breakpoint flags {breakpoints}, {dict(cov.counts)}")
    cov.check()
    # the rollout's finish on this trajectory: SB3's loop, bitwise, on real rewards
    obs, rew, done = (np.stack([d[k] for d in days]) for k in ("obs", "rew", "done"))
    assert obs.shape == (DAYS, T + 1, E, cfg.obs_dim) and rew.dtype == np.float64
    values, adv, ret, logp = policy.ppo_host_finish(obs, rew, done, value_weights(cfg.obs_dim), log_std(A), noise,
                                                    GAMMA, GAE_LAMBDA, "relu")
    want_values = policy.host_actions(obs.reshape(-1, cfg.obs_dim), value_weights(cfg.obs_dim), "relu")[0]
    assert values.tobytes() == want_values.reshape(DAYS, T + 1, E).tobytes()
    want_adv, want_ret = per_day_gae(rew, done, values, GAMMA, GAE_LAMBDA)
    assert adv.tobytes() == want_adv.tobytes(), name
    assert ret.tobytes() == want_ret.tobytes(), name
    assert np.unique(adv).size > adv.size // 2 and np.isfinite(adv).all() and np.isfinite(ret).all()
    assert np.isfinite(logp).all() and logp.min() < -1000.0   # the +-100 entries: z up to about 270
    print(f"{name}: reward min {rew.min():.1f}, |advantage| max {np.abs(adv).max():.1f}, log_prob min {logp.min():.1f}")
