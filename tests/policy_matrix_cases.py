"""The policy matrix shared by its CPU check (test_policy_matrix_cpu.py) and its GPU test
(test_gpu_policy_matrix.py): the station matrix's 18 rows (station_matrix_cases.ROWS, reused, not copied) with a
policy in the loop -- closed-loop captured days and PPO rollouts at every day length, station shape, penalty mode,
step kernel and RNG mode the plain step kernels are pinned at.

The reference is a closed loop on the CPU that reads nothing a device wrote: oracle observation -> host actor (relu,
so bitwise reproducible) -> clip to the station's Box -> oracle step (cpu_closed_loop).

The actor's weights are policy_cases.random_weights(obs_dim, act_dim, 11, out_scale=4.0), the value net's
random_weights(obs_dim, 1, 17, 30.0), log_std linspace(-1, 0.25, act_dim).  The station matrix's action recipe is
expressed through the clip (matrix_noise): a noise entry of -100 leaves the clipped action exactly at the Box's lower
bound (an exact 0.0, idle, on a charger without V2X; -1 with V2X and on the BESS), +100 exactly at the upper bound.
Every row keeps the recipe's seed 1000 A + T: with the library's fmaf host actor no count fell below MIN_COUNT
(test_policy_matrix_cpu.py prints them).
"""
import functools

import numpy as np

from policy_cases import random_weights
from station_matrix_cases import DAYS, E, IDS, MIN_COUNT, ROWS, SEED, Coverage, action_space, load_model_day, square_mode  # noqa: F401

ACTOR_SEED, VALUE_SEED = 11, 17
OUT_SCALE, VALUE_SCALE, NOISE_STD = 4.0, 30.0, 0.8
GAMMA, GAE_LAMBDA = 0.98, 0.9
LOW_NOISE, HIGH_NOISE = np.float32(-100.0), np.float32(100.0)
NET_ARCH = (33, 65)   # the any-width actor: widths that are no multiple of a tile
NET_ROWS = ("lean4_2h_nopv", "day10_15min", "general10_20min_v2x", "ref_lean16_30min_req")
DDPG_ROW = "general10_20min_v2x"
LEAN_ROWS = tuple(r.name for r in ROWS if "step_lean_kernel" in r.kernel)   # the rows with the fused policy day


def row_of(name):
    return ROWS[IDS.index(name)]


def actor_weights(obs_dim, act_dim):
    return random_weights(obs_dim, act_dim, ACTOR_SEED, out_scale=OUT_SCALE)


def value_weights(obs_dim):
    return random_weights(obs_dim, 1, VALUE_SEED, VALUE_SCALE)


def log_std(act_dim):
    return np.linspace(-1.0, 0.25, act_dim).astype(np.float32)


def matrix_noise(row, T, A):
    """[T, E, A] float32, one array for both days (a graph reuses its noise every day): station_matrix_cases'
    row_actions expressed through the clip."""
    N, bess = row.kw["number_of_chargers"], row.kw["battery_system_available_in_model"]
    assert A == N + int(bess)
    rng = np.random.default_rng(1000 * A + T)
    nz = rng.normal(0.0, NOISE_STD, (T, E, A)).astype(np.float32)
    r = rng.random(nz.shape)
    nz[r < 0.2] = LOW_NOISE
    nz[(r >= 0.2) & (r < 0.25)] = HIGH_NOISE
    idle = ((np.arange(E) % 8) == 5)[None, :] & (rng.random((T, E)) < 0.5)
    nz[..., :N][idle] = LOW_NOISE
    if bess:
        heavy = ((np.arange(E) % 4) == 0)[None, :] & (rng.random((T, E)) < 0.7)
        nz[..., -1][heavy] = LOW_NOISE
    assert np.isfinite(nz).all()
    return nz


def cpu_closed_loop(envs, obs0, weights, noise, low, high, host_actions):
    """The closed loop on the CPU: per step (a, env_a, obs, reward, done, info) -- the actor's a [E, A] and the env
    actions it was clipped to, and what the oracle envs answered: the next observation [E, O], rewards [E] float64,
    done flags [E] and the E info dicts.  host_actions is policy.host_actions (or a partial of it with a net_arch);
    envs hold a loaded or reset day whose t = 0 observation is obs0.  Needs no GPU, reads nothing a device wrote."""
    obs = np.ascontiguousarray(obs0, dtype=np.float32)
    for t in range(noise.shape[0]):
        a, env_a = host_actions(obs, weights, "relu", low, high, noise[t])
        outs = [e.step(env_a[i]) for i, e in enumerate(envs)]
        obs = np.stack([o[0] for o in outs])
        yield (a, env_a, obs, np.array([o[1] for o in outs], np.float64), np.array([o[2] for o in outs], bool),
               [o[3] for o in outs])


def net_host_actions(policy, net_arch=NET_ARCH):
    return functools.partial(policy.host_actions, net_arch=net_arch)


def given_actions(env_actions):
    """In host_actions' place: step t takes env_actions[t] as they are (the oracle driven by recorded env actions)."""
    steps = iter(env_actions)

    def take(obs, weights, activation, low, high, noise):
        a = next(steps)
        return a, a
    return take


def cpu_day(envs, obs0, weights, noise, low, high, host_actions, cov=None):
    """One day of cpu_closed_loop as arrays: obs [T + 1, E, O], act and env [T, E, A], rew [T, E] float64, done
    [T, E] uint8, ret [E] (summed step by step, as the kernels sum), infos [T][E]; counts the steps into `cov`."""
    obs, act, env, rew, done, infos = [np.asarray(obs0, np.float32)], [], [], [], [], []
    ret = np.zeros(len(envs))
    for a, env_a, o, r, d, info in cpu_closed_loop(envs, obs0, weights, noise, low, high, host_actions):
        act.append(a)
        env.append(env_a)
        obs.append(o)
        rew.append(r)
        done.append(d.astype(np.uint8))
        infos.append(info)
        ret = ret + r
        if cov is not None:
            cov.add_step(info)
    return dict(obs=np.stack(obs), act=np.stack(act), env=np.stack(env), rew=np.stack(rew), done=np.stack(done),
                ret=ret, infos=infos)


def inside_share(act, low, high):
    """The share of the stored actions strictly inside the Box: what the clip does not hide of the network."""
    return float(((act > low) & (act < high)).mean())


def check_actions(row, days, noise, low, high):
    """What the recipe promises of the CPU loop's days (a list of cpu_day's dicts); returns the inside-Box share.
    The -100 / +100 entries sit exactly on the Box; without V2X the chargers' lower bound is an exact 0.0 and no
    error or breakpoint flag is raised; done is true at step T - 1 only."""
    v2x = row.kw.get("vehicle_to_everything", False)
    N = row.kw["number_of_chargers"]
    act, env = np.stack([d["act"] for d in days]), np.stack([d["env"] for d in days])
    share = inside_share(act, low, high)
    assert 0.1 < share < 0.9, (row.name, share)
    np.testing.assert_array_equal(env, np.minimum(np.maximum(act, low), high))
    lo, hi = noise == LOW_NOISE, noise == HIGH_NOISE
    for e in env:
        assert (e[lo] == np.broadcast_to(low, e.shape)[lo]).all() and (e[hi] == np.broadcast_to(high, e.shape)[hi]).all()
    if not v2x:
        assert (low[:N] == 0).all()
        zeros = int((env[..., :N] == 0).sum())
        assert zeros >= DAYS * int(lo[..., :N].sum()) > 0, (row.name, zeros)
        assert not np.signbit(env[..., :N]).any()   # +0.0, not -0.0
    else:
        assert (low == -1).all()
    errors = sum(i["error"] != 0 for d in days for step in d["infos"] for i in step)
    breakpoints = sum(i["breakpoint"] != 0 for d in days for step in d["infos"] for i in step)
    assert errors == 0, (row.name, errors)
    assert (breakpoints > 0) == v2x, (row.name, breakpoints)
    for d in days:
        assert d["done"][-1].all() and not d["done"][:-1].any(), row.name
    return share
