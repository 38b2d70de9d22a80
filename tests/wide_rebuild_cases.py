"""The wide kernel's rebuild branch (pos_slow in WideGroup::run, csrc/sng_step_wide.h): stations, actions and the
count of the env-steps that need it, shared by the CPU check (test_wide_rebuild_cpu.py) and the GPU test
(test_gpu_lean_sums.py, test_wide_fast_loop_rebuild_vs_general_kernel_and_oracle).

The wide kernel chooses per wavefront (32 envs): a wavefront with a sign bit among its charger actions (a negative
action, -0.0, NaN) takes the general order for every env; otherwise its fast loop keeps running sums of the
positive powers per lane (lane 0: chargers [0, H) and N - 2; lane 1: [H, 2H) and N - 1; H = (N - 2) / 2) and uses
their sum as numpy's pairwise sum of the compacted powers where that is provably exact.  Where it is not -- at
least 8 positive powers, or positives on both lanes, and a sum above 2^28 times the smallest positive power -- the
env's first lane re-reads the records and the actions tile and runs the pairwise sum.  An action recipe that mixes
its categories within a wavefront (env % 4, one of them with -0.0) never reaches that: every wavefront takes the
general order.  Here the category is (env // 32) % 5, whole wavefronts, and only the last carries a sign bit.

RebuildCount judges from the per-charger powers where the rebuild was needed, where it changed the sum, and --
through a restatement of the oracle's reward, pinned to the oracle at every env-step it is used on -- where that
change reached the reward: only there does a kernel without the rebuild stop being bit-exact.
"""
import numpy as np

import oracle as O

E, SEED, WAVE_ENVS = 166, 4242, 32   # five whole wavefronts and one of 6 envs
KW10 = dict(number_of_chargers=10, time_interval="1h", charging_mode="bounded",
            vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
            battery_system_available_in_model=True)
CONFIG5 = dict(number_of_chargers=50, time_interval="15min", charging_mode="bounded",
               vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
               battery_system_available_in_model=True, extended_day=True, pv_noise=0.2, price_noise=0.1)
# station: (env kwargs, rng, the step kernel, whether a steps-only graph of it is the day kernel)
STATIONS = {
    "n10_reference": (KW10, "reference", "void sng::step_wide_kernel<10, 2, false, false, false>", False),
    "n10_device": (KW10, "device", "void sng::step_wide_kernel<10, 2, true, false, false>", True),
    "n50_config5_device": (CONFIG5, "device", "void sng::step_wide_kernel<50, 2, true, false, true>", False),
}
# Chosen on the CPU (test_wide_rebuild_cpu.py): a rebuilt sum differs from the running sum in its last bit, and
# the penalties of most steps absorb that before the reward; of seeds 0..7 this one leaves 3, 5 and over a hundred
# env-steps on the three stations whose reward shows it (seed 0 left none on the N = 10 device days)
ACTION_SEED = 2
TINY = np.array([1e-40, 1e-30, 3e-8, 1.0, 0.5], np.float32)


def rebuild_actions(N, T):
    """[T, E, N + 1] float32.  Per wavefront category (env // 32) % 5: Box-uniform; tiny positive (10^U(-12, 0));
    near-full charge; a choice of subnormal, tiny and full-scale values without a sign bit; the same choice with
    -0.0 (that wavefront takes the general order).  BESS U[-1, 1]; 20 % exact +0.0 throughout."""
    rng = np.random.default_rng([N, ACTION_SEED])
    cat = (np.arange(E) // WAVE_ENVS) % 5
    a = np.empty((T, E, N + 1), np.float32)
    a[:, :, :N] = rng.uniform(0.0, 1.0, (T, E, N))
    for c, draw in ((1, lambda n: 10.0 ** rng.uniform(-12, 0, (T, n, N))),
                    (2, lambda n: rng.uniform(0.6, 1.0, (T, n, N))),
                    (3, lambda n: rng.choice(TINY, (T, n, N))),
                    (4, lambda n: rng.choice(np.append(TINY, np.float32(-0.0)), (T, n, N)))):
        m = cat == c
        a[:, m, :N] = draw(int(m.sum()))
    a[:, :, N] = rng.uniform(-1.0, 1.0, (T, E))
    a[rng.random(a.shape) < 0.2] = 0.0
    signed = np.signbit(a[:, :, :N]).any(axis=(0, 2))
    assert (signed == (cat == 4)).all()   # no sign bit on a charger action outside the last category
    return a


def charging_powers(actions, occ):
    """charger.py:92-94 in float32, as NumPy 2 computes it for a float32 action: (a * 22) * 0.95 for an occupied
    charger with a > 0 under bounded charging, as float64; 0.0 elsewhere.  actions [E][N], occ [E][N] of a step."""
    a = np.asarray(actions, np.float32)
    p = (a * np.float32(22.0)) * np.float32(0.95)
    assert p.dtype == np.float32
    return np.where((np.asarray(occ) == 1) & (a > 0), p.astype(np.float64), 0.0)


def _seq(x):
    s = 0.0
    for v in x:
        s += v
    return s


def reward_from(p_charge, info, bess_action, price, dt, grid_cost_weight=0.75):
    """The oracle's reward of a step (orc_env_step: central_management_system.py:105-185, accountant.py:26-36)
    restated from its info with another charging total, for a bounded station with PV and BESS; price: the step's
    tariff with its profile factor."""
    rem = (p_charge + info["p_discharge"]) - info["solar_power"]
    if bess_action > 0:
        rem = -(-rem - info["bess_power"])
    elif bess_action < 0:
        rem = rem + info["bess_power"]
    energy = rem * dt
    cost = (energy * 0.8) * price if energy < 0 else energy * price
    return -(grid_cost_weight * abs(cost) + (0.8 * info["pen_battery"] + info["pen_vehicle"]))


class RebuildCount:
    """Over env-steps in wavefronts without a sign-bit charger action: those that satisfy the rebuild's condition,
    and among them those where the running sum is not numpy's pairwise sum (the rebuild mattered): `mattered` for
    the sum in charger order, `mattered_lanes` for the two lanes' partial sums combined, as the kernel keeps it,
    and `reward_changed` where the step's reward with that combined sum is not the oracle's -- a kernel without
    the rebuild cannot be bit-exact there."""

    def __init__(self, N, dt):
        self.N, self.dt, H = N, dt, (N - 2) // 2
        self.lane = [list(range(0, H)) + [N - 2], list(range(H, 2 * H)) + [N - 1]]
        self.fast_wave_steps = self.general_wave_steps = 0
        self.need = self.need_split_only = self.mattered = self.mattered_lanes = self.reward_changed = 0

    def add_step(self, actions, powers, infos, prices):
        """actions [E][A] of a step, the [E][N] float64 charger powers it gave, the oracle's info of every env and
        every env's price at the step."""
        N = self.N
        for w0 in range(0, len(actions), WAVE_ENVS):
            if np.signbit(actions[w0:w0 + WAVE_ENVS, :N]).any() or np.isnan(actions[w0:w0 + WAVE_ENVS, :N]).any():
                self.general_wave_steps += 1
                continue
            self.fast_wave_steps += 1
            for e in range(w0, min(w0 + WAVE_ENVS, len(actions))):
                row, inf, ba = powers[e], infos[e], float(actions[e, N])
                assert (row >= 0).all()
                pos = row[row > 0]
                exact = O.pairwise_sum(pos)
                # the restatements against the oracle: its charging total and its reward
                assert inf["p_charge"] == exact and inf["p_discharge"] == 0.0 and inf["error"] == 0
                assert reward_from(exact, inf, ba, prices[e], self.dt) == inf["reward"]
                if len(pos) == 0:
                    continue
                parts = [row[ix][row[ix] > 0] for ix in self.lane]
                split = len(parts[0]) > 0 and len(parts[1]) > 0
                lanes = _seq(parts[0]) + _seq(parts[1])
                if (len(pos) >= 8 or split) and not (lanes <= pos.min() * 2.0 ** 28):
                    self.need += 1
                    self.need_split_only += len(pos) < 8
                    self.mattered += _seq(pos) != exact
                    self.mattered_lanes += lanes != exact
                    self.reward_changed += reward_from(lanes, inf, ba, prices[e], self.dt) != inf["reward"]

    def summary(self):
        return {k: int(getattr(self, k)) for k in ("fast_wave_steps", "general_wave_steps", "need", "need_split_only",
                                                    "mattered", "mattered_lanes", "reward_changed")}

    def check(self, what):
        s = self.summary()
        assert s["fast_wave_steps"] > 0 and s["general_wave_steps"] > 0, (what, s)
        assert s["need"] > 0 and s["mattered"] > 0 and s["mattered_lanes"] > 0 and s["reward_changed"] > 0, (what, s)


def step_prices(cfg, envs, t):
    """Every env's tariff at step t with its day's profile factor (1.0 without price noise)."""
    base = cfg.tables()["price"][t]
    return [base * env.profiles()[1][t] for env in envs]
