"""Actions outside the Box and non-finite actions: the classes, the per-wavefront recipe and the rows shared by the
reference fixtures (golden/make_golden.py wild), their CPU check (test_wild_actions_cpu.py) and the GPU test
(test_gpu_wild_actions.py).

The reference never clips an action and never asks its Box: SmartNanogridEnv.step hands the float32 action to
charger.py and battery_energy_storage_system.py as it is, and so do step_tensors, EpisodeGraph and sng_step.  What
an action means is therefore the reference's arithmetic on it, class by class (CLASSES below).

The recipe is laid out by wavefront, because the wide kernel chooses its path per wavefront of 32 envs and the lean
kernel runs 64 envs per wavefront.  E = 70, two days, one [T, E, A] array per row:

  envs  0-31   non-negative classes only (above the Box, 1e37, the overflow classes, +inf, a subnormal, +0.0): the
               wide kernel's fast loop and the day kernel's register path meet +inf and the overflowing product
  envs 32-63   every class (NaN, -inf, negatives and -0.0 too) at even steps, non-negative only at odd steps: the
               day kernel leaves its register state for the general order and comes back, carrying SoC written
               under wild actions
  envs 64-69   non-negative only: the ragged last wavefront

The BESS slot draws from every class in every env: the wide kernel's choice looks at the charger actions only.
"""
import collections

import numpy as np

E, DAYS, SEED, WAVE_ENVS = 70, 2, 4242, 32
MIN_COUNT = 10   # station_matrix_cases.MIN_COUNT: no condition may hang on one vehicle

F32_MAX = float(np.finfo(np.float32).max)


def _bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


QNAN = _bits(0x7fc00000)        # the default quiet NaN
PNAN = _bits(0xffc12345)        # a quiet NaN with a sign and a payload
SUBNORMAL = np.float32(1e-40)

# name -> draw(rng, n) -> n float32 values of the class.  The charging product is fl32(fl32(fl32(a*22)*0.95)*dt):
#   big37     finite at dt <= 1 h (2.09e38), +inf at dt = 2 h where only the last factor overflows
#   ovf17     overflows at the first product already (1.7e37 * 22 = 3.74e38 > FLT_MAX), at every dt
#   ovf3e38   the same, close to FLT_MAX itself
CLASSES = collections.OrderedDict([
    ("zero", lambda rng, n: np.zeros(n, np.float32)),
    ("in_pos", lambda rng, n: (1.0 - rng.random(n)).astype(np.float32)),                 # (0, 1]
    ("gt1", lambda rng, n: (3.0 - 2.0 * rng.random(n)).astype(np.float32)),              # (1, 3]
    ("big30", lambda rng, n: np.full(n, 1e30, np.float32)),
    ("big37", lambda rng, n: np.full(n, 1e37, np.float32)),
    ("ovf17", lambda rng, n: np.full(n, 1.7e37, np.float32)),
    ("ovf3e38", lambda rng, n: np.full(n, 3e38, np.float32)),
    ("pinf", lambda rng, n: np.full(n, np.inf, np.float32)),
    ("sub", lambda rng, n: np.full(n, SUBNORMAL, np.float32)),
    ("nzero", lambda rng, n: np.full(n, -0.0, np.float32)),
    ("nsub", lambda rng, n: np.full(n, -SUBNORMAL, np.float32)),
    ("in_neg", lambda rng, n: (rng.random(n) - 1.0).astype(np.float32)),                 # [-1, 0)
    ("lt_m1", lambda rng, n: (-3.0 + 2.0 * rng.random(n)).astype(np.float32)),           # [-3, -1)
    ("ninf", lambda rng, n: np.full(n, -np.inf, np.float32)),
    ("qnan", lambda rng, n: np.full(n, QNAN, np.float32)),
    ("pnan", lambda rng, n: np.full(n, PNAN, np.float32)),
])
NAMES = list(CLASSES)
NONNEG = ["zero", "in_pos", "gt1", "big30", "big37", "ovf17", "ovf3e38", "pinf", "sub"]
NANS = ["qnan", "pnan"]
NEGATIVE = ["nsub", "in_neg", "lt_m1", "ninf"]          # a < 0: the charger discharges
ALL = NAMES
OVERFLOW = ["ovf17", "ovf3e38", "pinf"]                  # the float32 product is +inf at every dt
ZERO_FRAC = 0.2


def draw(rng, shape, names, zero_frac=ZERO_FRAC):
    """float32 `shape`: about `zero_frac` exact +0.0 (when "zero" is among `names`), the rest spread evenly over the
    other classes of `names` -- a shuffled round-robin, so that even a few dozen draws (the BESS slot of a short
    fixture) hold every class."""
    n = int(np.prod(shape))
    cycle = [k for k in names if k != "zero"]
    if "zero" in names:
        cycle += ["zero"] * max(1, round(len(cycle) * zero_frac / (1.0 - zero_frac)))
    pick = rng.permutation(np.arange(n) % len(cycle))
    out = np.empty(n, np.float32)
    for i, k in enumerate(cycle):
        m = pick == i
        out[m] = CLASSES[k](rng, int(m.sum()))
    return out.reshape(shape)


def classify(a):
    """The index into NAMES of every action of the float32 array `a`, from its value alone."""
    a = np.asarray(a, np.float32)
    bits = a.view(np.uint32)
    with np.errstate(invalid="ignore"):
        conds = [
            ("qnan", bits == np.uint32(0x7fc00000)), ("pnan", np.isnan(a)),
            ("pinf", a == np.inf), ("ninf", a == -np.inf),
            ("nzero", (a == 0) & np.signbit(a)), ("zero", a == 0),
            ("sub", (a > 0) & (a < np.finfo(np.float32).tiny)), ("nsub", (a < 0) & (a > -np.finfo(np.float32).tiny)),
            ("ovf3e38", a >= 1e38), ("ovf17", a >= 1.5e37), ("big37", a >= 1e36), ("big30", a >= 1e29),
            ("gt1", a > 1), ("in_pos", a > 0), ("lt_m1", a < -1), ("in_neg", a < 0),
        ]
    out = np.full(a.shape, -1, np.int8)
    for name, m in conds:
        out[(out < 0) & m] = NAMES.index(name)
    assert (out >= 0).all()
    return out


# ----------------------------------------------------------------------------------------------------------------
# the rows: the smallest set of stations that reaches every step kernel family
# ----------------------------------------------------------------------------------------------------------------
BASE = dict(charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
            battery_system_available_in_model=True)
Row = collections.namedtuple("Row", "name kw rng kernel day_kernel graph_step_nodes")


def _row(name, N, interval, kernel, rng="device", day_kernel=False, graph_step_nodes=False, **station):
    kw = dict(BASE, number_of_chargers=N, time_interval=interval, **station)
    if "min" in interval:
        kw["extended_day"] = True
    return Row(name, kw, rng, "void sng::" + kernel, day_kernel, graph_step_nodes)


ROWS = [
    # the N = 10 wide kernel on device-RNG packed days, and its day kernel (no V2X: a negative total raises)
    _row("wide10_device_day", 10, "1h", "step_wide_kernel<10, 2, true, false, false>", day_kernel=True),
    # the same on reference-RNG days: unpacked records
    _row("wide10_reference", 10, "1h", "step_wide_kernel<10, 2, false, false, false>", rng="reference"),
    # N = 50, 2 h days: 1e37 overflows in the product's last factor only (a finite power with an infinite change).
    # V2X: among 50 chargers a +inf power nearly always outweighs the negative ones, so a station without V2X
    # would raise at a handful of env-steps only
    _row("wide50_reference_2h_v2x", 50, "2h", "step_wide_kernel<50, 2, false, false, false>", rng="reference",
         graph_step_nodes=True, vehicle_to_everything=True),
    # the lean kernels: V2X takes every class with the breakpoint as its only flag; without V2X a negative total
    # raises per env
    _row("lean10_v2x", 10, "1h", "step_lean_kernel<10, true, false>", vehicle_to_everything=True),
    _row("lean4_no_v2x", 4, "1h", "step_lean_kernel<4, true, false>"),
    # the general kernel without diagnostics, FAST = false: a dt that is no power of two (the divergent discharge
    # branch divides by dt), and legacy promotion (the plain division of a float64 product)
    _row("general10_20min_v2x", 10, "20min", "step_kernel<10, 1, false, false, true>", vehicle_to_everything=True),
    _row("general8_legacy_v2x", 8, "1h", "step_kernel<8, 1, false, false, true>", vehicle_to_everything=True,
         numpy_legacy_promotion=True),
]
IDS = [r.name for r in ROWS]


def row_actions(row, T):
    """[T, E, A] float32 for `row`, used on both days (a captured graph reuses its actions every day; the days
    differ, so the same action meets other vehicles), laid out by wavefront as the module's docstring says."""
    N = row.kw["number_of_chargers"]
    bess = row.kw["battery_system_available_in_model"]
    rng = np.random.default_rng([N, T, 0x511d])
    a = np.empty((T, E, N + int(bess)), np.float32)
    a[:, :, :N] = draw(rng, (T, E, N), NONNEG)
    mixed = np.arange(E) // WAVE_ENVS == 1
    even = np.arange(T) % 2 == 0
    a[np.ix_(even, mixed, np.arange(N))] = draw(rng, (int(even.sum()), int(mixed.sum()), N), ALL)
    if bess:
        a[:, :, N] = draw(rng, (T, E), ALL)
    return a


def fast_wavefront(actions, N):
    """[ceil(E / 32)] bool of one step's [E, A] actions: the wavefronts of 32 envs without a sign bit or a NaN among
    their charger actions, which stay in the wide kernel's fast loop (wide_rebuild_cases.RebuildCount.add_step's
    predicate)."""
    out = []
    for w0 in range(0, len(actions), WAVE_ENVS):
        w = actions[w0:w0 + WAVE_ENVS, :N]
        out.append(not (np.signbit(w).any() or np.isnan(w).any()))
    return np.array(out)


def expected_powers(actions, occ, soc_prev, cap, dt, legacy=False):
    """'Charger power values' of one step as the reference computes them (charger.py:37-56, 92-94, 108-144) for
    float32 actions [E, N]: the float32 product (a * 22) * 0.95 under NumPy 2 (float64 with legacy promotion), the
    SoC change (power * dt) / capacity, and for every action that is neither zero nor positive -- a NaN too -- the
    clamp power -(SoC * capacity / dt) unless the new SoC is below zero: the flag ceil(0.5 * (1 + sign(calc))) is
    NaN for a NaN calc, and NaN is true.  occ, soc_prev, cap [E, N]: the step's occupancy and the SoC and capacity
    the charger reads.  The CPU test pins this restatement to the oracle's totals at every env-step."""
    a = np.asarray(actions, np.float32)
    with np.errstate(all="ignore"):
        if legacy:
            p = (a.astype(np.float64) * 22) * 0.95
            change = (p * dt) / cap
        else:
            p32 = (a * np.float32(22.0)) * np.float32(0.95)
            change = (p32 * np.float32(dt)).astype(np.float64) / cap
            p = p32.astype(np.float64)
        calc = soc_prev + change
        clamp = -((soc_prev * cap) / dt)
        power = np.where(a > 0, p, np.where(~(calc < 0), clamp, p))
    return np.where((occ == 1) & (a != 0), power, 0.0)


class WildCoverage:
    """Counts over the env-steps an oracle batch went through under the recipe: per class, how often it hit an
    occupied charger, an empty one and the BESS; the overflow classes that charged a vehicle to SoC 1.0; the NaN
    actions billed the finite clamp power; the oracle's error codes per env."""

    def __init__(self, row, T):
        self.row, self.T = row, T
        self.N = row.kw["number_of_chargers"]
        self.bess = row.kw["battery_system_available_in_model"]
        self.v2x = row.kw.get("vehicle_to_everything", False)
        self.occupied, self.empty, self.on_bess = (collections.Counter() for _ in range(3))
        self.overflow_full = self.nan_clamp = self.nan_bess_clamp = self.nan_rewards = self.inf_rewards = 0
        self.errors = np.zeros((4, E), np.int64)
        self.fast_wave_steps = self.general_wave_steps = 0

    def add_step(self, actions, occ, soc_before, soc_after, cap, powers, infos, bess_before, dt):
        """One step of every env: actions [E, A]; occ, soc_before, soc_after, cap [E, N] (the step's occupancy, the
        SoC and capacity charger.py reads, the SoC it wrote); powers [E, N] (what each charger billed, from the
        expected reference arithmetic); the oracle's infos; the BESS SoC before the step [E]."""
        N = self.N
        cls = classify(actions)
        fast = fast_wavefront(actions, N)
        self.fast_wave_steps += int(fast.sum())
        self.general_wave_steps += int((~fast).sum())
        for k, name in enumerate(NAMES):
            m = cls[:, :N] == k
            self.occupied[name] += int((m & (occ == 1)).sum())
            self.empty[name] += int((m & (occ != 1)).sum())
            if self.bess:
                self.on_bess[name] += int((cls[:, N] == k).sum())
        ovf = np.isin(cls[:, :N], [NAMES.index(k) for k in OVERFLOW]) & (occ == 1)
        assert (soc_after[ovf] == 1.0).all()   # min(inf, 1.0), never NaN
        self.overflow_full += int(ovf.sum())
        nan = np.isnan(actions[:, :N]) & (occ == 1)
        clamp = -((soc_before * cap) / dt)
        assert (powers[nan] == clamp[nan]).all() and np.isfinite(powers[nan]).all()
        self.nan_clamp += int(nan.sum())
        for e, inf in enumerate(infos):
            self.errors[inf["error"], e] += 1
            self.nan_rewards += int(np.isnan(inf["reward"]))
            self.inf_rewards += int(np.isinf(inf["reward"]))
            if self.bess and np.isnan(actions[e, N]):
                assert inf["bess_power"] == -((bess_before[e] * 80) / dt) and inf["bess_soc"] == 0.0
                self.nan_bess_clamp += 1

    def check(self):
        name = self.row.name
        what = (name, dict(self.occupied), dict(self.empty), dict(self.on_bess))
        for k in NAMES:
            assert self.occupied[k] >= MIN_COUNT and self.empty[k] >= 1, (k,) + what
            if self.bess:
                assert self.on_bess[k] >= MIN_COUNT, (k,) + what
        assert self.overflow_full >= MIN_COUNT and self.nan_clamp >= MIN_COUNT, (name, self.overflow_full, self.nan_clamp)
        if self.bess:
            assert self.nan_bess_clamp >= MIN_COUNT, (name, self.nan_bess_clamp)
        assert self.fast_wave_steps > 0 and self.general_wave_steps > 0
        # rewards the comparison must treat as equal to themselves: -inf (an infinite power billed) and NaN (inf - inf)
        assert self.nan_rewards >= MIN_COUNT and self.inf_rewards >= MIN_COUNT, (name, self.nan_rewards, self.inf_rewards)
        # error 3 (BESS SoC above 1) never: the SoC after an action is min(calc, 1.0) or max(0, calc)
        assert self.errors[3].sum() == 0 and self.errors[2].sum() == 0, (name, self.errors.sum(axis=1))
        mixed = np.arange(E) // WAVE_ENVS == 1
        if self.v2x:
            assert self.errors[1].sum() == 0, (name, self.errors.sum(axis=1))
        else:   # a negative total on a station without V2X: only where negative and NaN actions are
            assert self.errors[1][mixed].sum() >= MIN_COUNT, (name, self.errors.sum(axis=1))
            assert self.errors[1][~mixed].sum() == 0, (name, self.errors[1])
