"""GPU: the leaner step of day_station_kernel (csrc/sng_step_day.h, WideGroup::run<KEEP, STATION>) where it can go
wrong: the exact-sum test on integer bits (csrc/sng_exact_sum.h), the table rows staged in LDS, the record and actions
pointers carried from step to step, and the penalty sums added on both lanes.

As tests/test_gpu_day_station_kernel.py, three handles of one seed replay the default graph, the generic day kernel's
(generic_day=True) and T step nodes (step_nodes=True); after every replay the last step's observations, reward and
done, the day returns (by row where asked), every charger's SoC, the BESS SoC, the sticky flags, the flag summary, the
day counter and the checkpoint are equal bit for bit.  At 70 envs the same day also goes through the CPU oracle.

Rebuild boundary.  boundary_actions puts the positive charging powers of an env-step exactly 25 binades apart (the
running sum must stay: it is exact), 26 apart and 40 apart (the powers must be summed again in numpy's order), in
these arrangements, one per env % 8, every wavefront holding all of them:
  0  positives on the first lane's chargers only (0-3 and 8)          4  the smallest positive float32 action
  1  the largest on one lane, the smallest on the other                5  an action whose float32 product is +inf, alone
  2  fewer than eight positives (chargers 1, 5, 9: both lanes)         6  ... beside finite ones
  3  all ten chargers positive (eight to ten powers)                   7  no positive action at all
The oracle case counts, from the day's occupancy, the env-steps at each spread per arrangement and those where the two
lanes' running sums are not numpy's pairwise sum: a kernel that kept the running sum there is not bit-exact.

Tables.  No tariff of the station has 24 distinct prices: the default one has two (day and night), price_model 3
has twelve, and the PV power of every daylight hour is another value (asserted below).  The cases run the default
tariff and, for the staged rows, price_model 3, whose last step shows four distinct price entries.
Every step's price and PV value reach the day return through the reward; the four forecast entries reach a caller
through the last step's observation only (t + 3 = 26 included): a day kernel overwrites the observation block every
step and keeps no trajectory (a kept trajectory runs another kernel), so earlier steps' headers are not readable.
32 envs are one full wavefront, 33 and 70 leave a last wavefront of 1 and 6 envs.
"""
import numpy as np
import pytest

import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import wide_rebuild_cases as R  # noqa: E402
from smart_nanogrid_gym import SmartNanogridVecEnv  # noqa: E402
from smart_nanogrid_gym.vec_env import EpisodeGraph  # noqa: E402
from station_matrix_cases import square_mode  # noqa: E402
from test_gpu_bench_kernel import load_day  # noqa: E402
from test_gpu_day_kernel import KW10, flags_of  # noqa: E402
from test_gpu_day_station_kernel import GENERIC, STATION, three_forms  # noqa: E402

T, N = 24, 10
LANE = ([0, 1, 2, 3, 8], [4, 5, 6, 7, 9])   # the chargers of an env's two lanes
SPREADS = (25, 26, 40)
ARRANGEMENTS = 8


def boundary_actions(E, seed=0):
    """[T, E, 11] float32, no sign bit on a charger action (every wavefront takes the fast loop).  A significand x in
    [0.40, 0.70] gives a float32 power (x * 22) * 0.95 in [8.36, 14.63], exponent 3, and scaling x by 2^-s scales
    the power exactly: two occupied chargers with x and x' 2^-s bill powers exactly s binades apart, and every other
    power of the env-step lies between them.  s cycles through SPREADS with the step."""
    rng = np.random.default_rng([seed, E])
    a = np.zeros((T, E, N + 1), np.float32)
    a[:, :, N] = rng.uniform(-1.0, 1.0, (T, E))
    sig = lambda *shape: rng.uniform(0.40, 0.70, shape).astype(np.float32)   # noqa: E731
    for t in range(T):
        s = SPREADS[t % 3]
        for e in range(E):
            arr = e % ARRANGEMENTS
            if arr == 7:
                continue
            if arr in (5, 6):
                if arr == 6:
                    a[t, e, :N] = sig(N)
                    a[t, e, rng.integers(N, size=3)] = 0.0
                a[t, e, rng.integers(N)] = np.float32(1e38)
                continue
            if arr == 4:
                # 2^-149: the power (2^-149 * 22) * 0.95 is 21 * 2^-149, exponent -145; a power x 2^(s - 148) has s - 145
                chargers = list(rng.permutation(N))
                a[t, e, chargers[0]] = np.float32(2.0 ** -149)
                a[t, e, chargers[1:4]] = sig(3) * np.float32(2.0 ** (s - 148))
                a[t, e, chargers[4:7]] = sig(3) * np.float32(2.0 ** (s - 148 - rng.integers(0, s - 3)))
                continue
            chargers = {0: LANE[0], 2: [1, 5, 9], 3: list(range(N))}.get(arr)
            if arr == 1:
                first = int(rng.integers(2))
                hi, lo = rng.choice(LANE[first]), rng.choice(LANE[1 - first])
                rest = [c for c in range(N) if c not in (hi, lo)]
            else:
                hi, lo = rng.choice(chargers, 2, replace=False)
                rest = [c for c in chargers if c not in (hi, lo)]
            a[t, e, hi] = sig()
            a[t, e, lo] = sig() * np.float32(2.0 ** -s)
            for c in rest:
                a[t, e, c] = sig() * np.float32(2.0 ** -int(rng.integers(0, s + 1)))
            if arr in (0, 1):
                a[t, e, rng.choice(rest)] = 0.0
    assert not np.signbit(a[:, :, :N]).any() and np.isfinite(a).all()
    return a


KW10_HOURLY = dict(KW10, price_model=3)   # the tariff with the most distinct hours; the station's kernel all the same


def test_tables_differ_from_step_to_step():
    """What the table cases below rest on: the PV power of every daylight hour is another value, the hourly tariff
    has twelve values over the day, and the last step's four price entries (t = 23 .. 26) are four values."""
    tb = O.OracleConfig(**KW10_HOURLY).tables()
    pv = np.asarray(tb["pv_power"][:T])
    assert len(set(pv[pv > 0])) == int((pv > 0).sum()) >= 8, pv
    price = np.asarray(tb["price"])
    assert len(price) >= T + 3 and len(set(price[:T])) >= 12, price
    assert len(set(np.float32(price[T - 1:T + 3] / tb["price_max"]))) == 4, price[T - 1:T + 3]
    assert len(set(O.OracleConfig(**KW10).tables()["price"][:T])) == 2   # the default tariff: day and night


@pytest.mark.parametrize("E", [33, 70])
def test_hourly_tariff_day(E):
    three_forms(E, boundary_actions(E, seed=3), days=3, kw=KW10_HOURLY, day_returns=True)


@pytest.mark.parametrize("days", [1, 3])
@pytest.mark.parametrize("E", [32, 33, 70])
def test_boundary_days_against_generic_kernel_and_step_nodes(E, days):
    three_forms(E, boundary_actions(E, seed=days), days=days, day_returns=days > 1)


def test_per_env_flag_array_given():
    sticky, last = three_forms(70, boundary_actions(70, seed=5), days=3, info="flags")
    assert not sticky.any() and not last.any(), (sticky, last)   # a bounded station without a negative action raises none


def test_every_info_pointer_null():
    three_forms(70, boundary_actions(70, seed=6), days=1, info="nulls")


@pytest.mark.parametrize("name,kw,generic", [
    ("day_2h", dict(KW10, time_interval="2h"), GENERIC),
    ("requested_soc", dict(KW10, enable_requested_state_of_charge=True), "void sng::day_wide_kernel<10, 2, true, false>"),
])
def test_other_stations_keep_the_generic_kernel(name, kw, generic):
    steps = 12 if name == "day_2h" else T
    a = boundary_actions(33, seed=7)[:steps]
    three_forms(33, a, days=2, kw=kw, names={"station": generic, "generic": generic})


def test_boundary_day_against_the_oracle():
    square_mode(True)   # x*x squares, as on the GPU
    try:
        E = 70
        v = SmartNanogridVecEnv(E, seed=2027, rng="device", **KW10)
        v.reset_tensors()
        ivs, ratios = v.get_scenarios(0, E)
        envs = [O.OracleEnv(O.OracleConfig(**KW10), 0) for _ in range(E)]
        for e, iv, r in zip(envs, ivs, ratios):
            load_day(e, iv, r)
        occ = np.stack([np.asarray(iv["Charger_occupancy"]) for iv in ivs])   # [E][N][slots]
        acts = boundary_actions(E, seed=13)   # of seeds 8..13 the one that leaves most env-steps whose reward shows a kept sum
        g = EpisodeGraph(v, torch.from_numpy(acts).to(v.device), with_reset=False)
        assert g.day_kernel_name == STATION
        g.launch()
        torch.cuda.synchronize()
        ret = np.zeros(E)
        at = {(arr, s): 0 for arr in range(5) for s in SPREADS}
        inf_alone = inf_beside = none_positive = not_pairwise = reward_changed = 0
        price = O.OracleConfig(**KW10).tables()["price"]
        for t in range(T):
            outs = [e.step(acts[t, i]) for i, e in enumerate(envs)]
            ret = ret + np.array([x[1] for x in outs])
            pw = R.charging_powers(acts[t, :, :N], occ[:, :, t])
            for e in range(E):
                pos = pw[e][pw[e] > 0]
                assert outs[e][3]["p_charge"] == O.pairwise_sum(pos)
                arr = e % ARRANGEMENTS
                if len(pos) == 0:
                    none_positive += arr == 7
                    continue
                if np.isinf(pos).any():
                    inf_alone += len(pos) == 1
                    inf_beside += len(pos) > 1
                    continue
                ex = np.frexp(pos)[1]
                spread = int(ex.max() - ex.min())
                if (arr, spread) in at:
                    at[(arr, spread)] += 1
                lanes = sum(R._seq(pw[e][ix][pw[e][ix] > 0]) for ix in LANE)
                if spread <= 25:
                    assert lanes == O.pairwise_sum(pos), (t, e, pos)   # the criterion's claim, on this day's powers
                else:
                    not_pairwise += lanes != O.pairwise_sum(pos)
                    info = outs[e][3]
                    reward_changed += R.reward_from(lanes, info, float(acts[t, e, N]), price[t], 1.0) != info["reward"]
        print("env-steps per (arrangement, spread):", at, "inf alone / beside:", inf_alone, inf_beside,
              "no positive:", none_positive, "running sum not numpy's:", not_pairwise, "and the reward shows it:", reward_changed)
        assert all(n > 0 for n in at.values()), at
        assert inf_alone > 0 and inf_beside > 0 and none_positive > 0 and not_pairwise > 0 and reward_changed > 0
        np.testing.assert_array_equal(v.obs_d.cpu().numpy(), np.stack([x[0] for x in outs]))
        np.testing.assert_array_equal(v.reward_d.cpu().numpy(), np.array([x[1] for x in outs]))
        np.testing.assert_array_equal(v.return_d.cpu().numpy(), ret)
        np.testing.assert_array_equal(v.battery_state_of_charge(), np.array([e.bess_soc for e in envs]))
        assert bool(v.done_d.cpu().numpy().all()) and not flags_of(v).any()
        g.close()
        v.close()
    finally:
        square_mode(False)
