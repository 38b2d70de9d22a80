"""GPU: the lean step kernel's charging / discharging totals (csrc/sng_step_lean.h, step_lean_kernel).

The lean step (N <= 16, one lane per env, no diagnostics, NumPy-2 promotion, power-of-two dt) keeps the
running sums of the positive and negative charger powers and uses them as numpy's pairwise sums of the
compacted arrays (charging_station.py:289-293) whenever that is provably exact; other lanes compact their
powers into LDS and run the pairwise sum.  These tests drive both branches on purpose -- tiny and
subnormal charging actions (8+ positive float32 powers whose sum is not exact), near-full discharges at
V2X stations (8+ negative powers), ordinary Box actions -- and require:
  - the lean kernel's observations and rewards bit-exact against the general (diagnostics) kernel on the
    same days and actions, for every env, and against the CPU oracle for a sample of envs;
  - the slow branch to have been needed, and to have mattered (the running sum differs from numpy's
    pairwise sum) in some env-steps, judged from the per-charger powers the diagnostics kernel reports.

The wide step kernel (csrc/sng_step_wide.h; N = 10 without V2X, N = 50) keeps such sums per lane in its fast loop,
which a wavefront takes only when none of its charger actions carries a sign bit: the second test drives that
loop and its rebuild branch with a recipe laid out in whole wavefronts (wide_rebuild_cases.py).
"""
import ctypes

import numpy as np
import pytest

import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smart_nanogrid_gym import SmartNanogridVecEnv  # noqa: E402
from smart_nanogrid_gym.vec_env import EpisodeGraph  # noqa: E402
from test_gpu_bench_kernel import load_day  # noqa: E402
from test_gpu_day_kernel import assert_same  # noqa: E402
from wide_rebuild_cases import (E as RE, SEED as RSEED, STATIONS, RebuildCount, rebuild_actions,  # noqa: E402
                                step_prices)


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    O.lib().orc_set_square_mode.argtypes = [ctypes.c_int]
    O.lib().orc_set_square_mode(1)
    yield
    O.lib().orc_set_square_mode(0)


def _actions(rng, E, N, v2x):
    """Per env category (env % 4): Box-uniform; tiny positive (10^U(-12, 0)); heavy discharge (V2X) or
    near-full charge; a mix of subnormal, tiny and full-scale values.  20 % exact zeros throughout."""
    a = np.empty((E, N + 1), np.float32)
    lo = -1.0 if v2x else 0.0
    cat = np.arange(E) % 4
    a[:, :N] = rng.uniform(lo, 1.0, (E, N))
    m = cat == 1
    a[m, :N] = 10.0 ** rng.uniform(-12, 0, (m.sum(), N))
    m = cat == 2
    a[m, :N] = (-1.0 if v2x else 1.0) * rng.uniform(0.6, 1.0, (m.sum(), N))
    m = cat == 3
    a[m, :N] = rng.choice(np.array([1e-40, 1e-30, 3e-8, 1.0, 0.5, -0.0], np.float32), (m.sum(), N))
    a[:, N] = rng.uniform(-1.0, 1.0, E)
    a[rng.random(a.shape) < 0.2] = 0.0
    return a


def _seq(x):
    s = 0.0
    for v in x:
        s += v
    return s


@pytest.mark.parametrize("N,v2x", [(10, True), (16, True), (8, True), (10, False), (16, False), (50, True), (50, False)])
def test_lean_totals_vs_general_kernel_and_oracle(N, v2x):
    """N = 50 is BASELINE config 5's station (15-minute steps, extended day, stochastic profiles), stepped by
    the wide kernel, as is the N = 10 station without V2X.  These rows drive the wide kernel's general order
    only: _actions puts -0.0 into every fourth env, the wide kernel chooses per wavefront, and with this
    recipe and these seeds 0 of the 3,072 (N = 10) and 0 of the 12,288 (N = 50) wavefront-steps stay in its
    fast loop.  The fast loop's running sums and its rebuild of the positive powers from the records and the
    actions are driven by test_wide_fast_loop_rebuild_vs_general_kernel_and_oracle below."""
    E, seed = 2048, 4242 + N
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
              battery_system_available_in_model=True, vehicle_to_everything=v2x)
    if N == 50:
        kw.update(time_interval="15min", extended_day=True, pv_noise=0.2, price_noise=0.1)
    lean = SmartNanogridVecEnv(E, seed=seed, rng="reference", **kw)
    lean._info.flags = None
    diag = SmartNanogridVecEnv(E, seed=seed, rng="reference", info=True, **kw)
    diag._enable_info(per_charger=True)
    name = lean.step_kernel_name()
    if N == 50:
        assert name.startswith("void sng::step_wide_kernel<50, ") and name.endswith(", false, false, true>"), name
    elif N == 10 and not v2x:   # the headline station steps through the wide kernel (two lanes per env)
        assert name.startswith("void sng::step_wide_kernel<10, ") and name.endswith(", false, false, false>"), name
    else:
        assert name == f"void sng::step_lean_kernel<{N}, false, false>"
    T = lean.timesteps
    ids = np.arange(0, E, 16)
    cfg = O.OracleConfig(**kw)
    envs = [O.OracleEnv(cfg, seed + int(i)) for i in ids]
    rng = np.random.default_rng(N)
    need_pos = need_neg = mattered = 0
    for day in range(2):
        o_l = lean.reset_tensors().cpu().numpy()
        o_d = diag.reset_tensors().cpu().numpy()
        np.testing.assert_array_equal(o_l, o_d)
        np.testing.assert_array_equal(o_l[ids], np.stack([e.reset() for e in envs]))
        for t in range(T):
            a = _actions(rng, E, N, v2x)
            ad = torch.from_numpy(a).to(lean.device)
            ol, rl, _ = lean.step_tensors(ad)
            od, rd, _ = diag.step_tensors(ad)
            ol, rl, od, rd = ol.cpu().numpy(), rl.cpu().numpy(), od.cpu().numpy(), rd.cpu().numpy()
            np.testing.assert_array_equal(ol, od, err_msg=f"day {day} t {t}: obs, lean vs general")
            np.testing.assert_array_equal(rl, rd, err_msg=f"day {day} t {t}: reward, lean vs general")
            outs = [e.step(a[i]) for e, i in zip(envs, ids)]
            np.testing.assert_array_equal(ol[ids], np.stack([x[0] for x in outs]), err_msg=f"day {day} t {t}")
            np.testing.assert_array_equal(rl[ids], np.array([x[1] for x in outs]))
            pw = diag.charger_power_d.cpu().numpy()
            for row in pw:
                pos, neg = row[row > 0], row[row < 0]
                if len(neg) >= 8:
                    need_neg += 1
                    mattered += _seq(neg) != O.pairwise_sum(neg)
                if len(pos) >= 8 and not (_seq(pos) <= pos.min() * 2.0 ** 28):
                    need_pos += 1
                    mattered += _seq(pos) != O.pairwise_sum(pos)
    # the slow branch was needed for positives (and for negatives at V2X stations), and it mattered
    assert need_pos > 0 and mattered > 0, (need_pos, need_neg, mattered)
    if v2x:
        assert need_neg > 0, need_neg
    lean.close()
    diag.close()


@pytest.mark.parametrize("station", sorted(STATIONS))
def test_wide_fast_loop_rebuild_vs_general_kernel_and_oracle(station):
    """The wide kernel's fast loop with tiny positive actions (wide_rebuild_cases.py): wavefronts without a sign
    bit keep running sums, and env-steps whose sums are not provably exact rebuild the positive powers from the
    records and the actions tile (pos_slow in WideGroup::run) -- unpacked and packed records, and in the day
    kernel, whose actions tile is the current step's while the next step's inputs already sit in registers.
    Every env is bit-exact against the info=True twin and against the oracle (seeded seed + i, so config 5's
    profile factors match); the twin's per-charger powers show that the rebuild was needed, that it changed the
    sum, and that the change reached some env-step's reward (RebuildCount)."""
    kw, rng, kernel, day_kernel = STATIONS[station]
    wide = SmartNanogridVecEnv(RE, seed=RSEED, rng=rng, **kw)
    diag = SmartNanogridVecEnv(RE, seed=RSEED, rng=rng, info=True, **kw)
    diag._enable_info(per_charger=True)
    graphed = SmartNanogridVecEnv(RE, seed=RSEED, rng=rng, **kw) if day_kernel else None
    cfg = O.OracleConfig(**kw)
    N, T = cfg.N, wide.timesteps
    acts = rebuild_actions(N, T)
    acts_d = torch.from_numpy(acts).to(wide.device)
    envs = [O.OracleEnv(cfg, RSEED + e) for e in range(RE)]
    count = RebuildCount(N, cfg.dt)
    for day in range(2):
        obs = wide.reset_tensors().cpu().numpy()
        np.testing.assert_array_equal(obs, diag.reset_tensors().cpu().numpy())
        assert wide.step_kernel_name() == kernel, wide.step_kernel_name()
        if rng == "device":
            ivs, ratios = wide.get_scenarios(0, RE)
            ref0 = np.stack([load_day(e, iv, r, V=16) for e, iv, r in zip(envs, ivs, ratios)])
        else:
            ref0 = np.stack([e.reset() for e in envs])
        np.testing.assert_array_equal(obs, ref0, err_msg=f"{station} day {day}: reset vs oracle")
        if graphed is not None:
            np.testing.assert_array_equal(graphed.reset_tensors().cpu().numpy(), obs)
            g = EpisodeGraph(graphed, acts_d, with_reset=False)
            assert g.step_nodes_per_day == 1
            g.launch()
        ret = np.zeros(RE)
        for t in range(T):
            what = f"{station} day {day} t {t}"
            o, r, _ = wide.step_tensors(acts_d[t])
            od, rd, _ = diag.step_tensors(acts_d[t])
            o, r = o.cpu().numpy(), r.cpu().numpy()
            np.testing.assert_array_equal(o, od.cpu().numpy(), err_msg=what + ": obs, wide vs general")
            np.testing.assert_array_equal(r, rd.cpu().numpy(), err_msg=what + ": reward, wide vs general")
            prices = step_prices(cfg, envs, t)
            outs = [e.step(acts[t, i]) for i, e in enumerate(envs)]
            np.testing.assert_array_equal(o, np.stack([x[0] for x in outs]), err_msg=what + ": obs vs oracle")
            np.testing.assert_array_equal(r, np.array([x[1] for x in outs]), err_msg=what + ": reward vs oracle")
            ret = ret + r
            count.add_step(acts[t], diag.charger_power_d.cpu().numpy(), [x[3] for x in outs], prices)
        np.testing.assert_array_equal(wide.battery_state_of_charge(), np.array([e.bess_soc for e in envs]))
        np.testing.assert_array_equal(wide.return_d.cpu().numpy(), ret)
        if graphed is not None:   # the day kernel: against the eager handle, which equals the oracle
            assert_same(graphed, wide, f"{station} day {day}: day kernel vs eager steps")
            g.close()
    count.check(station)
    for v in (wide, diag, graphed):
        if v is not None:
            v.close()
