"""GPU: every step kernel family against the CPU oracle under actions outside the Box and non-finite actions
(wild_action_cases.py: above the Box, 1e30, 1e37, the values whose float32 charging product overflows, +-inf, NaN
with and without a payload, -0.0, subnormals, values below -1 and a fifth exact zeros, laid out by wavefront).

The reference never clips and never asks its Box, and neither do step_tensors, EpisodeGraph and sng_step; the
oracle is pinned to the reference under these classes by test_oracle_wild_golden.py, and the recipe's coverage is
asserted on the CPU by test_wild_actions_cpu.py.

One test per row, built like test_gpu_station_matrix: a handle without diagnostics (`fast`, its step kernel asserted
by name) and a twin with info=True (the general kernel with DIAG) start from the same seed and step two days.  At
every step the observations and rewards of all 70 envs equal the twin's and the oracle's -- NaN equal to NaN
(assert_array_equal), everything else exact; a NaN's sign and payload are not compared.  The twin's per-step flags
are the oracle's `error` / `breakpoint` (NEGATIVE_DEMAND <=> error 1, V2X_BREAKPOINT <=> breakpoint, nothing else),
and the sticky flags of `fast` are their OR over the steps so far.  After each day the vehicles' SoC, the BESS SoC
and the day return (NaN returns included) are compared as well.

The N = 10 device row runs both days again as one EpisodeGraph (one step node per day: the day kernel, which keeps
the SoC written under wild actions in registers and leaves them for the general order at every other step of the
mixed wavefront); the N = 50 row runs each day again as a steps-only graph of T step nodes.

general8_legacy_v2x goes against the oracle only: no reference fixture exists for legacy promotion, because the
reference at hand runs NumPy 2; the oracle's NumPy-1 arithmetic is pinned by the recorded PPO episodes inside the
Box alone.
"""
import ctypes
import re

import numpy as np
import pytest

import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import wild_action_cases as W  # noqa: E402
from smart_nanogrid_gym import SmartNanogridEnv, SmartNanogridVecEnv, _native  # noqa: E402
from smart_nanogrid_gym.settings import BESS_ABOVE_ONE, NEGATIVE_DEMAND  # noqa: E402
from smart_nanogrid_gym.vec_env import EpisodeGraph  # noqa: E402
from station_matrix_cases import square_mode  # noqa: E402
from test_gpu_day_kernel import flags_of  # noqa: E402
from test_gpu_station_matrix import load_exported_day  # noqa: E402

E, DAYS, SEED = W.E, W.DAYS, W.SEED
ND, BP = _native.FLAG_NEGATIVE_DEMAND, _native.FLAG_V2X_BREAKPOINT


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    square_mode(True)   # x*x squares, as on the GPU
    yield
    square_mode(False)


def same(a, b, what):
    """Equal with NaN equal to NaN (torch.equal and == are not)."""
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    b = b.cpu().numpy() if hasattr(b, "cpu") else np.asarray(b)
    np.testing.assert_array_equal(a, b, err_msg=what)


def assert_same_handles(a, b, what):
    """test_gpu_day_kernel.assert_same with NaN equal to NaN, and the vehicles' SoC."""
    torch.cuda.synchronize()
    for k in ("obs_d", "reward_d", "done_d", "return_d"):
        same(getattr(a, k), getattr(b, k), f"{what}: {k}")
    same(a.battery_state_of_charge(), b.battery_state_of_charge(), what + ": BESS SoC")
    same(a.vehicle_state_of_charge(), b.vehicle_state_of_charge(), what + ": vehicle SoC")
    assert a.day_counter() == b.day_counter(), what
    same(flags_of(a), flags_of(b), what + ": sticky flags")


def expected_flags(infos):
    return np.array([(ND if i["error"] == 1 else 0) | (BP if i["breakpoint"] else 0) for i in infos], np.uint32)


@pytest.mark.parametrize("name", W.IDS)
def test_wild_row_vs_general_kernel_and_oracle(name):
    row = W.ROWS[W.IDS.index(name)]
    kw, device = row.kw, row.rng == "device"
    v2x = kw.get("vehicle_to_everything", False)
    fast = SmartNanogridVecEnv(E, seed=SEED, rng=row.rng, **kw)
    diag = SmartNanogridVecEnv(E, seed=SEED, rng=row.rng, info=True, **kw)
    graphed = SmartNanogridVecEnv(E, seed=SEED, rng=row.rng, **kw) if row.graph_step_nodes else None
    cfg = O.OracleConfig(**kw)
    T = fast.timesteps
    assert T == cfg.T and fast.obs_dim == cfg.obs_dim and fast.act_dim == cfg.act_dim
    acts = W.row_actions(row, T)
    acts_d = torch.from_numpy(acts).to(fast.device)
    same(acts_d, acts, "the actions' bits reach the device")
    envs = [O.OracleEnv(cfg, 0 if device else SEED + e) for e in range(E)]
    sticky = np.zeros(E, np.uint32)
    errors = np.zeros(E, np.int64)
    nan_rewards = inf_rewards = 0
    day_returns = []
    for day in range(DAYS):
        obs = fast.reset_tensors().cpu().numpy()
        same(obs, diag.reset_tensors(), f"{name} day {day}: reset")
        assert fast.step_kernel_name() == row.kernel, (name, fast.step_kernel_name())
        parts = diag.step_kernel_name().rstrip(">").split("<")
        assert parts[0] == "void sng::step_kernel" and parts[1].split(", ")[2] == "true", diag.step_kernel_name()
        if device:   # the day, independently of any step kernel: into the oracle
            ivs, ratios = fast.get_scenarios(0, E)
            ref0 = np.stack([load_exported_day(e, iv, r) for e, iv, r in zip(envs, ivs, ratios)])
        else:
            ref0 = np.stack([e.reset() for e in envs])
        same(obs, ref0, f"{name} day {day}: reset vs oracle")
        g = None
        if graphed is not None:   # the same day as a steps-only graph: T step nodes
            same(graphed.reset_tensors(), obs, f"{name} day {day}: reset of the graphed handle")
            g = EpisodeGraph(graphed, acts_d, with_reset=False)
            assert g.step_nodes_per_day == T, (name, g.step_nodes_per_day)
            g.launch()
        ret = np.zeros(E)
        for t in range(T):
            what = f"{name} day {day} t {t}"
            o, r, d = fast.step_tensors(acts_d[t])
            ot, rt, dt = diag.step_tensors(acts_d[t])
            o, r, d = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()
            same(o, ot, what + ": obs vs general kernel")
            same(r, rt, what + ": reward vs general kernel")
            outs = [e.step(acts[t, i]) for i, e in enumerate(envs)]
            same(o, np.stack([x[0] for x in outs]), what + ": obs vs oracle")
            same(r, np.array([x[1] for x in outs]), what + ": reward vs oracle")
            assert bool(d.all()) == bool(d.any()) == (t == T - 1), what
            same(d, dt, what)
            want = expected_flags([x[3] for x in outs])
            same(diag.last_info()["flags"].astype(np.uint32), want, what + ": the twin's per-step flags vs oracle")
            sticky |= want
            same(flags_of(fast), sticky, what + ": sticky flags are the OR over the steps")
            errors += (want & ND) != 0
            nan_rewards += int(np.isnan(r).sum())
            inf_rewards += int(np.isinf(r).sum())
            ret = ret + r
        what = f"{name} after day {day}"
        b = fast.battery_state_of_charge()
        same(b, diag.battery_state_of_charge(), what)
        same(b, np.array([e.bess_soc for e in envs]), what + ": BESS SoC vs oracle")
        assert np.isfinite(b).all() and (b >= 0).all() and (b <= 1).all(), what
        soc = fast.vehicle_state_of_charge()
        same(soc, diag.vehicle_state_of_charge(), what)
        assert np.isfinite(soc).all(), what   # no action leaves a NaN in a vehicle's SoC
        same(flags_of(fast), flags_of(diag), what)
        same(fast.return_d, ret, what + ": day return vs oracle")
        day_returns.append(ret)
        if g is not None:
            assert_same_handles(graphed, fast, what + ": steps-only graph vs eager")
            g.close()
    # the recipe did what it is for on the days actually stepped
    assert nan_rewards >= W.MIN_COUNT and inf_rewards >= W.MIN_COUNT, (name, nan_rewards, inf_rewards)
    mixed = np.arange(E) // W.WAVE_ENVS == 1
    assert not (sticky & ~np.uint32(BP if v2x else ND)).any(), (name, sticky)
    if v2x:
        assert (sticky == BP).any(), name
    else:   # NEGATIVE_DEMAND per env: in the mixed wavefront, in no other
        assert errors[mixed].sum() >= W.MIN_COUNT and not errors[~mixed].any(), (name, errors)
    if row.day_kernel:
        captured_days_vs_eager(row, acts_d, fast, day_returns)
    for v in (fast, diag, graphed):
        if v is not None:
            v.close()


def captured_days_vs_eager(row, acts_d, fast, day_returns):
    """Both days as one EpisodeGraph launch on a fresh handle of the same seed (one step node per day: the day
    kernel), against `fast` after its eager days and the day returns found there, NaN returns included."""
    h = SmartNanogridVecEnv(E, seed=SEED, rng="device", **row.kw)
    rets = torch.zeros((DAYS, E), dtype=torch.float64, device=h.device)
    g = EpisodeGraph(h, acts_d, days=DAYS, day_returns=rets)
    assert g.step_nodes_per_day == 1, (row.name, g.step_nodes_per_day)
    g.launch()
    torch.cuda.synchronize()
    same(rets, np.stack(day_returns), f"{row.name}: day_returns")
    assert np.isnan(np.stack(day_returns)).any()
    h.return_d.copy_(rets[DAYS - 1])   # the graph's returns went into day_returns' rows, not into return_d
    assert_same_handles(h, fast, f"{row.name}: {DAYS} captured days vs eager days")
    g.close()
    h.close()


def test_step_host_reports_the_flags_of_wild_actions():
    """sng_step_host on the lean N = 4 station without V2X, reference-RNG days: the per-env flags it returns are
    those of a twin with info=True (NEGATIVE_DEMAND in the mixed wavefront's envs only), and so are its
    observations and rewards."""
    row = W.ROWS[W.IDS.index("lean4_no_v2x")]
    a_env = SmartNanogridVecEnv(E, seed=SEED, rng="reference", info=True, **row.kw)
    b_env = SmartNanogridVecEnv(E, seed=SEED, rng="reference", **row.kw)
    a_env.reset_tensors()
    b_env.reset_tensors()
    assert b_env.step_kernel_name() == "void sng::step_lean_kernel<4, false, false>"
    acts = W.row_actions(row, a_env.timesteps)
    obs = np.zeros((E, a_env.obs_dim), np.float32)
    rew = np.zeros(E)
    done = np.zeros(E, np.uint8)
    flags = np.zeros(E, np.uint32)
    seen = np.zeros(E, np.uint32)
    P = lambda x: ctypes.c_void_p(x.ctypes.data)   # noqa: E731
    for t in range(a_env.timesteps):
        act = np.ascontiguousarray(acts[t])
        oa, ra, _ = a_env.step_tensors(torch.from_numpy(act).to(a_env.device))
        flags[:] = 0xdead   # the call writes every env's slot
        _native.check(_native.lib().sng_step_host(b_env._h, P(act), P(obs), P(rew), P(done), P(flags),
                                                  ctypes.byref(b_env._info), ctypes.c_void_p(0)), b_env._h)
        torch.cuda.synchronize()
        same(flags, a_env.flags_d.cpu().numpy().astype(np.uint32), f"t {t}: flags")
        same(obs, oa, f"t {t}: obs")
        same(rew, ra, f"t {t}: reward")
        seen |= flags
    mixed = np.arange(E) // W.WAVE_ENVS == 1
    assert (seen[mixed] == ND).sum() >= W.MIN_COUNT and not seen[~mixed].any(), seen
    a_env.close()
    b_env.close()


KW10 = dict(W.BASE, number_of_chargers=10, time_interval="1h")


def test_negative_action_without_v2x_raises_the_reference_error():
    """central_management_system.py:158-159 through the three surfaces: SmartNanogridVecEnv.step,
    SmartNanogridEnv.step, and check_errors() after step_tensors."""
    match = re.escape(NEGATIVE_DEMAND)
    v = SmartNanogridVecEnv(8, seed=3, rng="reference", **KW10)
    v.reset()
    a = np.full((8, 11), -1.0, np.float32)
    with pytest.raises(ValueError, match=match):
        for _ in range(v.timesteps):
            v.step(a)
    v.close()
    env = SmartNanogridEnv(seed=3, rng="reference", **KW10)
    env.reset()
    with pytest.raises(ValueError, match=match):
        for _ in range(24):
            env.step(a[0])
    w = SmartNanogridVecEnv(8, seed=3, rng="reference", **KW10)
    w.reset_tensors()
    w.check_errors()   # nothing raised yet
    for _ in range(12):
        w.step_tensors(torch.from_numpy(a).to(w.device))   # the device path raises nothing by itself
    with pytest.raises(ValueError, match=match):
        w.check_errors()
    w.close()


@pytest.mark.parametrize("family, kw, info", [
    ("step_lean_kernel", dict(W.BASE, number_of_chargers=4, time_interval="1h"), False),
    ("step_wide_kernel", KW10, False),
    ("step_kernel", KW10, True),
])
def test_bess_soc_above_one_raises_the_flag_for_that_env_only(family, kw, info):
    """SNG_FLAG_BESS_SOC_ABOVE_1 (penaliser.py:110-111): one env's BESS SoC set to 1.25, zero actions.  The flag is
    raised for that env only, the battery penalty is 0, the oracle with bess_soc = 1.25 reports error 3, and the
    numpy step() raises the reference's message."""
    n, hot = 8, 3
    v = SmartNanogridVecEnv(n, seed=5, rng="reference", info=info, **kw)
    v.reset_tensors()
    assert v.step_kernel_name().startswith("void sng::" + family + "<"), v.step_kernel_name()
    soc = v.battery_state_of_charge()
    soc[hot] = 1.25
    v.set_battery_state_of_charge(soc)
    zeros = np.zeros((n, v.act_dim), np.float32)
    o, r, _ = v.step_tensors(torch.from_numpy(zeros).to(v.device))
    want = np.zeros(n, np.uint32)
    want[hot] = _native.FLAG_BESS_SOC_ABOVE_1
    same(flags_of(v), want, family)
    assert v.battery_state_of_charge()[hot] == 1.25
    cfg = O.OracleConfig(**kw)
    envs = [O.OracleEnv(cfg, 5 + e) for e in range(n)]
    for e, env in enumerate(envs):
        env.bess_soc = soc[e]
        env.reset()
    outs = [env.step(zeros[e]) for e, env in enumerate(envs)]
    assert [x[3]["error"] for x in outs] == [3 if e == hot else 0 for e in range(n)]
    same(o, np.stack([x[0] for x in outs]), family + ": obs vs oracle")
    same(r, np.array([x[1] for x in outs]), family + ": reward vs oracle")
    if info:
        li = v.last_info()
        same(li["flags"].astype(np.uint32), want, family)
        assert li["total_battery_penalty"][hot] == 0.0 and outs[hot][3]["pen_battery"] == 0.0
    with pytest.raises(ValueError, match=re.escape(BESS_ABOVE_ONE)):
        v.step(zeros)
    v.close()
