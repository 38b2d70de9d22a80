"""CPU: the wild-action recipe (wild_action_cases.py) is meaningful before it reaches a GPU.

Every row's two days are stepped through the oracle -- pinned to the reference under these very classes by
test_oracle_wild_golden.py -- on model days (oracle.device_day) for device-RNG rows and on the oracle's own days
for reference-RNG rows.  Per row: every class met an occupied charger and the BESS at least MIN_COUNT times and an
empty charger at least once; the overflow classes charged a vehicle to SoC 1.0 (never NaN); a NaN action billed
the reference's finite clamp power; a station without V2X reported error 1 in the mixed wavefront's envs only; no
env-step reported error 3: the BESS SoC after an action is min(calc, 1.0) or max(0, calc), and calc is NaN only
for a NaN action, whose max(0.0, NaN) is 0.0.

The per-charger powers come from wild_action_cases.expected_powers, a restatement of charger.py that is pinned
here to the oracle's charging and discharging totals at every env-step.
"""
import numpy as np
import pytest

import oracle as O
import wild_action_cases as W
from station_matrix_cases import load_model_day, square_mode


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    square_mode(True)   # x*x squares, as on the GPU: the arithmetic the GPU test compares with
    yield
    square_mode(False)


def test_classes_and_layout():
    rng = np.random.default_rng(0)
    for names in (W.NONNEG, W.ALL, W.NONNEG + W.NANS):
        a = W.draw(rng, (4000,), names)
        got = {W.NAMES[k] for k in np.unique(W.classify(a))}
        assert got == set(names)
        assert abs(((a == 0) & ~np.signbit(a)).mean() - W.ZERO_FRAC) < 0.05   # "about a fifth exact zeros"
    assert np.isnan(W.QNAN) and np.isnan(W.PNAN) and W.PNAN.view(np.uint32) == 0xffc12345
    assert 0 < W.SUBNORMAL < np.finfo(np.float32).tiny
    with np.errstate(over="ignore"):
        f = lambda a, dt: (np.float32(a) * np.float32(22) * np.float32(0.95)) * np.float32(dt)
        assert np.isfinite(f(1e37, 1.0)) and np.isinf(f(1e37, 2.0))          # the last factor alone overflows
        assert all(np.isinf(f(a, 0.25)) for a in (1.7e37, 3e38, np.inf))     # every dt
    row = W.ROWS[0]
    a = W.row_actions(row, 24)
    assert a.shape == (24, W.E, 11)
    for t in range(24):   # which wavefront-steps stay in the wide kernel's fast loop
        assert W.fast_wavefront(a[t], 10).tolist() == [True, t % 2 == 1, True], t
    assert np.isposinf(a[:, :32, :10]).any() and np.isposinf(a[:, 64:, :10]).any()


@pytest.mark.parametrize("name", W.IDS)
def test_row_meets_every_class(name):
    row = W.ROWS[W.IDS.index(name)]
    cfg = O.OracleConfig(**row.kw)
    T, N, E = cfg.T, cfg.N, W.E
    device = row.rng == "device"
    legacy = row.kw.get("numpy_legacy_promotion", False)
    envs = [O.OracleEnv(cfg, 0 if device else W.SEED + e) for e in range(E)]
    cov = W.WildCoverage(row, T)
    acts = W.row_actions(row, T)
    assert acts.shape == (T, E, cfg.act_dim)
    for day in range(W.DAYS):
        if device:
            for e, env in enumerate(envs):
                load_model_day(env, O.device_day(cfg, W.SEED, e, day, vmax=16))
        else:
            for env in envs:
                env.reset()
        before = [env.scenario(vmax=16) for env in envs]
        occ = np.stack([b["occ"] for b in before])
        for t in range(T):
            arrived = np.stack([(b["arrivals"] == t).any(axis=1) for b in before])
            src = np.where(arrived, t, t - 1)   # charger.py:62-67; python index -1 at t = 0
            soc_prev = np.stack([b["soc"][np.arange(N), src[e]] for e, b in enumerate(before)])
            cap = np.stack([b["cap"][np.arange(N), src[e]] for e, b in enumerate(before)])
            bess_before = np.array([env.bess_soc for env in envs]) if cfg.bess else None
            outs = [env.step(acts[t, e]) for e, env in enumerate(envs)]
            before = [env.scenario(vmax=16) for env in envs]
            soc_after = np.stack([b["soc"][:, t] for b in before])
            powers = W.expected_powers(acts[t, :, :N], occ[:, :, t], soc_prev, cap, cfg.dt, legacy)
            for e, out in enumerate(outs):
                pw = powers[e]
                np.testing.assert_array_equal(out[3]["p_charge"], O.pairwise_sum(pw[pw > 0]), err_msg=f"{name} {day} {t} {e}")
                np.testing.assert_array_equal(out[3]["p_discharge"], O.pairwise_sum(pw[pw < 0]), err_msg=f"{name} {day} {t} {e}")
            cov.add_step(acts[t], occ[:, :, t], soc_prev, soc_after, cap, powers, [o[3] for o in outs], bess_before, cfg.dt)
    print(name, "occupied", dict(cov.occupied), "empty", dict(cov.empty), "bess", dict(cov.on_bess), "overflow_full",
          cov.overflow_full, "nan_clamp", cov.nan_clamp, "errors", cov.errors.sum(axis=1).tolist(), "wave-steps",
          cov.fast_wave_steps, cov.general_wave_steps)
    cov.check()
