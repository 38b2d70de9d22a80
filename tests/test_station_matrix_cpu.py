"""CPU: every row of the station matrix (station_matrix_cases.py) is meaningful before it reaches a GPU.

Device-RNG rows: the oracle's model of the handle's days (oracle.device_day, pinned by test_device_day_model_cpu.py
and, on the GPU, by test_gpu_device_day_exact.py) is stepped through the oracle with the row's actions; reference-RNG
rows: the oracle's own days of envs seeded seed + i.  The row's coverage conditions are counted from the days and
the oracle's info, and every count must reach MIN_COUNT: the GPU's own day can differ from the model's at an
ambiguous wait (device_day_cases.AMBIGUOUS_SHARE_MAX), so no condition may hang on one vehicle.
"""
import numpy as np
import pytest

import oracle as O

from station_matrix_cases import (DAYS, E, IDS, ROWS, SEED, Coverage, action_space, load_model_day,  # noqa: E402
                                  row_actions, square_mode)


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    square_mode(True)   # x*x squares, as on the GPU: the arithmetic the GPU test compares with
    yield
    square_mode(False)


def test_rows_are_distinct_and_named_for_their_kernel():
    assert len(set(IDS)) == len(ROWS) == 18
    for r in ROWS:
        N = r.kw["number_of_chargers"]
        assert r.kernel.startswith("void sng::step_") and f"<{N}, " in r.kernel, r.name
        assert r.kernel.split("<")[0].endswith("wide_kernel") or not r.day_kernel, r.name
        assert not (r.day_kernel and r.graph_step_nodes), r.name
    assert sum(r.day_kernel for r in ROWS) == 7 and sum(r.graph_step_nodes for r in ROWS) == 1


@pytest.mark.parametrize("name", IDS)
def test_row_meets_its_coverage_conditions(name):
    row = ROWS[IDS.index(name)]
    cfg = O.OracleConfig(**row.kw)
    T = cfg.T
    acts = row_actions(row, action_space(row), T)
    assert acts.shape == (T, E, cfg.act_dim)
    device = row.rng == "device"
    envs = [O.OracleEnv(cfg, 0 if device else SEED + e) for e in range(E)]
    cov = Coverage(row, T)
    for day in range(DAYS):
        if device:
            days = [O.device_day(cfg, SEED, e, day, vmax=16) for e in range(E)]
            for env, d in zip(envs, days):
                load_model_day(env, d)
        else:
            for env in envs:
                env.reset()
            days = [env.scenario(vmax=16) for env in envs]
        cov.add_day(*(np.stack([d[k] for d in days]) for k in ("occ", "arrivals", "departures")))
        for t in range(T):
            outs = [env.step(acts[t, e]) for e, env in enumerate(envs)]
            assert all(o[2] for o in outs) == (t == T - 1)
            cov.add_step([o[3] for o in outs])
    print(name, dict(cov.counts))
    cov.check()
