"""CPU: the actions of wide_rebuild_cases.py reach the wide kernel's rebuild branch on every station the GPU test
(test_gpu_lean_sums.py) steps, judged before any GPU run from a float32 restatement of charger.py:92-94's product
on the oracle's days: the model of the device days (oracle.device_day), and the oracle's own days of envs seeded
seed + i for the reference-RNG station.  The restated powers are first pinned to the oracle's own totals.
"""
import numpy as np
import pytest

import oracle as O

from wide_rebuild_cases import (E, SEED, STATIONS, RebuildCount, charging_powers, rebuild_actions,  # noqa: E402
                                step_prices)


@pytest.mark.parametrize("station", sorted(STATIONS))
def test_actions_reach_the_rebuild_branch(station):
    kw, rng, _, _ = STATIONS[station]
    cfg = O.OracleConfig(**kw)
    N, T = cfg.N, cfg.T
    acts = rebuild_actions(N, T)
    envs = [O.OracleEnv(cfg, SEED + e) for e in range(E)]
    count = RebuildCount(N, cfg.dt)
    for day in range(2):
        if rng == "device":
            days = [O.device_day(cfg, SEED, e, day, vmax=16) for e in range(E)]
            for env, d in zip(envs, days):
                env.load(d["soc"], d["occ"], d["cap"], d["req"], d["arrivals"], d["departures"], d["ratio"])
        else:
            for env in envs:
                env.reset()
            days = [env.scenario(vmax=16) for env in envs]
        occ = np.stack([d["occ"] for d in days])
        for t in range(T):
            pw = charging_powers(acts[t, :, :N], occ[:, :, t])
            prices = step_prices(cfg, envs, t)
            infos = [env.step(acts[t, e])[3] for e, env in enumerate(envs)]
            # (RebuildCount pins the restated powers and reward to the oracle's totals in the fast-loop wavefronts)
            count.add_step(acts[t], pw, infos, prices)
    print(station, count.summary())
    count.check(station)
    # four wavefronts of six stay in the fast loop (a fifth carries -0.0)
    assert count.fast_wave_steps == 5 * 2 * T and count.general_wave_steps == 2 * T
