"""GPU: the plain `bench.py` run and `--dump-outputs`.

A plain run reports the headline fields and leaves what takes runs of its own (`roofline`, `cpu_baseline`) to
`--full`.  `--dump-outputs DIR` writes the buffers the last timed day left (obs, reward, done, day_return); they
must be the very arrays the same days give when this process replays them one day per graph: same seed, same
actions, warm-up days included."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, STEPS, WARMUP, SEED = 4096, 4, 2, 2024
KW = dict(number_of_chargers=10, time_interval="1h", charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse",
          pv_system_available_in_model=True, battery_system_available_in_model=True)


def test_plain_run_and_dumped_outputs(tmp_path):
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--envs", str(E), "--seed", str(SEED), "--dump-outputs", str(dump)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads(lines[0])
    assert out["steps"] == STEPS and out["value"] > 0 and out["unit"] == "env-steps/s" and out["dtype"] == "f64"
    assert out["higher_is_better"] is True and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(E * 24 * 1e3 / out["ms_per_step"], rel=1e-9)
    assert out["roofline"] is None and out["cpu_baseline"] is None   # --full
    D = out["config"]["days_per_graph_replay"]
    assert STEPS % D == 0
    got = {n: np.load(dump / f"{n}.npy") for n in ("obs", "reward", "done", "day_return")}
    assert sorted(os.listdir(dump)) == sorted(f"{n}.npy" for n in got)
    assert got["obs"].dtype == np.float32 and got["obs"].shape == (E, 29)
    assert all(got[n].dtype == np.float64 and got[n].shape == (E,) for n in ("reward", "day_return"))
    assert got["done"].dtype == np.float32 and got["done"].shape == (E,) and (got["done"] == 1).all()

    # the same days here: bench.py's actions (its generator recipe), one day per graph replay
    from smart_nanogrid_gym import EpisodeGraph, SmartNanogridVecEnv
    venv = SmartNanogridVecEnv(E, seed=SEED, device=0, rng="device", **KW)
    g = torch.Generator(device=venv.device).manual_seed(SEED)
    low = torch.tensor(venv.action_space.low, device=venv.device)
    high = torch.tensor(venv.action_space.high, device=venv.device)
    acts = low + (high - low) * torch.rand((venv.timesteps, E, venv.act_dim), generator=g, device=venv.device)
    acts = torch.where(torch.rand(acts.shape, generator=g, device=venv.device) < 0.2, torch.zeros_like(acts), acts)
    venv.reset_tensors(rng="device")
    graph = EpisodeGraph(venv, acts.contiguous(), with_reset=True, days=1)
    for _ in range(-(-WARMUP // D) * D + STEPS):
        graph.launch()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got["obs"], venv.obs_d.cpu().numpy())
    np.testing.assert_array_equal(got["reward"], venv.reward_d.cpu().numpy())
    np.testing.assert_array_equal(got["day_return"], venv.return_d.cpu().numpy())
    assert (got["day_return"] < 0).any() and np.isfinite(got["day_return"]).all()
    graph.close()
    venv.close()
