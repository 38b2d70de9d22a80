"""The bench's layout byte model (bench.step_kernel_bytes: what the step moves per env-step of a device-RNG
day) against the committed rocprofv3 PMC traffic of the same kernels (profiles/pmc_step_kernel.json,
FETCH_SIZE x 2 + WRITE_SIZE, separate passes): within 2 % at the headline (N = 10) and at config 5 (N = 50,
stochastic profiles), i.e. the step moves no bytes the model does not account for."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_layout_model_matches_pmc_traffic():
    import bench
    entries = json.load(open(os.path.join(ROOT, "profiles", "pmc_step_kernel.json")))
    seen = 0
    for e in entries:
        noise = e["chargers"] == 50   # config 5: stochastic profiles
        rd, wr = bench.step_kernel_bytes(e["chargers"], noise=noise)
        model = (rd + wr) * e["envs"]
        assert abs(e["bytes_per_launch"] / model - 1) < 0.02, (e["kernel"], e["bytes_per_launch"], model)
        seen += 1
    assert seen >= 2


def test_dump_outputs_formats_and_size_limit(tmp_path, monkeypatch):
    """--dump-outputs: float32 / float64 arrays of every env; past the size limit the same seeded, sorted sample
    of env rows of every array, identical from run to run."""
    import types

    import numpy as np
    import torch

    import bench
    E, O = 1000, 29
    rng = np.random.default_rng(0)
    venv = types.SimpleNamespace(num_envs=E, obs_d=torch.from_numpy(rng.random((E, O), np.float32)),
                                 reward_d=torch.from_numpy(-rng.random(E)), done_d=torch.ones(E, dtype=torch.uint8),
                                 return_d=torch.from_numpy(-rng.random(E)))
    bench.dump_outputs(str(tmp_path / "all"), venv, seed=7)
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert sorted(got) == ["day_return", "done", "obs", "reward"]
    assert got["obs"].dtype == np.float32 and np.array_equal(got["obs"], venv.obs_d.numpy())
    assert got["reward"].dtype == got["day_return"].dtype == np.float64 and got["done"].dtype == np.float32
    assert np.array_equal(got["day_return"], venv.return_d.numpy()) and (got["done"] == 1).all()
    limit = 20_000
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), venv, seed=7)
    s1 = {f[:-4]: np.load(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")}
    ids = s1["env_ids"].astype(np.int64)
    assert 0 < len(ids) < E and (np.diff(ids) > 0).all() and sum(a.nbytes for a in s1.values()) <= limit
    assert np.array_equal(s1["obs"], venv.obs_d.numpy()[ids]) and np.array_equal(s1["reward"], venv.reward_d.numpy()[ids])
    for name, a in s1.items():
        assert np.array_equal(a, np.load(tmp_path / "s2" / f"{name}.npy"))


def test_measurements_are_looked_up_by_build_id(tmp_path, monkeypatch):
    """VERDICT r4 (weak 5): a committed PMC or rocprof summary is quoted only for the build it measured (its
    sng_build_id()), never for another build that happens to keep the kernel's name."""
    import bench
    prof = tmp_path / "profiles"
    prof.mkdir()
    kernel = "void sng::step_wide_kernel<10, 2, true, false, false>"
    (prof / "pmc_step_kernel.json").write_text(json.dumps([
        dict(build_id="aaaaaaaaaaaa", kernel=kernel, envs=65536, chargers=10, bytes_per_launch=111, source="a"),
        dict(build_id="bbbbbbbbbbbb", kernel=kernel, envs=65536, chargers=10, bytes_per_launch=222, source="b")]))
    (prof / "r05_kernel_stats.csv").write_text(
        '"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n'
        f'"{kernel}(float const*, float*)",100,640000,6400.0,90.0,6000,7000,10.0\n')
    (prof / "kernel_stats_index.json").write_text(json.dumps([
        dict(file="profiles/r05_kernel_stats.csv", build_id="aaaaaaaaaaaa", envs=65536, chargers=10)]))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.load_pmc_traffic(65536, 10, kernel, "bbbbbbbbbbbb") == (222, "b")
    assert bench.load_pmc_traffic(65536, 10, kernel, "cccccccccccc") == (None, None)
    assert bench.rocprof_average_us(kernel, 65536, 10, "aaaaaaaaaaaa") == (6.4, "profiles/r05_kernel_stats.csv")
    assert bench.rocprof_average_us(kernel, 65536, 10, "bbbbbbbbbbbb") == (None, None)
    assert bench.rocprof_average_us(kernel, 65536, 50, "aaaaaaaaaaaa") == (None, None)
