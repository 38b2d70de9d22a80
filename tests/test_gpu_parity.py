"""GPU parity: the HIP step/reset path (through the C ABI) against the reference's golden
vectors and the CPU oracle.  All tests need an MI355X.

Tolerances: observations are compared bit for bit.  Rewards are compared bit for bit
against the oracle in x*x mode (the GPU squares with x*x); against the reference's own
numbers (libm pow(x, 2), which is off by one ulp on ~0.1 % of inputs) within 1e-12
relative -- far inside the 1e-5 the north star allows.
"""
import ctypes
import warnings

import numpy as np
import pytest

import oracle as O
from golden_util import case, cases, kat

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smart_nanogrid_gym import EpisodeGraph, SmartNanogridEnv, SmartNanogridVecEnv  # noqa: E402

INFO_MAP = {"grid_power": "grid_power", "total_charging_power": "p_charge",
            "total_discharging_power": "p_discharge", "battery_state_of_charge": "bess_soc",
            "total_vehicle_penalty": "pen_vehicle", "total_battery_penalty": "pen_battery",
            "grid_energy_cost": "grid_cost", "total_cost": "total_cost", "utilized_solar_energy": "solar_power",
            "battery_power_value": "bess_power", "battery_calculated_power": "bess_calc_power",
            "nonexistent_vehicle_penalty": "nonexistent", "initial_battery_soc": "bess_initial_soc"}


def rel_close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b)))


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    O.lib().orc_set_square_mode.argtypes = [ctypes.c_int]
    yield
    O.lib().orc_set_square_mode(0)


@pytest.mark.parametrize("name", [m["name"] for m in cases()])
def test_golden_cases_reference_rng_end_to_end(name):
    """Env seeded like the reference (np.random.seed(s); random.seed(s)): reset, step through every
    recorded day with the recorded actions, auto-reset between days (BESS carried over)."""
    meta, d = case(name)
    venv = SmartNanogridVecEnv(1, seed=meta["seed"], rng="reference", info=True, **meta["kwargs"])
    obs = venv.reset()
    for ep in range(meta["n_episodes"]):
        np.testing.assert_array_equal(obs[0], d["obs_reset"][ep])
        for t in range(meta["T"]):
            obs, rew, dones, infos = venv.step(d["actions"][ep][t][None])
            info = venv.last_info()
            final = infos[0].get("terminal_observation", obs[0])
            np.testing.assert_array_equal(final, d["obs"][ep][t], err_msg=f"ep{ep} t{t}")
            assert rel_close(rew[0], d["reward"][ep][t]), (ep, t, rew[0], d["reward"][ep][t])
            assert bool(dones[0]) == bool(d["done"][ep][t])
            for k, g in INFO_MAP.items():
                assert rel_close(info[k][0], d[g][ep][t]), (k, ep, t, info[k][0], d[g][ep][t])
            assert bool(info["flags"][0] & 8) == bool(d["breakpoint"][ep][t])
    venv.close()


@pytest.mark.parametrize("name", ["bpv_sparse_n10", "bpv_dense_req_n50", "v2x_bpv_n10", "bpv_2h_n10"])
def test_golden_cases_injected_scenario(name):
    """reset_from_arrays with the recorded day (reference layout) + recorded BESS SoC."""
    meta, d = case(name)
    venv = SmartNanogridVecEnv(1, seed=0, info=True, **meta["kwargs"])
    for ep in range(meta["n_episodes"]):
        venv.set_battery_state_of_charge(d["bess_soc_reset"][ep])
        obs = venv.reset_from_arrays(d["soc0"][ep][None], d["occ"][ep][None], d["cap"][ep][None],
                                     d["req"][ep][None], d["arrivals"][ep][None], d["departures"][ep][None],
                                     np.array([d["ratio"][ep]]))
        np.testing.assert_array_equal(obs[0], d["obs_reset"][ep])
        for t in range(meta["T"]):
            o, r, dn = venv.step_tensors(torch.from_numpy(d["actions"][ep][t][None]).to(venv.device))
            np.testing.assert_array_equal(o.cpu().numpy()[0], d["obs"][ep][t])
            assert rel_close(r.cpu().numpy()[0], d["reward"][ep][t])
    venv.close()


@pytest.mark.parametrize("sub", ["single_prediction_files", "training_files"])
def test_recorded_ppo_episode_replay(sub):
    """The reference's recorded PPO day (NumPy 1.24 promotion, 0.8 grid-cost weight) replayed on GPU."""
    k = kat(sub)
    iv, pr = k["iv"], k["pr"]
    venv = SmartNanogridVecEnv(1, info=True, number_of_chargers=k["N"], time_interval="1h", charging_mode="bounded",
                               vehicle_uncharged_penalty_mode="sparse", numpy_legacy_promotion=True,
                               grid_cost_weight=0.8)
    venv.set_battery_state_of_charge(k["bess_soc0"])
    venv.reset_from_initial_values(iv, k["ratio"], restore_requested_soc=True)
    for t in range(24):
        venv.step_tensors(torch.from_numpy(k["actions"][t][None]).to(venv.device))
        info = venv.last_info()
        assert rel_close(info["grid_power"][0], pr["Grid_power"][t])
        assert info["battery_state_of_charge"][0] == pr["Battery_state_of_charge"][t]
        assert rel_close(info["total_cost"][0], pr["Total_cost"][t])
        assert rel_close(info["total_vehicle_penalty"][0], pr["Total_vehicle_penalties"][t])
    np.testing.assert_array_equal(venv.vehicle_state_of_charge()[0], np.array(pr["SOC"])[:, 23])
    venv.close()


def _oracle_batch(kw, seed, idx):
    cfg = O.OracleConfig(**kw)
    return cfg, [O.OracleEnv(cfg, seed + int(i)) for i in idx]


@pytest.mark.parametrize("E,N,mode,lanes", [(4096, 10, "sparse", 1), (4096, 10, "sparse", 2), (4096, 10, "dense", 4),
                                            (1024, 50, "sparse", 0), (1024, 50, "dense", 4), (1000, 4, "on_departure", 2),
                                            (333, 1, "sparse", 0), (777, 7, "dense", 0), (300, 16, "sparse", 4),
                                            (512, 33, "dense", 0), (256, 128, "sparse", 0)])
def test_batched_reference_rng_vs_oracle_bit_exact(E, N, mode, lanes):
    """Config 2 (4,096 envs x 10 chargers x 24 steps): every env against the oracle seeded base+i,
    two consecutive days, random actions with 20 % exact zeros."""
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode=mode)
    seed = 1000 + N
    O.lib().orc_set_square_mode(1)
    venv = SmartNanogridVecEnv(E, seed=seed, rng="reference", step_lanes_per_env=lanes, **kw)
    cfg, envs = _oracle_batch(kw, seed, range(E))
    rng = np.random.default_rng(E + N)
    for day in range(2):
        obs = venv.reset() if day == 0 else obs
        np.testing.assert_array_equal(obs, np.stack([e.reset() for e in envs]))
        for t in range(cfg.T):
            a = rng.uniform(venv.action_space.low, venv.action_space.high, (E, venv.act_dim)).astype(np.float32)
            a[rng.random(a.shape) < 0.2] = 0
            obs, rew, dones, infos = venv.step(a)
            outs = [e.step(a[i]) for i, e in enumerate(envs)]
            ref_obs = np.stack([o[0] for o in outs])
            got = np.stack([inf.get("terminal_observation", obs[i]) for i, inf in enumerate(infos)])
            np.testing.assert_array_equal(got, ref_obs, err_msg=f"day{day} t{t}")
            np.testing.assert_array_equal(rew, np.array([o[1] for o in outs]))
            assert dones.all() == (t == cfg.T - 1)
    np.testing.assert_array_equal(venv.battery_state_of_charge(), np.array([e.bess_soc for e in envs]))
    venv.close()


@pytest.mark.parametrize("E,N,days", [(64, 10, 12), (32, 50, 6), (16, 128, 3)])
def test_reference_rng_many_days_stream_blocks(E, N, days):
    """Many consecutive reference-RNG days: numpy's stream of every env crosses its 624-word blocks in
    every way the device keeps it (mt_prepare_kernel: a twist, or none when the other block already
    holds the successor (kMtNextReady); a day that draws past both prepared blocks twists on its lane --
    N = 50 and 128 draw more than 624 words a day).  Obs and rewards bit-exact against the oracle's
    RandomState-equal streams, day after day (charging_station.py:200-279)."""
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
              battery_system_available_in_model=True)
    seed = 77 + N
    O.lib().orc_set_square_mode(1)
    venv = SmartNanogridVecEnv(E, seed=seed, rng="reference", **kw)
    cfg, envs = _oracle_batch(kw, seed, range(E))
    rng = np.random.default_rng(days + N)
    obs = venv.reset()
    for day in range(days):
        np.testing.assert_array_equal(obs, np.stack([e.reset() for e in envs]), err_msg=f"day{day} t=0")
        for t in range(cfg.T):
            a = rng.uniform(venv.action_space.low, venv.action_space.high, (E, venv.act_dim)).astype(np.float32)
            obs, rew, dones, infos = venv.step(a)
            outs = [e.step(a[i]) for i, e in enumerate(envs)]
            got = np.stack([inf.get("terminal_observation", obs[i]) for i, inf in enumerate(infos)])
            np.testing.assert_array_equal(got, np.stack([o[0] for o in outs]), err_msg=f"day{day} t{t}")
            np.testing.assert_array_equal(rew, np.array([o[1] for o in outs]), err_msg=f"day{day} t{t}")
    venv.close()


def test_full_size_sampled_parity_65536():
    """Config 3 size (65,536 envs x 10 chargers) with reference RNG: 512 sampled envs against the oracle,
    plus size-independent invariants on all envs."""
    E, N, seed = 65536, 10, 99
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse")
    O.lib().orc_set_square_mode(1)
    venv = SmartNanogridVecEnv(E, seed=seed, rng="reference", info=True, **kw)
    idx = np.random.default_rng(5).choice(E, 512, replace=False)
    cfg, envs = _oracle_batch(kw, seed, idx)
    obs = venv.reset()
    np.testing.assert_array_equal(obs[idx], np.stack([e.reset() for e in envs]))
    g = torch.Generator(device=venv.device).manual_seed(3)
    low = torch.tensor(venv.action_space.low, device=venv.device)
    high = torch.tensor(venv.action_space.high, device=venv.device)
    total = torch.zeros(E, dtype=torch.float64, device=venv.device)
    for t in range(cfg.T):
        a = low + (high - low) * torch.rand((E, venv.act_dim), generator=g, device=venv.device)
        a = torch.where(torch.rand(a.shape, generator=g, device=venv.device) < 0.2, torch.zeros_like(a), a)
        o, r, dn = venv.step_tensors(a)
        total += r
        ah = a.cpu().numpy()
        outs = [e.step(ah[i]) for e, i in zip(envs, idx)]
        oh = o.cpu().numpy()
        np.testing.assert_array_equal(oh[idx], np.stack([x[0] for x in outs]))
        np.testing.assert_array_equal(r.cpu().numpy()[idx], np.array([x[1] for x in outs]))
        # invariants on every env
        soc = oh[:, 8:8 + N]
        assert soc.min() >= 0 and soc.max() <= 1
        assert (r.cpu().numpy() <= 0).all()
        info = venv.last_info()
        assert (info["battery_state_of_charge"] >= 0).all() and (info["battery_state_of_charge"] <= 1).all()
        assert (info["flags"] == 0).all()
    ret = venv.last_info()["episode_return"]
    assert rel_close(ret, total.cpu().numpy(), 1e-9)
    venv.close()


def test_device_rng_day_distribution_and_invariants():
    """Device-generator days: same distributions as the reference generator (oracle MT draws)."""
    E, N = 65536, 10
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse")
    venv = SmartNanogridVecEnv(E, seed=7, rng="device", info=True, **kw)
    obs = venv.reset()
    occ0 = (obs[:, 8 + N:8 + 2 * N] > 0).mean()
    soc_occ = obs[:, 8:8 + N][obs[:, 8 + N:8 + 2 * N] > 0]
    ratio = venv.pv_ratio()
    # oracle statistics over 4,000 reference-RNG envs
    cfg = O.OracleConfig(**kw)
    ref_occ0, ref_soc, ref_ratio = [], [], []
    for i in range(4000):
        e = O.OracleEnv(cfg, 50_000 + i)
        o = e.reset()
        m = o[8 + N:8 + 2 * N] > 0
        ref_occ0.append(m.mean())
        ref_soc.extend(o[8:8 + N][m])
        ref_ratio.append(e.ratio)
    assert abs(occ0 - np.mean(ref_occ0)) < 0.01
    assert abs(soc_occ.mean() - np.mean(ref_soc)) < 0.01
    assert abs(ratio.mean() - np.mean(ref_ratio)) < 0.02
    assert set(np.unique(np.round(ratio * 100))).issubset(set(range(181)))
    occupancy = []
    g = torch.Generator(device=venv.device).manual_seed(1)
    for t in range(24):
        a = torch.rand((E, venv.act_dim), generator=g, device=venv.device)
        a[:, -1] = a[:, -1] * 2 - 1
        o, r, dn = venv.step_tensors(a)
        oh = o.cpu().numpy()
        occupancy.append((oh[:, 8 + N:8 + 2 * N] > 0).mean())
        assert oh[:, 8:8 + N].min() >= 0 and oh[:, 8:8 + N].max() <= 1
        assert (venv.last_info()["flags"] == 0).all()
    # mean occupancy over the day, reference generator: ~0.71 at N=10
    assert 0.66 < np.mean(occupancy) < 0.76
    # the occupancy curve over the day and the stay-length distribution at arrival match the
    # reference process (oracle MT draws, 3,000 days); occupancy reads from the departure column
    ref_curve, ref_stay = np.zeros(24), np.zeros(12)
    dev_stay = np.zeros(12)
    for i in range(3000):
        e = O.OracleEnv(cfg, 90_000 + i)
        o = e.reset()
        prev = np.zeros(N)
        for t in range(24):
            o, _, _, _ = e.step(np.zeros(cfg.act_dim, np.float32))
            d = np.rint(o[8 + N:8 + 2 * N] * 24)
            ref_curve[t] += (d > 0).mean() / 3000
            new = (d > 0) & (prev == 0)   # a vehicle that was not there at t-1 (departure steps are empty)
            for x in d[new]:
                ref_stay[min(int(x), 11)] += 1
            prev = d
    np.testing.assert_allclose(np.array(occupancy), ref_curve, atol=0.02)
    venv.reset_tensors()
    prev = torch.zeros((E, N), device=venv.device)
    for t in range(24):
        o, r, dn = venv.step_tensors(torch.zeros((E, venv.act_dim), device=venv.device))
        d = torch.round(o[:, 8 + N:8 + 2 * N] * 24)
        new = (d > 0) & (prev == 0)
        dev_stay += torch.bincount(d[new].clamp(max=11).long(), minlength=12).cpu().numpy()[:12]
        prev = d
    np.testing.assert_allclose(dev_stay / dev_stay.sum(), ref_stay / ref_stay.sum(), atol=0.01)
    venv.close()


def test_episode_graph_matches_eager_device_rng():
    E, N = 8192, 10
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse")
    acts = torch.rand((24, E, N + 1), device="cuda:0")
    acts[..., -1] = acts[..., -1] * 2 - 1
    a = SmartNanogridVecEnv(E, seed=11, rng="device", **kw)
    b = SmartNanogridVecEnv(E, seed=11, rng="device", **kw)
    graph = EpisodeGraph(b, acts)
    for day in range(3):
        a.reset_tensors()
        for t in range(24):
            oa, ra, da = a.step_tensors(acts[t])
        graph.launch()
        torch.cuda.synchronize()
        assert torch.equal(oa, b.obs_d) and torch.equal(ra, b.reward_d) and torch.equal(da, b.done_d)
        assert torch.equal(a.return_d, b.return_d)
    graph.close()
    a.close()
    b.close()


def test_every_device_reset_draws_a_new_day():
    """The device day counter is read by the reset and advanced by the day's first step; resets
    with no step in between (eager, or an eager reset followed by a graph replay) must still
    draw new days, and the same sequence of calls must give the same days."""
    E, N = 4096, 10
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse")
    acts = torch.rand((24, E, N + 1), device="cuda:0")

    def run(v):
        days = [v.reset_tensors().clone(), v.reset_tensors().clone()]   # twice, no step between
        for t in range(24):
            v.step_tensors(acts[t])
        days.append(v.reset_tensors().clone())
        g = EpisodeGraph(v, acts)   # an eager reset, then a graph whose reset must draw a new day
        g.launch()
        torch.cuda.synchronize()
        g.close()
        days.append(v.reset_tensors().clone())
        return days

    a = SmartNanogridVecEnv(E, seed=21, rng="device", **kw)
    b = SmartNanogridVecEnv(E, seed=21, rng="device", **kw)
    da, db = run(a), run(b)
    for x, y in zip(da, db):
        assert torch.equal(x, y)
    for i in range(len(da)):
        for j in range(i + 1, len(da)):
            assert not torch.equal(da[i], da[j]), (i, j)
    a.close()
    b.close()


def test_step_graph_follows_the_day_encoding():
    """A steps-only graph (the T steps of a day, no reset) replays the day that is loaded:
    device-RNG days are packed 8 B records, host-RNG days word + float64 planes (sng_layout.h).
    Captured after a host-RNG reset it steps that day like eager steps; after a device-RNG reset
    its replay is refused."""
    from smart_nanogrid_gym._native import NativeError
    E, N = 1024, 10
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse")
    acts = torch.rand((24, E, N + 1), device="cuda:0")
    a = SmartNanogridVecEnv(E, seed=3, rng="reference", **kw)
    b = SmartNanogridVecEnv(E, seed=3, rng="reference", **kw)
    a.reset_tensors()
    b.reset_tensors()
    day = EpisodeGraph(b, acts, with_reset=False)
    for t in range(24):
        oa, ra, _ = a.step_tensors(acts[t])
    day.launch()
    torch.cuda.synchronize()
    assert torch.equal(oa, b.obs_d) and torch.equal(ra, b.reward_d)
    b.reset_tensors(rng="device")
    with pytest.raises(NativeError):
        day.launch()
    day.close()
    a.close()
    b.close()


def test_single_env_gym_surface():
    env = SmartNanogridEnv(number_of_chargers=4, time_interval="1h", charging_mode="bounded",
                           vehicle_uncharged_penalty_mode="sparse", seed=12)
    meta, d = case("bpv_sparse_n4")
    obs, info = env.reset()
    assert info == {} and obs.dtype == np.float32 and obs.shape == env.observation_space.shape
    np.testing.assert_array_equal(obs, d["obs_reset"][0])
    for t in range(24):
        obs, r, term, trunc, info = env.step(d["actions"][0][t])
        np.testing.assert_array_equal(obs, d["obs"][0][t])
        assert isinstance(r, np.float64) and trunc is False and term == (t == 23)
    with pytest.raises(RuntimeError):
        env.step(d["actions"][0][0])
    env.close()


@pytest.mark.parametrize("n,v2x,rng", [(10, False, "reference"), (4, False, "device"), (10, True, "reference"),
                                       (7, False, "reference")])
def test_single_env_host_step_equals_device_buffer_step(n, v2x, rng):
    """SmartNanogridEnv.step's sng_step_host path (the kernel reads the actions from and
    writes its outputs to mapped host memory) gives bit for bit what round 5's torch path gives (device
    buffers, copies), over three days of each station kernel: the wide kernel (N = 10), the lean one (N = 4,
    V2X at N = 10) and the general one (N = 7); V2X days raise the reference's breakpoint warning through the
    host path's flags."""
    kw = dict(number_of_chargers=n, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse", vehicle_to_everything=v2x)
    envs = [SmartNanogridEnv(seed=31, rng=rng, **kw) for _ in range(2)]
    envs[1].step_path = "torch"
    rng_a = np.random.default_rng(n)
    lo, hi = envs[0].action_space.low, envs[0].action_space.high
    warned = []
    for day in range(3):
        o0, o1 = envs[0].reset()[0], envs[1].reset()[0]
        np.testing.assert_array_equal(o0, o1)
        for t in range(24):
            a = (lo + (hi - lo) * rng_a.random(lo.size)).astype(np.float32)
            a[rng_a.random(a.size) < 0.2] = 0
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                r0 = envs[0].step(a)
                r1 = envs[1].step(a)
            warned += [str(x.message) for x in w]
            np.testing.assert_array_equal(r0[0], r1[0])
            assert r0[0].dtype == np.float32 and r0[0].shape == envs[0].observation_space.shape
            assert isinstance(r0[1], np.float64) and r0[1] == r1[1] and r0[2:] == r1[2:] and r0[2] == (t == 23)
    assert envs[0].timestep == 0 and envs[0].simulated_single_day
    if v2x:
        assert any("breakpoint" in m for m in warned)
    for e in envs:
        e.close()


@pytest.mark.parametrize("E,N", [(100, 10), (333, 4), (70, 50)])
def test_step_host_batches_equal_step(E, N):
    """sng_step_host over a batch (several wavefronts, a ragged last one) writes the same observations, rewards and
    done flags into host memory as sng_step does into device buffers, and reports each env's step flags."""
    from smart_nanogrid_gym import _native
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="dense")
    a_env = SmartNanogridVecEnv(E, seed=8, rng="reference", **kw)
    b_env = SmartNanogridVecEnv(E, seed=8, rng="reference", **kw)
    a_env.reset_tensors()
    b_env.reset_tensors()
    rng = np.random.default_rng(E)
    lo, hi = a_env.action_space.low, a_env.action_space.high
    obs = np.zeros((E, a_env.obs_dim), np.float32)
    rew = np.zeros(E)
    done = np.zeros(E, np.uint8)
    flags = np.zeros(E, np.uint32)
    P = lambda x: ctypes.c_void_p(x.ctypes.data)   # noqa: E731
    for t in range(a_env.timesteps):
        act = (lo + (hi - lo) * rng.random((E, lo.size))).astype(np.float32)
        act[rng.random(act.shape) < 0.2] = 0
        o, r, d = a_env.step_tensors(torch.from_numpy(act).to(a_env.device))
        _native.check(_native.lib().sng_step_host(b_env._h, P(act), P(obs), P(rew), P(done), P(flags),
                                                  ctypes.byref(b_env._info), ctypes.c_void_p(0)), b_env._h)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(obs, o.cpu().numpy())
        np.testing.assert_array_equal(rew, r.cpu().numpy())
        np.testing.assert_array_equal(done, d.cpu().numpy())
        assert not flags.any()
    a_env.close()
    b_env.close()


@pytest.mark.parametrize("E,N,extra", [(100, 10, dict(vehicle_to_everything=True)), (70, 3, dict(charging_mode=""))])
def test_step_host_batches_report_raised_flags(E, N, extra):
    """sng_step_host's flag section with flags raised -- V2X breakpoints (central_management_system.py:160-165) and
    the charging-mode ValueError (charger.py:88) -- over a batch with a ragged last wavefront: after every step the
    returned per-env flags equal those a twin handle reports through sng_step with info=True (SngInfo.flags), and
    both handles' sticky flags (sng_read_errors) are the OR of the steps so far."""
    from smart_nanogrid_gym import _native
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="dense")
    kw.update(extra)
    a_env = SmartNanogridVecEnv(E, seed=8, rng="reference", info=True, **kw)
    b_env = SmartNanogridVecEnv(E, seed=8, rng="reference", **kw)
    a_env.reset_tensors()
    b_env.reset_tensors()
    rng = np.random.default_rng(E)
    lo, hi = a_env.action_space.low, a_env.action_space.high
    obs = np.zeros((E, a_env.obs_dim), np.float32)
    rew = np.zeros(E)
    done = np.zeros(E, np.uint8)
    flags = np.zeros(E, np.uint32)
    sticky = np.zeros(E, np.uint32)
    P = lambda x: ctypes.c_void_p(x.ctypes.data)   # noqa: E731
    U = ctypes.POINTER(ctypes.c_uint32)

    def read_sticky(env):
        out = np.zeros(E, np.uint32)
        _native.check(_native.lib().sng_read_errors(env._h, out.ctypes.data_as(U), 0, ctypes.c_void_p(0)), env._h)
        return out
    want = _native.FLAG_V2X_BREAKPOINT if "vehicle_to_everything" in extra else _native.FLAG_CHARGING_MODE
    mixed = 0
    for t in range(a_env.timesteps):
        act = (lo + (hi - lo) * rng.random((E, lo.size))).astype(np.float32)
        act[rng.random(act.shape) < 0.5] = 0
        a_env.step_tensors(torch.from_numpy(act).to(a_env.device))
        flags[:] = 0xdead   # the call writes every env's slot
        _native.check(_native.lib().sng_step_host(b_env._h, P(act), P(obs), P(rew), P(done), P(flags),
                                                  ctypes.byref(b_env._info), ctypes.c_void_p(0)), b_env._h)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(flags, a_env.flags_d.cpu().numpy().astype(np.uint32), err_msg=f"t {t}")
        assert not (flags & ~np.uint32(want)).any()
        sticky |= flags
        np.testing.assert_array_equal(read_sticky(b_env), sticky, err_msg=f"t {t}: sticky flags, host path")
        np.testing.assert_array_equal(read_sticky(a_env), sticky, err_msg=f"t {t}: sticky flags, device path")
        mixed += int(0 < np.count_nonzero(flags) < E)
    # flags were raised per env, not per batch: in both wavefronts, the ragged one included
    assert mixed > 0 and (sticky[:64] == want).any() and (sticky[64:] == want).any()
    a_env.close()
    b_env.close()


def test_step_tensors_converts_its_input():
    """step_tensors takes host, float64 and non-contiguous actions (converted to a contiguous float32 device tensor)
    and refuses a wrong shape; every form steps to the same day."""
    kw = dict(number_of_chargers=4, time_interval="1h", charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse")
    envs = [SmartNanogridVecEnv(64, seed=2, rng="device", **kw) for _ in range(3)]
    for v in envs:
        v.reset_tensors()
    g = torch.Generator().manual_seed(0)
    for t in range(24):
        a = torch.rand((5, 64), generator=g).t()                 # non-contiguous, host, float32
        outs = [envs[0].step_tensors(a.contiguous().to(envs[0].device)),
                envs[1].step_tensors(a),
                envs[2].step_tensors(a.double())]
        for o in outs[1:]:
            assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
    with pytest.raises(ValueError, match="shape"):
        envs[0].step_tensors(torch.zeros((64, 4), device=envs[0].device))
    for v in envs:
        v.close()


def test_single_env_host_step_raises_reference_errors():
    """The host path's per-step flags raise the reference's ValueError at the step that hit it (charging_mode=''
    leaves the positive-action branch unimplemented, charger.py:88) and refuse a wrong action size."""
    env = SmartNanogridEnv(number_of_chargers=3, time_interval="1h", charging_mode="",
                           vehicle_uncharged_penalty_mode="sparse", seed=3)
    env.reset()
    with pytest.raises(ValueError, match="charging mode"):
        for _ in range(24):
            env.step(np.ones(4, np.float32))
    env.close()
    env = SmartNanogridEnv(number_of_chargers=3, time_interval="1h", charging_mode="bounded",
                           vehicle_uncharged_penalty_mode="sparse", seed=3)
    env.reset()
    with pytest.raises(ValueError, match="4 elements"):
        env.step(np.ones(5, np.float32))
    env.close()


def test_reference_errors_are_raised():
    env = SmartNanogridVecEnv(2, number_of_chargers=3, time_interval="1h", charging_mode="",
                              vehicle_uncharged_penalty_mode="sparse")
    env.reset()
    with pytest.raises(ValueError, match="charging mode"):
        for _ in range(24):
            env.step(np.ones((2, 4), np.float32))
    env.close()
    env = SmartNanogridVecEnv(2, number_of_chargers=3, time_interval="1h", charging_mode="bounded",
                              vehicle_uncharged_penalty_mode="")
    with pytest.raises(ValueError, match="penalty mode"):
        env.reset()
    env.close()


@pytest.mark.parametrize("rng", ["device", "reference"])
def test_sharded_population_reproduces_single_gpu(rng):
    """Two handles with env_offset 0 / E/2 (what each rank of a 2-GPU run holds) give the same
    days, rewards and returns as one handle over all E envs."""
    E, N = 2048, 10
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse")
    full = SmartNanogridVecEnv(E, seed=5, rng=rng, **kw)
    halves = [SmartNanogridVecEnv(E // 2, seed=5, rng=rng, env_offset=k * (E // 2), **kw) for k in range(2)]
    acts = torch.rand((24, E, N + 1), device="cuda:0")
    acts[..., -1] = acts[..., -1] * 2 - 1
    for day in range(2):
        o_full = full.reset_tensors().clone()
        o_half = torch.cat([h.reset_tensors().clone() for h in halves])
        assert torch.equal(o_full, o_half)
        for t in range(24):
            of, rf, _ = full.step_tensors(acts[t])
            parts = [h.step_tensors(acts[t, k * (E // 2):(k + 1) * (E // 2)].contiguous()) for k, h in enumerate(halves)]
            assert torch.equal(of, torch.cat([p[0] for p in parts]))
            assert torch.equal(rf, torch.cat([p[1] for p in parts]))
        assert torch.equal(full.return_d, torch.cat([h.return_d for h in halves]))
    for v in [full] + halves:
        v.close()


def test_config4_full_size_eight_shards_reproduce_one_population():
    """BASELINE config 4 (262,144 envs x 10 chargers over 8 GPUs, 32,768 per GPU) at full size on
    one GPU: the 8 shard handles a world-8 run holds (env_offset r * 32,768) step bit for bit like
    one 262,144-env handle, so the RCCL all-gather of their day returns is the single population's
    returns.  Device RNG (the bench's resets), two days."""
    W, E, N = 8, 32768, 10
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse")
    full = SmartNanogridVecEnv(W * E, seed=2024, rng="device", **kw)
    shards = [SmartNanogridVecEnv(E, seed=2024, rng="device", env_offset=r * E, **kw) for r in range(W)]
    g = torch.Generator(device="cuda:0").manual_seed(11)
    for day in range(2):
        of = full.reset_tensors().clone()
        os_ = torch.cat([sh.reset_tensors().clone() for sh in shards])
        assert torch.equal(of, os_)
        for t in range(24):
            a = torch.rand((W * E, N + 1), generator=g, device="cuda:0")
            a[:, -1] = a[:, -1] * 2 - 1
            a = torch.where(torch.rand(a.shape, generator=g, device="cuda:0") < 0.2, torch.zeros_like(a), a)
            o, r, d = full.step_tensors(a)
            parts = [sh.step_tensors(a[k * E:(k + 1) * E].contiguous()) for k, sh in enumerate(shards)]
            assert torch.equal(o, torch.cat([p[0] for p in parts]))
            assert torch.equal(r, torch.cat([p[1] for p in parts]))
            assert torch.equal(d, torch.cat([p[2] for p in parts]))
        gathered = torch.cat([sh.return_d for sh in shards])
        assert torch.equal(full.return_d, gathered)
        ret = gathered.cpu().numpy()
        assert np.isfinite(ret).all() and (ret <= 0).all() and (ret < 0).mean() > 0.99
    for v in [full] + shards:
        v.close()


CONFIG5 = dict(number_of_chargers=50, time_interval="15min", charging_mode="bounded",
               vehicle_uncharged_penalty_mode="sparse", extended_day=True, pv_noise=0.2, price_noise=0.1)


@pytest.mark.parametrize("lanes", [1, 2])
def test_config5_extended_day_stochastic_profiles_vs_oracle(lanes):
    """BASELINE config 5 (50 chargers x 96 15-min steps, stochastic PV + price profiles), a
    build-defined generalisation with no reference oracle: bit-exact against the oracle's
    restatement of the same generalisation, reference RNG, two consecutive days."""
    E, seed = 192, 55
    O.lib().orc_set_square_mode(1)
    venv = SmartNanogridVecEnv(E, seed=seed, rng="reference", step_lanes_per_env=lanes, **CONFIG5)
    assert venv.timesteps == 96 and venv.slots == 97
    cfg, envs = _oracle_batch(CONFIG5, seed, range(E))
    rng = np.random.default_rng(17)
    obs = venv.reset()
    np.testing.assert_array_equal(obs, np.stack([e.reset() for e in envs]))
    for day in range(2):
        if day > 0:
            np.testing.assert_array_equal(obs, np.stack([e.reset() for e in envs]))
        for t in range(cfg.T):
            a = rng.uniform(venv.action_space.low, venv.action_space.high, (E, venv.act_dim)).astype(np.float32)
            a[rng.random(a.shape) < 0.2] = 0
            obs, rew, dones, infos = venv.step(a)
            outs = [e.step(a[i]) for i, e in enumerate(envs)]
            got = np.stack([inf.get("terminal_observation", obs[i]) for i, inf in enumerate(infos)])
            np.testing.assert_array_equal(got, np.stack([o[0] for o in outs]), err_msg=f"day{day} t{t}")
            np.testing.assert_array_equal(rew, np.array([o[1] for o in outs]))
            assert dones.all() == (t == cfg.T - 1)
    venv.close()


def test_config5_full_size_device_rng_day():
    """Config 5 at its full size (65,536 envs x 50 chargers x 96 steps) with GPU-generated days:
    a graph-replayed day equals the eager day bit for bit, and size-independent invariants hold."""
    E = 65536
    acts = torch.rand((96, E, 51), device="cuda:0")
    acts[..., -1] = acts[..., -1] * 2 - 1
    a = SmartNanogridVecEnv(E, seed=3, rng="device", info=True, **CONFIG5)
    b = SmartNanogridVecEnv(E, seed=3, rng="device", **CONFIG5)
    graph = EpisodeGraph(b, acts)
    a.reset_tensors()
    for t in range(96):
        o, r, dn = a.step_tensors(acts[t])
        soc = o[:, 8:58]
        assert bool(torch.isfinite(r).all()) and bool((r <= 0).all())
        assert float(soc.min()) >= 0 and float(soc.max()) <= 1
        assert (a.last_info()["flags"] == 0).all()
    graph.launch()
    torch.cuda.synchronize()
    assert torch.equal(o, b.obs_d) and torch.equal(r, b.reward_d) and torch.equal(a.return_d, b.return_d)
    graph.close()
    a.close()
    b.close()


@pytest.mark.parametrize("E,N", [(1000, 10), (515, 50), (333, 7)])
def test_unaligned_actions_take_the_scalar_staging_path(E, N):
    """Actions at a 4-byte (not 16-byte) aligned address switch the LDS staging to its scalar
    path; results are identical to the aligned run, including ragged last workgroups."""
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="dense")
    a = SmartNanogridVecEnv(E, seed=21, rng="reference", **kw)
    b = SmartNanogridVecEnv(E, seed=21, rng="reference", **kw)
    A = a.act_dim
    oa, ob = a.reset_tensors().clone(), b.reset_tensors().clone()
    assert torch.equal(oa, ob)
    g = torch.Generator(device="cuda:0").manual_seed(4)
    buf = torch.empty(E * A + 1, device="cuda:0")
    for t in range(a.timesteps):
        acts = torch.rand((E, A), generator=g, device="cuda:0")
        unaligned = buf[1:].view(E, A)
        unaligned.copy_(acts)
        assert unaligned.data_ptr() % 16 != 0 and unaligned.is_contiguous()
        oa, ra, da = a.step_tensors(acts)
        ob, rb, db = b.step_tensors(unaligned)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db)
    a.close()
    b.close()


def test_multi_day_graph_matches_eager_days():
    """EpisodeGraph(days=3): three device-RNG days per replay equal three eager days."""
    E, N = 4096, 10
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse")
    acts = torch.rand((24, E, N + 1), device="cuda:0")
    acts[..., -1] = acts[..., -1] * 2 - 1
    a = SmartNanogridVecEnv(E, seed=5, rng="device", **kw)
    b = SmartNanogridVecEnv(E, seed=5, rng="device", **kw)
    graph = EpisodeGraph(b, acts, days=3)
    for rep in range(2):
        for day in range(3):
            a.reset_tensors()
            for t in range(24):
                oa, ra, da = a.step_tensors(acts[t])
        graph.launch()
        torch.cuda.synchronize()
        assert torch.equal(oa, b.obs_d) and torch.equal(ra, b.reward_d) and torch.equal(a.return_d, b.return_d)
        np.testing.assert_array_equal(a.battery_state_of_charge(), b.battery_state_of_charge())
    graph.close()
    a.close()
    b.close()


def test_graph_day_returns_and_overlapped_exchange():
    """EpisodeGraph(day_returns=[D, E]) rows = the eager days' returns; the bench's double-buffered
    asynchronous RCCL exchange (world 1 here) delivers them while the next replay runs."""
    import socket

    import torch.distributed as dist

    from smart_nanogrid_gym.parallel import DayReturnExchange
    E, N, D = 2048, 10, 4
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse")
    acts = torch.rand((24, E, N + 1), device="cuda:0")
    acts[..., -1] = acts[..., -1] * 2 - 1
    a = SmartNanogridVecEnv(E, seed=21, rng="device", **kw)
    b = SmartNanogridVecEnv(E, seed=21, rng="device", **kw)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        x = DayReturnExchange(D, E, torch.device("cuda", 0))
        graphs = [EpisodeGraph(b, acts, days=D, day_returns=x.snap[k]) for k in range(2)]
        want = []
        for rep in range(4):
            k = rep % 2
            x.acquire(k)
            graphs[k].launch()
            x.gather(k)
            days = []
            for _ in range(D):
                a.reset_tensors()
                for t in range(24):
                    a.step_tensors(acts[t])
                days.append(a.return_d.clone())
            want.append(torch.stack(days))
        x.finish()
        torch.cuda.synchronize()
        for k in range(2):   # the last two replays
            assert torch.equal(x.gathered(k), want[2 + k]), k
        for gr in graphs:
            gr.close()
    finally:
        dist.destroy_process_group()
    a.close()
    b.close()
