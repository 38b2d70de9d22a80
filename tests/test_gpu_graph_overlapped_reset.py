"""GPU: the overlapped reset graph (sng_graph_create; csrc/sng_graph_form.h reset_overlapped) -- day d + 1 generated
into a second day slot while day d is stepped -- against the serial chain of the same days
(EpisodeGraph(serial_reset=True), SNG_GRAPH_SERIAL_RESET).

Twin handles with the same seed replay their graphs side by side.  After every one of three launches everything a
caller can read must be equal bit for bit: the last step's observations, reward and done, the day return row and
every day_returns row, the BESS SoC, the PV ratio, the sticky flags, the day counter, the loaded day's export
(get_scenarios) and the whole checkpoint (the loaded day's timeline, every charger's SoC).  After the replays an
eager device reset and one step on both handles agree as well: the next day index is right and the loaded day is
in the handle's own buffers.

The matrix: 2, 3 and 4 days (both parities of the slot rotation: the last day is always in the handle's own slot);
70 envs (two full 32-env wavefronts and one of 6) and 4,096 (enough for the generator and the day kernel to be in
flight together); day_wide_kernel, its T step nodes, day_lean_kernel (whose default is the serial chain: overlapped
by SNG_GRAPH_OVERLAPPED_RESET), and the requested-SoC stream; without and with day_returns.  One row is stepped through the CPU oracle from the oracle's own model of the device days
(oracle.device_day), independently of the serial form.
"""
import ctypes

import numpy as np
import pytest

import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smart_nanogrid_gym import SmartNanogridVecEnv  # noqa: E402
from smart_nanogrid_gym.vec_env import EpisodeGraph  # noqa: E402
from device_day_cases import padded  # noqa: E402
from test_gpu_bench_kernel import actions as bench_actions  # noqa: E402
from test_gpu_day_kernel import KW10, flags_of, make_actions  # noqa: E402

KW8 = dict(KW10, number_of_chargers=8)
STATIONS = {
    # name: (env kwargs, EpisodeGraph kwargs, step nodes per day)
    "wide10": (KW10, {}, 1),
    "wide10_step_nodes": (KW10, dict(step_nodes=True), 24),
    # the lean stations' default is the serial chain (csrc/sng_graph_form.h): overlapped by the flag
    "lean8": (KW8, dict(overlapped_reset=True), 1),
    "wide10_req": (dict(KW10, enable_requested_state_of_charge=True), {}, 1),
}
EXPORTED = 70   # envs whose export is decoded (the checkpoint holds every env's timeline)


def assert_same(a, b, what):
    torch.cuda.synchronize()
    assert torch.equal(a.obs_d, b.obs_d), what
    assert torch.equal(a.reward_d, b.reward_d), what
    assert torch.equal(a.done_d, b.done_d), what
    assert torch.equal(a.return_d, b.return_d), what
    assert np.array_equal(a.battery_state_of_charge(), b.battery_state_of_charge()), what
    assert np.array_equal(a.pv_ratio(), b.pv_ratio()), what
    assert a.day_counter() == b.day_counter(), what
    assert np.array_equal(flags_of(a), flags_of(b)), what
    first = a.num_envs - EXPORTED   # the last envs: the ragged wavefront's
    (iva, ra), (ivb, rb) = a.get_scenarios(first, EXPORTED), b.get_scenarios(first, EXPORTED)
    assert np.array_equal(ra, rb) and iva == ivb, what   # plain lists of finite numbers
    assert a.save_state() == b.save_state(), what


def twins(E, kw, seed):
    return (SmartNanogridVecEnv(E, seed=seed, rng="device", **kw), SmartNanogridVecEnv(E, seed=seed, rng="device", **kw))


def eager_day_start(a, b, acts, what):
    """An eager device reset and one step on both handles: the same next day from the same state."""
    oa, ob = a.reset_tensors(), b.reset_tensors()
    torch.cuda.synchronize()
    assert torch.equal(oa, ob), what
    a.step_tensors(acts[0])
    b.step_tensors(acts[0])
    torch.cuda.synchronize()
    assert torch.equal(a.obs_d, b.obs_d) and torch.equal(a.reward_d, b.reward_d), what
    assert a.day_counter() == b.day_counter(), what
    assert a.save_state() == b.save_state(), what


def twin_replays(E, station, days, with_returns, seed, overlapped=True, unstepped_reset=False, **graph_kw):
    kw, gkw, nodes = STATIONS[station]
    gkw = dict(gkw, **graph_kw)
    a, b = twins(E, kw, seed)
    acts = make_actions(a.timesteps, E, a.act_dim, seed=seed)
    ra = torch.zeros((days, E), dtype=torch.float64, device="cuda:0") if with_returns else None
    rb = torch.zeros((days, E), dtype=torch.float64, device="cuda:0") if with_returns else None
    ga = EpisodeGraph(a, acts, days=days, day_returns=ra, serial_reset=True, **gkw)   # wins over overlapped_reset
    gb = EpisodeGraph(b, acts, days=days, day_returns=rb, **gkw)
    assert not ga.reset_overlapped
    assert gb.reset_overlapped == overlapped
    assert ga.step_nodes_per_day == gb.step_nodes_per_day
    if not gkw.get("trajectory"):
        assert gb.step_nodes_per_day == nodes
    if unstepped_reset:   # a device day that is reset and never stepped still owns its day index
        a.reset_tensors()
        b.reset_tensors()
    day0 = b.day_counter()
    for rep in range(3):
        ga.launch()
        gb.launch()
        what = f"{station} E={E} days={days} replay {rep}"
        assert_same(a, b, what)
        assert b.day_counter() == day0 + int(unstepped_reset) + days * (rep + 1), what
        if with_returns:
            assert torch.equal(ra, rb), what
            assert all(bool((ra[d] != 0).any()) for d in range(days)), what
        else:
            assert bool((b.return_d != 0).any()), what
        if gkw.get("trajectory"):
            assert torch.equal(ga.obs_traj, gb.obs_traj) and torch.equal(ga.reward_traj, gb.reward_traj), what
            assert torch.equal(ga.done_traj, gb.done_traj), what
    eager_day_start(a, b, acts, f"{station} E={E} days={days} eager day after the replays")
    for x in (ga, gb, a, b):
        x.close()


@pytest.mark.parametrize("with_returns", [False, True], ids=["return_row", "day_returns"])
@pytest.mark.parametrize("station", list(STATIONS))
@pytest.mark.parametrize("E", [70, 4096])
@pytest.mark.parametrize("days", [2, 3, 4])
def test_overlapped_graph_equals_the_serial_chain(days, E, station, with_returns):
    twin_replays(E, station, days, with_returns, seed=100 * days + len(station))


def test_launch_after_an_unstepped_device_reset():
    twin_replays(70, "wide10", 3, False, seed=31, unstepped_reset=True)


@pytest.mark.parametrize("graph_kw,days", [(dict(trajectory=True), 2), ({}, 1)], ids=["trajectory", "one_day"])
def test_graphs_that_stay_serial(graph_kw, days):
    """Trajectory graphs and one-day graphs are captured as before, and still equal their SNG_GRAPH_SERIAL_RESET
    twins (which are then the same graph)."""
    twin_replays(70, "lean8", days, False, seed=32, overlapped=False, **graph_kw)   # even with the flag
    twin_replays(70, "wide10", days, False, seed=33, overlapped=False, **graph_kw)


def test_lean_station_default_is_serial():
    v = SmartNanogridVecEnv(70, seed=1, rng="device", **KW8)
    acts = make_actions(v.timesteps, 70, v.act_dim, seed=1)
    g = EpisodeGraph(v, acts, days=2)
    assert not g.reset_overlapped
    g.close()
    v.close()


@pytest.fixture()
def square_mode():
    O.lib().orc_set_square_mode.argtypes = [ctypes.c_int]
    O.lib().orc_set_square_mode(1)   # x*x squares, as on the GPU
    yield
    O.lib().orc_set_square_mode(0)


def test_last_day_of_three_vs_oracle(square_mode):
    """Independent of the serial form: the three days of one overlapped replay taken from the oracle's model of the
    device days (day indices 0, 1, 2 of the seed) and stepped by oracle envs, the BESS SoC carried from day to
    day.  What the replay leaves -- the last day's export, its last observations, rewards, day return, and the BESS
    SoC -- is the model's third day.  An eager twin handle exports each day's arrivals for the model's one
    excused value, the geometric wait within 1e-5 of an integer (test_gpu_device_day_exact.py)."""
    E, T, A, seed, days = 70, 24, 11, 77, 3
    cfg = O.OracleConfig(**KW10)
    v = SmartNanogridVecEnv(E, seed=seed, rng="device", **KW10)
    w = SmartNanogridVecEnv(E, seed=seed, rng="device", **KW10)
    rng = np.random.default_rng(E)
    heavy = (np.arange(E) % 4) == 0
    acts = np.stack([bench_actions(rng, E, A, heavy) for _ in range(T)])
    g = EpisodeGraph(v, torch.from_numpy(acts).to(v.device), days=days)
    assert g.reset_overlapped and g.step_nodes_per_day == 1
    g.launch()
    torch.cuda.synchronize()
    assert v.day_counter() == days
    envs = [O.OracleEnv(cfg, seed + e) for e in range(E)]
    for day in range(days):
        w.reset_tensors()   # never stepped: the next reset counts it
        assert w.day_counter() == day
        follow = [padded(iv["Arrivals"]) for iv in w.get_scenarios()[0]]
        model = [O.device_day(cfg, seed, e, day, follow[e]) for e in range(E)]
        for env, m in zip(envs, model):
            env.load(m["soc"], m["occ"], m["cap"], m["req"], m["arrivals"], m["departures"], m["ratio"])
        ret = np.zeros(E)
        for t in range(T):
            outs = [env.step(acts[t, i]) for i, env in enumerate(envs)]
            ret = ret + np.array([x[1] for x in outs])
    ivs, ratios = v.get_scenarios()
    np.testing.assert_array_equal(ratios, np.array([m["ratio"] for m in model]))
    for iv, m in zip(ivs, model):
        np.testing.assert_array_equal(padded(iv["Arrivals"]), m["arrivals"])
        np.testing.assert_array_equal(padded(iv["Departures"]), m["departures"])
        np.testing.assert_array_equal(np.asarray(iv["SOC"]), m["soc"])
        np.testing.assert_array_equal(np.asarray(iv["Vehicle_capacities"]), m["cap"])
    np.testing.assert_array_equal(v.obs_d.cpu().numpy(), np.stack([x[0] for x in outs]))
    np.testing.assert_array_equal(v.reward_d.cpu().numpy(), np.array([x[1] for x in outs]))
    np.testing.assert_array_equal(v.return_d.cpu().numpy(), ret)
    np.testing.assert_array_equal(v.battery_state_of_charge(), np.array([env.bess_soc for env in envs]))
    assert bool(v.done_d.cpu().numpy().all())
    for x in (g, v, w):
        x.close()
