"""GPU: the day kernel (day_wide_kernel, csrc/sng_step_day.h) -- a captured day's T steps as one graph node with
SoC, BESS SoC and the day return in registers -- against the same days captured as T step nodes
(EpisodeGraph(step_nodes=True)), against eager steps, and, independently of the step kernel, against the CPU oracle.

Twin handles with the same seed replay their graphs side by side; after every replay everything a caller can
read must be equal bit for bit: the last step's observations, reward and done, the day returns, the BESS SoC,
the day counter, the sticky error flags and the whole checkpoint (which holds every charger's SoC).

The day kernel exists for the 10-charger station of the wide family (no V2X, no stochastic profiles).  The
50-charger cases below run the same comparison: their graphs keep T step nodes today (N = 50 would spill, see
sng_kernels.hip), and they start checking the day kernel the day that station gets one.
"""
import ctypes

import numpy as np
import pytest

import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smart_nanogrid_gym import SmartNanogridVecEnv  # noqa: E402
from smart_nanogrid_gym._native import check, lib  # noqa: E402
from smart_nanogrid_gym.vec_env import EpisodeGraph  # noqa: E402
from test_gpu_bench_kernel import actions as bench_actions, load_day  # noqa: E402

KW10 = dict(number_of_chargers=10, time_interval="1h", charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse",
            pv_system_available_in_model=True, battery_system_available_in_model=True)
KW50 = dict(number_of_chargers=50, time_interval="15min", charging_mode="bounded",
            vehicle_uncharged_penalty_mode="sparse", extended_day=True, pv_noise=0.2, price_noise=0.1)


def make_actions(T, E, A, seed, low=0.0, offset_floats=0):
    """[T, E, A] device actions: chargers U[low, 1] with a fifth exact zeros, BESS U[-1, 1]; offset_floats moves
    the tensor's address off 16-byte alignment."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand((T, E, A), generator=g) * (1.0 - low) + low
    a[..., -1] = torch.rand((T, E), generator=g) * 2 - 1
    a[torch.rand((T, E, A), generator=g) < 0.2] = 0.0
    flat = torch.zeros(T * E * A + offset_floats, device="cuda:0")
    flat[offset_floats:] = a.reshape(-1).to("cuda:0")
    out = flat[offset_floats:].view(T, E, A)
    assert out.data_ptr() % 16 == (4 * offset_floats) % 16
    return out


def flags_of(v):
    f = np.zeros(v.num_envs, np.uint32)
    with torch.cuda.device(v.device):
        check(lib().sng_read_errors(v._h, f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 0, None), v._h)
    return f


def assert_same(a, b, what):
    torch.cuda.synchronize()
    assert torch.equal(a.obs_d, b.obs_d), what
    assert torch.equal(a.reward_d, b.reward_d), what
    assert torch.equal(a.done_d, b.done_d), what
    assert torch.equal(a.return_d, b.return_d), what
    assert np.array_equal(a.battery_state_of_charge(), b.battery_state_of_charge()), what
    assert a.day_counter() == b.day_counter(), what
    assert np.array_equal(flags_of(a), flags_of(b)), what
    assert a.save_state() == b.save_state(), what


def twin_replays(E, kw, acts, days=1, seed=5, with_returns=False, day_kernel=True):
    """Three replays of twin graphs, T step nodes against the default form; returns the flags raised."""
    a = SmartNanogridVecEnv(E, seed=seed, rng="device", **kw)
    b = SmartNanogridVecEnv(E, seed=seed, rng="device", **kw)
    ra = torch.zeros((days, E), dtype=torch.float64, device="cuda:0") if with_returns else None
    rb = torch.zeros((days, E), dtype=torch.float64, device="cuda:0") if with_returns else None
    ga = EpisodeGraph(a, acts, days=days, day_returns=ra, step_nodes=True)
    gb = EpisodeGraph(b, acts, days=days, day_returns=rb)
    assert ga.step_nodes_per_day == a.timesteps
    assert gb.step_nodes_per_day == (1 if day_kernel else b.timesteps)
    for rep in range(3):
        ga.launch()
        gb.launch()
        assert_same(a, b, f"replay {rep}")
        if with_returns:
            assert torch.equal(ra, rb) and bool((ra != 0).any()), f"replay {rep}"
    fl = flags_of(b)
    ga.close()
    gb.close()
    a.close()
    b.close()
    return fl


@pytest.mark.parametrize("E", [33, 100])   # 32 envs per wavefront: a ragged last wavefront
@pytest.mark.parametrize("mode", ["sparse", "dense"])
def test_two_days_match_step_nodes(E, mode):
    kw = dict(KW10, vehicle_uncharged_penalty_mode=mode)
    twin_replays(E, kw, make_actions(24, E, 11, seed=E), days=2)


def test_requested_soc_stream():
    kw = dict(KW10, enable_requested_state_of_charge=True)
    twin_replays(70, kw, make_actions(24, 70, 11, seed=1))


def test_negative_actions_take_the_general_order():
    """A negative charger action sends the wavefront through the general-order path, which keeps memory as its SoC
    state: the day kernel writes its SoC registers back before it and reloads them after it."""
    fl = twin_replays(70, KW10, make_actions(24, 70, 11, seed=2, low=-1.0))
    assert fl.any()


def test_config5_station():
    twin_replays(70, KW50, make_actions(96, 70, 51, seed=3), day_kernel=False)


def test_config5_station_v2x_raises_flags():
    kw = dict(KW50, vehicle_to_everything=True)
    fl = twin_replays(70, kw, make_actions(96, 70, 51, seed=4, low=-1.0), day_kernel=False)
    assert fl.any()


def test_actions_at_a_4_byte_aligned_address():
    twin_replays(33, KW10, make_actions(24, 33, 11, seed=6, offset_floats=1))


def test_day_returns_rows():
    twin_replays(64, KW10, make_actions(24, 64, 11, seed=7), days=2, with_returns=True)


def test_steps_only_graph_matches_eager_over_a_generated_day_and_its_replay():
    E = 70
    acts = make_actions(24, E, 11, seed=8)
    v = SmartNanogridVecEnv(E, seed=9, rng="device", **KW10)
    w = SmartNanogridVecEnv(E, seed=9, rng="device", **KW10)
    for new_day in (lambda x: x.reset_tensors(), lambda x: x.replay_tensors()):
        new_day(v)
        new_day(w)
        g = EpisodeGraph(v, acts, with_reset=False)
        assert g.step_nodes_per_day == 1
        g.launch()
        for t in range(24):
            w.step_tensors(acts[t])
        assert_same(v, w, "steps-only graph")
        g.close()
    v.close()
    w.close()


def test_replayed_day_with_a_requested_soc_plane():
    """A replayed day of a station with the requested SoC enabled: the replay clears the requests (req_zero), so
    the plan drops REQ and the day kernel is the one without the stream, on a day whose req plane exists."""
    E = 70
    kw = dict(KW10, enable_requested_state_of_charge=True)
    acts = make_actions(24, E, 11, seed=10)
    v = SmartNanogridVecEnv(E, seed=11, rng="device", **kw)
    w = SmartNanogridVecEnv(E, seed=11, rng="device", **kw)
    for x in (v, w):
        x.reset_tensors()
        assert x.step_kernel_name() == "void sng::step_wide_kernel<10, 2, true, true, false>"
        for t in range(24):   # the generated day itself, with its requests
            x.step_tensors(acts[t])
        x.replay_tensors()
        assert x.step_kernel_name() == "void sng::step_wide_kernel<10, 2, true, false, false>"
    g = EpisodeGraph(v, acts, with_reset=False)
    assert g.step_nodes_per_day == 1
    g.launch()
    for t in range(24):
        w.step_tensors(acts[t])
    assert_same(v, w, "steps-only graph of a replayed day with a req plane")
    assert bool((v.return_d != 0).any())
    g.close()
    v.close()
    w.close()


@pytest.fixture()
def square_mode():
    O.lib().orc_set_square_mode.argtypes = [ctypes.c_int]
    O.lib().orc_set_square_mode(1)   # x*x squares, as on the GPU
    yield
    O.lib().orc_set_square_mode(0)


def test_day_kernel_vs_oracle(square_mode):
    """Independent of the step kernel: a generated device day exported to the CPU oracle and stepped there."""
    E, T, A = 96, 24, 11
    v = SmartNanogridVecEnv(E, seed=2025, rng="device", **KW10)
    v.reset_tensors()
    ivs, ratios = v.get_scenarios(0, E)
    envs = [O.OracleEnv(O.OracleConfig(**KW10), 0) for _ in range(E)]
    for e, iv, r in zip(envs, ivs, ratios):
        load_day(e, iv, r)
    rng = np.random.default_rng(E)
    heavy = (np.arange(E) % 4) == 0
    acts = np.stack([bench_actions(rng, E, A, heavy) for _ in range(T)])
    g = EpisodeGraph(v, torch.from_numpy(acts).to(v.device), with_reset=False)
    assert g.step_nodes_per_day == 1
    g.launch()
    torch.cuda.synchronize()
    ret = np.zeros(E)
    for t in range(T):
        outs = [e.step(acts[t, i]) for i, e in enumerate(envs)]
        ret = ret + np.array([x[1] for x in outs])
    np.testing.assert_array_equal(v.obs_d.cpu().numpy(), np.stack([x[0] for x in outs]))
    np.testing.assert_array_equal(v.reward_d.cpu().numpy(), np.array([x[1] for x in outs]))
    np.testing.assert_array_equal(v.return_d.cpu().numpy(), ret)
    np.testing.assert_array_equal(v.battery_state_of_charge(), np.array([e.bess_soc for e in envs]))
    assert bool(v.done_d.cpu().numpy().all())
    g.close()
    v.close()
