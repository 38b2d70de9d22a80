"""GPU: the day kernel's step loop (day_wide_kernel, csrc/sng_step_day.h; WideGroup::run<KEEP>, csrc/sng_step_wide.h)
where what one step leaves in registers or in flight meets the next: the loop edge, the day boundary, the rare
paths beside the fast path, and the flags.

The kernel issues a step's loads a step ahead, drains them before the stores of the step in between, reads the
step's table constants at the step's own top and carries SoC, BESS SoC and the day return in registers.  None of
that may change a bit.  Every case uses the 10-charger station and device-RNG days, and compares bit for bit (NaN
equal to NaN): the last step's observations, rewards and dones, every day's returns, every charger's SoC, the BESS
SoC, the day counter, the sticky flags, the flag summary and the checkpoint -- captured days (one day-kernel node
per day) against eager resets and steps on a twin handle of the same seed, and, where it says so, the eager twin
against the CPU oracle at every step (the oracle is given each day as the GPU generated it).
"""
import numpy as np
import pytest

import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import wide_rebuild_cases as R  # noqa: E402
import wild_action_cases as W  # noqa: E402
from smart_nanogrid_gym import SmartNanogridVecEnv, _native  # noqa: E402
from smart_nanogrid_gym.vec_env import EpisodeGraph  # noqa: E402
from station_matrix_cases import square_mode  # noqa: E402
from test_gpu_day_kernel import KW10, flags_of  # noqa: E402
from test_gpu_station_matrix import load_exported_day  # noqa: E402

SEED = 77
ND = _native.FLAG_NEGATIVE_DEMAND
TINY = np.float32(1e-45)   # the smallest positive float32 (2^-149)


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    square_mode(True)   # x*x squares, as on the GPU
    yield
    square_mode(False)


def same(a, b, what):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    b = b.cpu().numpy() if hasattr(b, "cpu") else np.asarray(b)
    np.testing.assert_array_equal(a, b, err_msg=what)


def assert_same_handles(a, b, what):
    torch.cuda.synchronize()
    for k in ("obs_d", "reward_d", "done_d", "return_d", "flag_summary_d"):
        same(getattr(a, k), getattr(b, k), f"{what}: {k}")
    same(a.vehicle_state_of_charge(), b.vehicle_state_of_charge(), what + ": every charger's SoC")
    same(a.battery_state_of_charge(), b.battery_state_of_charge(), what + ": BESS SoC")
    assert a.day_counter() == b.day_counter(), what
    same(flags_of(a), flags_of(b), what + ": sticky flags")
    assert a.save_state() == b.save_state(), what + ": checkpoint"


def station(interval="1h", **more):
    kw = dict(KW10, time_interval=interval, **more)
    if "min" in interval:
        kw["extended_day"] = True
    return kw


def nonneg_actions(T, E, seed):
    """[T, E, 11] float32: chargers U[0, 1) with a fifth exact zeros, BESS U[-1, 1)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 1.0, (T, E, 11)).astype(np.float32)
    a[..., 10] = rng.uniform(-1.0, 1.0, (T, E))
    a[rng.random(a.shape) < 0.2] = 0.0
    return a


def captured_vs_eager(E, kw, actions, days, oracle=False, seed=SEED):
    """`days` days as ONE captured graph -- per day a reset and one day-kernel node -- against eager resets and
    steps on a twin of the same seed; with `oracle`, every eager day goes into the CPU oracle as generated and
    every eager step is held against it.  `actions(T)` gives the [T, E, 11] float32 array, reused every day.
    Returns the eager twin's sticky flags, its vehicles' SoC after the last day and the first day as exported."""
    eager = SmartNanogridVecEnv(E, seed=seed, rng="device", **kw)
    T = eager.timesteps
    acts = actions(T)
    assert acts.shape == (T, E, 11) and acts.dtype == np.float32
    acts_d = torch.from_numpy(acts).to(eager.device)
    same(acts_d, acts, "the actions' bits reach the device")
    cfg = O.OracleConfig(**kw) if oracle else None
    envs = [O.OracleEnv(cfg, 0) for _ in range(E)] if oracle else None
    day_returns, first_day = [], None
    for day in range(days):
        obs = eager.reset_tensors()
        ivs = None
        if oracle or day == 0:
            ivs, ratios = eager.get_scenarios(0, E)
            first_day = first_day or ivs
        if oracle:
            same(obs, np.stack([load_exported_day(e, iv, r) for e, iv, r in zip(envs, ivs, ratios)]), f"day {day}: reset")
        for t in range(T):
            o, r, d = eager.step_tensors(acts_d[t])
            if oracle:
                outs = [e.step(acts[t, i]) for i, e in enumerate(envs)]
                same(o, np.stack([x[0] for x in outs]), f"day {day} t {t}: obs vs oracle")
                same(r, np.array([x[1] for x in outs]), f"day {day} t {t}: reward vs oracle")
        torch.cuda.synchronize()
        assert bool(eager.done_d.all())
        if oracle:
            same(eager.battery_state_of_charge(), np.array([e.bess_soc for e in envs]), f"day {day}: BESS SoC vs oracle")
        day_returns.append(eager.return_d.cpu().numpy().copy())
    h = SmartNanogridVecEnv(E, seed=seed, rng="device", **kw)
    rets = torch.zeros((days, E), dtype=torch.float64, device=h.device)
    g = EpisodeGraph(h, acts_d, days=days, day_returns=rets)
    assert g.step_nodes_per_day == 1, g.step_nodes_per_day   # the day kernel
    g.launch()
    torch.cuda.synchronize()
    same(rets, np.stack(day_returns), "every day's returns")
    h.return_d.copy_(rets[days - 1])   # the graph's returns went into its day_returns rows, not into return_d
    assert_same_handles(h, eager, f"{days} captured days vs eager steps")
    out = flags_of(eager), eager.vehicle_state_of_charge(), first_day
    g.close()
    h.close()
    eager.close()
    return out


@pytest.mark.parametrize("interval", ["1h", "2h", "15min"])   # 24 steps, 12 (the shortest day) and 96 (the longest)
@pytest.mark.parametrize("E", [33, 70])   # a wavefront with one live env; a partial third wavefront
def test_three_captured_days_vs_eager_steps_and_oracle(E, interval):
    """State carried over the loop edge and over the day boundary: three days with their resets in one graph."""
    captured_vs_eager(E, station(interval), lambda T: nonneg_actions(T, E, seed=E + T), days=3, oracle=True)


def test_mixed_wavefront_zero_one_and_smallest_actions():
    """One wavefront, one step: lanes with an occupied charger beside lanes with an empty one, under actions of
    exactly 0, exactly 1.0 (the SoC saturates at 1) and the smallest positive float32."""
    E = 64

    def actions(T):
        a = nonneg_actions(T, E, seed=3)
        rng = np.random.default_rng(4)
        pick = rng.integers(0, 4, (T, 32, 10))   # the first wavefront: 0, 1.0, 2^-149, or the uniform draw
        w = a[:, :32, :10]
        w[pick == 0] = 0.0
        w[pick == 1] = 1.0
        w[pick == 2] = TINY
        for v in (0.0, 1.0, TINY):
            assert (w == np.float32(v)).any(axis=(1, 2)).all(), v   # each of them at every step
        return a

    _, soc, first_day = captured_vs_eager(E, station(), actions, days=2, oracle=True)
    occ = np.stack([np.asarray(iv["Charger_occupancy"]) for iv in first_day[:32]])   # [env, charger, step]
    assert occ.shape[:2] == (32, 10), occ.shape
    assert ((occ.min(axis=0) == 0) & (occ.max(axis=0) == 1)).any(), "no charger occupied in one env and empty in another"
    assert (soc[:32] == 1.0).any(), "no vehicle charged to exactly 1.0"


def test_one_negative_env_sends_only_its_wavefront_through_the_general_order():
    E = 96

    def actions(T):
        a = nonneg_actions(T, E, seed=5)
        a[::2, 40, 3] = -0.5
        for t in range(T):   # the other wavefronts stay on the fast path
            assert list(W.fast_wavefront(a[t], 10)) == [True, t % 2 == 1, True]
        return a

    captured_vs_eager(E, station(), actions, days=2)


def test_nan_and_inf_actions_beside_the_fast_path():
    """wild_action_cases' device-day row: +inf and overflowing products in the fast wavefronts, NaN, -inf and negative
    actions in the second wavefront at even steps."""
    row = W.ROWS[W.IDS.index("wide10_device_day")]
    assert row.day_kernel

    def actions(T):
        a = W.row_actions(row, T)
        assert np.isnan(a[:, 32:64, :10]).any() and np.isposinf(a[:, :32, :10]).any()
        assert all(W.fast_wavefront(a[t], 10)[0] and W.fast_wavefront(a[t], 10)[2] for t in range(T))
        return a

    fl, soc, _ = captured_vs_eager(W.E, row.kw, actions, days=W.DAYS, seed=W.SEED)
    assert (fl[32:64] & ND).any() and not fl[:32].any() and not fl[64:].any()
    assert np.isfinite(soc).all()


def test_rebuilt_sums_through_a_captured_day():
    """wide_rebuild_cases: inexact sums of eight or more positive powers (pos_slow), whole wavefronts by category."""
    kw, rng, _, day_kernel = R.STATIONS["n10_device"]
    assert rng == "device" and day_kernel
    captured_vs_eager(R.E, kw, lambda T: R.rebuild_actions(10, T), days=1, seed=R.SEED)


def test_flag_raised_at_one_step_and_not_at_the_next():
    """Envs that raise NEGATIVE_DEMAND at step 7 only: the sticky word and the summary of the day kernel are those of
    the day's T step nodes."""
    E, t_flag, who = 70, 7, [5, 37, 69]
    acts = nonneg_actions(24, E, seed=6)
    acts[t_flag, who, :10] = -1.0
    acts_d = torch.from_numpy(acts).to("cuda:0")
    a = SmartNanogridVecEnv(E, seed=SEED, rng="device", **KW10)
    b = SmartNanogridVecEnv(E, seed=SEED, rng="device", **KW10)
    ga = EpisodeGraph(a, acts_d, days=2, step_nodes=True)
    gb = EpisodeGraph(b, acts_d, days=2)
    assert ga.step_nodes_per_day == 24 and gb.step_nodes_per_day == 1
    for rep in range(2):
        ga.launch()
        gb.launch()
        assert_same_handles(b, a, f"replay {rep}: day kernel vs step nodes")
    fl = flags_of(b)
    others = np.setdiff1d(np.arange(E), who)
    assert (fl[who] & ND).any() and not fl[others].any(), fl
    assert bool(b.flag_summary_d.any())
    for x in (ga, gb, a, b):
        x.close()
