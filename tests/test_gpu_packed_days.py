"""GPU: every step kernel family's handling of a device-RNG day's packed records (PK = true) -- the STATIC bit
masked out of the record, no aux plane, an empty charger's SoC and departure entry taken from the record --
pinned to the general diagnostics kernel and, independently of any kernel, to the CPU oracle.

One 1 h day (T = 24) of E = 70 envs per row: the last wavefront is ragged both at 64 envs per wavefront
(64 + 6) and at 32 (32 + 32 + 6).  Each row asserts the kernel it is there for by its name, and steps a twin
handle with info=True (the general kernel with DIAG and PK) on the same day with the same actions: observations
and rewards of all 70 envs are equal at every step, the sticky flags and the BESS SoC after the day.  The day
is exported (get_scenarios) and loaded into oracle envs, which are stepped with the same actions, bit-exact.

SEED was chosen on the CPU with oracle.device_day (the model tests/test_device_day_model_cpu.py pins): in every
row's day some charger is empty at some step, some vehicle arrives after t = 0 and some vehicle departs before
T, so empty, arriving and departing records are all stepped.  Each row asserts that of the exported day.
"""
import ctypes

import numpy as np
import pytest

import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smart_nanogrid_gym import SmartNanogridVecEnv  # noqa: E402
from smart_nanogrid_gym._native import check, lib  # noqa: E402
from test_gpu_bench_kernel import load_day  # noqa: E402

E, T, SEED = 70, 24, 4242
BASE = dict(time_interval="1h", charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse",
            pv_system_available_in_model=True, battery_system_available_in_model=True)
GENERAL_DIAG = ", 1, true, true, true>"   # the twin: step_kernel<NC, 1, DIAG, FAST, PK>

# row: (station, handle-only arguments, the kernel's name prefix, a negative action in the first 32 envs)
ROWS = {
    "lean_n4": (dict(number_of_chargers=4), {}, "void sng::step_lean_kernel<4, true, ", False),
    "lean_n10_v2x": (dict(number_of_chargers=10, vehicle_to_everything=True), {},
                     "void sng::step_lean_kernel<10, true, ", False),
    "wide_n10_fast_loop": (dict(number_of_chargers=10), {}, "void sng::step_wide_kernel<10, 2, true, ", False),
    "wide_n10_one_wave_general_order": (dict(number_of_chargers=10), {},
                                        "void sng::step_wide_kernel<10, 2, true, ", True),
    "wide_n50": (dict(number_of_chargers=50), {}, "void sng::step_wide_kernel<50, 2, true, ", False),
    "general_runtime_n7": (dict(number_of_chargers=7), {}, "void sng::step_kernel<0, 1, false, true, true>", False),
    "general_two_lanes_n10": (dict(number_of_chargers=10), dict(step_lanes_per_env=2),
                              "void sng::step_kernel<10, 2, false, true, true>", False),
}


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    O.lib().orc_set_square_mode.argtypes = [ctypes.c_int]
    O.lib().orc_set_square_mode(1)   # x*x squares, as on the GPU
    yield
    O.lib().orc_set_square_mode(0)


def sticky_flags(v):
    f = np.zeros(v.num_envs, np.uint32)
    with torch.cuda.device(v.device):
        check(lib().sng_read_errors(v._h, f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 0, None), v._h)
    return f


def day_actions(venv, negative):
    """[T, E, A] Box-uniform actions (chargers in [-1, 1] with V2X), a fifth exact zeros, a twentieth exactly the
    upper bound.  negative: one charger action of one env of the first 32 is negative at every step."""
    rng = np.random.default_rng(venv.act_dim)
    lo, hi = venv.action_space.low, venv.action_space.high
    a = (lo + (hi - lo) * rng.random((T, E, venv.act_dim))).astype(np.float32)
    r = rng.random(a.shape)
    a[r < 0.2] = 0.0
    top = (r >= 0.2) & (r < 0.25)
    a[top] = hi[np.nonzero(top)[2]]
    if negative:
        assert (a[:, :, :-1] >= 0).all()
        for t in range(T):
            a[t, (5 * t) % 32, t % (venv.act_dim - 1)] = -0.5
    return a


@pytest.mark.parametrize("row", sorted(ROWS))
def test_packed_day_vs_general_kernel_and_oracle(row):
    station, handle_kw, prefix, negative = ROWS[row]
    kw = dict(BASE, **station)
    N = kw["number_of_chargers"]
    venv = SmartNanogridVecEnv(E, seed=SEED, rng="device", **kw, **handle_kw)
    twin = SmartNanogridVecEnv(E, seed=SEED, rng="device", info=True, **kw)
    assert venv.timesteps == T
    obs = venv.reset_tensors().cpu().numpy()
    np.testing.assert_array_equal(obs, twin.reset_tensors().cpu().numpy())
    assert venv.step_kernel_name().startswith(prefix), venv.step_kernel_name()
    name = twin.step_kernel_name()
    assert name.startswith("void sng::step_kernel<") and name.endswith(GENERAL_DIAG), name

    # the day, independently of any step kernel: into the oracle
    ivs, ratios = venv.get_scenarios(0, E)
    occ = np.array([iv["Charger_occupancy"] for iv in ivs])[:, :, :T]
    arrivals = np.concatenate([np.ravel(x) for iv in ivs for x in iv["Arrivals"]])
    departures = np.concatenate([np.ravel(x) for iv in ivs for x in iv["Departures"]])
    assert (occ == 0).any() and (arrivals > 0).any() and (departures < T).any(), row
    ids = np.arange(32, E) if negative else np.arange(E)   # the negative actions are outside this station's Box
    cfg = O.OracleConfig(**kw)
    envs = [O.OracleEnv(cfg, 0) for _ in ids]   # the days come from the GPU: the oracle's own RNG is unused
    ref0 = np.stack([load_day(e, ivs[i], ratios[i]) for e, i in zip(envs, ids)])
    np.testing.assert_array_equal(obs[ids], ref0, err_msg=f"{row}: reset")

    acts = day_actions(venv, negative)
    assert (acts[:, :32, :N] < 0).any() == (negative or "vehicle_to_everything" in kw)
    acts_d = torch.from_numpy(acts).to(venv.device)
    for t in range(T):
        o, r, d = venv.step_tensors(acts_d[t])
        ot, rt, _ = twin.step_tensors(acts_d[t])
        o, r = o.cpu().numpy(), r.cpu().numpy()
        np.testing.assert_array_equal(o, ot.cpu().numpy(), err_msg=f"{row} t {t}: vs general kernel")
        np.testing.assert_array_equal(r, rt.cpu().numpy(), err_msg=f"{row} t {t}: vs general kernel")
        outs = [e.step(acts[t, i]) for e, i in zip(envs, ids)]
        np.testing.assert_array_equal(o[ids], np.stack([x[0] for x in outs]), err_msg=f"{row} t {t}: vs oracle")
        np.testing.assert_array_equal(r[ids], np.array([x[1] for x in outs]), err_msg=f"{row} t {t}: vs oracle")
        assert bool(d.cpu().numpy().all()) == (t == T - 1)
    np.testing.assert_array_equal(sticky_flags(venv), sticky_flags(twin))
    bess = venv.battery_state_of_charge()
    np.testing.assert_array_equal(bess, twin.battery_state_of_charge())
    np.testing.assert_array_equal(bess[ids], np.array([e.bess_soc for e in envs]))
    venv.close()
    twin.close()
