"""GPU: day_station_kernel (csrc/sng_step_day.h), the day kernel of the default station with the station's switches
fixed at compile time, against the same graph captured with the generic day_wide_kernel (generic_day=True,
SNG_GRAPH_GENERIC_DAY) and as T step nodes (step_nodes=True), and against the CPU oracle.

Three handles of one seed replay their graphs side by side; after every replay everything a caller can read is
equal bit for bit: the last step's observations, reward and done, the day returns, the flag summary, every charger's
SoC, the BESS SoC, the day counter, the sticky flags and the whole checkpoint.  Every case asks the graph which kernel
its days run (EpisodeGraph.day_kernel_name, sng_graph_day_kernel_name), so a selection that silently fell back to the
generic kernel fails here.

The three SngInfo pointers the kernel keeps at run time are each given and not given (INFO below).  A handle made
without info=True passes the flag summary and the day return but no per-env flag array (info=True also passes the
diagnostic arrays, which are the general kernel's), so "flags" sets SngInfo.flags as bench.py --per-env-flags does
and compares the array (the last step's flags of every env) among the forms, and "nulls" clears the other two.

Shapes: 32 envs are one full wavefront; 33 and 70 leave a last wavefront of 1 and 6 envs (the one-float tail of the
tiles' copies, idle lanes).  One day, and three days whose resets run beside the steps in both day slots.  The graph
API steps whole days (launch_day's t0 and nt are 0 and T in every capture), so a day that starts at t0 > 0 has no
caller to test through; the steps-only graph below is the form without a reset.
"""
import numpy as np
import pytest

import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import wide_rebuild_cases as R  # noqa: E402
from smart_nanogrid_gym import SmartNanogridVecEnv  # noqa: E402
from smart_nanogrid_gym.vec_env import EpisodeGraph  # noqa: E402
from station_matrix_cases import square_mode  # noqa: E402
from test_gpu_bench_kernel import actions as bench_actions, load_day  # noqa: E402
from test_gpu_day_kernel import KW10, flags_of  # noqa: E402
from test_gpu_day_kernel_chain import assert_same_handles, nonneg_actions, same  # noqa: E402

STATION = "void sng::day_station_kernel<10, 2>"
GENERIC = "void sng::day_wide_kernel<10, 2, false, false>"
FORMS = {"station": ({}, STATION), "generic": (dict(generic_day=True), GENERIC), "nodes": (dict(step_nodes=True), "")}


INFO = ("default", "flags", "nulls")   # SngInfo: the handle's own; with the per-env flag array; without any pointer


def three_forms(E, acts, days=1, with_reset=True, kw=KW10, seed=77, info="default", day_returns=False, replays=2,
                names=None):
    """The default graph, the generic day kernel's and the step nodes', on handles of one seed; returns the sticky
    flags and, with info="flags", the per-env flag array after the last replay.  day_returns: every graph adds day d's
    returns into row d of a [days, E] tensor of its own.  names: the kernel each form must report, where it is not
    FORMS' (a station the predicate refuses)."""
    assert info in INFO
    acts_d = torch.from_numpy(np.ascontiguousarray(acts)).to("cuda:0")
    handles, graphs, rows = {}, {}, {}
    for form, (gkw, name) in FORMS.items():
        v = handles[form] = SmartNanogridVecEnv(E, seed=seed, rng="device", **kw)
        assert not v._info.flags and v._info.flag_summary and v._info.episode_return
        if info == "flags":
            v._info.flags = v.flags_d.data_ptr()   # as bench.py --per-env-flags
            v.flags_d.fill_(-1)   # no flag word is all ones: every env's must be written
        elif info == "nulls":
            v._info.flag_summary = v._info.episode_return = None
        if not with_reset:
            v.reset_tensors()
        if day_returns:
            rows[form] = torch.zeros((days, E), dtype=torch.float64, device="cuda:0")
        g = graphs[form] = EpisodeGraph(v, acts_d, with_reset=with_reset, days=days, day_returns=rows.get(form), **gkw)
        # the per-env flag array is not a diagnostic: the handle keeps the wide plan and the station its kernel
        assert g.day_kernel_name == (names or {}).get(form, name), (form, info, g.day_kernel_name)
        assert g.step_nodes_per_day == (v.timesteps if form == "nodes" else 1)
    for rep in range(replays if with_reset else 1):
        for g in graphs.values():
            g.launch()
        for other in ("generic", "nodes"):
            what = f"replay {rep}, info {info}: station-fixed day kernel vs {other}"
            assert_same_handles(handles["station"], handles[other], what)
            same(handles["station"].flags_d, handles[other].flags_d, what + ": per-env flags")
            if day_returns:
                same(rows["station"], rows[other], what + ": day returns by row")
    v = handles["station"]
    if day_returns:
        assert bool((rows["station"] != 0).any(dim=1).all()) and not bool(v.return_d.any())
    else:
        assert bool((v.return_d != 0).any()) == (info != "nulls")
    if info == "flags":
        assert not bool((v.flags_d == -1).any())
    else:
        assert not bool(v.flags_d.any())   # not given: not written
    if info == "nulls":
        assert not bool(v.flag_summary_d.any())
    fl = flags_of(v), v.flags_d.cpu().numpy().view(np.uint32)
    for x in list(graphs.values()) + list(handles.values()):
        x.close()
    return fl


@pytest.mark.parametrize("days", [1, 3])
@pytest.mark.parametrize("E", [32, 33, 70])
def test_reset_graphs(E, days):
    three_forms(E, nonneg_actions(24, E, seed=10 * E + days), days=days)


WILD_ENVS = (5, 40, 66)   # one in each of the three wavefronts of 70 envs


def wild_actions(E=70):
    """Env 5 (first wavefront) negative at even steps and at the last one, env 40 (second) NaN at step 3: those
    wavefronts take the general order there.  Env 66 (third) far above the Box, one action whose float32 product
    overflows: the fast loop's infinite-product path."""
    a = nonneg_actions(24, E, seed=3)
    a[::2, 5, 2] = -0.75
    a[23, 5, 6] = -0.5
    a[3, 40, 7] = np.nan
    a[:, 66, 1] = 2.5
    a[5, 66, 8] = 1e38
    return a


@pytest.mark.parametrize("days", [1, 3])
def test_per_env_flag_array_given(days):
    """SngInfo.flags given: the kernel's per-env flag store runs every step; the array holds the last step's flags of
    every env, raised ones among them, and is the same from all three forms.  Every odd env asks all ten chargers to
    discharge at steps 12 and 23: without V2X a negative demand is flagged wherever a vehicle is there to answer."""
    a = wild_actions()
    a[12, 1::2, :10] = -1.0
    a[23, 1::2, :10] = -1.0
    sticky, last = three_forms(70, a, days=days, info="flags")
    print("sticky", sticky.tolist(), "last step", last.tolist())
    assert sticky[1::2].any() and last[1::2].any(), (sticky, last)
    assert not (last & ~sticky).any(), (sticky, last)   # the sticky word holds every step's
    assert not last[[0, 38, 68]].any() and not sticky[[0, 38, 68]].any(), (sticky, last)


def test_flag_summary_and_day_return_not_given():
    """SngInfo.flag_summary and episode_return null: no summary word, no return; the sticky flags are still raised."""
    sticky, _ = three_forms(70, wild_actions(), days=3, info="nulls")
    assert sticky[5] and not sticky[[0, 39, 69]].any(), sticky


@pytest.mark.parametrize("info", ["default", "nulls"])
def test_day_returns_by_row(info):
    """day_returns given: day d's returns go to row d (in an overlapped graph through the second day slot's shadow
    return where the handle has one), with and without the handle's own return pointer."""
    three_forms(33, nonneg_actions(24, 33, seed=5), days=3, info=info, day_returns=True)


def test_steps_only_graph():
    three_forms(33, nonneg_actions(24, 33, seed=2), with_reset=False)


def test_negative_nan_and_out_of_box_actions():
    """wild_actions with the handle's own SngInfo (no per-env flag array)."""
    fl, _ = three_forms(70, wild_actions(), days=1)
    assert fl[5] and not fl[[0, 39, 69]].any(), fl


def test_rebuilt_positive_sums():
    """wide_rebuild_cases: eight or more positive powers whose running sum is not provably numpy's (pos_slow)."""
    kw, rng, _, day_kernel = R.STATIONS["n10_device"]
    assert rng == "device" and day_kernel and kw == KW10
    three_forms(R.E, R.rebuild_actions(10, 24), days=1, seed=R.SEED)


def test_another_day_length_keeps_the_generic_kernel():
    """The 2 h station is not the kernel's (T = 12): the default graph captures the generic kernel, and its results
    are the step nodes'."""
    kw = dict(KW10, time_interval="2h")
    three_forms(33, nonneg_actions(12, 33, seed=4), days=2, kw=kw, names={"station": GENERIC})


def test_station_kernel_vs_oracle():
    """Independent of the step kernels: a generated device day exported to the CPU oracle and stepped there."""
    square_mode(True)   # x*x squares, as on the GPU
    try:
        E, T, A = 70, 24, 11
        v = SmartNanogridVecEnv(E, seed=2026, rng="device", **KW10)
        v.reset_tensors()
        ivs, ratios = v.get_scenarios(0, E)
        envs = [O.OracleEnv(O.OracleConfig(**KW10), 0) for _ in range(E)]
        for e, iv, r in zip(envs, ivs, ratios):
            load_day(e, iv, r)
        rng = np.random.default_rng(E)
        acts = np.stack([bench_actions(rng, E, A, (np.arange(E) % 4) == 0) for _ in range(T)])
        g = EpisodeGraph(v, torch.from_numpy(acts).to(v.device), with_reset=False)
        assert g.day_kernel_name == STATION
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
    finally:
        square_mode(False)
