"""GPU: the nodes and edges a capture makes (include/sng.h: sng_graph_describe; csrc/sng_graph.cpp: capture_days),
pinned form by form to tests/golden/graph_listings.json.

The other GPU tests compare what graphs compute, and a wrong or missing edge between a generator and the day that
reads its slot can pass such a comparison.  Here every form of captured day is captured at 192 envs, described and
destroyed; nothing is launched.  A listing holds one line per node in hipGraphGetNodes order: the node's type, a kernel
node's name, grid, block and dynamic LDS, and the indices of the nodes it depends on.

The golden file was recorded from the commit before capture_days was split into parts, with sng_graph_describe alone
added to it (`python tests/test_gpu_graph_describe.py OUT.json` writes the listings of the build it runs on, after it
has captured every form twice and found both listings equal).
"""
import json
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "graph_listings.json")
E, T = 192, 24
BASE = dict(time_interval="1h", charging_mode="bounded", vehicle_uncharged_penalty_mode="sparse",
            pv_system_available_in_model=True, battery_system_available_in_model=True)


def _episode(n, rng="device", info=False, station=None, **graph_kw):
    def capture():
        from smart_nanogrid_gym import SmartNanogridVecEnv
        from smart_nanogrid_gym.vec_env import EpisodeGraph
        v = SmartNanogridVecEnv(E, seed=7, rng=rng, info=info, **dict(BASE, number_of_chargers=n, **(station or {})))
        if not graph_kw.get("with_reset", True):
            v.reset_tensors()
        actions = torch.zeros((T, E, v.act_dim), dtype=torch.float32, device=v.device)
        g = EpisodeGraph(v, actions, **graph_kw)
        return g, g.step_nodes_per_day, (g, v)
    return capture


def _closed_loop(n, net_arch=(64, 64), net=False, noise=False, **graph_kw):
    def capture():
        from smart_nanogrid_gym import ActionNoise, ClosedLoopGraph, MlpActor, SmartNanogridVecEnv
        v = SmartNanogridVecEnv(E, seed=7, rng="device", **dict(BASE, number_of_chargers=n))
        actor = MlpActor(v, "relu", net_arch=net_arch, net=net)
        source = ActionNoise(v, "gaussian", seed=3) if noise else None
        g = ClosedLoopGraph(v, actor, noise=source, **graph_kw)
        return g, g.step_nodes, (g, source, actor, v)
    return capture


# name -> (capture, days, nodes of a day's reset, nodes ahead of the first day)
FORMS = {
    # the default station: 10 chargers, device RNG
    "n10_steps_only": (_episode(10, with_reset=False), 1, 0, 0),
    "n10_reset_3days": (_episode(10, days=3), 3, 1, 0),
    "n10_reset_3days_serial": (_episode(10, days=3, serial_reset=True), 3, 1, 0),
    "n10_reset_2days_step_nodes": (_episode(10, days=2, step_nodes=True), 2, 1, 0),
    "n10_reset_3days_generic_day": (_episode(10, days=3, generic_day=True), 3, 1, 0),
    "n10_reset_3days_trajectory": (_episode(10, days=3, trajectory=True), 3, 1, 0),
    # 8 chargers: the lean family
    "n8_reset_2days": (_episode(8, days=2), 2, 1, 0),
    "n8_reset_3days_forced_overlap": (_episode(8, days=3, overlapped_reset=True), 3, 1, 0),
    "n8_reset_2days_trajectory": (_episode(8, days=2, trajectory=True), 2, 1, 0),
    "n8_reference_rng_steps_only": (_episode(8, rng="reference", with_reset=False), 1, 0, 0),
    # other stations
    "n4_actor_nodes_2days_trajectory": (_closed_loop(4, days=2, trajectory=True), 2, 1, 0),
    "n4_actor_forced_fused": (_closed_loop(4, fused=True), 1, 1, 0),
    "n4_net_actor_400_300": (_closed_loop(4, net_arch=(400, 300), net=True), 1, 1, 0),
    "n8_actor_gaussian_source_2days": (_closed_loop(8, noise=True, days=2), 2, 1, 2),   # the fill and its counter's bump
    # profile_kernel and observe0_kernel behind the generator: the observation tile is past the one-launch reset's 32 KB
    "n60_reset_1day_three_launches": (_episode(60, days=1, station=dict(pv_noise=0.2, price_noise=0.1)), 1, 3, 0),
    "n10_info_step_nodes": (_episode(10, info=True, days=1), 1, 1, 0),
}


def listing(name):
    """(lines, step nodes a day as the library reports them) of one fresh capture of the form."""
    g, step_nodes, owned = FORMS[name][0]()
    try:
        return g.describe().splitlines(), step_nodes
    finally:
        for x in owned:
            if x is not None:
                x.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_form_has_a_golden_listing(golden):
    assert sorted(golden) == sorted(FORMS)


@pytest.mark.parametrize("name", sorted(FORMS))
def test_captured_graph_is_the_recorded_one(golden, name):
    lines, step_nodes = listing(name)
    _, days, reset_nodes, ahead = FORMS[name]
    assert lines == golden[name], "\n".join(lines)
    # an overlapped graph's generators' stream ends in the node that advances the day counter
    overlapped_bump = 1 if any("bump_day_kernel" in x for x in lines) else 0
    assert len(lines) == ahead + days * (step_nodes + reset_nodes) + overlapped_bump, (len(lines), step_nodes)
    assert [int(x.split()[0]) for x in lines] == list(range(len(lines)))
    assert all(x.split()[1] == "kernel" and "?" not in x for x in lines), "every node is a named kernel"


if __name__ == "__main__":   # record the listings of the build this runs on
    sys.path[:0] = [ROOT, os.path.join(ROOT, "smart-nanogrid-gym_amd"), os.path.join(ROOT, "oracle")]
    out = {}
    for form in sorted(FORMS):
        first, second = listing(form)[0], listing(form)[0]
        assert first == second, f"{form}: two captures in one process differ"
        out[form] = first
        print(form, len(first), "nodes", flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
