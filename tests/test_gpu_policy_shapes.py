"""GPU: the shapes of the policy kernels that the policy matrix's E = 70 cannot reach.

  1. Every instantiation of the fused day, day_lean_policy_kernel<NC, PK, REQ>: NC in {1, 2, 4, 8, 16, and 10 with
     V2X} x packed / unpacked records x the requested-SoC stream -- 24 triples, 23 compiled (<1, true, true> keeps
     its 2 T nodes: csrc/sng_step_plan.h day_lean_compiled) -- with a trajectory at E = 72 and E = 200.  obs_dim =
     2 N + 9 is odd, so only with E a multiple of 4 are every step's observation, noise and action blocks 16 B
     multiples: there launch_policy_day keeps vec_io and vec_act, the path every production population takes and
     E = 70 never does.  E = 200 is three full 64-row blocks and a tail of 8: blockIdx.x up to 3.  The fused form
     must equal the node form bitwise, and the node form's stored actions its host model; the policy matrix pins the
     node form's env side to the oracle.
  2. rollout_gae_kernel's row blocks: a single partial block (E = 1, 4, 63), no partial block (E = 64, where the
     zero-fill loops do nothing), and four blocks (E = 200), against the host model bitwise.
  3. policy_kernel and policy_net_kernel (33-65) at E = 64, 72 and 200: full blocks only, an aligned tail block
     (the vector copy of a tail: rows * obs_dim % 4 == 0 needs E % 4 == 0), and blocks past the second.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from policy_cases import random_weights  # noqa: E402
from policy_net_cases import random_net_weights  # noqa: E402
from smart_nanogrid_gym import MlpActor, PpoHead, SmartNanogridVecEnv  # noqa: E402
from station_matrix_cases import square_mode  # noqa: E402
from test_gpu_policy import OUT_SCALE, SEED, T, assert_env_side_equal, closed_loop_day, make_noise, station  # noqa: E402
from test_gpu_ppo_rollout import DAYS, VALUE_SCALE, host, make_env, on, synthetic  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _square_mode():
    square_mode(True)   # x*x squares, as on the GPU
    yield
    square_mode(False)


# ------------------------------------------------------------------------------ 1. every fused instantiation
TRIPLES = [(nc, pk, req) for nc in (1, 2, 4, 8, 10, 16) for pk in (True, False) for req in (False, True)]
NOT_COMPILED = (1, True, True)


def test_the_sweep_lists_every_triple():
    assert len(TRIPLES) == len(set(TRIPLES)) == 24 and TRIPLES.count(NOT_COMPILED) == 1


@pytest.mark.parametrize("nc,pk,req", TRIPLES, ids=[f"n{n}-{'pk' if p else 'unpacked'}-{'req' if r else 'noreq'}"
                                                     for n, p, r in TRIPLES])
def test_fused_day_instantiation_equals_the_node_form(nc, pk, req):
    kw = station(nc, vehicle_to_everything=(nc == 10), enable_requested_state_of_charge=req)
    rng = "device" if pk else "reference"   # device days are packed records, reference days unpacked
    b = lambda x: "true" if x else "false"   # noqa: E731
    for E in (72, 200):
        what = f"<{nc}, {b(pk)}, {b(req)}> E = {E}"
        nodes = closed_loop_day(kw, rng, E)
        assert nodes["kernel"] == f"void sng::step_lean_kernel<{nc}, {b(pk)}, {b(req)}>", (what, nodes["kernel"])
        # every step's block is a 16 B multiple: the fused day keeps vec_io and vec_act
        assert (E * nodes["obs_dim"]) % 4 == 0 and (E * nodes["act_dim"]) % 4 == 0
        assert nodes["nodes"] == 2 * T
        for t in range(T):
            np.testing.assert_array_equal(nodes["act"][t], nodes["host"][t][0], err_msg=f"{what} t {t}: node form's a")
        inside = ((nodes["act"] > nodes["low"]) & (nodes["act"] < nodes["high"])).mean()
        assert 0.1 < inside < 0.9, (what, inside)
        assert (nodes["rew"] != 0).any() and nodes["done"][-1].all() and not nodes["done"][:-1].any()
        fused = closed_loop_day(kw, rng, E, fused=True)
        assert fused["nodes"] == (2 * T if (nc, pk, req) == NOT_COMPILED else 1), (what, fused["nodes"])
        np.testing.assert_array_equal(fused["act"], nodes["act"], err_msg=f"{what}: fused actions")
        assert_env_side_equal(fused, nodes, f"{what}: fused=True")


# ------------------------------------------------------------------------- 2. rollout_gae_kernel's row blocks
def synthetic_rows(v, seed):
    """test_gpu_ppo_rollout.synthetic at any E: its observations, rewards and noise; terminal flags that need no
    minimum population (both values mid-day and at a day's last step are forced on env 0)."""
    rng = np.random.default_rng(seed)
    T_, E = v.timesteps, v.num_envs
    recorded = [v.reset_tensors().cpu().numpy()]
    for _ in range(3):
        a = rng.uniform(v.action_space.low, v.action_space.high, (E, v.act_dim)).astype(np.float32)
        recorded.append(v.step_tensors(torch.from_numpy(a).to(v.device))[0].cpu().numpy())
    obs = np.stack([np.stack([recorded[(d + t) % 4] + np.float32(0.003 * (d * (T_ + 1) + t)) for t in range(T_ + 1)])
                    for d in range(DAYS)]).astype(np.float32)
    reward = -40.0 * rng.random((DAYS, T_, E))
    log_std = rng.uniform(-2.0, 0.5, v.act_dim).astype(np.float32)
    noise = (rng.normal(0, 1, (T_, E, v.act_dim)) * np.exp(log_std)).astype(np.float32)
    done = (rng.random((DAYS, T_, E)) < 0.2).astype(np.uint8)
    done[0, T_ // 2, 0], done[0, T_ // 2 + 1, 0] = 1, 0
    done[0, -1, 0], done[1, -1, 0] = 0, 1
    return obs, reward, done, noise, log_std


@pytest.mark.parametrize("E", [1, 4, 63, 64, 200])
def test_finish_row_blocks_equal_the_host_model(E):
    v = make_env(8, "2h", E)
    assert v.timesteps == 12
    if E >= 63:
        obs, reward, done, noise, log_std = synthetic(v, 8)
    else:
        obs, reward, done, noise, log_std = synthetic_rows(v, 8)
    assert obs.shape == (DAYS, 13, E, 25) and done.any() and not done.all()
    head = PpoHead(v, "relu").load(random_weights(v.obs_dim, 1, 17, VALUE_SCALE), log_std)
    obs_d, reward_d, done_d, noise_d = on(v, obs, reward, done, noise)
    for nz_d, nz in ((noise_d, noise), (None, None)):
        got = [host(x) for x in head.finish(obs_d, reward_d, done_d, nz_d, 0.98, 0.9)]
        torch.cuda.synchronize()
        want = head.host_finish(obs, reward, done, nz, 0.98, 0.9)
        for name, a, w in zip(("values", "advantages", "returns", "log_prob"), got, want):
            if nz is None and name == "log_prob":
                assert a is None and w is None
                continue
            assert a.shape == w.shape and a.dtype == w.dtype == np.float32
            np.testing.assert_array_equal(a, w, err_msg=f"E = {E} noise = {nz is not None}: {name}")
    assert np.unique(got[0]).size > got[0].size // 2, "degenerate values"
    head.close()
    v.close()


# ------------------------------------------------------------------ 3. policy_kernel and policy_net_kernel's blocks
@pytest.mark.parametrize("E", [64, 72, 200])
@pytest.mark.parametrize("N", [4, 10])
@pytest.mark.parametrize("net", [None, (33, 65)], ids=["policy_kernel", "policy_net_kernel-33x65"])
def test_actor_kernels_row_blocks_equal_the_host_model(net, N, E):
    v = SmartNanogridVecEnv(E, seed=SEED, rng="device", **station(N))
    rng = np.random.default_rng(5)
    recorded = [v.reset_tensors().clone()]
    for _ in range(3):   # observations of a day under way
        a = torch.from_numpy(rng.uniform(v.action_space.low, v.action_space.high, (E, v.act_dim)).astype(np.float32))
        recorded.append(v.step_tensors(a.to(v.device))[0].clone())
    noise = torch.from_numpy(make_noise(E, v.act_dim, 3)[0]).to(v.device)
    if net is None:
        actor = MlpActor(v, "relu").load(random_weights(v.obs_dim, v.act_dim, 11, OUT_SCALE))
    else:
        actor = MlpActor(v, "relu", net_arch=net).load(random_net_weights(v.obs_dim, v.act_dim, net, 11, OUT_SCALE))
    assert actor.net == (net is not None)
    clipped = checked = 0
    for obs in (recorded[0], recorded[-1]):
        a, env_a = (x.cpu().numpy() for x in actor.actions(obs, noise))
        want_a, want_env = actor.host_actions(obs, noise)
        np.testing.assert_array_equal(a, want_a, err_msg=f"N = {N} E = {E} {net}: a")
        np.testing.assert_array_equal(env_a, want_env, err_msg=f"N = {N} E = {E} {net}: env actions")
        np.testing.assert_array_equal(env_a, np.minimum(np.maximum(a, v.action_space.low), v.action_space.high))
        clipped += int((env_a != a).sum())
        checked += a.size
    assert 0 < clipped < checked   # the clip acts, and not everywhere
    actor.close()
    v.close()
