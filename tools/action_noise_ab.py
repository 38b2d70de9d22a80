#!/usr/bin/env python3
"""What the action noise costs when the library draws it (ActionNoise, action_noise_kernel) and when torch does, in
one process, on one box, runs alternating (modelled on tools/ppo_net_rollout_ab.py):

  fill_gaussian / fill_ou     -- ActionNoise.fill(1) of each kind: the fill kernel and the counter's bump;
  torch_gaussian_eager        -- the statement it replaces: scratch.normal_(), the scale by std [A], the copy into the
                                 [T, E, A] block (INTEGRATION.md section 3's PPO line);
  torch_ou_eager              -- the T-step Ornstein-Uhlenbeck loop of INTEGRATION.md section 3;
  torch_*_graph               -- each captured with torch.cuda.graph and replayed;
  rollout_source              -- PpoRollout(noise=source).launch(): fill, graph, finish;
  rollout_torch               -- the torch fill above, then PpoRollout.launch() with the caller's block, on the same build;
  rollout_alone               -- that launch without any fill (a stale block).

  tools/action_noise_ab.py [--envs 65536] [--chargers 8,10] [--reps 20] [--warmup 3] [--rounds 3]

For every station each round times `reps` launches of each form between HIP events after `warmup` launches of its own.
One JSON line per round, then a summary line with the build id, the minima, each form's spread and the floor: the time
sng_bandwidth_probe's copy kernel takes to store the block's bytes (nothing read), one dispatch and back to back, and
the fill kernels' ratio to it."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smart-nanogrid-gym_amd"))

import torch  # noqa: E402


def six(net):
    return [net[0].weight, net[0].bias, net[2].weight, net[2].bias, net[4].weight, net[4].bias]


def mlp(O, out, device):
    return torch.nn.Sequential(torch.nn.Linear(O, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                               torch.nn.Linear(64, out)).to(device)


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def one(args, N):
    from smart_nanogrid_gym import ActionNoise, MlpActor, PpoHead, PpoRollout, SmartNanogridVecEnv
    from smart_nanogrid_gym._native import check, lib
    from smart_nanogrid_gym.vec_env import _stream_handle

    E = args.envs
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
              battery_system_available_in_model=True)
    device = torch.device("cuda", 0)
    venv = SmartNanogridVecEnv(E, seed=args.seed, device=0, rng="device", **kw)
    venv._info.flags = None   # as bench.py without --per-env-flags
    T, O, A = venv.timesteps, venv.obs_dim, venv.act_dim
    torch.manual_seed(args.seed)
    pi, critic = mlp(O, A, device), mlp(O, 1, device)
    log_std = torch.full((A,), -0.5, device=device)
    std = log_std.exp()
    gauss = ActionNoise(venv, "gaussian", seed=1, scale=std)
    ou = ActionNoise(venv, "ou", seed=2, scale=0.5)
    # the rollouts: the library's source, and the caller's block
    actor, head = MlpActor(venv, "tanh").load(six(pi)), PpoHead(venv, "tanh").load(six(critic), log_std)
    ro_src = PpoRollout(venv, actor, head, days=1, noise=ActionNoise(venv, "gaussian", seed=3, scale=std))
    ro_old = PpoRollout(venv, actor, head, days=1)
    block, scratch = ro_old.noise, torch.empty((T, E, A), device=device)

    def torch_gaussian():
        scratch.normal_()
        block.copy_(scratch * std)

    theta, dt, sigma = 0.15, 1e-2, 0.5
    path = torch.empty((T, E, A), device=device)

    def torch_ou():
        prev = torch.zeros((E, A), device=device)
        for t in range(T):
            prev = prev * (1 - theta * dt) + sigma * dt ** 0.5 * torch.randn((E, A), device=device)
            path[t] = prev

    def rollout_torch():
        torch_gaussian()
        ro_old.launch()

    tg, to = captured(torch_gaussian), captured(torch_ou)
    forms = {"fill_gaussian": lambda: gauss.fill(1), "fill_ou": lambda: ou.fill(1),
             "torch_gaussian_eager": torch_gaussian, "torch_gaussian_graph": tg.replay,
             "torch_ou_eager": torch_ou, "torch_ou_graph": to.replay,
             "rollout_source": ro_src.launch, "rollout_torch": rollout_torch, "rollout_alone": ro_old.launch}

    def timed(run):
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    rows = []
    for r in range(args.rounds):
        row = {k: round(timed(v), 2) for k, v in forms.items()}
        rows.append(row)
        print(json.dumps({"chargers": N, "round": r, "launch_gpu_us": row}), flush=True)
    best = {k: min(r[k] for r in rows) for k in forms}
    spread = {k: round(max(r[k] for r in rows) - min(r[k] for r in rows), 2) for k in forms}
    nbytes = T * E * A * 4
    d_us, b_us = ctypes.c_float(), ctypes.c_float()
    check(lib().sng_bandwidth_probe(0, 0, nbytes, 20, ctypes.byref(d_us), ctypes.byref(b_us), _stream_handle(venv.device)))
    # the sample's moments, as a sanity check of what was timed
    z = gauss.fill(1) / std
    print(json.dumps({"build_id": lib().sng_build_id().decode(), "envs": E, "chargers": N, "T": T, "act_dim": A,
                      "block_bytes": nbytes, "launch_gpu_us_min": best, "launch_gpu_us_spread": spread,
                      "gaussian_sample": {"mean": float(z.mean()), "std": float(z.std())},
                      "floor": {"store_dispatch_us": round(d_us.value, 2), "store_back_to_back_us": round(b_us.value, 2),
                                "fill_gaussian_over_store": round(best["fill_gaussian"] / b_us.value, 2),
                                "fill_ou_over_store": round(best["fill_ou"] / b_us.value, 2)}}), flush=True)
    for x in (ro_src, ro_old):
        x.close()
    venv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--chargers", default="8,10")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    for N in (int(x) for x in args.chargers.split(",")):
        one(args, N)
    return 0


if __name__ == "__main__":
    sys.exit(main())
