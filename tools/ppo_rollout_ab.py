#!/usr/bin/env python3
"""What finishing a PPO rollout costs, and the same work in torch, in one process, on one box, runs alternating
(modelled on tools/policy_day_ab.py):

  finish       -- PpoHead.finish alone (rollout_gae_kernel: values, advantages, returns, log-probs) on the trajectory
                  of one closed-loop day;
  graph        -- that day's ClosedLoopGraph(trajectory=True) launch alone (reset + T x (actor, step));
  rollout      -- PpoRollout.launch(): the graph and the finishing kernel on one stream;
  torch_eager  -- the same finishing work on the same trajectory in torch: a torch.nn 64-64 tanh critic over the
                  (T + 1) E rows, the GAE loop over T in float32 tensors, Normal(0, std).log_prob(noise).sum(-1);
  torch_graph  -- torch_eager captured with torch.cuda.graph and replayed.

  tools/ppo_rollout_ab.py [--envs 65536] [--chargers 8] [--reps 20] [--warmup 3] [--rounds 3]

Each round times `reps` launches of each form between HIP events after `warmup` launches of its own.  One JSON line
per round with the device time per launch of every form, then one summary line with the build id, the minima, each
form's spread (max - min over the rounds), and the finishing kernel's floors: the bytes it must move, the time
sng_bandwidth_probe's copy kernel takes for as many bytes read and written (the HBM floor), and its fused
multiply-adds at the f32 vector peak, 32 a clock on every SIMD (the FMA floor: v_pk_fma_f32 with the weights as scalar
operand pairs, which is what the chains compile to)."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smart-nanogrid-gym_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--chargers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    from smart_nanogrid_gym import MlpActor, PpoHead, PpoRollout, SmartNanogridVecEnv
    from smart_nanogrid_gym._native import check, lib
    from smart_nanogrid_gym.vec_env import _stream_handle

    E, N = args.envs, args.chargers
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
              battery_system_available_in_model=True)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    venv = SmartNanogridVecEnv(E, seed=args.seed, device=0, rng="device", **kw)
    venv._info.flags = None   # as bench.py without --per-env-flags
    T, O, A = venv.timesteps, venv.obs_dim, venv.act_dim
    gamma, lam = 0.99, 0.95
    from closed_loop_bench import mlp_policy
    net, _ = mlp_policy(venv, args.seed)
    torch.manual_seed(args.seed)
    critic = torch.nn.Sequential(torch.nn.Linear(O, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                                 torch.nn.Linear(64, 1)).to(device)
    log_std = torch.full((A,), -0.5, device=device)
    actor = MlpActor(venv, "tanh").load([net[0].weight, net[0].bias, net[2].weight, net[2].bias, net[4].weight,
                                         net[4].bias])
    head = PpoHead(venv, "tanh").load([critic[0].weight, critic[0].bias, critic[2].weight, critic[2].bias,
                                       critic[4].weight, critic[4].bias], log_std)
    ro = PpoRollout(venv, actor, head, days=1, gamma=gamma, gae_lambda=lam)
    ro.noise.normal_().mul_(log_std.exp())
    ro.launch()
    torch.cuda.synchronize()
    g = ro.graph
    obs, reward, done, noise = g.obs_traj, g.reward_traj, g.done_traj, ro.noise
    # validate_args=False: the sample check reads a flag back on the host, which a stream capture does not permit
    dist = torch.distributions.Normal(torch.zeros(A, device=device), log_std.exp(), validate_args=False)
    out = {}

    @torch.no_grad()
    def torch_finish():
        v = critic(obs.reshape(-1, O)).reshape(T + 1, E)
        r, nn = reward[0].float(), 1.0 - done[0].float()
        gae = torch.zeros(E, device=device)
        adv = torch.empty((T, E), device=device)
        for t in reversed(range(T)):
            delta = r[t] + gamma * v[t + 1] * nn[t] - v[t]
            gae = delta + gamma * lam * nn[t] * gae
            adv[t] = gae
        out["values"], out["adv"], out["ret"] = v, adv, adv + v[:-1]
        out["lp"] = dist.log_prob(noise).sum(-1)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            torch_finish()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    tg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(tg):
        torch_finish()
    tg.replay()
    torch.cuda.synchronize()
    # the two sides agree (tanh and another summation order apart)
    values, adv, _, lp = head.finish(obs, reward, done, noise, gamma, lam)
    agree = {"values": float((values[0] - out["values"]).abs().max()), "advantages": float((adv[0] - out["adv"]).abs().max()),
             "log_prob": float((lp[0] - out["lp"]).abs().max())}
    forms = {"finish": lambda: head.finish(obs, reward, done, noise, gamma, lam), "graph": g.launch,
             "rollout": ro.launch, "torch_eager": torch_finish, "torch_graph": tg.replay}

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
        print(json.dumps({"round": r, "launch_gpu_us": row}), flush=True)
    best = {k: min(r[k] for r in rows) for k in forms}
    spread = {k: round(max(r[k] for r in rows) - min(r[k] for r in rows), 2) for k in forms}
    # the finishing kernel's floors
    read_bytes = (T + 1) * E * O * 4 + T * E * (8 + 1) + T * E * A * 4
    write_bytes = (T + 1) * E * 4 + 3 * T * E * 4
    d_us, b_us = ctypes.c_float(), ctypes.c_float()
    check(lib().sng_bandwidth_probe(0, read_bytes, write_bytes, 20, ctypes.byref(d_us), ctypes.byref(b_us),
                                    _stream_handle(venv.device)))
    props = torch.cuda.get_device_properties(0)
    clock_hz = float(getattr(props, "clock_rate", 2400000)) * 1e3
    fmas = (T + 1) * E * (O * 64 + 64 * 64 + 64)
    fma_floor_us = fmas / (props.multi_processor_count * 4 * 32 * clock_hz) * 1e6
    print(json.dumps({"build_id": lib().sng_build_id().decode(), "envs": E, "chargers": N, "T": T, "obs_dim": O,
                      "act_dim": A, "launch_gpu_us_min": best, "launch_gpu_us_spread": spread,
                      "max_abs_difference_to_torch": agree,
                      "finish_floors": {"read_bytes": read_bytes, "write_bytes": write_bytes,
                                        "hbm_copy_dispatch_us": round(d_us.value, 2), "fmas": fmas,
                                        "compute_units": props.multi_processor_count, "clock_ghz": clock_hz / 1e9,
                                        "fma_floor_us": round(fma_floor_us, 2),
                                        "finish_over_hbm_floor": round(best["finish"] / d_us.value, 2),
                                        "finish_over_fma_floor": round(best["finish"] / fma_floor_us, 2)}}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
