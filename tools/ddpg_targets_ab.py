#!/usr/bin/env python3
"""What the off-policy side of a DDPG iteration costs on the device, and the same work in torch, in one process, on
one box, runs alternating (modelled on tools/ppo_net_rollout_ab.py):

  push                 -- ReplayRing.push of one closed-loop day's trajectory (replay_push_kernel);
  sample               -- ReplayRing.sample(B) (replay_sample_kernel);
  targets              -- QCritic.targets(actor_target, samples): policy_net_kernel over next_obs, then q_net_kernel
                          with the target stage;
  torch_push           -- the same day copied into ring-shaped tensors with four copy_ (the reward converted);
  torch_eager_sample   -- torch.randint and index gathers of the same five outputs from the ring's tensors;
  torch_eager_targets  -- a torch.nn target actor and critic of the same widths on the same rows, the same formula;
  torch_graph_sample, torch_graph_targets -- those two captured with torch.cuda.graph and replayed.

  tools/ddpg_targets_ab.py [--envs 65536] [--chargers 4,10] [--batches 256,65536] [--net 400x300] [--reps 20]
                           [--warmup 3] [--rounds 3]

For every station, each round times `reps` launches of each form between HIP events after `warmup` launches of its
own.  One JSON line per round with the device time per launch of every form, then one summary line with the build id,
the minima, each form's spread (max - min over the rounds) and the floors: for push and sample the time
sng_bandwidth_probe's copy kernel takes for as many bytes read and written; for targets the multiply-adds of
policy_net_kernel and q_net_kernel as they pad them (K to 8, N to a tile, hidden2 to a chunk, rows to 64) at the
f32-input MFMA's rate, 128 multiply-adds a clock a compute unit."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smart-nanogrid-gym_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402


def up(v, to):
    return (v + to - 1) // to * to


def six(net):
    return [net[0].weight, net[0].bias, net[2].weight, net[2].bias, net[4].weight, net[4].bias]


def mlp(inputs, h1, h2, out, device):
    return torch.nn.Sequential(torch.nn.Linear(inputs, h1), torch.nn.ReLU(), torch.nn.Linear(h1, h2), torch.nn.ReLU(),
                               torch.nn.Linear(h2, out)).to(device)


def padded_macs(rows, K, h1, h2, out):
    return up(rows, 64) * (up(K, 8) * up(h1, 32) + up(h1, 8) * up(h2, 64) + up(h2, 8) * up(out, 32))


def one(args, N, arch):
    from smart_nanogrid_gym import ActionNoise, DdpgCollector, MlpActor, QCritic, ReplayRing, SmartNanogridVecEnv
    from smart_nanogrid_gym._native import check, lib
    from smart_nanogrid_gym.vec_env import _stream_handle

    E = args.envs
    h1, h2 = arch
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
              battery_system_available_in_model=True)
    device = torch.device("cuda", 0)
    venv = SmartNanogridVecEnv(E, seed=args.seed, device=0, rng="device", **kw)
    venv._info.flags = None   # as bench.py without --per-env-flags
    T, O, A = venv.timesteps, venv.obs_dim, venv.act_dim
    gamma = 0.99
    torch.manual_seed(args.seed)
    pi, pi_t, qf_t = mlp(O, h1, h2, A, device), mlp(O, h1, h2, A, device), mlp(O + A, h1, h2, 1, device)
    actor = MlpActor(venv, "relu", net_arch=arch, squash=True).load(six(pi))
    actor_t = MlpActor(venv, "relu", net_arch=arch, squash=True).load(six(pi_t))
    critic_t = QCritic(venv, arch).load(six(qf_t))
    noise = ActionNoise(venv, "ou", seed=args.seed, scale=0.5)
    ring = ReplayRing(venv, 2, seed=args.seed)
    col = DdpgCollector(venv, actor, noise, ring, days=1)
    col.launch()
    col.launch()
    torch.cuda.synchronize()
    g = col.graph
    n = len(ring)
    flat_obs = ring.obs.reshape(-1, O)          # [capacity (T + 1) E, O]
    flat_act = ring.actions.reshape(-1, A)
    flat_rew, flat_done = ring.reward.reshape(-1), ring.done.reshape(-1)
    shadow = [torch.empty_like(x) for x in (ring.obs, ring.actions, ring.reward, ring.done)]

    def torch_push():
        shadow[0][0].copy_(g.obs_traj[0])
        shadow[1][0].copy_(g.action_traj[0])
        shadow[2][0].copy_(g.reward_traj[0])   # float64 -> float32
        shadow[3][0].copy_(g.done_traj[0])

    summary = {"build_id": lib().sng_build_id().decode(), "envs": E, "chargers": N, "net_arch": list(arch), "T": T,
               "obs_dim": O, "act_dim": A, "ring_transitions": n, "batches": {}}
    props = torch.cuda.get_device_properties(0)
    clock_hz = float(getattr(props, "clock_rate", 2400000)) * 1e3

    def probe(read, write):
        d_us, b_us = ctypes.c_float(), ctypes.c_float()
        check(lib().sng_bandwidth_probe(0, read, write, 20, ctypes.byref(d_us), ctypes.byref(b_us),
                                        _stream_handle(venv.device)))
        return round(d_us.value, 2)

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

    def capture(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        tg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(tg):
            fn()
        tg.replay()
        torch.cuda.synchronize()
        return tg

    for B in args.batch_list:
        out = {}
        samples = ring.sample(B)

        @torch.no_grad()
        def torch_sample():
            i = torch.randint(n, (B,), device=device)
            row = i + (i // (T * E)) * E
            out["obs"], out["next_obs"] = flat_obs[row], flat_obs[row + E]
            out["actions"], out["rewards"] = flat_act[i], flat_rew[i].unsqueeze(1)
            out["dones"] = flat_done[i].float().unsqueeze(1)

        @torch.no_grad()
        def torch_targets():
            nobs = samples.next_observations
            a = torch.tanh(pi_t(nobs))
            q = qf_t(torch.cat([nobs, a], dim=1))
            out["y"] = samples.rewards + (1.0 - samples.dones) * gamma * q

        tg_sample, tg_targets = capture(torch_sample), capture(torch_targets)
        y, _ = critic_t.targets(actor_t, samples, gamma)
        torch.cuda.synchronize()
        agree = float((y - out["y"]).abs().max())   # tanhf and another summation order apart
        forms = {"push": lambda: ring.push(g), "sample": lambda: ring.sample(B),
                 "targets": lambda: critic_t.targets(actor_t, samples, gamma), "torch_push": torch_push,
                 "torch_eager_sample": torch_sample, "torch_eager_targets": torch_targets,
                 "torch_graph_sample": tg_sample.replay, "torch_graph_targets": tg_targets.replay}
        rows = []
        for r in range(args.rounds):
            row = {k: round(timed(v), 2) for k, v in forms.items()}
            rows.append(row)
            print(json.dumps({"chargers": N, "batch": B, "round": r, "launch_gpu_us": row}), flush=True)
        best = {k: min(r[k] for r in rows) for k in forms}
        spread = {k: round(max(r[k] for r in rows) - min(r[k] for r in rows), 2) for k in forms}
        step = T * E
        push_read = (T + 1) * E * O * 4 + step * A * 4 + step * 8 + step
        push_write = (T + 1) * E * O * 4 + step * A * 4 + step * 4 + step
        sample_read = B * ((2 * O + A) * 4 + 4 + 1)
        sample_write = B * ((2 * O + A) * 4 + 4 + 4 + 8)
        actor_macs, q_macs = padded_macs(B, O, h1, h2, A), padded_macs(B, O + A, h1, h2, 1)
        rate = props.multi_processor_count * 128 * clock_hz
        floors = {"push_read_bytes": push_read, "push_write_bytes": push_write,
                  "push_hbm_copy_dispatch_us": probe(push_read, push_write),
                  "sample_read_bytes": sample_read, "sample_write_bytes": sample_write,
                  "sample_hbm_copy_dispatch_us": probe(sample_read, sample_write),
                  "actor_padded_macs": actor_macs, "q_padded_macs": q_macs,
                  "real_macs": B * (O * h1 + h1 * h2 + h2 * A + (O + A) * h1 + h1 * h2 + h2),
                  "compute_units": props.multi_processor_count, "clock_ghz": clock_hz / 1e9,
                  "actor_mfma_floor_us": round(actor_macs / rate * 1e6, 2),
                  "q_mfma_floor_us": round(q_macs / rate * 1e6, 2)}
        summary["batches"][str(B)] = {"launch_gpu_us_min": best, "launch_gpu_us_spread": spread,
                                      "max_abs_difference_of_y_to_torch": agree, "floors": floors}
    print(json.dumps(summary), flush=True)
    for x in (col, critic_t, actor_t, actor, noise, ring, venv):
        x.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--chargers", default="4,10")
    ap.add_argument("--batches", default="256,65536")
    ap.add_argument("--net", default="400x300")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    args.batch_list = [int(b) for b in args.batches.split(",")]
    arch = tuple(int(h) for h in args.net.split("x"))
    torch.cuda.set_device(0)
    for N in (int(x) for x in args.chargers.split(",")):
        one(args, N, arch)
    return 0


if __name__ == "__main__":
    sys.exit(main())
