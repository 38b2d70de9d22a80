#!/usr/bin/env python3
"""What finishing a PPO rollout costs with a value net of its own widths, and the same work in torch, in one process,
on one box, runs alternating (modelled on tools/ppo_rollout_ab.py):

  finish       -- PpoHead(net_arch=...).finish alone (value_net_kernel over the (T + 1) E rows, then gae_scan_kernel:
                  values, advantages, returns, log-probs) on the trajectory of one closed-loop day;
  finish_nolp  -- the same without noise: no log-probability stage;
  graph        -- that day's ClosedLoopGraph(trajectory=True) launch alone (reset + T x (actor, step)), the actor of
                  the same widths;
  rollout      -- PpoRollout.launch(): the graph and the two finishing kernels on one stream;
  torch_eager  -- the same finishing work on the same trajectory in torch: a torch.nn tanh critic of the same widths
                  over the (T + 1) E rows, the GAE loop over T in float32 tensors, Normal(0, std).log_prob(noise).sum(-1);
  torch_graph  -- torch_eager captured with torch.cuda.graph and replayed.

  tools/ppo_net_rollout_ab.py [--envs 65536] [--chargers 8,10] [--nets 256x256,400x300] [--reps 20] [--warmup 3]
                              [--rounds 3]

For every station and net, each round times `reps` launches of each form between HIP events after `warmup` launches
of its own.  One JSON line per round with the device time per launch of every form, then one summary line with the
build id, the minima, each form's spread (max - min over the rounds) and the floors: value_net_kernel's multiply-adds
as it pads them (K to 8, N to a tile, hidden2 to a chunk, one output tile) at the f32-input MFMA's rate, 128
multiply-adds a clock a compute unit, which is the f32 vector peak; and gae_scan_kernel's bytes (reward, done, V and
the noise read; advantages, returns and log-probs written) as the time sng_bandwidth_probe's copy kernel takes for as
many bytes read and written."""
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


def mlp(O, h1, h2, out, device):
    return torch.nn.Sequential(torch.nn.Linear(O, h1), torch.nn.Tanh(), torch.nn.Linear(h1, h2), torch.nn.Tanh(),
                               torch.nn.Linear(h2, out)).to(device)


def one(args, N, arch):
    from smart_nanogrid_gym import MlpActor, PpoHead, PpoRollout, SmartNanogridVecEnv
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
    gamma, lam = 0.99, 0.95
    torch.manual_seed(args.seed)
    pi, critic = mlp(O, h1, h2, A, device), mlp(O, h1, h2, 1, device)
    log_std = torch.full((A,), -0.5, device=device)
    actor = MlpActor(venv, "tanh", net_arch=arch).load(six(pi))
    head = PpoHead(venv, "tanh", net_arch=arch).load(six(critic), log_std)
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
    forms = {"finish": lambda: head.finish(obs, reward, done, noise, gamma, lam),
             "finish_nolp": lambda: head.finish(obs, reward, done, None, gamma, lam), "graph": g.launch,
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
        print(json.dumps({"chargers": N, "net_arch": list(arch), "round": r, "launch_gpu_us": row}), flush=True)
    best = {k: min(r[k] for r in rows) for k in forms}
    spread = {k: round(max(r[k] for r in rows) - min(r[k] for r in rows), 2) for k in forms}
    # the floors
    n_rows = (T + 1) * E
    macs = up(n_rows, 64) * (up(O, 8) * up(h1, 32) + up(h1, 8) * up(h2, 64) + up(h2, 8) * 32)
    real_macs = n_rows * (O * h1 + h1 * h2 + h2)
    props = torch.cuda.get_device_properties(0)
    clock_hz = float(getattr(props, "clock_rate", 2400000)) * 1e3
    mfma_floor_us = macs / (props.multi_processor_count * 128 * clock_hz) * 1e6
    value_read, value_write = n_rows * O * 4, n_rows * 4
    scan_read = T * E * (8 + 1) + (T + 1) * E * 4 + T * E * A * 4
    scan_write = 3 * T * E * 4
    d_us, b_us = ctypes.c_float(), ctypes.c_float()
    check(lib().sng_bandwidth_probe(0, scan_read, scan_write, 20, ctypes.byref(d_us), ctypes.byref(b_us),
                                    _stream_handle(venv.device)))
    scan_floor = d_us.value
    check(lib().sng_bandwidth_probe(0, value_read, value_write, 20, ctypes.byref(d_us), ctypes.byref(b_us),
                                    _stream_handle(venv.device)))
    print(json.dumps({"build_id": lib().sng_build_id().decode(), "envs": E, "chargers": N, "net_arch": list(arch), "T": T,
                      "obs_dim": O, "act_dim": A, "launch_gpu_us_min": best, "launch_gpu_us_spread": spread,
                      "max_abs_difference_to_torch": agree,
                      "floors": {"value_rows": n_rows, "value_padded_macs": macs, "value_real_macs": real_macs,
                                 "compute_units": props.multi_processor_count, "clock_ghz": clock_hz / 1e9,
                                 "value_mfma_floor_us": round(mfma_floor_us, 2),
                                 "value_read_bytes": value_read, "value_write_bytes": value_write,
                                 "value_hbm_copy_dispatch_us": round(d_us.value, 2),
                                 "scan_read_bytes": scan_read, "scan_write_bytes": scan_write,
                                 "scan_hbm_copy_dispatch_us": round(scan_floor, 2),
                                 "finish_over_mfma_plus_scan_floor": round(best["finish"] / (mfma_floor_us + scan_floor), 2)}}),
          flush=True)
    ro.close()
    venv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--chargers", default="8,10")
    ap.add_argument("--nets", default="256x256,400x300")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    for N in (int(x) for x in args.chargers.split(",")):
        for arch in (tuple(int(h) for h in net.split("x")) for net in args.nets.split(",")):
            one(args, N, arch)
    return 0


if __name__ == "__main__":
    sys.exit(main())
