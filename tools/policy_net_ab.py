#!/usr/bin/env python3
"""A/B of closed-loop days with SB3's DDPG actor (400-300 relu, tanh, rescaled into the action Box) in the loop, and
of policy_net_kernel itself, in one process, on one box, runs alternating (beside tools/policy_day_ab.py, which keeps
its outputs):

  torch   -- what a user has without sng_policy_create_net: the same net as a torch.nn actor, with the rescale,
             between step_tensors calls, captured with torch.cuda.graph (policy_day_ab.py's "torch" form);
  ddpg    -- ClosedLoopGraph(venv, MlpActor.ddpg(venv)): T x (policy_net_kernel node, step node) per day;
  mfma64  -- ClosedLoopGraph with the 64-64 tanh actor through policy_net_kernel (MlpActor(net=True));
  valu64  -- ClosedLoopGraph with the same actor through policy_kernel (the default 64-64 path).

  tools/policy_net_ab.py [--envs 65536] [--chargers 4] [--days 40] [--warmup 4] [--rounds 3] [--forms a,b]
  tools/policy_net_ab.py --profile [--chargers 4] [--out DIR]

All forms run device-RNG days (reset + T steps), the DDPG forms with the same weights, no noise; each round times
`days` days of each form between HIP events after `warmup` days of its own.  One JSON line per round with the device
time per day of every form, then the actor kernels on their own (`launches` back-to-back sng_policy_actions launches
between two events, per round), then one summary line with the build id, the minima, each form's spread (max - min
over the rounds), the DDPG kernel's achieved TFLOP/s (2 x FMAs of the real widths) and env-steps/s.
--profile reads the kernel averages, in a run of their own: it starts `rocprofv3 --kernel-trace --stats` over a
child run of this tool (the ddpg, mfma64 and valu64 forms, one round) before this process has touched the GPU, and
prints one JSON line per kernel of the child's stats file: calls, average, minimum and maximum in us."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smart-nanogrid-gym_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--chargers", type=int, default=4)
    ap.add_argument("--days", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--forms", default="torch,ddpg,mfma64,valu64")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None, help="--profile: where rocprofv3 writes (a temporary directory otherwise)")
    args = ap.parse_args()
    if args.profile:
        return profile(args)
    from smart_nanogrid_gym import ClosedLoopGraph, MlpActor, SmartNanogridVecEnv
    from smart_nanogrid_gym._native import lib

    E, N = args.envs, args.chargers
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
              battery_system_available_in_model=True)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    venv = SmartNanogridVecEnv(E, seed=args.seed, device=0, rng="device", **kw)
    venv._info.flags = None   # as bench.py without --per-env-flags
    T, O, A = venv.timesteps, venv.obs_dim, venv.act_dim
    torch.manual_seed(args.seed)
    nn = torch.nn
    net = nn.Sequential(nn.Linear(O, 400), nn.ReLU(), nn.Linear(400, 300), nn.ReLU(), nn.Linear(300, A), nn.Tanh()).to(device)
    low = torch.as_tensor(venv.action_space.low, device=device)
    high = torch.as_tensor(venv.action_space.high, device=device)
    net64 = nn.Sequential(nn.Linear(O, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, A)).to(device)

    def six(n):
        return [n[0].weight, n[0].bias, n[2].weight, n[2].bias, n[4].weight, n[4].bias]

    @torch.no_grad()
    def torch_day():
        obs = venv.reset_tensors()
        for _ in range(T):
            s = net(obs)
            obs, _, _ = venv.step_tensors(low + (0.5 * (s + 1.0) * (high - low)))   # SB3's unscale_action

    forms, nodes, actors = {}, {}, {}
    wanted = args.forms.split(",")
    if "torch" in wanted:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                torch_day()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        tg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(tg):
            torch_day()
        forms["torch"] = tg.replay
    if "ddpg" in wanted:
        actors["ddpg"] = MlpActor.ddpg(venv).load(six(net))
    if "mfma64" in wanted:
        actors["mfma64"] = MlpActor(venv, "tanh", net=True).load(six(net64))
    if "valu64" in wanted:
        actors["valu64"] = MlpActor(venv, "tanh").load(six(net64))
    for name, actor in actors.items():
        g = ClosedLoopGraph(venv, actor)
        forms[name], nodes[name] = g.launch, g.step_nodes

    def timed(run, count):
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(count):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / count

    rows, krows = [], []
    obs = venv.reset_tensors().clone()
    for r in range(args.rounds):
        row = {k: round(timed(v, args.days), 2) for k, v in forms.items()}
        rows.append(row)
        print(json.dumps({"round": r, "day_gpu_us": row}), flush=True)
        krow = {k: round(timed(lambda a=a: a.actions(obs), args.launches), 2) for k, a in actors.items()}
        krows.append(krow)
        print(json.dumps({"round": r, "actor_launch_us": krow}), flush=True)
    best = {k: min(r[k] for r in rows) for k in forms}
    spread = {k: round(max(r[k] for r in rows) - min(r[k] for r in rows), 2) for k in forms}
    kbest = {k: min(r[k] for r in krows) for k in actors}
    kspread = {k: round(max(r[k] for r in krows) - min(r[k] for r in krows), 2) for k in actors}
    out = {"build_id": lib().sng_build_id().decode(), "envs": E, "chargers": N, "T": T,
           "kernel": venv.step_kernel_name(), "step_nodes": nodes, "day_gpu_us_min": best, "day_gpu_us_spread": spread,
           "actor_launch_us_min": kbest, "actor_launch_us_spread": kspread,
           "env_steps_per_s_min_time": {k: round(E * T / (v * 1e-6)) for k, v in best.items()}}
    if "ddpg" in kbest:
        fmas = O * 400 + 400 * 300 + 300 * A
        out["ddpg_fma_per_row"] = fmas
        out["ddpg_tflops_at_min"] = round(2 * fmas * E / (kbest["ddpg"] * 1e-6) / 1e12, 2)
    print(json.dumps(out), flush=True)
    return 0


def profile(args):
    out = args.out or tempfile.mkdtemp(prefix="policy_net_ab_")
    child = [sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--chargers", str(args.chargers),
             "--forms", "ddpg,mfma64,valu64", "--rounds", "1", "--days", "10", "--warmup", "2", "--launches", "20",
             "--seed", str(args.seed)]
    run = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run", "--output-format", "csv",
                          "--"] + child, capture_output=True, text=True)
    if run.returncode != 0:
        sys.stderr.write(run.stdout[-2000:] + run.stderr[-2000:])
        return run.returncode
    print(run.stdout.strip().splitlines()[-1])   # the child's summary line (its build id)
    stats = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
    if not stats:
        sys.stderr.write(f"no kernel stats under {out}\n")
        return 1
    with open(stats[0]) as f:
        for row in csv.DictReader(f):
            if "sng::" in row["Name"]:
                print(json.dumps({"kernel": row["Name"].split("(")[0], "calls": int(row["Calls"]),
                                  "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                                  "min_us": round(float(row["MinNs"]) / 1e3, 2),
                                  "max_us": round(float(row["MaxNs"]) / 1e3, 2)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
