#!/usr/bin/env python3
"""A/B of the ways to run closed-loop days with the 64-64 tanh MLP actor in the loop, in one process, on one box,
runs alternating (modelled on tools/day_kernel_ab.py):

  torch    -- tools/closed_loop_bench.py --policy mlp's graph (its mlp_policy): a torch.nn actor between
              step_tensors calls, captured with torch.cuda.graph;
  nodes    -- ClosedLoopGraph(step_nodes=True): T x (policy_kernel node, step node) per day;
  fused    -- ClosedLoopGraph(fused=True): day_lean_policy_kernel, one node a day, where the station has it (else the
              node form again; step_nodes says which);
  default  -- ClosedLoopGraph(): what policy_day_form (csrc/sng_graph_form.h) gives the plan.

  tools/policy_day_ab.py [--envs 65536] [--chargers 8] [--days 40] [--warmup 4] [--rounds 3] [--forms a,b]
  tools/policy_day_ab.py --profile [--chargers 8] [--out DIR]

All forms run device-RNG days (reset + T steps) with the same weights and no noise; each round times `days` days of
each form between HIP events after `warmup` days of its own.  One JSON line per round with the device time per day
of every form, then one summary line with the build id, the minima, each form's spread (max - min over the rounds)
and env-steps/s.
--profile reads the kernel averages, in a run of their own: it starts `rocprofv3 --kernel-trace --stats` over a
child run of this tool (the node and the fused form, one round) before this process has touched the GPU, and prints
one JSON line per kernel of the child's stats file: calls, average, minimum and maximum in us."""
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
    ap.add_argument("--chargers", type=int, default=8)
    ap.add_argument("--days", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--forms", default="torch,nodes,fused,default")
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
    T = venv.timesteps
    from closed_loop_bench import mlp_policy
    net, ctl = mlp_policy(venv, args.seed)
    actor = MlpActor(venv, "tanh").load([net[0].weight, net[0].bias, net[2].weight, net[2].bias, net[4].weight,
                                         net[4].bias])

    @torch.no_grad()
    def torch_day():
        obs = venv.reset_tensors()
        for _ in range(T):
            obs, _, _ = venv.step_tensors(ctl(obs))

    forms, nodes = {}, {}
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
    if "nodes" in wanted:
        g = ClosedLoopGraph(venv, actor, step_nodes=True)
        forms["nodes"], nodes["nodes"] = g.launch, g.step_nodes
    if "fused" in wanted:
        g = ClosedLoopGraph(venv, actor, fused=True)
        forms["fused"], nodes["fused"] = g.launch, g.step_nodes
    if "default" in wanted:
        g = ClosedLoopGraph(venv, actor)
        forms["default"], nodes["default"] = g.launch, g.step_nodes

    def timed(run):
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.days):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.days

    rows = []
    for r in range(args.rounds):
        row = {k: round(timed(v), 2) for k, v in forms.items()}
        rows.append(row)
        print(json.dumps({"round": r, "day_gpu_us": row}), flush=True)
    best = {k: min(r[k] for r in rows) for k in forms}
    spread = {k: round(max(r[k] for r in rows) - min(r[k] for r in rows), 2) for k in forms}
    print(json.dumps({"build_id": lib().sng_build_id().decode(), "envs": E, "chargers": N, "T": T,
                      "kernel": venv.step_kernel_name(), "step_nodes": nodes, "day_gpu_us_min": best,
                      "day_gpu_us_spread": spread,
                      "env_steps_per_s_min_time": {k: round(E * T / (v * 1e-6)) for k, v in best.items()}}), flush=True)
    return 0


def profile(args):
    out = args.out or tempfile.mkdtemp(prefix="policy_day_ab_")
    child = [sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--chargers", str(args.chargers),
             "--forms", "nodes,fused", "--rounds", "1", "--days", "10", "--warmup", "2", "--seed", str(args.seed)]
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
