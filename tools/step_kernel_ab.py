#!/usr/bin/env python3
"""Device time of one station's eager step kernel, for A/Bs of two builds of the library (SNG_LIBRARY):

  tools/step_kernel_ab.py [--envs E] [--chargers N] [--info] [--v2x] [--days 20] [--warmup-days 3] [--rounds 3]

Device-RNG days stepped eagerly by SmartNanogridVecEnv.time_step_kernels (HIP start/stop events on every step
kernel dispatch), Box-uniform actions with a fifth exact zeros, reused every day.  --info writes the per-step
diagnostics, which selects the general kernel.  One JSON line per round (median and mean over the round's
days x T dispatches, in us), then one summary line with the kernel's name and the library's build id.
tools/day_kernel_ab.py does the same for a captured day."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smart-nanogrid-gym_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--chargers", type=int, default=8)
    ap.add_argument("--info", action="store_true")
    ap.add_argument("--v2x", action="store_true")
    ap.add_argument("--days", type=int, default=20)
    ap.add_argument("--warmup-days", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    from smart_nanogrid_gym import SmartNanogridVecEnv
    from smart_nanogrid_gym._native import lib

    kw = dict(number_of_chargers=args.chargers, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
              battery_system_available_in_model=True, vehicle_to_everything=args.v2x)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    E = args.envs
    venv = SmartNanogridVecEnv(E, seed=args.seed, device=0, rng="device", info=args.info, **kw)
    T, A = venv.timesteps, venv.act_dim
    g = torch.Generator(device=device).manual_seed(args.seed)
    low = torch.tensor(venv.action_space.low, device=device)
    high = torch.tensor(venv.action_space.high, device=device)
    acts = low + (high - low) * torch.rand((T, E, A), generator=g, device=device)
    acts = torch.where(torch.rand(acts.shape, generator=g, device=device) < 0.2, torch.zeros_like(acts), acts).contiguous()
    venv.time_step_kernels(acts, days=args.warmup_days)
    rows = []
    for r in range(args.rounds):
        us = venv.time_step_kernels(acts, days=args.days).astype(np.float64) * 1e3
        rows.append({"median": round(float(np.median(us)), 3), "mean": round(float(us.mean()), 3)})
        print(json.dumps({"round": r, "step_us": rows[-1]}), flush=True)
    print(json.dumps({"build_id": lib().sng_build_id().decode(), "library": os.environ.get("SNG_LIBRARY", "in-tree"),
                      "kernel": venv.step_kernel_name(), "envs": E, "chargers": args.chargers, "T": T,
                      "dispatches_per_round": args.days * T,
                      "step_us_median": round(float(np.median([r["median"] for r in rows])), 3)}), flush=True)
    venv.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
