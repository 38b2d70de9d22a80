#!/usr/bin/env python3
"""A/B of the two forms a captured day can take (include/sng.h, sng_graph_create): one day-kernel node per day
against T step nodes (SNG_GRAPH_STEP_NODES), in one process, on one box, interleaved.

  tools/day_kernel_ab.py [--envs E] [--chargers N] [--time-interval 15min --extended-day --pv-noise s --price-noise s]
                         [--v2x] [--requested-soc] [--rng reference] [--steps-only]
                         [--days 100] [--graph-days 20] [--warmup 8] [--rounds 3] [--against serial_reset | generic_day]

The env, the actions and the graph shape are bench.py's (device-RNG days, `graph-days` days per replay, the day
return accumulated, no per-env flag array).  Each round replays the step-node graph for `days` days, then the
default graph, each between HIP events on the graphs' stream after `warmup` days of its own; one JSON line per
round with the device time per day of both forms, then one summary line.  With SNG_LIBRARY pointing at another
build of this source it measures that build the same way.
A station without a day kernel reports the same form twice (step_nodes_per_day says so).
--against serial_reset compares another pair of forms the same way: every day's reset ahead of its steps
(SNG_GRAPH_SERIAL_RESET) against the default, which generates day d + 1 beside day d's steps (reset_overlapped).
--against generic_day: day_wide_kernel (SNG_GRAPH_GENERIC_DAY) against the default, day_station_kernel at its station.
--steps-only (implied by --rng reference: a captured reset is device-RNG) times steps-only graphs: one day per
graph, an eager reset of the handle's RNG mode before every launch and the HIP events around the launch alone (the
reset keeps the device busy while the host queues the events and the graph, so the interval is the graph's)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smart-nanogrid-gym_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--chargers", type=int, default=10)
    ap.add_argument("--time-interval", default="1h")
    ap.add_argument("--extended-day", action="store_true")
    ap.add_argument("--pv-noise", type=float, default=0.0)
    ap.add_argument("--price-noise", type=float, default=0.0)
    ap.add_argument("--v2x", action="store_true")
    ap.add_argument("--requested-soc", action="store_true")
    ap.add_argument("--rng", choices=["device", "reference"], default="device")
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--days", type=int, default=100)
    ap.add_argument("--graph-days", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--against", choices=["step_nodes", "serial_reset", "generic_day"], default="step_nodes",
                    help="the other form: T step nodes per day, or every day's reset ahead of its steps "
                         "(SNG_GRAPH_SERIAL_RESET) against the default's overlapped reset, or the generic day kernel "
                         "(SNG_GRAPH_GENERIC_DAY) against the station-fixed one")
    args = ap.parse_args()
    from smart_nanogrid_gym import EpisodeGraph, SmartNanogridVecEnv
    from smart_nanogrid_gym._native import lib

    kw = dict(number_of_chargers=args.chargers, time_interval=args.time_interval, charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
              battery_system_available_in_model=True)
    if args.v2x:
        kw.update(vehicle_to_everything=True)
    if args.requested_soc:
        kw.update(enable_requested_state_of_charge=True)
    steps_only = args.steps_only or args.rng == "reference"
    if args.extended_day or args.pv_noise > 0 or args.price_noise > 0:
        kw.update(extended_day=args.extended_day, pv_noise=args.pv_noise, price_noise=args.price_noise)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    E = args.envs
    venv = SmartNanogridVecEnv(E, seed=args.seed, device=0, rng=args.rng, **kw)
    T, A = venv.timesteps, venv.act_dim
    g = torch.Generator(device=device).manual_seed(args.seed)
    low = torch.tensor(venv.action_space.low, device=device)
    high = torch.tensor(venv.action_space.high, device=device)
    acts = low + (high - low) * torch.rand((T, E, A), generator=g, device=device)
    acts = torch.where(torch.rand(acts.shape, generator=g, device=device) < 0.2, torch.zeros_like(acts), acts)
    acts = acts.contiguous()
    venv._info.flags = None   # as bench.py without --per-env-flags
    venv.reset_tensors(rng=args.rng)
    D = 1 if steps_only else max(1, args.graph_days)
    while args.days % D:
        D -= 1
    reset = not steps_only
    forms = {args.against: EpisodeGraph(venv, acts, with_reset=reset, days=D, **{args.against: True}),
             "default": EpisodeGraph(venv, acts, with_reset=reset, days=D)}
    nodes = {k: v.step_nodes_per_day for k, v in forms.items()}
    overlapped = {k: v.reset_overlapped for k, v in forms.items()}
    day_kernels = {k: getattr(v, "day_kernel_name", None) for k, v in forms.items()}   # None: a build before the entry

    def timed_steps_only(graph):
        total = 0.0
        for day in range(args.warmup + args.days):
            venv.reset_tensors(rng=args.rng)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.launch()
            e1.record()
            torch.cuda.synchronize()
            if day >= args.warmup:
                total += e0.elapsed_time(e1)
        return total * 1e3 / args.days

    def timed(graph):
        if steps_only:
            return timed_steps_only(graph)
        for _ in range(-(-args.warmup // D)):
            graph.launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.days // D):
            graph.launch()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.days

    rows = []
    for r in range(args.rounds):
        row = {k: round(timed(v), 3) for k, v in forms.items()}
        rows.append(row)
        print(json.dumps({"round": r, "day_gpu_us": row}), flush=True)
    best = {k: min(r[k] for r in rows) for k in forms}
    print(json.dumps({"build_id": lib().sng_build_id().decode(), "library": os.environ.get("SNG_LIBRARY", "in-tree"),
                      "envs": E, "chargers": args.chargers, "v2x": args.v2x, "requested_soc": args.requested_soc,
                      "rng": args.rng, "steps_only": steps_only, "kernel": venv.step_kernel_name(),
                      "T": T, "graph_days": D, "step_nodes_per_day": nodes, "reset_overlapped": overlapped, "day_kernel": day_kernels,
                      "day_gpu_us_min": best, "env_steps_per_s_min_time": {k: round(E * T / (v * 1e-6)) for k, v in best.items()},
                      f"ratio_{args.against}_over_default": round(best[args.against] / best["default"], 4)}), flush=True)
    for v in forms.values():
        v.close()
    venv.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
