#!/usr/bin/env python3
"""What DDPG's gradient step costs on the device, and the same update in torch, in one process, on one box, runs
alternating (modelled on tools/ddpg_targets_ab.py):

  update              -- DdpgLearner.update(samples, y): both nets' forward and backward passes, Adam, polyak and the
                         repack of the four device images (27 launches);
  train_step          -- DdpgLearner.train(ring, B, 1): sample + targets + update;
  torch_eager_update  -- the same update on torch.nn nets with torch.optim.Adam and SB3's polyak_update (foreach);
  torch_graph_update  -- that update captured with torch.cuda.graph and Adam(capturable=True), replayed;
  load_round_trip     -- what an update in torch costs a caller of the library besides: the four nets' weights to the
                         host and MlpActor.load / QCritic.load four times (pack on the CPU, upload), host wall time.

  tools/ddpg_update_ab.py [--envs 65536] [--chargers 4,10] [--batches 256,65536] [--net 400x300] [--reps 20]
                          [--warmup 3] [--rounds 3]

For every station and batch, each round times `reps` runs of each form between HIP events after `warmup` runs of its
own (load_round_trip with the host clock around a synchronise).  One JSON line per round, then one summary line with
the build id, the minima, each form's spread over the rounds, the largest difference of the weights after one update
from the same start to torch's, and the floors: the update's real multiply-adds at the f32-input MFMA's rate, 128 a
clock a compute unit, the bytes of the weights, moments and images an update must read and write at least, and for
each of the 27 launches its padded multiply-adds at that rate and its bytes at the HBM peak (`launches`).  The
kernels' own times come from a kernel trace of this tool (rocprofv3 --kernel-trace --stats, a run of its own).
load_round_trip is measured on this build: MlpActor.load and QCritic.load are the code they were before the learner."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smart-nanogrid-gym_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from ddpg_targets_ab import mlp, six  # noqa: E402


def launch_floors(B, O, A, h1, h2, rate, hbm):
    """An update's 27 launches in their order: the kernel, the product's M x N x K as learn_gemm_kernel pads it (M and N
    to 32-row and 32-column tiles, K to the MFMA's two), its multiply-adds at `rate` a second, and the bytes it must
    read and write once at `hbm` bytes a second."""
    up = lambda v, to: (v + to - 1) // to * to   # noqa: E731
    K = O + A
    out = []

    def gemm(name, M, N, Kr, extra=0):
        macs = up(M, 32) * up(N, 32) * up(Kr, 2)
        nbytes = 4 * (M * Kr + Kr * N + M * N + extra)
        out.append({"kernel": name, "M": M, "N": N, "K": Kr, "padded_macs": macs,
                    "mfma_floor_us": round(macs / rate * 1e6, 3), "bytes": nbytes,
                    "byte_floor_us": round(nbytes / hbm * 1e6, 3)})

    def plain(name, nbytes):
        out.append({"kernel": name, "bytes": nbytes, "byte_floor_us": round(nbytes / hbm * 1e6, 3)})

    def critic_forward():
        gemm("learn_gemm_kernel<relu> critic layer 1", B, h1, K)
        gemm("learn_gemm_kernel<relu> critic layer 2", B, h2, h1)
        gemm("learn_gemm_kernel<none> critic layer 3", B, 1, h2)

    def critic_backward():
        gemm("learn_gemm_kernel<mask> critic dh2", B, h2, 1, B * h2)
        gemm("learn_gemm_kernel<mask> critic dh1", B, h1, h2, B * h1)

    def step(name, params, image):   # master, two moments and target read and written, gradient both, two images
        plain(name, 4 * (params * (4 * 2 + 2) + 2 * image))
    critic_params, actor_params = K * h1 + h1 * h2 + h2 + h1 + h2 + 1, O * h1 + h1 * h2 + h2 * A + h1 + h2 + A
    plain("learn_concat_kernel", 4 * 2 * B * K)
    critic_forward()
    plain("learn_loss_kernel<critic>", 4 * 3 * B)
    critic_backward()
    gemm("learn_gemm_kernel<none> critic dW3, db3", 1, h2 + 1, B)
    gemm("learn_gemm_kernel<none> critic dW2, db2", h2, h1 + 1, B)
    gemm("learn_gemm_kernel<none> critic dW1, db1", h1, K + 1, B)
    step("learn_step_kernel<adam> critic", critic_params, critic_params)
    gemm("learn_gemm_kernel<relu> actor layer 1", B, h1, O)
    gemm("learn_gemm_kernel<relu> actor layer 2", B, h2, h1)
    gemm("learn_gemm_kernel<tanh> actor layer 3", B, A, h2, B * A)
    critic_forward()
    plain("learn_loss_kernel<actor>", 4 * 2 * B)
    critic_backward()
    gemm("learn_gemm_kernel<dtanh> action columns", B, A, h1, B * A)
    gemm("learn_gemm_kernel<mask> actor dh2", B, h2, A, B * h2)
    gemm("learn_gemm_kernel<mask> actor dh1", B, h1, h2, B * h1)
    gemm("learn_gemm_kernel<none> actor dW3, db3", A, h2 + 1, B)
    gemm("learn_gemm_kernel<none> actor dW2, db2", h2, h1 + 1, B)
    gemm("learn_gemm_kernel<none> actor dW1, db1", h1, O + 1, B)
    step("learn_step_kernel<adam> actor", actor_params, actor_params)
    assert len(out) == 27
    return out


def one(args, N, arch):
    from smart_nanogrid_gym import (ActionNoise, DdpgCollector, DdpgLearner, MlpActor, QCritic, ReplayRing,
                                    SmartNanogridVecEnv)
    from smart_nanogrid_gym._native import lib
    from smart_nanogrid_gym.ddpg import LEARNER_NETS, net_keys

    E = args.envs
    h1, h2 = arch
    kw = dict(number_of_chargers=N, time_interval="1h", charging_mode="bounded",
              vehicle_uncharged_penalty_mode="sparse", pv_system_available_in_model=True,
              battery_system_available_in_model=True)
    device = torch.device("cuda", 0)
    venv = SmartNanogridVecEnv(E, seed=args.seed, device=0, rng="device", **kw)
    venv._info.flags = None   # as bench.py without --per-env-flags
    O, A = venv.obs_dim, venv.act_dim
    gamma, tau, lr = 0.99, 0.005, 1e-3
    torch.manual_seed(args.seed)
    start = {"actor": mlp(O, h1, h2, A, device), "critic": mlp(O + A, h1, h2, 1, device),
             "actor_target": mlp(O, h1, h2, A, device), "critic_target": mlp(O + A, h1, h2, 1, device)}
    start_sd = {k: {n: p.detach().clone() for n, p in m.state_dict().items()} for k, m in start.items()}

    def handles():
        a = MlpActor(venv, "relu", net_arch=arch, squash=True).load(six(start["actor"]))
        a_t = MlpActor(venv, "relu", net_arch=arch, squash=True).load(six(start["actor_target"]))
        c, c_t = QCritic(venv, arch).load(six(start["critic"])), QCritic(venv, arch).load(six(start["critic_target"]))
        return a, c, a_t, c_t
    actor, critic, actor_t, critic_t = nets = handles()
    noise = ActionNoise(venv, "ou", seed=args.seed, scale=0.5)
    ring = ReplayRing(venv, 2, seed=args.seed)
    col = DdpgCollector(venv, actor, noise, ring, days=1)
    col.launch()
    col.launch()
    torch.cuda.synchronize()
    learner = DdpgLearner(venv, *nets, actor_lr=lr, critic_lr=lr, tau=tau, gamma=gamma)
    props = torch.cuda.get_device_properties(0)
    clock_hz = float(getattr(props, "clock_rate", 2400000)) * 1e3
    summary = {"build_id": lib().sng_build_id().decode(), "envs": E, "chargers": N, "net_arch": list(arch),
               "obs_dim": O, "act_dim": A, "batches": {}}

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

    def wall(run):
        run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            run()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / args.reps

    def torch_side(capturable):
        """(nets, update) of a torch learner from the common start."""
        t = {k: mlp(O + A if "critic" in k else O, h1, h2, 1 if "critic" in k else A, device) for k in start}
        for k, m in t.items():
            m.load_state_dict(start_sd[k])
        opt = {k: torch.optim.Adam(t[k].parameters(), lr=lr, capturable=capturable) for k in ("actor", "critic")}
        pairs = [(list(t[k + "_target"].parameters()), list(t[k].parameters())) for k in ("actor", "critic")]

        def update(obs, act, y):
            q = t["critic"](torch.cat([obs, act], 1))
            loss = ((q - y) ** 2).mean()
            opt["critic"].zero_grad(set_to_none=True)
            loss.backward()
            opt["critic"].step()
            a_loss = -t["critic"](torch.cat([obs, torch.tanh(t["actor"](obs))], 1)).mean()
            opt["actor"].zero_grad(set_to_none=True)
            a_loss.backward()
            opt["actor"].step()
            with torch.no_grad():
                for target, params in pairs:
                    torch._foreach_mul_(target, 1 - tau)
                    torch._foreach_add_(target, params, alpha=tau)
        return t, update

    for B in args.batch_list:
        samples = ring.sample(B)
        y, _ = critic_t.targets(actor_t, samples, gamma)
        obs, act, y = samples.observations.clone(), samples.actions.clone(), y.clone()
        frozen = samples._replace(observations=obs, actions=act)
        # one update from the common start on both sides: the largest difference of the weights
        fresh = handles()
        probe = DdpgLearner(venv, *fresh, actor_lr=lr, critic_lr=lr, tau=tau, gamma=gamma).update(frozen, y)
        t_nets, t_update = torch_side(False)
        t_update(obs, act, y)
        torch.cuda.synchronize()
        agree = max(float((probe.params[key] - p.detach()).abs().max())
                    for name, prefix in LEARNER_NETS.items()
                    for key, p in zip(net_keys(prefix), six(t_nets[name])))
        probe.close()
        for x in fresh:
            x.close()
        forms = {"update": lambda: learner.update(frozen, y), "train_step": lambda: learner.train(ring, B, 1),
                 "torch_eager_update": lambda: t_update(obs, act, y)}
        try:
            _, g_update = torch_side(True)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    g_update(obs, act, y)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            tg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(tg):
                g_update(obs, act, y)
            tg.replay()
            torch.cuda.synchronize()
            forms["torch_graph_update"] = tg.replay
            graph_note = "captured"
        except Exception as e:   # the capture is torch's to refuse
            graph_note = f"not captured: {type(e).__name__}: {str(e)[:200]}"
            torch.cuda.synchronize()

        def round_trip():
            for h, name in zip(nets, ("actor", "critic", "actor_target", "critic_target")):
                h.load([p.detach().cpu() for p in six(t_nets[name])])
        rows = []
        for r in range(args.rounds):
            row = {k: round(timed(v), 2) for k, v in forms.items()}
            rows.append(row)
            print(json.dumps({"chargers": N, "batch": B, "round": r, "gpu_us": row}), flush=True)
        best = {k: min(r[k] for r in rows) for k in forms}
        spread = {k: round(max(r[k] for r in rows) - min(r[k] for r in rows), 2) for k in forms}
        load_us = round(min(wall(round_trip) for _ in range(args.rounds)), 1)
        learner.load_state(learner.host_state())   # the four images back to the learner's masters
        K = O + A
        critic_macs, actor_macs = K * h1 + h1 * h2 + h2, O * h1 + h1 * h2 + h2 * A
        # critic: forward twice, dh2 / dh1 twice, the action columns once, weight gradients once; actor: each once
        macs = B * (2 * critic_macs + 2 * (h2 + h2 * h1) + h1 * A + critic_macs + 3 * actor_macs - O * h1)
        params = critic_macs + h1 + h2 + 1 + actor_macs + h1 + h2 + A
        rate = props.multi_processor_count * 128 * clock_hz
        floors = {"real_macs": macs, "compute_units": props.multi_processor_count, "clock_ghz": clock_hz / 1e9,
                  "mfma_floor_us": round(macs / rate * 1e6, 2),
                  # master, two moments and the target read and written, the gradient written and read, two images written
                  "state_bytes": params * 4 * (4 * 2 + 2 + 2)}
        floors["launches"] = launch_floors(B, O, A, h1, h2, rate, args.hbm_bytes_per_s)
        summary["batches"][str(B)] = {"gpu_us_min": best, "gpu_us_spread": spread, "torch_graph": graph_note,
                                      "load_round_trip_host_us": load_us,
                                      "max_abs_difference_of_weights_to_torch": agree, "floors": floors}
    print(json.dumps(summary), flush=True)
    for x in (learner, col, *nets, noise, ring, venv):
        x.close()


def trace_times(path, B, O, A, h1, h2):
    """Per launch of an update, from a rocprofv3 kernel trace (CSV) of a run of this tool at one batch size: the
    learner's dispatches in start order, cut into updates of 27 (set_state's two repack launches left out), and per
    position the minimum and the mean device time in us beside launch_floors' entry."""
    import csv
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "learn_" in r.get("Kernel_Name", "")
                and "learn_step_kernel<false>" not in r["Kernel_Name"] and "learn_step_kernelILb0" not in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    floors = launch_floors(B, O, A, h1, h2, 256 * 128 * 2.4e9, 8e12)
    updates = [rows[i:i + 27] for i in range(0, len(rows) - 26, 27)]
    updates = [u for u in updates if "concat" in u[0]["Kernel_Name"] and "step" in u[26]["Kernel_Name"]]
    out = []
    for i, fl in enumerate(floors):
        us = [(int(u[i]["End_Timestamp"]) - int(u[i]["Start_Timestamp"])) / 1e3 for u in updates]
        out.append(dict(fl, traced=updates[0][i]["Kernel_Name"][:40], us_min=round(min(us), 2), us_mean=round(sum(us) / len(us), 2)))
    total = [(int(u[26]["End_Timestamp"]) - int(u[0]["Start_Timestamp"])) / 1e3 for u in updates]
    print(json.dumps({"batch": B, "obs_dim": O, "act_dim": A, "net_arch": [h1, h2], "updates_traced": len(updates),
                      "update_first_start_to_last_end_us_min": round(min(total), 2),
                      "sum_of_kernel_us_min": round(sum(o["us_min"] for o in out), 2), "launches": out}))


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
    ap.add_argument("--hbm-bytes-per-s", type=float, default=8e12, help="the byte floors' rate: the part's HBM peak")
    ap.add_argument("--trace-csv", help="no run: per-launch times from this rocprofv3 kernel trace of a one-station, "
                                        "one-batch run (--chargers N --batches B)")
    args = ap.parse_args()
    args.batch_list = [int(b) for b in args.batches.split(",")]
    arch = tuple(int(h) for h in args.net.split("x"))
    if args.trace_csv:
        n = int(args.chargers.split(",")[0])
        trace_times(args.trace_csv, args.batch_list[0], 2 * n + 9, n + 1, *arch)
        return 0
    torch.cuda.set_device(0)
    for N in (int(x) for x in args.chargers.split(",")):
        one(args, N, arch)
    return 0


if __name__ == "__main__":
    sys.exit(main())
