#!/usr/bin/env python3
"""Cost of rsik_solve_path: the least-motion way through K fractions of the interval at each of T waypoints of n paths (straight
lines between config 2's poses), at (n, T, K) = (4096, 64, 16) and (256, 256, 64).  Forms:
  path              one rsik_solve_path launch (planned), start joints given;
  sweep             the rsik_solve_sweep launch over the T * n poses alone (what the other exact route starts with);
  sweep_torch       rsik_solve_sweep followed by torch: per waypoint a batched [K, K, n] angle_diff / sum / min with the skip rule,
                    then the backtrack and the gather of the winners' joints — the same answer as `path`;
  nearest_chain     T rsik_solve_nearest launches (planned), each seeded with the joints the one before wrote: the greedy answer, a
                    different one, for scale only (a waypoint without a winner hands NaN on: its cost is the same).
HIP events on the stream, the forms interleaved in rounds in one process after at least 50 ms of untimed launches, medians and the
spread of the rounds.  Prints one JSON line.

    python scripts/path_cost.py [--launches 2] [--rounds 5]
"""
import argparse
import contextlib
import io
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import make_config2_poses  # noqa: E402
from reachy2_symbolic_ik_amd import SymbolicIK  # noqa: E402

SHAPES = ((4096, 64, 16), (256, 256, 64))


def time_launch(launch, k):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(k):
        launch()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / k  # us per call of `launch`


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    f64, u8 = torch.float64, torch.uint8
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", device=0)
    sv = ik.solver
    pos, eul = make_config2_poses(2 * max(n for n, _, _ in SHAPES))
    out = {}
    for n, T, K in SHAPES:
        s = np.linspace(0.0, 1.0, T)[:, None, None]
        line = np.concatenate([pos[None, :n] + s * (pos[n:2 * n] - pos[:n])[None], eul[None, :n] + s * (eul[n:2 * n] - eul[:n])[None]], axis=2)
        pose = torch.as_tensor(np.ascontiguousarray(line.transpose(2, 0, 1))).to(dev)  # [6, T, n]
        flat = pose.reshape(6, T * n)
        start = torch.as_tensor(np.random.default_rng(5).uniform(-2.0, 2.0, size=(n, 7))).to(dev)
        grid = torch.linspace(0.0, 1.0, K, dtype=f64, device=dev)

        def bufs(*lead):
            return dict(interval=torch.empty(lead + (2,), dtype=f64, device=dev), reachable=torch.empty(lead, dtype=u8, device=dev),
                        state=torch.empty(lead, dtype=u8, device=dev))

        sweep_out = dict(bufs(T * n), joints=torch.empty((K, T * n, 7), dtype=f64, device=dev), elbow=torch.empty((K, T * n, 3), dtype=f64, device=dev),
                         projected=torch.empty((K, T * n), dtype=u8, device=dev), theta=torch.empty((K, T * n), dtype=f64, device=dev))
        sweep = sv.solve_sweep(flat, grid, policy="fraction", out=sweep_out, plan_only=True)["launch"]
        path_res = sv.solve_path(pose, grid, start, policy="fraction", plan_only=True)
        path = path_res["launch"]
        steps = []
        seed = start
        for t in range(T):
            near = sv.solve_nearest(pose[:, t], grid, seed, policy="fraction", plan_only=True)
            steps.append(near)
            seed = near["joints"]

        def nearest_chain():
            for near in steps:
                near["launch"]()

        picked = {}
        inf = torch.tensor(float("inf"), dtype=f64, device=dev)

        def cost(a, b):  # c(a, b) summed over the joints: [..., 7] -> [...]
            d = torch.remainder(b - a + math.pi, 2 * math.pi) - math.pi
            return (d * d).sum(dim=-1)

        def sweep_torch():
            sweep()
            J = sweep_out["joints"].view(K, T, n, 7)
            cand = (sweep_out["reachable"].view(T, n).bool())[None] & ~torch.isnan(J).any(dim=-1)  # [K, T, n]
            solved = cand.any(dim=0)  # [T, n]
            have = torch.zeros(n, dtype=torch.bool, device=dev)
            pj = torch.zeros((K, n, 7), dtype=f64, device=dev)
            pa = torch.full((K, n), float("inf"), dtype=f64, device=dev)
            pc = torch.zeros((K, n), dtype=torch.bool, device=dev)
            back = torch.empty((T, K, n), dtype=torch.int64, device=dev)
            for t in range(T):
                here = cand[:, t]
                first = torch.where(here, cost(start[None], J[:, t]), inf)
                total = torch.where(pc[:, None] & here[None], pa[:, None] + cost(pj[:, None], J[None, :, t]), inf)  # [i, j, n]
                best, back[t] = total.min(dim=0)
                a = torch.where(have[None], best, first)
                upd = solved[t]
                pj = torch.where(upd[None, :, None], torch.nan_to_num(J[:, t]), pj)
                pa = torch.where(upd[None], a, pa)
                pc = torch.where(upd[None], here, pc)
                have = have | upd
            k = pa.argmin(dim=0)  # [n]
            index = torch.full((T, n), -1, dtype=torch.int64, device=dev)
            for t in range(T - 1, -1, -1):
                index[t] = torch.where(solved[t], k, index[t])
                k = torch.where(solved[t], back[t].gather(0, k[None])[0], k)
            picked["index"] = index
            picked["cost"] = pa.min(dim=0).values
            picked["joints"] = torch.gather(J, 0, index.clamp(min=0)[None, :, :, None].expand(1, T, n, 7))[0]

        forms = {"path": path, "sweep": sweep, "sweep_torch": sweep_torch, "nearest_chain": nearest_chain}
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.05:  # at least 50 ms of untimed launches: settled clock, warm caches and allocator
            for f in forms.values():
                f()
            torch.cuda.synchronize()
        won = path_res["index"] >= 0
        agree = float((picked["index"][won] == path_res["index"][won].long()).double().mean()) if bool(won.any()) else 1.0
        same_skips = bool(((picked["index"] >= 0) == won).all())
        has = path_res["n_solved"] > 0
        cost_err = float((picked["cost"][has] - path_res["cost"][has]).abs().max()) if bool(has.any()) else 0.0
        tm = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, f in forms.items():
                tm[k].append(time_launch(f, args.launches))
        res = {"index_agrees_with_torch": round(agree, 6), "same_skipped_waypoints": same_skips, "largest_cost_difference": cost_err,
               "waypoints_solved": round(float(won.double().mean()), 4)}
        for k, v in tm.items():
            res[f"{k}_us"] = round(float(np.median(v)), 1)
            res[f"{k}_us_min_max"] = [round(float(np.min(v)), 1), round(float(np.max(v)), 1)]
        med = {k: float(np.median(v)) for k, v in tm.items()}
        res["path_over_sweep_torch"] = round(med["path"] / med["sweep_torch"], 4)
        res["path_over_sweep"] = round(med["path"] / med["sweep"], 4)
        res["path_over_nearest_chain"] = round(med["path"] / med["nearest_chain"], 4)
        res["path_samples_per_s"] = round(K * T * n / (med["path"] * 1e-6), 0)
        out[f"n_{n}_T_{T}_K_{K}"] = res
        del sweep_out, path_res, picked, sweep, path, steps
        torch.cuda.empty_cache()
    out["launches_per_median"] = args.launches * args.rounds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
