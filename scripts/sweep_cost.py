#!/usr/bin/env python3
"""Cost of rsik_solve_sweep: K elbow angles (fractions of the interval) for each of config 2's poses, n = 262 144 and 1 Mi,
K in {1, 4, 16, 64}, three ways to the same [K, n, 7] joints and [K, n, 3] elbows:
  (a) one rsik_solve_sweep with a shared grid of K fractions;
  (b) K launches of rsik_solve with RSIK_THETA_FRACTION, each into its slice of the same output buffers;
  (c) one rsik_solve on the poses tiled K times (the tiled inputs are built ahead and not timed).
HIP events on the stream, the three forms interleaved in rounds in one process, medians and the spread of the rounds.  Prints one
JSON line: us per form, samples per second, bytes per second of the sweep against the 8 TB/s roofline.

    python scripts/sweep_cost.py [--launches 5] [--rounds 7]
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import make_config2_poses  # noqa: E402
from reachy2_symbolic_ik_amd import SymbolicIK, _abi  # noqa: E402

ROOFLINE = 8e12  # bytes per second


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
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1 << 18, 1 << 20])
    ap.add_argument("--samples", type=int, nargs="*", default=[1, 4, 16, 64])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    f64, u8 = torch.float64, torch.uint8
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", device=0)
    sv = ik.solver
    pos, eul = make_config2_poses(max(args.sizes))
    out = {}
    for n in args.sizes:
        pose = torch.as_tensor(np.ascontiguousarray(np.concatenate([pos[:n].T, eul[:n].T], axis=0))).to(dev)
        for K in args.samples:
            grid = torch.linspace(0.0, 1.0, K, dtype=f64, device=dev) if K > 1 else torch.zeros(1, dtype=f64, device=dev)
            joints, elbow = torch.empty((K, n, 7), dtype=f64, device=dev), torch.empty((K, n, 3), dtype=f64, device=dev)
            per_pose = {"interval": torch.empty((n, 2), dtype=f64, device=dev), "reachable": torch.empty(n, dtype=u8, device=dev),
                        "state": torch.empty(n, dtype=u8, device=dev)}
            sweep_out = dict(per_pose, joints=joints, elbow=elbow, projected=torch.empty((K, n), dtype=u8, device=dev),
                             theta=torch.empty((K, n), dtype=f64, device=dev))
            a = sv.solve_sweep(pose, grid, policy="fraction", out=sweep_out, plan_only=True)
            cols = grid[:, None].expand(K, n).contiguous()
            plans = [sv.solve(pose, theta_policy=_abi.THETA_FRACTION, theta_in=cols[k], out=dict(per_pose, joints=joints[k], elbow=elbow[k]),
                              plan_only=True) for k in range(K)]
            tiled = pose.repeat(1, K)
            tiled_out = {"joints": torch.empty((K * n, 7), dtype=f64, device=dev), "elbow": torch.empty((K * n, 3), dtype=f64, device=dev),
                         "interval": torch.empty((K * n, 2), dtype=f64, device=dev), "reachable": torch.empty(K * n, dtype=u8, device=dev),
                         "state": torch.empty(K * n, dtype=u8, device=dev)}
            c = sv.solve(tiled, theta_policy=_abi.THETA_FRACTION, theta_in=cols.reshape(-1), out=tiled_out, plan_only=True)

            def k_launches(plans=plans):
                for q in plans:
                    q["launch"]()

            forms = {"sweep": a["launch"], "k_solves": k_launches, "tiled_solve": c["launch"]}
            for f in forms.values():  # warm-up, settled clock
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            assert torch.equal(tiled_out["joints"].view(K, n, 7).view(torch.int64), joints.view(torch.int64)), "the three forms must agree"
            t = {k: [] for k in forms}
            for _ in range(args.rounds):
                for k, f in forms.items():
                    t[k].append(time_launch(f, args.launches))
            res = {}
            for k, v in t.items():
                res[f"{k}_us"] = round(float(np.median(v)), 1)
                res[f"{k}_us_min_max"] = [round(float(np.min(v)), 1), round(float(np.max(v)), 1)]
            med = float(np.median(t["sweep"]))
            res["sweep_over_k_solves"] = round(med / float(np.median(t["k_solves"])), 4)
            res["sweep_over_tiled_solve"] = round(med / float(np.median(t["tiled_solve"])), 4)
            res["sweep_samples_per_s"] = round(K * n / (med * 1e-6), 0)
            nbytes = n * (48 + 18) + K * n * (56 + 24 + 1 + 8)  # read 48, written 16 + 1 + 1 per pose; 89 written per sample
            res["sweep_bytes_per_s"] = round(nbytes / (med * 1e-6), 0)
            res["sweep_fraction_of_8TBps"] = round(nbytes / (med * 1e-6) / ROOFLINE, 4)
            out[f"n_{n}_K_{K}"] = res
            del a, plans, c, tiled, tiled_out, sweep_out, joints, elbow, cols
            torch.cuda.empty_cache()
    out["launches_per_median"] = args.launches * args.rounds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
