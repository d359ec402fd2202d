#!/usr/bin/env python3
"""Cost of rsik_solve_nearest: of K fractions of the interval, the sample nearest to a seed row, for config 2's poses at
(n, K) = (262 144, 64), (4096, 64), (64, 1024), (2, 1024), and at 65 536, 32 768 and 16 384 x 64, between which the choice goes from
one lane per pose to eight.  Forms, all ending in the same [n, 7] joints:
  nearest_L1 / _L8 / _L64   one rsik_solve_nearest with RSIK_OPT_NEAREST_LANES forced to 1, 8, 64 lanes per pose;
  nearest_auto              the same with the library's own choice;
  sweep                     the rsik_solve_sweep launch alone (what the parent route starts with);
  sweep_torch               rsik_solve_sweep followed by torch's angle_diff / sum / argmin / gather on its [K, n, 7] output.
HIP events on the stream, the forms interleaved in rounds in one process after at least 50 ms of untimed launches, medians and the
spread of the rounds.  RSIK_OPT_NEAREST_LANES is set ahead of a form's burst of launches, outside its pair of events: between the events
every form is its planned launch and nothing else.  Prints one JSON line.

    python scripts/nearest_cost.py [--launches 5] [--rounds 7]
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
from reachy2_symbolic_ik_amd import SymbolicIK, _abi  # noqa: E402

SHAPES = ((1 << 18, 64), (1 << 16, 64), (1 << 15, 64), (1 << 14, 64), (4096, 64), (64, 1024), (2, 1024))


def time_launch(launch, k, setup=None):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if setup is not None:
        setup()
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
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    f64, u8 = torch.float64, torch.uint8
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", device=0)
    sv = ik.solver
    pos, eul = make_config2_poses(max(n for n, _ in SHAPES))
    out = {}
    for n, K in SHAPES:
        pose = torch.as_tensor(np.ascontiguousarray(np.concatenate([pos[:n].T, eul[:n].T], axis=0))).to(dev)
        seed = torch.as_tensor(np.random.default_rng(5).uniform(-2.0, 2.0, size=(n, 7))).to(dev)
        grid = torch.linspace(0.0, 1.0, K, dtype=f64, device=dev)
        per_pose = {"interval": torch.empty((n, 2), dtype=f64, device=dev), "reachable": torch.empty(n, dtype=u8, device=dev),
                    "state": torch.empty(n, dtype=u8, device=dev)}
        sweep_out = dict(per_pose, joints=torch.empty((K, n, 7), dtype=f64, device=dev), elbow=torch.empty((K, n, 3), dtype=f64, device=dev),
                         projected=torch.empty((K, n), dtype=u8, device=dev), theta=torch.empty((K, n), dtype=f64, device=dev))
        sweep = sv.solve_sweep(pose, grid, policy="fraction", out=sweep_out, plan_only=True)["launch"]
        near_out = dict(per_pose, index=torch.empty(n, dtype=torch.int32, device=dev), theta=torch.empty(n, dtype=f64, device=dev),
                        joints=torch.empty((n, 7), dtype=f64, device=dev), elbow=torch.empty((n, 3), dtype=f64, device=dev),
                        cost=torch.empty(n, dtype=f64, device=dev), projected=torch.empty(n, dtype=u8, device=dev))
        nearest = sv.solve_nearest(pose, grid, seed, policy="fraction", out=near_out, plan_only=True)["launch"]
        picked = {}

        def lanes_set(lanes):  # (the entry point reads the option at every call: set once per burst, ahead of its events)
            return lambda: sv.set_option(_abi.OPT_NEAREST_LANES, lanes)

        def sweep_torch():
            sweep()
            j = sweep_out["joints"]
            d = torch.remainder(j - seed[None] + math.pi, 2 * math.pi) - math.pi
            c = (d * d).sum(dim=2)
            c = torch.where(sweep_out["reachable"][None].bool() & ~torch.isnan(c), c, torch.full_like(c, float("inf")))
            idx = torch.argmin(c, dim=0)
            picked["index"] = idx
            picked["joints"] = torch.gather(j, 0, idx[None, :, None].expand(1, n, 7))[0]

        forms = {"nearest_L1": nearest, "nearest_L8": nearest, "nearest_L64": nearest, "nearest_auto": nearest,
                 "sweep": sweep, "sweep_torch": sweep_torch}
        setups = {"nearest_L1": lanes_set(1), "nearest_L8": lanes_set(8), "nearest_L64": lanes_set(64), "nearest_auto": lanes_set(0)}
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.05:  # at least 50 ms of untimed launches: settled clock, warm caches and allocator
            for k, f in forms.items():
                setups.get(k, lambda: None)()
                f()
            torch.cuda.synchronize()
        ok = sweep_out["reachable"].bool()
        agree = float((picked["index"][ok] == near_out["index"][ok].long()).double().mean()) if bool(ok.any()) else 1.0
        t = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, f in forms.items():
                t[k].append(time_launch(f, args.launches, setups.get(k)))
        res = {"index_agrees_with_torch": round(agree, 6)}
        for k, v in t.items():
            res[f"{k}_us"] = round(float(np.median(v)), 1)
            res[f"{k}_us_min_max"] = [round(float(np.min(v)), 1), round(float(np.max(v)), 1)]
        med = {k: float(np.median(v)) for k, v in t.items()}
        for lanes in (1, 8, 64):
            res[f"nearest_L{lanes}_over_sweep"] = round(med[f"nearest_L{lanes}"] / med["sweep"], 4)
        res["nearest_auto_over_sweep_torch"] = round(med["nearest_auto"] / med["sweep_torch"], 4)
        res["fastest_form"] = min((f"nearest_L{lanes}" for lanes in (1, 8, 64)), key=lambda k: med[k])
        res["nearest_auto_samples_per_s"] = round(K * n / (med["nearest_auto"] * 1e-6), 0)
        out[f"n_{n}_K_{K}"] = res
        sv.set_option(_abi.OPT_NEAREST_LANES, 0)
        del sweep_out, near_out, picked, sweep, nearest
        torch.cuda.empty_cache()
    out["launches_per_median"] = args.launches * args.rounds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
