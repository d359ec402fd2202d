#!/usr/bin/env python3
"""Cost of rsik_reach_map: a cubic grid of n_pos positions around the right shoulder (the box of the tests' grid) with n_rot random
orientations, n_pos x n_rot = 32768 x 512, 262144 x 64 and 4096 x 4096 (16.8 M poses each), three ways to the same four arrays
(count, state_count, theta_measure, mask):
  (a) one rsik_reach_map with all four outputs;
  (b) one rsik_solve under RSIK_THETA_NONE on the same poses tiled position-major (the tiled inputs are built ahead and not timed),
      with its interval, reachable and state outputs — the launch alone, no reduction;
  (c) form (b) followed by the torch reductions that produce the four arrays.
HIP events on the stream, the three forms interleaved in rounds in one process, medians and the spread of the rounds.  Prints one
JSON line: us per form, the ratios, poses per second.

    python scripts/reach_map_cost.py [--launches 3] [--rounds 7]
"""
import argparse
import contextlib
import io
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from reachy2_symbolic_ik_amd import SymbolicIK, _abi  # noqa: E402

SHAPES = [(32768, 512), (262144, 64), (4096, 4096)]


def time_launch(launch, k):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(k):
        launch()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / k  # us per call of `launch`


def grid_positions(n_pos):
    """A cubic grid of n_pos points over the box of the tests' map around the right shoulder (0, -0.2, 0); x varies slowest."""
    m = round(n_pos ** (1.0 / 3.0))
    assert m ** 3 == n_pos, "n_pos must be a cube"
    gx, gy, gz = np.meshgrid(np.linspace(-0.1, 0.7, m), -0.2 + np.linspace(-0.5, 0.5, m), np.linspace(-0.5, 0.5, m), indexing="ij")
    return np.ascontiguousarray(np.stack([gx.ravel(), gy.ravel(), gz.ravel()]))


def torch_reduce(res, n_pos, n_rot, bits):
    """The four arrays from rsik_solve's per-pose outputs (position-major), with torch."""
    ok = res["reachable"].view(n_pos, n_rot) != 0
    st = res["state"].view(n_pos, n_rot)
    itv = res["interval"].view(n_pos, n_rot, 2)
    w = itv[..., 1] - itv[..., 0]
    w = torch.where(itv[..., 0] > itv[..., 1], w + 2 * math.pi, w)
    words = (n_rot + 63) // 64
    padded = ok if n_rot == words * 64 else torch.nn.functional.pad(ok, (0, words * 64 - n_rot))
    return {"count": ok.sum(dim=1, dtype=torch.int32),
            "state_count": torch.stack([(st == c).sum(dim=1, dtype=torch.int32) for c in range(11)], dim=1),
            "theta_measure": torch.where(ok, w, torch.zeros_like(w)).sum(dim=1),
            "mask": (padded.view(n_pos, words, 64).to(torch.int64) << bits).sum(dim=2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", type=str, nargs="*", default=[f"{p}x{r}" for p, r in SHAPES])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    f64, u8 = torch.float64, torch.uint8
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", device=0)
    ik._upload()
    sv = ik.solver
    bits = torch.arange(64, dtype=torch.int64, device=dev)
    out = {}
    for shape in args.shapes:
        n_pos, n_rot = (int(v) for v in shape.split("x"))
        n = n_pos * n_rot
        pos = torch.as_tensor(grid_positions(n_pos)).to(dev)
        eul = torch.as_tensor(np.ascontiguousarray(np.random.default_rng(7).uniform(-np.pi, np.pi, size=(3, n_rot)))).to(dev)
        a = sv.reach_map(pos, eul, plan_only=True)
        tiled = torch.cat([pos.repeat_interleave(n_rot, dim=1), eul.repeat(1, n_pos)], dim=0).contiguous()
        solve_out = {"interval": torch.empty((n, 2), dtype=f64, device=dev), "reachable": torch.empty(n, dtype=u8, device=dev),
                     "state": torch.empty(n, dtype=u8, device=dev)}
        b = sv.solve(tiled, theta_policy=_abi.THETA_NONE, out=solve_out, plan_only=True)

        def solve_and_reduce(b=b, n_pos=n_pos, n_rot=n_rot):
            b["launch"]()
            return torch_reduce(b, n_pos, n_rot, bits)

        forms = {"reach_map": a["launch"], "solve": b["launch"], "solve_and_reduce": solve_and_reduce}
        for f in forms.values():  # warm-up, settled clock
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ref = solve_and_reduce()
        for key in ("count", "state_count", "mask"):
            assert torch.equal(ref[key], a[key]), f"the forms must agree: {key}"
        assert float((ref["theta_measure"] - a["theta_measure"]).abs().max()) <= n_rot ** 2 * 2 * math.pi * 2.0 ** -53
        t = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, f in forms.items():
                t[k].append(time_launch(f, args.launches))
        res = {"reachable_share": round(float(a["count"].sum()) / n, 4)}
        for k, v in t.items():
            res[f"{k}_us"] = round(float(np.median(v)), 1)
            res[f"{k}_us_min_max"] = [round(float(np.min(v)), 1), round(float(np.max(v)), 1)]
        med = float(np.median(t["reach_map"]))
        res["reach_map_over_solve"] = round(med / float(np.median(t["solve"])), 4)
        res["reach_map_over_solve_and_reduce"] = round(med / float(np.median(t["solve_and_reduce"])), 4)
        res["reach_map_poses_per_s"] = round(n / (med * 1e-6), 0)
        res["solve_poses_per_s"] = round(n / (float(np.median(t["solve"])) * 1e-6), 0)
        res["solve_and_reduce_poses_per_s"] = round(n / (float(np.median(t["solve_and_reduce"])) * 1e-6), 0)
        out[f"{n_pos}x{n_rot}"] = res
        del a, b, tiled, solve_out, ref, forms, solve_and_reduce
        torch.cuda.empty_cache()
    out["launches_per_median"] = args.launches * args.rounds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
