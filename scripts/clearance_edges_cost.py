#!/usr/bin/env python3
"""Cost of rsik_clearance_edges: the clearance along the motion between the waypoints of a path, on scripts/path_clear_cost.py's
workload and shapes ((n, T) = (4096, 64) with K = 16 and (256, 256) with K = 64; the joints are rsik_solve_path_clear's winners with
64 spheres and min_clearance = 0, skipped waypoints included as NaN rows; start joints given), S = 16 sub-steps.  The obstacles are
scripts/track_avoid_cost.py's seeded spheres.  Forms:
  edges_16, edges_64, edges_256
                    one rsik_clearance_edges call (planned) with that many spheres and all nine outputs: the per-edge kernel and
                    the per-path fold behind it;
  edges_64_edge_only
                    the same with 64 spheres and the four per-edge outputs alone: one kernel, no workspace;
  composed_16, composed_64, composed_256
                    the same answer composed from what the library offered before: the rows before each waypoint (a forward fill
                    over the NaN rows) and the interpolation in torch, written as [S + 1][T n][7]; one rsik_clearance launch with
                    n_rep = S + 1 over it (clearance and nearest); torch min / argmin / gather over the sub-steps, the bound, and the
                    per-path min / argmin / counts;
  clearance_16, clearance_64, clearance_256
                    that composition's rsik_clearance launch alone, on the interpolated rows it left behind.
HIP events on the stream, the forms interleaved in rounds in one process after at least 50 ms of untimed launches, medians and the
spread of the rounds.  Prints one JSON line.

    python scripts/clearance_edges_cost.py [--launches 2] [--rounds 5]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench import make_config2_poses  # noqa: E402
from path_cost import SHAPES, time_launch  # noqa: E402
from reachy2_symbolic_ik_amd import SymbolicIK  # noqa: E402
from reachy2_symbolic_ik_amd import constants as KC  # noqa: E402
from track_avoid_cost import RADIUS, make_scene  # noqa: E402

N_SUB = 16
SPHERES = (16, 64, 256)
MIN_CLEARANCE = 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    f64 = torch.float64
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", device=0)
    ik._upload()
    sv = ik.solver
    pos, eul = make_config2_poses(2 * max(n for n, _, _ in SHAPES))
    scenes = {s: make_scene(s, 0, dev)[0] for s in SPHERES}
    block = np.asarray(ik.consts)
    tip = float(np.linalg.norm(block[KC.C_TIPL:KC.C_TIPL + 3]))
    u, f = float(block[KC.C_UPPER_ARM]), float(block[KC.C_FOREARM])
    reach = torch.tensor([u + f + tip, u + f + tip, f + tip, f + tip, tip, tip, tip], dtype=f64, device=dev)
    S = N_SUB
    out = {}
    for n, T, K in SHAPES:
        s = np.linspace(0.0, 1.0, T)[:, None, None]
        line = np.concatenate([pos[None, :n] + s * (pos[n:2 * n] - pos[:n])[None], eul[None, :n] + s * (eul[n:2 * n] - eul[:n])[None]], axis=2)
        pose = torch.as_tensor(np.ascontiguousarray(line.transpose(2, 0, 1))).to(dev)  # [6, T, n]
        start = torch.as_tensor(np.random.default_rng(5).uniform(-2.0, 2.0, size=(n, 7))).to(dev)
        grid = torch.linspace(0.0, 1.0, K, dtype=f64, device=dev)
        won = sv.solve_path_clear(pose, grid, start, spheres=scenes[64], link_radius=RADIUS, min_clearance=0.0, influence=0.05, clearance_gain=100.0)
        J = won["joints"].clone()  # [T, n, 7], NaN rows at the skipped waypoints
        del won

        edges = {c: sv.clearance_edges(J, start, S, spheres=scenes[c], link_radius=RADIUS, min_clearance=MIN_CLEARANCE, plan_only=True) for c in SPHERES}
        edge_only = sv.clearance_edges(J, start, S, spheres=scenes[64], link_radius=RADIUS, want=sv.CLEARANCE_EDGES_OUTPUTS[:4], plan_only=True)
        q = torch.empty((S + 1, T * n, 7), dtype=f64, device=dev)
        clr = {c: sv.clearance(q, spheres=scenes[c], link_radius=RADIUS, want=("clearance", "nearest"), plan_only=True) for c in SPHERES}
        frac = (torch.arange(S, dtype=f64, device=dev) / S)[:, None, None, None]
        steps = torch.arange(T, device=dev)[:, None]
        picked = {}

        def composed(c):
            fin = torch.isfinite(J).all(dim=-1)  # [T, n]
            last = torch.cummax(torch.where(fin, steps, -1), dim=0).values
            prev = torch.cat([torch.full((1, n), -1, device=dev, dtype=last.dtype), last[:-1]], dim=0)  # the last waypoint before t
            a = torch.where((prev >= 0)[..., None], torch.gather(J, 0, prev.clamp(min=0)[..., None].expand(T, n, 7)), start[None])
            delta = torch.remainder(J - a + math.pi, 2 * math.pi) - math.pi
            qv = q.view(S + 1, T, n, 7)
            qv[:S] = a[None] + delta[None] * frac
            qv[S] = J
            clr[c]["launch"]()
            d = clr[c]["clearance"].view(S + 1, T, n)
            ec, es = d.min(dim=0)
            en = torch.gather(clr[c]["nearest"].view(S + 1, T, n, 2), 0, es[None, ..., None].expand(1, T, n, 2))[0]
            eb = ec - 0.5 * ((delta.abs() * reach).sum(dim=-1) / S)
            big = torch.where(fin, ec, float("inf"))
            pc, pt = big.min(dim=0)
            pb = torch.where(fin, eb, float("inf")).min(dim=0).values
            below = fin & (ec < MIN_CLEARANCE)
            picked.update(edge_clearance=ec, edge_sub=torch.where(fin, es, -1), edge_nearest=en, edge_bound=eb, path_clearance=pc,
                          path_edge=torch.stack([pt, torch.gather(es, 0, pt[None])[0]], dim=1), path_bound=pb, n_below=below.sum(dim=0),
                          first_below=torch.where(below.any(dim=0), below.int().argmax(dim=0), -1))

        forms = {f"edges_{c}": edges[c]["launch"] for c in SPHERES}
        forms["edges_64_edge_only"] = edge_only["launch"]
        for c in SPHERES:
            forms[f"composed_{c}"] = (lambda c=c: composed(c))
            forms[f"clearance_{c}"] = clr[c]["launch"]
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.05:  # at least 50 ms of untimed launches: settled clock, warm caches and allocator
            for fn in forms.values():
                fn()
            torch.cuda.synchronize()
        composed(64)
        torch.cuda.synchronize()
        got = edges[64]
        wp = got["edge_sub"] >= 0
        res = {"edges": int(wp.sum()), "rows_not_waypoints": int((~wp).sum()),
               "edge_clearance_same_bits_as_composed": round(float((got["edge_clearance"][wp] == picked["edge_clearance"][wp]).double().mean()), 6),
               "edge_clearance_largest_difference": float((got["edge_clearance"][wp] - picked["edge_clearance"][wp]).abs().max()),
               "edge_bound_largest_difference": float((got["edge_bound"][wp] - picked["edge_bound"][wp]).abs().max()),
               "edge_sub_agrees": round(float((got["edge_sub"][wp] == picked["edge_sub"][wp]).double().mean()), 6),
               "n_below_agrees": bool((got["n_below"] == picked["n_below"]).all()),
               "edges_whose_minimum_is_strictly_inside": round(float((got["edge_sub"] % S != 0)[wp].double().mean()), 4),
               "edges_below_0": round(float((got["edge_clearance"] < 0)[wp].double().mean()), 4),
               "edges_proven_free": round(float((got["edge_bound"] > 0)[wp].double().mean()), 4)}
        tm = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                tm[k].append(time_launch(fn, args.launches))
        med = {k: float(np.median(v)) for k, v in tm.items()}
        for k, v in tm.items():
            res[f"{k}_us"] = round(med[k], 1)
            res[f"{k}_us_min_max"] = [round(float(np.min(v)), 1), round(float(np.max(v)), 1)]
        for c in SPHERES:
            res[f"edges_{c}_over_composed"] = round(med[f"edges_{c}"] / med[f"composed_{c}"], 4)
            res[f"edges_{c}_over_clearance_alone"] = round(med[f"edges_{c}"] / med[f"clearance_{c}"], 4)
        res["fold_us"] = round(med["edges_64"] - med["edges_64_edge_only"], 1)
        out[f"n_{n}_T_{T}_S_{S}"] = res
        del edges, edge_only, clr, q, forms, picked, J
        torch.cuda.empty_cache()
    out["launches_per_median"] = args.launches * args.rounds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
