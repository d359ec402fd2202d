#!/usr/bin/env python3
"""Cost of rsik_solve_path_clear: rsik_solve_path among static obstacles, on scripts/path_cost.py's workload and shapes
((n, T, K) = (4096, 64, 16) and (256, 256, 64), straight lines between config 2's poses, start joints given).  The obstacles are
scripts/track_avoid_cost.py's seeded spheres, 0.25 ... 0.7 m from the shoulder with radii of 0.02 ... 0.06 m; link radii, influence
0.05 m.  Forms:
  clear_16, clear_64, clear_256
                    one rsik_solve_path_clear launch (planned) with that many spheres, the soft term alone (min_clearance -inf, gain
                    100): the candidates, and with them the dynamic programme's work, are rsik_solve_path's, so that the difference
                    to `path` is the price of the clearance of every sample;
  clear_64_hard     the same with 64 spheres and min_clearance = 0: blocked samples leave the dynamic programme;
  path              one rsik_solve_path launch (planned) on the same inputs;
  composed_64_hard  clear_64_hard's answer composed from what the library offered before: rsik_solve_sweep over the T * n poses,
                    rsik_clearance over its [K][T n][7] joints (n_rep = K), and scripts/path_cost.py's torch dynamic programme
                    with the mask d >= min_clearance and the node penalty, then the backtrack and the gather of the winners' joints.
HIP events on the stream, the forms interleaved in rounds in one process after at least 50 ms of untimed launches, medians and the
spread of the rounds.  Prints one JSON line.

    python scripts/path_clear_cost.py [--launches 2] [--rounds 5]
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
from track_avoid_cost import RADIUS, make_scene  # noqa: E402

INFLUENCE, GAIN = 0.05, 100.0
SPHERES = (16, 64, 256)


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
    scenes = {s: make_scene(s, 0, dev)[0] for s in SPHERES}
    out = {}
    for n, T, K in SHAPES:
        s = np.linspace(0.0, 1.0, T)[:, None, None]
        line = np.concatenate([pos[None, :n] + s * (pos[n:2 * n] - pos[:n])[None], eul[None, :n] + s * (eul[n:2 * n] - eul[:n])[None]], axis=2)
        pose = torch.as_tensor(np.ascontiguousarray(line.transpose(2, 0, 1))).to(dev)  # [6, T, n]
        flat = pose.reshape(6, T * n)
        start = torch.as_tensor(np.random.default_rng(5).uniform(-2.0, 2.0, size=(n, 7))).to(dev)
        grid = torch.linspace(0.0, 1.0, K, dtype=f64, device=dev)

        sweep_out = dict(interval=torch.empty((T * n, 2), dtype=f64, device=dev), reachable=torch.empty((T * n,), dtype=u8, device=dev),
                         state=torch.empty((T * n,), dtype=u8, device=dev), joints=torch.empty((K, T * n, 7), dtype=f64, device=dev),
                         elbow=torch.empty((K, T * n, 3), dtype=f64, device=dev), projected=torch.empty((K, T * n), dtype=u8, device=dev),
                         theta=torch.empty((K, T * n), dtype=f64, device=dev))
        sweep = sv.solve_sweep(flat, grid, policy="fraction", out=sweep_out, plan_only=True)["launch"]
        clr_res = sv.clearance(sweep_out["joints"], spheres=scenes[64], link_radius=RADIUS, want=("clearance",), plan_only=True)
        path_res = sv.solve_path(pose, grid, start, policy="fraction", plan_only=True)
        soft = {c: sv.solve_path_clear(pose, grid, start, spheres=scenes[c], link_radius=RADIUS, influence=INFLUENCE, clearance_gain=GAIN,
                                       plan_only=True) for c in SPHERES}
        hard = sv.solve_path_clear(pose, grid, start, spheres=scenes[64], link_radius=RADIUS, min_clearance=0.0, influence=INFLUENCE,
                                   clearance_gain=GAIN, plan_only=True)

        picked = {}
        inf = torch.tensor(float("inf"), dtype=f64, device=dev)
        zero = torch.zeros((), dtype=f64, device=dev)

        def cost(a, b):  # c(a, b) summed over the joints: [..., 7] -> [...]
            d = torch.remainder(b - a + math.pi, 2 * math.pi) - math.pi
            return (d * d).sum(dim=-1)

        def composed():
            sweep()
            clr_res["launch"]()
            J = sweep_out["joints"].view(K, T, n, 7)
            d = clr_res["clearance"].view(K, T, n)
            cand = (sweep_out["reachable"].view(T, n).bool())[None] & ~torch.isnan(J).any(dim=-1) & (d >= 0.0)  # [K, T, n]
            u = INFLUENCE - d
            pen = torch.where(d < INFLUENCE, (GAIN * u) * u, zero)
            solved = cand.any(dim=0)  # [T, n]
            have = torch.zeros(n, dtype=torch.bool, device=dev)
            pj = torch.zeros((K, n, 7), dtype=f64, device=dev)
            pa = torch.full((K, n), float("inf"), dtype=f64, device=dev)
            pc = torch.zeros((K, n), dtype=torch.bool, device=dev)
            back = torch.empty((T, K, n), dtype=torch.int64, device=dev)
            for t in range(T):
                here = cand[:, t]
                first = torch.where(here, cost(start[None], J[:, t]) + pen[:, t], inf)
                total = torch.where(pc[:, None] & here[None], pa[:, None] + cost(pj[:, None], J[None, :, t]), inf)  # [i, j, n]
                best, back[t] = total.min(dim=0)
                a = torch.where(have[None], best + pen[:, t], first)
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

        forms = {f"clear_{c}": soft[c]["launch"] for c in SPHERES}
        forms.update(clear_64_hard=hard["launch"], path=path_res["launch"], composed_64_hard=composed)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.05:  # at least 50 ms of untimed launches: settled clock, warm caches and allocator
            for f in forms.values():
                f()
            torch.cuda.synchronize()
        won = hard["index"] >= 0
        agree = float((picked["index"][won] == hard["index"][won].long()).double().mean()) if bool(won.any()) else 1.0
        same_skips = bool(((picked["index"] >= 0) == won).all())
        has = hard["n_solved"] > 0
        cost_err = float((picked["cost"][has] - hard["cost"][has]).abs().max()) if bool(has.any()) else 0.0
        free_won = path_res["index"] >= 0
        tm = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, f in forms.items():
                tm[k].append(time_launch(f, args.launches))
        res = {"index_agrees_with_torch": round(agree, 6), "same_skipped_waypoints": same_skips, "largest_cost_difference": cost_err,
               "waypoints_solved_path": round(float(free_won.double().mean()), 4), "waypoints_solved_hard": round(float(won.double().mean()), 4),
               "soft_paths_differing_from_path": {str(c): int((soft[c]["index"] != path_res["index"]).any(dim=0).sum()) for c in SPHERES},
               "soft_same_skips_as_path": all(bool(((soft[c]["index"] >= 0) == free_won).all()) for c in SPHERES),
               "candidates_blocked_hard": round(float(hard["blocked"].double().sum() / max(float(K * free_won.double().sum()), 1.0)), 4)}
        for k, v in tm.items():
            res[f"{k}_us"] = round(float(np.median(v)), 1)
            res[f"{k}_us_min_max"] = [round(float(np.min(v)), 1), round(float(np.max(v)), 1)]
        med = {k: float(np.median(v)) for k, v in tm.items()}
        for c in SPHERES:
            res[f"clear_{c}_over_path"] = round(med[f"clear_{c}"] / med["path"], 4)
        # The price of the constraint per sphere (the slope from the smallest to the largest scene), and per sphere, solved waypoint and
        # wave: a path is a wave, the chip has 1024 SIMDs, and the waves of a SIMD are taken as running one after another.  A launch
        # lasts as long as its longest wave, so the figure is given against the mean path and against the path with the most solved waypoints.
        waves_per_simd = max(1.0, n / 1024.0)
        per_sphere = (med[f"clear_{SPHERES[-1]}"] - med[f"clear_{SPHERES[0]}"]) / (SPHERES[-1] - SPHERES[0])
        solved_mean = float(path_res["n_solved"].double().mean())
        solved_most = int(path_res["n_solved"].max())
        res["us_per_sphere"] = round(per_sphere, 2)
        res["solved_waypoints_mean_most"] = [round(solved_mean, 1), solved_most]
        res["us_per_sphere_waypoint_wave_mean_path"] = round(per_sphere / (solved_mean * waves_per_simd), 4)
        res["us_per_sphere_waypoint_wave_longest_path"] = round(per_sphere / (solved_most * waves_per_simd), 4)
        res["clear_64_hard_over_composed"] = round(med["clear_64_hard"] / med["composed_64_hard"], 4)
        res["clear_64_hard_over_path"] = round(med["clear_64_hard"] / med["path"], 4)
        out[f"n_{n}_T_{T}_K_{K}"] = res
        del sweep_out, path_res, picked, sweep, soft, hard, clr_res, forms
        torch.cuda.empty_cache()
    out["launches_per_median"] = args.launches * args.rounds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
