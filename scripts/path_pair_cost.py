#!/usr/bin/env python3
"""Cost of rsik_solve_path_pair: the elbow paths of both arms of a robot chosen together, each arm an obstacle to the other.  Shapes
(robots, T, K) = (2048, 64, 16) and (128, 256, 16): straight lines between config 2's poses for the right arms, between their mirror
images for the left arms, start joints given; without a static scene and with scripts/track_avoid_cost.py's 64 seeded spheres; link
radii, min_clearance 0, influence 0.05 m, gain 100.  Forms:
  pair        one rsik_solve_path_pair launch (planned);
  composed    (i) the same answer composed from what the library offered before, the only other exact route: rsik_solve_sweep over
              the T * n poses, rsik_clearance over its [K][T n][7] joints for the link points (and the static clearance), then per
              waypoint a torch broadcast of the K^2 x 9 segment pairs (the five-candidate segment distance rsik_clearance uses), the
              mask and the penalty, and a torch dynamic programme over the K^2 states in rsik.h's two stages, the backtrack and the
              gather of the winners' joints;
  uncoupled   (ii) one rsik_solve_path_clear launch (planned) on the same 2 * robots rows with arm bytes 0, 1, 0, 1, ... and three
              static capsules in the partner's place: each arm alone, the lower mark.
HIP events on the stream, the forms interleaved in rounds in one process after at least 50 ms of untimed launches, medians and the
spread of the rounds.  Prints one JSON line.

    python scripts/path_pair_cost.py [--launches 2] [--rounds 5]
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
from path_cost import time_launch  # noqa: E402
from reachy2_symbolic_ik_amd import DualArmIK, SymbolicIK  # noqa: E402
from track_avoid_cost import RADIUS, make_scene  # noqa: E402

SHAPES = ((2048, 64, 16), (128, 256, 16))
HARD, INFLUENCE, GAIN = 0.0, 0.05, 100.0
MIRROR = np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0])  # a right arm's pose as the left arm's: y, roll and yaw change sign


def segment_distance(P0, e, Q0, f):
    """The distance of the segments P0 + s e and Q0 + t f, s, t in [0, 1] (broadcast over the leading dimensions): the smallest of
    the four end-point candidates and the interior critical point, as rsik_clearance forms it."""
    r = P0 - Q0
    ee, ff = (e * e).sum(-1), (f * f).sum(-1)
    b, c, fr = (e * f).sum(-1), (e * r).sum(-1), (f * r).sum(-1)
    inv_ee, inv_ff = 1.0 / ee.clamp(min=1e-300), 1.0 / ff.clamp(min=1e-300)
    den = ee * ff - b * b
    cl = lambda v: v.clamp(0.0, 1.0)  # noqa: E731
    s4 = cl((b * fr - c * ff) / torch.where(den > 1e-300, den, torch.ones_like(den)))
    cands = ((torch.zeros_like(b), cl(fr * inv_ff)), (torch.ones_like(b), cl((fr + b) * inv_ff)), (cl(-c * inv_ee), torch.zeros_like(b)),
             (cl((b - c) * inv_ee), torch.ones_like(b)), (s4, cl((b * s4 + fr) * inv_ff)))
    best = None
    for s, t in cands:
        v = r + s[..., None] * e - t[..., None] * f
        q = (v * v).sum(-1)
        best = q if best is None else torch.minimum(best, q)
    return best.sqrt()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    f64, u8 = torch.float64, torch.uint8
    with contextlib.redirect_stdout(io.StringIO()):
        r_arm = SymbolicIK("r_arm", device=0)
        sv = r_arm.solver
        r_arm._upload()
        SymbolicIK("l_arm", solver=sv)._upload()
        DualArmIK(solver=sv)
    most = max(n for n, _, _ in SHAPES)
    pos, eul = make_config2_poses(4 * most)
    pose6 = np.concatenate([pos, eul], axis=1)
    rad = torch.tensor(RADIUS, dtype=f64, device=dev)
    far_sphere = torch.tensor([[50.0, 0.0, 0.0, 0.1]], dtype=f64, device=dev)
    stand_in = make_scene(0, 3, dev)[1]  # (ii): three static capsules in the partner's place
    out = {}
    for robots, T, K in SHAPES:
        n = 2 * robots
        ends = np.empty((2, n, 6))
        ends[0, 0::2], ends[1, 0::2] = pose6[:robots], pose6[robots:2 * robots]
        ends[0, 1::2], ends[1, 1::2] = pose6[2 * most:2 * most + robots] * MIRROR, pose6[3 * most:3 * most + robots] * MIRROR
        s = np.linspace(0.0, 1.0, T)[:, None, None]
        line = ends[0][None] + s * (ends[1] - ends[0])[None]  # [T, n, 6]
        pose = torch.as_tensor(np.ascontiguousarray(line.transpose(2, 0, 1))).to(dev)  # [6, T, n]
        flat = pose.reshape(6, T * n)
        start = torch.as_tensor(np.random.default_rng(5).uniform(-2.0, 2.0, size=(n, 7))).to(dev)
        grid = torch.linspace(0.0, 1.0, K, dtype=f64, device=dev)
        arm = torch.tensor([0, 1], dtype=u8, device=dev).repeat(robots)
        arm_flat = arm.repeat(T)
        res = {}
        for scene_name, spheres in (("no_scene", None), ("spheres_64", make_scene(64, 0, dev)[0])):
            sweep_out = dict(interval=torch.empty((T * n, 2), dtype=f64, device=dev), reachable=torch.empty((T * n,), dtype=u8, device=dev),
                             state=torch.empty((T * n,), dtype=u8, device=dev), joints=torch.empty((K, T * n, 7), dtype=f64, device=dev),
                             elbow=torch.empty((K, T * n, 3), dtype=f64, device=dev), projected=torch.empty((K, T * n), dtype=u8, device=dev),
                             theta=torch.empty((K, T * n), dtype=f64, device=dev))
            sweep = sv.solve_sweep(flat, grid, policy="fraction", arm=arm_flat, out=sweep_out, plan_only=True)["launch"]
            clr_res = sv.clearance(sweep_out["joints"], spheres=far_sphere if spheres is None else spheres, link_radius=RADIUS, arm=arm_flat,
                                   want=("clearance", "link_points"), plan_only=True)
            kw = dict(link_radius=RADIUS, min_clearance=HARD, influence=INFLUENCE, clearance_gain=GAIN, policy="fraction", plan_only=True)
            pair = sv.solve_path_pair(pose, grid, start, spheres=spheres, **kw)
            alone = sv.solve_path_clear(pose, grid, start, spheres=spheres, capsules=stand_in, arm=arm, **kw)
            picked = {}
            inf = torch.tensor(float("inf"), dtype=f64, device=dev)
            zero = torch.zeros((), dtype=f64, device=dev)

            def cost(a, b):  # c(a, b) summed over the joints: [..., 7] -> [...]
                d = torch.remainder(b - a + math.pi, 2 * math.pi) - math.pi
                return (d * d).sum(dim=-1)

            def pen_of(d):
                u = INFLUENCE - d
                return torch.where(d < INFLUENCE, (GAIN * u) * u, zero)

            def composed():
                sweep()
                clr_res["launch"]()
                J = torch.nan_to_num(sweep_out["joints"].view(K, T, robots, 2, 7))
                LP = clr_res["link_points"].view(K, T, robots, 2, 4, 3)
                st = clr_res["clearance"].view(K, T, robots, 2)
                row = (sweep_out["reachable"].view(T, robots, 2).bool())[None] & ~torch.isnan(sweep_out["joints"].view(K, T, robots, 2, 7)).any(dim=-1)
                have = torch.zeros(robots, dtype=torch.bool, device=dev)
                pj = torch.zeros((K, robots, 2, 7), dtype=f64, device=dev)
                pa = torch.full((K, K, robots), float("inf"), dtype=f64, device=dev)
                back_a = torch.empty((T, K, K, robots), dtype=torch.int64, device=dev)
                back_b = torch.empty((T, K, K, robots), dtype=torch.int64, device=dev)
                solved_all = torch.empty((T, robots), dtype=torch.bool, device=dev)
                kk, ar = torch.arange(K, device=dev), torch.arange(robots, device=dev)
                for t in range(T):
                    PR, PL = LP[:, t, :, 0], LP[:, t, :, 1]  # [K, robots, 4, 3]
                    P0 = PR[:, None, :, :3, None, :]          # [a, 1, robots, link, 1, 3]
                    e = (PR[:, :, 1:] - PR[:, :, :3])[:, None, :, :, None, :]
                    Q0 = PL[None, :, :, None, :3, :]          # [1, b, robots, 1, link, 3]
                    f = (PL[:, :, 1:] - PL[:, :, :3])[None, :, :, None, :, :]
                    cross = (segment_distance(P0, e, Q0, f) - rad[:, None] - rad[None, :]).amin(dim=(-1, -2))  # [a, b, robots]
                    if spheres is None:
                        dR, dL = cross, cross
                    else:
                        dR, dL = torch.minimum(cross, st[:, t, :, 0][:, None]), torch.minimum(cross, st[:, t, :, 1][None, :])
                    cand = row[:, t, :, 0][:, None] & row[:, t, :, 1][None, :] & (dR >= HARD) & (dL >= HARD)  # [a, b, robots]
                    pen = pen_of(dR) + pen_of(dL)
                    Jt = J[:, t]
                    first = torch.where(cand, (cost(start.view(robots, 2, 7)[None, :, 0], Jt[:, :, 0])[:, None]
                                               + cost(start.view(robots, 2, 7)[None, :, 1], Jt[:, :, 1])[None, :]) + pen, inf)
                    cL = cost(pj[:, None, :, 1], Jt[None, :, :, 1])  # [b, b', robots]
                    cR = cost(pj[:, None, :, 0], Jt[None, :, :, 0])  # [a, a', robots]
                    B1, arg1 = (pa[:, :, None] + cL[None]).min(dim=1)      # [a, b', robots]
                    best, arg2 = (B1[:, None] + cR[:, :, None]).min(dim=0)  # [a', b', robots]
                    later = torch.where(cand, best + pen, inf)
                    a_new = torch.where(have[None, None], later, first)
                    upd = cand.any(dim=0).any(dim=0)
                    solved_all[t] = upd
                    back_a[t] = arg2
                    back_b[t] = arg1[arg2, kk[None, :, None].expand(K, K, robots), ar[None, None, :].expand(K, K, robots)]  # the b of (a, b')
                    pj = torch.where(upd[None, :, None, None], Jt, pj)
                    pa = torch.where(upd[None, None], a_new, pa)
                    have = have | upd
                flat_a = pa.reshape(K * K, robots)
                end = flat_a.argmin(dim=0)
                a, b = end // K, end % K
                index = torch.full((T, robots, 2), -1, dtype=torch.int64, device=dev)
                for t in range(T - 1, -1, -1):
                    sol = solved_all[t]
                    index[t, :, 0] = torch.where(sol, a, index[t, :, 0])
                    index[t, :, 1] = torch.where(sol, b, index[t, :, 1])
                    na, nb = back_a[t][a, b, ar], back_b[t][a, b, ar]
                    a, b = torch.where(sol, na, a), torch.where(sol, nb, b)
                picked["index"] = index.reshape(T, n)
                picked["cost"] = flat_a.min(dim=0).values
                picked["joints"] = torch.gather(sweep_out["joints"].view(K, T, n, 7), 0, picked["index"].clamp(min=0)[None, :, :, None].expand(1, T, n, 7))[0]

            forms = dict(pair=pair["launch"], composed=composed, uncoupled=alone["launch"])
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.05:  # at least 50 ms of untimed launches: settled clock, warm caches and allocator
                for fn in forms.values():
                    fn()
                torch.cuda.synchronize()
            won = pair["index"] >= 0
            agree = float((picked["index"][won] == pair["index"][won].long()).double().mean()) if bool(won.any()) else 1.0
            same_skips = bool(((picked["index"] >= 0) == won).all())
            has = pair["n_solved"] > 0
            cost_err = float((picked["cost"][has] - pair["cost"][has]).abs().max()) if bool(has.any()) else 0.0
            tm = {k: [] for k in forms}
            for _ in range(args.rounds):
                for k, fn in forms.items():
                    tm[k].append(time_launch(fn, args.launches))
            one = {"index_agrees_with_torch": round(agree, 6), "same_skipped_waypoints": same_skips, "largest_cost_difference": cost_err,
                   "waypoints_solved": round(float(won.double().mean()), 4),
                   "pairs_blocked_mean_per_waypoint": round(float(pair["blocked"].double().mean()), 2),
                   "rows_differing_from_uncoupled": int((pair["index"] != alone["index"]).any(dim=0).sum())}
            for k, v in tm.items():
                one[f"{k}_us"] = round(float(np.median(v)), 1)
                one[f"{k}_us_min_max"] = [round(float(np.min(v)), 1), round(float(np.max(v)), 1)]
            med = {k: float(np.median(v)) for k, v in tm.items()}
            one["pair_over_composed"] = round(med["pair"] / med["composed"], 4)
            one["pair_over_uncoupled"] = round(med["pair"] / med["uncoupled"], 4)
            res[scene_name] = one
            del sweep_out, clr_res, pair, alone, picked, forms, sweep
            torch.cuda.empty_cache()
        out[f"robots_{robots}_T_{T}_K_{K}"] = res
    out["launches_per_median"] = args.launches * args.rounds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
