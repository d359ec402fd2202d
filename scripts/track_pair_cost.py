#!/usr/bin/env python3
"""Cost of rsik_track_pair against the two things it stands between, on n_pairs robots of two arms and T goals per arm.  Goals, starts
and gains follow scripts/track_cost.py (the device's own forward kinematics of a smooth joint path, each arm on its own constants;
lambda = 0.05, kp = ko = 20, dt = 0.01, no feed-forward, no rest posture, no limits); rows are interleaved (2i the right arm of robot i,
2i + 1 its left arm); the static obstacles are scripts/track_avoid_cost.py's seeded spheres, link radii 0.05 / 0.04 / 0.03, influence
0.05 m, avoid_gain 20.
  pair:      one rsik_track_pair launch writing joints_steps [T,2 n_pairs,7];
  (a) avoid: one rsik_track_avoid launch from the same build on the same 2 n_pairs rows (arm bytes 0, 1, 0, 1, ...), the same spheres
             plus THREE STATIC capsules, writing the same: the yardstick, existing code doing the same number of pair tests per step;
             the difference is the price of the exchange and of forming the partner's capsules;
  (b) composed, at n_pairs = 256 x 64 steps only: what a caller has today.  Per step one rsik_clearance launch for the link_points of
             all rows, the partner's capsules formed in torch, then ONE rsik_clearance launch PER ROW (its obstacles are shared by
             every row of a launch, and every row has a partner of its own) for clearance and gradient, rsik_forward_kinematics, the
             pose error, the twist and the bias in torch, rsik_joint_rates with bias_rates, q + dt q' in torch.
Before (b) is timed its final joints are compared with pair's: the median and the maximum difference are reported, and `agree` says
whether the median is below 1e-9 rad (see scripts/track_avoid_cost.py on why single trajectories may part where the nearest pair
changes).
One process: untimed runs of every form first, then rounds with the forms alternating; HIP events on the stream around a window of
launches (as many as fill --track-window-s seconds) or one run of (b); median [min, max] of the rounds.  Prints one JSON line.

    python scripts/track_pair_cost.py [--shapes 2048x1000 131072x64] [--spheres 0 16 64] [--rounds 7] [--track-window-s 1.0]
                                      [--composed 256x64]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from reachy2_symbolic_ik_amd import DualArmIK  # noqa: E402
from track_avoid_cost import AVOID_GAIN, INFLUENCE, RADIUS, make_scene  # noqa: E402
from track_cost import DT, KO, KP, LAMBDA, timed  # noqa: E402


def make_pair_goals(sv, start, arm, T, seed):
    """track_cost.make_goals for rows of both arms: [T,12,n] goal matrices, the device's FK of the joint path."""
    n = len(start)
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda lo, hi: (lo + (hi - lo) * torch.rand((n, 7), generator=g, dtype=torch.float64)).to(start.device)  # noqa: E731
    delta, a, omega, phi = r(-0.05, 0.05), r(0.0, 0.1), r(0.05, 0.3), r(-np.pi, np.pi)
    goals = torch.empty((T, 12, n), dtype=torch.float64, device=start.device)
    chunk = max(1, (1 << 22) // n)
    for t0 in range(0, T, chunk):
        t = torch.arange(t0, min(t0 + chunk, T), dtype=torch.float64, device=start.device)[:, None, None]
        path = start + delta + a * torch.sin(omega * t + phi)  # [c,n,7]
        c = path.shape[0]
        p, R = sv.forward_kinematics(path.reshape(-1, 7), arm=arm.repeat(c))
        goals[t0:t0 + c, :9] = R.reshape(c, n, 9).permute(0, 2, 1)
        goals[t0:t0 + c, 9:] = p.reshape(c, n, 3).permute(0, 2, 1)
    return goals


def composed_loop(sv, goals, start, arm, out, spheres):
    """Form (b): the loop a caller of rsik_clearance and rsik_joint_rates runs for robots whose arms avoid each other."""
    T, n = goals.shape[0], len(start)
    dev = start.device
    one = torch.ones((), dtype=torch.float64, device=dev)
    far = torch.tensor([[9.0, 9.0, 9.0, 0.1]], dtype=torch.float64, device=dev)
    rad = torch.tensor(RADIUS, dtype=torch.float64, device=dev).reshape(1, 3, 1).expand(n, 3, 1)
    partner = torch.arange(n, device=dev) ^ 1
    d, grad = torch.empty((n,), dtype=torch.float64, device=dev), torch.empty((n, 7), dtype=torch.float64, device=dev)

    def run():
        q = start
        for t in range(T):
            lp = sv.clearance(q, spheres=far, arm=arm, want=("link_points",))["link_points"][partner]     # [n,4,3]: the partner's
            caps = torch.cat([lp[:, :3], lp[:, 1:], rad], dim=2).contiguous()                             # [n,3,7]
            for r in range(n):
                sv.clearance(q[r:r + 1], spheres=spheres, capsules=caps[r], link_radius=RADIUS, arm_uniform=r & 1, want=("clearance", "gradient"),
                             out={"clearance": d[r:r + 1], "gradient": grad[r:r + 1]})
            p, R = sv.forward_kinematics(q, arm=arm)
            Rg, pg = goals[t, :9].T.reshape(-1, 3, 3), goals[t, 9:].T
            D = Rg @ R.transpose(1, 2)
            w = 0.5 * torch.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], dim=1)
            s = w.norm(dim=1)
            angle = torch.atan2(s, 0.5 * (D.diagonal(dim1=1, dim2=2).sum(dim=1) - 1.0))
            big = s * s >= 2.0 ** -52
            e_o = w * torch.where(big, angle / torch.where(big, s, one), one)[:, None]
            v = torch.cat([KP * (pg - p), KO * e_o], dim=1)
            push = d < INFLUENCE
            q0 = torch.where(push[:, None], (AVOID_GAIN * (INFLUENCE - d))[:, None] * grad, torch.zeros_like(q))
            q = q + DT * sv.joint_rates(q, v, damping=LAMBDA, bias_rates=q0, arm=arm)["rates"]
            out[t] = q
        return q

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["2048x1000", "131072x64"])
    ap.add_argument("--spheres", nargs="*", type=int, default=[0, 16, 64])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--track-window-s", type=float, default=1.0)
    ap.add_argument("--composed", default="256x64", help="the shape form (b) is timed at, with the first of --spheres; '' leaves it out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        dual = DualArmIK(device=0)
    dual._upload()
    sv = dual.solver
    out = {"lambda": LAMBDA, "kp": KP, "ko": KO, "dt": DT, "influence": INFLUENCE, "avoid_gain": AVOID_GAIN, "rounds": args.rounds,
           "track_window_s": args.track_window_s}
    three = make_scene(0, 3, dev, seed=15)[1]  # (a)'s three static capsules in place of the partner's

    def inputs(n_pairs, T):
        n = 2 * n_pairs
        arm = (torch.arange(n, device=dev) & 1).to(torch.uint8)
        start = torch.as_tensor(np.random.default_rng(12).uniform(-1.5, 1.5, size=(n, 7))).to(dev)
        return arm, start, make_pair_goals(sv, start, arm, T, seed=13)

    def forms_of(arm, start, goals, spheres):
        kw = dict(damping=LAMBDA, spheres=spheres, link_radius=RADIUS, influence=INFLUENCE, avoid_gain=AVOID_GAIN, plan_only=True)
        pair = sv.track_pair(goals, start, DT, KP, KO, want=("joints", "clearance"), **kw)
        avoid = sv.track_avoid(goals, start, DT, KP, KO, capsules=three, arm=arm, want=("joints", "clearance"), **kw)
        return pair, avoid

    for shape in args.shapes:
        n_pairs, T = (int(x) for x in shape.split("x"))
        arm, start, goals = inputs(n_pairs, T)
        out[shape] = {}
        for n_spheres in args.spheres:
            spheres = make_scene(n_spheres, 0, dev)[0]
            pair, avoid = forms_of(arm, start, goals, spheres)
            forms = {"pair": pair["launch"], "avoid": avoid["launch"]}
            for f in forms.values():  # untimed runs first: warm-up, settled clock
                for _ in range(2):
                    f()
            torch.cuda.synchronize()
            res = {"all_finite": bool(torch.isfinite(pair["joints"]).all()),
                   "pushed_share": round(float((pair["clearance"] < INFLUENCE).double().mean()), 4)}
            assert res["all_finite"], res
            launches = {k: max(1, int(np.ceil(args.track_window_s * 1e6 / timed(f, 3)))) for k, f in forms.items()}
            res["launches_per_round"] = launches
            t = {k: [] for k in forms}
            for _ in range(args.rounds):
                for k, f in forms.items():
                    t[k].append(timed(f, launches[k]))
            for k, x in t.items():
                res[f"{k}_us"] = round(float(np.median(x)), 1)
                res[f"{k}_us_min_max"] = [round(float(np.min(x)), 1), round(float(np.max(x)), 1)]
                res[f"{k}_us_per_step"] = round(res[f"{k}_us"] / T, 3)
            res["pair_over_avoid"] = round(res["pair_us"] / res["avoid_us"], 3)
            out[shape][f"{n_spheres}+0"] = res
            del pair, avoid, forms, spheres
        del arm, start, goals
        torch.cuda.empty_cache()

    if args.composed:
        n_pairs, T = (int(x) for x in args.composed.split("x"))
        arm, start, goals = inputs(n_pairs, T)
        spheres = make_scene(args.spheres[0], 0, dev)[0]
        pair, _ = forms_of(arm, start, goals, spheres)
        loop_out = torch.empty((T, 2 * n_pairs, 7), dtype=torch.float64, device=dev)
        forms = {"pair": pair["launch"], "composed": composed_loop(sv, goals, start, arm, loop_out, spheres)}
        for f in forms.values():
            f()
        torch.cuda.synchronize()
        diff = (pair["joints"][-1] - loop_out[-1]).abs().max(dim=1).values
        res = {"spheres": args.spheres[0], "final_joints_median_diff": float(diff.median()), "final_joints_max_diff": float(diff.max()),
               "rows_above_1e-6": int((diff > 1e-6).sum())}
        res["agree"] = bool(res["final_joints_median_diff"] < 1e-9)
        k = max(1, int(np.ceil(args.track_window_s * 1e6 / timed(forms["pair"], 3))))
        t = {"pair": [timed(forms["pair"], k) for _ in range(args.rounds)], "composed": [timed(forms["composed"], 1) for _ in range(min(args.rounds, 3))]}
        for name, x in t.items():
            res[f"{name}_us"] = round(float(np.median(x)), 1)
            res[f"{name}_us_min_max"] = [round(float(np.min(x)), 1), round(float(np.max(x)), 1)]
        res["composed_over_pair"] = round(res["composed_us"] / res["pair_us"], 1)
        out["composed " + args.composed] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
