#!/usr/bin/env python3
"""Cost of rsik_track_avoid against the two things it stands between, on n trajectories of T goals (right arm).  Goals, starts and
gains are scripts/track_cost.py's (the device's own forward kinematics of a smooth joint path; lambda = 0.05, kp = ko = 20, dt = 0.01, no
feed-forward, no rest posture, no limits); the obstacles are seeded spheres and capsules 0.25 ... 0.7 m from the shoulder with radii of
2 ... 6 cm, link radii 0.05 / 0.04 / 0.03, influence 0.05 m, avoid_gain 20.
  avoid:     one rsik_track_avoid launch writing joints_steps [T,n,7];
  (a) track: one rsik_track launch on the same goals, writing the same: the difference is the price of avoidance per step;
  (b) composed: per step rsik_forward_kinematics, rsik_clearance (clearance and gradient), the pose error, the twist and the bias in torch,
             rsik_joint_rates with bias_rates, q + dt q' in torch, the step's joints stored into a [T,n,7] buffer.
Scenes: 16, 64 and 256 spheres, and 64 spheres + 64 capsules.  Shapes: 4096 x 1000 and 262 144 x 64.
Before anything is timed avoid and (b) must agree: the difference of the final joints is reported (median, maximum, rows above 1e-6
rad) and its median must stay below 1e-9 rad.  The two follow one definition, but where the nearest pair changes the gradient jumps, so
a trajectory that passes such a switch within the rounding of torch's arithmetic against the kernel's may part from its twin: the
maximum is reported, not asserted.
One process: untimed runs of every form first, then rounds with the forms alternating; HIP events on the stream around a window of
launches of avoid or (a) (as many as fill --track-window-s seconds) or one run of (b); median [min, max] of the rounds.  Prints one
JSON line.

    python scripts/track_avoid_cost.py [--shapes 4096x1000 262144x64] [--scenes 16+0 64+0 256+0 64+64] [--rounds 7] [--track-window-s 1.0]
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

from reachy2_symbolic_ik_amd import SymbolicIK  # noqa: E402
from track_cost import DT, KO, KP, LAMBDA, make_goals, timed  # noqa: E402

RADIUS = (0.05, 0.04, 0.03)
INFLUENCE, AVOID_GAIN = 0.05, 20.0
SHOULDER = np.array([0.0, -0.2, 0.0])


def make_scene(n_spheres, n_capsules, dev, seed=14):
    rng = np.random.default_rng(seed)

    def points(k):
        d = rng.normal(size=(k, 3))
        return SHOULDER + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.25, 0.7, size=(k, 1))

    sp = np.concatenate([points(n_spheres), rng.uniform(0.02, 0.06, size=(n_spheres, 1))], axis=1)
    a = points(n_capsules)
    d = rng.normal(size=(n_capsules, 3))
    cp = np.concatenate([a, a + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.1, 0.3, size=(n_capsules, 1)),
                         rng.uniform(0.02, 0.06, size=(n_capsules, 1))], axis=1)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(dev) if len(x) else None  # noqa: E731
    return t(sp), t(cp)


def composed_loop(sv, goals, start, out, spheres, capsules):
    """Form (b): the loop a caller of rsik_clearance and rsik_joint_rates runs, step by step."""
    T = goals.shape[0]
    one = torch.ones((), dtype=torch.float64, device=start.device)

    def run():
        q = start
        for t in range(T):
            p, R = sv.forward_kinematics(q)
            near = sv.clearance(q, spheres=spheres, capsules=capsules, link_radius=RADIUS, want=("clearance", "gradient"))
            Rg, pg = goals[t, :9].T.reshape(-1, 3, 3), goals[t, 9:].T
            D = Rg @ R.transpose(1, 2)
            w = 0.5 * torch.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], dim=1)
            s = w.norm(dim=1)
            angle = torch.atan2(s, 0.5 * (D.diagonal(dim1=1, dim2=2).sum(dim=1) - 1.0))
            big = s * s >= 2.0 ** -52
            e_o = w * torch.where(big, angle / torch.where(big, s, one), one)[:, None]
            v = torch.cat([KP * (pg - p), KO * e_o], dim=1)
            d = near["clearance"]
            push = d < INFLUENCE
            q0 = torch.where(push[:, None], (AVOID_GAIN * (INFLUENCE - d))[:, None] * near["gradient"], torch.zeros_like(q))
            q = q + DT * sv.joint_rates(q, v, damping=LAMBDA, bias_rates=q0)["rates"]
            out[t] = q
        return q

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["4096x1000", "262144x64"])
    ap.add_argument("--scenes", nargs="*", default=["16+0", "64+0", "256+0", "64+64"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--track-window-s", type=float, default=1.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", device=0)
    ik._upload()
    sv = ik.solver
    out = {"lambda": LAMBDA, "kp": KP, "ko": KO, "dt": DT, "influence": INFLUENCE, "avoid_gain": AVOID_GAIN, "rounds": args.rounds,
           "track_window_s": args.track_window_s}
    for shape in args.shapes:
        n, T = (int(x) for x in shape.split("x"))
        start = torch.as_tensor(np.random.default_rng(12).uniform(-1.5, 1.5, size=(n, 7))).to(dev)
        goals = make_goals(sv, start, T, seed=13)
        track = sv.track(goals, start, DT, KP, KO, damping=LAMBDA, want=("joints",), plan_only=True)
        loop_out = torch.empty((T, n, 7), dtype=torch.float64, device=dev)
        out[shape] = {}
        for scene in args.scenes:
            n_spheres, n_capsules = (int(x) for x in scene.split("+"))
            spheres, capsules = make_scene(n_spheres, n_capsules, dev)
            avoid = sv.track_avoid(goals, start, DT, KP, KO, damping=LAMBDA, spheres=spheres, capsules=capsules, link_radius=RADIUS,
                                   influence=INFLUENCE, avoid_gain=AVOID_GAIN, want=("joints", "clearance"), plan_only=True)
            forms = {"avoid": avoid["launch"], "track": track["launch"], "composed": composed_loop(sv, goals, start, loop_out, spheres, capsules)}
            for f in forms.values():  # untimed runs first: warm-up, settled clock
                for _ in range(2):
                    f()
            torch.cuda.synchronize()
            diff = (avoid["joints"][-1] - loop_out[-1]).abs().max(dim=1).values
            res = {"final_joints_median_diff": float(diff.median()), "final_joints_max_diff": float(diff.max()),
                   "rows_above_1e-6": int((diff > 1e-6).sum()), "all_finite": bool(torch.isfinite(avoid["joints"]).all()),
                   "pushed_share": round(float((avoid["clearance"] < INFLUENCE).double().mean()), 4)}
            assert res["all_finite"] and res["final_joints_median_diff"] < 1e-9, res
            launches = {k: max(1, int(np.ceil(args.track_window_s * 1e6 / timed(forms[k], 5)))) for k in ("avoid", "track")}
            res["launches_per_round"] = launches
            t = {k: [] for k in forms}
            for _ in range(args.rounds):
                for k, f in forms.items():
                    t[k].append(timed(f, launches.get(k, 1)))
            for k, x in t.items():
                res[f"{k}_us"] = round(float(np.median(x)), 1)
                res[f"{k}_us_min_max"] = [round(float(np.min(x)), 1), round(float(np.max(x)), 1)]
                res[f"{k}_us_per_step"] = round(res[f"{k}_us"] / T, 3)
            res["avoid_over_track"] = round(res["avoid_us"] / res["track_us"], 3)
            res["avoidance_us_per_step"] = round((res["avoid_us"] - res["track_us"]) / T, 3)
            res["composed_over_avoid"] = round(res["composed_us"] / res["avoid_us"], 2)
            out[shape][scene] = res
            del avoid, forms, spheres, capsules
        del track, goals, loop_out, start
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
