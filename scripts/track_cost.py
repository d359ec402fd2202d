#!/usr/bin/env python3
"""Cost of rsik_track against the loop it replaces, on n trajectories of T goals (right arm).  The goals are the device's own forward
kinematics of a smooth joint path, start + delta + a sin(omega t + phi) with |delta| <= 0.05, a <= 0.1, start uniform in
[-1.5, 1.5]^7; lambda = 0.05, kp = ko = 20, dt = 0.01, no feed-forward, no rest posture, no limits.
  (a) track:     one rsik_track launch writing joints_steps [T,n,7] (what the loop below leaves behind);
  (b) composed:  per step rsik_forward_kinematics, the pose error and the twist in torch (R_g R^T, its rotation vector, the gains),
                 rsik_joint_rates, q + dt q' in torch, the step's joints stored into a [T,n,7] buffer: two library launches and about
                 twenty torch kernels per step, the joints through memory between each of them.
Shapes: 4096 x 1000 (config 5's) and 262 144 x 64.
Before anything is timed the two must agree: the largest difference of the final joints is reported and must stay below 1e-6 rad
(both follow the same definition; they differ by the rounding of torch's arithmetic against the kernel's, carried through T steps).
One process: untimed runs of both forms first (code objects loaded, the clock settled), then rounds with the two forms alternating; HIP
events on the stream around a window of launches of (a) or one run of (b); median [min, max] of the rounds.  A single launch of (a)
is a millisecond or two, and a window of a fraction of a second measures the clock and the scheduler as much as the kernel: the
window of (a) is as many launches as fill --track-window-s seconds (counted from an untimed estimate, reported per shape as
track_launches_per_round and track_window_ms).  Prints one JSON line.

    python scripts/track_cost.py [--shapes 4096x1000 262144x64] [--rounds 7] [--track-window-s 1.0]
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

from reachy2_symbolic_ik_amd import SymbolicIK  # noqa: E402

LAMBDA, KP, KO, DT = 0.05, 20.0, 20.0, 0.01


def timed(fn, k):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(k):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / k  # us per call of `fn`


def make_goals(sv, start, T, seed):
    """[T,12,n] goal matrices: the device's FK of the joint path, in chunks of steps so that the path is never whole in memory."""
    n = len(start)
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda lo, hi: (lo + (hi - lo) * torch.rand((n, 7), generator=g, dtype=torch.float64)).to(start.device)  # noqa: E731
    delta, a, omega, phi = r(-0.05, 0.05), r(0.0, 0.1), r(0.05, 0.3), r(-np.pi, np.pi)
    goals = torch.empty((T, 12, n), dtype=torch.float64, device=start.device)
    chunk = max(1, (1 << 22) // n)
    for t0 in range(0, T, chunk):
        t = torch.arange(t0, min(t0 + chunk, T), dtype=torch.float64, device=start.device)[:, None, None]
        path = start + delta + a * torch.sin(omega * t + phi)  # [c,n,7]
        p, R = sv.forward_kinematics(path.reshape(-1, 7))
        c = path.shape[0]
        goals[t0:t0 + c, :9] = R.reshape(c, n, 9).permute(0, 2, 1)
        goals[t0:t0 + c, 9:] = p.reshape(c, n, 3).permute(0, 2, 1)
    return goals


def composed_loop(sv, goals, start, out):
    """Form (b): the loop a caller of rsik_joint_rates runs, step by step."""
    T = goals.shape[0]
    one = torch.ones((), dtype=torch.float64, device=start.device)

    def run():
        q = start
        for t in range(T):
            p, R = sv.forward_kinematics(q)
            Rg, pg = goals[t, :9].T.reshape(-1, 3, 3), goals[t, 9:].T
            D = Rg @ R.transpose(1, 2)
            w = 0.5 * torch.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], dim=1)
            s = w.norm(dim=1)
            angle = torch.atan2(s, 0.5 * (D.diagonal(dim1=1, dim2=2).sum(dim=1) - 1.0))
            big = s * s >= 2.0 ** -52
            e_o = w * torch.where(big, angle / torch.where(big, s, one), one)[:, None]
            v = torch.cat([KP * (pg - p), KO * e_o], dim=1)
            q = q + DT * sv.joint_rates(q, v, damping=LAMBDA)["rates"]
            out[t] = q
        return q

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["4096x1000", "262144x64"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--track-window-s", type=float, default=1.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", device=0)
    ik._upload()
    sv = ik.solver
    out = {"lambda": LAMBDA, "kp": KP, "ko": KO, "dt": DT, "rounds": args.rounds, "track_window_s": args.track_window_s}
    for shape in args.shapes:
        n, T = (int(x) for x in shape.split("x"))
        start = torch.as_tensor(np.random.default_rng(12).uniform(-1.5, 1.5, size=(n, 7))).to(dev)
        goals = make_goals(sv, start, T, seed=13)
        plan = sv.track(goals, start, DT, KP, KO, damping=LAMBDA, want=("joints",), plan_only=True)
        loop_out = torch.empty((T, n, 7), dtype=torch.float64, device=dev)
        forms = {"track": plan["launch"], "composed": composed_loop(sv, goals, start, loop_out)}
        for f in forms.values():  # untimed runs first: warm-up, settled clock
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        diff = (plan["joints"][-1] - loop_out[-1]).abs().max(dim=1).values
        res = {"final_joints_max_diff": float(diff.max()), "final_joints_median_diff": float(diff.median()),
               "all_finite": bool(torch.isfinite(plan["joints"]).all())}
        assert res["all_finite"] and res["final_joints_max_diff"] < 1e-6, res
        launches = max(1, int(np.ceil(args.track_window_s * 1e6 / timed(forms["track"], 5))))  # (untimed: it only sizes the window)
        res["track_launches_per_round"] = launches
        t = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, f in forms.items():
                t[k].append(timed(f, launches if k == "track" else 1))
        for k, x in t.items():
            res[f"{k}_us"] = round(float(np.median(x)), 1)
            res[f"{k}_us_min_max"] = [round(float(np.min(x)), 1), round(float(np.max(x)), 1)]
        res["track_window_ms"] = round(res["track_us"] * launches / 1e3, 1)
        res["track_us_per_step"] = round(res["track_us"] / T, 3)
        res["composed_us_per_step"] = round(res["composed_us"] / T, 3)
        res["composed_over_track"] = round(res["composed_us"] / res["track_us"], 2)
        res["track_ns_per_trajectory_step"] = round(res["track_us"] * 1e3 / (n * T), 4)
        out[shape] = res
        del plan, goals, loop_out, forms, start
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
