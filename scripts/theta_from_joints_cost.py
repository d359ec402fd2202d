#!/usr/bin/env python3
"""Cost of rsik_theta_from_joints: time per launch at 262 144 and 1 Mi rows for each instantiation (uniform arm / an arm byte per
row, pose / matrix goals), against the only way to get the same answer for a batch without it — one
rsik_control_continuous_step with timed_out = 1 on every row and the same current poses and joints, which runs this search and
a control step on top of it — and beside rsik_solve's cost per row at the same n.  HIP events on the stream, the forms
interleaved in rounds in one process, medians.  Prints one JSON line.

    python scripts/theta_from_joints_cost.py [--launches 10] [--rounds 5]
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

from reachy2_symbolic_ik_amd import ControlIK  # noqa: E402
from reachy2_symbolic_ik_amd.control_ik import matrices_to_m12_soa  # noqa: E402
from tests.scale_inputs import matrices_from_pose  # noqa: E402


def time_launch(launch, k):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(k):
        launch()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / k  # us per launch


def rows(n, seed=1):
    """Start poses in front of the right shoulder (mirrored for the rows of the left arm) and measured joints in +-0.6."""
    rng = np.random.default_rng(seed)
    arm = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    pos = np.array([0.38, -0.2, -0.1]) + rng.uniform(-0.22, 0.22, size=(n, 3))
    eul = np.array([0.0, -np.pi / 2, 0.0]) + rng.uniform(-0.7, 0.7, size=(n, 3))
    return pos, eul, arm, rng.uniform(-0.6, 0.6, size=(n, 7))


def mirrored(pos, eul, arm):
    s = np.where(arm == 1, -1.0, 1.0)
    one = np.ones(len(arm))
    return pos * np.stack([one, s, one], axis=1), eul * np.stack([s, one, s], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        c = ControlIK(urdf_path="config_files/reachy2_ik_minimal.urdf")
    sv = c._solver
    pts = [c.preferred_theta["r_arm"], c.preferred_theta["l_arm"]]
    out = {}
    for n in (1 << 18, 1 << 20):
        pos, eul, arm, cur = rows(n)
        cj = torch.as_tensor(cur).to(dev)
        forms = {}
        for mixed in (False, True):
            p, e = mirrored(pos, eul, arm) if mixed else (pos, eul)
            arm_t = torch.as_tensor(arm).to(dev) if mixed else None
            pose = torch.as_tensor(np.ascontiguousarray(np.concatenate([p.T, e.T], axis=0))).to(dev)
            m12 = matrices_to_m12_soa(matrices_from_pose(p, e), dev)
            tag = "mixed" if mixed else "r"
            buf = {k: torch.empty(s, dtype=torch.float64, device=dev) for k, s in (("theta", (n,)), ("joints", (n, 7)), ("bracket", (n, 2)), ("distance", (n,)))}
            buf["state"] = torch.empty((n,), dtype=torch.uint8, device=dev)
            c._upload_arms()
            forms[f"theta_pose_{tag}"] = sv.theta_from_joints(pose, cj, pts, arm=arm_t, out=buf, plan_only=True)["launch"]
            forms[f"theta_m12_{tag}"] = sv.theta_from_joints(m12, cj, pts, arm=arm_t, out=buf, plan_only=True)["launch"]
            st = c.new_continuous_state(arm_t if mixed else "r_arm", n)
            ones = torch.ones(n, dtype=torch.uint8, device=dev)
            step_out = {"joints": torch.empty((n, 7), dtype=torch.float64, device=dev), "reachable": torch.empty(n, dtype=torch.uint8, device=dev),
                        "state": torch.empty(n, dtype=torch.uint8, device=dev)}
            forms[f"step_timed_out_{tag}"] = (lambda who=(arm_t if mixed else "r_arm"), m12=m12, st=st, ones=ones, step_out=step_out:
                                              c.symbolic_inverse_kinematics_continuous_batch(who, m12, st, timed_out=ones, current_joints=cj,
                                                                                             current_pose=m12, out=step_out))
            if not mixed:
                forms["solve_r"] = c.symbolic_ik_solver["r_arm"].solve_batch(pose, plan_only=True)["launch"]
        for f in forms.values():  # warm-up, settled clock
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, f in forms.items():
                t[k].append(time_launch(f, args.launches))
        med = {k: float(np.median(v)) for k, v in t.items()}
        res = {k: round(v, 1) for k, v in med.items()}
        for tag in ("r", "mixed"):
            for g in ("pose", "m12"):
                res[f"ratio_theta_{g}_{tag}_to_step"] = round(med[f"theta_{g}_{tag}"] / med[f"step_timed_out_{tag}"], 4)
        res["ns_per_row_theta_pose_r"] = round(med["theta_pose_r"] * 1e3 / n, 3)
        res["ns_per_row_solve_r"] = round(med["solve_r"] * 1e3 / n, 3)
        res["launches_per_median"] = args.launches * args.rounds
        out[f"n_{n}_us"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
