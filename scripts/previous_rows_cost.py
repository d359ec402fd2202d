#!/usr/bin/env python3
"""Cost of per-row previous joints: rsik_control_discrete against rsik_control_discrete_rows on config 3 (262 144 goal
matrices, 64-point grid; r only, then r / l mixed) and rsik_solve against rsik_solve_rows on config 2 (1 Mi poses), timed with HIP events in one
process, the two forms interleaved in rounds.  Prints one JSON line.

    python scripts/previous_rows_cost.py [--launches 200] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import make_config2_poses, make_config3_matrices  # noqa: E402
from reachy2_symbolic_ik_amd import ControlIK, SymbolicIK  # noqa: E402
from reachy2_symbolic_ik_amd.control_ik import matrices_to_m12_soa  # noqa: E402


def time_launch(launch, k):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(k):
        launch()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / k  # us per launch


def compare(a, b, k, rounds, warmup=50):
    for _ in range(warmup):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(time_launch(a, k))
        tb.append(time_launch(b, k))
    return float(np.median(ta)), float(np.median(tb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    out = {}

    n3 = 1 << 18
    M = make_config3_matrices(n3)
    c = ControlIK(urdf_path="config_files/reachy2_ik_minimal.urdf")
    c.nb_search_points = 64
    m12 = matrices_to_m12_soa(M, torch.device("cuda", 0))
    ps = torch.as_tensor(np.tile(c._previous_sol_2x7()[0], (n3, 1))).cuda()
    uni = c.symbolic_inverse_kinematics_batch("r_arm", m12, plan_only=True)
    rows = c.symbolic_inverse_kinematics_batch("r_arm", m12, previous_sol=ps, plan_only=True)
    u, r = compare(uni["launch"], rows["launch"], args.launches, args.rounds)
    out["config3_discrete_us"] = {"uniform": round(u, 2), "rows": round(r, 2), "ratio": round(r / u, 4)}
    arm = torch.as_tensor((rng.uniform(size=n3) < 0.5).astype(np.uint8)).cuda()
    ps2 = c._previous_sol_2x7()
    uni = c.symbolic_inverse_kinematics_batch(arm, m12, plan_only=True)
    rows = c.symbolic_inverse_kinematics_batch(arm, m12, previous_sol=torch.as_tensor(ps2[arm.cpu().numpy()]).cuda(), plan_only=True)
    u, r = compare(uni["launch"], rows["launch"], args.launches, args.rounds)
    out["config3_mixed_arms_discrete_us"] = {"uniform": round(u, 2), "rows": round(r, 2), "ratio": round(r / u, 4)}

    n2 = 1 << 20
    ik = SymbolicIK("r_arm")
    pos, eul = make_config2_poses(n2)
    poses = torch.as_tensor(np.ascontiguousarray(np.concatenate([pos.T, eul.T], axis=0))).cuda()
    pj = torch.as_tensor(rng.uniform(-2, 2, size=(n2, 7))).cuda()
    uni = ik.solve_batch(poses, plan_only=True)
    rows = ik.solve_batch(poses, previous_joints=pj, plan_only=True)
    u, r = compare(uni["launch"], rows["launch"], args.launches, args.rounds)
    out["config2_solve_us"] = {"uniform": round(u, 2), "rows": round(r, 2), "ratio": round(r / u, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
