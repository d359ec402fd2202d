#!/usr/bin/env python3
"""Recorder of tests/golden/g19_start_theta.npz (TEST INFRASTRUCTURE — runs only where the reference is at hand).

Imports the real reference (pollen-robotics/reachy2_symbolic_ik, the way oracle/gen_golden.py does) and records what its
utils.get_best_theta_to_current_joints, tend_to_preferred_theta and get_best_continuous_theta2 return.  Numbers only.

    PYTHONDONTWRITEBYTECODE=1 python scripts/record_start_theta_golden.py --ref /path/to/reference/src [--out tests/golden]
    ... --check      regenerates and compares with the committed file

G19, per arm and for singularity_offset -1.01 and 0.03 ("so101", "so003"), 256 rows each:
    {arm}_{tag}_pos / _eul      the pose the arm is in (is_reachable_no_limits is called on it)
    {arm}_{tag}_cur             the joints it measured: +-0.6 as G7 draws them; every 8th row up to +-5 pi (angle_diff's wrap);
                                every 16th row within 1e-3 of the solution at the preferred theta (the shortcut)
    {arm}_{tag}_pref            the preferred theta handed over (four values per arm)
    {arm}_{tag}_theta           the returned theta
    {arm}_{tag}_low / _high     parsed from the returned text (NaN where it says "preferred_theta worked!")
The constructor's default arms-along-the-body pair is left out: it sits on an exact tie of the search (oracle/gen_golden.py, G7).
Rate limiter:
    tend_in [n,3] (previous_theta, d_theta_max, goal_theta), tend_ok [n], tend_theta [n]
    cont2_pos / cont2_eul / cont2_arm / cont2_so: the pose is_reachable is called on first; cont2_in [n,5] (previous_theta,
    interval 0 and 1 as is_reachable returned them, d_theta_max, preferred_theta), nb_search_points = 10;
    cont2_ok [n], cont2_theta [n], cont2_text [n] (0 nothing found, 1 "... ok et proche", 2 "... ok mais loin")
"""
import argparse
import contextlib
import io
import os
import re
import sys

import numpy as np

ARMS = ["r_arm", "l_arm"]
TAGS = (("so101", -1.01), ("so003", 0.03))
N_ROWS, N_TEND, N_CONT2 = 256, 240, 240
BASE = -4 * np.pi / 6
PREFS = {"r_arm": [BASE, BASE + 0.3, BASE - 0.5, 0.4], "l_arm": [-np.pi - BASE, -np.pi - BASE - 0.3, -np.pi - BASE + 0.5, 2.7]}
_NUM = r"([-+0-9.eE]+|nan|inf)"


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def start_rows(rng, arm, n):
    sgn = -1.0 if arm == "l_arm" else 1.0
    pos = np.array([0.38, -0.2, -0.1]) + rng.uniform(-0.22, 0.22, size=(n, 3))
    eul = np.array([0.0, -np.pi / 2, 0.0]) + rng.uniform(-0.7, 0.7, size=(n, 3))
    pos[:, 1] *= sgn
    eul[:, 0] *= sgn
    eul[:, 2] *= sgn
    cur = rng.uniform(-0.6, 0.6, size=(n, 7))
    far = np.arange(n) % 8 == 3
    cur[far] = rng.uniform(-5 * np.pi, 5 * np.pi, size=(int(far.sum()), 7))
    return pos, eul, cur


def generate(ref_src):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref_src)
    from reachy2_symbolic_ik import utils as U
    from reachy2_symbolic_ik.symbolic_ik import SymbolicIK

    rng = np.random.default_rng(19)
    data = {}
    for arm in ARMS:
        for tag, so in TAGS:
            solver = quiet(SymbolicIK, arm=arm, singularity_offset=so)
            pos, eul, cur = start_rows(rng, arm, N_ROWS)
            pref = np.array([PREFS[arm][i % 4] for i in range(N_ROWS)])
            theta, low, high = np.zeros(N_ROWS), np.full(N_ROWS, np.nan), np.full(N_ROWS, np.nan)
            for i in range(N_ROWS):
                pose = np.array([pos[i], eul[i]])
                if i % 16 == 5:  # a shortcut row: the joints of the preferred theta, nearly
                    ok, _, fn = solver.is_reachable_no_limits(pose)
                    assert ok
                    cur[i] = np.asarray(fn(pref[i])[0], dtype=float) + rng.uniform(-1e-3, 1e-3, size=7) + 2 * np.pi * (i % 32 == 5) * rng.integers(-2, 3, size=7)
                ok, _, fn = solver.is_reachable_no_limits(pose)
                assert ok
                theta[i], text = quiet(U.get_best_theta_to_current_joints, fn, 20, list(cur[i]), arm, pref[i])
                m = re.search(r"low = " + _NUM + r", high = " + _NUM, text)
                if m:
                    low[i], high[i] = float(m.group(1)), float(m.group(2))
                else:
                    assert text.startswith("preferred_theta worked!"), text
            pre = f"{arm}_{tag}_"
            data.update({pre + "pos": pos, pre + "eul": eul, pre + "cur": cur, pre + "pref": pref, pre + "theta": theta,
                         pre + "low": low, pre + "high": high})
    # tend_to_preferred_theta (utils.py:115-127)
    tin = np.stack([rng.uniform(-2 * np.pi, 2 * np.pi, N_TEND), rng.choice([0.01, 0.05, 0.5], N_TEND), rng.uniform(-2 * np.pi, 2 * np.pi, N_TEND)], axis=1)
    near = np.arange(N_TEND) % 3 == 0
    tin[near, 2] = tin[near, 0] + rng.uniform(-1.5, 1.5, int(near.sum())) * tin[near, 1] + 2 * np.pi * rng.integers(-1, 2, int(near.sum()))
    res = [U.tend_to_preferred_theta(a, np.array([-np.pi, np.pi]), None, d, g) for a, d, g in tin]
    data["tend_in"] = tin
    data["tend_ok"] = np.array([r[0] for r in res], dtype=np.uint8)
    data["tend_theta"] = np.array([float(r[1]) for r in res])
    # get_best_continuous_theta2 (utils.py:220-264) on the circle a fresh is_reachable leaves
    rows = {k: [] for k in ("pos", "eul", "arm", "so", "in", "ok", "theta", "text")}
    solvers = {(arm, so): quiet(SymbolicIK, arm=arm, singularity_offset=so) for arm in ARMS for _, so in TAGS}
    while len(rows["ok"]) < N_CONT2:
        k = len(rows["ok"])
        arm, so = ARMS[k % 2], TAGS[(k // 2) % 2][1]
        s = solvers[(arm, so)]
        pos, eul, _ = start_rows(rng, arm, 1)
        if k % 5 == 0:  # anywhere around the shoulder: narrow intervals, grids the elbow test empties
            pos = np.array([[0.0, 0.2 if arm == "l_arm" else -0.2, 0.0]]) + rng.uniform(-0.6, 0.6, size=(1, 3))
            eul = rng.uniform(-np.pi, np.pi, size=(1, 3))
        ok, interval, _, _ = quiet(s.is_reachable, np.array([pos[0], eul[0]]))
        if not ok:
            continue
        prev, dmax = rng.uniform(-np.pi, np.pi), float(rng.choice([0.01, 0.2, 3.0]))
        pref = PREFS[arm][0] if k % 3 else rng.uniform(-np.pi, np.pi)
        good, th, text = U.get_best_continuous_theta2(prev, interval, s.get_elbow_position, 10, dmax, pref, arm, so, 1.0, s.elbow_singularity_position)
        code = 2 if text.endswith("ok mais loin") else (1 if text.endswith("ok et proche") else 0)
        assert (code == 0) == (not good)
        for key, v in (("pos", pos[0]), ("eul", eul[0]), ("arm", k % 2), ("so", so), ("in", [prev, interval[0], interval[1], dmax, pref]),
                       ("ok", good), ("theta", float(th)), ("text", code)):
            rows[key].append(v)
    for key, v in rows.items():
        data["cont2_" + key] = np.array(v, dtype=np.uint8 if key in ("arm", "ok", "text") else np.float64)
    return data


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("RSIK_REFERENCE_SRC"), required="RSIK_REFERENCE_SRC" not in os.environ,
                    help="the src directory of a checkout of pollen-robotics/reachy2_symbolic_ik (or RSIK_REFERENCE_SRC)")
    ap.add_argument("--out", default=os.path.join(here, "..", "tests", "golden"))
    ap.add_argument("--check", action="store_true", help="regenerate and compare with the committed file")
    a = ap.parse_args()
    path = os.path.join(a.out, "g19_start_theta.npz")
    data = generate(a.ref)
    if a.check:
        old = np.load(path)
        assert sorted(old.files) == sorted(data), "different arrays"
        for k in data:
            assert np.array_equal(old[k], data[k], equal_nan=True), k
        print(f"{path}: {len(data)} arrays reproduced")
        return
    np.savez_compressed(path, **data)
    print(f"{path}: {os.path.getsize(path)} bytes; shortcut rows {int(sum(np.isnan(data[k]).sum() for k in data if k.endswith('_low')))}, "
          f"cont2 texts {np.bincount(data['cont2_text'], minlength=3).tolist()}, tend ok {int(data['tend_ok'].sum())}/{N_TEND}")


if __name__ == "__main__":
    main()
