"""What the GPU tests of the sampling entry points (rsik_solve_sweep, rsik_solve_nearest, rsik_solve_path) share with the tests that
launch them on other arm pairs: the launches of their main cases and the comparison of a launch with the library's own sweep.  The
acceptance rules (a) - (d) / (a) - (c) are stated in tests/test_gpu_solve_nearest.py and tests/test_gpu_solve_path.py.  No test in this
file: pytest does not rewrite its asserts, so every one of them carries its own message."""
import numpy as np

import nearest_workload as NW
import path_workload as PW
from compare import as_bits, bits, same_bits
from gpu_support import T, abi, arm_kwargs, soa, to_np

# rsik_solve_sweep
PER_SAMPLE = ("joints", "elbow")
PER_POSE = ("interval", "reachable", "state")
# rsik_solve_nearest
LANES = (0, 1, 8, 64)  # RSIK_OPT_NEAREST_LANES: the library's choice, and each form forced
ROWS = ("index", "theta", "joints", "elbow", "cost", "projected", "interval", "reachable", "state")
# rsik_solve_path
PER_WAYPOINT = ("index", "theta", "joints", "elbow", "projected", "step_cost", "interval", "reachable", "state")
PER_PATH = ("cost", "n_solved")
ALL = PER_WAYPOINT + PER_PATH


# ------------------------------------------------------------------------------------------ rsik_solve_sweep
def solve_columns(solver, p, policy, th_cols, torch, prev=None, **arm_kw):
    """The reference the entry point is defined against: one rsik_solve (rsik_solve_rows with `prev`) per theta column."""
    outs = [to_np(solver.solve(p, theta_policy=abi().THETA_FRACTION if policy == "fraction" else abi().THETA_EXPLICIT,
                               theta_in=T(col, torch), previous_joints_rows=prev, **arm_kw)) for col in th_cols]
    ref = {key: np.stack([o[key] for o in outs]) for key in PER_SAMPLE}
    for key in PER_POSE:
        for o in outs[1:]:
            np.testing.assert_array_equal(o[key], outs[0][key])
        ref[key] = outs[0][key]
    return ref


def check_against_solve(got, ref, what):
    for key in PER_SAMPLE + PER_POSE:
        assert got[key].shape == ref[key].shape, (what, key, got[key].shape, ref[key].shape)
        if got[key].dtype == np.float64:
            same_bits(got[key], ref[key], f"{what} {key}")
        else:
            np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{what} {key}")


# ------------------------------------------------------------------------------------------ rsik_solve_nearest
def same_nearest_outputs(a, b, what, rows=None, keys=ROWS):
    for key in keys:
        x, y = (a[key], b[key]) if rows is None else (a[key][rows], b[key][rows])
        np.testing.assert_array_equal(as_bits(x), as_bits(y), err_msg=f"{what}: {key}")


def check_nearest(got, sw, seed, what, weights=None, skip=False, need_gap=False):
    """(a) - (d) for one launch `got` against the library's sweep `sw` of the same inputs."""
    exp = NW.nearest_from_sweep(sw, seed, weights, skip)
    if need_gap:
        NW.gap_condition(exp, sw["reachable"], what)  # the condition on the inputs, before anything is compared
    n = len(seed)
    idx = got["index"]
    assert idx.dtype == np.int32 and idx.shape == (n,), (what, idx.dtype, idx.shape)
    np.testing.assert_array_equal(idx == -1, exp["index"] == -1, err_msg=what + ": rows without a candidate")
    has = idx >= 0
    rows = np.flatnonzero(has)
    assert (idx[has] < sw["joints"].shape[0]).all(), (what, "index past K", int(idx.max(initial=-1)))
    # (a)
    for key in ("theta", "joints", "elbow"):
        np.testing.assert_array_equal(bits(got[key][rows]), bits(sw[key][idx[rows], rows]), err_msg=f"{what}: {key} is not the sweep's sample")
        assert np.isnan(got[key][~has]).all(), (what, key)
    np.testing.assert_array_equal(got["projected"][rows], sw["projected"][idx[rows], rows], err_msg=what + ": projected")
    assert (got["projected"][~has] == 0).all() and got["projected"].dtype == np.uint8, (what, "projected", got["projected"].dtype)
    # (b)
    masked = np.where(exp["candidate"], exp["c"], np.inf)
    c_won = masked[idx[rows], rows]
    c_min = exp["c_min"][rows]
    excess = c_won - c_min
    print(f"{what}: {len(rows)} winners, largest c - c_min {float(excess.max(initial=0.0)):.3e}")
    assert (c_won <= c_min + NW.COST_TOL * np.maximum(1.0, c_min)).all(), (what, float(excess.max(initial=0.0)))
    # (c)
    clear = has & (exp["gap"] > NW.GAP)
    np.testing.assert_array_equal(idx[clear], exp["index"][clear], err_msg=what + ": index where the gap is clear")
    # (d)
    err = np.abs(got["cost"][rows] - np.sqrt(c_won))
    print(f"{what}: largest |cost - sqrt(c)| {float(err.max(initial=0.0)):.3e}")
    assert (err <= NW.COST_TOL).all() and np.isnan(got["cost"][~has]).all(), (what, float(err.max(initial=0.0)))
    # the per-pose outputs of is_reachable
    for key in ("interval", "reachable", "state"):
        np.testing.assert_array_equal(as_bits(got[key]), as_bits(sw[key]), err_msg=f"{what}: {key}")
    ok = sw["reachable"].astype(bool)
    assert (idx[~ok] == -1).all(), (what, "an index on an unreachable row")
    return exp


def main_launches(torch, kind, k):
    """The launches of the main nearest tests for one (kind, K): what, poses, thetas, seed rows (device), the keyword arguments
    solve_sweep and solve_nearest share, seed rows (host)."""
    pos, eul, arm, seed = NW.main_case(kind, k)
    p = soa(pos, eul, torch)
    kw = arm_kwargs(kind, arm, torch)
    prev_rows = T(np.random.default_rng(40 + k).uniform(-2, 2, size=(NW.N_MAIN, 7)), torch)
    seedT = T(seed, torch)
    for policy in ("fraction", "explicit"):
        for per_pose in (False, True):
            th = T(NW.main_thetas(policy, per_pose, k), torch)
            for prev in (None, prev_rows):
                what = f"{kind} K {k} {policy} per_pose {per_pose} prev {prev is not None}"
                yield what, p, th, seedT, dict(policy=policy, previous_joints=prev, **kw), seed


# ------------------------------------------------------------------------------------------ rsik_solve_path
def path_soa(pos, eul, torch):
    """[T,n,3] x 2 -> SoA [6, T, n] on the device."""
    return torch.as_tensor(np.ascontiguousarray(np.concatenate([pos, eul], axis=2).transpose(2, 0, 1))).cuda()


def path_arm_kwargs(arm, torch):
    """The arm bytes of the paths as the wrapper takes them: one byte per path where any is the left arm, else the right arm for
    the launch (arm_kwargs decides by the arrangement's name and passes arm=None)."""
    return dict(arm=T(arm, torch)) if arm.any() else dict(arm_uniform=0)


def lib_sweep(solver, p, th, policy, arm, torch):
    """The library's sweep over the T * n poses of p [6,T,n]; thetas [K] or [K,T,n]; the arm byte of a path at each of its waypoints."""
    t, n = int(p.shape[1]), int(p.shape[2])
    th = th if th.dim() == 1 else th.reshape(th.shape[0], t * n)
    return to_np(solver.solve_sweep(p.reshape(6, t * n), th, policy=policy, **path_arm_kwargs(np.tile(arm, t), torch)))


def same_path_outputs(a, b, what, keys=ALL, paths=None, waypoints=None):
    for key in keys:
        x, y = a[key], b[key]
        if key in PER_WAYPOINT:
            if waypoints is not None:
                x, y = x[waypoints[0]], y[waypoints[1]]
            if paths is not None:
                x, y = x[:, paths], y[:, paths]
        elif paths is not None:
            x, y = x[paths], y[paths]
        np.testing.assert_array_equal(as_bits(x), as_bits(y), err_msg=f"{what}: {key}")


def check_path(got, sw, t, n, what, start=None, weights=None, skip=False, need_gap=False):
    """(a) - (c) for one launch `got` against the library's sweep `sw` over the same poses."""
    exp = PW.path_dp(sw, t, n, start, weights, skip)
    if need_gap:
        PW.gap_condition(exp, what, seeded=start is not None)  # the condition on the inputs, before anything is compared
    idx = got["index"]
    k = sw["joints"].shape[0]
    assert idx.dtype == np.int32 and idx.shape == (t, n) and got["n_solved"].dtype == np.int32, (what, idx.dtype, idx.shape, got["n_solved"].dtype)
    # (a)
    np.testing.assert_array_equal(idx == -1, ~exp["solved"], err_msg=what + ": the skipped waypoints")
    np.testing.assert_array_equal(got["n_solved"], exp["n_solved"], err_msg=what)
    assert (idx < k).all(), (what, "index past K", int(idx.max(initial=-1)))
    tt, ii = np.nonzero(idx >= 0)
    pose = tt * n + ii
    for key in ("theta", "joints", "elbow"):
        np.testing.assert_array_equal(bits(got[key][tt, ii]), bits(sw[key][idx[tt, ii], pose]), err_msg=f"{what}: {key} is not the sweep's sample")
        assert np.isnan(got[key][idx < 0]).all(), (what, key)
    np.testing.assert_array_equal(got["projected"][tt, ii], sw["projected"][idx[tt, ii], pose], err_msg=what + ": projected")
    assert (got["projected"][idx < 0] == 0).all() and got["projected"].dtype == np.uint8, (what, "projected", got["projected"].dtype)
    assert np.isnan(got["step_cost"][idx < 0]).all() and not np.isnan(got["step_cost"][idx >= 0]).any(), (what, "step_cost NaN pattern")
    for key in ("interval", "reachable", "state"):
        np.testing.assert_array_equal(as_bits(got[key].reshape((t * n,) + got[key].shape[2:])), as_bits(sw[key]), err_msg=f"{what}: {key}")
    # (b)
    tol = PW.path_tol(t)
    has = exp["n_solved"] > 0
    along, step2 = PW.cost_along(sw, idx, t, n, start, weights)
    excess = along[has] - exp["cost"][has]
    err_cost = np.abs(got["cost"][has] - along[has])
    err_steps = np.abs(np.nansum(got["step_cost"] ** 2, axis=0)[has] - along[has])
    print(f"{what}: {int(has.sum())} paths, device path - optimum in [{float(excess.min(initial=0.0)):.3e}, {float(excess.max(initial=0.0)):.3e}], "
          f"|cost - recomputed| {float(err_cost.max(initial=0.0)):.3e}, |sum step_cost^2 - recomputed| {float(err_steps.max(initial=0.0)):.3e}, tol {tol:.1e}")
    assert (np.abs(excess) <= tol).all(), (what, float(np.abs(excess).max(initial=0.0)))
    assert (err_cost <= tol).all() and np.isnan(got["cost"][~has]).all(), (what, float(err_cost.max(initial=0.0)))
    assert (err_steps <= tol).all(), (what, float(err_steps.max(initial=0.0)))
    # (c)  (without start joints a path with one solved waypoint is an exact tie at 0, the lowest sample's on both sides)
    clear = exp["gap"] > PW.GAP
    if start is None:
        clear = clear | (exp["n_solved"] == 1)
    np.testing.assert_array_equal(idx[:, clear], exp["index"][:, clear], err_msg=what + ": index where the gap is clear")
    return exp


def launches(torch, t, k, seed, kind, n=PW.N_MAIN):
    """The launches of the main path test for one shape: FRACTION with the shared grid and EXPLICIT with an angle per waypoint and
    sample, each with and without start joints."""
    pos, eul, arm = PW.path_poses(seed, n, t, kind)
    p = path_soa(pos, eul, torch)
    start = PW.path_start(seed, n)
    explicit = np.random.default_rng(seed + 200).uniform(-np.pi, np.pi, size=(k, t, n))
    for policy, th in (("fraction", PW.path_fractions(k)), ("explicit", explicit)):
        for st in (None, start):
            yield f"T {t} K {k} seed {seed} {kind} n {n} {policy} start {st is not None}", p, T(th, torch), policy, arm, st
