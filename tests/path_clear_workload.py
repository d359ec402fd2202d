"""Inputs and the expected values of the rsik_solve_path_clear tests (tests/test_solve_path_clear_abi.py pins the helper on the checker
alone, tests/test_gpu_solve_path_clear.py uses it on the GPU).  No test in this file.

The entry point is rsik_solve_path with one more condition on a candidate and a node penalty, both functions of d, the clearance of a
sample's joints as rsik_clearance defines it.  The expected value is path_workload.path_dp's programme with both, from a sweep's
outputs and a table d [K, t n] — the library's own rsik_clearance over the library's own sweep joints on the GPU (the mask and the
penalty are then exact: no band around the threshold), clearance_workload.reference on the checker's tiled sweep on the CPU.

The arithmetic is rsik.h's: p = (gain u) u, u = influence - d where d < influence, else 0; at a path's first solved waypoint
A = c(start, J) + p (0 + p without a start row); later A(j) = (min_i (A(i) + c(J_prev[i], J[j]))) + p(j).  A forward table A and a
backward table B (B leaves the node's own penalty out, so that A + B counts it once) give the least cost of a path through every
sample, and `gap` as path_dp gives it."""
import numpy as np

import clearance_workload as CW
import jacobian_workload as JW
from path_workload import GAP, candidates, transition  # noqa: F401

PAIR = "default/default"
SCENE = "open"
HARD = (0.0, -np.inf)                   # min_clearance
SOFT = ((0.0, 0.0), (0.05, 100.0))      # (influence, clearance_gain)
COST_SUM_MAX = 128.0                    # (b): the running sum stays below this, so one of its roundings is below 2^-46 = 1.4e-14


def the_scene():
    return CW.scene(PAIR, SCENE)


def path_clear_tol(t):
    """(b): per waypoint one transition within COST_TOL and one exactly known penalty added to a running sum below COST_SUM_MAX,
    whose rounding (1.4e-14) is below COST_TOL: 2 T COST_TOL."""
    from nearest_workload import COST_TOL

    assert np.spacing(COST_SUM_MAX) / 2 < COST_TOL
    return 2 * t * COST_TOL


def penalty(d, influence, gain):
    """p = (gain u) u with u = influence - d where d < influence, 0 elsewhere (a NaN, +inf): a select, unfused, in that order."""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        u = influence - d
        return np.where(d < influence, (gain * u) * u, 0.0)


def checker_clearance(sweep_out, arm_rows, radius=CW.LINK_RADIUS, scene=None):
    """d [K, t n] of a sweep's joints [K, t n, 7] by clearance_workload.reference (NaN where the joints are not numbers); arm_rows
    [t n]: the arm byte of every pose."""
    j = np.asarray(sweep_out["joints"])
    k, rows = j.shape[:2]
    ref = CW.reference(JW.blocks_of(PAIR), j.reshape(k * rows, 7), np.tile(np.asarray(arm_rows), k), the_scene() if scene is None else scene,
                       radius, full=False)
    return ref["clearance"].reshape(k, rows)


def path_clear_dp(sweep_out, d, t, n, min_clearance=-np.inf, influence=0.0, gain=0.0, start=None, weights=None, skip_projected=False):
    """What rsik_solve_path_clear must return, from a sweep's outputs over the t * n poses and d [K, t n].  Returns index [t,n] int32
    (-1: skipped), cost [n] (penalties included; NaN: nothing solved), n_solved [n], step2 [t,n] (the transition cost alone into each
    waypoint along the optimum), blocked [t,n] uint8, solved [t,n], candidate [K,t,n], penalty [K,t,n], through [K,t,n] and gap [n]
    (second-best distinct path minus the optimum, inf without one)."""
    J = np.asarray(sweep_out["joints"])
    K = J.shape[0]
    J = np.nan_to_num(J.reshape(K, t, n, 7))  # (a row that is no candidate is never read: its NaN must not warn)
    d = np.asarray(d, dtype=np.float64).reshape(K, t, n)
    base = candidates(sweep_out, t, n, skip_projected, start)
    with np.errstate(invalid="ignore"):
        ok = d >= min_clearance  # (false for a NaN)
    cand = base & ok
    blocked = (base & ~ok).sum(axis=0).astype(np.uint8)
    p = penalty(d, influence, gain)
    solved = cand.any(axis=0)
    inf = np.inf

    # forward: A, and the argmin table
    A = np.full((K, t, n), inf)
    back = np.full((K, t, n), -1, dtype=np.int64)
    have = np.zeros(n, dtype=bool)
    pj, pa, pc = np.zeros((K, n, 7)), np.full((K, n), inf), np.zeros((K, n), dtype=bool)
    for s in range(t):
        here_c = cand[:, s]
        first = (np.zeros((K, n)) if start is None else transition(np.asarray(start)[None], J[:, s], weights)) + p[:, s]
        trans = transition(pj[:, None], J[None, :, s], weights)  # [i, j, n]
        total = np.where(pc[:, None] & here_c[None], pa[:, None] + trans, inf)
        best = total.min(axis=0) + p[:, s]  # the minimum first, then one more sum
        which = total.argmin(axis=0)        # (the first of equal minima: the lowest i)
        A[:, s] = np.where(here_c, np.where(have[None], best, first), inf)
        back[:, s] = np.where(have[None] & here_c, which, -1)
        upd = solved[s]
        pj = np.where(upd[None, :, None], J[:, s], pj)
        pa = np.where(upd[None], A[:, s], pa)
        pc = np.where(upd[None], here_c, pc)
        have = have | upd
    # backward: B(i) = min_j (c(J[i], J_next[j]) + (p_next(j) + B_next(j))), 0 at the last solved waypoint
    B = np.full((K, t, n), inf)
    have = np.zeros(n, dtype=bool)
    nj, nb, nc = np.zeros((K, n, 7)), np.full((K, n), inf), np.zeros((K, n), dtype=bool)
    for s in range(t - 1, -1, -1):
        here_c = cand[:, s]
        trans = transition(J[:, None, s], nj[None, :], weights)  # [i, j, n]
        total = np.where(here_c[:, None] & nc[None], trans + nb[None], inf)
        best = total.min(axis=1)
        B[:, s] = np.where(here_c, np.where(have[None], best, 0.0), inf)
        upd = solved[s]
        nj = np.where(upd[None, :, None], J[:, s], nj)
        nb = np.where(upd[None], B[:, s] + p[:, s], nb)
        nc = np.where(upd[None], here_c, nc)
        have = have | upd
    through = np.where(cand, A + B, inf)

    index = np.full((t, n), -1, dtype=np.int32)
    cost = np.full(n, np.nan)
    step2 = np.full((t, n), np.nan)
    for i in range(n):
        ts = np.flatnonzero(solved[:, i])
        if not len(ts):
            continue
        k = int(np.argmin(A[:, ts[-1], i]))
        cost[i] = A[k, ts[-1], i]
        for s in ts[::-1]:
            index[s, i] = k
            k = int(back[k, s, i])
        prev = None if start is None else np.asarray(start)[i]
        for s in ts:
            step2[s, i] = 0.0 if prev is None else transition(prev, J[index[s, i], s, i], weights)
            prev = J[index[s, i], s, i]
    others = through.copy()
    tt, ii = np.nonzero(index >= 0)
    others[index[tt, ii], tt, ii] = inf
    second = others.reshape(K * t, n).min(axis=0)
    with np.errstate(invalid="ignore"):
        gap = second - cost
    gap = np.where(np.isnan(gap), inf, gap)
    return dict(index=index, cost=cost, n_solved=solved.sum(axis=0).astype(np.int32), step2=step2, blocked=blocked, solved=solved,
                candidate=cand, base=base, penalty=p, through=through, gap=gap)


def clear_cost_along(sweep_out, pen, index, t, n, start=None, weights=None):
    """The cost, penalties included, of the path `index` [t,n] picks (-1: not there), in the device's order — (sum + transition) +
    penalty —: total [n] (NaN for an empty path) and step2 [t,n], the transitions alone.  pen: [K,t,n]."""
    J = np.asarray(sweep_out["joints"])
    J = J.reshape(J.shape[0], t, n, 7)
    total = np.full(n, np.nan)
    step2 = np.full((t, n), np.nan)
    for i in range(n):
        prev = None if start is None else np.asarray(start)[i]
        acc = None
        for s in range(t):
            k = index[s, i]
            if k < 0:
                continue
            row = J[k, s, i]
            step2[s, i] = 0.0 if prev is None else transition(prev, row, weights)
            acc = (step2[s, i] if acc is None else acc + step2[s, i]) + pen[k, s, i]
            prev = row
        if acc is not None:
            total[i] = acc
    return total, step2


TABLE_SHAPES = ((12, 8, 11), (70, 3, 21), (5, 64, 31))  # (T, K, seed) of the main shapes on which the conditions below are set


def input_conditions(con, free, what):
    """The conditions on the inputs (not measurements) for min_clearance = 0 on a shape of TABLE_SHAPES: `con` the expected value with
    the hard constraint, `free` path_workload.path_dp of the same sweep (same start row).  The share of the candidates that the
    constraint blocks is within [0.3, 0.8]; at least 20 waypoints rsik_solve_path solves are skipped; at least 20 solved waypoints
    have some but not all of their candidates blocked; at least 15 paths differ from the unconstrained optimum."""
    base = con["base"]
    share = float(con["blocked"].sum()) / max(int(base.sum()), 1)
    lost = int((free["solved"] & ~con["solved"]).sum())
    partial = int((con["solved"] & (con["blocked"] > 0)).sum())  # (solved: fewer blocked than candidates)
    differ = int((con["index"] != free["index"]).any(axis=0).sum())
    print(f"{what}: {share:.2f} of the candidates blocked, {lost} solved waypoints lost, {partial} solved waypoints partly blocked, "
          f"{differ} paths whose optimum differs from rsik_solve_path's")
    assert 0.3 <= share <= 0.8, (what, share)
    assert lost >= 20, (what, lost)
    assert partial >= 20, (what, partial)
    assert differ >= 15, (what, differ)
    return dict(share=share, lost=lost, partial=partial, differ=differ)


def soft_condition(off, on, what):
    """At least 5 paths whose optimum differs between clearance_gain 0 and 100 (same hard constraint, same start row)."""
    differ = int((off["index"] != on["index"]).any(axis=0).sum())
    print(f"{what}: the penalty changes the optimum on {differ} paths")
    assert differ >= 5, (what, differ)
    return differ
