"""Inputs and the expected values of the rsik_solve_path_pair tests (tests/test_solve_path_pair_abi.py pins the helper on the checker
alone, tests/test_gpu_solve_path_pair.py uses it on the GPU).  No test in this file.

Rows: n = 2 robots; row 2i is the right arm of robot i, row 2i + 1 its left arm (arm bytes 0, 1, 0, 1, ...).  A state of the dynamic
programme is a pair (a, b): sample a of the right arm with sample b of the left.  The expected value is built with NumPy from a sweep's
outputs over the t * n poses (joints [K, t n, 7], projected [K, t n], reachable [t n]) and a table d [K][K][t][robots][2] of the two
views of every pair: d[a, b, t, i, 0] = dR(a, b), the right arm's clearance at JR[a] with the left arm at JL[b] as three capsules behind
the static scene, d[..., 1] = dL(a, b) the same with the arms exchanged — the library's own rsik_clearance on the GPU (the mask and the
penalty are then exact), track_pair_workload.clearance on the checker's sweep on the CPU.

The arithmetic is rsik.h's: p(a, b) = pR + pL; at the first solved waypoint A = (cR(start) + cL(start)) + p (p alone without a start);
later, over the candidate pairs of the previous solved waypoint, B(a, b') = min_b (A(a, b) + cL(b, b')), the lowest b among equal
values, and A'(a', b') = (min_a (B(a, b') + cR(a, a'))) + p(a', b'), the lowest a among equal values.  A backward table gives the least
cost of a path through every state and from it `gap`, the second-best distinct path minus the optimum."""
import itertools

import numpy as np

import clearance_workload as CW
import jacobian_workload as JW
import track_pair_workload as TP
from checker_support import reachable_rich
from nearest_workload import COST_TOL
from path_clear_workload import COST_SUM_MAX, HARD, SOFT, penalty  # noqa: F401
from path_workload import GAP, candidates, path_fractions, path_start, transition  # noqa: F401

PAIR = "default/default"
LINK_RADIUS = CW.LINK_RADIUS
# (T, K, seed, robots): 19 robots leave the last workgroup ragged; K = 16 fills all four states of a lane; K = 3 is no power of two;
# T = 70 gives the output pass a second, ragged trip
MAIN_SHAPES = ((12, 8, 11, 19), (6, 16, 21, 9), (70, 3, 31, 5))
SMALL_SHAPES = ((1, 8, 11, 5), (12, 1, 11, 5), (12, 8, 51, 1))  # (seed 51: the one robot has solved and partly blocked waypoints)
NO_SCENE = TP.NO_SCENE


def the_scene():
    return CW.scene(PAIR, "open")


def path_pair_tol(t):
    """(b): per waypoint two transitions each within COST_TOL, two exactly known penalties, and four roundings of sums below
    COST_SUM_MAX, each 1.4e-14 < COST_TOL: 6 T COST_TOL."""
    assert np.spacing(COST_SUM_MAX) / 2 < COST_TOL
    return 6 * t * COST_TOL


def pair_poses(seed, robots, t):
    """The path tests' interpolation for the rows 0, 1, 0, 1, ...: straight lines between reachable_rich(seed) and
    reachable_rich(seed + 1), position and Euler angles interpolated linearly over t waypoints.  pos [t,n,3], eul [t,n,3], arm [n]."""
    arm = TP.arm_bytes(robots)
    n = 2 * robots
    p0, e0 = reachable_rich(seed, n, arm)
    p1, e1 = reachable_rich(seed + 1, n, arm)
    s = (np.linspace(0.0, 1.0, t) if t > 1 else np.zeros(1))[:, None, None]
    return p0[None] + s * (p1 - p0)[None], e0[None] + s * (e1 - e0)[None], arm


def checker_pair_clearance(sweep_out, t, robots, scene=None, radius=LINK_RADIUS):
    """d [K][K][t][robots][2] of a sweep's joints by track_pair_workload.clearance: for every (a, b) the rows (JR[a], JL[b]) of every
    (waypoint, robot), each against the scene and its partner."""
    J = np.asarray(sweep_out["joints"])
    k = J.shape[0]
    J = J.reshape(k, t * robots, 2, 7)
    blocks = JW.blocks_of(PAIR)
    scene = NO_SCENE if scene is None else scene
    d = np.empty((k, k, t, robots, 2))
    for a in range(k):
        for b in range(k):
            rows = np.stack([J[a, :, 0], J[b, :, 1]], axis=1).reshape(2 * t * robots, 7)
            d[a, b] = TP.clearance(blocks, rows, scene, radius=radius, full=False)["clearance"].reshape(t, robots, 2)
    return d


def path_pair_dp(sweep_out, d, t, robots, min_clearance=-np.inf, influence=0.0, gain=0.0, start=None, weights=None, skip_projected=False):
    """What rsik_solve_path_pair must return.  Returns index [t,n] int32 (-1: skipped), cost [robots] (NaN: nothing solved), n_solved
    [robots] int32, step2 [t,n] (each arm's own transition cost into the waypoint along the optimum), blocked [t,robots] uint16,
    solved [t,robots], row [K,t,n] (the row candidates), pair [K,K,t,robots] (the candidate pairs), penalty [K,K,t,robots],
    through [K,K,t,robots] and gap [robots]."""
    n = 2 * robots
    J = np.asarray(sweep_out["joints"])
    K = J.shape[0]
    J = np.nan_to_num(J.reshape(K, t, n, 7))
    d = np.asarray(d, dtype=np.float64).reshape(K, K, t, robots, 2)
    row = candidates(sweep_out, t, n, skip_projected, None)
    if start is not None:  # a start row that is not finite loses the whole robot
        fine = np.isfinite(np.asarray(start)).all(axis=1).reshape(robots, 2).all(axis=1)
        row = row & np.repeat(fine, 2)[None, None]
    both = row[:, None, :, 0::2] & row[None, :, :, 1::2]  # [a, b, t, robots]
    with np.errstate(invalid="ignore"):
        ok = (d[..., 0] >= min_clearance) & (d[..., 1] >= min_clearance)  # (false for a NaN)
    pair = both & ok
    blocked = (both & ~ok).sum(axis=(0, 1)).astype(np.uint16)
    pen = penalty(d[..., 0], influence, gain) + penalty(d[..., 1], influence, gain)  # pR first, then one sum
    solved = pair.any(axis=(0, 1))  # [t, robots]
    inf = np.inf

    index = np.full((t, n), -1, dtype=np.int32)
    cost = np.full(robots, np.nan)
    step2 = np.full((t, n), np.nan)
    through = np.full((K, K, t, robots), inf)
    gap = np.full(robots, inf)
    for i in range(robots):
        ts = np.flatnonzero(solved[:, i])
        if not len(ts):
            continue
        JR, JL = J[:, :, 2 * i], J[:, :, 2 * i + 1]  # [K, t, 7]
        A = np.full((len(ts), K, K), inf)
        back = np.zeros((len(ts), K, K, 2), dtype=np.int64)
        cRs, cLs = [], []
        for m, s in enumerate(ts):
            cp, p = pair[:, :, s, i], pen[:, :, s, i]
            if m == 0:
                if start is None:
                    first = p
                else:
                    cR0 = transition(np.asarray(start)[2 * i][None], JR[:, s], weights)
                    cL0 = transition(np.asarray(start)[2 * i + 1][None], JL[:, s], weights)
                    first = (cR0[:, None] + cL0[None, :]) + p
                A[0] = np.where(cp, first, inf)
                cRs.append(None)
                cLs.append(None)
                continue
            sp = ts[m - 1]
            cL = transition(JL[:, None, sp], JL[None, :, s], weights)  # [b, b']
            cR = transition(JR[:, None, sp], JR[None, :, s], weights)  # [a, a']
            cRs.append(cR)
            cLs.append(cL)
            with np.errstate(invalid="ignore"):
                v1 = A[m - 1][:, :, None] + cL[None, :, :]  # [a, b, b']
            B1 = v1.min(axis=1)                             # [a, b']
            arg1 = v1.argmin(axis=1)                        # the lowest b among equal values
            with np.errstate(invalid="ignore"):
                v2 = B1[:, None, :] + cR[:, :, None]        # [a, a', b']
            best = v2.min(axis=0)                           # [a', b']
            arg2 = v2.argmin(axis=0)                        # the lowest a among equal values
            A[m] = np.where(cp, best + p, inf)
            back[m, :, :, 0] = arg2
            back[m, :, :, 1] = arg1[arg2, np.arange(K)[None, :]]
        end = int(np.argmin(A[-1].reshape(-1)))  # the lowest a K + b among equal values
        cost[i] = A[-1].reshape(-1)[end]
        a, b = divmod(end, K)
        for m in range(len(ts) - 1, -1, -1):
            index[ts[m], 2 * i], index[ts[m], 2 * i + 1] = a, b
            a, b = back[m, a, b]
        prev = None if start is None else np.asarray(start)[2 * i:2 * i + 2]
        for s in ts:
            rows = np.stack([JR[index[s, 2 * i], s], JL[index[s, 2 * i + 1], s]])
            step2[s, 2 * i:2 * i + 2] = 0.0 if prev is None else transition(prev, rows, weights)
            prev = rows
        # backward: W(a, b) = min over the next waypoint's candidate pairs of cR + cL + p' + W', 0 at the last solved waypoint
        W = np.where(pair[:, :, ts[-1], i], 0.0, inf)
        through[:, :, ts[-1], i] = A[-1] + W
        for m in range(len(ts) - 2, -1, -1):
            nxt = np.where(pair[:, :, ts[m + 1], i], pen[:, :, ts[m + 1], i] + W, inf)  # [a', b']
            tot = cRs[m + 1][:, None, :, None] + cLs[m + 1][None, :, None, :] + nxt[None, None]  # [a, b, a', b']
            W = np.where(pair[:, :, ts[m], i], tot.min(axis=(2, 3)), inf)
            through[:, :, ts[m], i] = A[m] + W
        others = through[:, :, :, i].copy()
        others[index[ts, 2 * i], index[ts, 2 * i + 1], ts] = inf
        gap[i] = others.min() - cost[i]
    gap = np.where(np.isnan(gap), inf, gap)
    return dict(index=index, cost=cost, n_solved=solved.sum(axis=0).astype(np.int32), step2=step2, blocked=blocked, solved=solved,
                row=row, pair=pair, penalty=pen, through=through, gap=gap)


def pair_cost_along(sweep_out, pen, index, t, robots, start=None, weights=None):
    """The cost, penalties included, of the path `index` [t,n] picks (-1: not there), in the device's order — first (cR + cL) + p, later
    ((sum + cL) + cR) + p —: total [robots] (NaN for an empty path) and step2 [t,n], the transitions alone.  pen: [K,K,t,robots]."""
    n = 2 * robots
    J = np.asarray(sweep_out["joints"])
    J = J.reshape(J.shape[0], t, n, 7)
    total = np.full(robots, np.nan)
    step2 = np.full((t, n), np.nan)
    for i in range(robots):
        prev = None if start is None else np.asarray(start)[2 * i:2 * i + 2]
        acc = None
        for s in range(t):
            a, b = index[s, 2 * i], index[s, 2 * i + 1]
            if a < 0 or b < 0:
                continue
            rows = np.stack([J[a, s, 2 * i], J[b, s, 2 * i + 1]])
            c = np.zeros(2) if prev is None else transition(prev, rows, weights)
            step2[s, 2 * i:2 * i + 2] = c
            if acc is None:
                acc = (c[0] + c[1]) + pen[a, b, s, i] if prev is not None else pen[a, b, s, i]
            else:
                acc = ((acc + c[1]) + c[0]) + pen[a, b, s, i]
            prev = rows
        if acc is not None:
            total[i] = acc
    return total, step2


def every_path(sweep_out, exp, i, t, robots, start=None, weights=None):
    """Every path of robot i through the candidate pairs of its solved waypoints, enumerated, each summed in pair_cost_along's order:
    the solved waypoints ts, the costs [P] ascending and the paths' states [P, len(ts), 2]."""
    pair, pen = exp["pair"], exp["penalty"]
    k = pair.shape[0]
    ts = np.flatnonzero(pair[:, :, :, i].any(axis=(0, 1)))
    if not len(ts):
        return ts, np.zeros(0), np.zeros((0, 0, 2), dtype=np.int64)
    J = np.nan_to_num(np.asarray(sweep_out["joints"]).reshape(k, t, 2 * robots, 7))
    states =[np.argwhere(pair[:, :, s, i]) for s in ts]
    picks = np.array(list(itertools.product(*[range(len(x)) for x in states])), dtype=np.int64).reshape(-1, len(ts))
    acc = prev_r = prev_l = None
    for m, s in enumerate(ts):
        ab = states[m][picks[:, m]]
        rows_r, rows_l = J[ab[:, 0], s, 2 * i], J[ab[:, 1], s, 2 * i + 1]
        p = pen[ab[:, 0], ab[:, 1], s, i]
        if m == 0:
            acc = p if start is None else (transition(np.asarray(start)[2 * i][None], rows_r, weights)
                                           + transition(np.asarray(start)[2 * i + 1][None], rows_l, weights)) + p
        else:
            acc = ((acc + transition(prev_l, rows_l, weights)) + transition(prev_r, rows_r, weights)) + p
        prev_r, prev_l = rows_r, rows_l
    order = np.argsort(acc, kind="stable")
    return ts, acc[order], np.stack([states[m][picks[order, m]] for m in range(len(ts))], axis=1)


def pair_gap_condition(exp, what="", seeded=True):
    """path_workload.gap_condition's rule for robots: every robot it counts (a solved waypoint; without start joints more than one, a
    single solved waypoint with no penalty being an exact tie) has a gap above GAP.  Returns the counted robots and the smallest gap."""
    has = exp["n_solved"] > (0 if seeded else 1)
    gaps = exp["gap"][has]
    print(f"{what}: {int(has.sum())} robots counted, smallest gap {float(gaps.min(initial=np.inf)):.3e}, "
          f"{float(exp['solved'].mean()):.2f} of the waypoints solved")
    return has, gaps
