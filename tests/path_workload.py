"""Inputs and the expected values of the rsik_solve_path tests (tests/test_solve_path_abi.py pins the helper on the checker alone,
tests/test_gpu_solve_path.py uses it on the GPU).  No test in this file.

The entry point is defined against rsik_solve_sweep over the same n_steps * n poses (waypoint-major: pose t * n + i is waypoint t of
path i), so the expected value is built from a sweep's outputs (the library's own on the GPU, the checker's tiled batch on the CPU)
with NumPy: nearest_workload.costs' arithmetic for every transition, a forward table A and a backward table B.  A + B at (t, k) is
the cost of the best path through sample k of waypoint t; the smallest of them over k != the optimum's k is the second-best distinct
path, and `gap` is that minus the optimum."""
import numpy as np

from nearest_workload import COST_TOL, GAP  # noqa: F401  (nearest's derived per-cost bound, and its gap)
from checker_support import reachable_rich

N_MAIN = 37  # four paths per workgroup: ten workgroups, a ragged last one
# (T, K, seed, arm): 70 waypoints give the output pass a second, ragged trip of 64; K = 64 uses every lane
MAIN_SHAPES = ((12, 8, 11, "r"), (70, 3, 21, "mixed"), (5, 64, 31, "mixed"), (2, 8, 41, "r"))
# T = 1 and K = 1 on the seed-11 inputs, and a single path
SMALL_SHAPES = ((1, 8, 11, "r", N_MAIN), (12, 1, 11, "r", N_MAIN), (12, 8, 11, "r", 1))


def path_tol(t):
    """A path adds at most T costs, each within COST_TOL, and T roundings of the running sum."""
    return t * COST_TOL


def path_poses(seed, n, t, kind):
    """Straight lines between reachable_rich(seed) and reachable_rich(seed + 1): position and Euler angles interpolated linearly
    over t waypoints.  Returns pos [t,n,3], eul [t,n,3], arm [n] uint8 (mixed: default_rng(seed).integers(0, 2, n))."""
    arm = {"r": np.zeros(n, dtype=np.uint8), "l": np.ones(n, dtype=np.uint8),
           "mixed": np.random.default_rng(seed).integers(0, 2, n).astype(np.uint8)}[kind]
    p0, e0 = reachable_rich(seed, n, arm)
    p1, e1 = reachable_rich(seed + 1, n, arm)
    s = (np.linspace(0.0, 1.0, t) if t > 1 else np.zeros(1))[:, None, None]
    return p0[None] + s * (p1 - p0)[None], e0[None] + s * (e1 - e0)[None], arm


def path_fractions(k):
    return np.linspace(0.0, 1.0, k) if k > 1 else np.array([0.5])


def path_start(seed, n):
    """The joints each path starts from: uniform in [-2, 2]."""
    return np.random.default_rng(seed + 100).uniform(-2.0, 2.0, size=(n, 7))


def flat(a):
    """[t, n, ...] -> [t * n, ...]: the pose order of the sweep over the same poses."""
    a = np.asarray(a)
    return np.ascontiguousarray(a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:]))


def transition(a, b, weights=None):
    """c(a, b) = sum_q w_q d_q d_q, d_q = angle_diff(b_q, a_q), q = 0 ... 6 in that order: nearest_workload.costs' arithmetic, broadcast."""
    w = np.ones(7) if weights is None else np.asarray(weights, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = (b - a + np.pi) % (2 * np.pi) - np.pi
        c = np.zeros(d.shape[:-1])
        for q in range(7):
            c = c + (w[q] * d[..., q]) * d[..., q]
    return c


def candidates(sweep_out, t, n, skip_projected=False, start=None):
    """[K, t, n]: the pose is reachable, none of the joints is a NaN, the flag does not exclude it (rsik.h); none on a path whose
    start row is not finite."""
    j = np.asarray(sweep_out["joints"])
    k = j.shape[0]
    cand = (np.asarray(sweep_out["reachable"]).reshape(t, n) != 0)[None] & ~np.isnan(j).any(axis=-1).reshape(k, t, n)
    if skip_projected:
        cand = cand & (np.asarray(sweep_out["projected"]).reshape(k, t, n) == 0)
    if start is not None:
        cand = cand & np.isfinite(np.asarray(start)).all(axis=1)[None, None]
    return cand


def path_dp(sweep_out, t, n, start=None, weights=None, skip_projected=False):
    """What rsik_solve_path must return, from a sweep's outputs over the t * n poses (joints [K, t n, 7], projected [K, t n],
    reachable [t n]).  Returns index [t,n] int32 (-1: skipped), cost [n] (NaN: nothing solved), n_solved [n], step2 [t,n] (the
    transition cost into each waypoint along the optimum, NaN at a skipped one), candidate [K,t,n], through [K,t,n] (the least
    cost of a path through that sample, inf for none) and gap [n] (second-best distinct path minus the optimum, inf without one)."""
    J = np.asarray(sweep_out["joints"])
    K = J.shape[0]
    J = J.reshape(K, t, n, 7)
    cand = candidates(sweep_out, t, n, skip_projected, start)
    solved = cand.any(axis=0)  # [t, n]
    inf = np.inf

    def sweep_tables(order, first_cost, forward):
        """A (order = forward) or B (backward) [K,t,n] and the argmin tables; the state of the waypoint before is kept per path."""
        tab = np.full((K, t, n), inf)
        arg = np.full((K, t, n), -1, dtype=np.int64)
        have = np.zeros(n, dtype=bool)
        pj = np.zeros((K, n, 7))
        pa = np.full((K, n), inf)
        pc = np.zeros((K, n), dtype=bool)
        for s in order:
            c_here = cand[:, s]
            first = np.where(c_here, first_cost(J[:, s]), inf)
            if forward:  # forward: c(previous, this); tab[j] = min_i pa[i] + c(pj[i], J[j])
                trans = transition(pj[:, None], J[None, :, s], weights)  # [i, j, n]
            else:        # backward: c(this, next); tab[i] = min_j c(J[i], nj[j]) + pa[j]
                trans = transition(J[None, :, s], pj[:, None], weights)  # [j, i, n]: axis 0 is the other waypoint's sample
            with np.errstate(invalid="ignore"):
                total = pa[:, None] + trans
            total = np.where(pc[:, None] & c_here[None], total, inf)
            best = total.min(axis=0)
            which = total.argmin(axis=0)  # (the first of equal minima: the lowest sample of the other waypoint)
            here = np.where(have[None], best, first)
            tab[:, s] = np.where(solved[s][None], here, inf)
            arg[:, s] = np.where(have[None] & c_here & solved[s][None], which, -1)
            upd = solved[s]
            pj = np.where(upd[None, :, None], np.nan_to_num(J[:, s]), pj)
            pa = np.where(upd[None], tab[:, s], pa)
            pc = np.where(upd[None], c_here, pc)
            have = have | upd
        return tab, arg

    if start is None:
        a_first = lambda js: np.zeros(js.shape[:2])  # noqa: E731
    else:
        a_first = lambda js: transition(np.asarray(start)[None], js, weights)  # noqa: E731
    A, back = sweep_tables(list(range(t)), a_first, True)
    B, _ = sweep_tables(list(range(t - 1, -1, -1)), lambda js: np.zeros(js.shape[:2]), False)
    with np.errstate(invalid="ignore"):
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
    return dict(index=index, cost=cost, n_solved=solved.sum(axis=0).astype(np.int32), step2=step2, candidate=cand, through=through,
                gap=gap, solved=solved)


def cost_along(sweep_out, index, t, n, start=None, weights=None):
    """The cost of the path `index` [t,n] picks (-1: not there), recomputed from the sweep's joints: total [n] (NaN for an empty
    path) and step2 [t,n]."""
    J = np.asarray(sweep_out["joints"])
    J = J.reshape(J.shape[0], t, n, 7)
    total = np.full(n, np.nan)
    step2 = np.full((t, n), np.nan)
    for i in range(n):
        prev = None if start is None else np.asarray(start)[i]
        acc = None
        for s in range(t):
            if index[s, i] < 0:
                continue
            row = J[index[s, i], s, i]
            step2[s, i] = 0.0 if prev is None else transition(prev, row, weights)
            acc = step2[s, i] if acc is None else acc + step2[s, i]
            prev = row
        if acc is not None:
            total[i] = acc
    return total, step2


def greedy_chain(sweep_out, t, n, start=None, weights=None, skip_projected=False):
    """What t chained nearest calls give, each seeded with the winner before it (the first with `start`, or — without one — with
    zeros, its own cost not counted): index [t,n] and, through cost_along, its cost."""
    J = np.asarray(sweep_out["joints"])
    K = J.shape[0]
    J = J.reshape(K, t, n, 7)
    cand = candidates(sweep_out, t, n, skip_projected, start)
    index = np.full((t, n), -1, dtype=np.int32)
    seed = np.zeros((n, 7)) if start is None else np.asarray(start, dtype=np.float64).copy()
    for s in range(t):
        c = np.where(cand[:, s], transition(seed[None], J[:, s], weights), np.inf)
        has = cand[:, s].any(axis=0)
        k = c.argmin(axis=0)
        index[s, has] = k[has]
        seed[has] = J[k[has], s, has]
    return index


def gap_condition(expected, what="", seeded=True):
    """The condition on the inputs (not a measurement): at least 95 % of the paths with a solved waypoint have their optimum and
    their second-best distinct path more than GAP apart, so that on them the device's index must equal NumPy's exactly.  Without
    start joints a path with ONE solved waypoint costs exactly 0 through every candidate — a tie by definition, which the lowest
    sample wins on both sides —, so there the condition is on the paths with at least two solved waypoints."""
    has = expected["n_solved"] > (0 if seeded else 1)
    clear = expected["gap"][has] > GAP
    share = float(clear.mean()) if has.any() else 1.0
    print(f"{what}: {int(has.sum())} paths with {'a' if seeded else 'more than one'} solved waypoint, {share:.4f} of them with a gap above {GAP}; "
          f"{float(expected['solved'].mean()):.2f} of the waypoints solved, {int(expected['solved'].all(axis=0).sum())} paths whole")
    assert share >= 0.95, (what, share)
    return share
