"""The NumPy expected value of the rsik_clearance_edges tests (tests/test_clearance_edges_abi.py pins it on the checker alone,
tests/test_gpu_clearance_edges.py holds the device to it).  No test in this file.

The entry point is defined against rsik_clearance: an edge's samples q(s) are formed here in the order include/rsik.h fixes —
delta = angle_diff(b, a), s / S one division, then a product, then a sum, q(S) = b by a select — and d(s) is whatever `clearance_of`
returns for them: the library's own rsik_clearance on the GPU (then the comparison is bit for bit), clearance_workload.reference on
the CPU.  What is left is the fold over the samples (strictly less, then the lower s), the bound's formula and the fold over a path's
edges."""
import numpy as np

import clearance_workload as CW
import jacobian_workload as JW

PAIR = "default/default"
DIP = 1e-3            # an edge dips when its minimum lies more than this below both of its ends
FINE = 128            # the sub-steps the bound is held against on the CPU
BOUND_SLACK = 1e-9    # the bound is a statement about real numbers: d's own rounding (clearance_workload.CLEARANCE_BOUND, 1e-13) is far below this


def angle_diff(b, a):
    """utils.angle_diff(b, a) as path_workload.transition forms it."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(b) - np.asarray(a) + np.pi) % (2 * np.pi) - np.pi


def edges_of(joints, start=None):
    """The edges of joints [T,n,7] (a row with a NaN or an infinity is no waypoint) and an optional start [n,7]: wp [T,n] (row t is
    a waypoint of a path that is not lost), have_a [T,n] (the edge has a row to start from), a [T,n,7] (that row, zeros without)."""
    J = np.asarray(joints, dtype=np.float64)
    t, n = J.shape[:2]
    ok = np.isfinite(J).all(axis=2)
    if start is not None:
        start = np.asarray(start, dtype=np.float64)
        ok = ok & np.isfinite(start).all(axis=1)[None]  # a start row that is not numbers loses its path
    a = np.zeros((t, n, 7))
    have_a = np.zeros((t, n), dtype=bool)
    last = np.zeros((n, 7)) if start is None else np.where(np.isfinite(start).all(axis=1)[:, None], start, 0.0)
    have = np.zeros(n, dtype=bool) if start is None else np.isfinite(start).all(axis=1)
    for s in range(t):
        a[s], have_a[s] = last, have & ok[s]
        last = np.where(ok[s][:, None], J[s], last)
        have = have | ok[s]
    a[~have_a] = 0.0
    return ok, have_a, a


def samples(a, b, have_a, wp, n_sub, delta=None):
    """q [S+1, ..., 7] and valid [S+1, ...] of edges a -> b (any leading shape): q(s) = a + delta * (s / S) for s < S, q(S) = b; an
    edge without a row to start from has the one sample s = S.  delta: angle_diff(b, a) from elsewhere (the device's), or None."""
    b0 = np.where(wp[..., None], np.nan_to_num(np.asarray(b, dtype=np.float64), nan=0.0, posinf=0.0, neginf=0.0), 0.0)
    if delta is None:
        delta = angle_diff(b0, a)
    delta = np.where(have_a[..., None], delta, 0.0)
    q = np.empty((n_sub + 1,) + b0.shape)
    valid = np.zeros((n_sub + 1,) + b0.shape[:-1], dtype=bool)
    for s in range(n_sub):
        frac = np.float64(s) / np.float64(n_sub)
        step = delta * frac
        q[s] = a + step
        valid[s] = have_a
    q[n_sub], valid[n_sub] = b0, wp
    return q, valid, delta


def fold_samples(d, nearest, valid, wp):
    """edge_clearance, edge_sub, edge_nearest from d [S+1, ...], nearest [S+1, ..., 2] and valid: the least d over the valid samples,
    the lowest s that attains it (+inf everywhere: the edge's first s), that sample's pair; NaN, -1, (-1, -1) where wp is false."""
    dd = np.where(valid, d, np.inf)
    best = dd.min(axis=0)
    hit = valid & (dd == best[None])
    sub = np.argmax(hit, axis=0)  # (the first true)
    pair = np.take_along_axis(nearest, sub[None, ..., None], axis=0)[0]
    return (np.where(wp, best, np.nan), np.where(wp, sub, -1).astype(np.int32), np.where(wp[..., None], pair, -1).astype(np.int32))


def reach(blocks, arm):
    """R [n,7]: R_0 = R_1 = u + f + |tip|, R_2 = R_3 = f + |tip|, R_4 = R_5 = R_6 = |tip| of every path's arm."""
    rows = []
    for block in blocks:
        u, f, tip = JW.arm_lengths(block)
        rows.append([u + f + tip, u + f + tip, f + tip, f + tip, tip, tip, tip])
    return np.asarray(rows)[np.asarray(arm, dtype=np.int64)]


def bound(edge_clearance, delta, n_sub, R):
    """edge_bound = edge_clearance - 0.5 * (acc / S), acc = sum_k |delta_k| R_k, k = 0 ... 6 in order, unfused (delta: zeros on a
    one-sample edge).  R: [n,7], broadcast over the waypoints."""
    acc = np.zeros(delta.shape[:-1])
    for k in range(7):
        acc = acc + np.abs(delta[..., k]) * R[..., k]
    with np.errstate(invalid="ignore"):
        return edge_clearance - 0.5 * (acc / np.float64(n_sub))


def fold_paths(edge_clearance, edge_sub, edge_bound, min_clearance=-np.inf):
    """The per-path outputs from the per-edge ones [T,n]: path_clearance, path_edge [n,2] (t, s; the lowest t among equal values),
    path_bound, n_below, first_below; NaN, (-1, -1), NaN, 0, -1 for a path without a waypoint."""
    t, n = edge_clearance.shape
    pc, pb = np.full(n, np.nan), np.full(n, np.nan)
    pe = np.full((n, 2), -1, dtype=np.int32)
    nb, fb = np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    for i in range(n):
        ts = np.flatnonzero(edge_sub[:, i] >= 0)
        if not len(ts):
            continue
        c = edge_clearance[ts, i]
        k = int(np.argmin(c))  # (the first of equal minima)
        pc[i], pe[i], pb[i] = c[k], (ts[k], edge_sub[ts[k], i]), edge_bound[ts, i].min()
        low = ts[c < min_clearance]
        nb[i], fb[i] = len(low), (low[0] if len(low) else -1)
    return dict(path_clearance=pc, path_edge=pe, path_bound=pb, n_below=nb, first_below=fb)


def reference_clearance(arm, scene=None, radius=CW.LINK_RADIUS, chunk=32768):
    """clearance_of for expected(): clearance_workload.reference on the default arms, rows [m,7] with the path index of each."""
    sc = CW.scene(PAIR, "open") if scene is None else scene
    arm = np.asarray(arm)

    def clearance_of(q, path):
        outs = [CW.reference(JW.blocks_of(PAIR), q[lo:lo + chunk], arm[path[lo:lo + chunk]], sc, radius, full=False)
                for lo in range(0, len(q), chunk)]
        return np.concatenate([o["clearance"] for o in outs]), np.concatenate([o["nearest"] for o in outs])

    return clearance_of


def expected(joints, arm, n_sub, clearance_of, start=None, min_clearance=-np.inf, delta=None, blocks=None):
    """Every output of rsik_clearance_edges for joints [T,n,7], arm bytes [n] and d from clearance_of(q [m,7], path [m]) ->
    (clearance [m], nearest [m,2]); beside them wp, have_a, delta, the arm bytes and d [S+1,T,n] (+inf where there is no sample)."""
    J = np.asarray(joints, dtype=np.float64)
    t, n = J.shape[:2]
    wp, have_a, a = edges_of(J, start)
    q, valid, delta = samples(a, J, have_a, wp, n_sub, delta)
    path = np.broadcast_to(np.arange(n)[None, None], valid.shape)
    d = np.full(valid.shape, np.inf)
    near = np.full(valid.shape + (2,), -1, dtype=np.int32)
    if valid.any():
        d[valid], near[valid] = clearance_of(q[valid], path[valid])
    ec, es, en = fold_samples(d, near, valid, wp)
    eb = bound(ec, delta, n_sub, reach(JW.blocks_of(PAIR) if blocks is None else blocks, arm)[None])
    out = dict(edge_clearance=ec, edge_sub=es, edge_nearest=en, edge_bound=eb, wp=wp, have_a=have_a, delta=delta,
               d=np.where(valid, d, np.inf), valid=valid, arm=np.asarray(arm))
    out.update(fold_paths(ec, es, eb, min_clearance))
    return out


def dips(exp):
    """[T,n]: the edges whose minimum lies more than DIP below both of their ends (an edge with a row to start from)."""
    with np.errstate(invalid="ignore"):
        return exp["have_a"] & (exp["edge_clearance"] < np.minimum(exp["d"][0], exp["d"][-1]) - DIP)
