"""Inputs and the NumPy reference of the rsik_clearance tests (tests/test_clearance_abi.py pins the reference on the CPU alone,
tests/test_gpu_clearance.py holds the device to it).  No test in this file.

The reference is independent of the device code.  The four link points (shoulder, elbow, wrist, goal origin), the joint axes and the
joint origins come from jacobian_workload._walk (walk() below restates its loop for another dtype, so that the same reference runs in
np.longdouble).  A link against a sphere is the point-to-segment distance; a link against a capsule is the smallest of five candidates:
each end point of either segment against the other segment, and the solution of the 2 x 2 normal equations where it is interior to
both.  clearance = distance - link radius - obstacle radius; `nearest` is the first minimum in the order (obstacle 0, link 0),
(obstacle 0, link 1), (obstacle 0, link 2), (obstacle 1, link 0) ...; the gradient is u . (a_k x (x - o_k)) for the joints below the
link."""
import functools

import numpy as np

import jacobian_workload as JW
from reachy2_symbolic_ik_amd import constants as K

N_SET = JW.N_SET
PAIRS = JW.PAIRS
SETS = ("uniform", "wound", "singular")
SCENES = ("open", "deep")
LINK_RADIUS = (0.03, 0.05, 0.04)   # (the forearm the thickest: next to the parallel capsule link 1 wins over its neighbours' ends)
PAR_DISTANCE = 0.15
WALL_RADIUS = 10.0
LINK_JOINTS = (2, 4, 7)     # joints 0 ... LINK_JOINTS[l] - 1 move link l
FD_H = 1e-6
PAR_ROW = 5                 # the row one capsule of every scene is parallel to (its link 1, with the row's byte of arm_bytes())
KEEP_RUNNER_UP = 1e-4       # the kept rows: the runner-up at least this far behind,
KEEP_AXIS_DISTANCE = 0.02   # the witness points at least this far apart
# The device bounds, max(1e-13, 16 x E) with E the largest |float64 - longdouble| of the reference over the finite rows of every pair,
# set and scene (measured by tests/test_clearance_abi.py::test_device_bounds_come_from_the_reference, which asserts that they still
# come out of the reference):
#   E_d, clearance:                 3.44e-15  ->  16 E_d = 5.5e-14: the floor of 1e-13 holds  (the deep scene's 10 m wall: ulp(10))
#   E_g, gradient on the kept rows: 1.68e-15  ->  16 E_g = 2.7e-14: the floor of 1e-13 holds
# The factor 16 is for the device's own sin, cos, sqrt and reciprocal, a few ulp from libm's; the chain is held to 1e-13 elsewhere.
E_CLEARANCE = 3.5e-15
E_GRADIENT = 1.7e-15
CLEARANCE_BOUND = max(1e-13, 16 * E_CLEARANCE)
GRADIENT_BOUND = max(1e-13, 16 * E_GRADIENT)
# The reference gradient against central differences of the reference clearance at h = 1e-6 on the kept rows: 10 x the largest
# difference seen over every pair, set and scene (2.19e-9, against the 10 m wall; tests/test_clearance_abi.py measures it again).
FD_OBSERVED = 2.2e-9
FD_BOUND = 10 * FD_OBSERVED


# ------------------------------------------------------------------------------------------ the chain
def walk(block, joints, dtype=np.float64):
    """jacobian_workload._walk, in `dtype`: (link points [n,4,3], joint axes [n,7,3], joint origins [n,7,3])."""
    if dtype is np.float64:
        p, _, axes, origins = JW._walk(block, joints)
    else:
        q = np.asarray(joints, dtype=dtype)
        n = len(q)
        R = np.tile(np.eye(3, dtype=dtype), (n, 1, 1))
        p = np.zeros((n, 3), dtype=dtype)
        axes, origins = np.zeros((n, 7, 3), dtype=dtype), np.zeros((n, 7, 3), dtype=dtype)
        for step in JW._chain(block):
            if step[0] == "T":
                p = p + R @ np.asarray(step[1], dtype=dtype)
            elif step[0] == "R":
                R = R @ np.asarray(step[1], dtype=dtype)
            else:
                _, k, axis = step
                axes[:, k], origins[:, k] = R @ np.asarray(axis, dtype=dtype), p
                R = R @ JW._rot(axis, q[:, k]).astype(dtype, copy=False)
    return np.stack([origins[:, 0], origins[:, 2], origins[:, 4], p], axis=1), axes, origins


# ------------------------------------------------------------------------------------------ distances
def _dot(a, b):
    return (a * b).sum(axis=-1)


def point_segment(C, P0, e):
    """The point of the segment P0 + s e, s in [0, 1], nearest to C (broadcast over leading axes): (s, squared distance)."""
    ee = _dot(e, e)
    ok = ee > 0
    s = np.where(ok, np.clip(_dot(C - P0, e) / np.where(ok, ee, 1), 0, 1), 0)
    v = P0 + s[..., None] * e - C
    return s, _dot(v, v)


def segment_segment(P0, e, Q0, f):
    """The nearest points of P0 + s e and Q0 + t f, s, t in [0, 1]: (s, t, squared distance), the smallest of five candidates."""
    one = np.ones(np.broadcast_shapes(P0.shape, Q0.shape)[:-1], dtype=np.result_type(P0, Q0))
    t1, d1 = point_segment(P0, Q0, f)
    t2, d2 = point_segment(P0 + e, Q0, f)
    s3, d3 = point_segment(Q0, P0, e)
    s4, d4 = point_segment(Q0 + f, P0, e)
    a, b, c = _dot(e, e), _dot(e, f), _dot(f, f)
    r = P0 - Q0
    er, fr = _dot(e, r), _dot(f, r)
    den = a * c - b * b
    ok = den > 1e-14 * a * c
    safe = np.where(ok, den, 1)
    s5, t5 = (b * fr - c * er) / safe, (a * fr - b * er) / safe
    ok = ok & (s5 >= 0) & (s5 <= 1) & (t5 >= 0) & (t5 <= 1)
    v5 = r + s5[..., None] * e - t5[..., None] * f
    d5 = np.where(ok, _dot(v5, v5), np.inf)
    S = np.stack([0 * one, one, s3 * one, s4 * one, np.where(ok, s5, 0)])
    Tt = np.stack([t1 * one, t2 * one, 0 * one, one, np.where(ok, t5, 0)])
    D = np.stack([d1 * one, d2 * one, d3 * one, d4 * one, d5 * one])
    best = np.argmin(D, axis=0)[None]
    return np.take_along_axis(S, best, 0)[0], np.take_along_axis(Tt, best, 0)[0], np.take_along_axis(D, best, 0)[0]


def usable(rows):
    """The obstacles that count: every entry finite and the radius (last entry) >= 0."""
    rows = np.asarray(rows)
    with np.errstate(invalid="ignore"):
        return np.isfinite(rows).all(axis=1) & (rows[:, -1] >= 0)


def pair_table(points, spheres, capsules, radius, dtype=np.float64, chunk=256):
    """Every (row, obstacle, link): clearance c [n, m, 3] (+inf where the obstacle is skipped), s and t [n, m, 3] of the witness."""
    radius = np.asarray(radius, dtype=dtype)
    P0, e = points[:, None, :3, :], (points[:, 1:] - points[:, :3])[:, None]
    n, m = len(points), len(spheres) + len(capsules)
    c, s, t = (np.full((n, m, 3), np.inf, dtype=dtype), np.zeros((n, m, 3), dtype=dtype), np.zeros((n, m, 3), dtype=dtype))
    sp, cp = np.asarray(spheres, dtype=dtype).reshape(-1, 4), np.asarray(capsules, dtype=dtype).reshape(-1, 7)
    ok_s, ok_c = usable(sp), usable(cp)
    for lo in range(0, len(sp), chunk):
        idx = lo + np.flatnonzero(ok_s[lo:lo + chunk])
        if len(idx):
            ss, d2 = point_segment(sp[idx, None, :3][None], P0, e)
            c[:, idx], s[:, idx] = np.sqrt(d2) - radius - sp[idx, 3][None, :, None], ss
    idx = np.flatnonzero(ok_c)
    if len(idx):
        Q0 = cp[idx, None, :3][None]
        ss, tt, d2 = segment_segment(P0, e, Q0, cp[idx, None, 3:6][None] - Q0)
        c[:, len(sp) + idx], s[:, len(sp) + idx], t[:, len(sp) + idx] = np.sqrt(d2) - radius - cp[idx, 6][None, :, None], ss, tt
    return c, s, t


def reference(blocks, joints, arm, scene, radius=LINK_RADIUS, dtype=np.float64, full=True):
    """The outputs of rsik_clearance for joints [n,7] and arm bytes [n] on the two constant blocks of a pair: clearance [n], nearest
    [n,2], and with `full` witness [n,2,3], gradient [n,7], link_points [n,4,3], pairs [n,m,3] (the clearance of every pair),
    runner_up [n] (the smallest clearance of another pair) and axis_distance [n] (|x - y|)."""
    q = np.asarray(joints, dtype=dtype)
    arm = np.asarray(arm)
    n = len(q)
    bad = ~np.isfinite(q).all(axis=1)
    q0 = np.where(bad[:, None], 0, q)
    points, axes, origins = (np.zeros((n, 4, 3), dtype=dtype), np.zeros((n, 7, 3), dtype=dtype), np.zeros((n, 7, 3), dtype=dtype))
    for side in (0, 1):
        rows = np.flatnonzero(arm == side)
        if len(rows):
            points[rows], axes[rows], origins[rows] = walk(blocks[side], q0[rows], dtype)
    spheres, capsules = scene["spheres"], scene["capsules"]
    c, s, t = pair_table(points, spheres, capsules, radius, dtype)
    m = c.shape[1]
    flat = c.reshape(n, m * 3)
    win = np.argmin(flat, axis=1)
    rows = np.arange(n)
    best = flat[rows, win]
    none = ~np.isfinite(best) | bad
    nearest = np.where(none[:, None], -1, np.stack([win % 3, win // 3], axis=1)).astype(np.int32)
    out = dict(clearance=np.where(bad, np.nan, best), nearest=nearest)
    if not full:
        return out
    link, obs = win % 3, win // 3
    x = points[rows, link] + s.reshape(n, -1)[rows, win][:, None] * (points[rows, link + 1] - points[rows, link])
    rows_of = np.concatenate([np.pad(np.asarray(spheres, dtype=dtype).reshape(-1, 4)[:, :3], ((0, 0), (0, 3))),
                              np.asarray(capsules, dtype=dtype).reshape(-1, 7)[:, :6]])
    rows_of[:len(spheres), 3:] = rows_of[:len(spheres), :3]
    a, b = rows_of[obs, :3], rows_of[obs, 3:]
    y = a + t.reshape(n, -1)[rows, win][:, None] * (b - a)
    v = x - y
    d = np.sqrt(_dot(v, v))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where((d > 0)[:, None], v / np.where(d > 0, d, 1)[:, None], 0)
    g = _dot(u[:, None, :], np.cross(axes, x[:, None, :] - origins))
    g = np.where(np.arange(7)[None, :] < np.asarray(LINK_JOINTS)[link][:, None], g, 0)
    others = flat.copy()
    others[rows, win] = np.inf
    nan = np.full((), np.nan, dtype=dtype)
    out.update(witness=np.where(none[:, None, None], nan, np.stack([x, y], axis=1)),
               gradient=np.where(bad[:, None], nan, np.where(none[:, None], 0, g)),
               link_points=np.where(bad[:, None, None], nan, points), pairs=c, runner_up=others.min(axis=1),
               axis_distance=np.where(none, nan, d))
    return out


# ------------------------------------------------------------------------------------------ scenes
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def parallel_capsule(pair):
    """[1,7]: the capsule parallel to link 1 (elbow -> wrist) of row PAR_ROW of the uniform set (with the row's byte of arm_bytes()),
    as long as the link, PAR_DISTANCE beside it on the side the neighbouring links bend away from, radius 0.02."""
    side = int(JW.arm_bytes()[PAR_ROW])
    pts, _, _ = walk(JW.blocks_of(pair)[side], JW.joint_set("uniform")[PAR_ROW:PAR_ROW + 1])
    e = pts[0, 2] - pts[0, 1]
    away = -((pts[0, 0] - pts[0, 1]) + (pts[0, 3] - pts[0, 2]))
    off = away - e * (away @ e) / (e @ e)
    off *= PAR_DISTANCE / np.linalg.norm(off)
    return np.concatenate([pts[0, 1] + off, pts[0, 2] + off, [0.02]])[None]


@functools.lru_cache(maxsize=None)
def scene(pair, name):
    """A seeded scene of a pair, dict(spheres [S,4], capsules [Cp,7], par: the index among the capsules of the parallel one):
    "open"  20 spheres and 6 capsules inside the arms' reach (centres 0.2 ... 0.6 m from a shoulder), radii 0.01 ... 0.08; one sphere
            twice (an exact tie); a sphere with a NaN, one at infinity, one with a negative radius and a capsule with a NaN (skipped);
            one capsule with a == b; one capsule parallel to link 1 of row PAR_ROW of the uniform set, 0.15 m beside it
    "deep"  the same, and in front of them a wall behind the robot: a sphere of 10 m whose surface passes 0.1 m in front of the
            shoulders, so that every row penetrates it, deepest with whatever point of the arm reaches furthest back"""
    blocks = JW.blocks_of(pair)
    rng = np.random.default_rng(7300 + PAIRS.index(pair))
    sh = [np.asarray(b[K.C_SHOULDER:K.C_SHOULDER + 3], dtype=np.float64) for b in blocks]

    def inside(k):
        d = rng.normal(size=(k, 3))
        return np.array(sh)[np.arange(k) % 2] + d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.2, 0.6, size=(k, 1))

    spheres = np.concatenate([inside(20), rng.uniform(0.01, 0.08, size=(20, 1))], axis=1)
    spheres = np.concatenate([spheres[:7], [[np.nan, 0.1, 0.1, 0.05]], spheres[7:13], [[np.inf, 0.0, 0.0, 0.05]], spheres[13:],
                              [[0.3, 0.0, 0.0, -0.01]], spheres[3:4]])
    a = inside(6)
    d = rng.normal(size=(6, 3))
    capsules = np.concatenate([a, a + d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.1, 0.3, size=(6, 1)),
                               rng.uniform(0.01, 0.08, size=(6, 1))], axis=1)
    capsules[2, 3:6] = capsules[2, :3]
    capsules = np.concatenate([capsules[:4], [[0.2, np.nan, 0.0, 0.3, 0.1, 0.0, 0.03]], capsules[4:], parallel_capsule(pair)])
    if name == "deep":
        centre = (sh[0] + sh[1]) / 2 - [WALL_RADIUS, 0.0, 0.0]
        spheres = np.concatenate([[np.concatenate([centre, [max(np.linalg.norm(s - centre) for s in sh) + 0.1]])], spheres])
    elif name == "parallel":  # the parallel capsule alone
        spheres, capsules = np.zeros((0, 4)), parallel_capsule(pair)
    elif name != "open":
        raise KeyError(name)
    return _frozen(dict(spheres=np.ascontiguousarray(spheres), capsules=np.ascontiguousarray(capsules), par=len(capsules) - 1))


def kind_arm(kind, n=N_SET):
    return {"r": np.zeros(n, dtype=np.uint8), "l": np.ones(n, dtype=np.uint8), "mixed": JW.arm_bytes()[:n]}[kind]


@functools.lru_cache(maxsize=None)
def case(pair, set_name, scene_name, kind="mixed"):
    """A named case, computed once and frozen: joints q [N_SET,7], arm [N_SET], the scene sc, the reference ref, the central
    differences fd [N_SET,7] of the reference clearance at h = FD_H and the kept rows keep [N_SET]: the same winner at q +- h in every
    joint, the runner-up at least KEEP_RUNNER_UP behind, |x - y| >= KEEP_AXIS_DISTANCE, and not the parallel pair."""
    blocks, q, arm, sc = JW.blocks_of(pair), JW.joint_set(set_name), kind_arm(kind), scene(pair, scene_name)
    ref = reference(blocks, q, arm, sc)
    same = np.ones(len(q), dtype=bool)
    fd = np.zeros((len(q), 7))
    for k in range(7):
        step = np.zeros(7)
        step[k] = FD_H
        plus, minus = (reference(blocks, q + sgn * step, arm, sc, full=False) for sgn in (1.0, -1.0))
        same &= (plus["nearest"] == ref["nearest"]).all(axis=1) & (minus["nearest"] == ref["nearest"]).all(axis=1)
        fd[:, k] = (plus["clearance"] - minus["clearance"]) / (2 * FD_H)
    parallel = (np.arange(len(q)) == PAR_ROW) & (ref["nearest"][:, 1] == len(sc["spheres"]) + sc["par"])
    keep = (same & (ref["runner_up"] - ref["clearance"] >= KEEP_RUNNER_UP) & (ref["axis_distance"] >= KEEP_AXIS_DISTANCE) & ~parallel)
    return _frozen(dict(q=q, arm=arm, sc=sc, ref=_frozen(ref), fd=fd, keep=keep))
