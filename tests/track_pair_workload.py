"""Inputs, the NumPy reference and the tolerances of the rsik_track_pair tests (tests/test_track_pair_abi.py pins them on the CPU alone,
tests/test_gpu_track_pair.py holds the device to them).  No test in this file: pytest does not rewrite its asserts, so every one of
them carries its own message.

Rows: n = 2 n_pairs; row 2i is the right arm of robot i, row 2i + 1 its left arm (arm_bytes: 0, 1, 0, 1, ...), and row r's partner is
row r ^ 1.

The reference is track_avoid_workload.one_step with step 4a's obstacle list extended, per row, by the partner's three links as
capsules: (P_l, P_{l+1}, radius_l) with P = clearance_workload.walk's link points at the partner's joints BEFORE the step, skipped
(clearance_workload.usable) where the partner's joints are not numbers.  clearance_workload.reference takes one scene for every row, so
clearance() below restates its winner for a list that differs from row to row: the static part of the pair table is
clearance_workload.pair_table's, the partner's part clearance_workload.segment_segment's, and what follows (first minimum, witness,
gradient, runner-up) is reference()'s line for line.  one_step() and run() are track_avoid_workload's with that clearance in place of
clearance_workload.reference (they form the clearance inside, so they cannot be called with another one); with the partner's rows NaN
the result is track_avoid_workload.run's bit for bit on the live rows, and with avoid_gain = 0 in the five outputs the two share, which
tests/test_track_pair_abi.py asserts.

Per-step tolerance: track_avoid_workload.step_tolerance, unchanged.  Its two clearance terms, CLEARANCE_BOUND and GRADIENT_BOUND, bound
what the device's clearance and gradient differ by from the reference's for obstacles that are GIVEN.  Here the partner's capsule is
not given: the device builds it from link points it computed itself.  Those are held to the same forward-kinematics bound as the
row's own link points (they are the same chain, evaluated by the neighbouring lane), and the measured E below is the float64
reference against the longdouble reference with BOTH arms' points in the respective precision, so it contains that term.
tests/test_track_pair_abi.py measures E on the joints the pair run visits — the clearance on every (row, step), the gradient on the
kept and pushed ones — and asserts that max(1e-13, 16 E) does not exceed CW.CLEARANCE_BOUND and CW.GRADIENT_BOUND; it does not
(measured: E_d 1.4e-16 ... 2.5e-16, E_g 8.9e-16 ... 1.3e-15 over the three pairs), so the bounds used are those two, as they stand.

Inputs are track_workload's own: TW.starts(), TW.goals_of(pair, T, arm) with the arm bytes 0, 1, 0, 1, ...  The seeded starts put
both arms of a robot at the same joints, each on its own block, so the partner is near: measured on the reference without
avoidance (129 pairs x 33 steps, lambda 0.05, no static scene) it is within AW.INFLUENCE of the row on 0.198 (default/default),
0.328 (custom/custom) and 0.202 (default/ztip) of the (step, pair) cells, so both sides of the select occur.

The crossing case (crossing_case): N_CROSS robots, each hand sent to a constant goal on the other side of the chest, so that the
unobstructed reference runs bring the two forearms through each other; see CROSS_GOAL."""
import functools

import numpy as np

import clearance_workload as CW
import jacobian_workload as JW
import track_avoid_workload as AW
import track_workload as TW

PAIRS = AW.PAIRS
LINK_RADIUS = AW.LINK_RADIUS
INFLUENCE = AW.INFLUENCE
AVOID_GAIN = AW.AVOID_GAIN
N_SEED, T_SEED = 129, 33   # the seeded pair run whose shares test_track_pair_abi.py asserts
# The per-step cases of the GPU test (N_STEP robots, T_STEP steps, both of TW.LAMBDAS): (static scene, influence, with feed-forward, rest
# and limits).  With the "open" scene the static obstacles are the nearest on more cells, and at AW.INFLUENCE the reference has a link of
# the partner's as the nearest on a kept and pushed cell on only 0.081 ... 0.098 of them (default/default, default/ztip), short of the 0.1
# the test asks for; at 0.05 it is 0.104 ... 0.295.  With the terms as well default/default stays at 0.068 there, so that case has none.
N_STEP, T_STEP = 33, 6
STEP_CASES = (("none", AW.INFLUENCE, False), ("none", AW.INFLUENCE, True), ("open", 0.05, False))
NO_SCENE = dict(spheres=np.zeros((0, 4)), capsules=np.zeros((0, 7)))
for _a in NO_SCENE.values():
    _a.setflags(write=False)


def _frozen(a):
    a.setflags(write=False)
    return a


def arm_bytes(n_pairs):
    """[2 n_pairs] uint8: 0, 1, 0, 1, ..."""
    return _frozen(np.tile(np.array([0, 1], dtype=np.uint8), n_pairs))


def partner_capsules(points, radius=LINK_RADIUS):
    """The three capsules [3,7] a row's partner is, from the partner's link points [4,3]: (P_l, P_{l+1}, radius_l).  What the GPU tests
    hand to rsik_clearance behind the static capsules."""
    points = np.asarray(points)
    return np.concatenate([points[:3], points[1:], np.asarray(radius, dtype=points.dtype)[:, None]], axis=1)


# ------------------------------------------------------------------------------------------ step 4a with the partner
def clearance(blocks, joints, scene, radius=LINK_RADIUS, dtype=np.float64, full=True):
    """clearance_workload.reference for rows 2i (r block) and 2i + 1 (l block) whose obstacles are the scene's followed by the partner's
    three links.  Same outputs; obstacle index S + Cp + l is the partner's link l."""
    q = np.asarray(joints, dtype=dtype)
    n = len(q)
    assert n % 2 == 0, n
    bad = ~np.isfinite(q).all(axis=1)
    q0 = np.where(bad[:, None], 0, q)
    points, axes, origins = (np.zeros((n, 4, 3), dtype=dtype), np.zeros((n, 7, 3), dtype=dtype), np.zeros((n, 7, 3), dtype=dtype))
    for side in (0, 1):
        points[side::2], axes[side::2], origins[side::2] = CW.walk(blocks[side], q0[side::2], dtype)
    spheres, capsules = scene["spheres"], scene["capsules"]
    rad = np.asarray(radius, dtype=dtype)
    c, s, t = CW.pair_table(points, spheres, capsules, radius, dtype)
    # the partner's links: row r against the points of row r ^ 1, skipped where those are not numbers
    other = np.arange(n) ^ 1
    pp = np.where(bad[other][:, None, None], np.full((), np.nan, dtype=dtype), points[other])
    P0, e = points[:, None, :3, :], (points[:, 1:] - points[:, :3])[:, None]
    Q0, f = pp[:, :3, None, :], (pp[:, 1:] - pp[:, :3])[:, :, None, :]
    ok = ~bad[other]
    cp_, sp_, tp_ = (np.full((n, 3, 3), np.inf, dtype=dtype), np.zeros((n, 3, 3), dtype=dtype), np.zeros((n, 3, 3), dtype=dtype))
    if ok.any():
        ss, tt, d2 = CW.segment_segment(P0[ok], e[ok], Q0[ok], f[ok])
        cp_[ok], sp_[ok], tp_[ok] = np.sqrt(d2) - rad[None, None, :] - rad[None, :, None], ss, tt
    m_static = c.shape[1]
    c, s, t = np.concatenate([c, cp_], axis=1), np.concatenate([s, sp_], axis=1), np.concatenate([t, tp_], axis=1)
    # from here on clearance_workload.reference's lines
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
    static = obs < m_static
    lp = np.where(static, 0, obs - m_static)
    ends = np.where(static[:, None], rows_of[np.where(static, obs, 0)] if m_static else 0, np.concatenate([pp[rows, lp], pp[rows, lp + 1]], axis=1))
    a, b = ends[:, :3], ends[:, 3:]
    y = a + t.reshape(n, -1)[rows, win][:, None] * (b - a)
    v = x - y
    d = np.sqrt(CW._dot(v, v))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where((d > 0)[:, None], v / np.where(d > 0, d, 1)[:, None], 0)
    g = CW._dot(u[:, None, :], np.cross(axes, x[:, None, :] - origins))
    g = np.where(np.arange(7)[None, :] < np.asarray(CW.LINK_JOINTS)[link][:, None], g, 0)
    others = flat.copy()
    others[rows, win] = np.inf
    nan = np.full((), np.nan, dtype=dtype)
    out.update(witness=np.where(none[:, None, None], nan, np.stack([x, y], axis=1)),
               gradient=np.where(bad[:, None], nan, np.where(none[:, None], 0, g)),
               link_points=np.where(bad[:, None, None], nan, points), pairs=c, runner_up=others.min(axis=1),
               axis_distance=np.where(none, nan, d))
    return out


# ------------------------------------------------------------------------------------------ one step, and a run
def one_step(pair, q, goal_R, goal_p, lam, scene, influence=INFLUENCE, avoid_gain=AVOID_GAIN, radius=LINK_RADIUS, dt=TW.DT, kp=TW.KP,
             ko=TW.KO, ff=None, rest=None, rest_gain=0.0, limits=None, solver="lstsq"):
    """track_avoid_workload.one_step for rows 0, 1, 0, 1, ... with clearance() above as step 4a: the same dict."""
    q = np.asarray(q, dtype=np.float64)
    n = len(q)
    arm = arm_bytes(n // 2)
    blocks = JW.blocks_of(pair)
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (n,))
    skip = ~(np.isfinite(goal_R).all(axis=(1, 2)) & np.isfinite(goal_p).all(axis=1))
    if ff is not None:
        skip |= ~np.isfinite(ff).all(axis=1)
    gR, gp = np.where(skip[:, None, None], np.eye(3), goal_R), np.where(skip[:, None], 0.0, goal_p)
    # 4a
    c = clearance(blocks, q, scene, radius=radius)
    d, g = c["clearance"], c["gradient"]
    with np.errstate(invalid="ignore"):
        push = d < influence                                   # (False for +inf and for NaN)
    a = avoid_gain * (influence - np.where(push, d, influence))
    with np.errstate(over="ignore", invalid="ignore"):
        chain = TW.by_arm(blocks, arm, lambda block, rows: dict(zip(("e_p", "e_o", "err"), TW.pose_error(block, q[rows], gR[rows], gp[rows])),
                                                              J=JW.jacobian(block, q[rows])))
        e_p, e_o, err, J = chain["e_p"], chain["e_o"], chain["err"], chain["J"]
        v = np.concatenate([kp * e_p, ko * e_o], axis=1)
        if ff is not None:
            v = np.where(skip[:, None], 0.0, ff) + v
        # 4b
        q0 = np.zeros((n, 7)) if rest is None else rest_gain * (rest - q)
        q0 = np.where(push[:, None], q0 + a[:, None] * g, q0)
        solvable = np.isfinite(v).all(axis=1) & np.isfinite(q0).all(axis=1)
        rates = np.full((n, 7), np.nan)
        if solvable.any():
            rates[solvable] = TW._rates(J[solvable], v[solvable], lam[solvable], q0[solvable], solver)
        overflow = ~skip & ~np.isfinite(rates).all(axis=1)
        held = skip | overflow
        m = np.ones(n)
        if limits is not None:
            m = np.where(held, 1.0, np.maximum((np.abs(rates) / limits[0]).max(axis=1), 1.0))
            rates = np.where((m > 1.0)[:, None], rates / m[:, None], rates)
        moved_q = q + dt * rates
    if limits is not None:
        moved_q = np.minimum(np.maximum(moved_q, limits[1]), limits[2])
    return dict(joints=np.where(held[:, None], q, moved_q), rates=np.where(held[:, None], 0.0, rates), err=np.where(held[:, None], np.nan, err),
                clearance=d, nearest=c["nearest"], gradient=g, push=push, a=a, J=J, v=v, q0=q0, skip=skip, overflow=overflow, m=m,
                runner_up=c["runner_up"], axis_distance=c["axis_distance"])


def run(pair, start, goals_R, goals_p, lam, scene, solver="lstsq", **terms):
    """track_avoid_workload.run with one_step() above: the same dict, and partner [T,n]: the nearest obstacle is a link of the
    partner's."""
    T = len(goals_R)
    ff = terms.pop("ff", None)
    q = np.asarray(start, dtype=np.float64)
    n = len(q)
    out = dict(joints=np.empty((T, n, 7)), rates=np.empty((T, n, 7)), err=np.empty((T, n, 2)), clearance=np.empty((T, n)),
               push=np.empty((T, n), dtype=bool), keep=np.empty((T, n), dtype=bool), nearest=np.empty((T, n, 2), dtype=np.int32))
    influence = terms.get("influence", INFLUENCE)
    for t in range(T):
        s = one_step(pair, q, goals_R[t], goals_p[t], lam, scene, ff=None if ff is None else ff[t], solver=solver, **terms)
        for k in ("joints", "rates", "err", "clearance", "push", "nearest"):
            out[k][t] = s[k]
        out["keep"][t] = AW.kept(s, influence)
        q = s["joints"]
    out["final_joints"] = q
    blocks, arm = JW.blocks_of(pair), arm_bytes(n // 2)
    out["final_err"] = TW.by_arm(blocks, arm, lambda block, rows: dict(e=TW.pose_error(block, q[rows], goals_R[-1][rows], goals_p[-1][rows])[2]))["e"]
    bad_goal = ~(np.isfinite(goals_R[-1]).all(axis=(1, 2)) & np.isfinite(goals_p[-1]).all(axis=1))
    out["final_err"][bad_goal] = np.nan
    last = clearance(blocks, q, scene, radius=terms.get("radius", LINK_RADIUS), full=False)["clearance"]
    out["min_clearance"] = np.minimum(out["clearance"].min(axis=0), last)
    out["partner"] = out["nearest"][:, :, 1] >= len(scene["spheres"]) + len(scene["capsules"])
    return out


# ------------------------------------------------------------------------------------------ seeded cases
def scene_of(pair, name):
    """A static scene by name: "none", "sphere" (the first sphere of the "open" scene), "open" (clearance_workload's), "full"
    (track_avoid_workload.full_scene)."""
    if name == "none":
        return NO_SCENE
    if name == "full":
        return AW.full_scene(pair)
    sc = CW.scene(pair, "open")
    return dict(spheres=sc["spheres"][:1], capsules=sc["capsules"][:0]) if name == "sphere" else sc


def inputs(pair, n_pairs, n_steps, with_terms):
    """track_avoid_workload.inputs for the rows 0, 1, 0, 1, ... of n_pairs robots."""
    return AW.inputs(pair, 2 * n_pairs, n_steps, arm_bytes(n_pairs), with_terms)


@functools.lru_cache(maxsize=None)
def seeded_run(pair, influence=INFLUENCE):
    """The seeded pair run without a static scene (N_SEED robots, T_SEED steps, lambda 0.05, no further terms, restatement rates):
    run()'s dict, frozen."""
    d = inputs(pair, N_SEED, T_SEED, False)
    out = run(pair, d["start"], d["R"], d["p"], 0.05, NO_SCENE, solver="restatement", influence=influence)
    return {k: _frozen(a) for k, a in out.items()}


# ------------------------------------------------------------------------------------------ the crossing case
# N_CROSS robots.  The goals are FK of CROSS_GOAL (+-0.03 rad of seeded noise per entry), each arm on its own block: arms folded in
# front of the chest, the right wrist on the left side and above its elbow, the left wrist on the right side and below its elbow, so
# that the two forearms form an X whose axes pass 2.5 cm from each other (on the default arms, without the noise) while each hand
# stays 0.2 m from the other arm.  Found by a seeded random search over joint space for exactly those properties.  The arms start
# opened outwards by CROSS_OPEN (shoulder pitch and roll) from there.  Without avoidance the forearms end up through each other (the
# reference's min_clearance is about -(r_1 + r_1) = -0.1 on every robot); what can separate them with the hands at their goals is the
# elbows' swivel, which is the null space the push acts in.  As in AW.elbow_case the approach is slow and the push strong, so that the
# case is about the push.
N_CROSS, T_CROSS = 64, 64
CROSS_KP = 10.0
CROSS_GAIN = 200.0
CROSS_INFLUENCE = 0.10
CROSS_GOAL = np.array([[-1.3, 0.48, 0.03, -0.87, -0.17, -0.18, 0.07], [-1.46, -0.4, -1.84, -0.53, 0.19, -0.01, 0.03]])
CROSS_OPEN = np.array([[0.4, -0.6, 0.0, 0.0, 0.0, 0.0, 0.0], [0.4, 0.6, 0.0, 0.0, 0.0, 0.0, 0.0]])
CROSS_START = CROSS_GOAL - CROSS_OPEN


@functools.lru_cache(maxsize=None)
def crossing_case(pair):
    """dict of start [n,7], R, p (the constant goals [T,n,...]), free and avoid (run()'s dicts with avoid_gain 0 and CROSS_GAIN,
    kp = ko = CROSS_KP, influence CROSS_INFLUENCE, LAM_RUN, restatement rates, no static scene), gain [n_pairs] (the smaller of the two
    arms' min_clearance with avoidance minus the same without) and pairs [n_pairs] (gain >= AW.MIN_GAIN)."""
    n = 2 * N_CROSS
    blocks = JW.blocks_of(pair)
    start = np.tile(CROSS_START, (N_CROSS, 1)) + np.random.default_rng(7308).uniform(-0.03, 0.03, size=(n, 7))
    goal_q = start + np.tile(CROSS_OPEN, (N_CROSS, 1))
    g = TW.by_arm(blocks, arm_bytes(N_CROSS), lambda block, rows: dict(zip(("p", "R"), JW.fk(block, goal_q[rows]))))
    gR, gp = np.array(np.broadcast_to(g["R"], (T_CROSS,) + g["R"].shape)), np.array(np.broadcast_to(g["p"], (T_CROSS,) + g["p"].shape))
    kw = dict(solver="restatement", influence=CROSS_INFLUENCE, kp=CROSS_KP, ko=CROSS_KP)
    free = run(pair, start, gR, gp, TW.LAM_RUN, NO_SCENE, avoid_gain=0.0, **kw)
    avoid = run(pair, start, gR, gp, TW.LAM_RUN, NO_SCENE, avoid_gain=CROSS_GAIN, **kw)
    gain = avoid["min_clearance"].reshape(-1, 2).min(axis=1) - free["min_clearance"].reshape(-1, 2).min(axis=1)
    return dict(start=_frozen(start), R=_frozen(gR), p=_frozen(gp), free=free, avoid=avoid, gain=_frozen(gain),
                pairs=_frozen(gain >= AW.MIN_GAIN))
