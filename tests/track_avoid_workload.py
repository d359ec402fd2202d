"""Inputs, the NumPy reference and the derived tolerances of the rsik_track_avoid tests (tests/test_track_avoid_abi.py pins them on
the CPU alone, tests/test_gpu_track_avoid.py holds the device to them).  No test in this file: pytest does not rewrite its asserts, so
every one of them carries its own message.

The reference is track_workload.one_step with step 4 replaced as include/rsik.h (rsik_track_avoid) defines it: the clearance d, the
nearest pair and the gradient g of the current joints come from clearance_workload.reference, the bias is q0 = rest_gain (rest - q)
(zeros without a rest posture), and where d < influence it gains avoid_gain (influence - d) g.  Steps 1-3 and 5-8 are restated from
track_workload.one_step line for line (it forms q0 inside, so it cannot be called with another one); with no push anywhere the result
is track_workload.run's bit for bit (zeros as bias and no bias are the same numbers in joint_rates_workload.reference), which
tests/test_track_avoid_abi.py asserts.

Goals and starts are track_workload's.  Scenes: clearance_workload.scene(pair, "open"), and a one-sphere scene placed at an elbow of
the unobstructed reference run of a constant-goal case (elbow_case).

Per-step tolerance (2-norm of a trajectory's error in joints_steps[t], the device's own joints before the step fed into one_step):

    tol_t = track_workload's tol_t, evaluated with the full q0
            + dt avoid_gain (sqrt(7) GRADIENT_BOUND (influence - d) + CLEARANCE_BOUND |g|)      where the push acts

The second line is what the device's clearance and gradient may move q0 by: q0 gains a g with a = avoid_gain (influence - d);
|da| <= avoid_gain CLEARANCE_BOUND and |dg| <= sqrt(7) GRADIENT_BOUND (the bound is per entry), so |d(a g)| <= avoid_gain
(CLEARANCE_BOUND |g| + (influence - d) sqrt(7) GRADIENT_BOUND) to first order.  The map from q0 to the rates, I - J^T (J J^T + lambda^2
I)^-1 J, has norm <= 1, so the error of q0 arrives in the rates at most once, and dt times that in the joints.  The two bounds are
clearance_workload's, max(1e-13, 16 E) with E the reference's own float64-against-longdouble error; they were measured on the joint
sets of clearance_workload, so tests/test_track_avoid_abi.py measures E again on the joints the reference run visits and asserts that
max(1e-13, 16 E) does not exceed them.

The (trajectory, step) pairs that are compared (`keep`): |d - influence| >= BAND, so that the device, whose d differs by at most
CLEARANCE_BOUND, takes the same side of the select; and where the push acts the runner-up pair is at least KEEP_RUNNER_UP behind
(the device names the same pair) and the witness points are at least KEEP_AXIS_DISTANCE apart (the gradient's unit vector is well
defined), clearance_workload's two constants."""
import functools
import math

import numpy as np

import clearance_workload as CW
import jacobian_workload as JW
import track_workload as TW

PAIRS = TW.PAIRS
LINK_RADIUS = CW.LINK_RADIUS
INFLUENCE = 0.02          # m: with the "open" scene the push acts on some (trajectory, step) pairs of the seeded run and not on others
AVOID_GAIN = 20.0         # rad/s of bias per metre inside the influence distance and unit of gradient
BAND = 1e-9               # |d - influence| of a kept pair
FAR = np.array([10.0, 0.0, 0.0])   # "the scene moved 10 m away"
N_OPEN, T_OPEN = 257, 33  # the seeded run with the "open" scene whose shares test_track_avoid_abi.py asserts
MIN_GAIN = 0.01           # m: the rows of the elbow case that count are those the reference moves away by at least this
# The elbow case: N_ELBOW rows start within +-0.05 rad of ELBOW_BASE and go to the constant goal FK(start + ELBOW_DELTA), which carries
# the elbow some 10 cm; ONE sphere stands where the unobstructed reference run leaves the elbow of row ELBOW_ROW.
N_ELBOW, T_ELBOW, ELBOW_ROW = 128, 64, 0
ELBOW_BASE = np.array([0.2, -0.3, 0.1, -1.2, 0.1, 0.1, 0.0])
ELBOW_DELTA = np.array([0.35, 0.15, -0.3, 0.3, 0.0, 0.0, 0.0])
ELBOW_RADIUS = 0.04
ELBOW_INFLUENCE = 0.10
# At track_workload's KP = 50 the hand is at its goal, and the elbow inside the sphere, within eight steps, before any push has moved
# it, and min_clearance is that moment with and without avoidance.  The case is about the push, so the approach is slower (a tenth of
# the error per step) and the push strong: measured on the reference, 78 of 128 rows end at least 1 cm further out.
ELBOW_KP = 10.0
ELBOW_GAIN = 200.0


def _frozen(a):
    a.setflags(write=False)
    return a


def moved(scene, by=FAR):
    """The scene translated by `by` [3]."""
    sp, cp = np.array(scene["spheres"], dtype=np.float64), np.array(scene["capsules"], dtype=np.float64)
    sp[:, :3] += by
    cp[:, :3] += by
    cp[:, 3:6] += by
    return dict(spheres=sp, capsules=cp)


def full_scene(pair):
    """(256, 64): the "open" scene repeated.  A later copy of an obstacle ties with the first and loses to it (the first minimum wins),
    so clearance and nearest are the "open" scene's with the capsules' indices moved up by the spheres added."""
    sc = CW.scene(pair, "open")
    sp = np.concatenate([sc["spheres"]] * (256 // len(sc["spheres"]) + 1))[:256].copy()
    cp = np.concatenate([sc["capsules"]] * (64 // len(sc["capsules"]) + 1))[:64].copy()
    return dict(spheres=sp, capsules=cp)


# ------------------------------------------------------------------------------------------ one step, and a run
def one_step(pair, arm, q, goal_R, goal_p, lam, scene, influence=INFLUENCE, avoid_gain=AVOID_GAIN, radius=LINK_RADIUS, dt=TW.DT, kp=TW.KP,
             ko=TW.KO, ff=None, rest=None, rest_gain=0.0, limits=None, solver="lstsq"):
    """Steps 1-8 of rsik_track_avoid for rows of both arms (arm [n] bytes): dict of joints, rates, err, clearance [n], nearest [n,2],
    gradient [n,7], push [n] (the select of step 4b), and what the tolerance and the filter need: J, v, q0 (the full bias), m,
    runner_up, axis_distance, skip, overflow.  Steps 1-3 and 5-8 are track_workload.one_step's lines."""
    q = np.asarray(q, dtype=np.float64)
    arm = np.asarray(arm)
    n = len(q)
    blocks = JW.blocks_of(pair)
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (n,))
    skip = ~(np.isfinite(goal_R).all(axis=(1, 2)) & np.isfinite(goal_p).all(axis=1))
    if ff is not None:
        skip |= ~np.isfinite(ff).all(axis=1)
    gR, gp = np.where(skip[:, None, None], np.eye(3), goal_R), np.where(skip[:, None], 0.0, goal_p)
    # 4a
    c = CW.reference(blocks, q, arm, scene, radius=radius)
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


def avoid_term(step, influence=INFLUENCE, avoid_gain=AVOID_GAIN, dt=TW.DT):
    """What the device's clearance and gradient may add to a step's error in the joints [n]: 0 where the push does not act."""
    d = np.where(step["push"], step["clearance"], influence)
    g = np.linalg.norm(np.where(step["push"][:, None], step["gradient"], 0.0), axis=1)
    return dt * avoid_gain * (math.sqrt(7.0) * CW.GRADIENT_BOUND * (influence - d) + CW.CLEARANCE_BOUND * g)


def step_tolerance(step, q_before, lam, influence=INFLUENCE, avoid_gain=AVOID_GAIN, dt=TW.DT, kp=TW.KP, ko=TW.KO):
    """tol_t [n] of a one_step() result: track_workload's with the full q0, plus avoid_term."""
    return TW.step_tolerance(step, q_before, lam, dt=dt, kp=kp, ko=ko) + avoid_term(step, influence, avoid_gain, dt)


def kept(step, influence=INFLUENCE):
    """The rows of a one_step() result that are compared (see the module's docstring)."""
    with np.errstate(invalid="ignore"):
        band = np.abs(step["clearance"] - influence) >= BAND
        sure = (step["runner_up"] - step["clearance"] >= CW.KEEP_RUNNER_UP) & (step["axis_distance"] >= CW.KEEP_AXIS_DISTANCE)
    return band & (sure | ~step["push"])


def run(pair, arm, start, goals_R, goals_p, lam, scene, solver="lstsq", **terms):
    """one_step iterated over goals_R [T,n,3,3], goals_p [T,n,3] from start [n,7] (terms: influence, avoid_gain, radius, dt, kp, ko,
    ff [T,n,6], rest, rest_gain, limits).  Returns dict of joints, rates [T,n,7], err [T,n,2], clearance, push, keep [T,n], nearest
    [T,n,2], final_joints [n,7], final_err [n,2], min_clearance [n] (over the steps and at the final joints)."""
    T = len(goals_R)
    arm = np.asarray(arm)
    ff = terms.pop("ff", None)
    q = np.asarray(start, dtype=np.float64)
    n = len(q)
    out = dict(joints=np.empty((T, n, 7)), rates=np.empty((T, n, 7)), err=np.empty((T, n, 2)), clearance=np.empty((T, n)),
               push=np.empty((T, n), dtype=bool), keep=np.empty((T, n), dtype=bool), nearest=np.empty((T, n, 2), dtype=np.int32))
    influence = terms.get("influence", INFLUENCE)
    for t in range(T):
        s = one_step(pair, arm, q, goals_R[t], goals_p[t], lam, scene, ff=None if ff is None else ff[t], solver=solver, **terms)
        for k in ("joints", "rates", "err", "clearance", "push", "nearest"):
            out[k][t] = s[k]
        out["keep"][t] = kept(s, influence)
        q = s["joints"]
    out["final_joints"] = q
    blocks = JW.blocks_of(pair)
    out["final_err"] = TW.by_arm(blocks, arm, lambda block, rows: dict(e=TW.pose_error(block, q[rows], goals_R[-1][rows], goals_p[-1][rows])[2]))["e"]
    bad_goal = ~(np.isfinite(goals_R[-1]).all(axis=(1, 2)) & np.isfinite(goals_p[-1]).all(axis=1))
    out["final_err"][bad_goal] = np.nan
    last = CW.reference(blocks, q, arm, scene, radius=terms.get("radius", LINK_RADIUS), full=False)["clearance"]
    out["min_clearance"] = np.minimum(out["clearance"].min(axis=0), last)
    return out


# ------------------------------------------------------------------------------------------ seeded cases
def inputs(pair, n, n_steps, arm, with_terms):
    """track_support.inputs without torch: dict of R, p, m12, start and the terms (all of ff, rest, limits, or none)."""
    R, p = TW.goals_of(pair, n_steps, arm)
    d = dict(R=R, p=p, m12=TW.m12_of(R, p), start=TW.starts()[:n], ff=None, rest=None, rest_gain=0.0, limits=None)
    if with_terms:
        d.update(ff=np.ascontiguousarray(TW.feedforwards(n_steps)[:, :n]), rest=TW.rests()[:n], rest_gain=TW.REST_GAIN, limits=TW.LIMITS)
    return d


def terms_of(d, t=None):
    """The terms of a launch's inputs d as run() (t None) or one_step() (step t) takes them."""
    ff = d["ff"] if t is None or d["ff"] is None else d["ff"][t]
    return dict(ff=ff, rest=d["rest"], rest_gain=d["rest_gain"], limits=d["limits"])


@functools.lru_cache(maxsize=None)
def open_run(pair):
    """The seeded run with the "open" scene (N_OPEN rows with an arm byte each, T_OPEN steps, lambda 0.05, no further terms, the
    float64 restatement of the device's solve as the rates: the shares below do not see the difference): run()'s dict, frozen."""
    arm = JW.arm_bytes()[:N_OPEN]
    d = inputs(pair, N_OPEN, T_OPEN, arm, False)
    out = run(pair, arm, d["start"], d["R"], d["p"], 0.05, CW.scene(pair, "open"), solver="restatement")
    return {k: _frozen(a) for k, a in out.items()}


@functools.lru_cache(maxsize=None)
def elbow_case(pair, side):
    """The avoidance case on one block (see ELBOW_BASE): constant goals, LAM_RUN, KP, KO, DT, T_ELBOW steps.  Returns dict of start, R, p
    (the goals [T,n,...]), scene, free and avoid (run()'s dicts with avoid_gain 0 and ELBOW_GAIN, kp = ko = ELBOW_KP, influence
    ELBOW_INFLUENCE, restatement rates), gain [n] (the
    reference's min_clearance with avoidance minus the one without) and rows [n] (gain >= MIN_GAIN)."""
    block = JW.blocks_of(pair)[side]
    start = ELBOW_BASE + np.random.default_rng(7306).uniform(-0.05, 0.05, size=(N_ELBOW, 7))
    p, R = JW.fk(block, start + ELBOW_DELTA)
    gR, gp = np.array(np.broadcast_to(R, (T_ELBOW,) + R.shape)), np.array(np.broadcast_to(p, (T_ELBOW,) + p.shape))
    arm = np.full(N_ELBOW, side, dtype=np.uint8)
    plain = TW.run(block, start, gR, gp, TW.LAM_RUN, solver="restatement")
    elbow = CW.walk(block, plain["final_joints"][ELBOW_ROW:ELBOW_ROW + 1])[0][0, 1]
    scene = dict(spheres=_frozen(np.concatenate([elbow, [ELBOW_RADIUS]])[None]), capsules=_frozen(np.zeros((0, 7))))
    kw = dict(solver="restatement", influence=ELBOW_INFLUENCE, kp=ELBOW_KP, ko=ELBOW_KP)
    free = run(pair, arm, start, gR, gp, TW.LAM_RUN, scene, avoid_gain=0.0, **kw)
    avoid = run(pair, arm, start, gR, gp, TW.LAM_RUN, scene, avoid_gain=ELBOW_GAIN, **kw)
    gain = avoid["min_clearance"] - free["min_clearance"]
    return dict(start=_frozen(start), R=_frozen(gR), p=_frozen(gp), scene=scene, free=free, avoid=avoid, gain=_frozen(gain),
                rows=_frozen(gain >= MIN_GAIN))
