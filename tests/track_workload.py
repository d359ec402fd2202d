"""Inputs, the NumPy reference and the derived tolerances of the rsik_track tests (tests/test_track_abi.py pins them on the CPU alone,
tests/test_gpu_track.py and tests/test_gpu_track_edges.py hold the device to them).  No test in this file: pytest does not rewrite its
asserts, so every one of them carries its own message.

Built on jacobian_workload (fk, jacobian, joint_set, arm_bytes, blocks_of, PAIRS) and joint_rates_workload (reference: lstsq on the
stacked system, never the normal equations the device solves; tolerances).  one_step() restates steps 1-8 of include/rsik.h for a
batch of one arm block, run() iterates it.

Goals: the goal at step t is FK of a smooth joint path q_start + delta + a sin(omega t + phi), seeded, |delta| <= 0.05, a <= 0.1,
omega in [0.05, 0.3] rad per step: every goal is reachable and the rotation error stays far below pi.

Per-step tolerance (2-norm of a trajectory's error in joints_steps[t], the device's own joints_steps[t - 1] fed into one_step):

    tol_t = dt (tol_row(J, v, lambda, q0) + g |dv|) + 4 * 2^-53 |q|,      |dv| = kp E_p + ko E_o

tol_row and g are joint_rates_workload.tolerances'.  |dv| is what the device's forward kinematics may move the twist by: the existing
tests hold rsik_forward_kinematics to FK_ENTRY = 1e-14 per entry of the position and of the rotation against the NumPy chain
(tests/test_gpu_parity.py::test_device_forward_kinematics_matches_numpy_chain).  From that, with e = FK_ENTRY:
    E_p = sqrt(3) e                    the 2-norm of the position error;
    |dD_ij| <= |Rg_i| |dR_j| <= sqrt(3) e for D = Rg R^T, so each component of w = 1/2 (D21 - D12, ...) moves by at most sqrt(3) e,
    |dw| <= 3 e, |ds| <= 3 e, |dc| = 1/2 |d tr D| <= 1.5 sqrt(3) e <= 2.6 e, |d angle| <= |ds| + |dc| <= 5.6 e;
    e_o = (angle / s) w:  |d e_o| <= (angle / s)(|dw| + |ds|) + |d angle| <= 1.19 * 6 e + 5.6 e < 13 e for angle < 1 (angle / sin angle
    <= 1.19 there; the reference's own runs are asserted to stay below 1)
    E_o = 13 e                         bounds the error of e_o and (5.6 e) of the angle.
Rotation errors of any size (tests/test_gpu_track_edges.py) keep these terms and drop the substitution: per row, with the reference's
own angle and s,
    e_o_bound = (angle / s) 6 e + 5.6 e   where s^2 >= 2^-52: (angle / s)(|dw| + |ds|) + |d angle|, from d(w angle / s) =
                                          (angle / s) dw + w d angle / s - w angle ds / s^2 and |w| = s;
    e_o_bound = 3 e                       where s^2 < 2^-52: e_o = w and |dw| <= 3 e;
    E_ANGLE = 5.6 e                       at every angle: angle = atan2(s, c) moves by |c ds - s dc| <= |ds| + |dc| on the unit circle.
Near a half turn angle / s grows without bound (2e8 at s = 2^-26: e_o_bound = 1.2e-5 there): the direction of e_o is the direction of a
vector of length s known to 3 e.  The two branches of e_o agree to 1e-24 at the switch near 0 (angle / s - 1 = s^2 / 6) and differ by
the factor angle / s = 2e8 at the switch near pi, so the rows of the ladder (LADDER: 0 ... pi, both sides of both switches) keep
|s^2 2^52 - 1| >= 2^-6 near pi (band_margin): the device's s differs from the reference's by at most 3 e, 2e-6 relative at s = 2^-26,
and both take the same branch.  At the pi rung s is below 3 e and e_o = w: the loop does not turn (include/rsik.h).
Finite values that overflow: a step whose rates do not come out finite is held like a skipped step and err[0] is +infinity where
|e_p|^2 overflows (include/rsik.h); one_step follows the same rule (`overflow`).  Where such a step is taken with limits, the solve
without a rest term is linear in v, so the limited rates are the rates of v / m and their tolerance is
joint_rates_workload.tolerances at (J, v / m, lambda), m the reference's limit factor (FAR_RUNGS, FAR_HELD, far_inputs).
The limits add no term to tol_t.  For the clamp that is exact: a projection onto a box is non-expansive in the 2-norm.  For the rate
limit it is not: scaling by 1 / max_k (|q'_k| / rate_max_k) is a radial projection onto a weighted max-norm box, which is non-expansive
in that weighted max-norm but can expand a 2-norm difference, by up to sqrt(2) for equal rate_max and by more for unequal ones.  The
formula is kept as the definition of the check states it, without a factor for this; where the rate limit binds, the tests with limits
pass on the slack of tol_row and g, which are worst-case bounds (the GPU tests print the worst error / tol_t they see).  4 * 2^-53 |q|
is the rounding of q + dt q' and of the clamp's compare.  A per-step check compounds no error: it holds every step of a long run to
the one-step bound.

End-to-end tolerance (device against run() from the same start): A * sum_t tol_t, A the amplification of the reference alone:
run twice, the second time with the start perturbed by seeded noise of 1e-12 per entry; A = 4 x the worst ratio over the rows of
|difference at the end| to |difference at the start| (4: the device injects an error at every step and not once).  The end-to-end
case is the constant-goal case (constant_goal_case: the uniform set, 512 rows, lambda = 1e-3, kp = ko = 50, dt = 0.01, T = 64, the goal
FK(q_start + delta)).  Measured there with the float64 restatement in place of lstsq: the worst ratio is 0.927 ... 0.960 on the three
pairs and both blocks, A = 3.71 ... 3.84 (amplification(); tests/test_track_abi.py asserts A < 16).  The closed loop does not amplify:
the task-space part of a perturbation decays by kp dt per step, the null-space part stays.
With the MOVING goals above (the first 512 rows, T = 64, lambda = 1e-3) the same measurement, restatement rates and the same noise seed,
gives a worst ratio of 14.3 on default/default block 0 (6.8 ... 14.3 over the pairs and blocks), and three rows above 3 everywhere:
rows 55, 62 and 159 (14.3, 13.4 and 6.5 on default/default block 0), every other row at most 2.4.  These rows pass close to a straight
elbow while the goal moves: at lambda = 1e-3 the damped inverse has a gain of up to 1 / (2 lambda) = 500 there, and a perturbed start is
carried along.  A < 16 cannot be asserted of that run (4 x 14.3 = 57), so the issue's end-to-end test and A stay on the constant goal.
The moving goals are held end to end too, with an amplification PER ROW (run_gain): G_i = the 2-norm of the 7 x 7 matrix d q_end / d
q_start of the reference's run of row i, by forward differences of 1e-8 per start entry (restatement rates; 1e-9 and central
differences give the same figures to three digits, so the run is linear and its own rounding invisible at that size), and
A_i = 4 max(1, G_i): the matrix norm is the worst ratio over EVERY direction of the perturbation, which one draw of noise only samples,
and no factor below 1 can bound the sum, since the error of the last step arrives as it is.  Measured on the three pairs and both
blocks: median G 1.007 ... 1.008, G > 3 on five rows, 55 (16.6 ... 22.2), 62 (10.7 ... 12.2), 159 (11.0 ... 11.3), 485 (3.6 ... 4.2)
and 363 (3.2 ... 3.4), every other row at most 2.1.  tests/test_track_abi.py asserts that at least 95 % of the rows have G <= 4, so
that a per-row factor cannot hide a failure."""
import functools
import math

import numpy as np

import jacobian_workload as JW
import joint_rates_workload as W

PAIRS = JW.PAIRS
FK_ENTRY = 1e-14                      # what the existing tests hold rsik_forward_kinematics to, per entry
E_P = math.sqrt(3.0) * FK_ENTRY
E_O = 13.0 * FK_ENTRY
EPS = 2.0 ** -53
DT, KP, KO = 0.01, 50.0, 50.0
LAMBDAS = (1e-3, 0.05)
REST_GAIN = 2.0
# limits that bind on the seeded goals: the rates reach a few rad/s (kp times an error of up to 0.1 rad)
LIMITS = np.array([[1.0, 1.5, 2.0, 1.0, 3.0, 2.5, 1.5], [-2.05] * 7, [2.05] * 7])
LIMITS.setflags(write=False)
# a rate limit alone, twice as wide: it binds on some trajectories of the seeded goals' first step and not on others
RATE_LIMIT_ONLY = np.array([2.0 * LIMITS[0], [-np.inf] * 7, [np.inf] * 7])
RATE_LIMIT_ONLY.setflags(write=False)


def _frozen(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------ the pose error
def rotvec(D):
    """The rotation vector of rotations D [n,3,3] as include/rsik.h defines it (step 2): (e_o [n,3], angle [n]).  SciPy-free."""
    w = 0.5 * np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], axis=1)
    s = np.linalg.norm(w, axis=1)
    c = 0.5 * (np.trace(D, axis1=1, axis2=2) - 1.0)
    angle = np.arctan2(s, c)
    big = s * s >= 2.0 ** -52
    scale = np.where(big, angle / np.where(big, s, 1.0), 1.0)
    return w * scale[:, None], angle


def w_norm(D):
    """s = |w| of rotations D [n,3,3]: what rotvec's branch looks at."""
    w = 0.5 * np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], axis=1)
    return np.linalg.norm(w, axis=1)


def pose_error(block, q, goal_R, goal_p):
    """Steps 1-2 for joints q [n,7] on one arm block: (e_p [n,3], e_o [n,3], err [n,2]).  err[:, 0] = sqrt(|e_p|^2), +infinity where
    the square overflows."""
    p, R = JW.fk(block, q)
    e_p = goal_p - p
    e_o, angle = rotvec(goal_R @ R.transpose(0, 2, 1))
    with np.errstate(over="ignore"):
        return e_p, e_o, np.stack([np.sqrt((e_p * e_p).sum(axis=1)), angle], axis=1)


# ------------------------------------------------------------------------------------------ rotation errors of any size
E_ANGLE = 5.6 * FK_ENTRY              # |d angle| <= |ds| + |dc| at every angle (the docstring's term)
SWITCH = 2.0 ** -52                   # e_o = w (angle / s) where s^2 >= SWITCH, else e_o = w
BAND = 2.0 ** -6                      # how far from the switch, relative in s^2, every ladder row near pi stays
_H = 2.0 ** -26                       # sqrt(SWITCH)
LADDER = (0.0, 1e-12, 1e-9, _H * (1 - BAND), _H, _H * (1 + BAND), 1e-4,
          1.0, math.pi / 4, math.pi / 2 - 1e-9, math.pi / 2, math.pi / 2 + 1e-9, 3 * math.pi / 4, 2.0, 3.0,
          math.pi - 1e-3, math.pi - 1e-6, math.pi - _H * (1 + BAND), math.pi - _H * (1 - BAND), math.pi)
NEAR_ZERO_RUNGS = 7                   # the first rungs: there the two branches of e_o agree to 1e-24 and a row may sit on the switch
N_LADDER = 130                        # the ladder padded to two waves and two rows


def rodrigues(axes, angles):
    """Rotations [n,3,3] about unit axes [n,3] by angles [n], in float64."""
    a, t = np.asarray(axes, dtype=np.float64), np.asarray(angles, dtype=np.float64)
    S = np.zeros((len(a), 3, 3))
    S[:, 0, 1], S[:, 0, 2], S[:, 1, 0], S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
    c, s = np.cos(t)[:, None, None], np.sin(t)[:, None, None]
    return c * np.eye(3) + s * S + (1.0 - c) * (a[:, :, None] * a[:, None, :])


def rotated_goals(block, q, axes, angles):
    """Goals whose rotation error at joints q [n,7] is the prescribed rotation, up to the FK's e, and whose position error is 0:
    (R_g [n,3,3], p_g [n,3]) = (Rot(axis, angle) R_fk(q), p_fk(q)) from the NumPy chain."""
    p, R = JW.fk(block, q)
    return rodrigues(axes, angles) @ R, p


def e_o_bound(angle, s):
    """What the FK's e per entry may move e_o by, per row, at any angle (angle [n], s = |w| [n] of the reference): (angle / s) 6 e +
    5.6 e where s^2 >= 2^-52, 3 e where e_o = w."""
    angle, s = np.asarray(angle, dtype=np.float64), np.asarray(s, dtype=np.float64)
    big = s * s >= SWITCH
    return np.where(big, angle / np.where(big, s, 1.0) * 6.0 * FK_ENTRY + E_ANGLE, 3.0 * FK_ENTRY)


@functools.lru_cache(maxsize=None)
def ladder(n=N_LADDER):
    """The rotation errors of the edge tests: (angles [n], axes [n,3], rung [n]); row i stands on rung i mod len(LADDER), every row
    with a seeded unit axis of its own."""
    rung = np.arange(n) % len(LADDER)
    axes = np.random.default_rng(7307).normal(size=(n, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    return _frozen(np.array(LADDER)[rung]), _frozen(axes), _frozen(rung)


def ladder_goals(pair, arm, q):
    """The ladder's goals at joints q [n,7], each row on the block its arm byte names: dict of R [n,3,3], p [n,3], s [n] (the
    reference's |w| at q) and e_o [n] = e_o_bound of the reference's angle and s."""
    angles, axes, _ = ladder(len(q))

    def fn(block, rows):
        R, p = rotated_goals(block, q[rows], axes[rows], angles[rows])
        D = R @ JW.fk(block, q[rows])[1].transpose(0, 2, 1)
        s = w_norm(D)
        return dict(R=R, p=p, s=s, e_o=e_o_bound(rotvec(D)[1], s))

    return by_arm(JW.blocks_of(pair), arm, fn)


def band_margin(s):
    """|s^2 2^52 - 1| per row: the ladder keeps it >= BAND on every row that is not near 0, so that the device, whose s differs from
    the reference's by at most 3 e (2e-6 relative at s = 2^-26), takes the reference's branch of e_o."""
    return np.abs(np.asarray(s) ** 2 / SWITCH - 1.0)


# ------------------------------------------------------------------------------------------ one step, and a run
def _rates(J, v, lam, q0, solver):
    if solver == "lstsq":
        return W.reference(J, v, lam, q0)["rates"]
    assert solver == "restatement", solver
    return W.restatement(J, v, lam, q0)


def one_step(block, q, goal_R, goal_p, lam, dt=DT, kp=KP, ko=KO, ff=None, rest=None, rest_gain=0.0, limits=None, solver="lstsq"):
    """Steps 1-8 for a batch on one arm block: q [n,7], goal_R [n,3,3], goal_p [n,3], lam a number or [n], ff [n,6] or None,
    rest [n,7] or None, limits [3,7] or None.  Returns dict of joints [n,7] (after the step), rates [n,7] (after the limit),
    err [n,2], and what the tolerance needs: J [n,6,7], v [n,6], q0 [n,7] or None, m [n] (the factor of the rate limit, 1 where it
    does not bind).  A row whose goal or feed-forward is not numbers is skipped: joints held, rates 0, err NaN.  A row whose goal and
    feed-forward are numbers but whose rates do not come out finite (a twist that overflows) is held in the same way (`overflow`
    marks it).  err[:, 0] is sqrt(|e_p|^2): +infinity where the square overflows."""
    q = np.asarray(q, dtype=np.float64)
    n = len(q)
    skip = ~(np.isfinite(goal_R).all(axis=(1, 2)) & np.isfinite(goal_p).all(axis=1))
    if ff is not None:
        skip |= ~np.isfinite(ff).all(axis=1)
    gR, gp = np.where(skip[:, None, None], np.eye(3), goal_R), np.where(skip[:, None], 0.0, goal_p)
    with np.errstate(over="ignore", invalid="ignore"):
        e_p, e_o, err = pose_error(block, q, gR, gp)
        v = np.concatenate([kp * e_p, ko * e_o], axis=1)
        if ff is not None:
            v = np.where(skip[:, None], 0.0, ff) + v
        q0 = None if rest is None else rest_gain * (rest - q)
        J = JW.jacobian(block, q)
        solvable = np.isfinite(v).all(axis=1)  # (LAPACK refuses a right-hand side that is not numbers)
        rates = np.full((n, 7), np.nan)
        if solvable.any():
            rates[solvable] = _rates(J[solvable], v[solvable], np.broadcast_to(np.asarray(lam, dtype=np.float64), (n,))[solvable],
                                     None if q0 is None else q0[solvable], solver)
        overflow = ~skip & ~np.isfinite(rates).all(axis=1)
        held = skip | overflow
        m = np.ones(n)
        if limits is not None:
            m = np.where(held, 1.0, np.maximum((np.abs(rates) / limits[0]).max(axis=1), 1.0))
            rates = np.where((m > 1.0)[:, None], rates / m[:, None], rates)
        moved = q + dt * rates
    if limits is not None:
        moved = np.minimum(np.maximum(moved, limits[1]), limits[2])
    return dict(joints=np.where(held[:, None], q, moved), rates=np.where(held[:, None], 0.0, rates),
                err=np.where(held[:, None], np.nan, err), J=J, v=v, q0=q0, skip=skip, overflow=overflow, m=m)


def rates_tolerance(step, lam, kp=KP, ko=KO, e_o=E_O):
    """The part of tol_t that is the error of the rates [n]: tol_row + g |dv|; e_o a number or one per row (e_o_bound)."""
    t = W.tolerances(step["J"], step["v"], lam, step["q0"])
    return t["tol_row"] + t["g"] * (kp * E_P + ko * np.asarray(e_o, dtype=np.float64))


def step_tolerance(step, q_before, lam, dt=DT, kp=KP, ko=KO, e_o=E_O):
    """tol_t [n] of a one_step() result for the joints it started from; e_o: what bounds the error of e_o, E_O (angle < 1) or one
    value per row (e_o_bound)."""
    return dt * rates_tolerance(step, lam, kp, ko, e_o) + 4.0 * EPS * np.linalg.norm(q_before, axis=1)


def run(block, start, goals_R, goals_p, lam, solver="lstsq", with_tolerance=False, **terms):
    """one_step iterated over goals_R [T,n,3,3], goals_p [T,n,3] from start [n,7] (terms: dt, kp, ko, ff [T,n,6], rest, rest_gain,
    limits).  Returns dict of joints [T,n,7], rates [T,n,7], err [T,n,2], final_joints [n,7], final_err [n,2], and with_tolerance
    tol [T,n]: tol_t of every step of this run."""
    T = len(goals_R)
    ff = terms.pop("ff", None)
    q = np.asarray(start, dtype=np.float64)
    out = dict(joints=np.empty((T,) + q.shape), rates=np.empty((T,) + q.shape), err=np.empty((T, len(q), 2)))
    if with_tolerance:
        out["tol"] = np.empty((T, len(q)))
    for t in range(T):
        s = one_step(block, q, goals_R[t], goals_p[t], lam, ff=None if ff is None else ff[t], solver=solver, **terms)
        if with_tolerance:
            out["tol"][t] = step_tolerance(s, q, lam, **{k: terms[k] for k in ("dt", "kp", "ko") if k in terms})
        out["joints"][t], out["rates"][t], out["err"][t] = s["joints"], s["rates"], s["err"]
        q = s["joints"]
    out["final_joints"] = q
    out["final_err"] = pose_error(block, q, goals_R[-1], goals_p[-1])[2]
    bad_goal = ~(np.isfinite(goals_R[-1]).all(axis=(1, 2)) & np.isfinite(goals_p[-1]).all(axis=1))
    out["final_err"][bad_goal] = np.nan
    return out


# ------------------------------------------------------------------------------------------ seeded inputs
@functools.lru_cache(maxsize=None)
def starts(n=JW.N_SET):
    return JW.joint_set("uniform")[:n]


@functools.lru_cache(maxsize=None)
def joint_paths(T, n=JW.N_SET):
    """The smooth joint path the goals are FK of: [T,n,7] = start + delta + a sin(omega t + phi)."""
    rng = np.random.default_rng(7301)
    delta = rng.uniform(-0.05, 0.05, size=(n, 7))
    a = rng.uniform(0.0, 0.1, size=(n, 7))
    omega = rng.uniform(0.05, 0.3, size=(n, 7))
    phi = rng.uniform(-np.pi, np.pi, size=(n, 7))
    t = np.arange(T, dtype=np.float64)[:, None, None]
    return _frozen(starts(n) + delta + a * np.sin(omega * t + phi))


@functools.lru_cache(maxsize=None)
def side_goals(pair, T, n=JW.N_SET):
    """The goals of every row on the r block and on the l block: ((R [T,n,3,3], p [T,n,3]), (R, p)).  The goal of any arm arrangement
    is a row-wise pick (goals_of)."""
    out = []
    path = joint_paths(T, n).reshape(-1, 7)
    for block in JW.blocks_of(pair):
        p, R = JW.fk(block, path)
        out.append((_frozen(R.reshape(T, n, 3, 3)), _frozen(p.reshape(T, n, 3))))
    return tuple(out)


def goals_of(pair, T, arm, n=None):
    """(R [T,n,3,3], p [T,n,3]) of the first n = len(arm) rows, each from the block its arm byte names."""
    arm = np.asarray(arm)
    n = len(arm)
    (R0, p0), (R1, p1) = side_goals(pair, T)
    sel = arm == 1
    return np.where(sel[None, :, None, None], R1[:, :n], R0[:, :n]), np.where(sel[None, :, None], p1[:, :n], p0[:, :n])


def m12_of(R, p):
    """Goals (R [T,n,3,3], p [T,n,3]) in the ABI's layout [T,12,n]: R row-major, then t."""
    T, n = R.shape[:2]
    return np.ascontiguousarray(np.concatenate([R.reshape(T, n, 9), p], axis=2).transpose(0, 2, 1))


@functools.lru_cache(maxsize=None)
def feedforwards(T, n=JW.N_SET):
    return _frozen(np.random.default_rng(7302).uniform(-0.2, 0.2, size=(T, n, 6)))


@functools.lru_cache(maxsize=None)
def rests(n=JW.N_SET):
    return _frozen(np.random.default_rng(7303).uniform(-1.0, 1.0, size=(n, 7)))


def by_arm(blocks, arm, fn):
    """fn(block, rows) -> dict of arrays [len(rows), ...], evaluated per arm block on that arm's rows and put back together in the
    rows' order."""
    arm = np.asarray(arm)
    out = {}
    for side in (0, 1):
        rows = np.flatnonzero(arm == side)
        if not len(rows):
            continue
        for k, a in fn(blocks[side], rows).items():
            if k not in out:
                out[k] = np.empty((len(arm),) + a.shape[1:], dtype=a.dtype)
            out[k][rows] = a
    return out


def step_by_arm(pair, arm, q, goal_R, goal_p, lam, **terms):
    """one_step and its tolerance for rows of both arms: dict of joints, rates, err [n,...], tol [n] (tol_t, for the joints) and
    tol_rates [n] (its part for the rates).  e_o [n]: e_o_bound per row in place of E_O; tol_ko: the ko the tolerance is taken at
    where it is not the step's own."""
    blocks = JW.blocks_of(pair)
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (len(q),))
    ff, rest, e_o, tol_ko = terms.pop("ff", None), terms.pop("rest", None), terms.pop("e_o", None), terms.pop("tol_ko", None)
    gains = {k: terms[k] for k in ("dt", "kp", "ko") if k in terms}
    if tol_ko is not None:
        gains["ko"] = tol_ko

    def fn(block, rows):
        s = one_step(block, q[rows], goal_R[rows], goal_p[rows], lam[rows], ff=None if ff is None else ff[rows],
                     rest=None if rest is None else rest[rows], **terms)
        e = dict(e_o=np.broadcast_to(e_o, (len(q),))[rows]) if e_o is not None else {}
        rate_gains = {k: v for k, v in gains.items() if k != "dt"}
        with np.errstate(all="ignore"):  # (a twist that overflows has no tolerance: its rows are held, not compared)
            tol, tol_rates = step_tolerance(s, q[rows], lam[rows], **gains, **e), rates_tolerance(s, lam[rows], **rate_gains, **e)
        return dict(joints=s["joints"], rates=s["rates"], err=s["err"], tol=tol, tol_rates=tol_rates, overflow=s["overflow"], J=s["J"],
                    v=s["v"], m=s["m"])

    return by_arm(blocks, arm, fn)


def reference_terms(d, t):
    """The terms of step t of a launch's inputs d (ff [T,n,6] or None, rest, rest_gain, limits) as one_step takes them."""
    return dict(ff=None if d["ff"] is None else d["ff"][t], rest=d["rest"], rest_gain=d["rest_gain"], limits=d["limits"])


def check_every_step(pair, arm, d, lam, got, what):
    """The per-step check of a launch (d: its inputs, with R [T,n,3,3], p [T,n,3], start [n,7] and the terms; got: its joints and err
    per step): the device's own joints_steps[t - 1] fed into one_step, joints_steps[t] within tol_t, err_steps[t] within (E_p, E_o)
    of the reference's error at those joints.  For goals whose rotation error stays below 1 rad.  Returns the worst error / tol_t."""
    worst = 0.0
    for t in range(len(d["R"])):
        before = d["start"] if t == 0 else got["joints"][t - 1]
        ref = step_by_arm(pair, arm, before, d["R"][t], d["p"][t], lam, **reference_terms(d, t))
        e = np.linalg.norm(got["joints"][t] - ref["joints"], axis=1)
        worst = max(worst, float((e / ref["tol"]).max()))
        assert (e <= ref["tol"]).all(), (what, t, "joints", float((e / ref["tol"]).max()))
        de = np.abs(got["err"][t] - ref["err"])
        assert (de[:, 0] <= E_P).all() and (de[:, 1] <= E_O).all(), (what, t, "err", de.max(axis=0).tolist())
        assert (ref["err"][:, 1] < 1.0).all(), (what, t, "the rotation error is to stay far below pi")
    return worst


def goals_near(pair, arm, base, T):
    """Goals for starts other than starts(): FK of base + (joint_paths(T) - starts()), the seeded path carried over to joints base
    [n,7], each row on the block its arm byte names: (R [T,n,3,3], p [T,n,3])."""
    n = len(base)
    path = (base[None] + (joint_paths(T)[:, :n] - starts()[:n])).reshape(-1, 7)

    def fn(block, rows):
        p, R = JW.fk(block, path[rows])
        return dict(R=R, p=p)

    g = by_arm(JW.blocks_of(pair), np.tile(np.asarray(arm), T), fn)
    return g["R"].reshape(T, n, 3, 3), g["p"].reshape(T, n, 3)


# ------------------------------------------------------------------------------------------ finite goals and feed-forwards far outside reach
DBL_MAX = float(np.finfo(np.float64).max)
N_FAR, T_FAR, FAR_STEP, FAR_ROWS = 65, 3, 1, (0, 63, 64)
FAR_RUNGS = tuple(("goal", v) for v in (1e15, 1e150, 1e160, 1e300, 1e307)) + tuple(("ff", v) for v in (1e150, 1e300, 1e305, DBL_MAX))
# The rungs whose rates do not come out finite, on FAR_ROWS: kp * 1e307 is an infinity, and DBL_MAX in a position entry of the
# feed-forward overflows in the first sums of the solve.  A feed-forward entry of 1e305 does NOT overflow on these rows, in lstsq and in
# the float64 restatement of the device's algorithm alike: the rates are at most g * 1e305 <= 1e305 / (2 lambda) = 5e307
# (tests/test_track_abi.py pins both lists on the reference alone).
FAR_HELD = (("goal", 1e307), ("ff", DBL_MAX))
EP2_OVERFLOWS = 1.3e154               # from here on |e_p|^2 is an infinity and err[0] = +infinity


def far_inputs(d, kind, value):
    """The inputs d of a launch (R, p, m12, ff, ...: T_FAR steps, N_FAR rows) with one far value at step FAR_STEP of each of FAR_ROWS:
    a goal-position entry or a position entry of the feed-forward, the entry and the sign changing from row to row.  Returns the new
    dict; d is left as it is."""
    p, m12, ff = d["p"].copy(), d["m12"].copy(), d["ff"].copy()
    for i, row in enumerate(FAR_ROWS):
        x = value if i % 2 == 0 else -value
        if kind == "goal":
            p[FAR_STEP, row, i % 3] = m12[FAR_STEP, 9 + i % 3, row] = x
        else:
            ff[FAR_STEP, row, i % 3] = x
    return dict(d, p=p, m12=m12, ff=ff)


# ------------------------------------------------------------------------------------------ the constant-goal case and the amplification
CONVERGED = 1e-9     # m and rad: the rows of the constant-goal case that the reference brings below this are kept
N_RUN, T_RUN, LAM_RUN = 512, 64, 1e-3


@functools.lru_cache(maxsize=None)
def constant_goal_case(pair, side):
    """The convergence case on one block: the goal is the constant FK(q_start + delta), delta seeded in [-0.05, 0.05]^7, on the first
    N_RUN uniform rows, LAM_RUN, KP, KO, DT, T_RUN steps.  Returns (goals_R [T,n,3,3], goals_p [T,n,3], keep [n]): keep marks the
    rows the reference (the float64 restatement of the device's algorithm as the rates: 64 steps of lstsq per row change nothing the
    filter can see) ends below CONVERGED in both entries of final_err."""
    block = JW.blocks_of(pair)[side]
    delta = np.random.default_rng(7304).uniform(-0.05, 0.05, size=(N_RUN, 7))
    p, R = JW.fk(block, starts(N_RUN) + delta)
    gR, gp = np.broadcast_to(R, (T_RUN,) + R.shape), np.broadcast_to(p, (T_RUN,) + p.shape)
    ref = run(block, starts(N_RUN), gR, gp, LAM_RUN, solver="restatement")
    return _frozen(np.array(gR)), _frozen(np.array(gp)), _frozen((ref["final_err"] < CONVERGED).all(axis=1))


@functools.lru_cache(maxsize=None)
def amplification(pair, side):
    """(A, worst ratio) of the end-to-end case on one block, which is the constant-goal case: two runs of the reference (restatement
    rates), the second from a start perturbed by seeded noise of 1e-12 per entry."""
    block = JW.blocks_of(pair)[side]
    R, p, _ = constant_goal_case(pair, side)
    noise = np.random.default_rng(7305).uniform(-1e-12, 1e-12, size=(N_RUN, 7))
    a = run(block, starts(N_RUN), R, p, LAM_RUN, solver="restatement")["final_joints"]
    b = run(block, starts(N_RUN) + noise, R, p, LAM_RUN, solver="restatement")["final_joints"]
    ratio = float((np.linalg.norm(b - a, axis=1) / np.linalg.norm(noise, axis=1)).max())
    return 4.0 * ratio, ratio


# ------------------------------------------------------------------------------------------ the moving goals end to end, a gain per row
@functools.lru_cache(maxsize=None)
def moving_goal_case(pair, side):
    """The moving goals of the first N_RUN rows over T_RUN steps on one block: (goals_R [T,n,3,3], goals_p [T,n,3])."""
    R, p = side_goals(pair, T_RUN)[side]
    return _frozen(np.ascontiguousarray(R[:, :N_RUN])), _frozen(np.ascontiguousarray(p[:, :N_RUN]))


@functools.lru_cache(maxsize=None)
def run_gain(pair, side, h=1e-8):
    """G [n]: per row the 2-norm of d final_joints / d start of the reference's run on the moving goals (restatement rates, LAM_RUN),
    by forward differences of h per start entry.  The amplification of row i end to end is A_i = 4 max(1, G_i)."""
    block = JW.blocks_of(pair)[side]
    R, p = moving_goal_case(pair, side)
    base = run(block, starts(N_RUN), R, p, LAM_RUN, solver="restatement")["final_joints"]
    G = np.empty((N_RUN, 7, 7))
    for k in range(7):
        d = np.zeros((N_RUN, 7))
        d[:, k] = h
        G[:, :, k] = (run(block, starts(N_RUN) + d, R, p, LAM_RUN, solver="restatement")["final_joints"] - base) / h
    return _frozen(np.linalg.norm(G, ord=2, axis=(1, 2)))
