"""The shared workload of the theta-from-joints tests (tests/test_theta_from_joints_checker.py on the CPU,
tests/test_gpu_theta_from_joints.py on the GPU) and what both need of the CPU checker: the rows, the checker's answer for a
batch of them, a replay of the search in Python on the checker's get_joints, and the table of every bracket the search can
end in.  NumPy and the checker only: nothing here touches the product.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from compare import angle_diff
from oracle import oracle as orc

SEED = 20261016                     # chosen on the CPU: the checker's replay finds no near tie in the subsample (see near_ties)
N_FULL = 1 << 18                    # config-3 size
N_SUBSAMPLE = 1 << 14
TOLERANCE = 0.01                    # utils.py:294
NEAR_TIE = 1e-9                     # two sides of a comparison of the search closer than this can fall either way on the device
PREFERRED = (-4 * np.pi / 6, -np.pi + 4 * np.pi / 6)   # ControlIK.preferred_theta of r, l (control_ik.py:133-139)
BRACKET0 = ((-np.pi, np.pi), (0.0, 2 * np.pi))          # utils.py:288-292
NTHREADS = min(16, os.cpu_count() or 1)


def distance(joints, cur):
    """The search's objective (utils.py:297, 307-310): 7 joints against 7, or the constructor's 2x7 form (Q15)."""
    cur = np.asarray(cur, dtype=np.float64)
    if cur.size == 7:
        d = angle_diff(joints, cur.reshape(7))
    else:
        d = np.array([angle_diff(joints[q], cur.reshape(2, 7)[q, k]) for q in range(2) for k in range(7)])
    return float(np.sqrt(np.sum(d * d)))


def theta_workload(seed, n, arm=None, so=0.03, shortcut_every=16, far_every=8, arms=None):
    """pos [n,3], eul [n,3], arm [n] uint8, cur [n,7]: start poses an arm can be in (a box in front of the row's own shoulder,
    hand pointing forward within +-0.7 rad, as G7's), the joints it measured uniform in +-0.6 as G7 draws them, every
    `far_every`-th row up to +-5 pi (angle_diff's wrap), and every `shortcut_every`-th row within 1e-3 of the solution at the
    arm's preferred theta (the shortcut of utils.py:296-300), half of those moved by whole turns.  arms: the checker's (r, l) arms the
    shortcut rows are built on, the default arms with offset `so` where None."""
    rng = np.random.default_rng(seed)
    byte = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    if arm is not None:
        byte = np.full(n, int(arm), dtype=np.uint8)
    sgn = np.where(byte == 1, -1.0, 1.0)
    pos = np.array([0.38, -0.2, -0.1]) + rng.uniform(-0.22, 0.22, size=(n, 3))
    eul = np.array([0.0, -np.pi / 2, 0.0]) + rng.uniform(-0.7, 0.7, size=(n, 3))
    pos = pos * np.stack([np.ones(n), sgn, np.ones(n)], axis=1)
    eul = eul * np.stack([sgn, np.ones(n), sgn], axis=1)
    cur = rng.uniform(-0.6, 0.6, size=(n, 7))
    far = np.arange(n) % far_every == 3
    cur[far] = rng.uniform(-5 * np.pi, 5 * np.pi, size=(int(far.sum()), 7))
    short = np.flatnonzero(np.arange(n) % shortcut_every == 5)
    noise = rng.uniform(-1e-3, 1e-3, size=(len(short), 7))
    turns = rng.integers(-2, 3, size=(len(short), 7)) * (rng.uniform(size=(len(short), 1)) < 0.5)
    arms = arms or (orc.Arm("r_arm", so), orc.Arm("l_arm", so))
    for k, i in enumerate(short):
        sv = orc.Solver(arms[byte[i]])
        if sv.is_reachable_no_limits(pos[i], eul[i]):
            j, _, _ = sv.get_joints(PREFERRED[byte[i]])
            cur[i] = j + noise[k] + 2 * np.pi * turns[k]
    return pos, eul, byte, cur


def replay(sv, cur, arm_byte, pref, flip=None):
    """utils.py:267-331 in Python on a checker solver object `sv` (after is_reachable_no_limits), evaluation by evaluation.
    Returns dict(theta, low, high, shortcut, joints, distance, margins): margins[k] = |lhs - rhs| of the k-th comparison
    (k = 0: distance(preferred) against the tolerance; k >= 1: f1 against f2).  flip = k reverses that one comparison."""
    low, high = BRACKET0[int(arm_byte)]
    margins = []
    j, _, proj = sv.get_joints(pref)
    d = distance(j, cur)
    margins.append(abs(d - TOLERANCE))
    if (d < TOLERANCE) != (flip == 0):
        return dict(theta=pref, low=np.nan, high=np.nan, shortcut=True, joints=j, distance=d, margins=margins, projected=proj)
    while (high - low) > TOLERANCE:
        mid1 = low + (high - low) / 3
        mid2 = high - (high - low) / 3
        j1, _, _ = sv.get_joints(mid1)
        j2, _, _ = sv.get_joints(mid2)
        f1, f2 = distance(j1, cur), distance(j2, cur)
        margins.append(abs(f1 - f2))
        if (f1 < f2) != (flip == len(margins) - 1):
            high = mid2
        else:
            low = mid1
    best = (low + high) / 2
    j, _, proj = sv.get_joints(best)
    return dict(theta=best, low=low, high=high, shortcut=False, joints=j, distance=distance(j, cur), margins=margins, projected=proj)


def replay_row(arms, pos, eul, arm_byte, cur, pref, flip=None):
    sv = orc.Solver(arms[int(arm_byte)])
    assert sv.is_reachable_no_limits(pos, eul)
    out = replay(sv, cur, arm_byte, pref, flip=flip)
    out["solver"] = sv.buf.copy()
    return out


def near_ties(arms, pos, eul, arm, cur, pref=PREFERRED, rows=None):
    """Rows whose replayed search holds a comparison with sides closer than NEAR_TIE."""
    found = []
    for i in (range(len(pos)) if rows is None else rows):
        r = replay_row(arms, pos[i], eul[i], arm[i], cur[i], pref[int(arm[i])])
        if min(r["margins"]) <= NEAR_TIE:
            found.append(int(i))
    return found


def checker_batch(so, pos, eul, arm, cur, pref=PREFERRED, arms=None):
    """The checker's answer row by row (orc_get_best_theta_to_current_joints on one solver object per row, threads over
    chunks): ok [n] (is_reachable_no_limits), theta [n], shortcut [n], moved [n] (a projection moved the solver state during
    the search), joints [n,7] and distance [n] of the last evaluation for the rows that did not move (get_joints at the
    returned theta is then the same computation again), solver [n,19] (the object after the search).  arms: the checker's (r, l)
    arms, the default arms with offset `so` where None."""
    n = len(pos)
    out = dict(ok=np.zeros(n, dtype=bool), theta=np.full(n, np.nan), shortcut=np.zeros(n, dtype=bool), moved=np.zeros(n, dtype=bool),
               joints=np.full((n, 7), np.nan), distance=np.full(n, np.nan), solver=np.zeros((n, 19)))

    def work(lo, hi, arms=arms):
        arms = arms or (orc.Arm("r_arm", so), orc.Arm("l_arm", so))
        sv = [orc.Solver(a) for a in arms]
        for i in range(lo, hi):
            s = sv[int(arm[i])]
            s.buf = out["solver"][i]
            if not s.is_reachable_no_limits(pos[i], eul[i]):
                continue
            out["ok"][i] = True
            before = s.buf.copy()
            p = pref[int(arm[i])]
            j0, _, _ = s.get_joints(p)
            out["shortcut"][i] = distance(j0, cur[i]) < TOLERANCE
            s.buf[:] = before
            out["theta"][i] = s.best_theta_to_current_joints(cur[i], p)
            out["moved"][i] = not np.array_equal(s.buf[:9], before[:9])
            if not out["moved"][i]:
                keep = s.buf.copy()
                j, _, _ = s.get_joints(out["theta"][i])
                out["joints"][i] = j
                out["distance"][i] = distance(j, cur[i])
                s.buf[:] = keep

    step = max(1, (n + NTHREADS - 1) // NTHREADS)
    with ThreadPoolExecutor(NTHREADS) as ex:
        list(ex.map(lambda lo: work(lo, min(n, lo + step)), range(0, n, step)))
    return out


_BRACKETS = {}


def bracket_table(arm_byte):
    """Every (theta, low, high) the search can end in for this arm: its bracket starts from constants and each of its 16
    iterations takes one of two branches, so there are 2^16 ends, computed with the search's own float operations
    (utils.py:302-323).  Sorted by theta."""
    if arm_byte not in _BRACKETS:
        low, high = (np.array([v]) for v in BRACKET0[int(arm_byte)])
        while ((high - low) > TOLERANCE).any():
            assert ((high - low) > TOLERANCE).all()
            mid1 = low + (high - low) / 3
            mid2 = high - (high - low) / 3
            low, high = np.concatenate([low, mid1]), np.concatenate([mid2, high])
        theta = (low + high) / 2
        order = np.argsort(theta, kind="stable")
        _BRACKETS[arm_byte] = (theta[order], low[order], high[order])
    return _BRACKETS[arm_byte]


def bracket_of(theta, arm):
    """The final (low, high) of the searches that returned `theta` (looked up by the checker's theta: exact)."""
    out = np.full((len(theta), 2), np.nan)
    for a in (0, 1):
        m = np.flatnonzero((np.asarray(arm) == a) & np.isfinite(theta))
        if len(m) == 0:
            continue
        th, lo, hi = bracket_table(a)
        k = np.clip(np.searchsorted(th, theta[m]), 0, len(th) - 1)
        hit = th[k] == theta[m]
        out[m[hit], 0], out[m[hit], 1] = lo[k[hit]], hi[k[hit]]
    return out
