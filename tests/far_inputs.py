"""Finite inputs far outside the ranges the device math was written for: Euler angles, elbow angles and previous joints wound
up to DBL_MAX, positions up to DBL_MAX and down to the smallest denormal.  Deterministic (NumPy + mpmath); shared by
oracle/gen_golden.py (G22), tests/test_oracle_golden.py, tests/test_far_inputs_checker.py and tests/test_gpu_far_inputs.py.
No test in this file."""
import functools
import math

import mpmath as mp
import numpy as np

from rotations import euler_to_matrix

DBL_MAX = float(np.finfo(np.float64).max)
# fast_sincos takes its table row from (int)rint(x * 32 / pi): the integer leaves 32 bits at |x| = 2^31 pi / 32 = 2^26 pi.  The double
# nearest to that real number is 2^26 fl(pi), which lies BELOW it (fl(pi) < pi): EDGE itself is the last double in range.
EDGE = 2.0 ** 26 * math.pi
# (4e15 lies between 2^50, up to where the device's modulo has a quotient within one of the true one, and 2^53)
RUNGS = (7.0, 1e2, 1e4, 1e5, 1e6, 2.0 ** 27, 2.0e8, math.nextafter(EDGE, 0.0), math.nextafter(EDGE, math.inf), 2.2e8, 1e9, 1e12,
         1e15, 4e15, 1e16, 1e18, 1e22, 1e100, 1e300, DBL_MAX)
# the two rungs at the edge are wound to their own side of it: no further from zero than the one, no nearer than the other
SIDE = {math.nextafter(EDGE, 0.0): -1, math.nextafter(EDGE, math.inf): 1}
WALKED_FROM = 1e16       # from here on one ulp is more than a radian: the angle is found by walking doubles, not by adding turns
FIRST_BROKEN = 8         # index of the first rung above 2^31 pi / 32
BOUND_RUNG = 5           # index of 2^27
N_BASE = 32
SPREAD_POS, SPREAD_EUL = 0.08, 0.4
CENTRE_POS = np.array([0.38, -0.2, -0.28])
CENTRE_EUL = np.array([0.0, -np.pi / 2, 0.0])
SINGULARITY_OFFSET = 0.03
FAR_POSITIONS = (1e3, 1e10, 1e100, 1e154, 2e154, 1e300, DBL_MAX)
TINY_POSITIONS = (0.0, 5e-324, 1e-300)


def reduce_angle(x):
    """The double nearest to x - 2 pi round(x / 2 pi), in mpmath at log10|x| + 40 digits (60 at least)."""
    x = float(x)
    if abs(x) <= math.pi:
        return x
    with mp.workdps(max(60, int(math.log10(abs(x))) + 41)):
        t = mp.mpf(x)
        two_pi = 2 * mp.pi
        return float(t - two_pi * mp.nint(t / two_pi))


def reduce_angles(a):
    a = np.asarray(a, dtype=np.float64)
    return np.array([reduce_angle(v) for v in a.ravel()]).reshape(a.shape)


def wind(base, rung, sign):
    """The double nearest to base + round(sign * rung / 2 pi) * 2 pi (rungs below WALKED_FROM).  At the two rungs of SIDE the
    number of turns is the largest that keeps |value| <= rung, or the smallest that keeps |value| >= rung."""
    side = SIDE.get(rung, 0)
    with mp.workdps(60):
        two_pi = 2 * mp.pi
        b, t = mp.mpf(float(base)), sign * mp.mpf(rung)
        if side == 0:
            return float(b + mp.nint(t / two_pi) * two_pi)
        k = (t - b) / two_pi
        k = mp.floor(k) if side * sign < 0 else mp.ceil(k)
        v = float(b + k * two_pi)
        while side < 0 and abs(v) > rung:      # (the rounding to double may step across: one more turn)
            k -= sign
            v = float(b + k * two_pi)
        while side > 0 and abs(v) < rung:
            k += sign
            v = float(b + k * two_pi)
        return v


@functools.lru_cache(maxsize=None)
def walked(rung, sign, centre, count=N_BASE, within=SPREAD_EUL):
    """The first `count` doubles, walking from sign * rung away from zero (towards zero from DBL_MAX), whose reduction lies within
    `within` rad of `centre`: (doubles, reductions)."""
    x = sign * rung
    towards = 0.0 if rung == DBL_MAX else sign * math.inf
    xs, rs = [], []
    while len(xs) < count:
        r = reduce_angle(x)
        if abs(r - centre) <= within:
            xs.append(x)
            rs.append(r)
        x = math.nextafter(x, towards)
    return tuple(xs), tuple(rs)


def base_poses(arm="r_arm", n=N_BASE, seed=2200):
    rng = np.random.default_rng(seed)
    pos = CENTRE_POS + rng.uniform(-SPREAD_POS, SPREAD_POS, size=(n, 3))
    eul = CENTRE_EUL + rng.uniform(-SPREAD_EUL, SPREAD_EUL, size=(n, 3))
    return mirror(pos, eul) if arm == "l_arm" else (pos, eul)


def mirror(pos, eul):
    """r <-> l: y, roll and yaw change sign (exact in binary64, so a wound angle's mirror image is wound the same way)."""
    return pos * np.array([1.0, -1.0, 1.0]), eul * np.array([-1.0, 1.0, -1.0])


@functools.lru_cache(maxsize=None)
def _wound_rows_r():
    pos0, eul0 = base_poses("r_arm")
    P, E, T, G, S, L = [], [], [], [], [], []
    for g, rung in enumerate(RUNGS):
        for sign in (1.0, -1.0):
            for b in range(N_BASE):
                slot = (b + g) % 4          # 0, 1, 2: that Euler entry; 3: all three at once
                e, t = eul0[b].copy(), eul0[b].copy()
                for q in ((0, 1, 2) if slot == 3 else (slot,)):
                    if rung < WALKED_FROM:
                        e[q] = wind(eul0[b, q], rung, sign)
                        t[q] = reduce_angle(e[q])
                    else:
                        xs, rs = walked(rung, sign, float(CENTRE_EUL[q]))
                        e[q], t[q] = xs[b], rs[b]
                P.append(pos0[b]); E.append(e); T.append(t); G.append(g); S.append(sign); L.append(slot)
    return (np.array(P), np.array(E), np.array(T), np.array(G, dtype=np.int64), np.array(S), np.array(L, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def _wound_rows_cached():
    pos, eul, twin, rung, sign, slot = _wound_rows_r()
    n = len(pos)
    lp, le = mirror(pos, eul)
    _, lt = mirror(pos, twin)
    out = {}
    # r and l rows interleaved: both arms in every wave
    for key, a, b in (("pos", pos, lp), ("eul", eul, le), ("twin_eul", twin, lt), ("rung", rung, rung), ("slot", slot, slot),
                      ("sign", sign, sign)):
        out[key] = np.stack([a, b], axis=1).reshape((2 * n,) + a.shape[1:])
    # the sign of the wound VALUE: the mirror image flips roll and yaw, so slot 1 keeps it and the others change it
    flip = np.stack([np.zeros(n, dtype=bool), slot != 1], axis=1).reshape(-1)
    out["sign"] = np.where(flip, -out["sign"], out["sign"])
    out["arm"] = np.tile(np.array([0, 1], dtype=np.uint8), n)
    for v in out.values():
        v.setflags(write=False)
    return out


def wound_rows():
    """Pose rows with wound Euler angles: pos [n,3], eul [n,3], twin_eul [n,3] (the reduced twin's angles), arm [n] uint8,
    rung [n] (index into RUNGS), sign [n] (of the wound value in slots 0-2, of roll and yaw where slot is 3) and slot [n]
    (0-2, 3 = all three)."""
    return _wound_rows_cached()


@functools.lru_cache(maxsize=None)
def _far_thetas_cached():
    base = np.random.default_rng(2201).uniform(-np.pi, np.pi, size=len(RUNGS) * 2)
    th, tw, rg = [], [], []
    for g, rung in enumerate(RUNGS):
        for s, sign in enumerate((1.0, -1.0)):
            if rung < WALKED_FROM:
                x = wind(base[2 * g + s], rung, sign)
            else:
                x = sign * rung
            th.append(x); tw.append(reduce_angle(x)); rg.append(g)
    out = (np.array(th), np.array(tw), np.array(rg, dtype=np.int64))
    for v in out:
        v.setflags(write=False)
    return out


def far_thetas():
    """One angle per rung and sign: theta, its reduced twin, rung index.  From WALKED_FROM up the rung itself."""
    return _far_thetas_cached()


def position_rows(values, per_arm=4, together=True, signed_zero=False):
    """Each position entry in turn (and all three together) at +-v for v in values, the other entries at their base value:
    pos [n,3], eul [n,3], arm [n], value [n] (signed), entry [n] (0-2, 3 = all three)."""
    P, E, A, V, N = [], [], [], [], []
    for a, arm in enumerate(("r_arm", "l_arm")):
        pos0, eul0 = base_poses(arm)
        for v in values:
            for sign in (1.0, -1.0):
                for entry in range(4 if together else 3):
                    for b in range(per_arm):
                        p = pos0[b].copy()
                        if entry == 3:
                            p[:] = sign * v
                        else:
                            p[entry] = sign * v
                        P.append(p); E.append(eul0[b]); A.append(a); V.append(sign * v); N.append(entry)
    order = np.argsort(np.arange(len(P)) % (len(P) // 2), kind="stable")  # r and l rows interleaved
    return (np.array(P)[order], np.array(E)[order], np.array(A, dtype=np.uint8)[order], np.array(V)[order],
            np.array(N, dtype=np.int64)[order])


def far_position_rows():
    return position_rows(FAR_POSITIONS)


def tiny_position_rows():
    return position_rows(TINY_POSITIONS, together=False)


def preferred_theta_goals(per_arm=16):
    """Ordinary goals for the launches that take a far preferred_theta: pos [n,3], eul [n,3], arm [n], r and l interleaved."""
    pr, er = base_poses("r_arm")
    pl, el = base_poses("l_arm")
    pos = np.stack([pr[:per_arm], pl[:per_arm]], axis=1).reshape(-1, 3)
    eul = np.stack([er[:per_arm], el[:per_arm]], axis=1).reshape(-1, 3)
    return pos, eul, np.tile(np.array([0, 1], dtype=np.uint8), per_arm)


def goal_matrices(pos, eul):
    """Proper goal matrices [n,4,4]: the rotation of the (ordinary) Euler angles, pos as the translation column."""
    M = np.tile(np.eye(4), (len(pos), 1, 1))
    M[:, :3, :3] = euler_to_matrix(eul)
    M[:, :3, 3] = pos
    return M
