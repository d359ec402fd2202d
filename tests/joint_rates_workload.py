"""Inputs, the NumPy reference and the derived tolerance of the rsik_joint_rates tests (tests/test_joint_rates_abi.py pins them on the
CPU alone, tests/test_gpu_joint_rates.py holds the device to them).  No test in this file.

Joints, arm bytes, pairs and the reference Jacobian are jacobian_workload's.  Twists and biases are seeded, uniform in [-1, 1].  The
reference is numpy.linalg.lstsq per row on the stacked 13 x 7 system [J; lambda I] z = [v - J q0; 0], corrected once through its own
gradient with two more lstsq calls (reference() says why), rates = q0 + z: it never forms the normal equations the device solves.

The per-row tolerance (2-norm of the row's error in `rates`) is derived, not tuned:

    tol_row = sqrt(42) e_J (|y| + g (|q0| + 2 |J|_2 |y|)) + 128 * 2^-53 * kappa_2(A) |z|

with A = J J^T + lambda^2 I, y = A^-1 (v - J q0), z = J^T y, g = max_i sigma_i / (sigma_i^2 + lambda^2),
kappa_2(A) = (sigma_1^2 + lambda^2) / (sigma_6^2 + lambda^2), all from the SVD of the reference J.  The first term is the effect of J
being known to e_J = 1e-13 per entry (test_gpu_jacobian.J_TOL; sqrt(42) e_J = 6.5e-13 bounds the 2-norm of the error of J): z = J^T y
moves by dJ^T y, and y by A^-1 (dJ q0 + (dJ J^T + J dJ^T) y), which J^T maps with gain g.  The second is forming A (gamma_7) plus the
factorisation's backward error (gamma_19 * 6) through kappa(A).  For achieved_twist: |J|_2 tol_row + sqrt(42) e_J |rates|."""
import functools
import math

import numpy as np

import far_inputs as FI
import jacobian_workload as JW

LAMBDAS = (1e-3, 0.05, 1.0)
TINY_LAMBDA = 1e-7
J_ENTRY = 1e-13          # what the device's J is held to, per entry
FAR_J_ENTRY = 1e-9       # ... for a row with a far angle (include/rsik.h: answered like its reduced twin to 1e-9)
WOUND_J_ENTRY = 2e-13    # ... for the wound set: test_gpu_jacobian allows 1e-13 more against the unwound rows
EPS = 2.0 ** -53
PAIRS = JW.PAIRS


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def twists(n=JW.N_SET):
    return _frozen(np.random.default_rng(7201).uniform(-1.0, 1.0, size=(n, 6)))


@functools.lru_cache(maxsize=None)
def biases(n=JW.N_SET):
    return _frozen(np.random.default_rng(7202).uniform(-1.0, 1.0, size=(n, 7)))


def jacobian_rows(blocks, joints, arm):
    """The reference J [n,6,7] of joints [n,7] with one arm byte per row."""
    q, arm = np.asarray(joints, dtype=np.float64), np.asarray(arm)
    J = np.zeros((len(q), 6, 7))
    for side in (0, 1):
        rows = np.flatnonzero(arm == side)
        if len(rows):
            J[rows] = JW.jacobian(blocks[side], q[rows])
    return J


def _per_row(lam, n):
    return np.broadcast_to(np.asarray(lam, dtype=np.float64), (n,))


def reference(J, v, lam, q0=None):
    """rates [n,7] and achieved_twist [n,6] by lstsq per row on M z = b, M = [J; lambda I], b = [v - J q0; 0]; lam a number or [n].
    lstsq's answer is corrected once through its own gradient: g = M^T (b - M z), formed in long double, then
    z += lstsq(M, lstsq(M^T, g)) = (M^T M)^-1 g, still without forming M^T M.  Why: lstsq alone is backward stable for a perturbation
    of M of size eps |M|, which moves z by eps kappa(M) (|z| + kappa(M) |residual| / |M|), kappa(M) = sqrt(sigma_1^2 + lambda^2) /
    lambda whatever J is (the stacked matrix has the singular value lambda along the null direction of J).  Two places show it:
    at a straight or nearly straight elbow and lambda = 1e-3 the residual is of order 1 and lstsq alone sits at 5.1 and 3.4 times
    64 eps sqrt(kappa_2(A)) |z| against a 40-digit solve; at lambda = 1e-7, kappa(M) = 2e7, it is off by 1.4e-9 = 2.8 tol_row on row 243
    of the uniform set on the ztip arm, where the 40-digit solve and the device agree to 5e-15.  The gradient vanishes at the
    solution, so what the two lstsq calls of the correction lose is relative to the correction, not to z: after one step the error
    against 40 digits is 5e-15 and 6e-15 on the two sets at 1e-3 and 5e-15 on that row (a second step changes nothing)."""
    n = len(J)
    lam = _per_row(lam, n)
    q0 = np.zeros((n, 7)) if q0 is None else np.asarray(q0, dtype=np.float64)
    rates = np.empty((n, 7))
    M, b = np.zeros((13, 7)), np.zeros(13)
    for i in range(n):
        M[:6] = J[i]
        M[6:] = lam[i] * np.eye(7)
        b[:6] = v[i] - J[i] @ q0[i]
        z = np.linalg.lstsq(M, b, rcond=None)[0]
        Ml = M.astype(np.longdouble)
        g = (Ml.T @ (b.astype(np.longdouble) - Ml @ z.astype(np.longdouble))).astype(np.float64)
        z += np.linalg.lstsq(M, np.linalg.lstsq(M.T, g, rcond=None)[0], rcond=None)[0]
        rates[i] = q0[i] + z
    return dict(rates=rates, achieved_twist=np.einsum("nij,nj->ni", J, rates))


def tolerances(J, v, lam, q0=None, j_entry=J_ENTRY):
    """dict of tol_row [n] (rates), tol_achieved [n], and the parts: first, second (the two terms of tol_row), g, kappa, y_norm,
    z_norm, J_norm, residual_norm (|v - J q0|)."""
    n = len(J)
    lam = _per_row(lam, n)
    q0 = np.zeros((n, 7)) if q0 is None else np.asarray(q0, dtype=np.float64)
    U, s, Vt = np.linalg.svd(J, full_matrices=False)       # U [n,6,6], s [n,6], Vt [n,6,7]
    r = v - np.einsum("nij,nj->ni", J, q0)
    l2 = (lam * lam)[:, None]
    c = np.einsum("nji,nj->ni", U, r)                      # U^T r
    y = np.einsum("nij,nj->ni", U, c / (s * s + l2))
    z = np.einsum("nji,nj->ni", Vt, s * c / (s * s + l2))
    g = (s / (s * s + l2)).max(axis=1)
    kappa = (s[:, 0] ** 2 + l2[:, 0]) / (s[:, 5] ** 2 + l2[:, 0])
    yn, zn, qn = np.linalg.norm(y, axis=1), np.linalg.norm(z, axis=1), np.linalg.norm(q0, axis=1)
    e = math.sqrt(42.0) * j_entry
    first = e * (yn + g * (qn + 2.0 * s[:, 0] * yn))
    second = 128.0 * EPS * kappa * zn
    tol = first + second
    rates_norm = np.linalg.norm(q0 + z, axis=1)
    return dict(tol_row=tol, tol_achieved=s[:, 0] * tol + e * rates_norm, first=first, second=second, g=g, kappa=kappa, y_norm=yn,
                z_norm=zn, J_norm=s[:, 0], residual_norm=np.linalg.norm(r, axis=1))


def restatement(J, v, lam, q0=None, clamp=True):
    """The kernel's algorithm in float64 NumPy, all rows at once: A = J J^T + lambda^2 I, L D L^T in natural order with every pivot
    clamped from below at lambda^2 (clamp=False: not), the two triangular solves, rates = q0 + J^T y.  (Not its bits: NumPy does not
    fuse.)  Returns rates [n,7]."""
    n = len(J)
    lam = _per_row(lam, n)
    l2 = lam * lam
    q0 = np.zeros((n, 7)) if q0 is None else np.asarray(q0, dtype=np.float64)
    y = v - np.einsum("nij,nj->ni", J, q0)
    A = np.einsum("nik,njk->nij", J, J)
    A[:, range(6), range(6)] += l2[:, None]
    L = np.zeros((n, 6, 6))
    d = np.zeros((n, 6))
    with np.errstate(all="ignore"):
        for j in range(6):
            w = L[:, j, :j] * d[:, :j]
            dj = A[:, j, j] - (L[:, j, :j] * w).sum(axis=1)
            d[:, j] = np.maximum(dj, l2) if clamp else dj
            for i in range(j + 1, 6):
                L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * w).sum(axis=1)) / d[:, j]
        y = y.copy()
        for i in range(1, 6):
            y[:, i] -= (L[:, i, :i] * y[:, :i]).sum(axis=1)
        y /= d
        for i in range(4, -1, -1):
            y[:, i] -= (L[:, i + 1:, i] * y[:, i + 1:]).sum(axis=1)
        return q0 + np.einsum("nij,ni->nj", J, y)


def mp_rates(J, v, lam, q0=None, dps=40):
    """rates [n,7] from the 7 x 7 normal equations (J^T J + lambda^2 I) z = J^T (v - J q0) solved in mpmath at `dps` digits."""
    import mpmath as mp

    n = len(J)
    lam = _per_row(lam, n)
    q0 = np.zeros((n, 7)) if q0 is None else np.asarray(q0, dtype=np.float64)
    out = np.empty((n, 7))
    with mp.workdps(dps):
        for i in range(n):
            Jm = mp.matrix(J[i].tolist())
            r = mp.matrix(v[i].tolist()) - Jm * mp.matrix(q0[i].tolist())
            N = Jm.T * Jm + mp.mpf(float(lam[i])) ** 2 * mp.eye(7)
            z = mp.lu_solve(N, Jm.T * r)
            out[i] = [float(mp.mpf(float(q0[i, k])) + z[k]) for k in range(7)]
    return out


@functools.lru_cache(maxsize=None)
def far_rows():
    """test_gpu_jacobian.far_rows rebuilt (a test file must not be imported): one joint of a uniform row at a rung of
    tests/far_inputs.py (2^27, 1e15: wound by whole turns; 1e300: the double itself), each joint and each sign in turn, and the
    reduced twin of every row: (far [42,7], twin [42,7])."""
    base = JW.joint_set("uniform")
    far, twin = [], []
    for g, rung in enumerate((2.0 ** 27, 1e15, 1e300)):
        assert rung in FI.RUNGS
        for k in range(7):
            for s, sign in enumerate((1.0, -1.0)):
                row = base[(g * 7 + k) * 2 + s].copy()
                x = FI.wind(row[k], rung, sign) if rung < FI.WALKED_FROM else FI.walked(rung, sign, 0.0)[0][k]
                t = row.copy()
                row[k], t[k] = x, FI.reduce_angle(x)
                assert abs(x) >= rung / 2 and abs(t[k]) <= math.pi
                far.append(row); twin.append(t)
    return _frozen(np.array(far)), _frozen(np.array(twin))


# ------------------------------------------------------------------------------------------ references shared by the tests
@functools.lru_cache(maxsize=None)
def side_jacobians(pair, set_name):
    """(J of every row of a named set on the r block, on the l block): the reference J of any arm arrangement is a row-wise pick."""
    blocks = JW.blocks_of(pair)
    q = JW.joint_set(set_name)
    return tuple(_frozen(JW.jacobian(blocks[side], q)) for side in (0, 1))


@functools.lru_cache(maxsize=None)
def side_case(pair, set_name, lam, bias, j_entry=J_ENTRY):
    """The reference and the tolerances of every row of a named set at one lambda, with or without the seeded bias, on each block:
    a pair (r, l) of dicts with rates, achieved_twist, tol_row, tol_achieved and the tolerance's parts.  Computed once."""
    out = []
    v, q0 = twists(), (biases() if bias else None)
    for J in side_jacobians(pair, set_name):
        d = reference(J, v, lam, q0)
        d.update(tolerances(J, v, lam, q0, j_entry=j_entry))
        out.append({k: _frozen(a) for k, a in d.items()})
    return tuple(out)


def pick(case, arm, rows, key):
    """Rows `rows` (flat indices into the named set) of a side_case entry `key`, each from the block its arm byte names."""
    arm, rows = np.asarray(arm), np.asarray(rows)
    sel = arm.reshape((-1,) + (1,) * (case[0][key].ndim - 1)) == 1
    return np.where(sel, case[1][key][rows], case[0][key][rows])
