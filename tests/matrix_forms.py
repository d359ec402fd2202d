"""Goal matrices whose rotation block is not a rotation: seeded families of 3x3 blocks, and a 50-digit reference of what the
matrix -> Euler conversion should make of them.  NumPy and mpmath only (oracle/gen_golden.py imports this beside the reference, for
G23); nothing here touches the product, the checker or a GPU.  No test in this file.

What the conversion is (utils.py:84-90, SciPy's Rotation.from_matrix(...).as_euler("xyz")): a block with det <= 0 raises ValueError;
any other block stands for the nearest rotation, the orthogonal polar factor U V^T of its SVD.  The reference here is that factor
from mpmath.svd_r at 50 digits, and the Euler xyz angles read from it.  Angles are always compared as rotation matrices
(rotation_error): wrap-around and the free angle at gimbal lock do not matter.

Range: no entry is larger than 1e100 in magnitude, and every singular value of a block that has a positive or a negative
determinant lies in [1e-100, 1e100] (s R with s = 1e-100 has entries below 1e-100, its singular values are 1e-100), so that no
product of three entries overflows and no determinant vanishes (include/rsik.h "Goal matrices that are not rotations" states the
same range).

Families, ROWS = 3 * 64 + 1 blocks each (three full waves and a ragged lane):
  scaled       s R, s = 10^e, e in +-{1, 3, 5, 6, 7, 12, 30, 100}: both sides of where 24 unscaled Newton steps gave out (1e+-6).
  one_small    R1 diag(1, 1, c) R2, c = 10^-k, k = 1..8; and R1 diag(s, s, s c) R2, scale and flatness together.
  two_small    R1 diag(1, c, c) R2, c in {1e-1, 1e-2, 1e-3, 1e-4}: the polar factor's condition is 2 / (sigma_2 + sigma_3) = 1 / c,
               and the family's tolerance grows with it by itself (REF_ERR is SciPy's own error on the family).
  sheared      R (I + eps N), N fixed, eps in {1e-13, 1e-11, 1e-9, 1e-6, 1e-3, 0.1, 0.5}; blocks whose largest off-diagonal Gramian
               entry is (1 +- 1e-3) 1e-12 and pure scalings whose diagonal Gramian error is (1 +- 1e-3) 1e-5: both sides of the two
               thresholds of "already a rotation" (np.isclose(M M^T, I, atol=1e-12)).  The two branches differ by at most the
               threshold there, so one tolerance serves both sides.
  locked       scaled and sheared blocks of rotations whose pitch is within {0, 1e-9, 6e-8, 1.5e-7} of +-pi/2.
  left_handed  R diag(1, 1, -1), -R, odd permutation matrices, those times s in {1e-7, 1, 1e8}, sheared reflections (eps <= 0.1):
               det <= -1e-3 |r0| |r1| |r2|, so that no rounding order changes its sign.
  singular     det exactly 0 in any evaluation order: the zero block, a zero row, a zero column, two equal rows, rank 1; every entry
               a small integer times a power of two, so that every product and every sum of any evaluation is exact.
For the first five, det >= 1e-9 |r0| |r1| |r2| (check_family asserts all of it)."""
import functools

import numpy as np

from rotations import euler_to_matrix

SEED = 23
ROWS = 3 * 64 + 1
PROPER = ("scaled", "one_small", "two_small", "sheared", "locked")
IMPROPER = ("left_handed", "singular")
FAMILIES = PROPER + IMPROPER
N_ORDINARY = 256          # ordinary goals per arm that the family rows are interleaved with (G23 records their poses)

SCALE_EXPONENTS = (1, -1, 3, -3, 5, -5, 6, -6, 7, -7, 12, -12, 30, -30, 100, -100)
SHEAR_EPS = (1e-13, 1e-11, 1e-9, 1e-6, 1e-3, 0.1, 0.5)
LOCK_DELTAS = (0.0, 1e-9, 6e-8, 1.5e-7)

# SciPy 1.15.3's double-precision answer against the 50-digit reference, per family, as max |R(eul_scipy) - R(eul_ref)| over the
# family's rows: the reference's OWN error, measured by tests/test_matrix_forms_checker.py::test_scipy_against_mpmath (which prints
# it and holds it to these figures: measured 9.99e-16, 9.47e-15, 7.64e-13, 2.43e-6, 2.50e-6, rounded up with room for a last-bit
# difference in the sines and cosines of the comparison itself) — never taken from the device or the checker.
REF_ERR = {
    "scaled": 1.2e-15,
    "one_small": 1.0e-14,
    "two_small": 7.7e-13,
    "sheared": 2.5e-6,
    "locked": 2.6e-6,
}
EULER_FLOOR = 1e-12      # G8's bound on the conversion


def tolerance(family):
    """Euler angles as rotations: max(1e-12, 8 REF_ERR[family]).  The factor 8: the device's iteration and LAPACK's SVD round along
    different paths, each at condition x epsilon."""
    return max(EULER_FLOOR, 8.0 * REF_ERR[family])


# ------------------------------------------------------------------------------------------ the families
def _rotations(rng, n):
    """n proper rotations from uniform unit quaternions, orthonormal to rounding."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    Rm = np.empty((n, 3, 3))
    Rm[:, 0, 0] = 1 - 2 * (y * y + z * z); Rm[:, 0, 1] = 2 * (x * y - z * w); Rm[:, 0, 2] = 2 * (x * z + y * w)
    Rm[:, 1, 0] = 2 * (x * y + z * w); Rm[:, 1, 1] = 1 - 2 * (x * x + z * z); Rm[:, 1, 2] = 2 * (y * z - x * w)
    Rm[:, 2, 0] = 2 * (x * z - y * w); Rm[:, 2, 1] = 2 * (y * z + x * w); Rm[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return Rm


def _mm(*factors):
    """The product of 3x3 matrices by explicit multiplies and left-to-right sums: the same bits on every CPU (a BLAS product may
    fuse or reorder them), so that G23's recorded answers belong to the blocks every machine builds."""
    out = np.asarray(factors[0], dtype=np.float64)
    for B in factors[1:]:
        B = np.asarray(B, dtype=np.float64)
        out = np.array([[out[i, 0] * B[0, j] + out[i, 1] * B[1, j] + out[i, 2] * B[2, j] for j in range(3)] for i in range(3)])
    return out


def _shear_matrix():
    return np.random.default_rng(SEED + 100).uniform(-1.0, 1.0, size=(3, 3))


def _scaled(rng, Rm):
    s = 10.0 ** np.array([SCALE_EXPONENTS[i % len(SCALE_EXPONENTS)] for i in range(len(Rm))], dtype=np.float64)
    return Rm * s[:, None, None]


def _sheared(rng, Rm):
    n = len(Rm)
    N = _shear_matrix()
    out = np.empty_like(Rm)
    for i in range(n):
        kind = i % (len(SHEAR_EPS) + 4)
        if kind < len(SHEAR_EPS):
            out[i] = _mm(Rm[i], np.eye(3) + SHEAR_EPS[kind] * N)
        elif kind < len(SHEAR_EPS) + 2:
            # S R with S = I + a (e_p e_q^T + e_q e_p^T): the Gramian S S^T is I + 2 a K + a^2 K^2, its largest off-diagonal entry
            # 2 a = (1 +- 1e-3) 1e-12 (the entries' own rounding moves it by ~2e-16, a fifth of the margin)
            side = 1.0 + (1e-3 if kind == len(SHEAR_EPS) else -1e-3)
            p, q = [(0, 1), (0, 2), (1, 2)][(i // (len(SHEAR_EPS) + 4)) % 3]
            S = np.eye(3)
            S[p, q] = S[q, p] = 0.5e-12 * side
            out[i] = _mm(S, Rm[i])
        else:
            # s R with |s^2 - 1| = (1 +- 1e-3) 1e-5, s above and below 1 in turn
            side = 1.0 + (1e-3 if kind == len(SHEAR_EPS) + 2 else -1e-3)
            sign = 1.0 if (i // (len(SHEAR_EPS) + 4)) % 2 == 0 else -1.0
            out[i] = np.sqrt(1.0 + sign * 1e-5 * side) * Rm[i]
    return out


@functools.lru_cache(maxsize=None)
def blocks(family):
    """The family's [ROWS, 3, 3] blocks (float64, read-only): the same bytes in every process."""
    rng = np.random.default_rng([SEED, FAMILIES.index(family)])
    n = ROWS
    if family == "scaled":
        B = _scaled(rng, _rotations(rng, n))
    elif family == "one_small":
        R1, R2 = _rotations(rng, n), _rotations(rng, n)
        B = np.empty((n, 3, 3))
        mixes = [(s, c) for s in (1e-30, 1e-3, 1e3, 1e30) for c in (1e-2, 1e-5, 1e-8)]
        for i in range(n):
            if i % 3 < 2:
                s, c = 1.0, 10.0 ** -(1 + (i // 3 * 2 + i % 3) % 8)
            else:
                s, c = mixes[(i // 3) % len(mixes)]
            B[i] = _mm(R1[i], np.diag([s, s, s * c]), R2[i])
    elif family == "two_small":
        R1, R2 = _rotations(rng, n), _rotations(rng, n)
        B = np.empty((n, 3, 3))
        for i in range(n):
            c = (1e-1, 1e-2, 1e-3, 1e-4)[i % 4]
            B[i] = _mm(R1[i], np.diag([1.0, c, c]), R2[i])
    elif family == "sheared":
        B = _sheared(rng, _rotations(rng, n))
    elif family == "locked":
        eul = rng.uniform(-np.pi, np.pi, size=(n, 3))
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        eul[:, 1] = sign * (np.pi / 2 - np.array([LOCK_DELTAS[(i // 2) % len(LOCK_DELTAS)] for i in range(n)]))
        Rm = euler_to_matrix(eul)
        half = np.arange(n) % 3 == 0
        B = np.where(half[:, None, None], _scaled(rng, Rm), _sheared(rng, Rm))
    elif family == "left_handed":
        Rm = _rotations(rng, n)
        N = _shear_matrix()
        perms = [np.eye(3)[list(p)] for p in ((1, 0, 2), (0, 2, 1), (2, 1, 0))]
        B = np.empty((n, 3, 3))
        for i in range(n):
            kind, s = i % 4, (1.0, 1e-7, 1e8)[(i // 4) % 3]
            if kind == 0:
                B[i] = s * _mm(Rm[i], np.diag([1.0, 1.0, -1.0]))
            elif kind == 1:
                B[i] = s * -Rm[i]
            elif kind == 2:
                B[i] = s * perms[(i // 12) % 3]
            else:
                eps = (1e-9, 1e-3, 0.1)[(i // 12) % 3]
                B[i] = s * _mm(Rm[i], np.diag([1.0, -1.0, 1.0]), np.eye(3) + eps * N)
    elif family == "singular":
        B = np.zeros((n, 3, 3))
        for i in range(1, n):                                 # (row 0: the zero block)
            kind = (i - 1) % 4
            A = rng.integers(-4, 5, size=(3, 3)).astype(np.float64)
            if kind == 0:
                A[rng.integers(3)] = 0.0                      # a zero row
            elif kind == 1:
                A[:, rng.integers(3)] = 0.0                   # a zero column
            elif kind == 2:
                p, q = rng.permutation(3)[:2]
                A[q] = A[p]                                   # two equal rows
            else:
                u = 2.0 ** rng.integers(-2, 3, size=3) * rng.choice([-1.0, 1.0], size=3)
                A = np.outer(u, rng.integers(-4, 5, size=3).astype(np.float64))   # rank 1 (or 0), power-of-two row factors
            B[i] = A * 2.0 ** (-20, 0, 30)[(i // 4) % 3]
    else:
        raise KeyError(family)
    B = np.ascontiguousarray(B, dtype=np.float64)
    B.setflags(write=False)
    return B


def det_and_norms(B):
    """row 2 . (row 0 x row 1) and |r0| |r1| |r2| of [n,3,3] blocks, in float64."""
    det = np.einsum("ni,ni->n", B[:, 2], np.cross(B[:, 0], B[:, 1]))
    return det, np.prod(np.linalg.norm(B, axis=2), axis=1)


def check_family(family):
    """The conditions the family's docstring states, asserted."""
    B = blocks(family)
    assert B.shape == (ROWS, 3, 3) and np.isfinite(B).all(), family
    assert np.abs(B).max() <= 1e100, (family, np.abs(B).max())
    if family != "singular":
        sv = np.linalg.svd(B, compute_uv=False)
        assert sv.min() >= 1e-100 * (1 - 1e-9) and sv.max() <= 1e100 * (1 + 1e-9), (family, sv.min(), sv.max())
    det, norms = det_and_norms(B)
    if family in PROPER:
        assert (det >= 1e-9 * norms).all(), (family, float((det / norms).min()))
    elif family == "left_handed":
        assert (det <= -1e-3 * norms).all(), (family, float((det / norms).max()))
    else:
        assert (det == 0.0).all(), (family, det[det != 0.0][:4])
        # ... in any evaluation order: the cofactor expansion along each row and each column
        for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            for X in (B, np.transpose(B, (0, 2, 1))):
                d = np.einsum("ni,ni->n", X[:, perm[2]], np.cross(X[:, perm[0]], X[:, perm[1]]))
                assert (d == 0.0).all(), (family, perm)


# ------------------------------------------------------------------------------------------ the 50-digit reference
def _mp():
    import mpmath

    return mpmath


def exact_det_sign(B):
    """The sign (-1, 0, 1) of each block's determinant, computed exactly (50 digits hold every product of three doubles here)."""
    mp = _mp()
    out = np.zeros(len(B), dtype=np.int8)
    with mp.workdps(60):
        for i, A in enumerate(B):
            a = [[mp.mpf(float(x)) for x in row] for row in A]
            d = (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])
                 + a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))
            out[i] = int(mp.sign(d))
    return out


def _reference_one(A):
    mp = _mp()
    with mp.workdps(50):
        # (a power-of-two scale first: exact, and the polar factor does not see it; svd_r's own thresholds then see entries of order 1)
        top = float(np.max(np.abs(A)))
        e2 = int(np.floor(np.log2(top)))
        U, S, V = mp.svd_r(mp.matrix([[mp.mpf(float(x)) * mp.mpf(2) ** (-e2) for x in row] for row in A]))
        Q = U * V                                            # svd_r returns V^T: the orthogonal polar factor U V^T
        # extrinsic xyz angles of R = Rz(yaw) Ry(pitch) Rx(roll); at the lock the third angle is 0 (SciPy's convention; compared as rotations)
        sb = -Q[2, 0]
        cb = mp.sqrt(Q[0, 0] ** 2 + Q[1, 0] ** 2)
        pitch = mp.atan2(sb, cb)
        if cb > mp.mpf(10) ** -30:
            roll, yaw = mp.atan2(Q[2, 1], Q[2, 2]), mp.atan2(Q[1, 0], Q[0, 0])
        else:
            roll, yaw = mp.atan2(-Q[1, 2] * mp.sign(sb), Q[1, 1]) * mp.sign(sb), mp.mpf(0)
        eul = np.array([float(roll), float(pitch), float(yaw)])
        rot = np.array([[float(Q[i, j]) for j in range(3)] for i in range(3)])
    return eul, rot


@functools.lru_cache(maxsize=None)
def reference(family):
    """(euler [ROWS,3], rotation [ROWS,3,3]) of a proper family: the Euler xyz angles of the 50-digit polar factor, and that factor
    itself rounded to float64 — computed once per process, shared by the tests that need it, read-only."""
    assert family in PROPER, family
    got = [_reference_one(A) for A in blocks(family)]
    eul, rot = np.array([g[0] for g in got]), np.array([g[1] for g in got])
    eul.setflags(write=False)
    rot.setflags(write=False)
    return eul, rot


def rotation_error(eul_a, eul_b):
    """max |R(eul_a) - R(eul_b)| per row: how Euler angles are compared here (NaN where either row holds one)."""
    return np.max(np.abs(euler_to_matrix(eul_a) - euler_to_matrix(eul_b)), axis=(1, 2))


# ------------------------------------------------------------------------------------------ goal matrices and interleaving
def goal_matrices(B, pos):
    """[n,4,4] homogeneous matrices of blocks and translations."""
    M = np.tile(np.eye(4), (len(B), 1, 1))
    M[:, :3, :3] = B
    M[:, :3, 3] = pos
    return M


def family_matrices(g, arm):
    """{family: [ROWS,4,4]} for an arm ("r_arm" / "l_arm"): the family's blocks on the translations G23 recorded for them."""
    return {f: goal_matrices(blocks(f), g[f"{arm}_{f}_pos"]) for f in FAMILIES}


def ordinary_matrices(g, arm):
    """The arm's N_ORDINARY ordinary goals of G23: proper rotations (from their Euler angles) on reachable positions."""
    return goal_matrices(euler_to_matrix(g[f"{arm}_ordinary_eul"]), g[f"{arm}_ordinary_pos"])


def interleave(special, ordinary, seed=0):
    """Rows of `special` scattered among the rows of `ordinary` (both [k,...], same trailing shape) in a seeded random order that keeps
    each set's own order, so that rare-branch lanes share waves with ordinary lanes.  Returns (rows [ns + no, ...], index of each
    special row, index of each ordinary row)."""
    ns, no = len(special), len(ordinary)
    rng = np.random.default_rng([SEED, 7, seed, ns, no])
    where = np.sort(rng.permutation(ns + no)[:ns])
    rest = np.setdiff1d(np.arange(ns + no), where)
    out = np.empty((ns + no,) + special.shape[1:], dtype=special.dtype)
    out[where], out[rest] = special, ordinary
    return out, where, rest


# ------------------------------------------------------------------------------------------ against G23
INVALID_INPUT = 10       # RSIK_STATE_INVALID_INPUT / ORC_STATE_INVALID_INPUT
G23 = "g23_matrix_forms.npz"


def recorded_tolerance(family):
    """Euler angles against SciPy's own recorded answer (G23).  For sheared and locked REF_ERR is no rounding error: it is what SciPy's
    rule "a Gramian within np.isclose of the identity is a rotation already" costs on the blocks placed at its thresholds (2.5e-6 for a
    block scaled by 1 + 5e-6, whose quaternion is read from the block as it is).  An implementation of the same rule reproduces
    that, so against the recording those two families are held to G8's bound."""
    return EULER_FLOOR if family in ("sheared", "locked") else tolerance(family)


def check_euler(eul, g, arm, family, what):
    """Angles of the family's blocks from an implementation of the conversion: against the 50-digit reference and against G23 for a
    proper family (returns the two worst errors), NaN in every row that G23 records as raised."""
    pre = f"{arm}_{family}_"
    raised = g[pre + "euler_raised"].astype(bool)
    assert raised.all() if family in IMPROPER else not raised.any(), (what, family, "the recorded decisions")
    if family in IMPROPER:
        assert np.isnan(eul).all(), (what, family, "angles where the reference raises", np.flatnonzero(~np.isnan(eul).all(axis=1))[:8].tolist())
        return 0.0, 0.0
    assert np.isfinite(eul).all(), (what, family, "rows without angles", np.flatnonzero(~np.isfinite(eul).all(axis=1))[:8].tolist())
    e_ref = float(rotation_error(eul, reference(family)[0]).max())
    e_rec = float(rotation_error(eul, g[pre + "euler"]).max())
    print(f"{what} {arm} {family}: against mpmath {e_ref:.3e} (bound {tolerance(family):.1e}), against G23 {e_rec:.3e} "
          f"(bound {recorded_tolerance(family):.1e})")
    assert e_ref < tolerance(family), (what, family, "against the 50-digit reference", e_ref, tolerance(family))
    assert e_rec < recorded_tolerance(family), (what, family, "against G23", e_rec, recorded_tolerance(family))
    return e_ref, e_rec


def check_control(res, g, arm, family, what, tol):
    """A discrete control result (joints, reachable, state, emergency where present) over the family's rows against G23: flags and
    states exact on every row, joints within `tol` (the suite's TOL); INVALID_INPUT, reachable 0, NaN joints and emergency 0 on
    every row where the reference raised."""
    pre = f"{arm}_{family}_"
    raised = g[pre + "raised"].astype(bool)
    assert raised.all() if family in IMPROPER else not raised.any(), (what, family, "the recorded decisions")
    if family in IMPROPER:
        np.testing.assert_array_equal(res["state"], np.full(ROWS, INVALID_INPUT, dtype=np.uint8), err_msg=f"{what} {family} state")
        np.testing.assert_array_equal(res["reachable"], np.zeros(ROWS, dtype=np.uint8), err_msg=f"{what} {family} reachable")
        assert np.isnan(res["joints"]).all(), (what, family, "joints where the reference raises")
        if "emergency" in res:
            np.testing.assert_array_equal(res["emergency"], np.zeros(ROWS, dtype=np.uint8), err_msg=f"{what} {family} emergency")
        return 0.0
    np.testing.assert_array_equal(res["reachable"], g[pre + "reachable"], err_msg=f"{what} {family} reachable")
    np.testing.assert_array_equal(res["state"], g[pre + "state"], err_msg=f"{what} {family} state")
    err = float(np.max(np.abs(res["joints"] - g[pre + "joints"])))
    print(f"{what} {arm} {family}: joints against G23 {err:.3e}, {int(g[pre + 'reachable'].sum())} of {ROWS} reachable")
    assert err < tol, (what, family, "joints", err)
    return err
