"""Tolerances and comparisons shared by the CPU and the GPU tests.  NumPy and the standard library only (tests/far_inputs.py and
tests/scale_inputs.py, which oracle/gen_golden.py imports beside the reference, may import this).  No test in this file: pytest does not
rewrite its asserts, so every one of them carries its own message."""
import numpy as np

TOL = 1e-9              # asserted (north-star bar: 1e-6 rad; observed ~1e-12, so that regressions show)
NORTH_STAR_TOL = 1e-6
CONT_JOINT_TOL = 1e-7   # continuous control step by step: joints
CONT_THETA_TOL = 1e-9   # continuous control step by step: the carried theta


def bits(a):
    """float64 array as its bit patterns: equality that tells -0.0 from 0.0 and takes NaN as a value."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def as_bits(a):
    """bits() of a float64 array, any other array (flags, codes, indices) as it is."""
    return bits(a) if a.dtype == np.float64 else a


def same_bits(got, want, what):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def close(got, want, what, tol=TOL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN in different places"
    err = float(np.max(np.abs(np.nan_to_num(got) - np.nan_to_num(want)), initial=0.0))
    print(f"{what}: max err {err:.3e} over {got.shape}")
    assert err < tol, (what, err)
    return err


def singular_rows(j):
    """Fully extended arm (elbow pitch == 0 to rounding): elbow yaw and wrist yaw rotate about the same axis, and the reference's
    split between them is decided by 1e-17-level rounding noise (atan2 of two ~1e-17 numbers).  Only j2 + j6 is defined there;
    those rows are compared through that sum."""
    return np.abs(j[:, 3]) < 1e-12


def joints_close(got, want, what, tol=TOL):
    """Joints; rows whose elbow pitch is 0 to rounding (fully extended arm) define only j2 + j6, modulo 2 pi (check_symbolic)."""
    sing = singular_rows(want)
    close(got[~sing], want[~sing], what, tol)
    if sing.any():
        a, b = got[sing], want[sing]
        close(a[:, [0, 1, 3, 4, 5]], b[:, [0, 1, 3, 4, 5]], what + " (singular rows)", tol)
        dsum = (a[:, 2] + a[:, 6]) - (b[:, 2] + b[:, 6])
        err = float(np.max(np.abs(dsum - 2 * np.pi * np.round(dsum / (2 * np.pi)))))
        print(f"{what}: {int(sing.sum())} singular rows, j2 + j6 err {err:.3e}")
        assert err < 1e-7, (what, err)


def joint_error(got, want):
    """Largest |difference| over the rows whose elbow pitch is not 0 (joints_close compares the others through j2 + j6)."""
    rows = np.abs(want[:, 3]) >= 1e-12
    return float(np.max(np.abs(got[rows] - want[rows]), initial=0.0))


def angle_diff(a, b):
    """utils.py:486-490.  On Python floats this is the reference's own float arithmetic; on arrays NumPy's, the same IEEE
    operations as the checker's fmod form for these magnitudes, to rounding."""
    return ((a - b) + np.pi) % (2 * np.pi) - np.pi


def is_valid_angle(angle, i0, i1):
    """utils.py:468-474."""
    if i0 % (2 * np.pi) == i1 % (2 * np.pi):
        return True
    if i0 < i1:
        return i0 <= angle <= i1
    return i0 <= angle or angle <= i1
