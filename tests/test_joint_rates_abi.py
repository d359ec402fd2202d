"""CPU-side checks of rsik_joint_rates: declared, exported, bound, ABI version still 8, the Python surface exists, the argument check
that needs no device — and the reference and the tolerance of the GPU tests (tests/joint_rates_workload.py) pinned on the CPU alone:
lstsq against a 40-digit solve, a float64 restatement of the kernel's algorithm against the tolerance's second term, the conditions
that keep the tolerance from hiding a failure, and what the pivot clamp does at a straight elbow."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jacobian_workload as JW
import joint_rates_workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ("uniform", "wound", "singular", "near_singular")


# ------------------------------------------------------------------------------------------ surface
def test_joint_rates_entry_point_is_part_of_abi_8():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert _abi.ABI_VERSION == 8 == L.rsik_abi_version()
    assert "rsik_joint_rates" in _abi.PROTOTYPES
    assert isinstance(L.rsik_joint_rates, C._CFuncPtr)
    hdr = open(os.path.join(ROOT, "include", "rsik.h")).read()
    assert "#define RSIK_ABI_VERSION 8" in hdr
    decl = re.search(r"int rsik_joint_rates\(([^;]*)\);", hdr)
    assert decl, "include/rsik.h does not declare rsik_joint_rates"
    assert len(decl.group(1).split(",")) == len(_abi.PROTOTYPES["rsik_joint_rates"][1]) == 12
    assert int(re.search(r"#define RSIK_OPT_COUNT (\d+)", hdr).group(1)) == 9
    for words in ("clamped from below at lambda^2", "lambda = 0 is not offered", "(J J^T + lambda^2 I) y = twist - J q0"):
        assert words in hdr, words
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`rsik_joint_rates`" in doc and "joint_rates_batch" in doc


def test_joint_rates_entry_point_refuses_a_null_context():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert L.rsik_joint_rates(None, 0, 1, None, None, 0, None, 0.05, None, None, None, None) == _abi.RSIK_E_INVALID


def test_python_surface_exists():
    from reachy2_symbolic_ik_amd import DualArmIK, HipSolver, SymbolicIK

    for cls, name in ((HipSolver, "joint_rates"), (SymbolicIK, "joint_rates_batch"), (DualArmIK, "joint_rates_batch")):
        fn = getattr(cls, name)
        assert callable(fn), (cls.__name__, name)
        for word in ("|J q' - twist|^2 + lambda^2 |q' - q0|^2", "pivot clamp", "achieved_twist"):
            assert word in fn.__doc__, (cls.__name__, name, word)
    assert HipSolver.JOINT_RATES_OUTPUTS == ("rates", "achieved_twist")


# ------------------------------------------------------------------------------------------ the reference, on the CPU alone
def _rows(set_name, n, side=1, pair="custom/custom"):
    return W.side_jacobians(pair, set_name)[side][:n], W.twists()[:n], W.biases()[:n]


@pytest.mark.parametrize("lam", W.LAMBDAS)
@pytest.mark.parametrize("set_name", SETS)
def test_lstsq_against_a_40_digit_solve(set_name, lam):
    """The reference (lstsq on the stacked 13 x 7 system, corrected once through its gradient: joint_rates_workload.reference) against
    the normal equations solved in mpmath at 40 digits, 64 rows per set of custom/custom, with bias: per row within
    64 * 2^-53 * sqrt(kappa_2(A)) |z|.

    Measured (error / bound, worst row) at lambda = 1e-3 / 0.05 / 1.0: uniform 0.003 / 0.004 / 0.030, wound 0.003 / 0.004 / 0.025,
    singular 0.000 / 0.002 / 0.038, near_singular 0.000 / 0.001 / 0.033; the largest error is 3.2e-14.  lstsq alone, without the
    correction step, gives 5.1 (singular) and 3.4 (near_singular) at lambda = 1e-3: with a residual of order 1 a least-squares
    solution is sensitive to kappa^2 |residual| / |M|, not to kappa |z| alone."""
    J, v, q0 = _rows(set_name, 64)
    ref = W.reference(J, v, lam, q0)["rates"]
    exact = W.mp_rates(J, v, lam, q0)
    tol = W.tolerances(J, v, lam, q0)
    bound = 64.0 * W.EPS * np.sqrt(tol["kappa"]) * tol["z_norm"]
    err = np.linalg.norm(ref - exact, axis=1)
    print(f"{set_name} lambda {lam}: lstsq against 40 digits, max error / bound {(err / bound).max():.3f}, max error {err.max():.3e}, "
          f"max error / second term of tol_row {(err / tol['second']).max():.2e}")
    assert (err <= bound).all(), (set_name, lam, float((err / bound).max()))


@pytest.mark.parametrize("set_name", SETS)
def test_restated_algorithm_stays_within_the_second_term(set_name):
    """The kernel's algorithm restated in float64 NumPy (normal equations, natural-order L D L^T, clamp) against the reference on 256
    rows of custom/custom, both blocks, the three lambdas: the row's error within 128 * 2^-53 * kappa_2(A) |z|.  Measured: at most
    0.016 of it (0.0032 at lambda = 1e-3, 0.0027 at 0.05, 0.016 at 1.0, where kappa is about 2): the constant 128 is a bound, not a
    fit."""
    for side in (0, 1):
        J, v, q0 = _rows(set_name, 256, side)
        for lam in W.LAMBDAS:
            err = np.linalg.norm(W.restatement(J, v, lam, q0) - W.reference(J, v, lam, q0)["rates"], axis=1)
            second = W.tolerances(J, v, lam, q0)["second"]
            print(f"{set_name} slot {side} lambda {lam}: restatement against the reference, max error / second term {(err / second).max():.4f}")
            assert (err <= second).all(), (set_name, side, lam, float((err / second).max()))


@pytest.mark.parametrize("pair", W.PAIRS)
def test_restated_algorithm_at_a_tiny_lambda(pair):
    """lambda = 1e-7 on all 1024 uniform rows, both blocks of every pair, with bias: the restatement within tol_row of the reference.
    (lstsq alone, without the reference's correction step, sits at 2.8 tol_row on row 243 of the ztip arm.)"""
    v, q0 = W.twists(), W.biases()
    for side, J in enumerate(W.side_jacobians(pair, "uniform")):
        case = W.side_case(pair, "uniform", W.TINY_LAMBDA, True)[side]
        err = np.linalg.norm(W.restatement(J, v, W.TINY_LAMBDA, q0) - case["rates"], axis=1)
        print(f"{pair} slot {side} lambda {W.TINY_LAMBDA}: restatement against the reference, max error / tol_row {(err / case['tol_row']).max():.4f}")
        assert (err <= case["tol_row"]).all(), (pair, side, float((err / case["tol_row"]).max()))


# ------------------------------------------------------------------------------------------ the tolerance cannot hide a failure
@pytest.mark.parametrize("pair", W.PAIRS)
def test_tolerance_is_small_where_the_problem_is_well_posed(pair):
    """max tol_row over every named set, both blocks, with and without bias: <= 1e-6 at lambda = 0.05, <= 1e-10 at lambda = 1.0."""
    for lam, cap in ((0.05, 1e-6), (1.0, 1e-10)):
        worst = max(float(W.side_case(pair, name, lam, bias)[side]["tol_row"].max())
                    for name in SETS for bias in (False, True) for side in (0, 1))
        print(f"{pair} lambda {lam}: max tol_row {worst:.3e} (cap {cap:.0e})")
        assert worst <= cap, (pair, lam, worst)


@pytest.mark.parametrize("pair", W.PAIRS)
def test_tolerance_tells_a_wrong_sign_and_a_wrong_order(pair):
    """At lambda = 0.05 on the uniform rows: the reference with the sign of q0 flipped, and with the linear and angular halves of the
    twist swapped, each differ from it by more than 1000 tol_row on at least 90 % of the rows."""
    v, q0 = W.twists(), W.biases()
    for side, J in enumerate(W.side_jacobians(pair, "uniform")):
        case = W.side_case(pair, "uniform", 0.05, True)[side]
        flipped = W.reference(J, v, 0.05, -q0)["rates"]
        swapped = W.reference(J, np.concatenate([v[:, 3:], v[:, :3]], axis=1), 0.05, q0)["rates"]
        for what, other in (("q0 flipped", flipped), ("twist halves swapped", swapped)):
            share = float((np.linalg.norm(other - case["rates"], axis=1) > 1000.0 * case["tol_row"]).mean())
            print(f"{pair} slot {side}: {what} differs by more than 1000 tol_row on {share:.3f} of the rows")
            assert share >= 0.9, (pair, side, what, share)


def test_helpers_agree_with_each_other():
    """reference() minimises what it says: its rates satisfy the normal equations (J^T J + lambda^2 I)(rates - q0) = J^T (v - J q0) to
    rounding, achieved_twist is J . rates, a per-row lambda array equals the scalar, and pick() takes each row from its arm's block."""
    J, v, q0 = _rows("uniform", 128)
    ref = W.reference(J, v, 0.05, q0)
    z = ref["rates"] - q0
    lhs = np.einsum("nji,nj->ni", J, np.einsum("nij,nj->ni", J, z)) + 0.05 ** 2 * z
    rhs = np.einsum("nji,nj->ni", J, v - np.einsum("nij,nj->ni", J, q0))
    assert np.abs(lhs - rhs).max() < 1e-12
    assert np.array_equal(ref["achieved_twist"], np.einsum("nij,nj->ni", J, ref["rates"]))
    assert np.array_equal(W.reference(J, v, np.full(128, 0.05), q0)["rates"], ref["rates"])
    arm = JW.arm_bytes()[:128]
    case = W.side_case("custom/custom", "uniform", 0.05, True)
    got = W.pick(case, arm, np.arange(128), "rates")
    assert np.array_equal(got[arm == 1], case[1]["rates"][:128][arm == 1]) and np.array_equal(got[arm == 0], case[0]["rates"][:128][arm == 0])
    far, twin = W.far_rows()
    assert far.shape == twin.shape == (42, 7) and np.abs(twin).max() <= 2.0 and np.abs(far).max() >= 1e300


# ------------------------------------------------------------------------------------------ the pivot clamp
@pytest.mark.parametrize("set_name", ["singular", "near_singular"])
def test_pivot_clamp_at_a_straight_elbow(set_name):
    """lambda = 1e-7 on the 1024 rows of the singular (straight elbow) and the near-singular set, both blocks of custom/custom, with
    bias: the float64 restatement is finite in every row with the clamp.  Recorded without it: 0 rows not finite and 0 rows whose
    |rates - q0| exceeds |v - J q0| / lambda on either set — in NumPy's unfused arithmetic no pivot came out below lambda^2 = 1e-14
    on these rows; the clamp is the guarantee, not a repair of something seen."""
    lam = W.TINY_LAMBDA
    for side in (0, 1):
        J, v, q0 = _rows(set_name, JW.N_SET, side)
        with_clamp = W.restatement(J, v, lam, q0)
        without = W.restatement(J, v, lam, q0, clamp=False)
        limit = W.tolerances(J, v, lam, q0)["residual_norm"] / lam
        not_finite = int((~np.isfinite(without).all(axis=1)).sum())
        with np.errstate(invalid="ignore"):
            exceed = int((np.linalg.norm(without - q0, axis=1) > limit).sum())
        print(f"{set_name} slot {side} lambda {lam}: without the clamp {not_finite} rows not finite, {exceed} beyond |v - J q0| / lambda; "
              f"with it max |rates - q0| lambda / |v - J q0| = {(np.linalg.norm(with_clamp - q0, axis=1) / limit).max():.3g}")
        assert np.isfinite(with_clamp).all(), (set_name, side)
