"""Goal matrices that are not rotations (tests/matrix_forms.py, G23), on the CPU: the families themselves, the reference's own error,
the checker's conversion against G23 and the 50-digit reference, and its continuous step over a goal the reference raises on.
(The checker's discrete control path on G23 stands next to G8's in tests/test_oracle_golden.py.)"""
import hashlib

import numpy as np
import pytest

import matrix_forms as F
from checker_support import load
from compare import bits
from oracle import oracle as orc

ARMS = ("r_arm", "l_arm")


@pytest.fixture(scope="module")
def g23(golden_dir):
    return load(golden_dir, F.G23)


@pytest.mark.parametrize("family", F.FAMILIES)
def test_family_conditions_and_recorded_decisions(g23, family):
    """The family is what its description says, G23 was recorded on these very blocks, and every decision of the reference — raised
    or answered, in the conversion and in ControlIK — is the sign of the exact determinant."""
    F.check_family(family)
    B = F.blocks(family)
    assert bytes(g23[family + "_sha256"]) == hashlib.sha256(B.tobytes()).digest(), "G23 was recorded on other blocks"
    sign = F.exact_det_sign(B)
    assert (sign > 0).all() if family in F.PROPER else (sign < 0).all() if family == "left_handed" else (sign == 0).all(), family
    for arm in ARMS:
        pre = f"{arm}_{family}_"
        np.testing.assert_array_equal(g23[pre + "euler_raised"], (sign <= 0).astype(np.uint8))
        np.testing.assert_array_equal(g23[pre + "raised"], (sign <= 0).astype(np.uint8))
        np.testing.assert_array_equal(np.isnan(g23[pre + "euler"]).any(axis=1), sign <= 0)
        np.testing.assert_array_equal(np.isnan(g23[pre + "joints"]).any(axis=1), sign <= 0)
        assert (g23[pre + "state"][sign <= 0] == 255).all() and (g23[pre + "state"][sign > 0] <= 7).all()


@pytest.mark.parametrize("family", F.PROPER)
def test_scipy_against_mpmath(g23, family):
    """The reference's own error: SciPy's recorded double-precision angles against the 50-digit polar factor's, as rotations.  The
    figure REF_ERR[family] in tests/matrix_forms.py is this measurement (rounded up), and the families' tolerances follow from it."""
    err = max(float(F.rotation_error(g23[f"{arm}_{family}_euler"], F.reference(family)[0]).max()) for arm in ARMS)
    print(f"REF_ERR[{family}] measured {err:.3e}, recorded {F.REF_ERR[family]:.3e}, tolerance {F.tolerance(family):.3e}")
    assert 0.5 * F.REF_ERR[family] <= err <= F.REF_ERR[family], (family, err, F.REF_ERR[family])
    # the reference's Euler angles stand for the polar factor they were read from
    eul, rot = F.reference(family)
    assert float(np.max(np.abs(F.euler_to_matrix(eul) - rot))) < 1e-14


@pytest.mark.parametrize("family", F.FAMILIES)
def test_checker_conversion(g23, family):
    """orc.euler_from_matrix_xyz on every family: the 50-digit reference and G23 for det > 0, NaN angles for det <= 0."""
    eul = orc.euler_from_matrix_xyz(F.blocks(family))
    for arm in ARMS:
        F.check_euler(eul, g23, arm, family, "checker")


def test_checker_continuous_step_steps_over_bad_goals(g23):
    """The checker's continuous step on a reflection and on the zero block in the middle of a trajectory: INVALID_INPUT, no joints,
    previous_sol, init and the latch as they were — and the next ordinary step goes on as in a walk that never saw them."""
    arm = orc.Arm("r_arm", -1.01)
    goals = np.repeat(F.ordinary_matrices(g23, "r_arm")[:1], 6, axis=0)   # a trajectory that stands still: no continuity stop
    goals[:, 0, 3] += 1e-4 * np.arange(6)
    pref = -4 * np.pi / 6
    for bad_family, row in (("left_handed", 0), ("left_handed", 5), ("singular", 0), ("singular", 7)):
        bad = F.goal_matrices(F.blocks(bad_family)[row:row + 1], goals[2:3, :3, 3])[0]
        cs, twin = orc.ContinuousState(0.0, np.zeros(7)), orc.ContinuousState(0.0, np.zeros(7))
        for cs_k in (cs, twin):
            cs_k.buf[10] = 0.0
        for k in range(3):
            for c in (cs, twin):
                orc.control_continuous_step(arm, c, goals[k], k == 0, pref, pref, 0, np.zeros(7), goals[0])
        before = cs.buf.copy()
        assert before[9] == 0.0, "the walk latched before the bad goal"
        j, ok, st = orc.control_continuous_step(arm, cs, bad, False, pref, pref, 0, np.zeros(7), goals[0])
        assert st == F.INVALID_INPUT and not ok and np.isnan(j).all(), (bad_family, row, st, ok, j)
        np.testing.assert_array_equal(bits(cs.buf[1:]), bits(before[1:]), err_msg="previous_sol / init / latch / has_previous_sol")
        got = orc.control_continuous_step(arm, cs, goals[3], False, pref, pref, 0, np.zeros(7), goals[0])
        want = orc.control_continuous_step(arm, twin, goals[3], False, pref, pref, 0, np.zeros(7), goals[0])
        assert got[1:] == want[1:] and float(np.max(np.abs(got[0] - want[0]))) < 1e-7, (bad_family, row)
