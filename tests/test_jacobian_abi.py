"""CPU-side checks of rsik_jacobian: declared, exported, bound, ABI version still 8, the Python surface exists, the argument check
that needs no device — and the NumPy reference of the GPU tests (tests/jacobian_workload.py) pinned on the CPU alone, with the
conditions the named joint sets must meet for tests/test_gpu_jacobian.py to mean something and the solver link's bounds measured with
the CPU checker."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import arm_pairs
import fk_numpy
import jacobian_workload as JW
from checker_support import CheckerRows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ("uniform", "wound", "singular", "near_singular")


def test_jacobian_entry_point_is_part_of_abi_8():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert _abi.ABI_VERSION == 8 == L.rsik_abi_version()
    assert "rsik_jacobian" in _abi.PROTOTYPES
    assert isinstance(L.rsik_jacobian, C._CFuncPtr)
    hdr = open(os.path.join(ROOT, "include", "rsik.h")).read()
    assert "#define RSIK_ABI_VERSION 8" in hdr
    decl = re.search(r"int rsik_jacobian\(([^;]*)\);", hdr)
    assert decl, "include/rsik.h does not declare rsik_jacobian"
    assert len(decl.group(1).split(",")) == len(_abi.PROTOTYPES["rsik_jacobian"][1]) == 9
    assert int(re.search(r"#define RSIK_OPT_COUNT (\d+)", hdr).group(1)) == 9
    assert "signed maximal minors" in hdr
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`rsik_jacobian`" in doc


def test_jacobian_entry_point_refuses_a_null_context():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert L.rsik_jacobian(None, 0, 1, None, None, 0, None, None, None) == _abi.RSIK_E_INVALID


def test_python_surface_exists():
    from reachy2_symbolic_ik_amd import DualArmIK, HipSolver, SymbolicIK

    for cls, name in ((HipSolver, "jacobian"), (SymbolicIK, "jacobian_batch"), (DualArmIK, "jacobian_batch")):
        fn = getattr(cls, name)
        assert callable(fn) and "signed minors" in fn.__doc__, (cls.__name__, name)
        for word in ("null_vector", "manipulability", "not normalised"):
            assert word in fn.__doc__, (cls.__name__, name, word)
    assert HipSolver.JACOBIAN_OUTPUTS == ("jacobian", "null_vector", "manipulability")


# ------------------------------------------------------------------------------------------ the reference, on the CPU alone
def _fk_numpy_arm(name, arm):
    from reachy2_symbolic_ik_amd.constants import default_ik_parameters

    P = arm_pairs.geometry_of(name).get("ik_parameters") or default_ik_parameters()
    return lambda q: fk_numpy.forward_kinematics(q, P[arm + "_shoulder_position"], P[arm + "_shoulder_orientation"],
                                                 P[arm + "_upper_arm_size"], P[arm + "_forearm_size"], P[arm + "_tip_position"][2])


@pytest.mark.parametrize("name", ["default", "ztip"])
def test_helper_fk_is_fk_numpy(name):
    """The chain of jacobian_workload, built from the packed constant block, against tests/fk_numpy.py (built from the geometry's own
    parameters) on the arms whose tip lies on z: 1e-14."""
    q = JW.joint_set("uniform")
    for side, arm in enumerate(("r", "l")):
        block = JW.blocks_of(f"{name}/{name}" if name == "default" else ("ztip/default", "default/ztip")[side])[side]
        p, R = JW.fk(block, q)
        p2, R2 = _fk_numpy_arm(name, arm)(q)
        err = max(float(np.abs(p - p2).max()), float(np.abs(R - R2).max()))
        print(f"{name} {arm}: helper FK against fk_numpy {err:.3e}")
        assert err < 1e-14, (name, arm, err)


@pytest.mark.parametrize("pair", JW.PAIRS)
def test_helper_jacobian_is_the_derivative_of_helper_fk(pair):
    """Central differences of the helper's FK at h = 1e-6 (truncation about 1e-12, rounding about eps / h = 1e-10): 1e-8, on the
    uniform and the wound set; the custom arm's tip has x / y components."""
    for side, block in enumerate(JW.blocks_of(pair)):
        for name in ("uniform", "wound"):
            q = JW.joint_set(name)[:256]
            err = float(np.abs(JW.jacobian(block, q) - JW.fd_jacobian(lambda x: JW.fk(block, x), q)).max())
            print(f"{pair} slot {side} {name}: J against central differences {err:.3e}")
            assert err < 1e-8, (pair, side, name, err)


@pytest.mark.parametrize("pair", JW.PAIRS)
def test_helper_minors(pair):
    """J . null = 0 to rounding (7e-15), |null| = sqrt(det(J J^T)) to 1e-9 relative where the manipulability is >= 1e-4, and every row
    of the singular set has manipulability < 1e-9."""
    blocks, arm = JW.blocks_of(pair), JW.arm_bytes()
    ref = JW.reference(blocks, JW.joint_set("uniform"), arm)
    J, null, w = ref["jacobian"], ref["null_vector"], ref["manipulability"]
    res = float(np.abs(np.einsum("nij,nj->ni", J, null)).max())
    gram = np.sqrt(np.linalg.det(J @ J.transpose(0, 2, 1)))
    big = w >= 1e-4
    rel = float((np.abs(gram[big] - w[big]) / w[big]).max())
    sing = float(JW.reference(blocks, JW.joint_set("singular"), arm)["manipulability"].max())
    print(f"{pair}: max |J . null| {res:.3e}, |null| against sqrt(det(J J^T)) {rel:.3e} relative on {int(big.sum())} rows, "
          f"singular set manipulability <= {sing:.3e}")
    assert res < 1e-15 * 7
    assert big.sum() >= 900 and rel < 1e-9
    assert sing < 1e-9
    assert np.array_equal(JW.signed_minors(J[:4])[:, 1], -np.linalg.det(J[:4][:, :, [0, 2, 3, 4, 5, 6]]))


def test_helper_rows_that_are_not_numbers():
    q = JW.joint_set("uniform")[:8].copy()
    q[2, 5], q[5, 0] = np.nan, -np.inf
    ref = JW.reference(JW.blocks_of("default/default"), q, JW.arm_bytes()[:8])
    for key, v in ref.items():
        rows = np.isnan(v.reshape(8, -1))
        assert rows[[2, 5]].all() and not rows[[0, 1, 3, 4, 6, 7]].any(), key


# ------------------------------------------------------------------------------------------ what the named sets must be
@pytest.mark.parametrize("pair", JW.PAIRS)
def test_named_sets(pair):
    """At least 80 % of the uniform set has manipulability >= 1e-3; both arm bytes are present, in every wave; the wound set is the
    uniform set plus whole turns and stays within +-6 pi; the singular set's elbow is exactly straight, the near-singular one's within
    1e-6 ... 1e-3 of it; the golden joints are finite."""
    blocks, arm = JW.blocks_of(pair), JW.arm_bytes()
    w = JW.reference(blocks, JW.joint_set("uniform"), arm)["manipulability"]
    print(f"{pair}: manipulability 5th percentile {np.percentile(w, 5):.3e}, median {np.median(w):.3e}, share >= 1e-3 {(w >= 1e-3).mean():.3f}")
    assert (w >= 1e-3).mean() >= 0.8
    per_wave = arm.reshape(-1, 64).sum(axis=1)
    assert ((per_wave > 0) & (per_wave < 64)).all()
    for name in SETS:
        q = JW.joint_set(name)
        assert q.shape == (JW.N_SET, 7) and np.isfinite(q).all(), name
    u, wd = JW.joint_set("uniform"), JW.joint_set("wound")
    turns = (wd - u) / (2 * np.pi)
    assert np.abs(turns - np.round(turns)).max() < 1e-15 and np.abs(np.round(turns)).max() == 2 and np.abs(wd).max() <= JW.SIX_PI
    assert np.abs(u).max() <= 2.0
    assert (JW.joint_set("singular")[:, 3] == 0.0).all()
    ns = np.abs(JW.joint_set("near_singular")[:, 3])
    assert 1e-6 <= ns.min() and ns.max() <= 1e-3 and (JW.joint_set("near_singular")[:, 3] < 0).any()
    gj, ga = JW.golden_joints()
    assert gj.shape == (512, 7) and set(ga.tolist()) == {0, 1}


# ------------------------------------------------------------------------------------------ the link to the solver, on the checker
def _checker_link():
    from reachy2_symbolic_ik_amd import constants as K

    pos, eul, arm, theta = JW.link_poses()
    blocks = JW.blocks_of("default/default")
    out = {}
    for name, d in (("minus", -JW.LINK_H), ("plus", JW.LINK_H), ("mid", 0.0)):
        rows = CheckerRows(arm)  # a fresh object per sample: a projection moves the object's goal
        assert rows.reach(pos, eul)["reachable"].all()
        out[name] = rows.joints(theta + d)
    projected = out["minus"]["projected"] | out["plus"]["projected"]
    keep, dq, ref = JW.link_measure(blocks, out["minus"]["joints"], out["plus"]["joints"], out["mid"]["joints"], projected, arm,
                                    [b[K.C_ELBOW_LIMIT] for b in blocks])
    return arm, keep, dq, ref


def test_link_filter_keeps_half_of_the_reachable_rows():
    arm, keep, _, _ = _checker_link()
    print(f"solver link: {int(keep.sum())} of {len(keep)} reachable rows kept (r {int(keep[arm == 0].sum())}, l {int(keep[arm == 1].sum())})")
    assert keep.sum() * 2 >= len(keep)
    assert keep[arm == 0].sum() >= 64 and keep[arm == 1].sum() >= 64


def test_link_bounds_come_from_the_reference():
    """The bounds of tests/test_gpu_jacobian.py::test_null_vector_is_the_solve_s_self_motion are 10 x what the CPU checker's
    get_joints at theta +- 1e-5 and the NumPy reference give on the kept rows: max |J . dq| and max 1 - |cos(null, dq)|.  Measured
    here again; the constants in jacobian_workload must be that, rounded up (no more than twice it: the last bits of the
    measurement may differ between libm builds).  The sign of null . dq/dtheta is recorded: negative on
    every kept row of both arms."""
    arm, keep, dq, ref = _checker_link()
    jdq, cos, signs = JW.link_figures(ref["jacobian"], ref["null_vector"], dq, keep)
    for side in (0, 1):
        a, b, s = JW.link_figures(ref["jacobian"], ref["null_vector"], dq, keep & (arm == side))
        print(f"solver link, {'rl'[side]} rows: max |J . dq| {a:.3e}, max 1 - |cos(null, dq)| {b:.3e}, sign of null . dq {sorted(set(s.tolist()))}")
    assert 10 * jdq <= JW.LINK_JDQ_BOUND <= 20 * jdq, (jdq, JW.LINK_JDQ_BOUND)
    assert 10 * cos <= JW.LINK_COS_BOUND <= 20 * cos, (cos, JW.LINK_COS_BOUND)
    assert (signs == -1.0).all()
