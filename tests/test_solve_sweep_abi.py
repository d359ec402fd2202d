"""CPU-side checks of rsik_solve_sweep: declared, exported, bound, ABI version still 8, the Python surface exists, the argument
check that needs no device — and the expected-value helper of the GPU tests (tests/sweep_workload.py) pinned on the checker
alone: sample k of the tiled batch is a fresh is_reachable followed by one get_joints at that theta, so the reference side of
tests/test_gpu_solve_sweep.py does not depend on the order of the samples."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from compare import bits
from oracle import oracle as orc
from sweep_workload import columns, expected_tiled, fraction_theta, sweep_poses, sweep_thetas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_entry_point_is_part_of_abi_8():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert _abi.ABI_VERSION == 8 == L.rsik_abi_version()
    assert "rsik_solve_sweep" in _abi.PROTOTYPES
    assert isinstance(L.rsik_solve_sweep, C._CFuncPtr)
    hdr = open(os.path.join(ROOT, "include", "rsik.h")).read()
    assert "#define RSIK_ABI_VERSION 8" in hdr
    decl = re.search(r"int rsik_solve_sweep\(([^;]*)\);", hdr)
    assert decl, "include/rsik.h does not declare rsik_solve_sweep"
    assert len(decl.group(1).split(",")) == len(_abi.PROTOTYPES["rsik_solve_sweep"][1]) == 17
    assert "within ABI version 8" in hdr
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`rsik_solve_sweep`" in doc


def test_sweep_entry_point_refuses_a_null_context():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert L.rsik_solve_sweep(None, 0, None, None, 0, 1, _abi.THETA_FRACTION, None, 0, None, None, None, None, None, None, None,
                              None) == _abi.RSIK_E_INVALID


def test_python_surface_exists():
    from reachy2_symbolic_ik_amd import DualArmIK, HipSolver, SymbolicIK

    for cls, name in ((HipSolver, "solve_sweep"), (SymbolicIK, "sweep_batch"), (DualArmIK, "sweep_batch")):
        fn = getattr(cls, name)
        assert callable(fn) and "permute(1, 0, 2)" in fn.__doc__, (cls.__name__, name)


@pytest.mark.parametrize("policy", ["fraction", "explicit"])
@pytest.mark.parametrize("per_pose", [False, True])
def test_tiled_batch_is_fresh_is_reachable_plus_one_get_joints(policy, per_pose):
    """tests/sweep_workload.expected_tiled against the checker's solver OBJECT: for every (sample, pose) a new orc.Solver,
    is_reachable, ONE get_joints at that sample's theta — bit for bit, the projection flag included."""
    n, k = 400, 3
    pos, eul, arm = sweep_poses("mixed", 21, n)
    arms = (orc.Arm("r_arm", 0.03), orc.Arm("l_arm", 0.03))
    thetas = sweep_thetas(policy, per_pose, k, n, 22)
    ref = expected_tiled(orc, arms, pos, eul, arm, policy, thetas)
    th = columns(thetas, n)
    assert ref["joints"].shape == (k, n, 7) and ref["projected"].shape == (k, n) and ref["interval"].shape == (n, 2)
    n_ok = 0
    for q in range(k):
        for i in range(n):
            sv = orc.Solver(arms[int(arm[i])])
            ok, itv, st = sv.is_reachable(pos[i], eul[i])
            assert ok == bool(ref["reachable"][i]) and st == ref["state"][i]
            if not ok:
                assert np.isnan(ref["joints"][q, i]).all() and np.isnan(ref["elbow"][q, i]).all() and ref["projected"][q, i] == 0
                assert np.isnan(ref["theta"][q, i])
                continue
            n_ok += 1
            theta = fraction_theta(itv[None, :], th[q, i])[0] if policy == "fraction" else th[q, i]
            assert bits(theta) == bits(ref["theta"][q, i])
            j, e, p = sv.get_joints(theta)
            assert np.array_equal(bits(j), bits(ref["joints"][q, i])) and np.array_equal(bits(e), bits(ref["elbow"][q, i]))
            assert p == bool(ref["projected"][q, i])
            assert np.array_equal(bits(itv), bits(ref["interval"][i]))
    assert n_ok >= 0.3 * k * n
