"""CPU-side checks of rsik_solve_nearest: declared, exported, bound with 22 arguments, ABI version still 8, the Python surface
exists, the argument check that needs no device — and the expected-value helper of the GPU tests
(tests/nearest_workload.nearest_from_sweep) exercised on the checker's tiled sweep: ties go to the lower sample, a row whose
samples all project has no candidate under the flag, and the inputs of the GPU tests satisfy the gap condition on their own."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from checker_support import default_arms
from nearest_workload import GAP, KS, gap_condition, main_case, main_thetas, nearest_from_sweep, seeds, skip_projected_case
from oracle import oracle as orc
from sweep_workload import expected_tiled, sweep_poses, sweep_thetas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nearest_entry_point_is_part_of_abi_8():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert _abi.ABI_VERSION == 8 == L.rsik_abi_version()
    assert "rsik_solve_nearest" in _abi.PROTOTYPES
    assert isinstance(L.rsik_solve_nearest, C._CFuncPtr)
    hdr = open(os.path.join(ROOT, "include", "rsik.h")).read()
    assert "#define RSIK_ABI_VERSION 8" in hdr
    decl = re.search(r"int rsik_solve_nearest\(([^;]*)\);", hdr)
    assert decl, "include/rsik.h does not declare rsik_solve_nearest"
    assert len(decl.group(1).split(",")) == len(_abi.PROTOTYPES["rsik_solve_nearest"][1]) == 22
    assert "#define RSIK_OPT_NEAREST_LANES 8" in hdr and "#define RSIK_OPT_COUNT 9" in hdr
    assert "#define RSIK_NEAREST_SKIP_PROJECTED 1" in hdr
    assert _abi.OPT_NEAREST_LANES == 8 and _abi.NEAREST_SKIP_PROJECTED == 1
    flat = " ".join(hdr.replace("*", " ").split())  # (whatever the comment's line breaks are)
    assert "a pose can be reachable and still have index -1" in flat, "the header must say that a reachable row can have no winner"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`rsik_solve_nearest`" in doc


def test_nearest_entry_point_refuses_a_null_context():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert L.rsik_solve_nearest(None, 0, None, None, 0, 1, _abi.THETA_FRACTION, None, 0, None, None, None, 0,
                                None, None, None, None, None, None, None, None, None) == _abi.RSIK_E_INVALID


def test_python_surface_exists():
    from reachy2_symbolic_ik_amd import DualArmIK, HipSolver, SymbolicIK

    for cls, name in ((HipSolver, "solve_nearest"), (SymbolicIK, "nearest_batch"), (DualArmIK, "nearest_batch")):
        fn = getattr(cls, name)
        assert callable(fn) and "index [n] int32" in " ".join(fn.__doc__.split()), (cls.__name__, name)


def test_a_duplicated_theta_column_gives_the_lower_sample():
    """K = 6, per-pose explicit theta, columns 1 and 4 equal, seed = the joints of sample 4: both have cost 0, sample 1 wins."""
    n, k = 300, 6
    pos, eul, arm = sweep_poses("mixed", 71, n)
    thetas = sweep_thetas("explicit", True, k, n, 72)
    thetas[4] = thetas[1]
    ref = expected_tiled(orc, default_arms(), pos, eul, arm, "explicit", thetas)
    ok = ref["reachable"].astype(bool)
    assert ok.sum() >= 50
    seed = np.where(ok[:, None], ref["joints"][4], seeds(n, 73))
    exp = nearest_from_sweep(ref, seed)
    assert (exp["index"][ok] == 1).all() and (exp["c_min"][ok] == 0.0).all() and (exp["gap"][ok] == 0.0).all()
    assert (exp["index"][~ok] == -1).all() and np.isinf(exp["c_min"][~ok]).all()


def test_a_row_whose_samples_all_project_has_no_candidate_under_the_flag():
    pos, eul, arm, thetas, ref, mixed, all_projected = skip_projected_case(orc)
    ok = ref["reachable"].astype(bool)
    seed = np.where(ok[:, None], ref["joints"][0], seeds(len(pos), 33))
    free = nearest_from_sweep(ref, seed)
    assert (free["index"][mixed | all_projected] == 0).all() and (free["c_min"][mixed | all_projected] == 0.0).all()
    exp = nearest_from_sweep(ref, seed, skip_projected=True)
    assert (exp["index"][all_projected] == -1).all() and np.isinf(exp["c_min"][all_projected]).all()
    assert (exp["index"][mixed] >= 1).all()
    won = exp["index"][mixed]
    assert (ref["projected"][won, np.flatnonzero(mixed)] == 0).all()
    assert (exp["index"][~ok] == -1).all()
    assert (mixed & (exp["gap"] > GAP)).sum() >= 20, "the GPU test compares index on these rows"


def test_a_nan_seed_row_or_theta_is_no_candidate():
    n, k = 200, 3
    pos, eul, arm = sweep_poses("r", 75, n)
    thetas = sweep_thetas("explicit", True, k, n, 76)
    ok_rows = np.flatnonzero(expected_tiled(orc, default_arms(), pos, eul, arm, "explicit", thetas)["reachable"])
    row = int(ok_rows[0])
    thetas[1, row] = np.nan
    ref = expected_tiled(orc, default_arms(), pos, eul, arm, "explicit", thetas)
    seed = seeds(n, 77)
    seed[int(ok_rows[1]), 3] = np.nan
    exp = nearest_from_sweep(ref, seed)
    assert not exp["candidate"][1, row] and exp["index"][row] in (0, 2)
    assert exp["index"][int(ok_rows[1])] == -1


@pytest.mark.parametrize("kind", ["r", "l", "mixed"])
def test_the_inputs_of_the_gpu_tests_satisfy_the_gap_condition(kind):
    """For every shape and seed tests/test_gpu_solve_nearest.py uses in its main test, on the checker's joints: at least 95 % of the
    reachable rows have their two best candidates more than GAP apart (the GPU test asserts the same on the library's sweep)."""
    for k in KS:
        pos, eul, arm, seed = main_case(kind, k)
        for policy in ("fraction", "explicit"):
            for per_pose in (False, True):
                ref = expected_tiled(orc, default_arms(), pos, eul, arm, policy, main_thetas(policy, per_pose, k), nthreads=4)
                for skip in (False, True):
                    exp = nearest_from_sweep(ref, seed, skip_projected=skip)
                    gap_condition(exp, ref["reachable"], f"{kind} K {k} {policy} per_pose {per_pose} skip {skip}")
    assert GAP == 1e-9
    if kind == "mixed":  # the weights test's inputs
        pos, eul, arm, seed = main_case(kind, 8)
        ref = expected_tiled(orc, default_arms(), pos, eul, arm, "fraction", main_thetas("fraction", True, 8), nthreads=4)
        for w in ((1, 1, 1, 1, 0, 0, 0), (0, 0, 0, 0, 2, 3, 5)):
            gap_condition(nearest_from_sweep(ref, seed, weights=w), ref["reachable"], f"weights {w}")
        unit = nearest_from_sweep(ref, seed)["index"]
        for w in ((1, 1, 1, 1, 0, 0, 0), (0, 0, 0, 0, 2, 3, 5)):
            assert (nearest_from_sweep(ref, seed, weights=w)["index"] != unit).sum() >= 10, "weights that change no winner test nothing"
