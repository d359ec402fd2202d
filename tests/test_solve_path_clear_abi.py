"""CPU-side checks of rsik_solve_path_clear: declared, exported, bound with 37 arguments, ABI version still 8 and RSIK_OPT_COUNT still 9,
a NULL context refused, the Python surface exists — and the expected-value helper of the GPU tests
(tests/path_clear_workload.path_clear_dp) exercised on the checker's tiled sweep with clearance_workload.reference as d: it finds what
trying every path finds, it is path_dp where nothing is blocked and the gain is 0, and the inputs of the GPU tests satisfy the
conditions those tests rely on."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from path_clear_workload import (HARD, SOFT, TABLE_SHAPES, checker_clearance, clear_cost_along, input_conditions, path_clear_dp,
                                 path_clear_tol, soft_condition, COST_SUM_MAX)
from checker_support import default_arms
from oracle import oracle as orc
from path_workload import GAP, MAIN_SHAPES, N_MAIN, flat, gap_condition, path_dp, path_fractions, path_poses, path_start
from sweep_workload import expected_tiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def checker_case(t, k, seed, kind, n=N_MAIN):
    """The checker's tiled sweep over a shape's poses and the reference clearance of its joints."""
    pos, eul, arm = path_poses(seed, n, t, kind)
    sw = expected_tiled(orc, default_arms(), flat(pos), flat(eul), np.tile(arm, t), "fraction", path_fractions(k), nthreads=4)
    return sw, checker_clearance(sw, np.tile(arm, t))


def test_the_entry_point_is_part_of_abi_8():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert _abi.ABI_VERSION == 8 == L.rsik_abi_version()
    hdr = open(os.path.join(ROOT, "include", "rsik.h")).read()
    assert "#define RSIK_ABI_VERSION 8" in hdr and "#define RSIK_OPT_COUNT 9" in hdr
    name = "rsik_solve_path_clear"
    assert name in _abi.PROTOTYPES and isinstance(getattr(L, name), C._CFuncPtr)
    decl = re.search(r"int %s\(([^;]*)\);" % name, hdr)
    assert decl, f"include/rsik.h does not declare {name}"
    assert len(decl.group(1).split(",")) == len(_abi.PROTOTYPES[name][1]) == 37
    flat_hdr = " ".join(hdr.replace("*", " ").split())  # (whatever the comment's line breaks are)
    assert "the minimum first, then one more sum" in flat_hdr and "rsik_solve_path_workspace_bytes answers for both calls" in flat_hdr
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert name in open(os.path.join(ROOT, doc)).read(), doc


def test_the_entry_point_refuses_a_null_context():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    args = [None, 0, 1, None, None, 0, 1, _abi.THETA_FRACTION, None, 0, None, None, 0, None, 1, None, 0, None, 0.0, 0.0, 0.0, None, 0]
    assert L.rsik_solve_path_clear(*args, *([None] * 14)) == _abi.RSIK_E_INVALID


def test_python_surface_exists():
    from reachy2_symbolic_ik_amd import DualArmIK, HipSolver, SymbolicIK

    for cls, name in ((HipSolver, "solve_path_clear"), (SymbolicIK, "path_clear_batch"), (DualArmIK, "path_clear_batch")):
        fn = getattr(cls, name)
        doc = " ".join(fn.__doc__.split())
        assert callable(fn) and "min_clearance" in doc and "blocked" in doc and "nearest" in doc, (cls.__name__, name)
    assert "rsik_solve_path_clear" in HipSolver.solve_path_clear.__doc__


def test_the_dp_finds_what_trying_every_path_finds():
    """T = 4, K = 3, n = 12 with the scene, both hard constraints and both parameter pairs, with and without a start row: the cost
    (penalties included) and, where it is the only minimum, the samples of all the paths through the solved waypoints, enumerated,
    against path_clear_dp; `gap` is the enumeration's second-best distinct path minus the best."""
    t, k, n = 4, 3, 12
    sw, d = checker_case(t, k, 11, "r", n=n)
    tol = path_clear_tol(t)
    tried = 0
    for hard in HARD:
        for influence, gain in SOFT:
            for start in (None, path_start(11, n)):
                exp = path_clear_dp(sw, d, t, n, hard, influence, gain, start)
                cand, pen = exp["candidate"], exp["penalty"]
                assert 0 < exp["solved"].sum()
                for i in range(n):
                    ts = np.flatnonzero(cand[:, :, i].any(axis=0))
                    if not len(ts):
                        assert np.isnan(exp["cost"][i]) and (exp["index"][:, i] == -1).all()
                        continue
                    totals = []
                    for pick in itertools.product(*[np.flatnonzero(cand[:, s, i]) for s in ts]):
                        idx = np.full((t, 1), -1, dtype=np.int32)
                        idx[ts, 0] = pick
                        one = {"joints": sw["joints"].reshape(k, t, n, 7)[:, :, i:i + 1].reshape(k, t, 7)}
                        total = clear_cost_along(one, pen[:, :, i:i + 1], idx, t, 1, None if start is None else start[i:i + 1])[0][0]
                        totals.append((total, pick))
                    totals.sort(key=lambda v: v[0])
                    tried += len(totals)
                    assert abs(totals[0][0] - exp["cost"][i]) <= tol, i
                    if len(totals) > 1:
                        assert abs((totals[1][0] - totals[0][0]) - exp["gap"][i]) <= tol, i
                        if totals[1][0] - totals[0][0] > GAP:
                            assert tuple(exp["index"][ts, i]) == tuple(totals[0][1]), i
                    along = np.nansum(exp["step2"][:, i]) + pen[exp["index"][ts, i], ts, i].sum()
                    np.testing.assert_allclose(along, exp["cost"][i], rtol=0, atol=tol)
    assert tried > 1000


@pytest.mark.parametrize("shape", MAIN_SHAPES[:2])
def test_the_dp_is_path_dp_when_nothing_is_blocked_and_the_gain_is_0(shape):
    """min_clearance = -inf with gain 0, and min_clearance = 0 against a d that is 1 m everywhere: index, cost, n_solved, step2 and the
    skipped waypoints are path_dp's exactly, `gap` is path_dp's, blocked is 0."""
    t, k, seed, kind = shape
    n = N_MAIN
    sw, d = checker_case(t, k, seed, kind)
    for start in (None, path_start(seed, n)):
        ref = path_dp(sw, t, n, start)
        for exp in (path_clear_dp(sw, d, t, n, -np.inf, 0.05, 0.0, start), path_clear_dp(sw, np.ones_like(d), t, n, 0.0, 0.05, 100.0, start)):
            for key in ("index", "n_solved", "solved"):
                np.testing.assert_array_equal(exp[key], ref[key], err_msg=key)
            for key in ("cost", "step2"):
                np.testing.assert_array_equal(exp[key].view(np.uint64), ref[key].view(np.uint64), err_msg=key)
            assert (exp["blocked"] == 0).all() and exp["blocked"].dtype == np.uint8
            np.testing.assert_allclose(exp["gap"], ref["gap"], rtol=0, atol=path_clear_tol(t))


@pytest.mark.parametrize("shape", MAIN_SHAPES)
def test_the_inputs_of_the_gpu_tests_satisfy_their_conditions(shape):
    """For every main shape, on the checker's joints and the reference clearance, in all four combinations of the hard constraint and
    the start row: with (0.05, 100) at least 95 % of the paths gap_condition counts have a gap above GAP and no cost reaches
    COST_SUM_MAX; on the three shapes of TABLE_SHAPES the constraint blocks 30 ... 80 % of the candidates, at least 20 solved
    waypoints are lost, at least 20 are partly blocked, at least 15 paths differ from the unconstrained optimum and at least 5 differ
    between gain 0 and gain 100."""
    t, k, seed, kind = shape
    n = N_MAIN
    sw, d = checker_case(t, k, seed, kind)
    on_table = (t, k, seed) in TABLE_SHAPES
    cand_d = d.reshape(k, t, n)[path_clear_dp(sw, d, t, n)["base"]]
    print(f"T {t} K {k} seed {seed}: the candidates' clearance spans {cand_d.min():+.3f} ... {cand_d.max():+.3f} m, median {np.median(cand_d):+.3f}")
    for start in (None, path_start(seed, n)):
        free = path_dp(sw, t, n, start)
        for hard in HARD:
            what = f"T {t} K {k} seed {seed} {kind} start {start is not None} min_clearance {hard}"
            off = path_clear_dp(sw, d, t, n, hard, *SOFT[0], start)
            on = path_clear_dp(sw, d, t, n, hard, *SOFT[1], start)
            gap_condition(on, what + " (0.05, 100)", seeded=start is not None)
            has = on["n_solved"] > 0
            assert (on["cost"][has] < COST_SUM_MAX).all() and (off["cost"][has] < COST_SUM_MAX).all(), what
            print(f"{what}: the largest path cost {float(on['cost'][has].max(initial=0.0)):.1f}, the smallest gap "
                  f"{float(on['gap'][has & (on['n_solved'] > (0 if start is not None else 1))].min(initial=np.inf)):.2e}")
            if on_table:
                soft_condition(off, on, what)
                if hard == 0.0:
                    input_conditions(off, free, what)
