"""CPU-side checks of rsik_solve_path_pair: both symbols declared, exported and bound with the header's argument count, ABI version
still 8 and RSIK_OPT_COUNT still 9, a NULL context refused, the Python surface exists, the documents name the entry point — and the
expected-value helper of the GPU tests (tests/path_pair_workload.path_pair_dp) exercised on the checker's tiled sweep with
track_pair_workload.clearance as d: it finds what trying every path finds, it is path_dp row by row where nothing couples the arms,
and the inputs of the GPU tests satisfy the conditions those tests rely on."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import path_pair_workload as PP
from checker_support import default_arms
from oracle import oracle as orc
from path_workload import GAP, flat, path_dp, path_fractions, path_start
from sweep_workload import expected_tiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rsik_solve_path_pair"


@functools.lru_cache(maxsize=None)
def checker_case(t, k, seed, robots, scene=False):
    """The checker's tiled sweep over a shape's poses and the reference's two views of every pair of its samples."""
    pos, eul, arm = PP.pair_poses(seed, robots, t)
    sw = expected_tiled(orc, default_arms(), flat(pos), flat(eul), np.tile(arm, t), "fraction", path_fractions(k), nthreads=4)
    d = PP.checker_pair_clearance(sw, t, robots, PP.the_scene() if scene else None)
    d.setflags(write=False)
    return sw, d


def test_the_entry_points_are_part_of_abi_8():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert _abi.ABI_VERSION == 8 == L.rsik_abi_version()
    hdr = open(os.path.join(ROOT, "include", "rsik.h")).read()
    assert "#define RSIK_ABI_VERSION 8" in hdr and "#define RSIK_OPT_COUNT 9" in hdr
    for name in (NAME, NAME + "_workspace_bytes"):
        assert name in _abi.PROTOTYPES and isinstance(getattr(L, name), C._CFuncPtr), name
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert decl, f"include/rsik.h does not declare {name}"
        assert len(decl.group(1).split(",")) == len(_abi.PROTOTYPES[name][1]), name
    assert len(_abi.PROTOTYPES[NAME][1]) == 35 and len(_abi.PROTOTYPES[NAME + "_workspace_bytes"][1]) == 4
    flat_hdr = " ".join(hdr.replace("*", " ").split())  # (whatever the comment's line breaks are)
    assert "the lowest a n_theta + b among equal values" in flat_hdr and "pR first, then one sum" in flat_hdr
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md", os.path.join("docs", "experiments.md"), os.path.join("scripts", "README.md")):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc


def test_the_entry_point_refuses_a_null_context_and_the_workspace_query_its_arguments():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    args = [None, 0, 1, None, 1, _abi.THETA_FRACTION, None, 0, None, None, 0, None, 0, None, 0, None, 0.0, 0.0, 0.0, None, 0]
    assert L.rsik_solve_path_pair(*args, *([None] * 14)) == _abi.RSIK_E_INVALID
    b = C.c_size_t(0)
    q = L.rsik_solve_path_pair_workspace_bytes
    assert q(3, 5, 16, None) == _abi.RSIK_E_INVALID
    for bad in ((-1, 5, 4), (3, 0, 4), (3, 65537, 4), (3, 5, 0), (3, 5, 17)):
        assert q(*bad, C.byref(b)) == _abi.RSIK_E_INVALID, bad
    sizes = {}
    for n_pairs in (0, 1, 7):
        for t in (1, 2, 70):
            for k in (1, 3, 16):
                assert q(n_pairs, t, k, C.byref(b)) == _abi.RSIK_OK
                sizes[n_pairs, t, k] = b.value
                assert b.value >= n_pairs * t * k * k, "a backpointer byte per state"
    for (n_pairs, t, k), v in sizes.items():  # monotone in each argument
        for other, w in sizes.items():
            if other[0] >= n_pairs and other[1] >= t and other[2] >= k:
                assert w >= v, ((n_pairs, t, k), other)


def test_python_surface_exists():
    from reachy2_symbolic_ik_amd import DualArmIK, HipSolver

    for cls, name in ((HipSolver, "solve_path_pair"), (DualArmIK, "path_pair_batch")):
        fn = getattr(cls, name)
        doc = " ".join(fn.__doc__.split())
        assert callable(fn) and NAME in doc and "min_clearance" in doc and "blocked" in doc and "nearest" in doc, (cls.__name__, name)
    assert callable(HipSolver.solve_path_pair_workspace_bytes)


def test_the_dp_finds_what_trying_every_path_finds():
    """T = 4, K = 3, 3 robots, without and with the scene, both hard constraints and both parameter pairs, with and without start
    rows: the cost (penalties included), the gap and, where the gap exceeds GAP, the samples against every path through the candidate
    pairs of the solved waypoints, enumerated."""
    t, k, robots = 4, 3, 3
    tol = PP.path_pair_tol(t)
    tried = 0
    for scene in (False, True):
        sw, d = checker_case(t, k, 11, robots, scene)
        for hard in PP.HARD:
            for influence, gain in PP.SOFT:
                for start in (None, path_start(11, 2 * robots)):
                    exp = PP.path_pair_dp(sw, d, t, robots, hard, influence, gain, start)
                    assert exp["solved"].sum() > 0
                    for i in range(robots):
                        ts, costs, paths = PP.every_path(sw, exp, i, t, robots, start)
                        if not len(ts):
                            assert np.isnan(exp["cost"][i]) and (exp["index"][:, 2 * i:2 * i + 2] == -1).all()
                            continue
                        tried += len(costs)
                        assert abs(costs[0] - exp["cost"][i]) <= tol, (i, costs[0], exp["cost"][i])
                        assert (exp["index"][:, 2 * i] >= 0).sum() == len(ts) == exp["n_solved"][i]
                        if len(costs) > 1:
                            assert abs((costs[1] - costs[0]) - exp["gap"][i]) <= tol, (i, costs[1] - costs[0], exp["gap"][i])
                            if costs[1] - costs[0] > GAP:
                                np.testing.assert_array_equal(exp["index"][ts, 2 * i:2 * i + 2], paths[0], err_msg=str(i))
                        along = PP.pair_cost_along(sw, exp["penalty"], exp["index"], t, robots, start)[0][i]
                        assert abs(along - exp["cost"][i]) <= tol, i
    print(f"{tried} paths tried")
    assert tried > 1000


@pytest.mark.parametrize("shape", PP.MAIN_SHAPES[:2])
def test_the_dp_is_path_dp_per_row_when_nothing_couples_the_arms(shape):
    """d = 1 m everywhere with min_clearance 0 and gain 0, and the true d with min_clearance = -inf and gain 0: on robots all of whose
    waypoints are solved for both arms the index rows are path_dp's of the same rows exactly, and the cost is the sum of the two
    within path_pair_tol."""
    t, k, seed, robots = shape
    n = 2 * robots
    sw, d = checker_case(t, k, seed, robots)
    tol = PP.path_pair_tol(t)
    whole_seen = 0
    for start in (None, path_start(seed, n)):
        ref = path_dp(sw, t, n, start)
        whole = ref["solved"].reshape(t, robots, 2).all(axis=(0, 2))
        whole_seen += int(whole.sum())
        for exp in (PP.path_pair_dp(sw, np.ones_like(d), t, robots, 0.0, 0.05, 0.0, start),
                    PP.path_pair_dp(sw, d, t, robots, -np.inf, 0.05, 0.0, start)):
            assert (exp["blocked"] == 0).all() and exp["blocked"].dtype == np.uint16
            rows = np.repeat(whole, 2)
            np.testing.assert_array_equal(exp["index"][:, rows], ref["index"][:, rows])
            both = ref["cost"].reshape(robots, 2).sum(axis=1)
            assert (np.abs(exp["cost"][whole] - both[whole]) <= tol).all(), float(np.abs(exp["cost"][whole] - both[whole]).max(initial=0.0))
    assert whole_seen >= 2, "robots whose waypoints are all solved for both arms"


@pytest.mark.parametrize("shape", PP.MAIN_SHAPES)
def test_the_inputs_of_the_gpu_tests_satisfy_their_conditions(shape):
    """For every main shape, without and with the scene, on the checker's joints and the reference clearance, in all combinations of
    the hard constraint, the soft term and the start rows: no path cost reaches COST_SUM_MAX and every robot the gap condition counts
    has a gap above GAP.  On (12, 8, 11, 19) without a scene: min_clearance 0 changes at least one robot's path, the soft term alone
    changes at least one, at least one solved waypoint is lost and at least ten cells are partly blocked."""
    t, k, seed, robots = shape
    n = 2 * robots
    for scene in (False, True):
        sw, d = checker_case(t, k, seed, robots, scene)
        exps = {}
        for start in (None, path_start(seed, n)):
            for hard in PP.HARD:
                for influence, gain in PP.SOFT:
                    what = f"T {t} K {k} seed {seed} robots {robots} scene {scene} start {start is not None} min_clearance {hard} ({influence}, {gain})"
                    exp = PP.path_pair_dp(sw, d, t, robots, hard, influence, gain, start)
                    exps[start is not None, hard, gain] = exp
                    solved = exp["n_solved"] > 0
                    top = float(exp["cost"][solved].max(initial=0.0))
                    assert top < PP.COST_SUM_MAX, (what, top)
                    has, gaps = PP.pair_gap_condition(exp, what, seeded=start is not None)
                    print(f"{what}: the largest path cost {top:.1f}")
                    assert (gaps > GAP).all(), (what, np.flatnonzero(has)[gaps <= GAP].tolist(), gaps.min())
        if shape == PP.MAIN_SHAPES[0] and not scene:
            for seeded in (False, True):
                free, con = exps[seeded, -np.inf, 0.0], exps[seeded, 0.0, 0.0]
                soft, both = exps[seeded, -np.inf, 100.0], exps[seeded, 0.0, 100.0]
                with_solved = int((free["n_solved"] > 0).sum())
                hard_differs = int((con["index"] != free["index"]).any(axis=0).reshape(robots, 2).any(axis=1).sum())
                soft_differs = int((soft["index"] != free["index"]).any(axis=0).reshape(robots, 2).any(axis=1).sum())
                both_differ = int((both["index"] != free["index"]).any(axis=0).reshape(robots, 2).any(axis=1).sum())
                lost = int((free["solved"] & ~con["solved"]).sum())
                partly = int((con["solved"] & (con["blocked"] > 0)).sum())
                both_rows = free["row"][:, None, :, 0::2] & free["row"][None, :, :, 1::2]
                cross = d[both_rows]
                print(f"start {seeded}: {with_solved} robots with a solved waypoint; min_clearance 0 changes {hard_differs}, the soft term {soft_differs}, "
                      f"both {both_differ}; {lost} solved waypoints lost, {partly} cells partly blocked; of the pairs of row candidates "
                      f"{float((cross.min(axis=-1) < 0).mean()):.3f} penetrate and {float((cross.min(axis=-1) < 0.05).mean()):.3f} are within 0.05 m; "
                      f"the two views differ on {float((cross[:, 0] != cross[:, 1]).mean()):.2f} of them, by at most {float(np.abs(cross[:, 0] - cross[:, 1]).max()):.1e}")
                assert hard_differs >= 1 and soft_differs >= 1 and lost >= 1 and partly >= 10, (hard_differs, soft_differs, lost, partly)
