"""CPU-side checks of rsik_solve_path: declared, exported, bound with 26 (4) arguments, ABI version still 8, the Python surface exists,
what needs no device (a NULL context, the size helper) — and the expected-value helper of the GPU tests (tests/path_workload.path_dp)
exercised on the checker's tiled sweep: it finds what trying every path finds, it is never worse than the greedy chain, a skipped
waypoint is as good as absent, and the inputs of the GPU tests satisfy the gap condition on their own."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from checker_support import default_arms
from oracle import oracle as orc
from path_workload import (GAP, MAIN_SHAPES, N_MAIN, SMALL_SHAPES, candidates, cost_along, flat, gap_condition, greedy_chain, path_dp,
                           path_fractions, path_poses, path_start, path_tol, transition)
from sweep_workload import expected_tiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def checker_sweep(t, k, seed, kind, n=N_MAIN, thetas=None, policy="fraction"):
    pos, eul, arm = path_poses(seed, n, t, kind)
    th = path_fractions(k) if thetas is None else thetas
    return expected_tiled(orc, default_arms(), flat(pos), flat(eul), np.tile(arm, t), policy, th, nthreads=4)


def test_path_entry_points_are_part_of_abi_8():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert _abi.ABI_VERSION == 8 == L.rsik_abi_version()
    hdr = open(os.path.join(ROOT, "include", "rsik.h")).read()
    assert "#define RSIK_ABI_VERSION 8" in hdr and "#define RSIK_OPT_COUNT 9" in hdr
    for name, count in (("rsik_solve_path", 26), ("rsik_solve_path_workspace_bytes", 4)):
        assert name in _abi.PROTOTYPES and isinstance(getattr(L, name), C._CFuncPtr), name
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert decl, f"include/rsik.h does not declare {name}"
        assert len(decl.group(1).split(",")) == len(_abi.PROTOTYPES[name][1]) == count, name
    assert "#define RSIK_PATH_SKIP_PROJECTED 1" in hdr and "#define RSIK_PATH_UNWIND 2" in hdr
    assert _abi.PATH_SKIP_PROJECTED == 1 and _abi.PATH_UNWIND == 2
    flat_hdr = " ".join(hdr.replace("*", " ").split())  # (whatever the comment's line breaks are)
    assert "the lowest i among equal values" in flat_hdr and "a waypoint can be reachable and skipped" in flat_hdr
    for doc in ("INTEGRATION.md", "README.md"):
        assert "rsik_solve_path" in open(os.path.join(ROOT, doc)).read(), doc


def test_path_entry_point_refuses_a_null_context():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert L.rsik_solve_path(None, 0, 1, None, None, 0, 1, _abi.THETA_FRACTION, None, 0, None, None, 0, None, 0,
                             None, None, None, None, None, None, None, None, None, None, None) == _abi.RSIK_E_INVALID


def test_the_size_helper_needs_no_device_and_is_monotone():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()

    def size(n, t, k):
        b = C.c_size_t(12345)
        rc = L.rsik_solve_path_workspace_bytes(n, t, k, C.byref(b))
        return rc, b.value

    assert size(0, 1, 1) == (_abi.RSIK_OK, 0)
    rc, base = size(37, 12, 8)
    assert rc == _abi.RSIK_OK and base >= 37 * 12 * 8, "the backpointer table alone is n * n_steps * n_theta bytes"
    assert size(38, 12, 8)[1] > base and size(37, 13, 8)[1] > base and size(37, 12, 9)[1] > base
    for n, t in ((1, 1), (5, 7), (4096, 64), (256, 65536)):
        sizes = [size(n, t, k)[1] for k in range(1, 65)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), (n, t)
    for bad in ((-1, 1, 1), (1, 0, 1), (1, 65537, 1), (1, 1, 0), (1, 1, 65)):
        assert size(*bad) == (_abi.RSIK_E_INVALID, 12345), bad
    assert L.rsik_solve_path_workspace_bytes(1, 1, 1, None) == _abi.RSIK_E_INVALID


def test_python_surface_exists():
    from reachy2_symbolic_ik_amd import DualArmIK, HipSolver, SymbolicIK

    for cls, name in ((HipSolver, "solve_path"), (SymbolicIK, "path_batch"), (DualArmIK, "path_batch")):
        fn = getattr(cls, name)
        assert callable(fn) and "index [T, n] int32" in " ".join(fn.__doc__.split()), (cls.__name__, name)


def test_the_dp_finds_what_trying_every_path_finds():
    """T = 4, K = 3, with and without a start row: the cost and (where it is the only minimum) the samples of all 3 ^ 4 paths through
    the solved waypoints, enumerated, against path_dp; `gap` is the enumeration's second-best distinct path minus the best."""
    t, k, n = 4, 3, 12
    ref = checker_sweep(t, k, 11, "r", n=n)
    for start in (None, path_start(11, n)):
        exp = path_dp(ref, t, n, start)
        cand = candidates(ref, t, n)
        assert 0 < exp["solved"].sum() and (exp["n_solved"] >= 3).sum() >= 3
        for i in range(n):
            ts = np.flatnonzero(cand[:, :, i].any(axis=0))
            if not len(ts):
                assert np.isnan(exp["cost"][i]) and (exp["index"][:, i] == -1).all()
                continue
            totals = []
            for pick in itertools.product(*[np.flatnonzero(cand[:, s, i]) for s in ts]):
                idx = np.full((t, 1), -1, dtype=np.int32)
                idx[ts, 0] = pick
                one = {"joints": ref["joints"].reshape(k, t, n, 7)[:, :, i:i + 1].reshape(k, t, 7)}
                totals.append((cost_along(one, idx, t, 1, None if start is None else start[i:i + 1])[0][0], pick))
            totals.sort(key=lambda v: v[0])
            assert abs(totals[0][0] - exp["cost"][i]) <= path_tol(t), i
            if len(totals) > 1:
                assert abs((totals[1][0] - totals[0][0]) - exp["gap"][i]) <= path_tol(t), i
                if totals[1][0] - totals[0][0] > GAP:
                    assert tuple(exp["index"][ts, i]) == tuple(totals[0][1]), i
            np.testing.assert_allclose(np.nansum(exp["step2"][:, i]), exp["cost"][i], rtol=0, atol=path_tol(t))


def test_a_duplicated_sample_gives_the_lower_one():
    """Explicit angles with samples 1 and 2 equal: whatever the optimum, sample 2 never appears (the lowest index among equal values)."""
    t, n = 6, 20
    th = np.array([0.3, -1.1, -1.1, 2.0])
    ref = checker_sweep(t, 4, 11, "r", n=n, thetas=th, policy="explicit")
    exp = path_dp(ref, t, n, path_start(11, n))
    assert (exp["index"] == 1).sum() >= 5 and not (exp["index"] == 2).any()


def test_a_skipped_waypoint_is_as_good_as_absent():
    """A path whose middle (first, last) waypoint has no candidate gives, at the other waypoints, what the path without it gives."""
    t, k, n = 6, 4, 10
    ref = checker_sweep(t, k, 11, "r", n=n)
    start = path_start(11, n)
    for gone in (0, 3, t - 1):
        holed = {key: v.copy() for key, v in ref.items()}
        holed["reachable"].reshape(t, n)[gone] = 0
        keep = [s for s in range(t) if s != gone]
        short = {"joints": ref["joints"].reshape(k, t, n, 7)[:, keep].reshape(k, (t - 1) * n, 7),
                 "projected": ref["projected"].reshape(k, t, n)[:, keep].reshape(k, -1), "reachable": ref["reachable"].reshape(t, n)[keep].reshape(-1)}
        a, b = path_dp(holed, t, n, start), path_dp(short, t - 1, n, start)
        assert (a["index"][gone] == -1).all() and np.isnan(a["step2"][gone]).all()
        np.testing.assert_array_equal(a["index"][keep], b["index"])
        np.testing.assert_array_equal(a["cost"], b["cost"])
        np.testing.assert_array_equal(a["step2"][keep], b["step2"])


@pytest.mark.parametrize("shape", MAIN_SHAPES + tuple(s[:4] for s in SMALL_SHAPES[:2]))
def test_the_inputs_of_the_gpu_tests_satisfy_the_gap_condition(shape):
    """For every main shape of tests/test_gpu_solve_path.py, on the checker's joints, with and without a start row: at least 95 % of
    the paths with a solved waypoint have a second-best distinct path more than GAP above the optimum, the skip rule is exercised by
    the inputs themselves, and the optimum is never worse than the greedy chain."""
    t, k, seed, kind = shape
    n = N_MAIN
    ref = checker_sweep(t, k, seed, kind)
    for start in (None, path_start(seed, n)):
        exp = path_dp(ref, t, n, start)
        what = f"T {t} K {k} seed {seed} {kind} start {start is not None}"
        if k > 1 and (t > 1 or start is not None):  # (one sample, or one waypoint nothing is measured against: one path, no second)
            gap_condition(exp, what, seeded=start is not None)
        if t >= 5:
            assert 0 < (~exp["solved"]).sum() and (exp["solved"].all(axis=0)).sum() < n, "the main shapes hold skipped waypoints"
        along, step2 = cost_along(ref, exp["index"], t, n, start)
        has = exp["n_solved"] > 0
        assert has.sum() >= n // 2
        assert (np.abs(along[has] - exp["cost"][has]) <= path_tol(t)).all() and np.isnan(exp["cost"][~has]).all()
        np.testing.assert_array_equal(step2, exp["step2"])
        greedy, _ = cost_along(ref, greedy_chain(ref, t, n, start), t, n, start)
        assert (exp["cost"][has] <= greedy[has] + path_tol(t)).all(), what
        better = int((greedy[has] - exp["cost"][has] > GAP).sum())
        print(f"{what}: the optimum beats the greedy chain on {better} of {int(has.sum())} paths, "
              f"median ratio {float(np.median(exp['cost'][has] / np.maximum(greedy[has], 1e-300))):.2f}")
        if (t, k, seed) == (12, 8, 11) and start is None:
            assert better >= 10, "the GPU test asks for at least 10"
    assert GAP == 1e-9


def test_transition_is_nearests_cost():
    from nearest_workload import costs

    rng = np.random.default_rng(5)
    j, s, w = rng.uniform(-3, 3, (4, 9, 7)), rng.uniform(-3, 3, (9, 7)), rng.uniform(0, 2, 7)
    np.testing.assert_array_equal(transition(s[None], j, w), costs(j, s, w))
