"""CPU-side checks of rsik_clearance_edges: declared, exported, bound with 25 arguments, ABI version still 8 and RSIK_OPT_COUNT still 9,
a NULL context refused, the workspace function monotone, the Python surface exists, the documents name the symbol — and the
expected-value helper of the GPU tests (tests/clearance_edges_workload.py) on the checker's tiled sweep, path_clear_dp's winners
(min_clearance 0, (0.05, 100), start rows) and clearance_workload.reference as d: the conditions on the inputs that
tests/test_gpu_clearance_edges.py relies on.  They are conditions, not measurements; the figures in brackets are what the reference
gave when they were set."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import clearance_edges_workload as EW
from checker_support import default_arms
from oracle import oracle as orc
from path_clear_workload import TABLE_SHAPES, checker_clearance, path_clear_dp
from path_workload import MAIN_SHAPES, N_MAIN, flat, path_fractions, path_poses, path_start
from sweep_workload import expected_tiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rsik_clearance_edges"
SHAPES = tuple(s for s in MAIN_SHAPES if s[:3] in TABLE_SHAPES)  # (12, 8, 11, r), (70, 3, 21, mixed), (5, 64, 31, mixed)


# ------------------------------------------------------------------------------------------ surface
def test_the_entry_point_is_part_of_abi_8():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert _abi.ABI_VERSION == 8 == L.rsik_abi_version()
    hdr = open(os.path.join(ROOT, "include", "rsik.h")).read()
    assert "#define RSIK_ABI_VERSION 8" in hdr and "#define RSIK_OPT_COUNT 9" in hdr
    for name, count in ((NAME, 25), (NAME + "_workspace_bytes", 3)):
        assert name in _abi.PROTOTYPES and isinstance(getattr(L, name), C._CFuncPtr), name
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert decl, f"include/rsik.h does not declare {name}"
        assert len(decl.group(1).split(",")) == len(_abi.PROTOTYPES[name][1]) == count, name
    flat_hdr = " ".join(hdr.replace("*", " ").split())  # (whatever the comment's line breaks are)
    for words in ("NOT A WAYPOINT", "1-Lipschitz", "is never below edge_bound", "the lowest s that attains it"):
        assert words in flat_hdr, words
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md", os.path.join("docs", "experiments.md"), os.path.join("scripts", "README.md")):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc
    assert "CE.1" in open(os.path.join(ROOT, "docs", "experiments.md")).read()
    assert os.path.exists(os.path.join(ROOT, "scripts", "clearance_edges_cost.py"))


def test_the_entry_point_refuses_a_null_context():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    args = [None, 0, 1, None, None, 0, None, 16, None, 1, None, 0, None, 0.0, None, 0]
    assert L.rsik_clearance_edges(*args, *([None] * 9)) == _abi.RSIK_E_INVALID


def test_the_workspace_function_is_monotone():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()

    def ws(n, t):
        b = C.c_size_t(123)
        rc = L.rsik_clearance_edges_workspace_bytes(n, t, C.byref(b))
        return rc, b.value

    last = -1
    for n, t in ((0, 1), (1, 1), (1, 2), (2, 2), (37, 12), (37, 70), (130, 70), (4096, 64), (4096, 65536)):
        rc, b = ws(n, t)
        assert rc == _abi.RSIK_OK and b >= last and b % 8 == 0 and b >= 20 * n * t, (n, t, b)
        last = b
    for n, t in ((-1, 1), (1, 0), (1, 65537), (2 ** 62, 65536)):
        assert ws(n, t) == (_abi.RSIK_E_INVALID, 123), (n, t)
    assert L.rsik_clearance_edges_workspace_bytes(1, 1, None) == _abi.RSIK_E_INVALID


def test_python_surface_exists():
    from reachy2_symbolic_ik_amd import DualArmIK, HipSolver, SymbolicIK

    for cls, name in ((HipSolver, "clearance_edges"), (SymbolicIK, "clearance_edges_batch"), (DualArmIK, "clearance_edges_batch")):
        fn = getattr(cls, name)
        doc = " ".join(fn.__doc__.split())
        assert callable(fn) and "edge_bound" in doc and "n_sub" in doc, (cls.__name__, name)
    assert NAME in HipSolver.clearance_edges.__doc__
    assert HipSolver.CLEARANCE_EDGES_OUTPUTS == ("edge_clearance", "edge_sub", "edge_nearest", "edge_bound", "path_clearance",
                                                 "path_edge", "path_bound", "n_below", "first_below")


# ------------------------------------------------------------------------------------------ the helper on the checker's sweep
@functools.lru_cache(maxsize=None)
def winners(shape):
    """The joints [T,n,7] path_clear_dp picks on the checker's tiled sweep of a shape (NaN at a skipped waypoint), the arm bytes and
    the start rows."""
    t, k, seed, kind = shape
    n = N_MAIN
    pos, eul, arm = path_poses(seed, n, t, kind)
    sw = expected_tiled(orc, default_arms(), flat(pos), flat(eul), np.tile(arm, t), "fraction", path_fractions(k), nthreads=4)
    d = checker_clearance(sw, np.tile(arm, t))
    start = path_start(seed, n)
    idx = path_clear_dp(sw, d, t, n, 0.0, 0.05, 100.0, start)["index"]
    J = np.asarray(sw["joints"]).reshape(k, t, n, 7)
    tt, ii = np.nonzero(idx >= 0)
    joints = np.full((t, n, 7), np.nan)
    joints[tt, ii] = J[idx[tt, ii], tt, ii]
    return joints, arm, start


@functools.lru_cache(maxsize=None)
def on_checker(shape, n_sub):
    joints, arm, start = winners(shape)
    return EW.expected(joints, arm, n_sub, EW.reference_clearance(arm), start)


def test_the_helper_s_edges_samples_and_folds():
    """A hand-made path: a NaN row is bridged, the first waypoint without a start row is the one sample s = S, a start row that is
    not numbers loses its path alone, the samples are a + delta * (s / S) the short way round, and the folds take the first minimum."""
    J = np.zeros((4, 3, 7))
    J[:, 0, 0] = [3.0, np.nan, -3.0, -2.0]
    J[:, 1, 0] = [0.5, 1.0, 1.5, np.inf]
    J[:, 2, 0] = [0.1, 0.2, 0.3, 0.4]
    wp, have_a, a = EW.edges_of(J)
    assert wp.tolist() == [[True, True, True], [False, True, True], [True, True, True], [True, False, True]]
    assert have_a.tolist() == [[False] * 3, [False, True, True], [True, True, True], [True, False, True]]
    assert a[2, 0, 0] == 3.0 and a[3, 0, 0] == -3.0 and a[2, 1, 0] == 1.0
    q, valid, delta = EW.samples(a, J, have_a, wp, 4)
    assert valid[:, 0, 0].tolist() == [False] * 4 + [True] and valid[:, 1, 0].tolist() == [False] * 5 and valid[:, 2, 0].all()
    assert abs(delta[2, 0, 0] - (2 * np.pi - 6.0)) < 1e-15 and q[4, 2, 0, 0] == -3.0 and q[0, 2, 0, 0] == 3.0
    assert q[2, 2, 0, 0] == 3.0 + delta[2, 0, 0] * 0.5 > 3.0  # the short way round: through pi, not through 0
    start = np.zeros((3, 7))
    start[1, 3] = np.nan
    wp2, have2, _ = EW.edges_of(J, start)
    assert not wp2[:, 1].any() and wp2[:, [0, 2]].tolist() == wp[:, [0, 2]].tolist() and have2[0].tolist() == [True, False, True]
    d = np.array([[0.3], [0.1], [0.1], [np.inf]])
    near = np.arange(8, dtype=np.int32).reshape(4, 1, 2)
    ok = np.ones((4, 1), dtype=bool)
    ec, es, en = EW.fold_samples(d, near, ok, np.array([True]))
    assert (ec[0], es[0], en[0].tolist()) == (0.1, 1, [2, 3])
    ec, es, en = EW.fold_samples(np.full((4, 1), np.inf), np.full((4, 1, 2), -1, dtype=np.int32), ok & (np.arange(4) >= 2)[:, None], np.array([True]))
    assert (ec[0], es[0], en[0].tolist()) == (np.inf, 2, [-1, -1])
    out = EW.fold_paths(np.array([[0.2, np.nan], [0.1, np.nan], [0.1, np.nan]]), np.array([[3, -1], [0, -1], [2, -1]]),
                        np.array([[0.0, np.nan], [0.05, np.nan], [-0.1, np.nan]]), 0.15)
    assert out["path_clearance"][0] == 0.1 and out["path_edge"].tolist() == [[1, 0], [-1, -1]] and out["path_bound"][0] == -0.1
    assert out["n_below"].tolist() == [2, 0] and out["first_below"].tolist() == [1, -1] and np.isnan(out["path_clearance"][1])


def test_edges_dip_between_clear_waypoints():
    """S = 16 on (12, 8, 11, r): at least 10 % of the edges have a minimum more than 1e-3 m below both ends [17.0 %] and at least 50 %
    have edge_bound > 0 [66.8 %]; on (70, 3, 21, mixed) at least 90 % have edge_bound > 0 [93.9 %]."""
    for shape, dip_share, free_share in ((SHAPES[0], 0.10, 0.50), (SHAPES[1], None, 0.90)):
        exp = on_checker(shape, 16)
        edges = int(exp["wp"].sum())
        dip = EW.dips(exp).sum() / edges
        with np.errstate(invalid="ignore"):
            free = (exp["edge_bound"] > 0).sum() / edges
            ends = np.where(exp["have_a"], np.minimum(exp["d"][0], exp["d"][-1]), exp["d"][-1])[exp["wp"]]
            neg = ((ends < 0).mean(), (exp["edge_clearance"][exp["wp"]] < 0).mean())
            deepest = float((ends - exp["edge_clearance"][exp["wp"]]).max())
        print(f"{shape}: {edges} edges, {100 * dip:.1f} % dip, deepest {deepest:.3f} m, {100 * free:.1f} % with edge_bound > 0, negative "
              f"clearance at the ends {100 * neg[0]:.1f} % -> over 16 sub-steps {100 * neg[1]:.1f} %")
        assert shape[:3] == (12, 8, 11) or shape[:3] == (70, 3, 21)
        if dip_share is not None:
            assert dip >= dip_share, (shape, dip)
        assert free >= free_share, (shape, free)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_bound_lies_below_a_finer_sampling(shape):
    """On all three table shapes and S in {4, 16}: edge_bound <= the minimum over 128 sub-steps + 1e-9 on every edge [it held on all
    1805 edges; smallest slack 2e-4 m at S = 16]."""
    fine = on_checker(shape, EW.FINE)["edge_clearance"]
    for n_sub in (4, 16):
        exp = on_checker(shape, n_sub)
        wp = exp["wp"]
        slack = (fine - exp["edge_bound"])[wp]
        print(f"{shape} S {n_sub}: {int(wp.sum())} edges, smallest (minimum over {EW.FINE} sub-steps - edge_bound) {float(slack.min()):.3e} m")
        assert (slack >= -EW.BOUND_SLACK).all(), (shape, n_sub, float(slack.min()))
        assert (exp["edge_bound"][wp] <= exp["edge_clearance"][wp]).all()
        np.testing.assert_array_equal(exp["path_clearance"], np.where(wp.any(axis=0), np.nanmin(np.where(wp, exp["edge_clearance"], np.inf), axis=0), np.nan))
