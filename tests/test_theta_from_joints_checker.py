"""What the theta-from-joints GPU tests (tests/test_gpu_theta_from_joints.py) lean on, pinned without a GPU: the CPU checker
reproduces the reference's recorded start thetas and rate-limiter rows (G19, scripts/record_start_theta_golden.py), the C ABI
declares and exports the new entry points at ABI version 8, and the shared workload (tests/theta_workload.py) holds the cases
the GPU tests need — with no near tie of the search in its subsample.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
import theta_workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("r_arm", "l_arm")
TAGS = (("so101", -1.01), ("so003", 0.03))


@pytest.fixture(scope="module")
def g19(golden_dir):
    return np.load(os.path.join(golden_dir, "g19_start_theta.npz"))


def test_checker_reproduces_g19_start_thetas(g19):
    """orc.Solver.best_theta_to_current_joints against the reference's returned theta, 1e-9 (the tolerance of
    test_previous_theta_init_Q15 for the same function); the bracket parsed from the reference's text is the one the table of
    all brackets gives for that theta, and the shortcut rows are the rows the reference answered "preferred_theta worked!"."""
    for a, arm in enumerate(ARMS):
        for tag, so in TAGS:
            pre = f"{arm}_{tag}_"
            pos, eul, cur, pref = (g19[pre + k] for k in ("pos", "eul", "cur", "pref"))
            A = orc.Arm(arm, so)
            theta = np.zeros(len(pos))
            for i in range(len(pos)):
                sv = orc.Solver(A)
                assert sv.is_reachable_no_limits(pos[i], eul[i])
                theta[i] = sv.best_theta_to_current_joints(cur[i], pref[i])
            err = np.max(np.abs(theta - g19[pre + "theta"]))
            print(f"{pre}: theta err {err:.3e}")
            assert err < 1e-9, (pre, err)
            short = np.isnan(g19[pre + "low"])
            assert short.sum() == 16 and np.array_equal(theta[short], pref[short])
            br = W.bracket_of(np.where(short, np.nan, theta), np.full(len(pos), a))
            assert np.array_equal(np.isnan(br[:, 0]), short)
            assert np.nanmax(np.abs(br[:, 0] - g19[pre + "low"])) < 1e-12 and np.nanmax(np.abs(br[:, 1] - g19[pre + "high"])) < 1e-12
            assert (np.abs(cur) > np.pi).any()


def tend(previous_theta, d_theta_max, goal):
    """utils.py:115-127 / 252-264 on the checker's angle_diff."""
    ad = orc.lib().orc_angle_diff(float(goal), float(previous_theta))
    if abs(ad) < d_theta_max:
        return True, float(goal)
    return False, float(previous_theta) + (ad / abs(ad)) * d_theta_max


def cont2(sv, previous_theta, interval, nb, d_theta_max, pref):
    """utils.py:220-264 on the checker's get_best_discrete_theta: (reachable, theta, which text)."""
    found, goal = sv.best_discrete_theta(interval, nb, pref, previous_theta=previous_theta)
    if not found:
        return False, float(previous_theta), 0
    near, th = tend(previous_theta, d_theta_max, goal)
    return True, th, 1 if near else 2


def test_checker_reproduces_g19_rate_limiter(g19):
    """tend_to_preferred_theta and get_best_continuous_theta2 restated on the checker's primitives: booleans and texts exact,
    theta to 1e-12."""
    got = [tend(*row) for row in g19["tend_in"]]
    np.testing.assert_array_equal([g[0] for g in got], g19["tend_ok"].astype(bool))
    assert np.max(np.abs(np.array([g[1] for g in got]) - g19["tend_theta"])) < 1e-12
    assert 0 < g19["tend_ok"].sum() < len(got)
    arms = {(a, so): orc.Arm(ARMS[a], so) for a in (0, 1) for _, so in TAGS}
    n = len(g19["cont2_ok"])
    for i in range(n):
        sv = orc.Solver(arms[(int(g19["cont2_arm"][i]), float(g19["cont2_so"][i]))])
        ok, interval, _ = sv.is_reachable(g19["cont2_pos"][i], g19["cont2_eul"][i])
        prev, i0, i1, dmax, pref = g19["cont2_in"][i]
        assert ok and abs(interval[0] - i0) < 1e-9 and abs(interval[1] - i1) < 1e-9
        good, th, text = cont2(sv, prev, np.array([i0, i1]), 10, dmax, pref)
        assert (good, text) == (bool(g19["cont2_ok"][i]), int(g19["cont2_text"][i])), i
        assert abs(th - g19["cont2_theta"][i]) < 1e-12, (i, th, g19["cont2_theta"][i])
    assert set(g19["cont2_text"].tolist()) == {0, 1, 2}


def test_abi_declares_and_exports_the_entry_points():
    from reachy2_symbolic_ik_amd import _abi

    with open(os.path.join(ROOT, "include", "rsik.h")) as fh:
        header = fh.read()
    assert re.search(r"#define RSIK_ABI_VERSION 8\b", header) and _abi.ABI_VERSION == 8
    for name in ("rsik_theta_from_joints", "rsik_theta_from_joints_state"):
        assert re.search(r"\bint " + name + r"\(rsik_ctx \*ctx, int64_t n,", header), name
        assert name in _abi.PROTOTYPES
    assert re.search(r"#define RSIK_STAGE_TEND_TO_PREFERRED_THETA 17\b", header) and _abi.STAGE_TEND_TO_PREFERRED_THETA == 17
    assert re.search(r"#define RSIK_STAGE_BEST_CONTINUOUS_THETA2 18\b", header) and _abi.STAGE_BEST_CONTINUOUS_THETA2 == 18
    assert re.search(r"#define RSIK_STAGE_COUNT 19\b", header)
    assert _abi.STAGE_ROW[17] == (3, 2) and _abi.STAGE_ROW[18] == (19, 4)
    assert len(_abi.PROTOTYPES["rsik_theta_from_joints"][1]) == 13 and len(_abi.PROTOTYPES["rsik_theta_from_joints_state"][1]) == 10
    lib = _abi.load()                       # (binds every prototype: a missing export raises)
    assert lib.rsik_abi_version() == 8
    assert isinstance(lib.rsik_theta_from_joints, C._CFuncPtr) and isinstance(lib.rsik_theta_from_joints_state, C._CFuncPtr)


def test_utils_module_has_the_reference_names():
    import inspect

    from reachy2_symbolic_ik_amd import utils as U

    assert list(inspect.signature(U.get_best_theta_to_current_joints).parameters) == [
        "get_joints", "nb_search_points", "current_joints", "arm", "preferred_theta"]
    assert list(inspect.signature(U.tend_to_preferred_theta).parameters) == [
        "previous_theta", "interval", "get_joints", "d_theta_max", "goal_theta"]
    assert list(inspect.signature(U.get_best_continuous_theta2).parameters) == [
        "previous_theta", "interval", "get_elbow_position", "nb_search_points", "d_theta_max", "preferred_theta", "arm",
        "singularity_offset", "singularity_limit_coeff", "elbow_singularity_position"]
    assert "live inside the continuous control kernels" not in U.__doc__


def test_bracket_table():
    """16 iterations, 65 536 ends per arm; the replay of a row ends in one of them."""
    for a in (0, 1):
        th, lo, hi = W.bracket_table(a)
        assert len(th) == 1 << 16 and ((hi - lo) <= W.TOLERANCE).all() and ((hi - lo) > W.TOLERANCE * 2 / 3 * 0.99).all()
        assert lo.min() == W.BRACKET0[a][0] and hi.max() == W.BRACKET0[a][1]


def test_workload_holds_the_cases():
    """Both arms inside every wave, shortcut rows, rows whose search moves the solver state through the elbow projection
    (offset 0.03) and none that does without it (-1.01), measured joints beyond +-pi — and no near tie: the replay of the
    16 384-row subsample with the checker's get_joints finds no comparison whose sides are within 1e-9 (cap: 1 row in 10 000)."""
    n = W.N_SUBSAMPLE
    pos, eul, arm, cur = W.theta_workload(W.SEED, n)
    assert 0.45 < arm.mean() < 0.55
    waves = arm.reshape(-1, 64).sum(axis=1)
    assert ((waves > 0) & (waves < 64)).all()
    assert (np.abs(cur) > np.pi).any(axis=1).mean() > 0.1
    ref = W.checker_batch(0.03, pos, eul, arm, cur)
    assert ref["ok"].all()
    print(f"shortcut {ref['shortcut'].mean():.4f}, moved by a projection {ref['moved'].mean():.4f}")
    assert 0.05 < ref["shortcut"].mean() < 0.08 and np.array_equal(ref["theta"][ref["shortcut"]], np.take(W.PREFERRED, arm)[ref["shortcut"]])
    assert ref["moved"].mean() > 0.02
    ref2 = W.checker_batch(-1.01, pos[:2048], eul[:2048], arm[:2048], cur[:2048])
    assert not ref2["moved"].any()
    arms = (orc.Arm("r_arm", 0.03), orc.Arm("l_arm", 0.03))
    ties = W.near_ties(arms, pos, eul, arm, cur)
    print(f"near ties in {n} rows: {ties}")
    assert len(ties) <= n // 10000
    # the replay is the checker's own search: same theta, and its bracket is the table's
    rows = np.arange(0, n, 97)
    rep = [W.replay_row(arms, pos[i], eul[i], arm[i], cur[i], W.PREFERRED[arm[i]]) for i in rows]
    assert np.array_equal([r["theta"] for r in rep], ref["theta"][rows])
    br = W.bracket_of(ref["theta"], arm)[rows]
    for r, b in zip(rep, br):
        assert r["shortcut"] or (r["low"], r["high"]) == (b[0], b[1])
    for r, i in zip(rep, rows):
        np.testing.assert_array_equal(r["solver"][:16], ref["solver"][i][:16])
