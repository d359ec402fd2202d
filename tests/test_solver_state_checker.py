"""Pins what the solver-state GPU tests (tests/test_gpu_solver_state.py) lean on, on the CPU checker alone.

Those tests compare rsik_reach_state / rsik_joints_from_state / rsik_elbow_from_state, launched as batches, with the checker's
stateful solver object (oracle.Solver, one per row) and, at full size, with the checker's OpenMP batch.  Here, without a GPU:
the batch is the object bit for bit; the object reproduces the reference's own numbers (G3); and the seeded sample both files
draw from holds every case the GPU tests need, in shares large enough to mean something.
"""
import os

import numpy as np

from checker_support import ELBOW_LIMIT, SHOULDER_Y, CheckerRows, _check_symbolic, state_workload
from compare import bits
from oracle import oracle as orc


def test_batch_is_the_object_row_by_row():
    """orc.solve_batch (OpenMP, mixed arms, every outcome) is orc.Solver.is_reachable followed by one get_joints(interval[0]),
    bit for bit in every output: this is what lets the full-size GPU test take the batch as the reference of the first call."""
    n = 30000
    pos, eul, arm = state_workload(7, n)
    R, L = orc.Arm("r_arm", 0.03), orc.Arm("l_arm", 0.03)
    ref = orc.solve_batch(R, L, pos, eul, arm_id=arm, nthreads=min(4, os.cpu_count() or 1))
    rows = CheckerRows(arm, arms=(R, L))
    got = rows.reach(pos, eul)
    np.testing.assert_array_equal(got["reachable"], ref["reachable"])
    np.testing.assert_array_equal(got["state"], ref["state"])
    np.testing.assert_array_equal(bits(got["interval"]), bits(ref["interval"]))
    m = np.flatnonzero(ref["reachable"])
    assert len(m) > 0.04 * n and 0.3 < arm[m].mean() < 0.7
    out = rows.joints(got["interval"][:, 0], rows=m)
    for k in ("joints", "elbow"):
        np.testing.assert_array_equal(bits(out[k][m]), bits(ref[k][m]), err_msg=k)
        assert np.isnan(ref[k][ref["reachable"] == 0]).all(), k
    np.testing.assert_array_equal(out["projected"][m], ref["projected"][m])
    assert ref["projected"][ref["reachable"] == 0].sum() == 0


def test_object_reproduces_g3(golden_dir):
    """G3 (the reference's own numbers: both arms, singularity_offset 0.03 and -1.01, theta = interval[0] and the recorded
    interior theta) through the checker's solver OBJECT, one per row, at the bar test_oracle_golden.py holds the batch to."""
    g = np.load(os.path.join(golden_dir, "g3_reachable.npz"))
    for a, arm in enumerate(("r_arm", "l_arm")):
        pos, eul = g[f"{arm}_pos"], g[f"{arm}_eul"]
        n = len(pos)
        for tag, so in (("so003", 0.03), ("so101", -1.01)):
            for kind in ("i0", "in"):
                pre = f"{arm}_{tag}_{kind}_"
                rows = CheckerRows(np.full(n, a, dtype=np.uint8), so=so)
                res = rows.reach(pos, eul)
                m = np.flatnonzero(res["reachable"])
                theta = res["interval"][:, 0] if kind == "i0" else g[pre + "theta"]
                res.update(rows.joints(theta, rows=m))
                _check_symbolic(res, g, pre)
        assert (g[f"{arm}_so003_i0_elbow_len"] == 3).mean() > 0.1


def test_sample_holds_the_cases():
    """The shares of state_workload the GPU tests rest on, asserted on the checker alone (singularity_offset 0.03; measured on
    20 000 - 40 000 rows: reachable 6-9 %, projection at the first get_joints 34-37 % of those, refused before any geometry slot is
    written 68-76 %, elbow pitch on its +-127 degree clamp 6.1 % of the solved rows, is_reachable_no_limits succeeds everywhere)."""
    n = 30000
    pos, eul, arm = state_workload(11, n)
    assert 0.45 < arm.mean() < 0.55
    waves = arm[: n - n % 64].reshape(-1, 64).sum(axis=1)
    assert ((waves > 0) & (waves < 64)).all(), "r and l must alternate inside every wave"
    sentinel = 1000.0 + np.arange(19.0)
    rows = CheckerRows(arm, init=np.tile(sentinel, (n, 1)))
    res = rows.reach(pos, eul)
    assert set(np.unique(res["state"]).tolist()) >= {0, 1, 2, 3, 4}
    ok = res["reachable"].astype(bool)
    assert ok.mean() >= 0.04
    early = np.isin(res["state"], (1, 2))
    untouched = (rows.buf[:, :16] == sentinel[:16]).all(axis=1)
    np.testing.assert_array_equal(untouched, early)          # the early refusals, and only they, assign nothing
    assert early.mean() >= 0.50
    wrist_only = res["state"] == 3                          # "wrist out of range": goal and wrist assigned, the circle not
    assert (rows.buf[wrist_only, 9:16] == sentinel[9:16]).all() and (rows.buf[wrist_only, 0:9] != sentinel[0:9]).all()
    assert (rows.buf[ok | (res["state"] == 4)][:, :16] != sentinel[:16]).all()
    assert (rows.buf[:, 16:] == sentinel[16:]).all()         # is_reachable never touches the elbow
    m = np.flatnonzero(ok)
    out = rows.joints(res["interval"][:, 0], rows=m)
    assert out["projected"][m].mean() >= 0.20
    clamp = np.abs(np.abs(out["joints"][m, 3]) - ELBOW_LIMIT) < 1e-12
    assert clamp.mean() <= 0.10
    # uniform arms draw from the same box around their own shoulder
    for a in (0, 1):
        p1, e1, b1 = state_workload(11, 4000, arm=a)
        assert (b1 == a).all() and abs(p1[:, 1].mean() - SHOULDER_Y[a]) < 0.05
        assert CheckerRows(b1).reach(p1, e1)["reachable"].mean() >= 0.04
    # is_reachable_no_limits: every row of the sample, interval [-pi, pi]
    nl = CheckerRows(arm[:10000]).reach(pos[:10000], eul[:10000], no_limits=True)
    assert nl["reachable"].all() and (nl["interval"] == (-np.pi, np.pi)).all()
