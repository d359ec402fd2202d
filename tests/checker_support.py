"""What the tests share of the CPU checker (oracle/): seeded samples, the checker's solver object row by row, the default and the
custom arms, and the comparisons against the reference's recordings that both the checker's tests and the GPU tests hold their
results to.  NumPy and the checker only: nothing here touches the product.  No test in this file: pytest does not rewrite its
asserts, so every one of them carries its own message."""
import os

import numpy as np

import scale_inputs as SC
from compare import TOL, singular_rows
from oracle import oracle as orc

SHOULDER_Y = (-0.2, 0.2)            # r, l (symbolic_ik.py:40-51)
ELBOW_LIMIT = np.radians(127.0)     # symbolic_ik.py:72, 853-861

CUSTOM_GEOMETRY = dict(  # must match oracle/gen_golden.py CUSTOM_GEOMETRY (G9)
    ik_parameters={
        "r_shoulder_position": np.array([0.012, -0.185, 0.021]), "r_shoulder_orientation": [-11.0, 3.5, 7.0],
        "r_upper_arm_size": 0.305, "r_forearm_size": 0.262, "r_tip_position": np.array([0.013, -0.008, 0.094]),
        "l_shoulder_position": np.array([0.012, 0.185, 0.021]), "l_shoulder_orientation": [11.0, 3.5, -7.0],
        "l_upper_arm_size": 0.305, "l_forearm_size": 0.262, "l_tip_position": np.array([0.013, 0.008, 0.094]),
    },
    elbow_limit=115, wrist_limit=38.0, backward_limit=0.035, singularity_offset=0.05, singularity_limit_coeff=0.8)


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def default_arms(so=0.03):
    """The checker's default arm pair (r, l) with singularity_offset `so`."""
    return orc.Arm("r_arm", so), orc.Arm("l_arm", so)


# ------------------------------------------------------------------------------------------ seeded samples
def state_workload(seed, n, arm=None):
    """The sample of the solver-state tests: positions from the smoke() box around the row's own shoulder ([0, -+0.2, 0] +- 0.6),
    Euler angles from +-pi and one arm byte per row (0 = r, 1 = l) — random, so r and l alternate inside every 64-lane wave and
    across every 256-thread block, or the same `arm` in every row.  Returns pos [n,3], eul [n,3], arm [n] uint8."""
    rng = np.random.default_rng(seed)
    box = rng.uniform(-0.6, 0.6, size=(n, 3))
    eul = rng.uniform(-np.pi, np.pi, size=(n, 3))
    byte = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    if arm is not None:
        byte = np.full(n, int(arm), dtype=np.uint8)
    pos = box + np.stack([np.zeros(n), np.where(byte == 1, SHOULDER_Y[1], SHOULDER_Y[0]), np.zeros(n)], axis=1)
    return pos, eul, byte


def reachable_rich(seed, n, arm):
    """The poses of test_ragged_sizes_match_checker (most of them reachable), mirrored for the rows of the left arm."""
    rng = np.random.default_rng(seed)
    pos = np.array([0.25, -0.2, -0.15]) + rng.uniform(-0.25, 0.25, size=(n, 3))
    eul = np.array([0, -np.pi / 2, 0]) + rng.uniform(-0.8, 0.8, size=(n, 3))
    sgn = np.where(np.asarray(arm) == 1, -1.0, 1.0)
    return pos * np.stack([np.ones(n), sgn, np.ones(n)], axis=1), eul * np.stack([sgn, np.ones(n), sgn], axis=1)


# ------------------------------------------------------------------------------------------ the checker's object, row by row
class CheckerRows:
    """n independent solver objects of the checker (one orc_solver_t per row: slots 0-15 laid out like the device row, 16-18 the
    elbow of the last get_joints), stepped row by row on the host the way n scalar callers of the reference would step theirs."""

    def __init__(self, arm_byte, so=0.03, arms=None, init=None):
        self.arm = np.asarray(arm_byte, dtype=np.uint8)
        self.n = len(self.arm)
        self.arms = arms if arms is not None else default_arms(so)
        self._sv = [orc.Solver(a) for a in self.arms]
        self.width = len(self._sv[0].buf)
        assert self.width == 19, ("the checker's solver row", self.width)
        self.buf = np.zeros((self.n, self.width))
        if init is not None:
            self.buf[:, :init.shape[1]] = init

    def solver(self, i):
        sv = self._sv[int(self.arm[i] != 0)]
        sv.buf = self.buf[i]          # this row's object
        return sv

    def reach(self, pos, eul, no_limits=False):
        ok = np.zeros(self.n, dtype=np.uint8)
        st = np.zeros(self.n, dtype=np.uint8)
        itv = np.full((self.n, 2), np.nan)
        for i in range(self.n):
            sv = self.solver(i)
            if no_limits:
                ok[i] = sv.is_reachable_no_limits(pos[i], eul[i])
                if ok[i]:
                    itv[i] = (-np.pi, np.pi)
            else:
                o, itv[i], st[i] = sv.is_reachable(pos[i], eul[i])
                ok[i] = o
        return dict(reachable=ok, state=st, interval=itv)

    def joints(self, theta, previous_joints=None, rows=None):
        j = np.full((self.n, 7), np.nan)
        e = np.full((self.n, 3), np.nan)
        p = np.zeros(self.n, dtype=np.uint8)
        for i in (range(self.n) if rows is None else rows):
            j[i], e[i], p[i] = self.solver(i).get_joints(theta[i], None if previous_joints is None else previous_joints[i])
        return dict(joints=j, elbow=e, projected=p)

    def elbow(self, theta, rows=None):
        e = np.full((self.n, 3), np.nan)
        for i in (range(self.n) if rows is None else rows):
            e[i] = self.solver(i).get_elbow_position(theta[i])
        return e


# ------------------------------------------------------------------------------------------ against the reference's recordings
def _check_symbolic(res, g, prefix, n_expected=None):
    """A batch of the checker (or of its object, row by row) against a recorded set: flags and state codes exact, numbers within
    TOL, fully stretched rows through j2 + j6 (singular_rows), the projected flag against the recorded elbow's length."""
    reach = g[prefix + "reachable"]
    np.testing.assert_array_equal(res["reachable"], reach)
    np.testing.assert_array_equal(res["state"], g[prefix + "state"])
    m = reach.astype(bool)
    assert np.all(np.isnan(res["joints"][~m])), f"{prefix}joints: numbers on {int((~np.isnan(res['joints'][~m])).sum())} unreachable slots"
    assert np.all(np.isnan(res["interval"][~m])), f"{prefix}interval: numbers on {int((~np.isnan(res['interval'][~m])).sum())} unreachable slots"
    sing = singular_rows(g[prefix + "joints"]) & m
    for k in ("interval", "joints", "elbow"):
        mm = m & ~sing if k == "joints" else m
        err = np.max(np.abs(res[k][mm] - g[prefix + k][mm])) if mm.any() else 0.0
        assert err < TOL, f"{prefix}{k}: max err {err}"
    if sing.any():
        a, b = res["joints"][sing], g[prefix + "joints"][sing]
        err = np.max(np.abs(a[:, [0, 1, 3, 4, 5]] - b[:, [0, 1, 3, 4, 5]]))
        assert err < TOL, f"{prefix}joints (singular rows): max err {err}"
        dsum = (a[:, 2] + a[:, 6]) - (b[:, 2] + b[:, 6])  # defined modulo 2 pi only (elbow yaw is not wrapped, Q3)
        err = np.max(np.abs(dsum - 2 * np.pi * np.round(dsum / (2 * np.pi))))
        assert err < TOL, f"{prefix}joints (singular rows): j2 + j6 err {err}"
    # Q2: reference returns a 3-vector elbow exactly when the projection branch fired
    np.testing.assert_array_equal(res["projected"][m], (g[prefix + "elbow_len"][m] == 3).astype(np.uint8))


def _check_scale_set(g, pre, res, n, joints_key="joints", tol=1e-9):
    """A G14 set against results over the same n inputs: flags and state codes by SHA-256 (and by per-state counts, which say
    where a difference lies), every 64th row's numbers to `tol`."""
    assert len(res["reachable"]) == n == int(g[pre + "n"]), (pre, len(res["reachable"]), n, int(g[pre + "n"]))
    counts = np.bincount(res["state"], minlength=9)
    assert counts.tolist() == g[pre + "state_counts"].tolist(), (pre, counts.tolist(), g[pre + "state_counts"].tolist())
    assert SC.sha256(res["reachable"]) == str(g[pre + "reachable_sha256"]), pre + "reachable"
    assert SC.sha256(res["state"]) == str(g[pre + "state_sha256"]), pre + "state"
    sub = slice(None, None, SC.SUBSAMPLE)
    np.testing.assert_array_equal(res["reachable"][sub], g[pre + "sub_reachable"])
    np.testing.assert_array_equal(res["state"][sub], g[pre + "sub_state"])
    worst = 0.0
    for key in ("interval", joints_key):
        if pre + "sub_" + key not in g.files:
            continue
        want, got = g[pre + "sub_" + key], res[key][sub]
        m = ~np.isnan(want).any(axis=1)
        if key == "interval":
            assert np.array_equal(m, g[pre + "sub_reachable"].astype(bool)), (pre, "recorded intervals and flags disagree")
        # the fully stretched arm's elbow-yaw / wrist-yaw split is atan2 of two 1e-17 numbers in the reference itself (Q23): j2 + j6
        ok = m & ~(np.abs(want[:, 3]) < 1e-12) if key == joints_key else m
        worst = max(worst, float(np.max(np.abs(got[ok] - want[ok]))))
    assert worst < tol, (pre, worst)
    return worst


def _check_scale_continuous(g, res, theta, latched, joints_tol=1e-7):
    """G16 against a walk of the same trajectories: `res` = joints [n_steps, n_traj, 7], reachable, state [n_steps, n_traj]; `theta` = the
    carried previous_theta at the end [n_traj], `latched` = the emergency stop at the end [n_traj]."""
    counts = np.bincount(res["state"].ravel(), minlength=11)
    assert counts.tolist() == g["state_counts"].tolist(), (counts.tolist(), g["state_counts"].tolist())
    assert SC.sha256(res["reachable"]) == str(g["reachable_sha256"]), "reachable digest"
    assert SC.sha256(res["state"]) == str(g["state_sha256"]), "state digest"
    sub = slice(None, None, SC.SUBSAMPLE_TRAJ)
    np.testing.assert_array_equal(res["state"][:, sub], g["sub_state"])
    err = float(np.max(np.abs(res["joints"][:, sub] - g["sub_joints"])))
    assert err < joints_tol, err
    last = float(np.max(np.abs(res["joints"][-1] - g["last_joints"])))
    assert last < joints_tol, ("last joints", last)
    dth = float(np.max(np.abs(theta - g["last_previous_theta"])))
    assert dth < 1e-9, ("last previous_theta", dth)
    np.testing.assert_array_equal(np.asarray(latched) != 0, g["emergency_stop"] != 0)
    assert int(g["state_counts"][9:].sum()) == 0, ("recorded states above 8", g["state_counts"][9:].tolist())
    return err
