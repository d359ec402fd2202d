"""The shared workload of the control tests on arm pairs (tests/test_control_pairs_checker.py on the CPU,
tests/test_gpu_control_arm_pairs.py on the GPU) and what both need of the CPU checker.  NumPy and the checker only: nothing here
touches the product.  No test in this file.

Rows: G4's goal matrices (dvt_r_arm_M / dvt_l_arm_M: half uniform around the shoulder, half wrist-reachable), 500 matrices, each
once as an r row and once as an l row: 1000 rows, r and l alternating inside every wave.  Per-pair population counts of these rows,
measured on the checker (nb_search_points 64, unconstrained, preferred angle -4 pi / 6; tests/test_control_pairs_checker.py prints
and asserts them): POPULATIONS below.
"""
import ctypes as C
import os

import numpy as np

from oracle import oracle as orc

N = 1000                       # three full 256-row workgroups, a ragged fourth with a ragged last wave
STATES = (0, 1, 2, 3, 4, 6)    # what rsik_control_discrete can return for a goal of numbers
NBS = (10, 64, 100)            # 100 needs a second cooperative round of the wave
PREFERRED = (-4 * np.pi / 6, 2.9)   # the left arm's mirror image of 2.9 leaves [-pi, pi]: the pref_free path
HINGE = 1e-9                   # a decision that rests on a margin below this may fall either way on the device
HINGE_SHARE = 0.005
PTS = (-4 * np.pi / 6, -np.pi + 4 * np.pi / 6)   # ControlIK.preferred_theta of r, l (control_ik.py:133-139)
DEFAULT_SOL = np.array([[0.0, 0.2617993877991494, -0.17453292519943295, 0.0, 0.0, 0.0, 0.0],
                        [0.0, -0.2617993877991494, 0.17453292519943295, 0.0, 0.0, 0.0, 0.0]])
N_TRAJ, N_STEPS = 96, 25       # the size of test_control_continuous_against_checker_dvt_and_emergency

# pair -> per arm (r, l): occurrences of the states 0, 1, 2, 3, 4, 6; rows whose search found a theta / failed after the shortcut
# failed.  Measured on the checker by tests/test_control_pairs_checker.py::test_discrete_inputs (pytest -s prints them).
POPULATIONS = {
    "default/custom": (([80, 135, 125, 36, 38, 86], 48, 86), ([68, 110, 133, 33, 64, 92], 43, 92)),
    "ztip/default": (([70, 134, 135, 35, 41, 85], 44, 85), ([89, 120, 124, 26, 54, 87], 51, 87)),
    "custom/custom": (([64, 126, 135, 29, 63, 83], 42, 83), ([68, 110, 133, 33, 64, 92], 43, 92)),
    "default@-1.01/ztip@-1.01": (([96, 135, 125, 36, 38, 70], 63, 70), ([92, 119, 134, 28, 62, 65], 61, 65)),
    "default@-1.01/default@0.03": (([96, 135, 125, 36, 38, 70], 63, 70), ([89, 120, 124, 26, 54, 87], 51, 87)),
    "default@s*-1e-3/default@s*-1e-3": (([96, 135, 125, 36, 38, 70], 63, 70), ([108, 120, 124, 26, 54, 68], 69, 68)),
    "default@s*+1e-3/default@s*+1e-3": (([96, 135, 125, 36, 38, 70], 63, 70), ([108, 120, 124, 26, 54, 68], 69, 68)),
    "default@s3/default@s3": (([93, 135, 125, 36, 38, 73], 60, 73), ([106, 120, 124, 26, 54, 70], 67, 70)),
}


def control_rows(golden_dir):
    """M [1000, 4, 4], arm [1000] uint8: rows 2 i and 2 i + 1 hold the same matrix for r and for l."""
    g = np.load(os.path.join(golden_dir, "g4_control_discrete.npz"))
    r, l = g["dvt_r_arm_M"], g["dvt_l_arm_M"]
    half = len(r) // 2   # the first half of each set is uniform, the second wrist-reachable
    M = np.concatenate([r[:125], r[half:half + 125], l[:125], l[half:half + 125]])
    order = np.random.default_rng(4).permutation(len(M))
    M = np.repeat(M[order], 2, axis=0)
    arm = (np.arange(N) % 2).astype(np.uint8)
    assert M.shape == (N, 4, 4)
    return np.ascontiguousarray(M), arm


def checker_discrete(arms, M, arm, nb, mode, pref, rows=None, nthreads=4):
    """orc.control_discrete_batch with the pair's two arms; rows = (previous_sol rows [n, 7], bucket [n], vectors [buckets, 7]) for a
    previous_sol per row drawn from a few vectors: bucket by bucket, since the checker takes one vector per call."""
    kw = dict(nb_search_points=nb, constrained_mode=mode, preferred_theta=pref, nthreads=nthreads)
    if rows is None:
        return orc.control_discrete_batch(arms[0], arms[1], M, arm_id=arm, **kw)
    _, bucket, vecs = rows
    out = None
    for b in range(len(vecs)):
        idx = np.flatnonzero(bucket == b)
        r = orc.control_discrete_batch(arms[0], arms[1], M[idx], arm_id=arm[idx], previous_sol=np.stack([vecs[b], vecs[b]]), **kw)
        out = out or {k: np.empty((len(M),) + v.shape[1:], v.dtype) for k, v in r.items()}
        for k in out:
            out[k][idx] = r[k]
    return out


def search_rows(arms, M, arm, nb, pref):
    """utils.get_best_discrete_theta (utils.py:334-396) replayed per row on the checker's own is_reachable and get_elbow_position,
    point by point: reach [n] (is_reachable), shortcut [n] (the preferred theta is valid and its elbow ok), found [n] (the grid search
    found a theta; only where it ran), grid [n] the grid points evaluated, plane_fail [n] those where the singularity-plane half of
    is_elbow_ok fails, margin [n] the smallest |residual| of either half of is_elbow_ok over the points evaluated and the gap between
    the best and the second-best distance to the preferred theta among the ok grid points (inf where nothing was evaluated).
    Neither the constrained mode nor previous_sol enters: the search sees the pose's own interval and the preferred theta as the arm's
    side mirrors it, the same in both modes (control_ik.py:225-252); the mode's interval and previous_sol act on the theta it returns."""
    L = orc.lib()
    n = len(M)
    pos = np.ascontiguousarray(M[:, :3, 3])
    eul = orc.euler_from_matrix_xyz(M)
    out = dict(reach=np.zeros(n, bool), shortcut=np.zeros(n, bool), found=np.zeros(n, bool), grid=np.zeros(n, int),
               plane_fail=np.zeros(n, int), margin=np.full(n, np.inf))
    e = np.zeros(3)
    ep = e.ctypes.data_as(C.POINTER(C.c_double))
    consts = []
    for a in arms:
        es = a.field("elbow_singularity_position")
        consts.append((a.field("side"), a.field("singularity_limit_coeff"), a.field("singularity_offset"), es,
                       float(orc.interval_limit(a, 0, pref)[2])))
    for i in range(n):
        a = arms[int(arm[i])]
        side, coeff, so, es, p = consts[int(arm[i])]
        sv = orc.Solver(a)
        ok, itv, _ = sv.is_reachable(pos[i], eul[i])
        if not ok:
            continue
        out["reach"][i] = True
        svp = sv.buf.ctypes.data_as(C.POINTER(C.c_double))

        def residuals(theta):
            L.orc_get_elbow_position(svp, float(theta), ep)
            return e[1] * side + 0.2, e[2] - ((e[0] - es[0]) * coeff + es[2] - so)   # both below 0: the elbow is ok

        margin = np.inf
        if L.orc_is_valid_angle(p, itv.ctypes.data_as(C.POINTER(C.c_double))):
            ry, rp = residuals(p)
            margin = min(abs(ry), abs(rp))
            if ry < 0 and rp < 0:
                out["shortcut"][i], out["margin"][i] = True, margin
                continue
        if abs(abs(itv[0]) + abs(itv[1]) - 2 * np.pi) < 0.00001:
            lo, hi = np.pi / 2, np.pi / 2 + 2 * np.pi
        elif itv[0] < itv[1]:
            lo, hi = itv[0], itv[1]
        else:
            lo, hi = itv[0], itv[1] + 2 * np.pi
        thetas = np.linspace(lo, hi, nb)
        dist = []
        for t in thetas:
            ry, rp = residuals(t)
            margin = min(margin, abs(ry), abs(rp))
            out["plane_fail"][i] += rp >= 0
            if ry < 0 and rp < 0:
                dist.append(abs(L.orc_angle_diff(float(t), p)))
        out["grid"][i] = nb
        out["found"][i] = len(dist) > 0
        if len(dist) > 1:
            d = np.sort(dist)
            margin = min(margin, d[1] - d[0])
        out["margin"][i] = margin
    return out


# ------------------------------------------------------------------------------------------ trajectories
def jumpy_goals(rng, arm, ntraj, nsteps):
    """The jumpy goal sequences of test_control_continuous_against_checker_dvt_and_emergency: Ms [ntraj, nsteps, 4, 4] random walks
    of a pose in front of the trajectory's own shoulder, every fourth trajectory jumping at step 12 (the continuity check latches the
    emergency stop).  arm: "r_arm" / "l_arm", or an arm byte per trajectory."""
    from scipy.spatial.transform import Rotation as R

    if isinstance(arm, str):
        ys = np.full(ntraj, -0.2 if arm == "r_arm" else 0.2)
    else:
        ys = np.where(np.asarray(arm) == 0, -0.2, 0.2)
    Ms = np.zeros((ntraj, nsteps, 4, 4))
    for k in range(ntraj):
        base = np.array([0.35, ys[k], -0.25])
        p = base + rng.uniform(-0.15, 0.15, 3)
        e = np.array([0.0, -np.pi / 2, 0.0]) + rng.uniform(-0.5, 0.5, 3)
        for i in range(nsteps):
            jump = 0.2 if (k % 4 == 0 and i == 12) else 0.004   # a few trajectories jump -> continuity emergency stop
            p = p + rng.uniform(-jump, jump, 3)
            e = e + rng.uniform(-jump, jump, 3)
            Ms[k, i] = np.eye(4)
            Ms[k, i, :3, :3] = R.from_euler("xyz", e).as_matrix()
            Ms[k, i, :3, 3] = p
    return Ms


def trajectories(seed=78):
    """96 x 25 jumpy goals with an arm byte per trajectory (r and l in blocks of four, so both arms hold jumping trajectories), the
    measured joints and the pose each trajectory starts from: Ms [96, 25, 4, 4], arm [96], start_joints [96, 7], start_pose [96, 4, 4].
    Every eighth trajectory is moved 0.45 m away from the body from step 18 on: the unreachable fallback."""
    rng = np.random.default_rng(seed)
    arm = ((np.arange(N_TRAJ) // 4) % 2).astype(np.uint8)
    Ms = jumpy_goals(rng, arm, N_TRAJ, N_STEPS)
    far = np.arange(N_TRAJ) % 8 == 2
    Ms[far, 18:, 0, 3] += 0.45
    start_j = rng.uniform(-0.6, 0.6, size=(N_TRAJ, 7))   # generic start: no tie in the start-up search
    start_pose = Ms[:, 0].copy()
    start_pose[:, :3, 3] += rng.uniform(-0.02, 0.02, size=(N_TRAJ, 3))
    return Ms, arm, start_j, start_pose


def start_state(arm):
    """[11, n] the trajectory state as ControlIK.new_continuous_state lays it out: previous_theta (the arm's preferred theta),
    previous_sol (the arms along the body), init = 1, no emergency stop, has_previous_sol = 1."""
    n = len(arm)
    st = np.zeros((11, n))
    st[0] = np.asarray(PTS)[arm]
    st[1:8] = DEFAULT_SOL[arm].T
    st[8] = 1.0
    st[10] = 1.0
    return st


def checker_trajectories(arms, Ms, arm, start_j, start_pose, mode=0, nthreads=8):
    """One orc.control_continuous_step per trajectory-step with that trajectory's arm, threaded over trajectories: joints
    [steps, n, 7], reachable / state [steps, n], theta [steps, n] (the carried theta after the step), latched [steps, n]."""
    from concurrent.futures import ThreadPoolExecutor

    ntraj, nsteps = Ms.shape[:2]
    st0 = start_state(arm)
    out = dict(joints=np.zeros((nsteps, ntraj, 7)), reachable=np.zeros((nsteps, ntraj), np.uint8), state=np.zeros((nsteps, ntraj), np.uint8),
               theta=np.zeros((nsteps, ntraj)), latched=np.zeros((nsteps, ntraj), bool), previous_sol=np.zeros((ntraj, 7)))

    def walk(k):
        a = arms[int(arm[k])]
        cs = orc.ContinuousState(st0[0, k], st0[1:8, k])
        prev = start_pose[k]
        for i in range(nsteps):
            j, ok, code = orc.control_continuous_step(a, cs, Ms[k, i], timed_out=(i == 0), preferred_theta_arg=-4 * np.pi / 6,
                                                      preferred_theta_self=PTS[int(arm[k])], constrained_mode=mode,
                                                      current_joints=(start_j[k] if i == 0 else cs.previous_sol), current_pose=prev)
            out["joints"][i, k], out["reachable"][i, k], out["state"][i, k] = j, ok, code
            out["theta"][i, k], out["latched"][i, k] = cs.previous_theta, cs.emergency_stop
            prev = Ms[k, i]
        out["previous_sol"][k] = cs.previous_sol

    with ThreadPoolExecutor(nthreads) as ex:
        list(ex.map(walk, range(ntraj)))
    return out


# ------------------------------------------------------------------------------------------ rows at the plane's threshold
N_CAP = 1 << 17


def cap_rows(seed=79, n=N_CAP):
    """Goals of the default arms on which the singularity plane of offset s* + 1e-3 (arm_pairs.threshold_offset) still decides: it
    cuts only the few centimetres of the upper-arm sphere that are highest along (-1, 0, 1), up and behind the shoulder, and on the 1000
    G4 rows it decides nothing.  Of 400 000 goals uniform in +-0.7 m around the shoulder the checker answered four differently with
    and without that plane, all near (0.04, -0.2, 0.18): the r rows are uniform in a box around that point with a uniform
    orientation, the l row is the mirror image of the r row.  M [n, 4, 4], arm [n] uint8, r and l alternating."""
    from scipy.spatial.transform import Rotation as R

    rng = np.random.default_rng(seed)
    m = n // 2
    Mr = np.tile(np.eye(4), (m, 1, 1))
    Mr[:, :3, :3] = R.from_euler("xyz", rng.uniform(-np.pi, np.pi, size=(m, 3))).as_matrix()
    Mr[:, :3, 3] = np.array([0.04, -0.2, 0.18]) + rng.uniform(-1.0, 1.0, size=(m, 3)) * np.array([0.04, 0.2, 0.12])
    S = np.diag([1.0, -1.0, 1.0, 1.0])
    M = np.empty((n, 4, 4))
    M[0::2] = Mr
    M[1::2] = S @ Mr @ S
    return M, (np.arange(n) % 2).astype(np.uint8)
