"""GPU tests of finite inputs far outside the ranges the device math was written for (tests/far_inputs.py): Euler angles, elbow
angles and previous joints wound up to DBL_MAX, positions up to DBL_MAX and down to the smallest denormal.  include/rsik.h
promises an answer for every row, and the reference answers all of these (libm reduces any finite angle exactly).

The reference is the CPU checker with each row's own arm, pinned to the reference itself by G22 (tests/test_oracle_golden.py)
and shown free of libm's argument reduction and of decision margins by tests/test_far_inputs_checker.py.  Flags, states and the
projected bit are exact, joints / interval / elbow within TOL, on every row.  Legs: A the wound angles against the checker, B the
same rows against their reduced twins through the kernel itself, C far and tiny positions, D far theta_in / state theta /
preferred theta / previous joints, E isolation: ordinary rows next to far ones keep their bits."""
import numpy as np
import pytest

import far_inputs as F
import theta_workload as W
from arm_pairs import checker_arms, upload
from checker_support import CheckerRows
from compare import CONT_JOINT_TOL, CONT_THETA_TOL, TOL
from gpu_support import (_bits_equal, _rows_except, abi, check_against_checker, make_control, make_symbolic, orc, soa, to_np,  # noqa: F401
                         torch_mod)
from nearest_workload import GAP, nearest_from_sweep, seeds
from path_workload import path_dp
from rotations import euler_to_matrix, m12_soa_to_matrices
from sweep_workload import expected_tiled

pytestmark = pytest.mark.gpu

# the default pair launches FORM 2 / TIPZ (goal_from_euler_tipz), "default/custom" FORM 1 and the general goal path (rot_from_euler)
PAIRS = ("default", "default/custom")
KS = (1, 8)


def _setup(pair, orc):
    """(HipSolver with the pair uploaded, the checker's two arms)."""
    if pair == "default":
        solver, r, l = make_symbolic(F.SINGULARITY_OFFSET)
        r._upload()
        l._upload()
        return solver, (orc.Arm("r_arm", F.SINGULARITY_OFFSET), orc.Arm("l_arm", F.SINGULARITY_OFFSET))
    return upload(pair), checker_arms(pair)


def _T(a, torch, dtype=np.float64):
    return torch.as_tensor(np.array(a, dtype=dtype, order="C")).cuda()  # (a copy: the workload's arrays are read-only)


def _close(got, want, what, tol=TOL):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN pattern", np.flatnonzero(np.isnan(got) != np.isnan(want))[:10])
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
    worst = float(np.nanmax(err, initial=0.0))
    print(f"{what}: max |diff| {worst:.3e}")
    assert worst <= tol, (what, worst, np.argwhere(err > tol)[:10].tolist())


def _same_reach(got, ref, what):
    for k in ("reachable", "state"):
        np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(ref[k]), err_msg=f"{what} {k}")
    _close(got["interval"], ref["interval"], what + " interval")


def _check_solve(got, ref, what, per_rung=None):
    if per_rung is not None:
        rung, names = per_rung
        for g in range(len(names)):
            m = rung == g
            for k in ("reachable", "state"):
                np.testing.assert_array_equal(np.asarray(got[k])[m], np.asarray(ref[k])[m], err_msg=f"{what} {k}, rung {names[g]!r}")
    _same_reach(got, ref, what)
    if "joints" in got:
        if per_rung is not None:  # (the first rung that differs names itself)
            rung, names = per_rung
            for g in range(len(names)):
                m = rung == g
                _close(got["joints"][m], ref["joints"][m], f"{what} joints, rung {names[g]!r}")
        _close(got["joints"], ref["joints"], what + " joints")
    if "elbow" in got:
        _close(got["elbow"], ref["elbow"], what + " elbow")


def _only_near_ties(arms, differ, pos, eul, arm, cur, pref, what, at_most):
    """Rows on which two runs of the ternary search (utils.py:302-323) ended in different thetas: few, and on each of them the
    checker's replay of the search holds a comparison whose sides are closer than W.NEAR_TIE — the only way it can fall otherwise."""
    rows = [int(i) for i in np.flatnonzero(differ)]
    assert len(rows) <= at_most, (what, rows[:10])
    ties = W.near_ties(arms, pos, eul, arm, cur, pref=pref, rows=rows)
    assert sorted(ties) == rows, (what, "theta differs on a row without a near tie", sorted(set(rows) - set(ties)))


def _ordinary_thetas(n, seed):
    return np.random.default_rng(seed).uniform(-np.pi, np.pi, size=n)


# ------------------------------------------------------------------------------------------ A / B: wound Euler angles
@pytest.mark.parametrize("pair", PAIRS)
def test_wound_angles_solve(torch_mod, orc, pair):
    """rsik_solve (mixed arms, every theta policy's output set), rsik_solve_rows, rsik_reach_state + rsik_joints_from_state: the
    wound rows against the checker (A) and, through the kernel itself, against their reduced twins (B)."""
    torch, A = torch_mod, abi()
    solver, arms = _setup(pair, orc)
    w = F.wound_rows()
    pos, eul, twin, arm = w["pos"], w["eul"], w["twin_eul"], w["arm"]
    n = len(pos)
    armT = _T(arm, torch, np.uint8)
    th = _ordinary_thetas(n, 1)
    u = np.random.default_rng(2).uniform(0.0, 1.0, size=n)
    prev = np.random.default_rng(3).uniform(-3.0, 3.0, size=(n, 7))
    names = F.RUNGS
    for what, policy, theta_in in (("interval0", A.THETA_INTERVAL0, None), ("explicit", A.THETA_EXPLICIT, th),
                                   ("fraction", A.THETA_FRACTION, u), ("none", A.THETA_NONE, None)):
        kw = dict(arm=armT, theta_policy=policy, theta_in=None if theta_in is None else _T(theta_in, torch))
        got = to_np(solver.solve(soa(pos, eul, torch), **kw))
        ref = orc.solve_batch(arms[0], arms[1], pos, eul, arm_id=arm, theta_policy=0 if policy == A.THETA_NONE else policy, theta_in=theta_in)
        assert ("joints" in got) == (policy != A.THETA_NONE)
        _check_solve(got, ref, f"{pair} A {what}", per_rung=(w["rung"], names))
        tw = to_np(solver.solve(soa(pos, twin, torch), **kw))
        _check_solve(got, tw, f"{pair} B {what}", per_rung=(w["rung"], names))
    # rsik_solve_rows: one previous-joints row per pose
    kw = dict(arm=armT, theta_policy=A.THETA_EXPLICIT, theta_in=_T(th, torch), previous_joints_rows=_T(prev, torch))
    got = to_np(solver.solve(soa(pos, eul, torch), **kw))
    ref = orc.solve_batch(arms[0], arms[1], pos, eul, arm_id=arm, theta_policy=1, theta_in=th)  # (no row is exactly singular: prev is not read)
    _check_solve(got, ref, f"{pair} A rows")
    _check_solve(got, to_np(solver.solve(soa(pos, twin, torch), **kw)), f"{pair} B rows")
    # the solver-state pair of calls: the state row keeps the angles as they came
    ok = ref["reachable"].astype(bool)
    out = {}
    for tag, e in (("wound", eul), ("twin", twin)):
        st = solver.new_solver_state(n)
        rs = to_np(solver.reach_state(soa(pos, e, torch), st, arm=armT))
        js = to_np(solver.joints_from_state(st, _T(th, torch), arm=armT, previous_joints=_T(prev, torch)))
        out[tag] = (rs, js, st.cpu().numpy())
    rs, js, S = out["wound"]
    _same_reach(rs, ref, f"{pair} A reach_state")
    np.testing.assert_array_equal(S[ok][:, 3:6], eul[ok])
    _close(js["joints"][ok], ref["joints"][ok], f"{pair} A joints_from_state joints")
    _close(js["elbow"][ok], ref["elbow"][ok], f"{pair} A joints_from_state elbow")
    _same_reach(rs, out["twin"][0], f"{pair} B reach_state")
    _close(js["joints"][ok], out["twin"][1]["joints"][ok], f"{pair} B joints_from_state joints")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("pair", PAIRS)
def test_wound_angles_sampling(torch_mod, orc, pair, k):
    """rsik_solve_sweep, rsik_solve_nearest and rsik_solve_path at K = 1 and 8 on the wound rows: against the checker's tiled sweep
    (and NumPy's argmin / dynamic programme over it), and against the twins through the kernels."""
    torch = torch_mod
    solver, arms = _setup(pair, orc)
    w = F.wound_rows()
    pos, eul, twin, arm = w["pos"], w["eul"], w["twin_eul"], w["arm"]
    n = len(pos)
    armT = _T(arm, torch, np.uint8)
    frac = np.linspace(0.0, 1.0, k) if k > 1 else np.array([0.5])
    exp = expected_tiled(orc, arms, pos, eul, arm, "fraction", frac)
    got = to_np(solver.solve_sweep(soa(pos, eul, torch), _T(frac, torch), policy="fraction", arm=armT))
    tw = to_np(solver.solve_sweep(soa(pos, twin, torch), _T(frac, torch), policy="fraction", arm=armT))
    for what, ref in ((f"{pair} A sweep K={k}", exp), (f"{pair} B sweep K={k}", tw)):
        _same_reach(got, ref, what)
        np.testing.assert_array_equal(got["projected"], ref["projected"], err_msg=what)
        for key in ("joints", "elbow", "theta"):
            _close(got[key], ref[key], f"{what} {key}")
    # nearest: the winner NumPy picks from the checker's sweep, wherever its lead is clear
    seed = seeds(n, 77)
    want = nearest_from_sweep(exp, seed)
    clear = want["gap"] > GAP
    assert clear[exp["reachable"] != 0].mean() > 0.95 or k == 1
    kw = dict(policy="fraction", arm=armT)
    near = to_np(solver.solve_nearest(soa(pos, eul, torch), _T(frac, torch), _T(seed, torch), **kw))
    near_tw = to_np(solver.solve_nearest(soa(pos, twin, torch), _T(frac, torch), _T(seed, torch), **kw))
    _same_reach(near, exp, f"{pair} A nearest K={k}")
    np.testing.assert_array_equal(near["index"][clear], want["index"][clear])
    m = np.flatnonzero(clear & (want["index"] >= 0))
    _close(near["joints"][m], exp["joints"][want["index"][m], m], f"{pair} A nearest K={k} joints")
    assert np.isnan(near["joints"][want["index"] < 0]).all()
    _same_reach(near, near_tw, f"{pair} B nearest K={k}")
    np.testing.assert_array_equal(near["index"][clear], near_tw["index"][clear])
    _close(near["joints"][clear], near_tw["joints"][clear], f"{pair} B nearest K={k} joints")
    # path: two waypoints per path, the rows of one arm paired up (row i and row i + n/2 keep their arm: r and l alternate)
    t, half = 2, n // 2
    start = seeds(half, 78)
    p_soa = torch.stack([soa(pos, eul, torch).reshape(6, t, half), soa(pos, twin, torch).reshape(6, t, half)])
    arm_p = arm[:half]
    assert np.array_equal(arm[:half], arm[half:])
    want = path_dp(exp, t, half, start=start)
    kw = dict(start_joints=_T(start, torch), policy="fraction", arm=_T(arm_p, torch, np.uint8))
    path = to_np(solver.solve_path(p_soa[0].contiguous(), _T(frac, torch), **kw))
    path_tw = to_np(solver.solve_path(p_soa[1].contiguous(), _T(frac, torch), **kw))
    for key in ("reachable", "state"):
        np.testing.assert_array_equal(path[key].reshape(-1), exp[key], err_msg=f"{pair} A path {key}")
        np.testing.assert_array_equal(path[key], path_tw[key], err_msg=f"{pair} B path {key}")
    clear = want["gap"] > GAP
    np.testing.assert_array_equal(path["index"][:, clear], want["index"][:, clear])
    np.testing.assert_array_equal(path["index"][:, clear], path_tw["index"][:, clear])
    J = exp["joints"].reshape(k, t, half, 7)
    for q in range(t):
        m = np.flatnonzero(clear & (want["index"][q] >= 0))
        _close(path["joints"][q, m], J[want["index"][q, m], q, m], f"{pair} A path K={k} joints, waypoint {q}")
    _close(path["joints"][:, clear], path_tw["joints"][:, clear], f"{pair} B path K={k} joints")


@pytest.mark.parametrize("pair", PAIRS)
def test_wound_angles_theta_from_joints_and_stages(torch_mod, orc, pair):
    """rsik_theta_from_joints with a pose goal, RSIK_STAGE_WRIST_POSITION and RSIK_STAGE_POSE_IN_REACH on the wound rows."""
    torch, A = torch_mod, abi()
    solver, arms = _setup(pair, orc)
    w = F.wound_rows()
    pos, eul, twin, arm = w["pos"], w["eul"], w["twin_eul"], w["arm"]
    n = len(pos)
    cur = np.random.default_rng(5).uniform(-1.5, 1.5, size=(n, 7))
    armT = _T(arm, torch, np.uint8)
    ref = W.checker_batch(None, pos, eul, arm, cur, arms=arms)
    got = to_np(solver.theta_from_joints(soa(pos, eul, torch), _T(cur, torch), W.PREFERRED, arm=armT))
    check_against_checker(got, ref, None, pos, eul, arm, cur, f"{pair} A theta_from_joints", arms=arms)
    tw = to_np(solver.theta_from_joints(soa(pos, twin, torch), _T(cur, torch), W.PREFERRED, arm=armT))
    np.testing.assert_array_equal(got["state"], tw["state"])
    same = np.abs(got["theta"] - tw["theta"]) <= 1e-12
    _only_near_ties(arms, ~same, pos, twin, arm, cur, W.PREFERRED, f"{pair} B theta_from_joints", n // 1000)
    _close(got["joints"][same], tw["joints"][same], f"{pair} B theta_from_joints joints")
    # the stages take one arm per launch
    for a in (0, 1):
        rows = np.flatnonzero(arm == a)
        pose, pose_tw = np.concatenate([pos[rows], eul[rows]], axis=1), np.concatenate([pos[rows], twin[rows]], axis=1)
        tip = arms[a].field("tip_position") * np.array([-1.0, 1.0, 1.0])       # S:418-425
        want = pos[rows] + np.einsum("nij,j->ni", euler_to_matrix(twin[rows]), tip)
        wr = solver.stage(A.STAGE_WRIST_POSITION, _T(pose, torch), a).cpu().numpy()
        _close(wr, want, f"{pair} A wrist stage, arm {a}")
        _close(wr, solver.stage(A.STAGE_WRIST_POSITION, _T(pose_tw, torch), a).cpu().numpy(), f"{pair} B wrist stage, arm {a}")
        o = solver.stage(A.STAGE_POSE_IN_REACH, _T(pose, torch), a).cpu().numpy()
        assert (o[:, 0] == 1.0).all() and (o[:, 4] == 7.0).all()  # the angles play no part: every base position is in reach
        np.testing.assert_array_equal(o[:, 1:4], pos[rows])


# ------------------------------------------------------------------------------------------ C: far and tiny positions
def _pose_in_reach(arm_c, pos):
    """S:284-307 in NumPy: (in reach, position, state code) — the norm overflows to inf as the reference's does."""
    s, L, pm, bl = (arm_c.field(k) for k in ("shoulder_position", "max_arm_length", "projection_margin", "backward_limit"))
    gp = pos.copy()
    st = np.full(len(pos), 7)
    with np.errstate(over="ignore", invalid="ignore"):
        dv = pos - s
        d = np.sqrt(dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1] + dv[:, 2] * dv[:, 2])
        far = d > L
        gp[far] = (s + dv / (d + pm)[:, None] * L)[far]
    st[far] = 1
    back = gp[:, 0] < bl
    gp[back, 0] = bl
    st[back] = 2
    return (st == 7).astype(np.float64), gp, st


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("rows", ["far", "tiny"])
def test_far_and_tiny_positions_solve(torch_mod, orc, pair, rows):
    """The entry points of leg A on positions up to DBL_MAX (the squared distance overflows from 1.34e154 on: the reference's
    norm is inf, its direction 0, the goal the shoulder itself) and down to the smallest denormal."""
    torch, A = torch_mod, abi()
    solver, arms = _setup(pair, orc)
    pos, eul, arm, val, entry = F.far_position_rows() if rows == "far" else F.tiny_position_rows()
    n = len(pos)
    armT = _T(arm, torch, np.uint8)
    th = _ordinary_thetas(n, 11)
    for what, policy, theta_in in (("interval0", A.THETA_INTERVAL0, None), ("explicit", A.THETA_EXPLICIT, th), ("none", A.THETA_NONE, None)):
        got = to_np(solver.solve(soa(pos, eul, torch), arm=armT, theta_policy=policy, theta_in=None if theta_in is None else _T(theta_in, torch)))
        ref = orc.solve_batch(arms[0], arms[1], pos, eul, arm_id=arm, theta_policy=0 if policy == A.THETA_NONE else policy, theta_in=theta_in)
        _check_solve(got, ref, f"{pair} C {rows} {what}", per_rung=(np.searchsorted(np.unique(np.abs(val)), np.abs(val)), np.unique(np.abs(val))))
    ref = orc.solve_batch(arms[0], arms[1], pos, eul, arm_id=arm, theta_policy=1, theta_in=th)
    if rows == "far":
        assert not ref["reachable"].any() and set(ref["state"]) <= {1, 2}
        if pair == "default":
            assert (ref["state"][np.abs(val) >= 2e154] == 2).all()
    got = to_np(solver.solve(soa(pos, eul, torch), arm=armT, theta_policy=A.THETA_EXPLICIT, theta_in=_T(th, torch),
                             previous_joints_rows=_T(np.zeros((n, 7)), torch)))
    _check_solve(got, ref, f"{pair} C {rows} rows")
    st = solver.new_solver_state(n)
    _same_reach(to_np(solver.reach_state(soa(pos, eul, torch), st, arm=armT)), ref, f"{pair} C {rows} reach_state")
    ok = ref["reachable"].astype(bool)
    js = to_np(solver.joints_from_state(st, _T(th, torch), arm=armT))
    _close(js["joints"][ok], ref["joints"][ok], f"{pair} C {rows} joints_from_state")
    for k in KS:
        frac = np.linspace(0.0, 1.0, k) if k > 1 else np.array([0.5])
        exp = expected_tiled(orc, arms, pos, eul, arm, "fraction", frac)
        got = to_np(solver.solve_sweep(soa(pos, eul, torch), _T(frac, torch), policy="fraction", arm=armT))
        _same_reach(got, exp, f"{pair} C {rows} sweep K={k}")
        np.testing.assert_array_equal(got["projected"], exp["projected"])
        _close(got["joints"], exp["joints"], f"{pair} C {rows} sweep K={k} joints")
        seed = seeds(n, 79)
        want = nearest_from_sweep(exp, seed)
        near = to_np(solver.solve_nearest(soa(pos, eul, torch), _T(frac, torch), _T(seed, torch), policy="fraction", arm=armT))
        _same_reach(near, exp, f"{pair} C {rows} nearest K={k}")
        clear = want["gap"] > GAP
        np.testing.assert_array_equal(near["index"][clear], want["index"][clear])
        path = to_np(solver.solve_path(soa(pos, eul, torch).reshape(6, 1, n), _T(frac, torch), policy="fraction", arm=armT))
        np.testing.assert_array_equal(path["state"][0], exp["state"])
        np.testing.assert_array_equal(path["reachable"][0], exp["reachable"])
        assert (path["index"][0][exp["reachable"] == 0] == -1).all()
    for a in (0, 1):
        m = np.flatnonzero(arm == a)
        pose = np.concatenate([pos[m], eul[m]], axis=1)
        o = solver.stage(A.STAGE_POSE_IN_REACH, _T(pose, torch), a).cpu().numpy()
        ok_, gp, code = _pose_in_reach(arms[a], pos[m])
        np.testing.assert_array_equal(o[:, 0], ok_)
        np.testing.assert_array_equal(o[:, 4], code)
        _close(o[:, 1:4], gp, f"{pair} C {rows} pose-in-reach stage, arm {a}")
        tip = arms[a].field("tip_position") * np.array([-1.0, 1.0, 1.0])
        want = pos[m] + np.einsum("nij,j->ni", euler_to_matrix(eul[m]), tip)
        wr = solver.stage(A.STAGE_WRIST_POSITION, _T(pose, torch), a).cpu().numpy()
        scale = np.maximum(1.0, np.abs(want))  # (a far position: the wrist is the position to rounding, one ulp of ITS size)
        _close(wr / scale, want / scale, f"{pair} C {rows} wrist stage, arm {a}")
    cur = np.random.default_rng(6).uniform(-1.5, 1.5, size=(n, 7))
    ref = W.checker_batch(None, pos, eul, arm, cur, arms=arms)
    got = to_np(solver.theta_from_joints(soa(pos, eul, torch), _T(cur, torch), W.PREFERRED, arm=armT))
    np.testing.assert_array_equal(got["state"] == 0, ref["ok"])
    okr = ref["ok"] & ~ref["moved"]
    same = np.abs(got["theta"] - ref["theta"]) <= 1e-12
    _only_near_ties(arms, ref["ok"] & ~same, pos, eul, arm, cur, W.PREFERRED, f"{pair} C {rows} theta_from_joints", max(1, n // 1000))
    _close(got["joints"][okr & same], ref["joints"][okr & same], f"{pair} C {rows} theta_from_joints joints")


@pytest.mark.parametrize("rows", ["far", "tiny"])
def test_far_and_tiny_translations_control(torch_mod, orc, rows):
    """The same positions as the translation column of proper goal matrices: rsik_control_discrete, rsik_control_discrete_rows and
    one rsik_control_continuous_step, both arms in one launch, against the checker; and every ordinary row of a launch that holds
    far rows keeps the bits of the launch in which those rows held ordinary goals (E)."""
    torch = torch_mod
    pos, eul, arm, val, entry = F.far_position_rows() if rows == "far" else F.tiny_position_rows()
    n = len(pos)
    M = F.goal_matrices(pos, eul)
    base = {a: F.base_poses(name) for a, name in enumerate(("r_arm", "l_arm"))}
    pos0 = np.array([base[int(a)][0][i % 4] for i, a in enumerate(arm)])
    # every third row stays ordinary
    far_rows = np.flatnonzero(np.arange(n) % 3 != 0)
    mixed = F.goal_matrices(pos0, eul)
    mixed[far_rows] = M[far_rows]
    clean = F.goal_matrices(pos0, eul)
    c = make_control()
    armT = _T(arm, torch, np.uint8)
    ar, al = orc.Arm("r_arm", -1.01), orc.Arm("l_arm", -1.01)
    keep = _rows_except(torch, n, far_rows)
    ps = np.array([c.previous_sol["r_arm"], c.previous_sol["l_arm"]], dtype=np.float64)
    for what, kw in (("discrete", {}), ("discrete_rows", dict(previous_sol=ps[arm]))):
        got = c.symbolic_inverse_kinematics_batch(armT, mixed, **kw)
        got = {k: v.clone() for k, v in got.items()}
        base_run = c.symbolic_inverse_kinematics_batch(armT, clean, **kw)
        torch.cuda.synchronize()
        for k in got:
            assert _bits_equal(torch, got[k][keep], base_run[k][keep]), (what, k)
        ref = orc.control_discrete_batch(ar, al, mixed, arm_id=arm, nb_search_points=int(c.nb_search_points))
        g = to_np(got)
        np.testing.assert_array_equal(g["reachable"], ref["reachable"], err_msg=what)
        np.testing.assert_array_equal(g["state"], ref["state"], err_msg=what)
        assert not g["emergency"].any()
        _close(g["joints"], ref["joints"], f"C {rows} {what} joints", tol=CONT_JOINT_TOL)
        if rows == "far":
            assert not g["reachable"][far_rows].any() and set(g["state"][far_rows]) <= {1, 2}
    # one continuous step (the first of a trajectory: timed out, re-initialised from the ordinary pose the arm is in)
    c1, c2 = make_control(), make_control()
    st1, st2 = c1.new_continuous_state(armT, n), c2.new_continuous_state(armT, n)
    to = np.ones(n, dtype=np.uint8)
    got = c1.symbolic_inverse_kinematics_continuous_batch(armT, mixed, st1, timed_out=to, current_pose=clean)
    base_run = c2.symbolic_inverse_kinematics_continuous_batch(armT, clean, st2, timed_out=to, current_pose=clean)
    torch.cuda.synchronize()
    for k in got:
        assert _bits_equal(torch, got[k][keep], base_run[k][keep]), ("continuous step", k)
    assert _bits_equal(torch, st1[:, keep], st2[:, keep])
    g, S = to_np(got), st1.cpu().numpy()
    for i in range(n):
        name = ("r_arm", "l_arm")[int(arm[i])]
        cs = orc.ContinuousState(c1.previous_theta[name], c1.previous_sol[name])
        j, ok, code = orc.control_continuous_step((ar, al)[int(arm[i])], cs, mixed[i], timed_out=True, preferred_theta_arg=-4 * np.pi / 6,
                                                  preferred_theta_self=c1.preferred_theta[name], constrained_mode=0,
                                                  current_joints=cs.previous_sol, current_pose=clean[i])
        assert ok == bool(g["reachable"][i]) and code == g["state"][i], (i, code, g["state"][i])
        assert np.array_equal(np.isnan(j), np.isnan(g["joints"][i])) and np.nanmax(np.abs(j - g["joints"][i]), initial=0.0) < CONT_JOINT_TOL, i
        assert abs(cs.previous_theta - S[0, i]) < CONT_THETA_TOL and np.max(np.abs(cs.previous_sol - S[1:8, i])) < CONT_JOINT_TOL, i


def _far_trajectories(torch, traj):
    """The goal matrices of a run [n_steps, 12, n] with far and tiny translations in some trajectories: a single step in the
    middle, the first step, the last step, a stretch, every step from some point on, and the whole trajectory."""
    n_steps, _, n = traj.shape
    t = traj.clone()
    cases = {}
    plan = [(slice(n_steps // 2, n_steps // 2 + 1), 9, 1e300), (slice(0, 1), 10, -2e154), (slice(n_steps - 1, n_steps), 11, F.DBL_MAX),
            (slice(n_steps // 3, n_steps // 3 + 9), 9, -1e154), (slice((2 * n_steps) // 3, n_steps), 10, 1e10), (slice(0, n_steps), 11, 5e-324)]
    picks = sorted(set(np.linspace(0, n - 1, len(plan)).astype(int).tolist()))
    assert len(picks) == len(plan), "one trajectory per placement"
    for col, (steps, row, v) in zip(picks, plan):
        t[steps, row, col] = v
        cases.setdefault(col, []).extend(range(*steps.indices(n_steps)))
    return t, {k: sorted(set(v)) for k, v in cases.items()}


def test_continuous_run_far_translations(torch_mod, orc):
    """rsik_control_continuous_run, the steps form and the pipeline: trajectories with far / tiny translations are answered step by
    step as the checker answers them, and every other trajectory — outputs and carried state — is bit for bit a clean run's."""
    torch = torch_mod
    from bench import make_config5_trajectories

    A = abi()
    n_traj, n_steps = 9, 131
    traj = make_config5_trajectories(n_traj, n_steps, seed=123)
    far, cases = _far_trajectories(torch, traj)
    c = make_control()
    hs = c._solver
    st0 = c.new_continuous_state("r_arm", n_traj)
    keep = _rows_except(torch, n_traj, sorted(cases))
    results = {}
    try:
        for name, mode in (("steps", A.CONT_RUN_STEPS), ("phased", A.CONT_RUN_PHASED)):
            hs.set_option(A.OPT_CONT_RUN_MODE, mode)
            runs = []
            for T in (traj, far):
                st = st0.clone()
                o = c.run_continuous_trajectories("r_arm", T, st, first_step_timed_out=True, current_pose=traj[0])
                hs.synchronize()
                runs.append(({k: v.clone() for k, v in o.items()}, st.clone()))
            (co, cst), (bo, bst) = runs
            for k in co:
                assert _bits_equal(torch, bo[k][:, keep], co[k][:, keep]), (name, k)
            assert _bits_equal(torch, bst[:, keep], cst[:, keep]), (name, "cont_state")
            results[name] = (bo, bst)
    finally:
        hs.set_option(A.OPT_CONT_RUN_MODE, A.CONT_RUN_AUTO)
    (so_, sst), (po, pst) = results["steps"], results["phased"]
    assert _bits_equal(torch, so_["state"], po["state"]) and _bits_equal(torch, so_["reachable"], po["reachable"])
    assert torch.equal(torch.isnan(so_["joints"]), torch.isnan(po["joints"]))
    assert float((torch.nan_to_num(so_["joints"]) - torch.nan_to_num(po["joints"])).abs().max()) <= 1e-9
    a = orc.Arm("r_arm", -1.01)
    cols = sorted(cases)
    Ms = m12_soa_to_matrices(far[:, :, torch.as_tensor(cols).cuda()].cpu().numpy())
    M0 = m12_soa_to_matrices(traj[:1, :, torch.as_tensor(cols).cuda()].cpu().numpy())[0]
    J, Fl, S = (so_[k].cpu().numpy() for k in ("joints", "reachable", "state"))
    for col, k in enumerate(cols):
        cs = orc.ContinuousState(c.previous_theta["r_arm"], c.previous_sol["r_arm"])
        for i in range(n_steps):
            j, ok, code = orc.control_continuous_step(a, cs, Ms[i, col], timed_out=(i == 0), preferred_theta_arg=-4 * np.pi / 6,
                                                      preferred_theta_self=c.preferred_theta["r_arm"], constrained_mode=0,
                                                      current_joints=cs.previous_sol, current_pose=M0[col])
            assert ok == bool(Fl[i, k]) and code == S[i, k], (k, i, code, S[i, k])
            assert np.array_equal(np.isnan(j), np.isnan(J[i, k])) and np.nanmax(np.abs(j - J[i, k]), initial=0.0) < CONT_JOINT_TOL, (k, i)
        assert abs(cs.previous_theta - float(sst[0, k])) < CONT_THETA_TOL
        assert cs.emergency_stop == bool(sst[9, k] != 0)


# ------------------------------------------------------------------------------------------ D: other caller angles
@pytest.mark.parametrize("pair", PAIRS)
def test_far_elbow_angles(torch_mod, orc, pair):
    """theta_in of RSIK_THETA_EXPLICIT, the explicit grids of sweep / nearest / path, the theta of the two state entry points and
    the preferred theta of rsik_theta_from_joints at every rung and sign: against the checker, and against the reduced twin
    through the kernel."""
    torch, A = torch_mod, abi()
    solver, arms = _setup(pair, orc)
    th, tw, rg = F.far_thetas()
    k = len(th)
    reps = 8
    pos = np.concatenate([np.repeat(F.base_poses(name)[0][:reps], k, axis=0) for name in ("r_arm", "l_arm")])
    eul = np.concatenate([np.repeat(F.base_poses(name)[1][:reps], k, axis=0) for name in ("r_arm", "l_arm")])
    arm = np.repeat(np.array([0, 1], dtype=np.uint8), reps * k)
    order = np.random.default_rng(9).permutation(len(pos))   # r and l mixed inside every wave
    pos, eul, arm = pos[order], eul[order], arm[order]
    theta, twin, rung = np.tile(th, 2 * reps)[order], np.tile(tw, 2 * reps)[order], np.tile(rg, 2 * reps)[order]
    n = len(pos)
    armT = _T(arm, torch, np.uint8)
    ref = orc.solve_batch(arms[0], arms[1], pos, eul, arm_id=arm, theta_policy=1, theta_in=theta)
    got = to_np(solver.solve(soa(pos, eul, torch), arm=armT, theta_policy=A.THETA_EXPLICIT, theta_in=_T(theta, torch)))
    _check_solve(got, ref, f"{pair} D theta_in", per_rung=(rung, F.RUNGS))
    got_tw = to_np(solver.solve(soa(pos, eul, torch), arm=armT, theta_policy=A.THETA_EXPLICIT, theta_in=_T(twin, torch)))
    _check_solve(got, got_tw, f"{pair} D theta_in against the twin", per_rung=(rung, F.RUNGS))
    ok = ref["reachable"].astype(bool)
    assert ok.mean() > 0.5
    # the state entry points
    st = solver.new_solver_state(n)
    solver.reach_state(soa(pos, eul, torch), st, arm=armT)
    js = to_np(solver.joints_from_state(st, _T(theta, torch), arm=armT))
    _close(js["joints"][ok], ref["joints"][ok], f"{pair} D joints_from_state")
    _close(js["elbow"][ok], ref["elbow"][ok], f"{pair} D joints_from_state elbow")
    st_tw = solver.new_solver_state(n)
    solver.reach_state(soa(pos, eul, torch), st_tw, arm=armT)
    js_tw = to_np(solver.joints_from_state(st_tw, _T(twin, torch), arm=armT))
    proj = st.cpu().numpy()[:, 19] != 0   # (a projected get_joints moves the circle on the row: the elbow of that row is the moved one)
    el = solver.elbow_from_state(st_tw, _T(theta, torch)).cpu().numpy()
    el_tw = solver.elbow_from_state(st_tw, _T(twin, torch)).cpu().numpy()
    _close(el[ok], el_tw[ok], f"{pair} D elbow_from_state against the twin")
    _close(el[ok & ~proj], ref["elbow"][ok & ~proj], f"{pair} D elbow_from_state")
    _close(js["joints"][ok], js_tw["joints"][ok], f"{pair} D joints_from_state against the twin")
    # the explicit grids: every far angle, as one shared grid
    p8 = np.concatenate([F.base_poses(name)[0] for name in ("r_arm", "l_arm")])
    e8 = np.concatenate([F.base_poses(name)[1] for name in ("r_arm", "l_arm")])
    a8 = np.repeat(np.array([0, 1], dtype=np.uint8), F.N_BASE)
    m = len(p8)
    exp = expected_tiled(orc, arms, p8, e8, a8, "explicit", th)
    a8T = _T(a8, torch, np.uint8)
    sw = to_np(solver.solve_sweep(soa(p8, e8, torch), _T(th, torch), policy="explicit", arm=a8T))
    sw_tw = to_np(solver.solve_sweep(soa(p8, e8, torch), _T(tw, torch), policy="explicit", arm=a8T))
    _same_reach(sw, exp, f"{pair} D sweep")
    np.testing.assert_array_equal(sw["projected"], exp["projected"])
    np.testing.assert_array_equal(sw["projected"], sw_tw["projected"])
    for q in range(k):
        _close(sw["joints"][q], exp["joints"][q], f"{pair} D sweep joints, theta {th[q]!r}")
    _close(sw["joints"], sw_tw["joints"], f"{pair} D sweep joints against the twin")
    _close(sw["elbow"], exp["elbow"], f"{pair} D sweep elbow")
    okm = exp["reachable"] != 0
    np.testing.assert_array_equal(sw["theta"][:, okm], np.repeat(th[:, None], int(okm.sum()), axis=1))  # the angle as it came
    seed = seeds(m, 80)
    want = nearest_from_sweep(exp, seed)
    clear = want["gap"] > GAP
    near = to_np(solver.solve_nearest(soa(p8, e8, torch), _T(th, torch), _T(seed, torch), policy="explicit", arm=a8T))
    np.testing.assert_array_equal(near["index"][clear], want["index"][clear])
    mm = np.flatnonzero(clear & (want["index"] >= 0))
    _close(near["joints"][mm], exp["joints"][want["index"][mm], mm], f"{pair} D nearest joints")
    np.testing.assert_array_equal(near["theta"][mm], th[want["index"][mm]])
    start = seeds(m, 81)
    wantp = path_dp(exp, 1, m, start=start)
    path = to_np(solver.solve_path(soa(p8, e8, torch).reshape(6, 1, m), _T(th, torch), start_joints=_T(start, torch), policy="explicit", arm=a8T))
    clear = wantp["gap"] > GAP
    np.testing.assert_array_equal(path["index"][:, clear], wantp["index"][:, clear])
    mm = np.flatnonzero(clear & (wantp["index"][0] >= 0))
    _close(path["joints"][0, mm], exp["joints"][wantp["index"][0, mm], mm], f"{pair} D path joints")
    # the preferred theta of rsik_theta_from_joints: a launch constant per arm, one launch per rung and sign
    cur = np.random.default_rng(7).uniform(-1.5, 1.5, size=(m, 7))
    for q in range(k):
        pref = (float(th[q]), float(-th[q]))
        pref_tw = (float(tw[q]), float(-tw[q]))
        a_ = to_np(solver.theta_from_joints(soa(p8, e8, torch), _T(cur, torch), pref, arm=a8T))
        b_ = to_np(solver.theta_from_joints(soa(p8, e8, torch), _T(cur, torch), pref_tw, arm=a8T))
        np.testing.assert_array_equal(a_["state"], b_["state"])
        # the search itself never sees the preferred theta: the same bracket; where the shortcut is taken, the theta as it came
        short = np.isnan(b_["bracket"][:, 0])
        np.testing.assert_array_equal(np.isnan(a_["bracket"][:, 0]), short, err_msg=repr(th[q]))
        np.testing.assert_array_equal(a_["theta"][~short], b_["theta"][~short], err_msg=repr(th[q]))
        _close(a_["joints"], b_["joints"], f"{pair} D preferred theta {th[q]!r} joints")
        ref_q = W.checker_batch(None, p8, e8, a8, cur, pref=pref, arms=arms)
        same = np.abs(a_["theta"] - ref_q["theta"]) <= 1e-12
        _only_near_ties(arms, ref_q["ok"] & ~same, p8, e8, a8, cur, pref, f"{pair} D preferred theta {th[q]!r}", 1)


def test_far_previous_joints_at_the_exact_singularity(torch_mod, orc):
    """The construct of test_exact_singularity_reads_its_own_previous_joints_row (a circle of radius 0 straight beside the
    shoulder: q.x == 0 && q.z == 0 bit for bit) with previous joints at every rung: the shoulder pitch returned is the previous
    one as it came, and the rest of the chain is built from ITS sine and cosine — the checker's, and the reduced twin's."""
    torch = torch_mod
    import contextlib
    import io

    from reachy2_symbolic_ik_amd import HipSolver, SymbolicIK
    from reachy2_symbolic_ik_amd.constants import default_ik_parameters
    prm = default_ik_parameters()
    prm["r_shoulder_orientation"] = [0, 0, 0]
    prm["l_shoulder_orientation"] = [0, 0, 0]
    so = -1.01
    solver = HipSolver(0)
    with contextlib.redirect_stdout(io.StringIO()):
        SymbolicIK("r_arm", ik_parameters=prm, singularity_offset=so, solver=solver)._upload()
        SymbolicIK("l_arm", ik_parameters=prm, singularity_offset=so, solver=solver)._upload()
    arms = (orc.Arm("r_arm", so, ik_parameters=prm), orc.Arm("l_arm", so, ik_parameters=prm))
    th, tw, rg = F.far_thetas()
    reps = 4
    n = len(th) * reps
    rng = np.random.default_rng(12)
    arm = (np.arange(n) % 2).astype(np.uint8)
    sy, side = np.where(arm == 1, 0.2, -0.2), np.where(arm == 1, 1.0, -1.0)
    u = f = 0.28
    ey = sy + side * u
    bend, roll = rng.uniform(0.5, 2.5, size=n), rng.uniform(0.0, 2 * np.pi, size=n)
    wrist = np.stack([f * np.sin(bend) * np.cos(roll), ey + side * f * np.cos(bend), f * np.sin(bend) * np.sin(roll)], axis=1)
    hand = np.zeros((n, 32))
    hand[:, 3:6] = rng.uniform(-1.0, 1.0, size=(n, 3))
    hand[:, 6:9] = wrist
    hand[:, 0:3] = wrist + rng.uniform(-0.05, 0.05, size=(n, 3)) + np.array([0.08, 0.0, 0.0])
    hand[:, 10] = ey
    hand[:, 13:16] = np.stack([np.zeros(n), side, np.zeros(n)], axis=1)
    theta = rng.uniform(-np.pi, np.pi, size=n)
    prev, prev_tw = rng.uniform(-3.0, 3.0, size=(n, 7)), None
    prev[:, 0] = np.repeat(th, reps)
    prev[:, 2] = np.repeat(th[::-1], reps)
    prev_tw = prev.copy()
    prev_tw[:, 0], prev_tw[:, 2] = np.repeat(tw, reps), np.repeat(tw[::-1], reps)
    armT = _T(arm, torch, np.uint8)
    out = to_np(solver.joints_from_state(_T(hand, torch), _T(theta, torch), arm=armT, previous_joints=_T(prev, torch)))
    out_tw = to_np(solver.joints_from_state(_T(hand, torch), _T(theta, torch), arm=armT, previous_joints=_T(prev_tw, torch)))
    rows = CheckerRows(arm, arms=arms)
    rows.buf[:, :16] = hand[:, :16]
    want = rows.joints(theta, previous_joints=prev)
    assert np.array_equal(want["joints"][:, 0].view(np.uint64), prev[:, 0].view(np.uint64)), "the checker takes its exact branch"
    assert np.array_equal(out["joints"][:, 0].view(np.uint64), prev[:, 0].view(np.uint64)), "shoulder pitch = previous_joints[0] as it came"
    rung = np.repeat(rg, reps)
    for g, name in enumerate(F.RUNGS):
        m = rung == g
        _close(out["joints"][m, 1:], want["joints"][m, 1:], f"D previous joints, rung {name!r}")
        _close(out["joints"][m, 1:], out_tw["joints"][m, 1:], f"D previous joints against the twin, rung {name!r}")
    _close(out["elbow"], want["elbow"], "D previous joints elbow")


def test_far_preferred_theta_control_discrete(torch_mod, orc):
    """preferred_theta of rsik_control_discrete at every rung and sign (its sine and cosine are the host libm's; the kernel compares
    the angle itself, unwrapped, as the reference does — G22 holds the reference's answers to these very calls): flags, states and
    joints as the checker's."""
    torch = torch_mod
    th, tw, rg = F.far_thetas()
    pos, eul, arm = F.preferred_theta_goals()
    M = F.goal_matrices(pos, eul)
    c = make_control()
    armT = _T(arm, torch, np.uint8)
    ar, al = orc.Arm("r_arm", -1.01), orc.Arm("l_arm", -1.01)
    for q in range(len(th)):
        got = to_np(c.symbolic_inverse_kinematics_batch(armT, M, preferred_theta=float(th[q])))
        ref = orc.control_discrete_batch(ar, al, M, arm_id=arm, nb_search_points=int(c.nb_search_points), preferred_theta=float(th[q]))
        np.testing.assert_array_equal(got["reachable"], ref["reachable"], err_msg=repr(th[q]))
        np.testing.assert_array_equal(got["state"], ref["state"], err_msg=repr(th[q]))
        _close(got["joints"], ref["joints"], f"D control_discrete preferred theta {th[q]!r}", tol=CONT_JOINT_TOL)


def test_far_preferred_theta_continuous(torch_mod, orc):
    """preferred_theta and preferred_theta_self of rsik_control_continuous_step and rsik_control_continuous_run.  The serial
    phases wrap angles with a modulo written for bounded values and carry the theta they start from step to step, so these entry
    points answer below 2^27 — as the checker does, step by step — and REFUSE a finite preferred theta from 2^27 up
    (RSIK_E_INVALID: nothing launched, outputs and carried state untouched); never a wrong row."""
    torch, A = torch_mod, abi()
    from bench import make_config5_trajectories

    bound = 2.0 ** 27
    last = float(np.nextafter(bound, 0.0))
    th = np.concatenate([F.far_thetas()[0], [last, -last, bound, -bound]])   # every rung and sign, and both sides of the bound itself
    n_traj, n_steps = 9, 24
    traj = make_config5_trajectories(n_traj, n_steps, seed=123)
    Ms = m12_soa_to_matrices(traj.cpu().numpy())           # [steps, n, 4, 4]
    a = orc.Arm("r_arm", -1.01)
    c = make_control()
    hs = c._solver
    own = c.preferred_theta["r_arm"]
    below = [q for q in range(len(th)) if abs(th[q]) < bound]
    assert 2 * F.BOUND_RUNG + 2 <= len(below) <= 2 * F.BOUND_RUNG + 4 and len(th) - len(below) >= 2 * (len(F.RUNGS) - F.BOUND_RUNG)

    def checker_run(pref_arg, pref_self):
        J, Fl, S, TH = np.zeros((n_steps, n_traj, 7)), np.zeros((n_steps, n_traj), bool), np.zeros((n_steps, n_traj), int), np.zeros(n_traj)
        for k in range(n_traj):
            cs = orc.ContinuousState(c.previous_theta["r_arm"], c.previous_sol["r_arm"])
            for i in range(n_steps):
                J[i, k], Fl[i, k], S[i, k] = orc.control_continuous_step(a, cs, Ms[i, k], timed_out=(i == 0), preferred_theta_arg=pref_arg,
                                                                         preferred_theta_self=pref_self, constrained_mode=0,
                                                                         current_joints=cs.previous_sol, current_pose=Ms[0, k])
            TH[k] = cs.previous_theta
        return J, Fl, S, TH

    try:
        for q in range(len(th)):
            for which in ("arg", "self"):
                pref_arg = float(th[q]) if which == "arg" else -4 * np.pi / 6
                c.preferred_theta["r_arm"] = float(th[q]) if which == "self" else own
                what = f"D continuous preferred_theta ({which}) {th[q]!r}"
                for mode in (A.CONT_RUN_STEPS, A.CONT_RUN_PHASED):
                    hs.set_option(A.OPT_CONT_RUN_MODE, mode)
                    st = c.new_continuous_state("r_arm", n_traj)
                    before = st.clone()
                    if q in below:
                        o = c.run_continuous_trajectories("r_arm", traj, st, first_step_timed_out=True, current_pose=traj[0], preferred_theta=pref_arg)
                        hs.synchronize()
                        J, Fl, S, TH = checker_run(pref_arg, c.preferred_theta["r_arm"])
                        g = to_np(o)
                        np.testing.assert_array_equal(g["reachable"] != 0, Fl, err_msg=what)
                        np.testing.assert_array_equal(g["state"], S, err_msg=what)
                        _close(g["joints"], J, what + " run joints", tol=CONT_JOINT_TOL)
                        _close(st[0].cpu().numpy(), TH, what + " carried theta", tol=CONT_THETA_TOL)
                    else:
                        with pytest.raises(A.RsikError) as e:
                            c.run_continuous_trajectories("r_arm", traj, st, first_step_timed_out=True, current_pose=traj[0], preferred_theta=pref_arg)
                        assert e.value.code == A.RSIK_E_INVALID and "2^27" in str(e.value), what
                        hs.synchronize()
                        assert _bits_equal(torch, st, before), what
                hs.set_option(A.OPT_CONT_RUN_MODE, A.CONT_RUN_AUTO)
                # one step of the step entry point (the first of a trajectory: timed out, so the start theta is searched from the preferred one)
                st = c.new_continuous_state("r_arm", n_traj)
                before = st.clone()
                to = np.ones(n_traj, dtype=np.uint8)
                if q in below:
                    o = to_np(c.symbolic_inverse_kinematics_continuous_batch("r_arm", Ms[0], st, timed_out=to, current_pose=Ms[0], preferred_theta=pref_arg))
                    np.testing.assert_array_equal(o["state"], S[0], err_msg=what)
                    _close(o["joints"], J[0], what + " step joints", tol=CONT_JOINT_TOL)
                else:
                    with pytest.raises(A.RsikError) as e:
                        c.symbolic_inverse_kinematics_continuous_batch("r_arm", Ms[0], st, timed_out=to, current_pose=Ms[0], preferred_theta=pref_arg)
                    assert e.value.code == A.RSIK_E_INVALID, what
                    assert _bits_equal(torch, st, before), what
    finally:
        c.preferred_theta["r_arm"] = own
        hs.set_option(A.OPT_CONT_RUN_MODE, A.CONT_RUN_AUTO)


# ------------------------------------------------------------------------------------------ E: isolation
@pytest.mark.parametrize("pair", PAIRS)
def test_ordinary_rows_next_to_far_rows_keep_their_bits(torch_mod, orc, pair):
    """A launch that holds far rows among ordinary ones returns, for every ordinary row, the bits of the launch in which the far
    rows held ordinary goals: rsik_solve (explicit theta), rsik_solve_sweep, rsik_solve_nearest, rsik_reach_state."""
    torch, A = torch_mod, abi()
    solver, arms = _setup(pair, orc)
    w = F.wound_rows()
    n = len(w["pos"])
    pf, ef, af, vf, nf = F.far_position_rows()
    th_far = F.far_thetas()[0]
    pos, eul, theta = w["pos"].copy(), w["twin_eul"].copy(), _ordinary_thetas(n, 21)
    clean = (pos.copy(), eul.copy(), theta.copy())
    rng = np.random.default_rng(22)
    bad = np.sort(rng.choice(n, size=n // 8, replace=False))   # scattered over every workgroup
    for q, row in enumerate(bad):
        kind = q % 3
        if kind == 0:
            eul[row] = w["eul"][row]
        elif kind == 1:
            pos[row] = pf[q % len(pf)]
        else:
            theta[row] = th_far[q % len(th_far)]
    keep = _rows_except(torch, n, bad)
    armT = _T(w["arm"], torch, np.uint8)
    frac = np.linspace(0.0, 1.0, 8)
    seed = seeds(n, 82)

    def run(p, e, t):
        out = {}
        res = solver.solve(soa(p, e, torch), arm=armT, theta_policy=A.THETA_EXPLICIT, theta_in=_T(t, torch))
        out.update({"solve " + k: v.clone() for k, v in res.items()})
        res = solver.solve_sweep(soa(p, e, torch), _T(np.stack([t] * 2), torch), policy="explicit", arm=armT)
        out.update({"sweep " + k: (v if v.dim() == 1 or v.shape[0] == n else v.transpose(0, 1)).clone() for k, v in res.items()})
        res = solver.solve_nearest(soa(p, e, torch), _T(frac, torch), _T(seed, torch), policy="fraction", arm=armT)
        out.update({"nearest " + k: v.clone() for k, v in res.items()})
        st = solver.new_solver_state(n)
        res = solver.reach_state(soa(p, e, torch), st, arm=armT)
        out.update({"reach_state " + k: v.clone() for k, v in res.items()})
        out["solver state"] = st.clone()
        torch.cuda.synchronize()
        return out

    a, b = run(pos, eul, theta), run(*clean)
    for k in a:
        assert a[k].shape[0] == n, k
        assert _bits_equal(torch, a[k][keep], b[k][keep]), (pair, k)
