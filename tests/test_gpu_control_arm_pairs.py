"""GPU tests (-m gpu, MI355X) of the control launches and rsik_theta_from_joints on arm pairs that are not the default mirror pair
(tests/arm_pairs.CONTROL_PAIRS and threshold_family()), through HipSolver on a solver from arm_pairs.upload_control(pair), against the CPU
checker with the pair's two arms.  What each kernel must get right that the default pair cannot show:

A. rsik_control_discrete / rsik_control_discrete_rows: grid_theta_candidates' closed forms on other shoulder offsets, upper-arm
   lengths, plane slopes and tip offsets; sweep_theta_grid's fetch of another lane's arm slot on slots that really differ; PLANE
   compiled out for both arms, kept although one arm never binds, and chosen 1e-3 on either side of its threshold.
B. rsik_control_continuous_step and rsik_control_continuous_run (steps, phased, phased in blocks of 8) with an arm byte per
   trajectory, step by step against the checker's state machine, from an explicit start state and a timed-out first step.
C. rsik_theta_from_joints with an arm byte per row: FORM 1 on two arms that differ, FORM 1 against FORM 2 on custom/custom.

tests/test_control_pairs_checker.py asserts the conditions on these inputs on the checker alone; the checker's theta search on the
two non-default geometries is pinned to the reference by G21, its solve by G9 and G20 (tests/test_oracle_golden.py).  Every
tolerance is imported from the module that owns it.

Not covered here: the solver-state kernels (rsik_reach_state, rsik_joints_from_state, rsik_theta_from_joints_state) and the FK
kernels (rsik_forward_kinematics, rsik_fk_residual) take MIXED only, with no FORM or PLANE choice, and stay on the default pair."""
import numpy as np
import pytest

import control_workload as W
import theta_workload as TW
from arm_pairs import CONTROL_PAIRS, checker_arms, control_expectation, threshold_family, upload_control
from compare import CONT_JOINT_TOL, CONT_THETA_TOL, TOL, bits, joint_error, joints_close
from gpu_support import T, _same_run, abi, bucket_vectors, check_against_checker, goal_tensor, m12, to_np, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

FAMILY = list(threshold_family())


def previous_rows(seed, n=W.N, buckets=16):
    """A previous_sol per row as tests/test_gpu_previous_rows.py draws it (gpu_support.bucket_vectors), from `buckets` vectors (the checker takes one vector per
    call): (rows [n, 7], bucket [n], vectors [buckets, 7])."""
    rng = np.random.default_rng(seed)
    vecs = bucket_vectors(rng, buckets)
    bucket = rng.integers(0, buckets, size=n)
    return vecs[bucket], bucket, vecs


def check_discrete(got, ref, what):
    """reachable, state and the emergency verdict exact on every row, joints within TOL (joints_close); returns the largest joint
    difference."""
    for key in ("reachable", "state"):
        np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{what} {key}")
    # (the checker reports whether the stop tripped, the library which joint tripped it)
    np.testing.assert_array_equal(got["emergency"] != 0, ref["emergency"] != 0, err_msg=f"{what} emergency")
    joints_close(got["joints"], ref["joints"], what + " joints", tol=TOL)
    return joint_error(got["joints"], ref["joints"])


# ------------------------------------------------------------------------------------------ A. discrete control
@pytest.mark.parametrize("pair", list(CONTROL_PAIRS) + FAMILY)
def test_control_discrete_on_arm_pairs(torch_mod, golden_dir, pair):
    """The 1000 rows of control_workload.control_rows, an arm byte per row: every RSIK_OPT_SWEEP_MODE x nb_search_points 10, 64, 100 x
    both constrained modes x preferred angle -4 pi / 6 and 2.9, rsik_control_discrete and rsik_control_discrete_rows (a previous_sol per
    row from 16 vectors), against orc.control_discrete_batch with the pair's arms.  No row is set aside: on the checker none of these
    rows rests on a margin below 1e-9 (tests/test_control_pairs_checker.py prints the count per launch)."""
    torch = torch_mod
    _abi = abi()
    M, arm = W.control_rows(golden_dir)
    arms = checker_arms(pair)
    solver = upload_control(pair)
    mm, armT = m12(M, torch), T(arm, torch)
    rows = previous_rows(31)
    rowsT = T(rows[0], torch)
    worst, launches = 0.0, 0
    for nb in W.NBS:
        for pref in W.PREFERRED:
            for mode in (0, 1):
                ref = W.checker_discrete(arms, M, arm, nb, mode, pref)
                ref_rows = W.checker_discrete(arms, M, arm, nb, mode, pref, rows=rows)
                assert ref_rows["emergency"].any() and not ref_rows["emergency"].all()
                for sweep in (0, 1, 2):
                    solver.set_option(_abi.OPT_SWEEP_MODE, sweep)
                    kw = dict(arm=armT, nb_search_points=nb, preferred_theta=pref, constrained_mode=mode)
                    what = f"{pair} nb {nb} pref {pref:.2f} mode {mode} sweep {sweep}"
                    got = to_np(solver.control_discrete(mm, previous_sol=W.DEFAULT_SOL, **kw))
                    worst = max(worst, check_discrete(got, ref, what))
                    got = to_np(solver.control_discrete(mm, previous_sol_rows=rowsT, **kw))
                    worst = max(worst, check_discrete(got, ref_rows, what + " rows"))
                    launches += 2
    solver.set_option(_abi.OPT_SWEEP_MODE, 0)
    print(f"{pair}: {launches} launches, largest joint difference against the checker {worst:.3e}")


@pytest.mark.parametrize("which", [0, 1])
def test_control_discrete_where_the_threshold_plane_decides(torch_mod, which):
    """s* - 1e-3 (PLANE = false) and s* + 1e-3 (PLANE = true) on control_workload.cap_rows, the goals on which the plane of offset
    s* + 1e-3 decides (at least 20 rows per arm, tests/test_control_pairs_checker.py): a launch that drops the plane at s* + 1e-3, or
    keeps a wrong one at s* - 1e-3, answers those rows differently."""
    torch = torch_mod
    _abi = abi()
    pair = FAMILY[which]
    assert control_expectation(pair) == (2, bool(which))
    M, arm = W.cap_rows()
    arms = checker_arms(pair)
    solver = upload_control(pair)
    mm, armT = m12(M, torch), T(arm, torch)
    worst = 0.0
    for nb in W.NBS:
        for pref in W.PREFERRED:
            ref = W.checker_discrete(arms, M, arm, nb, 0, pref, nthreads=8)
            for sweep in (0, 1, 2):
                solver.set_option(_abi.OPT_SWEEP_MODE, sweep)
                got = to_np(solver.control_discrete(mm, arm=armT, nb_search_points=nb, preferred_theta=pref, previous_sol=W.DEFAULT_SOL))
                worst = max(worst, check_discrete(got, ref, f"{pair} cap rows nb {nb} pref {pref:.2f} sweep {sweep}"))
    solver.set_option(_abi.OPT_SWEEP_MODE, 0)
    print(f"{pair} cap rows: largest joint difference against the checker {worst:.3e}")


# ------------------------------------------------------------------------------------------ B. continuous control
def check_continuous(got, theta, latched, ref, i, what):
    np.testing.assert_array_equal(got["reachable"], ref["reachable"][i], err_msg=f"{what} step {i} reachable")
    np.testing.assert_array_equal(got["state"], ref["state"][i], err_msg=f"{what} step {i} state")
    err = float(np.max(np.abs(got["joints"] - ref["joints"][i])))
    assert err < CONT_JOINT_TOL, (what, i, err)
    if theta is not None:
        assert np.max(np.abs(theta - ref["theta"][i])) < CONT_THETA_TOL, (what, i)
        np.testing.assert_array_equal(latched != 0.0, ref["latched"][i], err_msg=f"{what} step {i} latch")
    return err


@pytest.mark.parametrize("pair", list(CONTROL_PAIRS) + FAMILY[:2])
def test_control_continuous_on_arm_pairs(torch_mod, pair):
    """96 trajectories x 25 steps, an arm byte per trajectory, from an explicit start state and a timed-out first step with
    current_joints (the start-up search runs, in its PAIR form where PLANE is false): the step kernel launch by launch, then the run
    entry point as steps, phased, and phased in blocks of 8, each against one orc.control_continuous_step per trajectory-step with
    that trajectory's arm — flags and state codes exact at every step, joints within 1e-7, the carried theta within 1e-9, the latch
    row the checker's — and the run forms against each other (_same_run)."""
    torch = torch_mod
    A = abi()
    Ms, arm, start_j, start_pose = W.trajectories()
    ref = W.checker_trajectories(checker_arms(pair), Ms, arm, start_j, start_pose)
    solver = upload_control(pair)
    armT, sjT, spT = T(arm, torch), T(start_j, torch), m12(start_pose, torch)
    steps = torch.stack([m12(Ms[:, i], torch) for i in range(W.N_STEPS)]).contiguous()   # [steps, 12, n]

    def fresh_state():
        st = solver.new_continuous_state(W.N_TRAJ)
        st[:11].copy_(T(W.start_state(arm), torch))
        return st

    worst = 0.0
    st = fresh_state()
    for i in range(W.N_STEPS):
        got = to_np(solver.control_continuous_step(
            steps[i], st, W.PTS, arm=armT, timed_out=T(np.full(W.N_TRAJ, 1 if i == 0 else 0, dtype=np.uint8), torch),
            current_joints=(sjT if i == 0 else None), current_pose_m12=(spT if i == 0 else steps[i - 1])))
        worst = max(worst, check_continuous(got, st[0].cpu().numpy(), st[9].cpu().numpy(), ref, i, f"{pair} step kernel"))
    assert np.max(np.abs(st[1:8].cpu().numpy().T - ref["previous_sol"])) < CONT_JOINT_TOL
    runs = {}
    try:
        for name, run_mode, blk in (("steps", A.CONT_RUN_STEPS, 0), ("phased", A.CONT_RUN_PHASED, 0), ("phased, blocks of 8", A.CONT_RUN_PHASED, 8)):
            solver.set_option(A.OPT_CONT_RUN_MODE, run_mode)
            solver.set_option(A.OPT_CONT_BLOCK_STEPS, blk)
            st = fresh_state()
            res = solver.control_continuous_run(steps, st, W.PTS, arm=armT, first_step_timed_out=True, current_joints=sjT, current_pose_m12=spT)
            solver.synchronize()
            assert res.run_form == (A.CONT_FORM_STEPS if run_mode == A.CONT_RUN_STEPS else A.CONT_FORM_PHASED), (pair, name, res.run_form)
            runs[name] = {k: v.clone() for k, v in res.items()}
            runs[name]["cont_state"] = st[:11].clone()
            out = to_np(res)
            for i in range(W.N_STEPS):
                worst = max(worst, check_continuous({k: v[i] for k, v in out.items()}, None, None, ref, i, f"{pair} run {name}"))
            end = st.cpu().numpy()
            assert np.max(np.abs(end[0] - ref["theta"][-1])) < CONT_THETA_TOL, (pair, name)
            np.testing.assert_array_equal(end[9] != 0.0, ref["latched"][-1], err_msg=f"{pair} run {name} latch")
            assert np.max(np.abs(end[1:8].T - ref["previous_sol"])) < CONT_JOINT_TOL, (pair, name)
    finally:
        solver.set_option(A.OPT_CONT_RUN_MODE, A.CONT_RUN_AUTO)
        solver.set_option(A.OPT_CONT_BLOCK_STEPS, 0)
    for name in ("phased", "phased, blocks of 8"):
        _same_run(torch, runs["steps"], runs[name], (pair, "steps", name))
    print(f"{pair}: largest joint difference against the checker {worst:.3e}")


# ------------------------------------------------------------------------------------------ C. rsik_theta_from_joints
@pytest.mark.parametrize("pair", ["default/custom", "ztip/default", "default@-1.01/ztip@-1.01", "default@-1.01/default@0.03", "custom/custom"])
def test_theta_from_joints_on_arm_pairs(torch_mod, pair):
    """theta_workload's rows at n = 300 built on the pair's arms, an arm byte per row, pose and matrix goals, against the checker's
    best_theta_to_current_joints with each row's own arm under the acceptance rule of tests/test_gpu_theta_from_joints.py;
    custom/custom under RSIK_OPT_NO_MIRROR (FORM 1) gives the bits of the default launch (FORM 2)."""
    torch = torch_mod
    A = abi()
    n = 300
    arms = checker_arms(pair)
    form, _ = control_expectation(pair)
    pos, eul, arm, cur = TW.theta_workload(TW.SEED + 7, n, arms=arms)
    assert 100 < arm.sum() < 200
    ref = TW.checker_batch(None, pos, eul, arm, cur, arms=arms)
    assert ref["shortcut"].sum() >= 10 and (~ref["shortcut"]).sum() >= 200
    solver = upload_control(pair)
    outs = {}
    for goal_kind in ("pose", "matrix"):
        for no_mirror in ((0, 1) if form == 2 else (0,)):
            solver.set_option(A.OPT_NO_MIRROR, no_mirror)
            res = solver.theta_from_joints(goal_tensor(goal_kind, pos, eul, torch), T(cur, torch), TW.PREFERRED, arm=T(arm, torch))
            torch.cuda.synchronize()
            outs[goal_kind, no_mirror] = to_np(res)
            check_against_checker(outs[goal_kind, no_mirror], ref, None, pos, eul, arm, cur, f"{pair} {goal_kind} no_mirror {no_mirror}", arms=arms)
        solver.set_option(A.OPT_NO_MIRROR, 0)
        if form == 2:
            for key, v in outs[goal_kind, 0].items():
                w = outs[goal_kind, 1][key]
                x, y = (bits(v), bits(w)) if v.dtype == np.float64 else (v, w)
                np.testing.assert_array_equal(x, y, err_msg=f"{pair} {goal_kind}: {key} under NO_MIRROR")
    ok = np.isfinite(ref["joints"]).all(axis=1)
    print(f"{pair}: largest joint difference against the checker {float(np.max(np.abs(outs['pose', 0]['joints'][ok] - ref['joints'][ok]))):.3e}")
