"""GPU tests of include/rsik.h "Goal matrices that are not rotations": the families of tests/matrix_forms.py — rotation blocks that
are scaled, flattened, sheared, at gimbal lock, left-handed or singular — through every entry point that takes a goal matrix.

Where SciPy answers (det > 0) the device answers the same: the nearest rotation's angles against a 50-digit reference and against
the reference's recording (G23), flags and states exactly, joints within the suite's TOL.  Where SciPy raises ValueError (det <= 0)
the row is RSIK_STATE_INVALID_INPUT with NaN outputs, exactly like a row that is not numbers, and the scalar drop-in raises the
same ValueError.  The family rows are interleaved with ordinary goals, which keep the bits they have in a launch without them.
"""
import numpy as np
import pytest

import matrix_forms as F
import theta_workload as W
from checker_support import load
from compare import TOL, same_bits
from gpu_support import (T, _bits_equal, _rows_except, check_against_checker, m12, make_control, make_symbolic, orc,  # noqa: F401
                         to_np, torch_mod)
from rotations import m12_soa_to_matrices

pytestmark = pytest.mark.gpu

ARMS = ("r_arm", "l_arm")
INVALID = F.INVALID_INPUT


@pytest.fixture(scope="module")
def g23(golden_dir):
    return load(golden_dir, F.G23)


def _launch_rows(g23, arms):
    """Every family's rows of the given arms interleaved with those arms' ordinary goals.  Returns the matrices [n,4,4], the arm byte
    per row, {(arm, family): row indices}, the ordinary rows' indices, and a twin of the matrices in which every row of a family
    that the reference raises on holds an ordinary goal of its arm."""
    special, sp_arm, ordinary, or_arm, keys = [], [], [], [], []
    for arm in arms:
        fam = F.family_matrices(g23, arm)
        for f in F.FAMILIES:
            special.append(fam[f])
            keys.append((arm, f))
        sp_arm.append(np.full(len(F.FAMILIES) * F.ROWS, ARMS.index(arm), dtype=np.uint8))
        ordinary.append(F.ordinary_matrices(g23, arm))
        or_arm.append(np.full(F.N_ORDINARY, ARMS.index(arm), dtype=np.uint8))
    special, ordinary = np.concatenate(special), np.concatenate(ordinary)
    M, where, rest = F.interleave(special, ordinary, seed=len(arms))
    byte = np.empty(len(M), dtype=np.uint8)
    byte[where], byte[rest] = np.concatenate(sp_arm), np.concatenate(or_arm)
    index = {key: where[k * F.ROWS:(k + 1) * F.ROWS] for k, key in enumerate(keys)}
    twin = M.copy()
    for (arm, f), idx in index.items():
        if f in F.IMPROPER:
            twin[idx] = F.ordinary_matrices(g23, arm)[np.arange(F.ROWS) % F.N_ORDINARY]
    return M, byte, index, rest, twin


# ------------------------------------------------------------------------------------------ 1. rsik_matrix_to_pose
@pytest.mark.parametrize("identity_shortcut", [0, 1])
def test_matrix_to_pose_on_every_family(torch_mod, g23, identity_shortcut):
    """Families with det > 0: the angles against the 50-digit reference and against G23, as rotations.  det <= 0: NaN angles, the
    position passed through.  The ordinary rows among them keep the bits of a launch that holds only ordinary rows."""
    torch = torch_mod
    solver, _, _ = make_symbolic(0.03)
    for arm in ARMS:
        M, _, index, rest, _ = _launch_rows(g23, (arm,))
        pose = solver.matrix_to_pose(m12(M, torch), identity_shortcut=bool(identity_shortcut)).cpu().numpy()
        alone = solver.matrix_to_pose(m12(M[rest], torch), identity_shortcut=bool(identity_shortcut)).cpu().numpy()
        same_bits(pose[:, rest], alone, f"{arm}: the ordinary rows")
        assert np.isfinite(alone).all()
        for (a, f), idx in index.items():
            same_bits(pose[:3, idx].T, M[idx, :3, 3], f"{arm} {f}: the position")
            F.check_euler(pose[3:6, idx].T, g23, a, f, f"matrix_to_pose shortcut {identity_shortcut}")


# ------------------------------------------------------------------------------------------ 2. rsik_control_discrete (_rows)
@pytest.mark.parametrize("per_row_previous", [0, 1])
@pytest.mark.parametrize("kind", ["r", "l", "mixed"])
def test_control_discrete_on_every_family(torch_mod, g23, kind, per_row_previous):
    """rsik_control_discrete and rsik_control_discrete_rows under RSIK_EULER_AUTO and ALWAYS: G23's flags and states on every row of
    every family, its joints within TOL; the invalid-input contract where the reference raised; every other row bit for bit what
    it is in a twin launch whose bad rows hold an ordinary goal; AUTO and ALWAYS agree."""
    torch = torch_mod
    arms = {"r": ("r_arm",), "l": ("l_arm",), "mixed": ARMS}[kind]
    M, byte, index, rest, twin = _launch_rows(g23, arms)
    n = len(M)
    bad = np.concatenate([idx for (a, f), idx in index.items() if f in F.IMPROPER])
    keep = _rows_except(torch, n, bad)
    results = {}
    for mode in ("auto", "always"):
        c = make_control()
        c.euler_roundtrip = mode
        name = T(byte, torch) if kind == "mixed" else arms[0]
        prev = T(c._previous_sol_2x7()[byte], torch) if per_row_previous else None
        got = {k: v.clone() for k, v in c.symbolic_inverse_kinematics_batch(name, M, previous_sol=prev).items()}
        ref = c.symbolic_inverse_kinematics_batch(name, twin, previous_sol=prev)
        torch.cuda.synchronize()
        for k in got:
            assert _bits_equal(torch, got[k][keep], ref[k][keep]), (mode, k, "rows beside the bad ones")
        assert (ref["state"] != INVALID).all(), "the twin launch holds a bad row"
        res = to_np(got)
        for (a, f), idx in index.items():
            F.check_control({k: v[idx] for k, v in res.items()}, g23, a, f, f"{kind} rows {per_row_previous} {mode}", TOL)
        results[mode] = res
    a, b = results["auto"], results["always"]
    for k in ("reachable", "state", "emergency"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"auto / always: {k}")
    assert np.array_equal(np.isnan(a["joints"]), np.isnan(b["joints"]))
    err = float(np.nanmax(np.abs(a["joints"] - b["joints"])))
    print(f"{kind} rows {per_row_previous}: auto against always {err:.3e}")
    assert err < TOL, err


# ------------------------------------------------------------------------------------------ 3. the continuous step and run
N_TRAJ, N_STEPS = 65, 70
PROPER_TRAJ = {3: ("scaled", 14), 20: ("one_small", 21), 40: ("sheared", 6), 41: ("two_small", 3), 57: ("locked", 0)}
PROPER_STEPS = (0, 9, 10, 33, 69)
BAD_TRAJ = {10: ("left_handed", 0, (5,)), 11: ("left_handed", 7, (0, 1)), 33: ("singular", 0, (30, 31, 32, 33)),
            64: ("singular", 6, (63, 64, 69)), 48: ("left_handed", 2, tuple(range(40, 70)))}


def _trajectories(torch):
    """[N_STEPS, N_TRAJ, 4, 4] goals of ordinary smooth trajectories (the benchmark's generator) and two variants of them.  `goals`:
    a few trajectories keep ONE orientation — the nearest rotation of a block of a proper family — and hold that block itself at some
    steps (the same goal to the reference: the trajectory stays continuous); a few others hold a block the reference raises on at
    some steps.  `twin`: the same, but the bad steps hold the ordinary goal they replaced."""
    from bench import make_config5_trajectories

    base = m12_soa_to_matrices(make_config5_trajectories(N_TRAJ, N_STEPS, seed=23).cpu().numpy())
    goals = base.copy()
    for k, (f, row) in PROPER_TRAJ.items():
        goals[:, k, :3, :3] = F.reference(f)[1][row]
        for s in PROPER_STEPS:
            goals[s, k, :3, :3] = F.blocks(f)[row]
    twin = goals.copy()
    for k, (f, row, steps) in BAD_TRAJ.items():
        for s in steps:
            goals[s, k, :3, :3] = F.blocks(f)[row]
    return goals, twin


def _walk_checker(orc, c, Ms, pose0):
    """One trajectory [n_steps,4,4] through the checker's continuous step (pose0: the current pose its first call is handed): joints,
    reachable, state per step and the state it ends in."""
    a = orc.Arm("r_arm", -1.01)
    cs = orc.ContinuousState(c.previous_theta["r_arm"], c.previous_sol["r_arm"])
    J, ok, st = np.empty((len(Ms), 7)), np.empty(len(Ms), dtype=np.uint8), np.empty(len(Ms), dtype=np.uint8)
    for i, M in enumerate(Ms):
        J[i], ok[i], st[i] = orc.control_continuous_step(a, cs, M, timed_out=(i == 0), preferred_theta_arg=-4 * np.pi / 6,
                                                         preferred_theta_self=c.preferred_theta["r_arm"], constrained_mode=0,
                                                         current_joints=cs.previous_sol, current_pose=pose0)
    return J, ok, st, cs


def _check_special_trajectories(orc, c, goals, pose0, out, st, what):
    """The trajectories that hold family goals, step by step against the checker: flags and states exact, joints to 1e-7 (the
    suite's bound for a walk), INVALID_INPUT and NaN joints on the bad steps, and the carried state the checker ends in."""
    J, ok, code = (out[k].cpu().numpy() for k in ("joints", "reachable", "state"))
    st = st.cpu().numpy()
    for k in sorted(set(PROPER_TRAJ) | set(BAD_TRAJ)):
        wj, wok, wst, cs = _walk_checker(orc, c, goals[:, k], pose0[k])
        np.testing.assert_array_equal(code[:, k], wst, err_msg=f"{what}: trajectory {k} states")
        np.testing.assert_array_equal(ok[:, k], wok, err_msg=f"{what}: trajectory {k} flags")
        assert np.array_equal(np.isnan(J[:, k]), np.isnan(wj)), (what, k, "NaN joints in other places")
        assert float(np.nanmax(np.abs(J[:, k] - wj))) < 1e-7, (what, k, float(np.nanmax(np.abs(J[:, k] - wj))))
        if k in BAD_TRAJ:
            steps = np.array(BAD_TRAJ[k][2])
            live = wst[steps] != 8
            assert live.any() and (code[steps[live], k] == INVALID).all() and np.isnan(J[steps[live], k]).all(), (what, k)
            assert not ok[steps, k].any(), (what, k)
        else:
            assert (code[:, k] != INVALID).all(), (what, k)
        assert abs(cs.previous_theta - st[0, k]) < 1e-9 and float(np.max(np.abs(cs.previous_sol - st[1:8, k]))) < 1e-7, (what, k)
        assert cs.emergency_stop == bool(st[9, k] != 0), (what, k)


def test_continuous_run_steps_over_goals_the_reference_raises_on(torch_mod, orc):
    """rsik_control_continuous_run as RSIK_CONT_RUN_STEPS and RSIK_CONT_RUN_PHASED, 65 trajectories x 70 steps: steps that hold a
    block of a proper family are answered like the checker answers them; a step that holds a reflection or a singular block reports
    INVALID_INPUT and NaN joints and the trajectory goes on; every other trajectory is bit for bit that of the twin run; the two
    forms agree (flags, states and the carried theta bit for bit, joints to 1e-9: gpu_support._same_run says why not their bits)."""
    torch = torch_mod
    A = __import__("reachy2_symbolic_ik_amd")._abi
    goals, twin = _trajectories(torch)
    c = make_control()
    hs = c._solver
    st0 = c.new_continuous_state("r_arm", N_TRAJ)
    keep = _rows_except(torch, N_TRAJ, sorted(BAD_TRAJ))
    results = {}
    try:
        for name, mode in (("steps", A.CONT_RUN_STEPS), ("phased", A.CONT_RUN_PHASED)):
            hs.set_option(A.OPT_CONT_RUN_MODE, mode)
            runs = []
            for Ms in (goals, twin):
                st = st0.clone()
                o = c.run_continuous_trajectories("r_arm", Ms, st, first_step_timed_out=True, current_pose=twin[0])
                hs.synchronize()
                runs.append(({k: v.clone() for k, v in o.items()}, st.clone()))
            (go, gst), (to, tst) = runs
            for k in go:
                assert _bits_equal(torch, go[k][:, keep], to[k][:, keep]), (name, k, "the other trajectories")
            assert _bits_equal(torch, gst[:, keep], tst[:, keep]), (name, "cont_state of the other trajectories")
            assert (to["state"] != INVALID).all(), "the twin run holds a bad goal"
            _check_special_trajectories(orc, c, goals, twin[0], go, gst, name)
            results[name] = (go, gst)
    finally:
        hs.set_option(A.OPT_CONT_RUN_MODE, A.CONT_RUN_AUTO)
    (so, sst), (po, pst) = results["steps"], results["phased"]
    assert _bits_equal(torch, so["state"], po["state"]) and _bits_equal(torch, so["reachable"], po["reachable"])
    assert torch.equal(torch.isnan(so["joints"]), torch.isnan(po["joints"]))
    assert float((torch.nan_to_num(so["joints"]) - torch.nan_to_num(po["joints"])).abs().max()) <= 1e-9
    assert _bits_equal(torch, sst[0], pst[0]) and torch.equal(sst[8:11], pst[8:11])
    assert float((sst[1:8] - pst[1:8]).abs().max()) <= 1e-9


def test_continuous_step_leaves_the_state_of_a_bad_goal_alone(torch_mod, orc):
    """rsik_control_continuous_step, launch by launch over the same trajectories: on a bad step previous_sol, init and the latch of
    that trajectory are bit for bit what they were, the other trajectories bit for bit those of the twin, and the walk ends where
    the checker's ends."""
    torch = torch_mod
    goals, twin = _trajectories(torch)
    c, c2 = make_control(), make_control()
    st, st2 = c.new_continuous_state("r_arm", N_TRAJ), c2.new_continuous_state("r_arm", N_TRAJ)
    keep = _rows_except(torch, N_TRAJ, sorted(BAD_TRAJ))
    outs = {k: [] for k in ("joints", "reachable", "state")}
    for i in range(N_STEPS):
        to = np.full(N_TRAJ, 1 if i == 0 else 0, dtype=np.uint8)
        before = st.clone()
        got = c.symbolic_inverse_kinematics_continuous_batch("r_arm", goals[i], st, timed_out=to, current_pose=twin[0])
        ref = c2.symbolic_inverse_kinematics_continuous_batch("r_arm", twin[i], st2, timed_out=to, current_pose=twin[0])
        torch.cuda.synchronize()
        for k in outs:
            assert _bits_equal(torch, got[k][keep], ref[k][keep]), (i, k)
            outs[k].append(got[k].clone())
        assert _bits_equal(torch, st[:, keep], st2[:, keep]), i
        for k, (_, _, steps) in BAD_TRAJ.items():
            if i in steps and i > 0 and int(got["state"][k]) == INVALID:
                assert _bits_equal(torch, st[1:11, k], before[1:11, k]), (i, k, "previous_sol / init / latch / has_previous_sol")
                assert bool(torch.isnan(got["joints"][k]).all()) and int(got["reachable"][k]) == 0
    _check_special_trajectories(orc, c, goals, twin[0], {k: torch.stack(v) for k, v in outs.items()}, st, "step kernel")


# ------------------------------------------------------------------------------------------ 4. rsik_theta_from_joints
def test_theta_from_joints_with_a_matrix_goal(torch_mod, orc, g23):
    """rsik_theta_from_joints on goal matrices of every family, r and l in one launch: det > 0 against the checker on the checker's
    own angles of the block; det <= 0 gives INVALID_INPUT and NaN outputs in that row, and no other row changes."""
    torch = torch_mod
    solver, _, _ = make_symbolic(0.03)
    M, byte, index, rest, twin = _launch_rows(g23, ARMS)
    n = len(M)
    cur = np.random.default_rng(F.SEED).uniform(-0.6, 0.6, size=(n, 7))
    got = to_np(solver.theta_from_joints(m12(M, torch), T(cur, torch), W.PREFERRED, arm=T(byte, torch)))
    ref = to_np(solver.theta_from_joints(m12(twin, torch), T(cur, torch), W.PREFERRED, arm=T(byte, torch)))
    bad = np.zeros(n, dtype=bool)
    for (a, f), idx in index.items():
        bad[idx] = f in F.IMPROPER
    assert (got["state"][bad] == INVALID).all() and (ref["state"] != INVALID).all()
    for k in ("theta", "joints", "bracket", "distance"):
        assert np.isnan(got[k][bad]).all(), k
        same_bits(got[k][~bad], ref[k][~bad], f"{k}: the other rows")
    same_bits(got["state"][~bad].astype(np.float64), ref["state"][~bad].astype(np.float64), "state: the other rows")
    proper = np.concatenate([idx for (a, f), idx in index.items() if f in F.PROPER])
    pos, eul = M[proper, :3, 3], orc.euler_from_matrix_xyz(M[proper])
    want = W.checker_batch(0.03, pos, eul, byte[proper], cur[proper])
    ok = want["ok"]
    assert ok.mean() > 0.9, ok.mean()
    assert (got["state"][proper][~ok] == 9).all(), "rows the checker's is_reachable_no_limits refuses"
    rows = proper[ok]
    check_against_checker({k: v[rows] for k, v in got.items()}, {k: v[ok] for k, v in want.items()}, 0.03, pos[ok], eul[ok],
                          byte[rows], cur[rows], "matrix goals of the proper families")


# ------------------------------------------------------------------------------------------ 5. the scalar drop-in
def test_scalar_drop_in_raises_value_error_like_scipy(torch_mod, g23):
    """ControlIK.symbolic_inverse_kinematics (discrete, continuous) and utils.get_euler_from_homogeneous_matrix raise SciPy's
    ValueError for a reflection and for the zero block, the object's state stays as it was, and a batch never raises."""
    from reachy2_symbolic_ik_amd import utils

    c = make_control()
    M = np.eye(4)
    M[:3, 3] = [0.4, -0.25, -0.2]
    c.symbolic_inverse_kinematics("r_arm", M, "continuous")
    th, ps, init = c.previous_theta["r_arm"], np.array(c.previous_sol["r_arm"]).copy(), c.init
    reflection, zero = M.copy(), M.copy()
    reflection[:3, :3] = F.blocks("left_handed")[0]
    zero[:3, :3] = 0.0
    for bad in (reflection, zero):
        for kind in ("discrete", "continuous"):
            with pytest.raises(ValueError, match="^Non-positive determinant"):
                c.symbolic_inverse_kinematics("r_arm", bad, kind)
        with pytest.raises(ValueError, match="^Non-positive determinant"):
            utils.get_euler_from_homogeneous_matrix(bad)
    assert abs(c.previous_theta["r_arm"] - th) < 1e-15 and np.array_equal(np.array(c.previous_sol["r_arm"]), ps)
    assert c.init == init and not c.emergency_stop
    nan = M.copy()
    nan[0, 0] = np.nan
    with pytest.raises(np.linalg.LinAlgError):
        c.symbolic_inverse_kinematics("r_arm", nan, "discrete")
    j1, ok1, s1 = c.symbolic_inverse_kinematics("r_arm", M, "continuous")
    twin = make_control()  # the same two good calls, nothing in between
    twin.symbolic_inverse_kinematics("r_arm", M, "continuous")
    j2, ok2, s2 = twin.symbolic_inverse_kinematics("r_arm", M, "continuous")
    assert ok1 == ok2 and s1 == s2 and np.max(np.abs(np.array(j1) - np.array(j2))) < 1e-9
    res = to_np(c.symbolic_inverse_kinematics_batch("r_arm", np.stack([reflection, zero, M])))
    assert res["state"][:2].tolist() == [INVALID, INVALID] and res["state"][2] != INVALID and np.isnan(res["joints"][:2]).all()
    pos, eul = utils.get_euler_from_homogeneous_matrix(F.goal_matrices(F.blocks("scaled")[15:16], M[None, :3, 3])[0])
    assert float(F.rotation_error(eul[None], F.reference("scaled")[0][15:16])[0]) < F.tolerance("scaled")
