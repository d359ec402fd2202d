"""rsik_theta_from_joints / rsik_theta_from_joints_state and the rate-limiter stages on the GPU, against the CPU checker
(oracle.Solver, one object per row) and the reference's own recordings (G19) — never against the code under test.

Where the search's decisions agree it only adds and divides by 3 numbers below 2 pi, so theta and the bracket agree to 1e-12;
joints and the distance use TOL, the joint tolerance of the state path (tests/compare.py).  A row whose theta
differs is only accepted as a NEAR TIE: the replay of its search with the checker's get_joints must hold a comparison whose two
sides are within 1e-9 (a hundred times the 1e-11 rad the project holds its joints to), and the device's theta must be what the
search gives with that one comparison reversed; at most 1 row in 10 000.  The expected bracket of a row is looked up by the
checker's theta in the table of all 2^16 brackets the search can end in (tests/theta_workload.py).
"""
import contextlib
import io
import os

import numpy as np
import pytest

import scale_inputs as SC
import theta_workload as W
from checker_support import CheckerRows
from compare import close, same_bits
from gpu_support import EXACT, KINDS, URDF, T, arm_kwargs, check_against_checker, goal_tensor, make_symbolic, soa, to_np, torch_mod  # noqa: F401
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SOS = (-1.01, 0.03)


def kind_workload(kind, n, seed=W.SEED, so=0.03):
    return W.theta_workload(seed + KINDS.index(kind), n, arm={"r": 0, "l": 1, "mixed": None}[kind], so=so)


# ------------------------------------------------------------------------------------------ the fused entry point, full size
@pytest.mark.parametrize("so", SOS)
@pytest.mark.parametrize("kind", KINDS)
def test_fused_against_checker_full_size(torch_mod, kind, so):
    """262 144 rows (config-3 size), pose and matrix goals of the same rows, row by row against the checker."""
    torch = torch_mod
    n = W.N_FULL
    pos, eul, arm, cur = kind_workload(kind, n, so=so)
    ref = W.checker_batch(so, pos, eul, arm, cur)
    print(f"{kind} so {so}: shortcut {ref['shortcut'].mean():.4f}, moved {ref['moved'].mean():.4f}")
    assert ref["shortcut"].mean() > 0.05 and (ref["moved"].mean() > 0.02) == (so > 0)
    solver, _, _ = make_symbolic(so)
    outs = {}
    for goal_kind in ("pose", "matrix"):
        res = solver.theta_from_joints(goal_tensor(goal_kind, pos, eul, torch), T(cur, torch), W.PREFERRED, **arm_kwargs(kind, arm, torch))
        torch.cuda.synchronize()
        outs[goal_kind] = to_np(res)
        check_against_checker(outs[goal_kind], ref, so, pos, eul, arm, cur, f"{kind} so {so} {goal_kind}")


# ------------------------------------------------------------------------------------------ the reference's recordings
@pytest.fixture(scope="module")
def g19(golden_dir):
    return np.load(os.path.join(golden_dir, "g19_start_theta.npz"))


def check_g19(theta, bracket, g, pre, rows, what):
    err = np.max(np.abs(theta - g[pre + "theta"][rows]))
    print(f"{what}: theta err {err:.3e} over {len(rows)} rows")
    assert err < 1e-9, (what, err)
    want = np.stack([g[pre + "low"][rows], g[pre + "high"][rows]], axis=1)
    close(bracket, want, what + " bracket", tol=1e-9)


@pytest.mark.parametrize("tag,so", (("so101", -1.01), ("so003", 0.03)))
def test_g19_through_the_fused_and_the_state_entry(g19, torch_mod, tag, so):
    torch = torch_mod
    solver, _, _ = make_symbolic(so)
    for a, arm in enumerate(("r_arm", "l_arm")):
        pre = f"{arm}_{tag}_"
        for p in np.unique(g19[pre + "pref"]):
            rows = np.flatnonzero(g19[pre + "pref"] == p)
            pos, eul, cur = g19[pre + "pos"][rows], g19[pre + "eul"][rows], g19[pre + "cur"][rows]
            for goal_kind in ("pose", "matrix"):
                res = to_np(solver.theta_from_joints(goal_tensor(goal_kind, pos, eul, torch), T(cur, torch), [p, p], arm_uniform=a))
                assert (res["state"] == 0).all()
                check_g19(res["theta"], res["bracket"], g19, pre, rows, f"{pre}{goal_kind} pref {p:.3f}")
            st = solver.new_solver_state(len(rows))
            rs = solver.reach_state(soa(pos, eul, torch), st, arm_uniform=a, no_limits=True)
            assert bool(rs["reachable"].all())
            res = to_np(solver.theta_from_joints_state(st, T(cur, torch), [p, p], arm_uniform=a))
            check_g19(res["theta"], res["bracket"], g19, pre, rows, f"{pre}state pref {p:.3f}")


def test_g19_through_the_utils_functions(g19, torch_mod):
    """The three drop-in functions of reachy2_symbolic_ik_amd.utils with the reference's signatures: theta to 1e-9, booleans and
    texts exact."""
    from reachy2_symbolic_ik_amd import SymbolicIK
    from reachy2_symbolic_ik_amd import utils as U

    for arm in ("r_arm", "l_arm"):
        for tag, so in (("so101", -1.01), ("so003", 0.03)):
            pre = f"{arm}_{tag}_"
            with contextlib.redirect_stdout(io.StringIO()):
                s = SymbolicIK(arm, singularity_offset=so)
            for i in range(0, 256, 4 if so < 0 else 3):
                ok, _, fn = s.is_reachable_no_limits(np.array([g19[pre + "pos"][i], g19[pre + "eul"][i]]))
                assert ok
                theta, text = U.get_best_theta_to_current_joints(fn, 20, list(g19[pre + "cur"][i]), arm, g19[pre + "pref"][i])
                assert abs(theta - g19[pre + "theta"][i]) < 1e-9, (pre, i)
                if np.isnan(g19[pre + "low"][i]):
                    assert text == "preferred_theta worked!" and theta == g19[pre + "pref"][i]
                else:
                    low, high = (float(v.split(",")[0]) for v in text.split("= ")[1:3])
                    assert abs(low - g19[pre + "low"][i]) < 1e-9 and abs(high - g19[pre + "high"][i]) < 1e-9
    for row, ok, th in zip(g19["tend_in"], g19["tend_ok"], g19["tend_theta"]):
        got = U.tend_to_preferred_theta(row[0], np.array([-np.pi, np.pi]), None, row[1], row[2])
        assert got[0] == bool(ok) and abs(got[1] - th) < 1e-9, row
    solvers = {}
    for i in range(len(g19["cont2_ok"])):
        key = (("r_arm", "l_arm")[int(g19["cont2_arm"][i])], float(g19["cont2_so"][i]))
        if key not in solvers:
            with contextlib.redirect_stdout(io.StringIO()):
                solvers[key] = SymbolicIK(key[0], singularity_offset=key[1])
        s = solvers[key]
        ok, interval, _, _ = s.is_reachable(np.array([g19["cont2_pos"][i], g19["cont2_eul"][i]]))
        assert ok
        prev, i0, i1, dmax, pref = g19["cont2_in"][i]
        good, th, text = U.get_best_continuous_theta2(prev, np.array([i0, i1]), s.get_elbow_position, 10, dmax, pref, key[0], key[1], 1.0,
                                                      s.elbow_singularity_position)
        code = 2 if text.endswith("ok mais loin") else (1 if text.endswith("ok et proche") else 0)
        assert (good, code) == (bool(g19["cont2_ok"][i]), int(g19["cont2_text"][i])), i
        assert abs(th - g19["cont2_theta"][i]) < 1e-9, i


def test_rate_limiter_stages_as_batches(g19, torch_mod):
    """The two new rsik_stage operations on whole batches (HipSolver.stage), against G19."""
    from reachy2_symbolic_ik_amd import _abi

    torch = torch_mod
    solver, r, l = make_symbolic(0.03)
    out = solver.stage(_abi.STAGE_TEND_TO_PREFERRED_THETA, T(g19["tend_in"], torch)).cpu().numpy()
    np.testing.assert_array_equal(out[:, 0], g19["tend_ok"].astype(np.float64))
    assert np.max(np.abs(out[:, 1] - g19["tend_theta"])) < 1e-9


# ------------------------------------------------------------------------------------------ the state entry point
@pytest.mark.parametrize("kind", KINDS)
def test_state_entry_is_the_fused_one_where_nothing_moves(torch_mod, kind):
    """singularity_offset -1.01: no projection can fire, the two entry points walk the same search — theta and bracket bit for bit."""
    torch = torch_mod
    n = 8192 + 37
    pos, eul, arm, cur = kind_workload(kind, n, seed=5, so=-1.01)
    solver, _, _ = make_symbolic(-1.01)
    kw = arm_kwargs(kind, arm, torch)
    fused = to_np(solver.theta_from_joints(soa(pos, eul, torch), T(cur, torch), W.PREFERRED, **kw))
    st = solver.new_solver_state(n)
    solver.reach_state(soa(pos, eul, torch), st, no_limits=True, **kw)
    res = to_np(solver.theta_from_joints_state(st, T(cur, torch), W.PREFERRED, **kw))
    same_bits(res["theta"], fused["theta"], "theta")
    same_bits(res["bracket"], fused["bracket"], "bracket")
    close(st.cpu().numpy()[:, 24:31], fused["joints"], "slots 24-30 against the fused joints")


@pytest.mark.parametrize("kind", KINDS)
def test_state_entry_leaves_the_checker_objects_state(torch_mod, kind):
    """singularity_offset 0.03: every row ends in the state the checker's solver object ends in after the same get_joints calls
    (goal position and wrist moved by every projection that fired, slots 16-19 and 24-30 of the last evaluation)."""
    torch = torch_mod
    n = 3000
    pos, eul, arm, cur = kind_workload(kind, n, seed=9)
    solver, _, _ = make_symbolic(0.03)
    kw = arm_kwargs(kind, arm, torch)
    st = solver.new_solver_state(n)
    solver.reach_state(soa(pos, eul, torch), st, no_limits=True, **kw)
    res = to_np(solver.theta_from_joints_state(st, T(cur, torch), W.PREFERRED, **kw))
    S = st.cpu().numpy()
    rows = CheckerRows(arm, so=0.03)
    assert rows.reach(pos, eul, no_limits=True)["reachable"].all()
    rep = [W.replay(rows.solver(i), cur[i], arm[i], W.PREFERRED[arm[i]]) for i in range(n)]
    moved = np.array([not np.array_equal(rows.buf[i, :3], pos[i]) for i in range(n)])
    print(f"{kind}: {int(moved.sum())} of {n} rows moved by a projection")
    assert moved.mean() > 0.02
    theta = np.array([r["theta"] for r in rep])
    assert (np.abs(res["theta"] - theta) <= EXACT).all()
    close(res["bracket"], np.array([[r["low"], r["high"]] for r in rep]), "bracket", tol=EXACT)
    close(S[:, 0:16], rows.buf[:, 0:16], "slots 0-15")
    close(S[:, 16:19], rows.buf[:, 16:19], "slots 16-18 (elbow of the last get_joints)")
    np.testing.assert_array_equal(S[:, 19], np.array([float(r["projected"]) for r in rep]))
    close(S[:, 24:31], np.array([r["joints"] for r in rep]), "slots 24-30")


def test_state_entry_constructor_form(torch_mod):
    """n_current = 14, the list-of-both-arms form of ControlIK.__init__ (Q15), against the checker's 2x7 form on generic rows."""
    torch = torch_mod
    n = 2048
    pos, eul, arm, _ = kind_workload("mixed", n, seed=13)
    cur = np.random.default_rng(14).uniform(-0.6, 0.6, size=(n, 14))
    solver, _, _ = make_symbolic(0.03)
    st = solver.new_solver_state(n)
    solver.reach_state(soa(pos, eul, torch), st, arm=T(arm, torch), no_limits=True)
    res = to_np(solver.theta_from_joints_state(st, T(cur, torch), W.PREFERRED, arm=T(arm, torch)))
    rows = CheckerRows(arm, so=0.03)
    rows.reach(pos, eul, no_limits=True)
    theta = np.array([rows.solver(i).best_theta_to_current_joints(cur[i].reshape(2, 7), W.PREFERRED[arm[i]]) for i in range(n)])
    assert (np.abs(res["theta"] - theta) <= EXACT).all(), np.flatnonzero(~(np.abs(res["theta"] - theta) <= EXACT))
    close(st.cpu().numpy()[:, 0:9], rows.buf[:, 0:9], "goal and wrist after the search")


# ------------------------------------------------------------------------------------------ agreement with the start-up that exists
@pytest.mark.parametrize("name", ("r_arm", "l_arm", "mixed"))
def test_new_continuous_state_is_the_timed_out_start_up(torch_mod, name):
    """new_continuous_state(current_joints, current_pose) + one step with timed_out = 0 gives, bit for bit, the joints, flags and
    state rows of today's default state + the same step with timed_out = 1 and those current_joints / current_pose."""
    torch = torch_mod
    from reachy2_symbolic_ik_amd import ControlIK

    n = 4096 + 11
    kind = {"r_arm": "r", "l_arm": "l", "mixed": "mixed"}[name]
    pos, eul, arm, cur = kind_workload(kind, n, seed=21)
    rng = np.random.default_rng(22)
    goal = SC.matrices_from_pose(pos + rng.uniform(-0.01, 0.01, size=pos.shape), eul + rng.uniform(-0.02, 0.02, size=eul.shape))
    cur_pose = SC.matrices_from_pose(pos, eul)
    for is_dvt in (False, True):
        with contextlib.redirect_stdout(io.StringIO()):
            c = ControlIK(urdf_path=URDF, is_dvt=is_dvt)
        who = name if name != "mixed" else T(arm, torch)
        cj = T(cur, torch)
        st_a = c.new_continuous_state(who, n)
        a = c.symbolic_inverse_kinematics_continuous_batch(who, goal, st_a, timed_out=torch.ones(n, dtype=torch.uint8, device="cuda"),
                                                           current_joints=cj, current_pose=cur_pose)
        st_b = c.new_continuous_state(who, n, current_joints=cj, current_pose=cur_pose)
        assert np.array_equal(st_b[1:8].cpu().numpy(), cur.T) and bool((st_b[8] == 1).all()) and bool((st_b[10] == 1).all())
        b = c.symbolic_inverse_kinematics_continuous_batch(who, goal, st_b, timed_out=torch.zeros(n, dtype=torch.uint8, device="cuda"))
        for k in ("joints", "reachable", "state"):
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (name, is_dvt, k)
        same_bits(st_a.cpu().numpy(), st_b.cpu().numpy(), f"{name} dvt {is_dvt} state rows")
        # and start_theta_batch is row 0 of that state
        th = c.start_theta_batch(who, cur_pose, cj)["theta"]
        st_c = c.new_continuous_state(who, n, current_joints=cj, current_pose=cur_pose)
        same_bits(th.cpu().numpy(), st_c[0].cpu().numpy(), "start_theta_batch")
        # without the two arguments: exactly what it returned before
        st_d = c.new_continuous_state(who, n).cpu().numpy()
        assert (st_d[8] == 1).all() and (st_d[10] == 1).all() and (st_d[11:] == 0).all()
        for k, nm in enumerate(("r_arm", "l_arm")):
            m = arm == k
            assert (st_d[0, m] == c.previous_theta[nm]).all() and (st_d[1:8, m] == np.asarray(c.previous_sol[nm]).reshape(7, 1)).all()


# ------------------------------------------------------------------------------------------ hostile rows, sizes, arguments
def test_rows_that_are_not_numbers_stay_in_their_rows(torch_mod):
    torch = torch_mod
    n = 1000
    pos, eul, arm, cur = kind_workload("mixed", n, seed=31)
    solver, _, _ = make_symbolic(0.03)
    for goal_kind in ("pose", "matrix"):
        g = goal_tensor(goal_kind, pos, eul, torch)
        clean = to_np(solver.theta_from_joints(g, T(cur, torch), W.PREFERRED, arm=T(arm, torch)))
        gb, cb = g.clone(), T(cur, torch)
        bad_goal, bad_cur = np.array([3, 64, 65, 500, 999]), np.array([7, 127, 640])
        for k, i in enumerate(bad_goal):
            gb[k % gb.shape[0], int(i)] = (float("nan"), float("inf"), -float("inf"))[k % 3]
        for k, i in enumerate(bad_cur):
            cb[int(i), k * 3] = (float("nan"), float("inf"), -float("inf"))[k % 3]
        got = to_np(solver.theta_from_joints(gb, cb, W.PREFERRED, arm=T(arm, torch)))
        bad = np.zeros(n, dtype=bool)
        bad[bad_goal] = bad[bad_cur] = True
        assert (got["state"][bad] == 10).all() and (got["state"][~bad] == 0).all()
        for k in ("theta", "joints", "bracket", "distance"):
            assert np.isnan(got[k][bad]).all(), k
            same_bits(got[k][~bad], clean[k][~bad], f"{goal_kind} {k}: the other rows")


def test_a_pose_is_reachable_no_limits_refuses(torch_mod):
    """A solver whose projection_margin is negative lets is_reachable_no_limits fail (symbolic_ik.py:343-345): state 9, NaN."""
    torch = torch_mod
    from reachy2_symbolic_ik_amd import SymbolicIK

    from reachy2_symbolic_ik_amd.constants import default_ik_parameters

    with contextlib.redirect_stdout(io.StringIO()):
        s = SymbolicIK("r_arm", projection_margin=-0.05)
    A = orc.Arm("r_arm", 0.03, ik_parameters=default_ik_parameters(), projection_margin=-0.05)
    pos = np.array([[2.0, -0.2, 0.0], [0.4, -0.2, -0.1]])
    eul = np.array([[0.0, -np.pi / 2, 0.0]] * 2)
    want = [orc.Solver(A).is_reachable_no_limits(pos[i], eul[i]) for i in range(2)]
    assert want == [False, True]
    res = to_np(s.theta_from_joints_batch(soa(pos, eul, torch), np.zeros((2, 7))))
    assert res["state"].tolist() == [9, 0] and np.isnan(res["theta"][0]) and np.isnan(res["joints"][0]).all() and np.isfinite(res["theta"][1])
    assert np.isnan(res["bracket"][0]).all() and np.isnan(res["distance"][0])


@pytest.mark.parametrize("n", (1, 63, 65, 257, 1000))
def test_ragged_sizes_and_null_outputs(torch_mod, n):
    """Guard rows behind every output stay as they were; a launch with every optional output NULL writes the same theta."""
    torch = torch_mod
    pos, eul, arm, cur = kind_workload("mixed", n + 5, seed=41)
    solver, _, _ = make_symbolic(0.03)
    big = to_np(solver.theta_from_joints(soa(pos, eul, torch), T(cur, torch), W.PREFERRED, arm=T(arm, torch)))
    guard = 7
    shapes = {"theta": (n + guard,), "joints": (n + guard, 7), "bracket": (n + guard, 2), "distance": (n + guard,)}
    bufs = {k: torch.full(s, -77.0, dtype=torch.float64, device="cuda") for k, s in shapes.items()}
    bufs["state"] = torch.full((n + guard,), 99, dtype=torch.uint8, device="cuda")
    out = {k: v[:n] for k, v in bufs.items()}
    res = solver.theta_from_joints(soa(pos[:n], eul[:n], torch), T(cur[:n], torch), W.PREFERRED, arm=T(arm[:n], torch), out=out)
    assert all(res[k].data_ptr() == out[k].data_ptr() for k in out)
    for k, v in bufs.items():
        h = v.cpu().numpy()
        same_bits(h[:n].astype(np.float64), big[k][:n].astype(np.float64), f"n {n} {k}")
        assert (h[n:] == (99 if k == "state" else -77.0)).all(), k
    only = solver.theta_from_joints(soa(pos[:n], eul[:n], torch), T(cur[:n], torch), W.PREFERRED, arm=T(arm[:n], torch), want=())
    assert set(only) == {"theta"}
    same_bits(only["theta"].cpu().numpy(), big["theta"][:n], "theta with every optional output NULL")


def test_both_forms_of_an_arm_byte_per_row_give_the_same_bits(torch_mod):
    """Mirror-image arms let a mixed launch read only the constants with a handedness per lane; RSIK_OPT_NO_MIRROR forces the form
    that reads every constant per lane (what arms that are not mirror images get).  Same numbers, so same bits — and the checker."""
    torch = torch_mod
    from reachy2_symbolic_ik_amd import _abi

    n = 20000
    pos, eul, arm, cur = kind_workload("mixed", n, seed=71)
    solver, _, _ = make_symbolic(0.03)
    a = to_np(solver.theta_from_joints(soa(pos, eul, torch), T(cur, torch), W.PREFERRED, arm=T(arm, torch)))
    solver.set_option(_abi.OPT_NO_MIRROR, 1)
    b = to_np(solver.theta_from_joints(soa(pos, eul, torch), T(cur, torch), W.PREFERRED, arm=T(arm, torch)))
    solver.set_option(_abi.OPT_NO_MIRROR, 0)
    for k in a:
        same_bits(a[k].astype(np.float64), b[k].astype(np.float64), k)
    ref = W.checker_batch(0.03, pos, eul, arm, cur)
    check_against_checker(b, ref, 0.03, pos, eul, arm, cur, "every constant per lane")


def test_empty_batches_null_pointers_and_shapes(torch_mod):
    import ctypes as C

    torch = torch_mod
    from reachy2_symbolic_ik_amd import _abi

    solver, r, l = make_symbolic(0.03)
    pref = (C.c_double * 2)(*W.PREFERRED)
    lib, h = solver.lib, solver._h
    assert lib.rsik_theta_from_joints(h, 0, 0, None, None, 0, None, None, None, None, None, None, None) == _abi.RSIK_OK
    assert lib.rsik_theta_from_joints_state(h, 0, None, None, 0, None, 7, None, None, None) == _abi.RSIK_OK
    pos, eul, arm, cur = kind_workload("r", 8, seed=51)
    g, cj, th = soa(pos, eul, torch), T(cur, torch), torch.empty(8, dtype=torch.float64, device="cuda")
    cols = (C.c_void_p * 6)(*[g[k].data_ptr() for k in range(6)])
    E = _abi.RSIK_E_INVALID
    assert lib.rsik_theta_from_joints(h, 8, 0, cols, None, 0, cj.data_ptr(), pref, None, None, None, None, None) == E
    assert lib.rsik_theta_from_joints(h, 8, 0, cols, None, 0, None, pref, th.data_ptr(), None, None, None, None) == E
    assert lib.rsik_theta_from_joints(h, 8, 0, None, None, 0, cj.data_ptr(), pref, th.data_ptr(), None, None, None, None) == E
    assert lib.rsik_theta_from_joints(h, 8, 0, cols, None, 0, cj.data_ptr(), None, th.data_ptr(), None, None, None, None) == E
    assert lib.rsik_theta_from_joints(h, 8, 2, cols, None, 0, cj.data_ptr(), pref, th.data_ptr(), None, None, None, None) == E
    assert lib.rsik_theta_from_joints(h, -1, 0, cols, None, 0, cj.data_ptr(), pref, th.data_ptr(), None, None, None, None) == E
    st = solver.new_solver_state(8)
    assert lib.rsik_theta_from_joints_state(h, 8, st.data_ptr(), None, 0, cj.data_ptr(), 8, pref, th.data_ptr(), None) == E
    assert lib.rsik_theta_from_joints_state(h, 8, None, None, 0, cj.data_ptr(), 7, pref, th.data_ptr(), None) == E
    assert lib.rsik_theta_from_joints(h, 8, 0, cols, None, 0, cj.data_ptr(), pref, th.data_ptr(), None, None, None, None) == _abi.RSIK_OK
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        solver.theta_from_joints(g[:5], cj, W.PREFERRED)
    with pytest.raises(ValueError):
        solver.theta_from_joints(g, cj[:7], W.PREFERRED)
    with pytest.raises(ValueError):
        solver.theta_from_joints(g.float(), cj, W.PREFERRED)
    with pytest.raises(ValueError):
        solver.theta_from_joints(g, cj, [0.0])
    with pytest.raises(ValueError):
        solver.theta_from_joints(g, cj, W.PREFERRED, out={"theta": torch.empty(9, dtype=torch.float64, device="cuda")})
    with pytest.raises(ValueError):
        solver.theta_from_joints(g, cj, W.PREFERRED, arm=torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        solver.theta_from_joints_state(st, torch.zeros((8, 9), dtype=torch.float64), W.PREFERRED)
    with contextlib.redirect_stdout(io.StringIO()):
        from reachy2_symbolic_ik_amd import ControlIK

        c = ControlIK(urdf_path=URDF)
    with pytest.raises(ValueError):
        c.new_continuous_state("r_arm", 8, current_joints=cj)


def test_capture_and_replay_with_refilled_inputs(torch_mod):
    torch = torch_mod
    n = 4096
    solver, r, l = make_symbolic(0.03)
    sets = [kind_workload("mixed", n, seed=s) for s in (61, 62)]
    g, cj, arm = soa(sets[0][0], sets[0][1], torch).clone(), T(sets[0][3], torch).clone(), T(sets[0][2], torch).clone()
    out = {"theta": torch.empty(n, dtype=torch.float64, device="cuda"), "joints": torch.empty((n, 7), dtype=torch.float64, device="cuda"),
           "bracket": torch.empty((n, 2), dtype=torch.float64, device="cuda"), "distance": torch.empty(n, dtype=torch.float64, device="cuda"),
           "state": torch.empty(n, dtype=torch.uint8, device="cuda")}
    eager = [to_np(solver.theta_from_joints(soa(p, e, torch), T(c, torch), W.PREFERRED, arm=T(a, torch))) for p, e, a, c in sets]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            solver.theta_from_joints(g, cj, W.PREFERRED, arm=arm, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for k, (p, e, a, c) in enumerate(sets):
        g.copy_(soa(p, e, torch)); cj.copy_(T(c, torch)); arm.copy_(T(a, torch))
        graph.replay()
        torch.cuda.synchronize()
        for key in out:
            same_bits(out[key].cpu().numpy().astype(np.float64), eager[k][key].astype(np.float64), f"replay {k} {key}")
