"""Per-row previous joints (rsik_solve_rows / rsik_control_discrete_rows): n independent callers, each with its own last
solution, in one launch.  Checked against the CPU checker (oracle/), whose batch drivers take one previous vector per call,
by bucketing rows that share a vector; against the reference's own G11 recordings; and against the launch-uniform entry
points bit for bit."""
import copy
import os

import numpy as np
import pytest

from compare import NORTH_STAR_TOL, TOL
from gpu_support import bucket_vectors, m12, make_control, make_symbolic_dual, orc, soa, to_np, torch_mod, wrist_pitch  # noqa: F401

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)


def random_poses(n, seed):
    rng = np.random.default_rng(seed)
    pos = np.array([0.0, -0.1, 0.0]) + rng.uniform(-0.7, 0.7, size=(n, 3))
    return pos, rng.uniform(-np.pi, np.pi, size=(n, 3))


def assert_same(a, b, keys=None):
    for k in keys or a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ------------------------------------------------------------------------------------------ discrete against the checker
@pytest.mark.parametrize("nb,mode,with_cj", [(20, "unconstrained", False), (20, "low_elbow", True),
                                             (64, "unconstrained", True), (64, "low_elbow", False)])
def test_discrete_rows_config3_against_checker(torch_mod, orc, nb, mode, with_cj):
    """262 144 config-3 goal matrices, mixed arms, one previous_sol per row from 256 buckets: flags, state codes and the
    emergency verdict bit for bit, joints within the config-3 bounds, every cause bit tripped somewhere."""
    from bench import make_config3_matrices

    n = 1 << 18
    M = make_config3_matrices(n, seed=20250204 + 7)
    rng = np.random.default_rng(nb + (7 if with_cj else 0) + (100 if mode == "low_elbow" else 0))
    arm = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    vecs = bucket_vectors(rng, 256)
    bucket = rng.integers(0, 256, size=n)
    prev = vecs[bucket]
    cj = rng.uniform(-np.pi, np.pi, size=(n, 7)) if with_cj else None
    c = make_control()
    c.nb_search_points = nb
    res = to_np(c.symbolic_inverse_kinematics_batch(torch_mod.as_tensor(arm).cuda(), M, constrained_mode=mode,
                                                    current_joints=None if cj is None else torch_mod.as_tensor(cj).cuda(),
                                                    previous_sol=torch_mod.as_tensor(prev).cuda()))
    R, L = orc.Arm("r_arm", -1.01), orc.Arm("l_arm", -1.01)
    mc = {"unconstrained": 0, "low_elbow": 1}[mode]
    ref = {k: np.empty_like(v) for k, v in res.items()}
    for b in range(256):
        idx = np.nonzero(bucket == b)[0]
        r = orc.control_discrete_batch(R, L, M[idx], arm_id=arm[idx], nb_search_points=nb, constrained_mode=mc,
                                       previous_sol=np.stack([vecs[b], vecs[b]]),
                                       current_joints=None if cj is None else cj[idx], nthreads=NTHREADS)
        for k in ref:
            ref[k][idx] = r[k]
    for k in ("reachable", "state"):
        np.testing.assert_array_equal(res[k], ref[k], err_msg=k)
    # the checker reports whether the stop tripped (0 / 1); the cause bits are checked against the reference (G11)
    np.testing.assert_array_equal(res["emergency"] != 0, ref["emergency"] != 0)
    err = np.abs(res["joints"] - ref["joints"])
    assert np.max(err) < NORTH_STAR_TOL and np.quantile(err, 0.9999) < 1e-9
    for bit in (1, 2, 4):
        assert np.any(res["emergency"] & bit), bit
    assert len(np.unique(res["state"])) >= 3
    # a few thousand rows, every one with a vector of its own, through the checker one row per call
    k = 2000
    own = bucket_vectors(rng, k)
    sel = rng.choice(n, size=k, replace=False)
    res2 = to_np(c.symbolic_inverse_kinematics_batch(torch_mod.as_tensor(arm[sel]).cuda(), M[sel], constrained_mode=mode,
                                                     current_joints=None if cj is None else torch_mod.as_tensor(cj[sel]).cuda(),
                                                     previous_sol=torch_mod.as_tensor(own).cuda()))
    for i in range(k):
        r = orc.control_discrete_batch(R, L, M[sel[i]:sel[i] + 1], arm_id=arm[sel[i]:sel[i] + 1], nb_search_points=nb,
                                       constrained_mode=mc, previous_sol=np.stack([own[i], own[i]]),
                                       current_joints=None if cj is None else cj[sel[i]:sel[i] + 1])
        for key in ("reachable", "state"):
            assert res2[key][i] == r[key][0], (key, i)
        assert (res2["emergency"][i] != 0) == (r["emergency"][0] != 0), i
        assert np.max(np.abs(res2["joints"][i] - r["joints"][0])) < NORTH_STAR_TOL


def test_g11_discrete_rows_in_one_launch(golden_dir, torch_mod):
    """G11, the reference itself: every discrete row of an arm in ONE launch, each with its own recorded previous_sol."""
    g = np.load(os.path.join(golden_dir, "g11_emergency.npz"))
    c = make_control()
    for a, arm in enumerate(("r_arm", "l_arm")):
        pre = f"{arm}_discrete_"
        prev = np.ascontiguousarray(g[pre + "current_joints"][:, a, :])
        res = to_np(c.symbolic_inverse_kinematics_batch(arm, g[pre + "M"], previous_sol=torch_mod.as_tensor(prev).cuda()))
        np.testing.assert_array_equal(res["reachable"].astype(bool), g[pre + "ok1"].astype(bool))
        assert np.max(np.abs(res["joints"] - g[pre + "joints1"])) < TOL
        np.testing.assert_array_equal(res["emergency"], g[pre + "cause"])


# ------------------------------------------------------------------------------------------ solve
@pytest.mark.parametrize("no_tipz", [0, 1])
def test_solve_rows_near_singular_catalogue(golden_dir, torch_mod, orc, no_tipz):
    """G1 catalogue (mixed arms, both singularity offsets) with a random previous_joints row per pose, on the TIPZ and the
    general path.  The catalogue's fully extended poses are singular to rounding, not exactly, so get_joints does not read
    previous_joints there (the checker keeps it on none of them): every row is rsik_solve's answer bit for bit, and the near-
    singular rows agree with the checker run with that row's own previous_joints.  (No input found so far makes the solve
    kernel's exact-singularity branch fire; the per-row read is exercised by the discrete tests above.)"""
    from reachy2_symbolic_ik_amd import _abi

    g = np.load(os.path.join(golden_dir, "g1_catalogue.npz"))
    rng = np.random.default_rng(5 + no_tipz)
    for tag, so in (("so003_", 0.03), ("so101_", -1.01)):
        solver, _, _ = make_symbolic_dual(so)
        solver.set_option(_abi.OPT_NO_TIPZ, no_tipz)
        n = len(g["arm"])
        prev = rng.uniform(-3.0, 3.0, size=(n, 7))
        p, arm = soa(g["pos"], g["eul"], torch_mod), torch_mod.as_tensor(g["arm"]).cuda()
        rows = to_np(solver.solve(p, arm=arm, previous_joints_rows=torch_mod.as_tensor(prev).cuda()))
        uni = to_np(solver.solve(p, arm=arm, previous_joints=np.zeros(7)))
        assert_same(rows, uni)
        sing = (np.abs(g[tag + "joints"][:, 3]) < 1e-12) & g[tag + "reachable"].astype(bool)
        assert sing.sum() >= 3
        R, L = orc.Arm("r_arm", so), orc.Arm("l_arm", so)
        for i in np.nonzero(sing)[0]:
            ref = orc.solve_batch(R, L, g["pos"][i:i + 1], g["eul"][i:i + 1], arm_id=g["arm"][i:i + 1], previous_joints=prev[i])
            a, b = rows["joints"][i], ref["joints"][0]
            # (fully extended arm: only j2 + j6 is defined, as in test_gpu_parity.check_symbolic)
            assert np.max(np.abs(a[[0, 1, 3, 4, 5]] - b[[0, 1, 3, 4, 5]])) < TOL
            dsum = (a[2] + a[6]) - (b[2] + b[6])
            assert abs(dsum - 2 * np.pi * np.round(dsum / (2 * np.pi))) < 1e-7


# ------------------------------------------------------------------------------------------ uniform equivalence
def test_solve_rows_uniform_is_rsik_solve(torch_mod):
    """Every row holding the launch-uniform vector: rsik_solve_rows returns rsik_solve's bits, every theta policy, uniform
    and mixed arms."""
    from reachy2_symbolic_ik_amd import _abi

    solver, _, _ = make_symbolic_dual(0.03)
    n = 40000
    pos, eul = random_poses(n, 21)
    rng = np.random.default_rng(22)
    p = soa(pos, eul, torch_mod)
    arm = torch_mod.as_tensor((rng.uniform(size=n) < 0.5).astype(np.uint8)).cuda()
    theta = torch_mod.as_tensor(rng.uniform(0, 1, size=n)).cuda()
    pj = rng.uniform(-2, 2, size=7)
    rows = torch_mod.as_tensor(np.tile(pj, (n, 1))).cuda()
    for policy in (_abi.THETA_INTERVAL0, _abi.THETA_EXPLICIT, _abi.THETA_FRACTION, _abi.THETA_NONE):
        th = theta if policy in (_abi.THETA_EXPLICIT, _abi.THETA_FRACTION) else None
        for a in (None, arm):
            kw = dict(arm=a, arm_uniform=1, theta_policy=policy, theta_in=th)
            u = to_np(solver.solve(p, previous_joints=pj, **kw))
            r = to_np(solver.solve(p, previous_joints_rows=rows, **kw))
            assert u["reachable"].sum() > 1000
            assert_same(r, u)


@pytest.mark.parametrize("with_cj", [False, True])
def test_discrete_rows_uniform_is_rsik_control_discrete(torch_mod, with_cj):
    """Every row holding its arm's launch-uniform previous_sol: rsik_control_discrete_rows returns rsik_control_discrete's
    bits.  Without current_joints, the rows that find no theta fall back to previous_sol and take the sin / cos of its wrist
    on the device instead of from the host's libm: those (and only those) may differ, within TOL."""
    from bench import make_config3_matrices

    n = 1 << 16
    M = make_config3_matrices(n, seed=99)
    rng = np.random.default_rng(23)
    arm = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    ps = rng.uniform(-4 * np.pi, 4 * np.pi, size=(2, 7))
    ps[:, 5] = wrist_pitch(rng, 2)
    cj = torch_mod.as_tensor(rng.uniform(-np.pi, np.pi, size=(n, 7))).cuda() if with_cj else None
    c = make_control()
    s = c._solver
    mm = m12(M, torch_mod)
    for a in (None, torch_mod.as_tensor(arm).cuda()):
        arm_of_row = arm if a is not None else np.zeros(n, np.uint8)
        rows = torch_mod.as_tensor(ps[arm_of_row]).cuda()
        kw = dict(arm=a, arm_uniform=0, nb_search_points=20, current_joints=cj)
        u = to_np(s.control_discrete(mm, previous_sol=ps, **kw))
        r = to_np(s.control_discrete(mm, previous_sol_rows=rows, **kw))
        assert_same(r, u, ("reachable", "state", "emergency"))
        fallback = u["reachable"] == 0
        assert fallback.sum() > 100  # the population whose wrist sin / cos is evaluated differently
        if with_cj:
            assert_same(r, u, ("joints",))
        else:
            np.testing.assert_array_equal(r["joints"][~fallback], u["joints"][~fallback])
            diff = np.any(r["joints"] != u["joints"], axis=1)
            assert diff.sum() <= fallback.sum()
            assert np.max(np.abs(r["joints"][fallback] - u["joints"][fallback])) < TOL


# ------------------------------------------------------------------------------------------ row isolation
def test_rows_that_are_not_numbers_stay_in_their_rows(torch_mod):
    """NaN / +-inf in some rows' previous vectors change nothing in any other row; the poisoned rows follow the "Rows that
    are not numbers" rule (their joints that depend on a bad value are NaN, flags and state codes are the ordinary ones,
    a NaN never trips an emergency stop)."""
    from bench import make_config3_matrices

    n = 1 << 15
    rng = np.random.default_rng(31)
    bad = rng.uniform(size=n) < 0.05
    poison = np.array([np.nan, np.inf, -np.inf])

    def poisoned(v):
        v = v.copy()
        cols = rng.integers(0, 7, size=int(bad.sum()))
        v[np.nonzero(bad)[0], cols] = poison[rng.integers(0, 3, size=int(bad.sum()))]
        return v

    # solve: previous_joints is read only at an exact singularity, so every row keeps its bits
    solver, _, _ = make_symbolic_dual(0.03)
    pos, eul = random_poses(n, 32)
    p = soa(pos, eul, torch_mod)
    clean = rng.uniform(-2, 2, size=(n, 7))
    a = to_np(solver.solve(p, previous_joints_rows=torch_mod.as_tensor(clean).cuda()))
    b = to_np(solver.solve(p, previous_joints_rows=torch_mod.as_tensor(poisoned(clean)).cuda()))
    assert_same({k: v[~bad] for k, v in b.items()}, {k: v[~bad] for k, v in a.items()})
    # discrete
    M = make_config3_matrices(n, seed=33)
    c = make_control()
    mm = m12(M, torch_mod)
    clean = rng.uniform(-4 * np.pi, 4 * np.pi, size=(n, 7))
    dirty = poisoned(clean)
    arm = torch_mod.as_tensor((rng.uniform(size=n) < 0.5).astype(np.uint8)).cuda()
    a = to_np(c._solver.control_discrete(mm, arm=arm, previous_sol_rows=torch_mod.as_tensor(clean).cuda()))
    b = to_np(c._solver.control_discrete(mm, arm=arm, previous_sol_rows=torch_mod.as_tensor(dirty).cuda()))
    assert_same({k: v[~bad] for k, v in b.items()}, {k: v[~bad] for k, v in a.items()})
    assert_same({k: v[bad] for k, v in b.items()}, {k: v[bad] for k, v in a.items()}, ("reachable", "state"))
    nonfinite = ~np.isfinite(dirty[bad])
    assert np.all(np.isnan(b["joints"][bad][nonfinite]))
    em = b["emergency"][bad]
    for k, bit in ((0, 1), (2, 2), (6, 4)):
        assert not np.any(em[nonfinite[:, k]] & bit)


# ------------------------------------------------------------------------------------------ Python layers
def test_python_layers_and_shape_errors(torch_mod):
    solver, r, dual = make_symbolic_dual(0.03)
    n = 5000
    pos, eul = random_poses(n, 41)
    rng = np.random.default_rng(42)
    p = soa(pos, eul, torch_mod)
    prev = torch_mod.as_tensor(rng.uniform(-2, 2, size=(n, 7))).cuda()
    arm = torch_mod.as_tensor((rng.uniform(size=n) < 0.5).astype(np.uint8)).cuda()
    assert_same(to_np(r.solve_batch(p, previous_joints=prev)), to_np(solver.solve(p, arm_uniform=0, previous_joints_rows=prev)))
    assert_same(to_np(dual.solve_batch(arm, p, previous_joints=prev.cpu().numpy())),
                to_np(solver.solve(p, arm=arm, previous_joints_rows=prev)))
    # (7,) keeps the launch-uniform path
    assert_same(to_np(r.solve_batch(p, previous_joints=[0.1] * 7)), to_np(solver.solve(p, previous_joints=[0.1] * 7)))
    for bad in (np.zeros((n, 6)), np.zeros((n + 1, 7)), np.zeros((n, 7, 1))):
        with pytest.raises(ValueError):
            r.solve_batch(p, previous_joints=bad)
    with pytest.raises(ValueError):
        solver.solve(p, previous_joints=np.zeros(7), previous_joints_rows=prev)

    from bench import make_config3_matrices

    M = make_config3_matrices(4096, seed=43)
    c = make_control()
    c.previous_sol["r_arm"] = np.full(7, 0.25)
    before = (copy.deepcopy(c.previous_sol), c.emergency_stop)
    ps = torch_mod.as_tensor(rng.uniform(-4 * np.pi, 4 * np.pi, size=(4096, 7))).cuda()
    got = to_np(c.symbolic_inverse_kinematics_batch("r_arm", M, previous_sol=ps))
    want = to_np(c._solver.control_discrete(m12(M, torch_mod), arm_uniform=0, nb_search_points=int(c.nb_search_points),
                                            orbita3d_max_angle=float(c.orbita3D_max_angle), previous_sol_rows=ps))
    assert_same(got, want)
    assert c.emergency_stop == before[1] and c.previous_sol.keys() == before[0].keys()
    for k in before[0]:
        np.testing.assert_array_equal(c.previous_sol[k], before[0][k])
    for bad in (np.zeros((4096, 6)), np.zeros((4095, 7)), np.zeros(7)):
        with pytest.raises(ValueError):
            c.symbolic_inverse_kinematics_batch("r_arm", M, previous_sol=bad)
    with pytest.raises(ValueError):
        c._solver.control_discrete(m12(M, torch_mod), previous_sol=np.zeros((2, 7)), previous_sol_rows=ps)


def test_planned_rows_launches_replay_from_a_graph(torch_mod):
    """plan_only=True with per-row previous vectors, recorded into a torch.cuda.graph: the replay gives the eager bits."""
    from bench import make_config3_matrices

    solver, r, _ = make_symbolic_dual(0.03)
    n = 8192
    pos, eul = random_poses(n, 51)
    rng = np.random.default_rng(52)
    p = soa(pos, eul, torch_mod)
    prev = torch_mod.as_tensor(rng.uniform(-2, 2, size=(n, 7))).cuda()
    M = make_config3_matrices(n, seed=53)
    c = make_control()
    ps = torch_mod.as_tensor(rng.uniform(-4 * np.pi, 4 * np.pi, size=(n, 7))).cuda()
    eager_s = to_np(r.solve_batch(p, previous_joints=prev))
    eager_d = to_np(c.symbolic_inverse_kinematics_batch("l_arm", M, previous_sol=ps))
    plan_s = r.solve_batch(p, previous_joints=prev, plan_only=True)
    plan_d = c.symbolic_inverse_kinematics_batch("l_arm", M, previous_sol=ps, plan_only=True)
    plan_s["launch"]()
    plan_d["launch"]()
    torch_mod.cuda.synchronize()
    for plan in (plan_s, plan_d):
        for k, v in plan.items():
            if hasattr(v, "zero_"):
                v.zero_()
    g = torch_mod.cuda.CUDAGraph()
    with torch_mod.cuda.graph(g, capture_error_mode="thread_local"):
        cs = torch_mod.cuda.current_stream().cuda_stream
        plan_s["launch"](cs)
        plan_d["launch"](cs)
    g.replay()
    torch_mod.cuda.synchronize()
    assert_same(to_np(plan_s), eager_s)
    assert_same(to_np(plan_d), eager_d)
