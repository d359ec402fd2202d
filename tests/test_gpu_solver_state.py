"""GPU tests (-m gpu, MI355X) of the solver-state entry points AS BATCHES: rsik_reach_state, rsik_joints_from_state and
rsik_elbow_from_state (csrc/rsik_kernel_state.hpp), plus the mixed-arm instantiation of the FK kernels.

Every caller that keeps the reference's call shape (is_reachable(pose), then the returned get_joints closure,
get_elbow_position, is_reachable_no_limits) runs through these three kernels, and joints_state_kernel is the only caller of
joints_from_theta<FRESH = false>: measured |wrist - elbow| and |tip - wrist|, the exact singularity-plane test, the tip taken
through to_elbow(toff + pos), the stored goal moved and the wrist recomputed when the projection fires, the circle frame
rebuilt from the stored normal.  The fused kernels share none of that.

Reference: the CPU checker's solver OBJECT (oracle.Solver), one per row, stepped call by call on the host
(tests/test_solver_state_checker.py pins it to the reference's G3 and to the checker's batch).  Bars are the project's own:
reachable / state / projection flag bit-exact, numbers within TOL = 1e-9 row by row, the config-2 bars at full size
(max < NORTH_STAR_TOL, 0.9999-quantile < 1e-9).  Exact-singular rows (elbow pitch 0) are compared like check_symbolic does:
j2 + j6 modulo 2 pi.  Every figure is printed before it is asserted (pytest -s shows them).
"""
import os

import numpy as np
import pytest

import scale_inputs as SC
from checker_support import ELBOW_LIMIT, CheckerRows, _check_scale_set, reachable_rich, state_workload
from compare import NORTH_STAR_TOL, close, joints_close, same_bits
from fk_numpy import forward_kinematics
from gpu_support import (KINDS, T, _bits_equal, _rows_except, arm_kwargs, cols, last_error, make_symbolic, orc, ptr, raw_call, soa,  # noqa: F401
                         to_np, torch_mod)
from rotations import euler_to_matrix

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)
SHOULDER = {0: np.array([0.0, -0.2, 0.0]), 1: np.array([0.0, 0.2, 0.0])}
SHOULDER_OFFSET_DEG = {0: [-15, 0, 10], 1: [15, 0, -10]}


# ------------------------------------------------------------------------------------------ helpers
def workload(kind, seed, n):
    pos, eul, arm = state_workload(seed, n, arm={"r": 0, "l": 1, "mixed": None}[kind])
    if kind == "mixed" and n >= 512:
        waves = arm[: n - n % 64].reshape(-1, 64).sum(axis=1)
        assert ((waves > 0) & (waves < 64)).all(), "r and l must alternate inside every wave (and so across every block)"
    return pos, eul, arm


def inside(interval, u):
    a, b = interval[:, 0], interval[:, 1].copy()
    b[a > b] += 2 * np.pi
    return a + u * (b - a)


def raw_reach(solver, n, p, st, arm=None, arm_uniform=0, no_limits=0, interval=None, reachable=None, state=None):
    """rsik_reach_state on the caller's own buffers (the wrapper allocates its outputs): returns the ABI's code."""
    return raw_call(solver, "rsik_reach_state", n, cols(p, 6), ptr(arm), int(arm_uniform), int(no_limits), ptr(st), ptr(interval),
                    ptr(reachable), ptr(state))


def raw_joints(solver, n, st, theta, arm=None, arm_uniform=0, prev=None, joints=None, elbow=None):
    return raw_call(solver, "rsik_joints_from_state", n, ptr(st), ptr(arm), int(arm_uniform), ptr(theta), ptr(prev), ptr(joints), ptr(elbow))


def raw_elbow(solver, n, st, theta, elbow):
    return raw_call(solver, "rsik_elbow_from_state", n, ptr(st), ptr(theta), ptr(elbow))


def check_reach(rs, ref, what):
    np.testing.assert_array_equal(rs["reachable"], ref["reachable"], err_msg=what)
    np.testing.assert_array_equal(rs["state"], ref["state"], err_msg=what)
    close(rs["interval"], ref["interval"], what + " interval")


def check_row_results(S, out, what):
    """Slots 16-18 / 24-30 of the row are the returned elbow / joints; 31 is reserved."""
    same_bits(S[:, 16:19], out["elbow"], what + " slots 16-18")
    same_bits(S[:, 24:31], out["joints"], what + " slots 24-30")


# ------------------------------------------------------------------------------------------ a. sequences, row by row
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("so", [0.03, -1.01])
def test_sequences_against_the_checker_object(torch_mod, orc, so, kind):
    """test_scalar_state_semantics_Q1 at thousands of rows: reach_state, three joints_from_state calls on the same state tensor
    (theta = interval[0], a theta inside the interval, a theta anywhere in [-2 pi, 2 pi]: the second and third start from what a
    projection left behind), then elbow_from_state — after every call the outputs and slots 0-15 of every reachable row against
    the checker's object of that row."""
    torch = torch_mod
    n = 40000
    pos, eul, arm = workload(kind, 1000 + KINDS.index(kind), n)
    kw = arm_kwargs(kind, arm, torch)
    solver, _, _ = make_symbolic(so)
    rows = CheckerRows(arm, so=so)
    st = solver.new_solver_state(n)
    rs = to_np(solver.reach_state(soa(pos, eul, torch), st, **kw))
    ref = rows.reach(pos, eul)
    check_reach(rs, ref, "reach_state")
    S = st.cpu().numpy()
    close(S[:, :16], rows.buf[:, :16], "slots 0-15 after reach_state")
    same_bits(S[:, 20:22], rs["interval"], "slots 20-21")
    np.testing.assert_array_equal(S[:, 22], rs["reachable"])
    np.testing.assert_array_equal(S[:, 23], rs["state"])
    assert not S[:, 16:20].any() and not S[:, 24:].any()
    m = np.flatnonzero(ref["reachable"])
    assert len(m) >= 0.04 * n
    rng = np.random.default_rng(5)
    itv = np.nan_to_num(ref["interval"])
    thetas = (itv[:, 0], inside(itv, rng.uniform(0.02, 0.98, size=n)), rng.uniform(-2 * np.pi, 2 * np.pi, size=n))
    fired = 0
    for call, th in enumerate(thetas):
        what = f"so {so} {kind} get_joints call {call}"
        theta = np.zeros(n)
        theta[m] = th[m]
        head = S[:, 20:24].copy()
        out = to_np(solver.joints_from_state(st, T(theta, torch), **kw))
        want = rows.joints(theta, rows=m)
        S = st.cpu().numpy()
        np.testing.assert_array_equal(S[m, 19], want["projected"][m], err_msg=what + " projection flag")
        joints_close(out["joints"][m], want["joints"][m], what + " joints")
        close(out["elbow"][m], want["elbow"][m], what + " elbow")
        close(S[m, :16], rows.buf[m, :16], what + " slots 0-15")
        check_row_results(S, out, what)
        same_bits(S[:, 20:24], head, what + " slots 20-23")
        assert not S[:, 31].any()
        fired += int(want["projected"][m].sum())
    assert (fired > 0.2 * len(m)) if so > 0 else fired == 0
    theta = rng.uniform(-np.pi, np.pi, size=n)
    e = solver.elbow_from_state(st, T(theta, torch)).cpu().numpy()
    close(e[m], rows.elbow(theta, rows=m)[m], f"so {so} {kind} get_elbow_position")
    same_bits(st.cpu().numpy(), S, "elbow_from_state does not write the state")


# ------------------------------------------------------------------------------------------ b. the slots a call leaves alone
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("prefill", ["sentinel", "reachable"])
def test_reach_state_writes_only_what_the_reference_assigns(torch_mod, orc, prefill, kind):
    """include/rsik.h "Solver-state entry points": only the fields the reference would have assigned are written.  The state
    tensor starts from a sentinel or from the rows a reachable batch left; which of slots 0-15 a call may change is taken from the
    checker's object started from the same row (early "Pose out of reach" / "Backward pose": none; "wrist out of range": goal and
    wrist, not the circle).  Slots 16-19 and 24-31 are never written; 20-23 always are."""
    torch = torch_mod
    n = 30000
    pos, eul, arm = workload(kind, 2000 + KINDS.index(kind), n)
    kw = arm_kwargs(kind, arm, torch)
    solver, _, _ = make_symbolic(0.03)
    if prefill == "sentinel":
        st = T(np.tile(1000.0 + np.arange(32.0), (n, 1)), torch)
    else:
        p0, e0 = reachable_rich(3, n, arm)
        st = solver.new_solver_state(n)
        r0 = solver.reach_state(soa(p0, e0, torch), st, **kw)
        assert float(r0["reachable"].double().mean()) > 0.5
        solver.joints_from_state(st, torch.nan_to_num(r0["interval"][:, 0]).contiguous(), **kw)
    pre = st.cpu().numpy().copy()
    rows = CheckerRows(arm, init=pre[:, :19])
    rs = to_np(solver.reach_state(soa(pos, eul, torch), st, **kw))
    ref = rows.reach(pos, eul)
    check_reach(rs, ref, "reach_state")
    S = st.cpu().numpy()
    # which slots the reference assigns: what a checker object started from a sentinel no longer holds (a slot may be assigned
    # the value it held: the wrist's x is backward_limit after every backward shift)
    marked = CheckerRows(arm, init=np.tile(1000.0 + np.arange(19.0), (n, 1)))
    marked.reach(pos, eul)
    assigned = marked.buf[:, :16] != 1000.0 + np.arange(16.0)
    early = np.isin(ref["state"], (1, 2))
    late = np.isin(ref["state"], (3, 5))
    print(f"{prefill} {kind}: early refusals {early.mean():.3f}, later refusals {late.mean():.4f}, reachable {ref['reachable'].mean():.3f}")
    assert early.mean() >= 0.5 and late.sum() > 0 and not assigned[early].any()
    assert assigned[late][:, :9].all() and not assigned[late][:, 9:].any()
    assert assigned[~early & ~late].all()
    same_bits(S[:, :16][~assigned], pre[:, :16][~assigned], "slots the reference leaves alone")
    close(S[:, :16][assigned], rows.buf[:, :16][assigned], "slots the reference assigns")
    same_bits(S[:, 16:20], pre[:, 16:20], "slots 16-19")
    same_bits(S[:, 24:32], pre[:, 24:32], "slots 24-31")
    same_bits(S[:, 20:22], rs["interval"], "slots 20-21")
    np.testing.assert_array_equal(S[:, 22], rs["reachable"])
    np.testing.assert_array_equal(S[:, 23], rs["state"])


# ------------------------------------------------------------------------------------------ c. no_limits = 1 as a batch
@pytest.mark.parametrize("kind", KINDS)
def test_no_limits_batch_against_the_checker_object(torch_mod, orc, kind):
    """is_reachable_no_limits as a batch: reachability, [-pi, pi], the geometry slots and get_joints on that state, row by row."""
    torch = torch_mod
    n = 20000
    pos, eul, arm = workload(kind, 3000 + KINDS.index(kind), n)
    kw = arm_kwargs(kind, arm, torch)
    solver, _, _ = make_symbolic(0.03)
    rows = CheckerRows(arm)
    st = solver.new_solver_state(n)
    rs = to_np(solver.reach_state(soa(pos, eul, torch), st, no_limits=True, **kw))
    ref = rows.reach(pos, eul, no_limits=True)
    np.testing.assert_array_equal(rs["reachable"], ref["reachable"])
    ok = ref["reachable"].astype(bool)
    assert ok.mean() > 0.99
    assert (rs["state"][ok] == 0).all() and (rs["interval"][ok] == (-np.pi, np.pi)).all()
    S = st.cpu().numpy()
    close(S[:, :16], rows.buf[:, :16], f"no_limits {kind} slots 0-15")
    m = np.flatnonzero(ok)
    theta = np.random.default_rng(8).uniform(-np.pi, np.pi, size=n)
    out = to_np(solver.joints_from_state(st, T(theta, torch), **kw))
    want = rows.joints(theta, rows=m)
    S = st.cpu().numpy()
    np.testing.assert_array_equal(S[m, 19], want["projected"][m])
    assert 0.05 < want["projected"][m].mean() < 0.95
    joints_close(out["joints"][m], want["joints"][m], f"no_limits {kind} joints")
    close(out["elbow"][m], want["elbow"][m], f"no_limits {kind} elbow")
    close(S[m, :16], rows.buf[m, :16], f"no_limits {kind} slots 0-15 after get_joints")
    check_row_results(S, out, f"no_limits {kind}")


def test_g5_helpers_as_batches(golden_dir, torch_mod):
    """G5 (the reference's own get_elbow_position at four thetas and is_reachable_no_limits + get_joints), every row and not the
    120 of the scalar test: each arm as a uniform launch, and both arms interleaved in one launch with an arm byte per row."""
    torch = torch_mod
    g = np.load(os.path.join(golden_dir, "g5_helpers.npz"))
    solver, _, _ = make_symbolic(0.03)
    sets = {}
    for a, name in enumerate(("r_arm", "l_arm")):
        sets[name] = dict(arm=np.full(len(g[f"{name}_pos"]), a, dtype=np.uint8),
                          **{k: g[f"{name}_{k}"] for k in ("pos", "eul", "thetas", "elbow_at_theta", "nolimits_ok", "nolimits_joints", "nolimits_elbow")})
    both = {k: np.concatenate([sets["r_arm"][k], sets["l_arm"][k]]) for k in sets["r_arm"]}
    perm = np.random.default_rng(1).permutation(len(both["arm"]))
    sets["mixed"] = {k: v[perm] for k, v in both.items()}
    for name, s in sets.items():
        kind = {"r_arm": "r", "l_arm": "l", "mixed": "mixed"}[name]
        kw = arm_kwargs(kind, s["arm"], torch)
        n = len(s["arm"])
        p = soa(s["pos"], s["eul"], torch)
        st = solver.new_solver_state(n)
        rs = to_np(solver.reach_state(p, st, **kw))
        have = ~np.isnan(s["elbow_at_theta"][:, 0, 0])
        np.testing.assert_array_equal(rs["reachable"].astype(bool), have)
        for k in range(4):
            e = solver.elbow_from_state(st, T(s["thetas"][:, k], torch)).cpu().numpy()
            close(e[have], s["elbow_at_theta"][have, k], f"G5 {name} elbow at theta {k}")
        rs = to_np(solver.reach_state(p, st, no_limits=True, **kw))
        np.testing.assert_array_equal(rs["reachable"], s["nolimits_ok"])
        ok = s["nolimits_ok"].astype(bool)
        assert ok.mean() > 0.9 and (rs["interval"][ok] == (-np.pi, np.pi)).all()
        out = to_np(solver.joints_from_state(st, T(s["thetas"][:, 0], torch), **kw))
        joints_close(out["joints"][ok], s["nolimits_joints"][ok], f"G5 {name} no_limits joints")
        close(out["elbow"][ok], s["nolimits_elbow"][ok], f"G5 {name} no_limits elbow")


# ------------------------------------------------------------------------------------------ d. ragged sizes and bleed
@pytest.mark.parametrize("kind", ["r", "mixed"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_ragged_sizes_do_not_bleed(torch_mod, orc, n, kind):
    """Tail handling of the 256-thread blocks: any n; three guard rows behind the state tensor and behind every output keep
    their bits through reach_state, joints_from_state and elbow_from_state, and the n rows are the checker's."""
    torch = torch_mod
    rng = np.random.default_rng(300 + n)
    arm = (rng.uniform(size=n) < 0.5).astype(np.uint8) if kind == "mixed" else np.zeros(n, dtype=np.uint8)
    pos, eul = reachable_rich(100 + n, n, arm)
    solver, _, _ = make_symbolic(0.03)
    armT = T(arm, torch) if kind == "mixed" else None
    G = 3
    f64, u8 = torch.float64, torch.uint8
    st = torch.full((n + G, 32), 777.0, dtype=f64, device="cuda")
    st[:n] = 0.0
    interval = torch.full((n + G, 2), 777.0, dtype=f64, device="cuda")
    reachable = torch.full((n + G,), 77, dtype=u8, device="cuda")
    state = torch.full((n + G,), 77, dtype=u8, device="cuda")
    joints = torch.full((n + G, 7), 777.0, dtype=f64, device="cuda")
    elbow = torch.full((n + G, 3), 777.0, dtype=f64, device="cuda")
    elbow2 = torch.full((n + G, 3), 777.0, dtype=f64, device="cuda")
    rows = CheckerRows(arm)
    assert raw_reach(solver, n, soa(pos, eul, torch), st, arm=armT, interval=interval, reachable=reachable, state=state) == 0
    ref = rows.reach(pos, eul)
    check_reach(dict(reachable=reachable[:n].cpu().numpy(), state=state[:n].cpu().numpy(), interval=interval[:n].cpu().numpy()),
                ref, f"n {n} {kind}")
    m = np.flatnonzero(ref["reachable"])
    assert len(m) > 0 or n < 3
    theta = np.nan_to_num(ref["interval"][:, 0])
    thT = T(theta, torch)
    assert raw_joints(solver, n, st, thT, arm=armT, joints=joints, elbow=elbow) == 0
    assert raw_elbow(solver, n, st, thT, elbow2) == 0
    torch.cuda.synchronize()
    want = rows.joints(theta, rows=m)
    S = st.cpu().numpy()
    joints_close(joints[:n].cpu().numpy()[m], want["joints"][m], f"n {n} {kind} joints")
    close(elbow[:n].cpu().numpy()[m], want["elbow"][m], f"n {n} {kind} elbow")
    close(S[m, :16], rows.buf[m, :16], f"n {n} {kind} slots 0-15")
    np.testing.assert_array_equal(S[m, 19], want["projected"][m])
    close(elbow2[:n].cpu().numpy()[m], rows.elbow(theta, rows=m)[m], f"n {n} {kind} get_elbow_position")
    for t, v in ((st, 777.0), (interval, 777.0), (joints, 777.0), (elbow, 777.0), (elbow2, 777.0), (reachable, 77), (state, 77)):
        assert bool((t[n:] == v).all()), "a store ran past the end of the batch"


# ------------------------------------------------------------------------------------------ e. previous_joints rows
@pytest.mark.parametrize("tag,so", [("so003_", 0.03), ("so101_", -1.01)])
def test_previous_joints_rows_near_singular_catalogue(golden_dir, torch_mod, orc, tag, so):
    """G1 catalogue, r and l mixed, a different random previous_joints row per pose handed to rsik_joints_from_state on the
    device, against the checker's get_joints(theta, previous_joints) of that row.  The catalogue's stretched-arm rows are singular
    to rounding, not exactly (tests/test_gpu_previous_rows.py): they are compared through j2 + j6 modulo 2 pi."""
    torch = torch_mod
    g = np.load(os.path.join(golden_dir, "g1_catalogue.npz"))
    arm = g["arm"].astype(np.uint8)
    n = len(arm)
    prev = np.random.default_rng(6).uniform(-3.0, 3.0, size=(n, 7))
    solver, _, _ = make_symbolic(so)
    rows = CheckerRows(arm, so=so)
    st = solver.new_solver_state(n)
    rs = to_np(solver.reach_state(soa(g["pos"], g["eul"], torch), st, arm=T(arm, torch)))
    ref = rows.reach(g["pos"], g["eul"])
    check_reach(rs, ref, "catalogue")
    np.testing.assert_array_equal(rs["reachable"], g[tag + "reachable"])
    m = np.flatnonzero(ref["reachable"])
    theta = np.nan_to_num(ref["interval"][:, 0])
    out = to_np(solver.joints_from_state(st, T(theta, torch), arm=T(arm, torch), previous_joints=T(prev, torch)))
    want = rows.joints(theta, previous_joints=prev, rows=m)
    sing = np.abs(want["joints"][m, 3]) < 1e-12
    assert sing.sum() >= 3
    joints_close(out["joints"][m], want["joints"][m], f"catalogue {tag} joints")
    joints_close(out["joints"][m], g[tag + "joints"][m], f"catalogue {tag} joints against the reference")
    close(out["elbow"][m], want["elbow"][m], f"catalogue {tag} elbow")


def test_exact_singularity_reads_its_own_previous_joints_row(torch_mod, orc):
    """The state tensor is caller-owned, so this path can be handed a row no pose produces: an arm whose shoulder orientation
    offsets are zero (M_shoulder_torso is then Ry(pi/2) transposed, with exact zeros in its y row and column) and a circle of
    radius 0 centred straight beside the shoulder, at s + (0, -+u, 0).  The elbow is then (0, y, 0) exactly, q.x == 0 && q.z == 0
    holds bit for bit in the kernel (rsik_device.hpp "exact singularity: keep the previous pitch") and in the checker
    (symbolic_ik.py:751-753), and the shoulder pitch returned is previous_joints[0] OF THAT ROW — a different value in every row,
    r and l mixed in one launch, rows of an ordinary pose in between.  The wrist is put beside the elbow with the forearm bent, so
    the elbow-yaw branch (pw.y == 0 && pw.z == 0) does not fire: with the arm stretched along y the reference's Rz(-shoulder_roll)
    carries cos(pi/2) = 6e-17 into P_elbow_wrist and does not take its branch, while the kernel's rotation rows, built without
    evaluating the angle, give exact zeros and would — no row was found on which both take it."""
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
        SymbolicIK("r_arm", ik_parameters=prm, singularity_offset=so, solver=solver)
        SymbolicIK("l_arm", ik_parameters=prm, singularity_offset=so, solver=solver)
    arms = (orc.Arm("r_arm", so, ik_parameters=prm), orc.Arm("l_arm", so, ik_parameters=prm))
    n = 600
    rng = np.random.default_rng(12)
    arm = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    sy = np.where(arm == 1, 0.2, -0.2)
    side = np.where(arm == 1, 1.0, -1.0)
    u = f = 0.28
    special = np.arange(n) % 3 != 1
    # ordinary rows first: a reachable-rich batch through reach_state
    pos, eul = reachable_rich(13, n, arm)
    rows = CheckerRows(arm, arms=arms)
    st = solver.new_solver_state(n)
    armT = T(arm, torch)
    rs = to_np(solver.reach_state(soa(pos, eul, torch), st, arm=armT))
    ref = rows.reach(pos, eul)
    check_reach(rs, ref, "custom arm")
    ordinary = ~special & ref["reachable"].astype(bool)
    assert ordinary.sum() > 50
    # the hand-written rows: the same buffer for the kernel and for the checker's object
    S = st.cpu().numpy().copy()
    k = int(special.sum())
    hand = np.zeros((k, 32))
    ey = sy[special] + side[special] * u
    bend = rng.uniform(0.5, 2.5, size=k)                      # elbow pitch of the hand-written rows
    roll = rng.uniform(0.0, 2 * np.pi, size=k)
    wrist = np.stack([f * np.sin(bend) * np.cos(roll), ey + side[special] * f * np.cos(bend), f * np.sin(bend) * np.sin(roll)], axis=1)
    hand[:, 3:6] = rng.uniform(-1.0, 1.0, size=(k, 3))
    hand[:, 6:9] = wrist
    hand[:, 0:3] = wrist + rng.uniform(-0.05, 0.05, size=(k, 3)) + np.array([0.08, 0.0, 0.0])
    hand[:, 9] = 0.0
    hand[:, 10] = ey
    hand[:, 11] = 0.0
    hand[:, 12] = 0.0
    hand[:, 13:16] = np.stack([np.zeros(k), side[special], np.zeros(k)], axis=1)
    S[special] = hand
    rows.buf[special, :16] = hand[:, :16]
    st.copy_(T(S, torch))
    prev = rng.uniform(-3.0, 3.0, size=(n, 7))
    theta = np.where(special, rng.uniform(-np.pi, np.pi, size=n), np.nan_to_num(ref["interval"][:, 0]))
    m = np.flatnonzero(special | ordinary)
    out = to_np(solver.joints_from_state(st, T(theta, torch), arm=armT, previous_joints=T(prev, torch)))
    want = rows.joints(theta, previous_joints=prev, rows=m)
    same_bits(want["joints"][special, 0], prev[special, 0], "the checker takes its exact branch on the hand-written rows")
    same_bits(out["joints"][special, 0], prev[special, 0], "shoulder pitch = that row's previous_joints[0]")
    assert not np.any(out["joints"][ordinary, 0] == prev[ordinary, 0])
    joints_close(out["joints"][m], want["joints"][m], "hand-written and ordinary rows")
    close(out["elbow"][m], want["elbow"][m], "elbow")
    # and without previous_joints the branch returns 0
    out0 = to_np(solver.joints_from_state(T(S, torch), T(theta, torch), arm=armT))
    assert not out0["joints"][special, 0].any()


@pytest.mark.parametrize("kind", KINDS)
def test_no_previous_joints_is_zeros_and_null_outputs_leave_the_same_rows(torch_mod, kind):
    """previous_joints = NULL is a zero tensor bit for bit, and a launch with joints = NULL / elbow = NULL (the scalar drop-in's
    form) leaves the state rows a launch with outputs leaves."""
    torch = torch_mod
    n = 20000
    pos, eul, arm = workload(kind, 5000 + KINDS.index(kind), n)
    kw = arm_kwargs(kind, arm, torch)
    solver, _, _ = make_symbolic(0.03)
    st = solver.new_solver_state(n)
    rs = solver.reach_state(soa(pos, eul, torch), st, **kw)
    theta = torch.nan_to_num(rs["interval"][:, 0]).contiguous()
    base = st.clone()
    a = solver.joints_from_state(st, theta, **kw)
    st_b = base.clone()
    b = solver.joints_from_state(st_b, theta, previous_joints=torch.zeros((n, 7), dtype=torch.float64, device="cuda"), **kw)
    st_c = base.clone()
    assert raw_joints(solver, n, st_c, theta, arm=kw.get("arm"), arm_uniform=kw.get("arm_uniform", 0)) == 0
    torch.cuda.synchronize()
    Sa = st.cpu().numpy()
    for k in ("joints", "elbow"):
        same_bits(a[k].cpu().numpy(), b[k].cpu().numpy(), k)
    same_bits(Sa, st_b.cpu().numpy(), "state rows, previous_joints zeros")
    same_bits(Sa, st_c.cpu().numpy(), "state rows, joints = elbow = NULL")
    assert int(rs["reachable"].sum()) > 0.04 * n


# ------------------------------------------------------------------------------------------ f. one row is the batch's row
@pytest.mark.parametrize("arm_name", ["r_arm", "l_arm"])
def test_scalar_drop_in_is_the_batch_row(torch_mod, arm_name):
    """SymbolicIK.is_reachable -> get_joints x 2 -> get_elbow_position (one row in pinned host memory per call) gives bit for bit
    the numbers of the same rows of a batch launch (many rows in device memory)."""
    torch = torch_mod
    a = int(arm_name == "l_arm")
    n_rich, n_any = 300, 100
    arm = np.full(n_rich + n_any, a, dtype=np.uint8)
    p1, e1 = reachable_rich(61 + a, n_rich, arm[:n_rich])
    p2, e2, _ = state_workload(62 + a, n_any, arm=a)
    pos, eul = np.concatenate([p1, p2]), np.concatenate([e1, e2])
    n = len(pos)
    solver, r, l = make_symbolic(0.03)
    ik = l if a else r
    kw = dict(arm=None, arm_uniform=a)
    st = solver.new_solver_state(n)
    rs = to_np(solver.reach_state(soa(pos, eul, torch), st, **kw))
    S0 = st.cpu().numpy().copy()
    rng = np.random.default_rng(63)
    th1 = np.nan_to_num(rs["interval"][:, 0])
    th2 = rng.uniform(-np.pi, np.pi, size=n)
    th3 = rng.uniform(-np.pi, np.pi, size=n)
    o1 = to_np(solver.joints_from_state(st, T(th1, torch), **kw))
    S1 = st.cpu().numpy().copy()
    o2 = to_np(solver.joints_from_state(st, T(th2, torch), **kw))
    S2 = st.cpu().numpy().copy()
    e3 = solver.elbow_from_state(st, T(th3, torch)).cpu().numpy()
    from reachy2_symbolic_ik_amd import STATE_STRINGS

    solved = 0
    for i in range(n):
        ok, interval, fn, state = ik.is_reachable(np.array([pos[i], eul[i]]))
        assert ok == bool(rs["reachable"][i]) and state == STATE_STRINGS[rs["state"][i]], i
        if not ok:
            continue
        solved += 1
        same_bits(interval, rs["interval"][i], f"row {i} interval")
        same_bits(np.concatenate([ik.goal_pose.ravel(), ik.wrist_position, ik.intersection_circle[0], [ik.intersection_circle[1]],
                                  ik.intersection_circle[2]]), S0[i, :16], f"row {i} geometry after is_reachable")
        for th, o, S in ((th1, o1, S1), (th2, o2, S2)):
            j, e = fn(th[i])
            same_bits(j, o["joints"][i], f"row {i} joints")
            same_bits(e[:3], o["elbow"][i], f"row {i} elbow")
            assert len(e) == (3 if S[i, 19] else 4)
            same_bits(np.concatenate([ik.goal_pose[0], ik.wrist_position]), S[i, [0, 1, 2, 6, 7, 8]], f"row {i} goal and wrist")
        same_bits(ik.get_elbow_position(th3[i])[:3], e3[i], f"row {i} get_elbow_position")
    assert solved > 200 and S1[:, 19].sum() > 20


# ------------------------------------------------------------------------------------------ g. full size
def test_config2_full_size_mixed_arms_state_path_against_checker(torch_mod, orc):
    """Config 2's 1 Mi reachable poses with an arm byte per pose (l poses mirrored): reach_state + joints_from_state(interval[0])
    against the checker's batch at the bars of test_config2_full_size_against_checker, the projection flag of every row, and
    rsik_solve's flags and states on the same batch identical to reach_state's."""
    torch = torch_mod
    from bench import make_config2_poses

    n = 1 << 20
    pos, eul = make_config2_poses(n, seed=20250204)
    arm = (np.random.default_rng(99).uniform(size=n) < 0.5).astype(np.uint8)
    sgn = np.where(arm == 1, -1.0, 1.0)
    pos = pos * np.stack([np.ones(n), sgn, np.ones(n)], axis=1)
    eul = eul * np.stack([sgn, np.ones(n), sgn], axis=1)
    solver, _, _ = make_symbolic(0.03)
    p, armT = soa(pos, eul, torch), T(arm, torch)
    st = solver.new_solver_state(n)
    rs = solver.reach_state(p, st, arm=armT)
    out = solver.joints_from_state(st, rs["interval"][:, 0].contiguous(), arm=armT)
    fused = to_np(solver.solve(p, arm=armT))
    res = dict(to_np(rs), **to_np(out))
    flag = st[:, 19].cpu().numpy()
    ref = orc.solve_batch(orc.Arm("r_arm", 0.03), orc.Arm("l_arm", 0.03), pos, eul, arm_id=arm, nthreads=NTHREADS)
    np.testing.assert_array_equal(res["reachable"], ref["reachable"])
    np.testing.assert_array_equal(res["state"], ref["state"])
    np.testing.assert_array_equal(fused["reachable"], res["reachable"])
    np.testing.assert_array_equal(fused["state"], res["state"])
    assert res["reachable"].all() and 0.45 < arm.mean() < 0.55
    np.testing.assert_array_equal(flag, ref["projected"])
    assert 0.2 < flag.mean() < 0.6
    for k in ("joints", "interval", "elbow"):
        err = np.abs(res[k] - ref[k])
        print(f"{k}: state path max {np.max(err):.3e} q0.9999 {np.quantile(err, 0.9999):.3e}; "
              f"fused max {np.max(np.abs(fused[k] - ref[k])):.3e}")
        assert np.max(err) < NORTH_STAR_TOL and np.quantile(err, 0.9999) < 1e-9, k


def test_scale_digests_of_the_reference_through_the_state_path(golden_dir, torch_mod):
    """G14 — the reference itself, no checker in between, on the path its callers use: reach_state over config 2's generator
    before filtering (1 Mi poses per arm, every outcome) reproduces the SHA-256 of its reachable / state arrays, and with
    joints_from_state(interval[0]) every 64th row's interval and joints."""
    torch = torch_mod
    g = np.load(os.path.join(golden_dir, "g14_scale.npz"))
    solver, _, _ = make_symbolic(0.03)
    for a, arm in enumerate(("r_arm", "l_arm")):
        pos, eul = SC.config2_unfiltered(arm)
        assert SC.sha256(np.concatenate([pos, eul], axis=1)) == str(g[f"c2_{arm}_input_sha256"]), "the seeded inputs did not regenerate"
        st = solver.new_solver_state(len(pos))
        rs = solver.reach_state(soa(pos, eul, torch), st, arm_uniform=a)
        out = solver.joints_from_state(st, rs["interval"][:, 0].contiguous(), arm_uniform=a)
        res = dict(to_np(rs), joints=out["joints"].cpu().numpy())
        print(arm, "worst", _check_scale_set(g, f"c2_{arm}_", res, SC.N_CONFIG2))


# ------------------------------------------------------------------------------------------ h. checker-free property
@pytest.mark.parametrize("kind", KINDS)
def test_fk_of_the_first_get_joints_is_the_stored_goal(torch_mod, kind):
    """Only the state path exposes this: after reach_state and the FIRST joints_from_state, forward kinematics of the returned
    joints (tests/fk_numpy.py, on the host) gives back the goal the state row now holds — slots 0-2, slots 3-5 — on projected rows
    too, which test_fk_of_ik_is_identity_full_size has to avoid.  Position to that test's 1e-9 m, rotation to its 1e-8 (on the
    checker's own joints the position residual is <= 3.6e-16 m).  Rows whose elbow pitch sits on its clamp are left out (the
    clamped arm does not reach the goal).  Not a property of a second call after a projection: the reference keeps a stale
    circle there (0.1 - 0.6 m in the checker)."""
    torch = torch_mod
    n = 200000
    pos, eul, arm = workload(kind, 8000 + KINDS.index(kind), n)
    kw = arm_kwargs(kind, arm, torch)
    solver, _, _ = make_symbolic(0.03)
    st = solver.new_solver_state(n)
    rs = to_np(solver.reach_state(soa(pos, eul, torch), st, **kw))
    out = to_np(solver.joints_from_state(st, T(np.nan_to_num(rs["interval"][:, 0]), torch), **kw))
    S = st.cpu().numpy()
    ok = rs["reachable"].astype(bool)
    clamp = np.abs(np.abs(out["joints"][:, 3]) - ELBOW_LIMIT) < 1e-12
    keep = ok & ~clamp
    left_out = (ok & clamp).sum() / ok.sum()
    projected = S[keep, 19].mean()
    print(f"{kind}: reachable {ok.mean():.3f}, on the clamp {left_out:.3f}, projected among the kept {projected:.3f}")
    assert ok.mean() >= 0.04 and left_out <= 0.10 and projected >= 0.20
    worst_p = worst_r = 0.0
    for a in (0, 1):
        sel = keep & (arm == a)
        if not sel.any():
            continue
        p_fk, R_fk = forward_kinematics(out["joints"][sel], SHOULDER[a], SHOULDER_OFFSET_DEG[a], 0.28, 0.28, 0.10)
        worst_p = max(worst_p, float(np.max(np.abs(p_fk - S[sel, 0:3]))))
        worst_r = max(worst_r, float(np.max(np.abs(R_fk - euler_to_matrix(S[sel, 3:6])))))
    print(f"{kind}: FK residual position {worst_p:.3e} m, rotation {worst_r:.3e}")
    assert worst_p < 1e-9 and worst_r < 1e-8


# ------------------------------------------------------------------------------------------ i. rows that are not numbers
def test_rows_that_are_not_numbers_stay_in_their_rows(torch_mod):
    """include/rsik.h "Rows that are not numbers" in joints_state_kernel and elbow_state_kernel: a NaN theta, a NaN in one row's
    previous_joints and a NaN-poisoned state row change that row only; every other row — outputs and state — is bit for bit that
    of the clean launch."""
    torch = torch_mod
    n = 3000
    arm = (np.random.default_rng(70).uniform(size=n) < 0.5).astype(np.uint8)
    pos, eul = reachable_rich(71, n, arm)
    solver, _, _ = make_symbolic(0.03)
    armT = T(arm, torch)
    base = solver.new_solver_state(n)
    rs = solver.reach_state(soa(pos, eul, torch), base, arm=armT)
    rng = np.random.default_rng(72)
    theta = torch.nan_to_num(rs["interval"][:, 0]).contiguous()
    prev = T(rng.uniform(-2, 2, size=(n, 7)), torch)
    st = base.clone()
    clean = {k: v.clone() for k, v in solver.joints_from_state(st, theta, arm=armT, previous_joints=prev).items()}
    clean_e = solver.elbow_from_state(base, theta).clone()
    bad_rows = rng.choice(n, size=18, replace=False)
    th_rows, prev_rows, st_rows = bad_rows[:6], bad_rows[6:12], bad_rows[12:]
    theta2, prev2, base2 = theta.clone(), prev.clone(), base.clone()
    for q, row in enumerate(th_rows):
        theta2[row] = (float("nan"), float("inf"), float("-inf"))[q % 3]
    for q, row in enumerate(prev_rows):
        prev2[row, q] = float("nan")
    for q, row in enumerate(st_rows):
        base2[row, (0, 4, 7, 10, 12, 14)[q]] = float("nan")
    st2 = base2.clone()
    got = solver.joints_from_state(st2, theta2, arm=armT, previous_joints=prev2)
    got_e = solver.elbow_from_state(base2, theta2)
    torch.cuda.synchronize()
    keep = _rows_except(torch, n, bad_rows)
    for k in clean:
        assert _bits_equal(torch, got[k][keep], clean[k][keep]), k
    assert _bits_equal(torch, st2[keep], st[keep]) and _bits_equal(torch, got_e[keep], clean_e[keep])
    # a theta that is not a number: everything that depends on it is NaN.  (The elbow pitch goes through the clamp, written
    # fmin(fmax(.)) in the kernel: a NaN comes out as NaN or as the limit, "what comparisons that are all false select".)
    b = torch.as_tensor(th_rows, device="cuda")
    assert torch.isnan(got["joints"][b][:, [0, 1, 2, 4, 5, 6]]).all() and torch.isnan(got["elbow"][b]).all() and torch.isnan(got_e[b]).all()
    j3 = got["joints"][b][:, 3]
    print("elbow pitch of the rows whose theta is not a number:", j3.cpu().numpy())
    assert (torch.isnan(j3) | ((j3.abs() - float(ELBOW_LIMIT)).abs() < 1e-12)).all()
    # previous_joints is read only at an exact singularity: those rows keep their bits as well
    b = torch.as_tensor(prev_rows, device="cuda")
    assert _bits_equal(torch, got["joints"][b], clean["joints"][b])
    b = torch.as_tensor(st_rows, device="cuda")
    assert torch.isnan(got["joints"][b]).any(dim=1).all()
    assert _bits_equal(torch, st2[:, 20:24], base2[:, 20:24])


def test_empty_batches_and_null_pointers(torch_mod):
    """n = 0 on joints_from_state / elbow_from_state returns empty tensors; a required pointer that is NULL gives RSIK_E_INVALID
    with a message and launches nothing."""
    torch = torch_mod
    from reachy2_symbolic_ik_amd import _abi

    solver, _, _ = make_symbolic(0.03)
    f64 = torch.float64
    z = torch.zeros((0,), dtype=f64, device="cuda")
    out = solver.joints_from_state(solver.new_solver_state(0), z)
    assert out["joints"].shape == (0, 7) and out["elbow"].shape == (0, 3)
    out = solver.joints_from_state(solver.new_solver_state(0), z, arm=torch.zeros((0,), dtype=torch.uint8, device="cuda"),
                                   previous_joints=torch.zeros((0, 7), dtype=f64, device="cuda"))
    assert out["joints"].shape == (0, 7)
    assert solver.elbow_from_state(solver.new_solver_state(0), z).shape == (0, 3)
    assert raw_joints(solver, 0, None, None) == _abi.RSIK_OK and raw_elbow(solver, 0, None, None, None) == _abi.RSIK_OK
    n = 300
    arm = np.zeros(n, dtype=np.uint8)
    pos, eul = reachable_rich(81, n, arm)
    st = solver.new_solver_state(n)
    p = soa(pos, eul, torch)
    rs = solver.reach_state(p, st)
    theta = torch.nan_to_num(rs["interval"][:, 0]).contiguous()
    elbow = torch.full((n, 3), 777.0, dtype=f64, device="cuda")
    before = st.clone()
    for call, who in ((lambda: raw_joints(solver, n, None, theta), "rsik_joints_from_state"),
                      (lambda: raw_joints(solver, n, st, None), "rsik_joints_from_state"),
                      (lambda: raw_joints(solver, -1, st, theta), "rsik_joints_from_state"),
                      (lambda: raw_elbow(solver, n, None, theta, elbow), "rsik_elbow_from_state"),
                      (lambda: raw_elbow(solver, n, st, None, elbow), "rsik_elbow_from_state"),
                      (lambda: raw_elbow(solver, n, st, theta, None), "rsik_elbow_from_state"),
                      (lambda: raw_elbow(solver, -1, st, theta, elbow), "rsik_elbow_from_state"),
                      (lambda: raw_reach(solver, n, p, None), "rsik_reach_state"),
                      (lambda: raw_reach(solver, n, None, st), "rsik_reach_state")):
        rc = call()
        assert rc == _abi.RSIK_E_INVALID, (who, rc)
        assert who in last_error(solver), (who, last_error(solver))
    torch.cuda.synchronize()
    assert torch.equal(st.view(torch.int64), before.view(torch.int64)) and bool((elbow == 777.0).all())


# ------------------------------------------------------------------------------------------ j. mixed arms in the FK kernels
def test_fk_kernels_with_an_arm_byte_per_row(torch_mod):
    """fk_kernel<true>: forward_kinematics and fk_residual (pose form and matrix form) with an arm tensor are, row by row and bit
    for bit, the two uniform launches; forward_kinematics stays within the 1e-14 of
    test_device_forward_kinematics_matches_numpy_chain against tests/fk_numpy.py."""
    torch = torch_mod
    n = 5000 + 37
    rng = np.random.default_rng(90)
    arm = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    waves = arm[: n - n % 64].reshape(-1, 64).sum(axis=1)
    assert ((waves > 0) & (waves < 64)).all()
    j = rng.uniform(-np.pi, np.pi, size=(n, 7))
    solver, _, _ = make_symbolic(0.03)
    jT, armT = T(j, torch), T(arm, torch)
    pm, Rm = (t.cpu().numpy() for t in solver.forward_kinematics(jT, arm=armT))
    uni = [tuple(t.cpu().numpy() for t in solver.forward_kinematics(jT, arm_uniform=a)) for a in (0, 1)]
    is_l = arm == 1
    same_bits(pm, np.where(is_l[:, None], uni[1][0], uni[0][0]), "position")
    same_bits(Rm, np.where(is_l[:, None, None], uni[1][1], uni[0][1]), "rotation")
    assert np.abs(uni[0][0] - uni[1][0]).min() > 1e-6   # the two arms do differ
    for a in (0, 1):
        p_ref, R_ref = forward_kinematics(j[arm == a], SHOULDER[a], SHOULDER_OFFSET_DEG[a], 0.28, 0.28, 0.10)
        close(pm[arm == a], p_ref, f"FK position arm {a}", tol=1e-14)
        close(Rm[arm == a], R_ref, f"FK rotation arm {a}", tol=1e-14)
    pos, eul, _ = state_workload(91, n)
    goal6 = soa(pos, eul, torch)
    goal12 = T(np.concatenate([euler_to_matrix(eul).reshape(n, 9).T, pos.T], axis=0), torch)
    for goal in (goal6, goal12):
        em = solver.fk_residual(goal, jT, arm=armT).cpu().numpy()
        eu = [solver.fk_residual(goal, jT, arm_uniform=a).cpu().numpy() for a in (0, 1)]
        same_bits(em, np.where(is_l[:, None], eu[1], eu[0]), f"fk_residual, {goal.shape[0]} columns")
        assert np.isfinite(em).all() and np.abs(eu[0] - eu[1]).max() > 1e-3
