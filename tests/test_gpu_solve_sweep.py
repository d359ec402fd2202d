"""GPU tests (-m gpu, MI355X) of rsik_solve_sweep (csrc/rsik_kernel_sweep.hpp): K elbow angles per pose from one launch.

The entry point is defined against what exists: sample (k, i) is, bit for bit, rsik_solve's (rsik_solve_rows') row for pose i at
that sample's theta, and the samples do not depend on each other or on their order.  So the first reference is the library's own
rsik_solve, column by column (bits); the second the CPU checker on the tiled batch (tests/sweep_workload.expected_tiled, pinned on
the checker alone by tests/test_solve_sweep_abi.py): reachable / state / projected bit-exact, numbers within TOL = 1e-9, rows whose
elbow pitch is 0 compared through j2 + j6 modulo 2 pi (joints_close).  Sizes are the smallest at which the kernel can go wrong:
several 256-pose blocks with a ragged last block and a ragged last wave, r and l alternating inside every wave.
"""
import numpy as np
import pytest

from checker_support import ELBOW_LIMIT, reachable_rich
from compare import bits, close, joints_close, same_bits
from gpu_support import KINDS, T, abi, arm_kwargs, cols, last_error, make_symbolic, orc, ptr, raw_call, soa, to_np, torch_mod  # noqa: F401
from sampling_support import PER_POSE, check_against_solve, solve_columns
from sweep_workload import columns, expected_tiled, fraction_theta, sweep_poses, sweep_thetas

pytestmark = pytest.mark.gpu



def raw_sweep(solver, n, p, k, policy, thetas, per_pose, arm=None, arm_uniform=0, prev=None, joints=None, elbow=None,
              projected=None, theta=None, interval=None, reachable=None, state=None):
    """rsik_solve_sweep on the caller's own buffers: returns the ABI's code."""
    return raw_call(solver, "rsik_solve_sweep", n, cols(p, 6), ptr(arm), int(arm_uniform), int(k), int(policy), ptr(thetas), int(per_pose),
                    ptr(prev), ptr(joints), ptr(elbow), ptr(projected), ptr(theta), ptr(interval), ptr(reachable), ptr(state))


# ------------------------------------------------------------------------------------------ 1. each sample is rsik_solve's row
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [1, 3, 8])
def test_each_sample_is_the_row_of_rsik_solve(torch_mod, kind, k):
    """n = 1000 (three full blocks, a ragged last one with a ragged last wave), both policies, both forms of theta_in, with and
    without a random previous_joints row per pose, under both values of RSIK_OPT_NO_MIRROR and of RSIK_OPT_NO_TIPZ: joints, elbow,
    interval, reachable and state of sample k have the bits of rsik_solve(policy, theta_in = column k) (rsik_solve_rows with
    previous_joints); theta has the bits of NumPy's a + u * (b - a) (fraction) or of the input (explicit), NaN where the pose is
    not reachable; projected is 0 there."""
    torch = torch_mod
    _abi = abi()
    n = 1000
    pos, eul, arm = sweep_poses(kind, 500 + k, n)
    p = soa(pos, eul, torch)
    kw = arm_kwargs(kind, arm, torch)
    solver, _, _ = make_symbolic(0.03)
    prev_rows = T(np.random.default_rng(40 + k).uniform(-2, 2, size=(n, 7)), torch)
    for no_mirror in (0, 1):
        for no_tipz in (0, 1):
            solver.set_option(_abi.OPT_NO_MIRROR, no_mirror)
            solver.set_option(_abi.OPT_NO_TIPZ, no_tipz)
            for policy in ("fraction", "explicit"):
                for per_pose in (False, True):
                    thetas = sweep_thetas(policy, per_pose, k, n, 600 + k)
                    th = columns(thetas, n)
                    if policy == "fraction":
                        assert (th[0] == 0.0).all() and (k == 1 or (th[-1] == 1.0).all())
                    else:
                        assert np.abs(th).max() > np.pi
                    for prev in (None, prev_rows):
                        what = f"{kind} K {k} {policy} per_pose {per_pose} prev {prev is not None} no_mirror {no_mirror} no_tipz {no_tipz}"
                        got = to_np(solver.solve_sweep(p, T(thetas, torch), policy=policy, previous_joints=prev, **kw))
                        ref = solve_columns(solver, p, policy, th, torch, prev=prev, **kw)
                        check_against_solve(got, ref, what)
                        ok = ref["reachable"].astype(bool)
                        assert ok[0::2].mean() >= 0.04 and ok[1::2].mean() > 0.5, what
                        want_theta = np.stack([fraction_theta(ref["interval"], u) for u in th]) if policy == "fraction" else th.copy()
                        want_theta[:, ~ok] = np.nan
                        assert np.array_equal(np.isnan(got["theta"]), np.isnan(want_theta)), what
                        same_bits(got["theta"][:, ok], want_theta[:, ok], what + " theta")
                        assert got["projected"].dtype == np.uint8 and got["projected"].max() <= 1
                        assert (got["projected"][:, ~ok] == 0).all(), what
                        assert np.isnan(got["joints"][:, ~ok]).all() and np.isnan(got["elbow"][:, ~ok]).all(), what


# ------------------------------------------------------------------------------------------ 2. against the checker
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [1, 3, 8])
def test_sweep_against_the_checker(torch_mod, orc, kind, k):
    """The shapes of test 1 against orc.solve_batch on the tiled batch: reachable / state / projected bit-exact, joints, elbow and
    interval within TOL.  The inputs are checked on the checker before anything is launched: among the reachable samples at
    least 5 % project and at least 5 % do not, and (K > 1) at least one pose has both kinds among its own samples."""
    torch = torch_mod
    n = 1000
    pos, eul, arm = sweep_poses(kind, 500 + k, n)
    arms = (orc.Arm("r_arm", 0.03), orc.Arm("l_arm", 0.03))
    cases = []
    for policy in ("fraction", "explicit"):
        for per_pose in (False, True):
            thetas = sweep_thetas(policy, per_pose, k, n, 600 + k)
            ref = expected_tiled(orc, arms, pos, eul, arm, policy, thetas, nthreads=4)
            ok = ref["reachable"].astype(bool)
            pr = ref["projected"][:, ok]
            both = int(((pr.max(axis=0) == 1) & (pr.min(axis=0) == 0)).sum())
            print(f"{kind} K {k} {policy} per_pose {per_pose}: reachable {ok.mean():.3f}, projected {pr.mean():.3f} of the reachable "
                  f"samples, {both} poses with both kinds")
            assert 0.05 <= pr.mean() <= 0.95 and (k == 1 or both >= 1)
            cases.append((policy, per_pose, thetas, ref))
    p = soa(pos, eul, torch)
    solver, _, _ = make_symbolic(0.03)
    for policy, per_pose, thetas, ref in cases:
        what = f"{kind} K {k} {policy} per_pose {per_pose}"
        got = to_np(solver.solve_sweep(p, T(thetas, torch), policy=policy, **arm_kwargs(kind, arm, torch)))
        for key in ("reachable", "state", "projected"):
            np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{what} {key}")
        ok = ref["reachable"].astype(bool)
        close(got["interval"], ref["interval"], what + " interval")
        close(got["theta"], ref["theta"], what + " theta")
        for q in range(k):
            assert np.isnan(got["joints"][q][~ok]).all() and np.isnan(got["elbow"][q][~ok]).all()
            joints_close(got["joints"][q][ok], ref["joints"][q][ok], f"{what} sample {q} joints")
            close(got["elbow"][q][ok], ref["elbow"][q][ok], f"{what} sample {q} elbow")


# ------------------------------------------------------------------------------------------ 3. order does not matter
def test_sample_order_does_not_matter(torch_mod, orc):
    """n = 300, K = 4, per-pose explicit theta chosen with the checker so that sample 0 of at least 20 poses projects and a later
    sample of the same pose does not: the sweep over the samples in reverse order returns the reversed arrays, bit for bit.  A
    wrist carried over from a projected sample into the next one would show here."""
    torch = torch_mod
    n, k = 300, 4
    arm = np.zeros(n, dtype=np.uint8)
    pos, eul = reachable_rich(31, n, arm)
    arms = (orc.Arm("r_arm", 0.03), orc.Arm("l_arm", 0.03))
    grid = np.linspace(0.0, 1.0, 9)
    probe = expected_tiled(orc, arms, pos, eul, arm, "fraction", grid)
    ok = probe["reachable"].astype(bool)
    thetas = np.random.default_rng(32).uniform(-np.pi, np.pi, size=(k, n))
    chosen = 0
    for i in np.flatnonzero(ok):
        yes, no = np.flatnonzero(probe["projected"][:, i] == 1), np.flatnonzero(probe["projected"][:, i] == 0)
        if len(yes) and len(no):
            thetas[0, i] = probe["theta"][yes[0], i]
            thetas[1 + chosen % (k - 1), i] = probe["theta"][no[0], i]
            chosen += 1
    ref = expected_tiled(orc, arms, pos, eul, arm, "explicit", thetas)
    mixed = (ref["projected"][0] == 1) & (ref["projected"][1:].min(axis=0) == 0) & ok
    print(f"{int(mixed.sum())} poses whose sample 0 projects and a later sample does not")
    assert mixed.sum() >= 20
    p = soa(pos, eul, torch)
    solver, _, _ = make_symbolic(0.03)
    fwd = to_np(solver.solve_sweep(p, T(thetas, torch), policy="explicit"))
    rev = to_np(solver.solve_sweep(p, T(thetas[::-1], torch), policy="explicit"))
    np.testing.assert_array_equal(fwd["projected"], ref["projected"])
    for key in ("joints", "elbow", "theta"):
        same_bits(rev[key], fwd[key][::-1], key)
    np.testing.assert_array_equal(rev["projected"], fwd["projected"][::-1])
    for key in PER_POSE:
        np.testing.assert_array_equal(bits(rev[key]) if rev[key].dtype == np.float64 else rev[key],
                                      bits(fwd[key]) if fwd[key].dtype == np.float64 else fwd[key])


# ------------------------------------------------------------------------------------------ 4. ragged sizes and bleed
@pytest.mark.parametrize("kind", ["r", "mixed"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257])
def test_ragged_sizes_do_not_bleed(torch_mod, n, kind):
    """K = 3; three guard rows behind every output keep their sentinel, and all K slabs of every output are rsik_solve's: a tail
    store of slab k that ran on would land in the head of slab k + 1."""
    torch = torch_mod
    _abi = abi()
    k, G = 3, 3
    rng = np.random.default_rng(300 + n)
    arm = (rng.uniform(size=n) < 0.5).astype(np.uint8) if kind == "mixed" else np.zeros(n, dtype=np.uint8)
    pos, eul = reachable_rich(100 + n, n, arm)
    p = soa(pos, eul, torch)
    kw = arm_kwargs(kind, arm, torch)
    solver, _, _ = make_symbolic(0.03)
    thetas = sweep_thetas("fraction", True, k, n, 700 + n)
    ref = solve_columns(solver, p, "fraction", thetas, torch, **kw)
    f64, u8 = torch.float64, torch.uint8

    def guarded(rows, width, dtype, fill):
        t = torch.full((rows + G, width) if width else (rows + G,), fill, dtype=dtype, device="cuda")
        return t

    joints, elbow = guarded(k * n, 7, f64, 777.0), guarded(k * n, 3, f64, 777.0)
    projected, theta = guarded(k * n, 0, u8, 77), guarded(k * n, 0, f64, 777.0)
    interval, reachable, state = guarded(n, 2, f64, 777.0), guarded(n, 0, u8, 77), guarded(n, 0, u8, 77)
    rc = raw_sweep(solver, n, p, k, _abi.THETA_FRACTION, T(thetas, torch), 1, joints=joints, elbow=elbow, projected=projected,
                   theta=theta, interval=interval, reachable=reachable, state=state, **kw)
    assert rc == _abi.RSIK_OK, last_error(solver)
    torch.cuda.synchronize()
    for t, rows, v in ((joints, k * n, 777.0), (elbow, k * n, 777.0), (projected, k * n, 77), (theta, k * n, 777.0),
                       (interval, n, 777.0), (reachable, n, 77), (state, n, 77)):
        assert bool((t[rows:] == v).all()), "a store ran past the end of its array"
    got = dict(joints=joints[:k * n].reshape(k, n, 7), elbow=elbow[:k * n].reshape(k, n, 3), interval=interval[:n],
               reachable=reachable[:n], state=state[:n])
    check_against_solve(to_np(got), ref, f"n {n} {kind}")
    ok = ref["reachable"].astype(bool)
    assert ok.any() or n < 3
    th = theta[:k * n].reshape(k, n).cpu().numpy()
    want = np.stack([fraction_theta(ref["interval"], u) for u in thetas])
    same_bits(th[:, ok], want[:, ok], "theta")
    assert np.isnan(th[:, ~ok]).all() and (projected[:k * n].reshape(k, n).cpu().numpy()[:, ~ok] == 0).all()


# ------------------------------------------------------------------------------------------ 5. rows that are not numbers
def test_rows_that_are_not_numbers_stay_where_they_are(torch_mod):
    """include/rsik.h "Rows that are not numbers", n = 3000, K = 4.  A NaN / +inf / -inf in one column of 12 poses: those poses report
    RSIK_STATE_INVALID_INPUT, reachable 0, NaN in every sample, projected 0.  A NaN in one entry of a per-pose theta array: only
    that (sample, pose) changes; one in a shared grid: only that sample.  Everything else has the bits of the clean launch."""
    torch = torch_mod
    _abi = abi()
    n, k = 3000, 4
    rng = np.random.default_rng(90)
    arm = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    pos, eul = reachable_rich(91, n, arm)
    p = soa(pos, eul, torch)
    armT = T(arm, torch)
    solver, _, _ = make_symbolic(0.03)
    per_pose = sweep_thetas("fraction", True, k, n, 92)
    shared = sweep_thetas("fraction", False, k, n, 93)

    def run(poses, thetas):
        res = solver.solve_sweep(poses, T(thetas, torch), policy="fraction", arm=armT)
        torch.cuda.synchronize()
        return to_np(res)

    def unchanged(got, clean, sample_mask):
        """sample_mask [k, n]: True where the (sample, pose) must keep the clean launch's bits"""
        for key in ("joints", "elbow", "theta"):
            assert np.array_equal(bits(got[key])[sample_mask], bits(clean[key])[sample_mask]), key
        assert np.array_equal(got["projected"][sample_mask], clean["projected"][sample_mask])

    clean = run(p, per_pose)
    ok = clean["reachable"].astype(bool)
    # a. poses that are not numbers
    bad = rng.choice(n, size=12, replace=False)
    p2 = p.clone()
    for q, row in enumerate(bad):
        p2[q % 6, row] = (float("nan"), float("inf"), float("-inf"))[q % 3]
    got = run(p2, per_pose)
    keep = np.ones((k, n), dtype=bool)
    keep[:, bad] = False
    unchanged(got, clean, keep)
    for key in PER_POSE:
        assert np.array_equal(bits(got[key][keep[0]]) if got[key].dtype == np.float64 else got[key][keep[0]],
                              bits(clean[key][keep[0]]) if got[key].dtype == np.float64 else clean[key][keep[0]]), key
    assert (got["state"][bad] == _abi.STATE_INVALID_INPUT).all() and (got["reachable"][bad] == 0).all()
    assert np.isnan(got["interval"][bad]).all() and np.isnan(got["joints"][:, bad]).all() and np.isnan(got["elbow"][:, bad]).all()
    assert np.isnan(got["theta"][:, bad]).all() and (got["projected"][:, bad] == 0).all()

    def poisoned(j, e):
        """joints / elbow rows of samples whose theta is a NaN: NaN, except that the elbow pitch goes through the clamp, written
        fmin(fmax(.)): a NaN comes out as NaN or as the limit (tests/test_gpu_solver_state.py, section i)"""
        assert np.isnan(j[:, [0, 1, 2, 4, 5, 6]]).all() and np.isnan(e).all()
        j3 = j[:, 3]
        print("elbow pitch of the samples whose theta is not a number:", j3)
        assert (np.isnan(j3) | (np.abs(np.abs(j3) - ELBOW_LIMIT) < 1e-12)).all()

    # b. one entry of a per-pose theta array
    row = int(np.flatnonzero(ok)[len(np.flatnonzero(ok)) // 2])
    th2 = per_pose.copy()
    th2[2, row] = np.nan
    got = run(p, th2)
    keep = np.ones((k, n), dtype=bool)
    keep[2, row] = False
    unchanged(got, clean, keep)
    for key in PER_POSE:
        np.testing.assert_array_equal(got[key], clean[key])
    poisoned(got["joints"][2, row][None], got["elbow"][2, row][None])
    assert np.isnan(got["theta"][2, row])
    # c. one entry of a shared grid
    clean_s = run(p, shared)
    sh2 = shared.copy()
    sh2[1] = np.nan
    got = run(p, sh2)
    keep = np.ones((k, n), dtype=bool)
    keep[1] = False
    unchanged(got, clean_s, keep)
    for key in PER_POSE:
        np.testing.assert_array_equal(got[key], clean_s[key])
    poisoned(got["joints"][1][ok], got["elbow"][1][ok])
    assert np.isnan(got["theta"][1]).all() and np.isnan(got["joints"][1][~ok]).all()


# ------------------------------------------------------------------------------------------ 6. arguments
def test_arguments(torch_mod):
    """What the entry point refuses (with the whole text of rsik_last_error, also where a call has two faults; nothing written),
    n = 0, and optional outputs left out."""
    torch = torch_mod
    _abi = abi()
    from reachy2_symbolic_ik_amd import HipSolver

    n, k = 300, 3
    arm = np.zeros(n, dtype=np.uint8)
    pos, eul = reachable_rich(81, n, arm)
    p = soa(pos, eul, torch)
    solver, _, _ = make_symbolic(0.03)
    f64, u8 = torch.float64, torch.uint8
    th = T(np.linspace(0.0, 1.0, k), torch)
    big = T(np.linspace(0.0, 1.0, 4097), torch)
    outs = dict(joints=torch.full((k, n, 7), 777.0, dtype=f64, device="cuda"), elbow=torch.full((k, n, 3), 777.0, dtype=f64, device="cuda"),
                projected=torch.full((k, n), 77, dtype=u8, device="cuda"), theta=torch.full((k, n), 777.0, dtype=f64, device="cuda"),
                interval=torch.full((n, 2), 777.0, dtype=f64, device="cuda"), reachable=torch.full((n,), 77, dtype=u8, device="cuda"),
                state=torch.full((n,), 77, dtype=u8, device="cuda"))
    FR = _abi.THETA_FRACTION
    no_joints = {key: v for key, v in outs.items() if key != "joints"}
    calls = {
        "n_theta 0": (lambda: raw_sweep(solver, n, p, 0, FR, th, 0, **outs), "n_theta must be in [1, 4096]"),
        "n_theta 4097": (lambda: raw_sweep(solver, n, p, 4097, FR, big, 0, **outs), "n_theta must be in [1, 4096]"),
        "interval0": (lambda: raw_sweep(solver, n, p, k, _abi.THETA_INTERVAL0, th, 0, **outs), "theta_policy must be RSIK_THETA_EXPLICIT or RSIK_THETA_FRACTION"),
        "none": (lambda: raw_sweep(solver, n, p, k, _abi.THETA_NONE, th, 0, **outs), "theta_policy must be RSIK_THETA_EXPLICIT or RSIK_THETA_FRACTION"),
        "theta_in NULL": (lambda: raw_sweep(solver, n, p, k, FR, None, 0, **outs), "theta_in is NULL"),
        "joints NULL": (lambda: raw_sweep(solver, n, p, k, FR, th, 0, **no_joints), "joints is NULL"),
        "pose_soa NULL": (lambda: raw_sweep(solver, n, None, k, FR, th, 0, **outs), "pose_soa is NULL"),
        "n -1": (lambda: raw_sweep(solver, -1, p, k, FR, th, 0, **outs), "n < 0"),
        # two faults in one call: the one the entry point tests first is the one it reports
        "n_theta 0 and interval0": (lambda: raw_sweep(solver, n, p, 0, _abi.THETA_INTERVAL0, th, 0, **outs), "n_theta must be in [1, 4096]"),
        "theta_in NULL and pose_soa NULL": (lambda: raw_sweep(solver, n, None, k, FR, None, 0, **outs), "pose_soa is NULL"),
    }
    for name, (call, text) in calls.items():
        rc = call()
        assert rc == _abi.RSIK_E_INVALID, (name, rc)
        assert last_error(solver) == "rsik_solve_sweep: " + text, (name, last_error(solver))
    torch.cuda.synchronize()
    for key, t in outs.items():
        assert bool((t == (777.0 if t.dtype == f64 else 77)).all()), key
    bare = HipSolver(0)  # no arm uploaded
    assert raw_sweep(bare, n, p, k, FR, th, 0, **outs) == _abi.RSIK_E_NOT_SET
    assert last_error(bare) == "rsik_solve_sweep: constants of the requested arm were not uploaded"
    assert raw_sweep(bare, n, p, k, FR, th, 0, arm=T(arm, torch), **outs) == _abi.RSIK_E_NOT_SET
    assert last_error(bare) == "rsik_solve_sweep: per-pose arm ids need both arms' constants (rsik_set_arm)"
    bare.close()
    # n = 0
    assert raw_sweep(solver, 0, None, k, FR, th, 0) == _abi.RSIK_OK
    empty = solver.solve_sweep(torch.zeros((6, 0), dtype=f64, device="cuda"), th)
    assert empty["joints"].shape == (k, 0, 7) and empty["elbow"].shape == (k, 0, 3) and empty["projected"].shape == (k, 0)
    assert empty["theta"].shape == (k, 0) and empty["interval"].shape == (0, 2) and empty["state"].shape == (0,)
    # every optional output left out: the joints of a full launch
    full = solver.solve_sweep(p, th)
    only = torch.full((k, n, 7), 777.0, dtype=f64, device="cuda")
    assert raw_sweep(solver, n, p, k, FR, th, 0, joints=only) == _abi.RSIK_OK, last_error(solver)
    torch.cuda.synchronize()
    same_bits(only.cpu().numpy(), full["joints"].cpu().numpy(), "joints alone")
    no_elbow = solver.solve_sweep(p, th, want_elbow=False)
    assert "elbow" not in no_elbow
    same_bits(no_elbow["joints"].cpu().numpy(), full["joints"].cpu().numpy(), "want_elbow=False")


# ------------------------------------------------------------------------------------------ 7. Python surface
def test_python_surface(torch_mod):
    """SymbolicIK.sweep_batch(poses, n_theta=5) and DualArmIK.sweep_batch return the documented shapes and the bits of
    HipSolver.solve_sweep; fractions 0 and 1 of a reachable pose whose interval does not wrap return interval[0] (bit for bit) and
    interval[1] (to the two roundings of the fraction formula)."""
    torch = torch_mod
    from reachy2_symbolic_ik_amd import DualArmIK

    n, k = 500, 5
    arm = (np.random.default_rng(60).uniform(size=n) < 0.5).astype(np.uint8)
    pos_r, eul_r = reachable_rich(61, n, np.zeros(n, dtype=np.uint8))
    solver, r, _ = make_symbolic(0.03)
    poses = np.stack([pos_r, eul_r], axis=1)  # [n,2,3]
    res = to_np(r.sweep_batch(poses, n_theta=k))
    assert res["joints"].shape == (k, n, 7) and res["elbow"].shape == (k, n, 3) and res["projected"].shape == (k, n)
    assert res["theta"].shape == (k, n) and res["interval"].shape == (n, 2) and res["reachable"].shape == (n,) and res["state"].shape == (n,)
    grid = torch.linspace(0.0, 1.0, k, dtype=torch.float64)
    raw = to_np(solver.solve_sweep(soa(pos_r, eul_r, torch), grid, policy="fraction", arm_uniform=0))
    for key in res:
        assert np.array_equal(res[key].view(np.uint8), raw[key].view(np.uint8)), key
    ok = res["reachable"].astype(bool) & (res["interval"][:, 0] <= res["interval"][:, 1])
    assert ok.sum() > 50
    same_bits(res["theta"][0][ok], res["interval"][ok, 0], "fraction 0 is interval[0]")
    # fraction 1 is i0 + 1.0 * (i1 - i0) with the kernel's own rounding (include/rsik.h): two roundings of numbers below 2 pi, so
    # within 2 ulp(2 pi) = 1.8e-15 of interval[1] (on the checker 102 of 240 such rows differ from it, by 4.4e-16 at the most)
    same_bits(res["theta"][-1][ok], fraction_theta(res["interval"][ok], 1.0), "fraction 1")
    assert np.abs(res["theta"][-1][ok] - res["interval"][ok, 1]).max() <= 1.8e-15
    per_pose_view = r.sweep_batch(poses, n_theta=k)["joints"].permute(1, 0, 2)
    assert tuple(per_pose_view.shape) == (n, k, 7)
    # explicit angles, one column per pose, with a previous_joints row per pose
    th = sweep_thetas("explicit", True, 2, n, 62)
    prev = np.random.default_rng(63).uniform(-2, 2, size=(n, 7))
    a = to_np(r.sweep_batch(poses, thetas=th, policy="explicit", previous_joints=prev))
    b = to_np(solver.solve_sweep(soa(pos_r, eul_r, torch), T(th, torch), policy="explicit", previous_joints=T(prev, torch)))
    for key in a:
        assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key
    # both arms
    pos, eul = reachable_rich(61, n, arm)
    dual = DualArmIK(solver=solver, singularity_offset=0.03)
    d = to_np(dual.sweep_batch(arm, np.stack([pos, eul], axis=1), n_theta=k))
    raw = to_np(solver.solve_sweep(soa(pos, eul, torch), grid, arm=T(arm, torch)))
    assert d["joints"].shape == (k, n, 7)
    for key in d:
        assert np.array_equal(d[key].view(np.uint8), raw[key].view(np.uint8)), key
    # what the Python driver refuses before any launch, by its whole text
    p = soa(pos_r, eul_r, torch)
    refused = {
        "policy must be 'fraction' or 'explicit'": lambda: solver.solve_sweep(p, grid, policy="interval0"),
        "thetas must have shape [K] or [K, n]": lambda: solver.solve_sweep(p, torch.zeros((k, n, 1), dtype=torch.float64)),
        "thetas: between 1 and 4096 samples per pose": lambda: solver.solve_sweep(p, torch.zeros(4097, dtype=torch.float64)),
        f"thetas: expected shape {(k, n)}, got {(k, n + 1)}": lambda: solver.solve_sweep(p, torch.zeros((k, n + 1), dtype=torch.float64)),
    }
    for text, call in refused.items():
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
