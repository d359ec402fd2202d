"""CPU-side checks of rsik_track: declared, exported, bound, ABI version still 8, the Python surface exists, the argument check that needs
no device — and the reference and the tolerances of the GPU tests (tests/track_workload.py) pinned on the CPU alone: one_step against
joint_rates_workload.reference, the convergence filter's share, the amplification, the gain per row on the moving goals, the rotation-vector helper against SciPy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jacobian_workload as JW
import joint_rates_workload as W
import track_workload as TW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ surface
def test_track_entry_point_is_part_of_abi_8():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert _abi.ABI_VERSION == 8 == L.rsik_abi_version()
    assert "rsik_track" in _abi.PROTOTYPES
    assert isinstance(L.rsik_track, C._CFuncPtr)
    hdr = open(os.path.join(ROOT, "include", "rsik.h")).read()
    assert "#define RSIK_ABI_VERSION 8" in hdr
    decl = re.search(r"int rsik_track\(([^;]*)\);", hdr)
    assert decl, "include/rsik.h does not declare rsik_track"
    assert len(decl.group(1).split(",")) == len(_abi.PROTOTYPES["rsik_track"][1]) == 21
    assert int(re.search(r"#define RSIK_OPT_COUNT (\d+)", hdr).group(1)) == 9
    for words in ("it MUST be a rotation", "At a rotation by pi the direction is undefined", "exactly what rsik_joint_rates defines",
                  "the direction is kept", "is skipped"):
        assert words in hdr, words
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`rsik_track`" in doc and "track_batch" in doc


def test_track_entry_point_refuses_a_null_context():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert L.rsik_track(None, 0, 1, None, None, 0, None, 0.01, 1.0, 1.0, None, 0.05, None, None, 0.0, None,
                        None, None, None, None, None) == _abi.RSIK_E_INVALID


def test_python_surface_exists():
    from reachy2_symbolic_ik_amd import DualArmIK, HipSolver, SymbolicIK

    for cls, name in ((HipSolver, "track"), (SymbolicIK, "track_batch"), (DualArmIK, "track_batch")):
        fn = getattr(cls, name)
        assert callable(fn), (cls.__name__, name)
        for word in ("final_err", "one launch"):
            assert word in fn.__doc__, (cls.__name__, name, word)
    assert HipSolver.TRACK_OUTPUTS == ("joints", "rates", "err", "final_joints", "final_err")


# ------------------------------------------------------------------------------------------ the reference, on the CPU alone
@pytest.mark.parametrize("pair", TW.PAIRS)
def test_one_step_without_feedback_is_an_integration_of_the_joint_rates_reference(pair):
    """kp = ko = 0 and a feed-forward twist: one_step equals q + dt * joint_rates_workload.reference(J, ff, lambda, q0), with and
    without the rest term, exactly; err is the pose error of the goal and does not enter."""
    n = 64
    q, ff, rest = TW.starts(n), TW.feedforwards(1)[0, :n], TW.rests(n)
    for side, block in enumerate(JW.blocks_of(pair)):
        R, p = (g[0, :n] for g in TW.side_goals(pair, 1)[side])
        J = JW.jacobian(block, q)
        for lam in TW.LAMBDAS:
            s = TW.one_step(block, q, R, p, lam, kp=0.0, ko=0.0, ff=ff)
            assert np.array_equal(s["joints"], q + TW.DT * W.reference(J, ff, lam)["rates"]), (pair, side, lam)
            s = TW.one_step(block, q, R, p, lam, kp=0.0, ko=0.0, ff=ff, rest=rest, rest_gain=TW.REST_GAIN)
            want = W.reference(J, ff, lam, TW.REST_GAIN * (rest - q))["rates"]
            assert np.array_equal(s["rates"], want) and np.array_equal(s["joints"], q + TW.DT * want), (pair, side, lam, "rest")
            assert np.isfinite(s["err"]).all() and (s["err"][:, 1] < 1.0).all()


@pytest.mark.parametrize("pair", TW.PAIRS)
def test_limits_and_skipped_rows_of_the_reference(pair):
    """With limits no |rate_k| exceeds rate_max_k by more than a rounding, the direction is the unlimited one, the joints stay in the
    box; a row whose goal or feed-forward is not numbers is held, with rates 0 and err NaN, and the other rows do not change."""
    n = 64
    block = JW.blocks_of(pair)[0]
    q, ff = TW.starts(n), TW.feedforwards(1)[0, :n].copy()
    R, p = (g[0, :n].copy() for g in TW.side_goals(pair, 1)[0])
    free = TW.one_step(block, q, R, p, 0.05, ff=ff)
    lim = TW.one_step(block, q, R, p, 0.05, ff=ff, limits=TW.RATE_LIMIT_ONLY)
    bound = (np.abs(free["rates"]) / TW.RATE_LIMIT_ONLY[0]).max(axis=1) > 1.0
    print(f"{pair}: the rate limit binds on {int(bound.sum())} of {n} rows")
    assert bound.sum() >= n // 4 and (~bound).sum() >= 4
    assert (np.abs(lim["rates"]) <= TW.RATE_LIMIT_ONLY[0] * (1 + 2.0 ** -52)).all()
    cos = (lim["rates"] * free["rates"]).sum(axis=1) / (np.linalg.norm(lim["rates"], axis=1) * np.linalg.norm(free["rates"], axis=1))
    assert (np.abs(cos - 1.0) < 1e-12).all()
    assert np.array_equal(lim["rates"][~bound], free["rates"][~bound])
    boxed = TW.one_step(block, q, R, p, 0.05, ff=ff, limits=TW.LIMITS)["joints"]
    assert (boxed >= TW.LIMITS[1]).all() and (boxed <= TW.LIMITS[2]).all()
    R[3, 1, 1], p[7, 2], ff[11, 5] = np.nan, np.inf, -np.inf
    s = TW.one_step(block, q, R, p, 0.05, ff=ff)
    hit = np.zeros(n, dtype=bool)
    hit[[3, 7, 11]] = True
    assert np.array_equal(s["joints"][hit], q[hit]) and (s["rates"][hit] == 0.0).all() and np.isnan(s["err"][hit]).all()
    for k in ("joints", "rates", "err"):
        assert np.array_equal(s[k][~hit], free[k][~hit]), k


@pytest.mark.parametrize("pair", TW.PAIRS)
def test_the_convergence_filter_keeps_at_least_95_percent(pair):
    """The constant-goal case (track_workload.constant_goal_case): the share of rows the reference brings below 1e-9 m and 1e-9 rad in
    64 steps is at least 95 % on both blocks, so that the filter cannot hide a failure.  Measured: 99.4 % (509 of 512) on every pair
    and block."""
    for side in (0, 1):
        keep = TW.constant_goal_case(pair, side)[2]
        print(f"{pair} slot {side}: the reference converges on {int(keep.sum())} of {len(keep)} rows")
        assert keep.mean() >= 0.95, (pair, side, float(keep.mean()))


@pytest.mark.parametrize("pair", TW.PAIRS)
def test_the_closed_loop_does_not_amplify(pair):
    """The amplification A of the end-to-end case (track_workload.amplification: the constant-goal case) is below 16 on both blocks.
    Measured: worst ratio 0.927 ... 0.960, A = 3.71 ... 3.84.  And the reference's own runs, on the constant goal and on the moving goals
    (33 steps, the longest the GPU tests launch them for), keep the rotation error below 1 rad at every step."""
    for side in (0, 1):
        A, ratio = TW.amplification(pair, side)
        print(f"{pair} slot {side}: worst |difference at the end| / |difference at the start| = {ratio:.3f}, A = {A:.2f}")
        assert A < 16.0, (pair, side, A)
        block, n = JW.blocks_of(pair)[side], TW.N_RUN
        R, p = TW.side_goals(pair, 33)[side]
        gR, gp, _ = TW.constant_goal_case(pair, side)
        for what, ref in (("moving goals", TW.run(block, TW.starts(n), R[:, :n], p[:, :n], TW.LAM_RUN, solver="restatement")),
                          ("constant goal", TW.run(block, TW.starts(n), gR, gp, TW.LAM_RUN, solver="restatement"))):
            print(f"{pair} slot {side} {what}: largest rotation error of the run {ref['err'][:, :, 1].max():.3f} rad")
            assert (ref["err"][:, :, 1] < 1.0).all(), (pair, side, what)


@pytest.mark.parametrize("pair", TW.PAIRS)
def test_the_gain_per_row_on_moving_goals_is_large_on_few_rows(pair):
    """track_workload.run_gain, the amplification per row that the end-to-end test on the moving goals uses: at least 95 % of the rows
    have G <= 4 on both blocks, so that a factor per row cannot hide a failure, and every G is a number.  Measured: 99.2 % and
    99.4 %, the median 1.007 ... 1.008, the largest 22.2 (row 55)."""
    for side in (0, 1):
        G = TW.run_gain(pair, side)
        print(f"{pair} slot {side}: G <= 4 on {int((G <= 4.0).sum())} of {len(G)} rows, median {np.median(G):.3f}, largest {G.max():.1f} "
              f"(row {int(G.argmax())})")
        assert np.isfinite(G).all() and (G <= 4.0).mean() >= 0.95, (pair, side, float((G <= 4.0).mean()))


def test_rotation_vector_helper_against_scipy():
    """track_workload.rotvec (SciPy-free) against Rotation.from_matrix(D).as_rotvec() on 4096 seeded rotations of angle below 3 rad:
    1e-14 per entry, the angle to 1e-14; and the small-angle branch (s^2 < 2^-52) returns w itself."""
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(7306)
    axis = rng.normal(size=(4096, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = np.concatenate([rng.uniform(0.0, 3.0, size=3072), 10.0 ** rng.uniform(-12.0, -1.0, size=1024)])
    D = Rotation.from_rotvec(axis * angle[:, None]).as_matrix()
    e_o, got_angle = TW.rotvec(D)
    want = Rotation.from_matrix(D).as_rotvec()
    print(f"rotvec against SciPy: max difference {np.abs(e_o - want).max():.3e}, angle {np.abs(got_angle - angle).max():.3e}")
    assert np.abs(e_o - want).max() <= 1e-14
    assert np.abs(got_angle - angle).max() <= 1e-14
    tiny = Rotation.from_rotvec(axis[:8] * 1e-9).as_matrix()
    e_o, _ = TW.rotvec(tiny)
    w = 0.5 * np.stack([tiny[:, 2, 1] - tiny[:, 1, 2], tiny[:, 0, 2] - tiny[:, 2, 0], tiny[:, 1, 0] - tiny[:, 0, 1]], axis=1)
    assert np.array_equal(e_o, w)


# ------------------------------------------------------------------------------------------ rotation errors of any size
LADDER_ROWS = 64


def _ladder_case(k):
    """Rung k on LADDER_ROWS rows of custom/custom, r block: (R_g [n,3,3], R [n,3,3]) with seeded unit axes."""
    block = JW.blocks_of("custom/custom")[0]
    q = TW.starts(LADDER_ROWS)
    axes = np.random.default_rng(7308 + k).normal(size=(LADDER_ROWS, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    R_g, _ = TW.rotated_goals(block, q, axes, np.full(LADDER_ROWS, TW.LADDER[k]))
    return R_g, JW.fk(block, q)[1]


def test_the_ladder_keeps_clear_of_the_switch_near_pi():
    """The ladder's band condition: |s^2 2^52 - 1| >= 2^-6 on every row that is not near 0, on the rows the GPU test launches (every
    pair, an arm byte per row) and on the rows of the checks below, so that an s that differs by 3 e takes the same branch of e_o;
    and the padded ladder holds every rung at least six times."""
    angles, axes, rung = TW.ladder()
    assert len(TW.LADDER) == 20 and np.bincount(rung).min() >= 6 and np.allclose(np.linalg.norm(axes, axis=1), 1.0, atol=1e-15)
    for pair in TW.PAIRS:
        g = TW.ladder_goals(pair, JW.arm_bytes()[:TW.N_LADDER], TW.starts()[:TW.N_LADDER])
        margin = TW.band_margin(g["s"])[rung >= TW.NEAR_ZERO_RUNGS]
        print(f"{pair}: smallest |s^2 2^52 - 1| away from 0: {margin.min():.4f}")
        assert (margin >= TW.BAND).all(), pair
        assert (6.0 * TW.FK_ENTRY / g["s"][(rung >= TW.NEAR_ZERO_RUNGS) & (rung < 19)] < TW.BAND / 64).all()
    for k in range(TW.NEAR_ZERO_RUNGS, len(TW.LADDER)):
        R_g, R = _ladder_case(k)
        assert (TW.band_margin(TW.w_norm(R_g @ R.transpose(0, 2, 1))) >= TW.BAND).all(), k


def test_e_o_bound_bounds_the_movement_of_the_reference():
    """R perturbed by seeded noise of e = FK_ENTRY per entry: at every rung e_o moves by at most e_o_bound (2-norm) and the angle by
    at most E_ANGLE, on 64 rows of custom/custom.  Measured: the worst movement / bound is 0.42, at the pi rung (0.18 at
    pi - 2^-26 (1 + 2^-6), where the bound is 1.2e-5); the angle moves by at most 1.2e-14."""
    noise = np.random.default_rng(7309).uniform(-TW.FK_ENTRY, TW.FK_ENTRY, size=(LADDER_ROWS, 3, 3))
    worst = 0.0
    for k, a in enumerate(TW.LADDER):
        R_g, R = _ladder_case(k)
        D = R_g @ R.transpose(0, 2, 1)
        e_o, angle = TW.rotvec(D)
        e_o2, angle2 = TW.rotvec(R_g @ (R + noise).transpose(0, 2, 1))
        bound = TW.e_o_bound(angle, TW.w_norm(D))
        ratio = float((np.linalg.norm(e_o2 - e_o, axis=1) / bound).max())
        worst = max(worst, ratio)
        print(f"rung {k:2d} angle {a!r}: e_o moves by at most {ratio:.3g} of e_o_bound ({bound.max():.3e}), the angle by {np.abs(angle2 - angle).max():.3e}")
        assert ratio <= 1.0, (k, ratio)
        assert (np.abs(angle2 - angle) <= TW.E_ANGLE).all(), k
    print(f"worst movement / bound {worst:.3g}")


def test_the_reference_angle_against_mpmath_and_at_a_half_turn():
    """rotvec's angle against mpmath's angle of the same (R_g, R) pair at 50 digits, at every rung, 8 rows each: 4 ulp(pi) = 1.8e-15.
    At the pi rung the reference's |e_o| is below 3 e and its angle within E_ANGLE of pi."""
    import mpmath as mp

    worst = 0.0
    for k in range(len(TW.LADDER)):
        R_g, R = (a[:8] for a in _ladder_case(k))
        e_o, angle = TW.rotvec(R_g @ R.transpose(0, 2, 1))
        with mp.workdps(50):
            for i in range(len(R)):
                D = mp.matrix(R_g[i].tolist()) * mp.matrix(R[i].tolist()).T
                w = [(D[2, 1] - D[1, 2]) / 2, (D[0, 2] - D[2, 0]) / 2, (D[1, 0] - D[0, 1]) / 2]
                want = mp.atan2(mp.sqrt(sum(x * x for x in w)), (D[0, 0] + D[1, 1] + D[2, 2] - 1) / 2)
                worst = max(worst, abs(float(mp.mpf(float(angle[i])) - want)))
                assert abs(float(mp.mpf(float(angle[i])) - want)) <= 4.0 * np.spacing(np.pi), (k, i)
        if k == len(TW.LADDER) - 1:
            assert (np.linalg.norm(e_o, axis=1) < 3.0 * TW.FK_ENTRY).all() and (np.abs(angle - np.pi) <= TW.E_ANGLE).all()
    print(f"the reference's angle against mpmath: {worst:.3e}")


def test_step_tolerance_takes_e_o_per_row():
    """step_tolerance with the default is what it was; with e_o per row it is linear in it."""
    block = JW.blocks_of("custom/custom")[0]
    n = 16
    q = TW.starts(n)
    R, p = (g[0, :n] for g in TW.side_goals("custom/custom", 1)[0])
    s = TW.one_step(block, q, R, p, 0.05)
    t = W.tolerances(s["J"], s["v"], 0.05, None)
    base = TW.DT * (t["tol_row"] + t["g"] * (TW.KP * TW.E_P + TW.KO * TW.E_O)) + 4.0 * TW.EPS * np.linalg.norm(q, axis=1)
    assert np.array_equal(TW.step_tolerance(s, q, 0.05), base)
    e_o = np.linspace(1.0, 2.0, n) * TW.E_O
    assert np.allclose(TW.step_tolerance(s, q, 0.05, e_o=e_o) - base, TW.DT * t["g"] * TW.KO * (e_o - TW.E_O), rtol=1e-12, atol=0.0)


# ------------------------------------------------------------------------------------------ finite values that overflow
@pytest.mark.parametrize("lam", TW.LAMBDAS)
def test_which_far_rungs_overflow_in_the_reference(lam):
    """The far rungs of the GPU test on the reference alone (custom/custom, the far rows, step 1 from the reference's own step 0):
    the rates are not finite exactly on track_workload.FAR_HELD, with lstsq and with the float64 restatement of the device's
    algorithm alike; such a row is held like a skipped one (joints kept, rates 0, err NaN) instead of NaN joints; on the other rungs
    the step is taken, with limits every |rate_k| <= rate_max_k (1 + 2^-52), and err[0] is +infinity from |e_p| = 1.3e154 on."""
    pair, n = "custom/custom", TW.N_FAR
    arm = JW.arm_bytes()[:n]
    rows = list(TW.FAR_ROWS)
    R, p = TW.goals_of(pair, TW.T_FAR, arm)
    clean = dict(R=R, p=p, m12=TW.m12_of(R, p), ff=np.ascontiguousarray(TW.feedforwards(TW.T_FAR)[:, :n]))
    q1 = TW.step_by_arm(pair, arm[rows], TW.starts()[rows], R[0][rows], p[0][rows], lam, ff=clean["ff"][0][rows], limits=TW.LIMITS)["joints"]
    for kind, value in TW.FAR_RUNGS:
        d = TW.far_inputs(clean, kind, value)
        assert np.array_equal(np.flatnonzero((d["m12"] != clean["m12"]).any(axis=(0, 1)) | (d["ff"] != clean["ff"]).any(axis=(0, 2))), rows)
        assert np.array_equal(TW.m12_of(d["R"], d["p"]), d["m12"])
        for solver in ("lstsq", "restatement"):
            s = TW.step_by_arm(pair, arm[rows], q1, d["R"][1][rows], d["p"][1][rows], lam, ff=d["ff"][1][rows], limits=TW.LIMITS, solver=solver)
            held = (kind, value) in TW.FAR_HELD
            assert (s["overflow"] == held).all(), (kind, value, solver, s["overflow"].tolist())
            if held:
                assert np.array_equal(s["joints"], q1) and (s["rates"] == 0.0).all() and np.isnan(s["err"]).all(), (kind, value, solver)
            else:
                assert np.isfinite(s["rates"]).all() and (np.abs(s["rates"]) <= TW.LIMITS[0] * (1 + 2.0 ** -52)).all(), (kind, value, solver)
                far = kind == "goal" and value >= TW.EP2_OVERFLOWS
                assert (np.isposinf(s["err"][:, 0]) if far else np.isfinite(s["err"][:, 0])).all(), (kind, value, solver, s["err"].tolist())
