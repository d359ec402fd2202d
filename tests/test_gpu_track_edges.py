"""GPU tests (-m gpu, MI355X) of rsik_track (csrc/rsik_kernel_track.hpp) at the edges of its domain, which tests/test_gpu_track.py
stays away from: rotation errors from 0 to a half turn (both ends of the s^2 < 2^-52 branch, the c <= 0 side of fast_atan2), a goal that
is reached exactly, starts on the wound set, the singular set and the far rungs of tests/far_inputs.py, and finite goals and
feed-forwards so large that the arithmetic overflows.  Against the NumPy reference and the derived tolerances of
tests/track_workload.py (pinned on the CPU alone by tests/test_track_abi.py).

Shapes: n = 130 (two waves and two rows: a wave boundary and a partial last wave) unless a test says otherwise, n_steps 1 or 3,
dt, kp, ko = DT, KP, KO, lambda in LAMBDAS, an arm byte per trajectory.  Every tolerance is one of E_ANGLE, E_P, e_o_bound,
step_tolerance (and rates_tolerance, its part for the rates), joint_rates_workload.tolerances at (J, v / m, lambda), and the 1e-9
include/rsik.h gives for far angles."""
import fractions
import itertools

import numpy as np
import pytest

import jacobian_workload as JW
import joint_rates_workload as W
import track_workload as TW
from compare import bits
from gpu_support import T, torch_mod  # noqa: F401
from track_support import OUTS, inputs, inputs_of, kind_arm, launch, row_alone, solver_of
from track_support import solvers_do_not_outlive_the_module  # noqa: F401

pytestmark = pytest.mark.gpu

N = TW.N_LADDER
E3 = 3.0 * TW.FK_ENTRY


def with_all_terms(d, n, n_steps=1):
    return dict(d, ff=np.ascontiguousarray(TW.feedforwards(n_steps)[:, :n]), rest=TW.rests()[:n], rest_gain=TW.REST_GAIN, limits=TW.LIMITS)


# ------------------------------------------------------------------------------------------ 1. rotation errors of any size
@pytest.mark.parametrize("pair", TW.PAIRS)
def test_rotation_errors_from_zero_to_a_half_turn(torch_mod, pair):
    """One step towards the goals of track_workload.ladder (a prescribed rotation error per row, 0 ... pi, no position error), without
    and with feed-forward, rest and limits, at both lambdas: err_steps[0][:, 1] within E_ANGLE of the reference's angle and
    err_steps[0][:, 0] <= E_P on every row; the rates within rates_tolerance and the joints within step_tolerance of one_step, with
    e_o_bound per row in place of E_O.  At the pi rung the rates are those of the same step at ko = 0, within the tolerance for an
    e_o of 3 e: the loop does not turn towards a goal a half turn away.  Rows 0, 63, 64 and the last launched alone carry the bits they
    have in the batch."""
    torch = torch_mod
    arm, start = kind_arm("mixed", N), TW.starts()[:N]
    g = TW.ladder_goals(pair, arm, start)
    angles, _, rung = TW.ladder(N)
    assert (TW.band_margin(g["s"])[rung >= TW.NEAR_ZERO_RUNGS] >= TW.BAND).all(), "a ladder row sits on the switch of e_o"
    at_pi = rung == len(TW.LADDER) - 1
    plain = inputs_of(g["R"][None], g["p"][None], start)
    for lam, (name, d) in itertools.product(TW.LAMBDAS, (("no terms", plain), ("feed-forward, rest and limits", with_all_terms(plain, N)))):
        what = f"{pair} lambda={lam} {name}"
        got = launch(torch, pair, "mixed", arm, d, lam)
        assert all(np.isfinite(a).all() for a in got.values()), what
        ref = TW.step_by_arm(pair, arm, start, g["R"], g["p"], lam, e_o=g["e_o"], **TW.reference_terms(d, 0))
        e_angle = np.abs(got["err"][0][:, 1] - ref["err"][:, 1])
        e_rates = np.linalg.norm(got["rates"][0] - ref["rates"], axis=1)
        e_joints = np.linalg.norm(got["joints"][0] - ref["joints"], axis=1)
        for k, a in enumerate(TW.LADDER):
            r = rung == k
            print(f"{what} rung {k:2d} angle {a!r}: angle error / E_ANGLE {(e_angle[r] / TW.E_ANGLE).max():.3g}, rates / tolerance "
                  f"{(e_rates[r] / ref['tol_rates'][r]).max():.3g}, joints / tol_t {(e_joints[r] / ref['tol'][r]).max():.3g}")
        assert (e_angle <= TW.E_ANGLE).all(), (what, "angle", int(e_angle.argmax()), float(e_angle.max()))
        assert (got["err"][0][:, 0] <= TW.E_P).all(), (what, "position error", float(got["err"][0][:, 0].max()))
        assert (e_rates <= ref["tol_rates"]).all(), (what, "rates", int((e_rates / ref["tol_rates"]).argmax()), float((e_rates / ref["tol_rates"]).max()))
        assert (e_joints <= ref["tol"]).all(), (what, "joints", int((e_joints / ref["tol"]).argmax()), float((e_joints / ref["tol"]).max()))
        # a half turn: the rates of ko = 0
        still = launch(torch, pair, "mixed", arm, d, lam, ko=0.0, want=("rates",))["rates"][0]
        ref0 = TW.step_by_arm(pair, arm, start, g["R"], g["p"], lam, ko=0.0, tol_ko=TW.KO, e_o=E3, **TW.reference_terms(d, 0))
        turn = np.linalg.norm(got["rates"][0] - still, axis=1)
        print(f"{what}: at a half turn the rates differ from those at ko = 0 by at most {(turn[at_pi] / ref0['tol_rates'][at_pi]).max():.3g} of the tolerance")
        assert at_pi.sum() >= 6 and (turn[at_pi] <= ref0["tol_rates"][at_pi]).all(), (what, "a half turn", float((turn / ref0["tol_rates"])[at_pi].max()))
        for i in (0, 63, 64, N - 1):
            alone = launch(torch, pair, "mixed", arm[i:i + 1], row_alone(d, i), lam)
            for o in OUTS:
                pick = got[o][:, i:i + 1] if got[o].ndim == 3 else got[o][i:i + 1]
                assert np.array_equal(bits(alone[o]), bits(pick)), (what, o, f"trajectory {i} launched alone")


# ------------------------------------------------------------------------------------------ 2. a goal that is reached exactly
@pytest.mark.parametrize("set_name", ["uniform", "wound", "singular"])
def test_a_goal_that_is_reached_exactly(torch_mod, set_name):
    """The goal of every step is the device's own rsik_forward_kinematics of the start: track_chain forms the position and the rotation
    from the expressions of forward_kinematics, and D(i, j) and D(j, i) are one fma chain with its factors swapped, so the pose error
    is exactly zero: err_steps and final_err are 0.0, the rates 0.0, and every joints_steps[t] and final_joints carry the bits of
    start, over 3 steps at both lambdas."""
    torch = torch_mod
    steps = 3
    arm, start = kind_arm("mixed", N), JW.joint_set(set_name)[:N]
    for pair, lam in itertools.product(TW.PAIRS, TW.LAMBDAS):
        what = f"{pair} {set_name} lambda={lam}"
        p, R = solver_of(pair).forward_kinematics(T(start, torch), arm=T(arm, torch))
        torch.cuda.synchronize()
        p, R = p.cpu().numpy(), R.cpu().numpy()
        assert np.isfinite(p).all() and np.isfinite(R).all(), what
        d = inputs_of(np.broadcast_to(R, (steps,) + R.shape), np.broadcast_to(p, (steps,) + p.shape), start)
        got = launch(torch, pair, "mixed", arm, d, lam)
        print(f"{what}: largest err_steps {got['err'].max(axis=(0, 1)).tolist()}, largest |rate| {np.abs(got['rates']).max():.3e}")
        assert (got["err"] == 0.0).all(), (what, "err_steps", got["err"].max(axis=(0, 1)).tolist())
        assert (got["rates"] == 0.0).all(), (what, "rates_steps", float(np.abs(got["rates"]).max()))
        for t in range(steps):
            assert np.array_equal(bits(got["joints"][t]), bits(start)), (what, t, "joints_steps")
        assert np.array_equal(bits(got["final_joints"]), bits(start)), (what, "final_joints")
        assert (got["final_err"] == 0.0).all(), (what, "final_err", got["final_err"].max(axis=0).tolist())


# ------------------------------------------------------------------------------------------ 3. far start joints
FAR_TOL = 1e-9      # include/rsik.h: a far angle is answered like its reduced twin to 1e-9 (rsik_jacobian)


def far_starts():
    """One joint of a uniform row at 2^27, 1e15 or 1e300, each joint in turn (21 rows, the sign alternating), and the reduced twins:
    rows of joint_rates_workload.far_rows."""
    far, twin = W.far_rows()
    rows = [(g * 7 + k) * 2 + k % 2 for g in range(3) for k in range(7)]
    return np.ascontiguousarray(far[rows]), np.ascontiguousarray(twin[rows])


def test_wound_singular_and_far_starts(torch_mod):
    """One step from the wound set gives the rates, the error and the motion (joints - start: the joints stay wound) of the unwound
    rows to 1e-9, without terms and with a feed-forward and a rate limit.  One joint at 2^27, 1e15 or 1e300: rates and error within 1e-9
    of the reduced twin's and finite, and joints_steps[0] = fl(start + dt rates) in every joint, the far one included.  The singular
    set (a straight elbow) over 3 steps at both lambdas: the per-step check of tests/test_gpu_track.py, and every output finite."""
    torch = torch_mod
    pair = "custom/custom"
    arm = kind_arm("mixed", N)
    plain_q, wound_q = JW.joint_set("uniform")[:N], JW.joint_set("wound")[:N]
    R, p = TW.goals_of(pair, 1, arm)
    for lam, terms in itertools.product(TW.LAMBDAS, ((), ("ff",))):
        kw = dict(ff=TW.feedforwards(1)[:, :N], limits=TW.RATE_LIMIT_ONLY) if terms else {}
        a, b = (launch(torch, pair, "mixed", arm, inputs_of(R, p, q, **kw), lam) for q in (wound_q, plain_q))
        figures = {"rates": np.abs(a["rates"] - b["rates"]).max(), "err": np.abs(a["err"] - b["err"]).max(),
                   "motion": np.abs((a["joints"][0] - wound_q) - (b["joints"][0] - plain_q)).max()}
        print(f"wound set against the unwound rows, lambda={lam} terms={terms}: " + ", ".join(f"{k} {v:.3e}" for k, v in figures.items()))
        assert all(np.isfinite(x).all() for x in a.values()), (lam, terms)
        assert all(v <= FAR_TOL for v in figures.values()), (lam, terms, figures)

    far, twin = far_starts()
    n = len(far)
    assert n == 21
    arm = kind_arm("mixed", n)
    delta = TW.joint_paths(1)[0, :n] - TW.starts()[:n]
    g = TW.by_arm(JW.blocks_of(pair), arm, lambda block, rows: dict(zip("pR", JW.fk(block, (twin + delta)[rows]))))
    R, p = g["R"][None], g["p"][None]
    for lam in TW.LAMBDAS:
        a, b = (launch(torch, pair, "mixed", arm, inputs_of(R, p, q, ff=TW.feedforwards(1)[:, :n]), lam) for q in (far, twin))
        figures = {"rates": np.abs(a["rates"] - b["rates"]).max(), "err": np.abs(a["err"] - b["err"]).max()}
        print(f"far starts against their reduced twins, lambda={lam}: " + ", ".join(f"{k} {v:.3e}" for k, v in figures.items()))
        assert np.isfinite(a["rates"]).all() and np.isfinite(a["err"]).all() and np.isfinite(a["final_err"]).all(), lam
        assert all(v <= FAR_TOL for v in figures.values()), (lam, figures)
        F = fractions.Fraction
        want = np.array([[float(F(far[i, k]) + F(TW.DT) * F(a["rates"][0, i, k])) for k in range(7)] for i in range(n)])
        off = np.abs(a["joints"][0] - want)
        assert (off <= np.spacing(np.abs(far))).all(), (lam, "joints_steps[0] against fl(start + dt rates)", float((off / np.spacing(np.abs(far))).max()))
        assert np.array_equal(bits(a["final_joints"]), bits(a["joints"][0])), lam

    steps = 3
    arm = kind_arm("mixed", N)
    start = JW.joint_set("singular")[:N]
    R, p = TW.goals_near(pair, arm, start, steps)
    plain = inputs_of(R, p, start)
    for lam, (name, d) in itertools.product(TW.LAMBDAS, (("no terms", plain), ("feed-forward, rest and limits", with_all_terms(plain, N, steps)))):
        what = f"{pair} singular set lambda={lam} {name}"
        got = launch(torch, pair, "mixed", arm, d, lam)
        assert all(np.isfinite(x).all() for x in got.values()), what
        worst = TW.check_every_step(pair, arm, d, lam, got, what)
        print(f"{what}: every step within tol_t, worst error / tol_t {worst:.3g}")


# ------------------------------------------------------------------------------------------ 4. finite values that overflow
MODES = (("limits", TW.LIMITS), ("a rate limit alone", TW.RATE_LIMIT_ONLY), ("no limits", None))


def _without_far_step(d):
    keep = [t for t in range(TW.T_FAR) if t != TW.FAR_STEP]
    return dict(d, m12=np.ascontiguousarray(d["m12"][keep]), R=d["R"][keep], p=d["p"][keep], ff=np.ascontiguousarray(d["ff"][keep])), keep


@pytest.mark.parametrize("lam", TW.LAMBDAS)
def test_finite_goals_and_feedforwards_far_outside_reach(torch_mod, lam):
    """n = 65, 3 steps, an ordinary feed-forward; at step 1 of trajectories 0, 63 and 64 one goal-position entry stands at 1e15 ...
    1e307 or one feed-forward entry at 1e150 ... DBL_MAX (track_workload.FAR_RUNGS), with the limits, with a rate limit alone and
    without limits.  Everywhere: every other trajectory carries the clean run's bits, with limits no |rate_k| exceeds
    rate_max_k (1 + 2^-52) at any step and with the box every joint of every step lies inside it.  Where the rates overflow
    (track_workload.FAR_HELD: the goal at 1e307, the feed-forward at DBL_MAX) the step is held exactly as a skipped step: joints_steps[1]
    has the bits of joints_steps[0], rates_steps[1] = 0, err_steps[1] = NaN, and steps 0 and 2 carry the bits of the run with step 1
    removed.  On every other rung the step is taken: the rates are finite and, with limits, stand against one_step's from the
    device's joints_steps[0] within joint_rates_workload.tolerances at (J, v / m, lambda), m the reference's limit factor (without a
    rest term the solve is linear in v); err_steps[1][:, 0] is |e_p| to 4 ulp below 1.3e154 on the goal rungs (E_P on the feed-forward
    rungs, where e_p is ordinary) and +infinity above; err_steps[1][:, 1] is within E_ANGLE."""
    torch = torch_mod
    pair, n, steps = "custom/custom", TW.N_FAR, TW.T_FAR
    arm = kind_arm("mixed", n)
    rows = list(TW.FAR_ROWS)
    hit = np.zeros(n, dtype=bool)
    hit[rows] = True
    s = TW.FAR_STEP
    clean_runs = {}
    for (mode, limits), (kind, value) in itertools.product(MODES, TW.FAR_RUNGS):
        what = f"lambda={lam} {mode}, {kind} entry at {value!r}"
        clean = dict(inputs(pair, n, steps, arm, ("ff",)), limits=limits)
        if mode not in clean_runs:
            clean_runs[mode] = launch(torch, pair, "mixed", arm, clean, lam)
        base = clean_runs[mode]
        d = TW.far_inputs(clean, kind, value)
        got = launch(torch, pair, "mixed", arm, d, lam)
        for o in OUTS:
            g, b = (x[o].reshape(-1, n, x[o].shape[-1]) for x in (got, base))
            assert np.array_equal(bits(g[:, ~hit]), bits(b[:, ~hit])), (what, o, "another trajectory's bits changed")
        if limits is not None:
            assert (np.abs(got["rates"]) <= limits[0] * (1.0 + 2.0 ** -52)).all(), (what, "a rate beyond rate_max", got["rates"][:, hit].tolist())
            assert (got["joints"] >= limits[1]).all() and (got["joints"] <= limits[2]).all() and (got["final_joints"] >= limits[1]).all() \
                and (got["final_joints"] <= limits[2]).all(), (what, "a joint outside the box", got["joints"][:, hit].tolist())
        before = np.ascontiguousarray(got["joints"][s - 1][rows])
        ref = TW.step_by_arm(pair, arm[rows], before, d["R"][s][rows], d["p"][s][rows], lam, ff=d["ff"][s][rows], limits=limits)
        held = (kind, value) in TW.FAR_HELD
        assert (ref["overflow"] == held).all(), (what, "the reference's own rates", ref["overflow"].tolist())
        rates, err = got["rates"][s][rows], got["err"][s][rows]
        print(f"{what}: rates_steps[1] largest |entry| per far row {np.abs(rates).max(axis=1).tolist()}, err_steps[1] {err.tolist()}")
        if held:
            assert np.array_equal(bits(np.ascontiguousarray(got["joints"][s][rows])), bits(before)), (what, "the joints are held", got["joints"][s][rows].tolist())
            assert (rates == 0.0).all(), (what, "rates_steps[1] of a held step", rates.tolist())
            assert np.isnan(err).all(), (what, "err_steps[1] of a held step", err.tolist())
            cut, keep = _without_far_step(d)
            removed = launch(torch, pair, "mixed", arm, cut, lam)
            for o in ("joints", "rates", "err"):
                assert np.array_equal(bits(got[o][keep][:, hit]), bits(removed[o][:, hit])), (what, o, "the run with step 1 removed")
            for o in ("final_joints", "final_err"):
                assert np.array_equal(bits(got[o][hit]), bits(removed[o][hit])), (what, o, "the run with step 1 removed")
            continue
        assert np.isfinite(rates).all() and np.isfinite(got["joints"]).all(), (what, "the rates of a step that is taken", rates.tolist())
        assert not np.isnan(err).any(), (what, "err_steps[1] of a step that is taken", err.tolist())
        e_p = ref["err"][:, 0]
        if kind == "goal" and value >= TW.EP2_OVERFLOWS:
            assert np.isposinf(e_p).all() and np.isposinf(err[:, 0]).all(), (what, "err_steps[1][:, 0]", err[:, 0].tolist())
        elif kind == "goal":
            assert (np.abs(err[:, 0] - e_p) <= 4.0 * np.spacing(e_p)).all(), (what, "err_steps[1][:, 0]", err[:, 0].tolist(), e_p.tolist())
        else:
            assert (np.abs(err[:, 0] - e_p) <= TW.E_P).all(), (what, "err_steps[1][:, 0]", err[:, 0].tolist(), e_p.tolist())
        assert (np.abs(err[:, 1] - ref["err"][:, 1]) <= TW.E_ANGLE).all(), (what, "err_steps[1][:, 1]", err[:, 1].tolist())
        if limits is not None:
            tol = W.tolerances(ref["J"], ref["v"] / ref["m"][:, None], lam)["tol_row"]
            e = np.linalg.norm(rates - ref["rates"], axis=1)
            print(f"{what}: limit factor m {ref['m'].tolist()}, rates error / tolerance {(e / tol).tolist()}")
            assert (e <= tol).all(), (what, "rates against one_step", (e / tol).tolist())


def test_far_values_at_the_last_step_reach_final_err(torch_mod):
    """final_err is step 2 once more: with the last goal's position at 1e160 its first entry is +infinity, never NaN, on the three far
    trajectories, and the rotation entry stays within E_ANGLE of the reference's at final_joints."""
    torch = torch_mod
    pair, n, lam = "custom/custom", TW.N_FAR, 0.05
    arm = kind_arm("mixed", n)
    rows = list(TW.FAR_ROWS)
    d = dict(inputs(pair, n, 2, arm, ("ff",)), limits=TW.LIMITS)
    p, m12 = d["p"].copy(), d["m12"].copy()
    for i, row in enumerate(rows):
        p[1, row, i % 3] = m12[1, 9 + i % 3, row] = 1e160
    got = launch(torch, pair, "mixed", arm, dict(d, p=p, m12=m12), lam)
    assert np.isposinf(got["final_err"][rows, 0]).all() and np.isposinf(got["err"][1][rows, 0]).all(), got["final_err"][rows].tolist()
    ref = TW.by_arm(JW.blocks_of(pair), arm[rows], lambda block, r: dict(
        err=TW.pose_error(block, got["final_joints"][rows][r], d["R"][1][rows][r], p[1][rows][r])[2]))["err"]
    assert (np.abs(got["final_err"][rows, 1] - ref[:, 1]) <= TW.E_ANGLE).all(), got["final_err"][rows].tolist()
