"""GPU tests (-m gpu, MI355X) of rsik_track (csrc/rsik_kernel_track.hpp): closed-loop tracking of goal trajectories in one launch, against
the NumPy reference and the derived tolerances of tests/track_workload.py (pinned on the CPU alone by tests/test_track_abi.py), against
the loop composed of rsik_forward_kinematics, torch and rsik_joint_rates, and against itself bit for bit.

Shapes: n in {1, 63, 64, 65, 257}, n_steps in {1, 2, 33}, arms uniform r, uniform l and a byte per trajectory, on the pairs of
jacobian_workload.PAIRS.  A trajectory's error is the 2-norm of (device - reference) over its seven joints."""
import contextlib
import io
import itertools

import numpy as np
import pytest

import arm_pairs
import jacobian_workload as JW
import track_workload as TW
from compare import bits
from gpu_support import T, abi, last_error, ptr, raw_call, torch_mod  # noqa: F401
from track_support import ALL, CONFIGS, NONE, OUTS, inputs, kind_arm, launch, row_alone, same, solver_of
from track_support import solvers_do_not_outlive_the_module  # noqa: F401
from track_workload import check_every_step, reference_terms

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)
STEPS = (1, 2, 33)


# ------------------------------------------------------------------------------------------ 1. values and bits per shape
@pytest.mark.parametrize("pair", TW.PAIRS)
def test_every_shape_values_and_bits(torch_mod, pair):
    """For every n, n_steps and arm arrangement, at lambda 1e-3 and 0.05, without and with feed-forward, rest and limits (all three
    together): final_joints has the bits of joints_steps[-1]; a second launch, each output alone and a damping array filled with
    lambda are bit for bit; an arm byte per trajectory equals the two uniform launches row by row; trajectories 0, 64 and 256 of the
    n = 257 launch have the bits of the same trajectory launched alone with n = 1.  The per-step check of every step (values of
    joints_steps and err_steps), for all four combinations at every n and n_steps, runs on the launch with an arm byte per trajectory:
    the uniform launches are tied to it bit for bit, row by row."""
    torch = torch_mod
    for n, n_steps in itertools.product(SIZES, STEPS):
        full = {}
        for kind in ("r", "l", "mixed"):
            arm = kind_arm(kind, n)
            for c, (lam, terms) in enumerate(CONFIGS):
                what = f"{pair} n={n} n_steps={n_steps} {kind} lambda={lam} terms={terms}"
                d = inputs(pair, n, n_steps, arm, terms)
                got = full[kind, c] = launch(torch, pair, kind, arm, d, lam)
                assert got["joints"].shape == got["rates"].shape == (n_steps, n, 7) and got["err"].shape == (n_steps, n, 2), what
                assert got["final_joints"].shape == (n, 7) and got["final_err"].shape == (n, 2), what
                assert all(np.isfinite(a).all() for a in got.values()), what
                assert np.array_equal(bits(got["final_joints"]), bits(got["joints"][-1])), (what, "final_joints")
                same(launch(torch, pair, kind, arm, d, lam), got, what + " twice")
                for o in OUTS:
                    same(got, launch(torch, pair, kind, arm, d, lam, want=(o,)), what + f" {o} alone")
                same(launch(torch, pair, kind, arm, d, np.full(n, lam)), got, what + " damping array filled with lambda")
                if kind == "mixed":
                    worst = check_every_step(pair, arm, d, lam, got, what)
                    print(f"{what}: every step within tol_t, worst error / tol_t {worst:.3g}")
                if n == 257:
                    for i in (0, 64, 256):
                        alone = launch(torch, pair, kind, arm[i:i + 1], row_alone(d, i), lam)
                        for o in OUTS:
                            pick = got[o][:, i:i + 1] if got[o].ndim == 3 else got[o][i:i + 1]
                            assert np.array_equal(bits(alone[o]), bits(pick)), (what, o, f"trajectory {i} launched alone")
        is_l = kind_arm("mixed", n) == 1
        for c in range(len(CONFIGS)):
            for o in OUTS:
                sel = is_l[None, :, None] if full["mixed", c][o].ndim == 3 else is_l[:, None]
                want = np.where(sel, full["l", c][o], full["r", c][o])
                assert np.array_equal(bits(full["mixed", c][o]), bits(want)), (pair, n, n_steps, c, o, "arm byte per trajectory")


# ------------------------------------------------------------------------------------------ 2. the prefix property
@pytest.mark.parametrize("terms", [NONE, ALL])
def test_prefix_property(torch_mod, terms):
    """The first 2 steps of an n_steps = 33 run have the bits of the n_steps = 2 run, and the n_steps = 33 run equals an n_steps = 16
    run followed by an n_steps = 17 run started from its final_joints, bit for bit (n = 257, an arm byte per trajectory)."""
    torch = torch_mod
    pair, n = "custom/custom", 257
    arm = kind_arm("mixed", n)
    d = inputs(pair, n, 33, arm, terms)
    whole = launch(torch, pair, "mixed", arm, d, 0.05)

    def part(lo, hi, start):
        cut = dict(d, m12=np.ascontiguousarray(d["m12"][lo:hi]), start=start, ff=None if d["ff"] is None else np.ascontiguousarray(d["ff"][lo:hi]))
        return launch(torch, pair, "mixed", arm, cut, 0.05)

    two = part(0, 2, d["start"])
    for o in ("joints", "rates", "err"):
        assert np.array_equal(bits(two[o]), bits(whole[o][:2])), (terms, o, "the first two steps")
    a = part(0, 16, d["start"])
    b = part(16, 33, a["final_joints"])
    for o in ("joints", "rates", "err"):
        assert np.array_equal(bits(np.concatenate([a[o], b[o]])), bits(whole[o])), (terms, o, "16 steps and then 17")
    for o in ("final_joints", "final_err"):
        assert np.array_equal(bits(b[o]), bits(whole[o])), (terms, o)


# ------------------------------------------------------------------------------------------ 3. end to end
def _end_to_end(torch, pair, side, gR, gp, A, what):
    """The device's joints after every step t against track_workload.run (lstsq rates) from the same start, within A * sum of tol_s
    over s <= t; A a number or one per row."""
    kind = "rl"[side]
    start = TW.starts(TW.N_RUN)
    d = dict(m12=TW.m12_of(gR, gp), start=start, ff=None, rest=None, rest_gain=0.0, limits=None)
    got = launch(torch, pair, kind, kind_arm(kind, TW.N_RUN), d, TW.LAM_RUN, want=("joints", "final_joints"))
    ref = TW.run(JW.blocks_of(pair)[side], start, gR, gp, TW.LAM_RUN, with_tolerance=True)
    assert (ref["err"][:, :, 1] < 1.0).all(), (what, "the rotation error is to stay far below pi")
    bound = A * np.cumsum(ref["tol"], axis=0)
    e = np.linalg.norm(got["joints"] - ref["joints"], axis=2)
    print(f"{pair} {kind} {what}: end to end over {TW.T_RUN} steps, A = {np.min(A):.2f} ... {np.max(A):.2f}, max error {e.max():.3e}, "
          f"max error / bound {(e / bound).max():.3g}, largest bound {bound.max():.3e}, median bound at the end {np.median(bound[-1]):.3e}")
    assert (e <= bound).all(), (pair, kind, what, float((e / bound).max()))
    assert np.array_equal(bits(got["final_joints"]), bits(got["joints"][-1]))


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("pair", TW.PAIRS)
def test_end_to_end_against_the_reference_run(torch_mod, pair, side):
    """The end-to-end case of track_workload (the constant-goal case: T = 64 steps of n = 512 uniform rows, lambda = 1e-3), each arm in a
    uniform launch, device against track_workload.run from the same start: the joints after every step t within A * sum of tol_s
    over s <= t, A the reference's own amplification on that block."""
    gR, gp, _ = TW.constant_goal_case(pair, side)
    _end_to_end(torch_mod, pair, side, gR, gp, TW.amplification(pair, side)[0], "constant goal")


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("pair", TW.PAIRS)
def test_end_to_end_on_moving_goals(torch_mod, pair, side):
    """The moving goals of track_workload (T = 64 steps of n = 512 uniform rows, lambda = 1e-3), each arm in a uniform launch, device
    against track_workload.run from the same start: the joints of row i after every step t within A_i * sum of tol_s over s <= t,
    A_i = 4 max(1, G_i) the reference's own amplification of that row (track_workload.run_gain: the norm of d q_end / d q_start; 22 on
    the worst row, which passes close to a straight elbow, 1.0 on the median row)."""
    gR, gp = TW.moving_goal_case(pair, side)
    _end_to_end(torch_mod, pair, side, gR, gp, 4.0 * np.maximum(1.0, TW.run_gain(pair, side))[None, :], "moving goals")


# ------------------------------------------------------------------------------------------ 4. convergence
@pytest.mark.parametrize("pair", TW.PAIRS)
def test_a_constant_goal_is_reached(torch_mod, pair):
    """The constant-goal case of track_workload (goal FK(q + delta), 512 rows, lambda = 1e-3, kp = ko = 50, dt = 0.01, 64 steps), each
    arm in a uniform launch: final_err is at most 2e-9 in both entries on the rows the reference brings below 1e-9, and finite on
    every row."""
    torch = torch_mod
    for side, kind in enumerate(("r", "l")):
        gR, gp, keep = TW.constant_goal_case(pair, side)
        d = dict(m12=TW.m12_of(gR, gp), start=TW.starts(TW.N_RUN), ff=None, rest=None, rest_gain=0.0, limits=None)
        got = launch(torch, pair, kind, kind_arm(kind, TW.N_RUN), d, TW.LAM_RUN, want=("final_err",))["final_err"]
        print(f"{pair} {kind}: kept {int(keep.sum())} of {len(keep)}, max final_err on them {got[keep].max(axis=0).tolist()}")
        assert keep.mean() >= 0.95 and np.isfinite(got).all(), (pair, kind)
        assert (got[keep] <= 2e-9).all(), (pair, kind, got[keep].max(axis=0).tolist())


# ------------------------------------------------------------------------------------------ 5. the composed loop
def _composed_step(torch, solver, arm_t, q, goal, ff, rest, lam, limits):
    """One step of the loop a caller of rsik_joint_rates runs: rsik_forward_kinematics, steps 2-4 in torch, rsik_joint_rates, steps 6-8
    in torch.  goal [12,n]."""
    p, R = solver.forward_kinematics(q, arm=arm_t)
    Rg, pg = goal[:9].T.reshape(-1, 3, 3), goal[9:].T
    D = Rg @ R.transpose(1, 2)
    w = 0.5 * torch.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], dim=1)
    s = w.norm(dim=1)
    angle = torch.atan2(s, 0.5 * (D.diagonal(dim1=1, dim2=2).sum(dim=1) - 1.0))
    big = s * s >= 2.0 ** -52
    e_o = w * torch.where(big, angle / torch.where(big, s, torch.ones_like(s)), torch.ones_like(s))[:, None]
    v = ff + torch.cat([TW.KP * (pg - p), TW.KO * e_o], dim=1)
    rates = solver.joint_rates(q, v, damping=lam, bias_rates=TW.REST_GAIN * (rest - q), arm=arm_t)["rates"]
    m = (rates.abs() / limits[0]).max(dim=1).values
    rates = torch.where((m > 1.0)[:, None], rates / m[:, None], rates)
    return torch.minimum(torch.maximum(q + TW.DT * rates, limits[1]), limits[2])


@pytest.mark.parametrize("pair", TW.PAIRS)
def test_against_the_composed_loop(torch_mod, pair):
    """T = 8 steps, n = 257, an arm byte per trajectory, with feed-forward, rest and limits: each step made of
    rsik_forward_kinematics, torch arithmetic and rsik_joint_rates, started from the single launch's own joints before that step, lands
    within tol_t of the single launch's joints after it."""
    torch = torch_mod
    n, steps, lam = 257, 8, 0.05
    arm = kind_arm("mixed", n)
    d = inputs(pair, n, steps, arm, ALL)
    got = launch(torch, pair, "mixed", arm, d, lam, want=("joints",))["joints"]
    solver, arm_t = solver_of(pair), T(arm, torch)
    m12, ff, rest, limits = T(d["m12"], torch), T(d["ff"], torch), T(d["rest"], torch), T(d["limits"], torch)
    worst = 0.0
    for t in range(steps):
        before = d["start"] if t == 0 else got[t - 1]
        composed = _composed_step(torch, solver, arm_t, T(before, torch), m12[t], ff[t], rest, lam, limits).cpu().numpy()
        tol = TW.step_by_arm(pair, arm, before, d["R"][t], d["p"][t], lam, **reference_terms(d, t))["tol"]
        e = np.linalg.norm(composed - got[t], axis=1)
        worst = max(worst, float(e.max()))
        assert (e <= tol).all(), (pair, t, float((e / tol).max()))
    print(f"{pair}: the composed loop against the single launch, largest difference {worst:.3e} rad")


# ------------------------------------------------------------------------------------------ 6. limits
@pytest.mark.parametrize("pair", ["default/default", "custom/custom"])
def test_limits(torch_mod, pair):
    """A rate_max that binds (the box infinite): in one step every |rate_k| <= rate_max_k (1 + 2^-52), the direction is the unlimited
    run's to 1e-12, and the trajectories where it does not bind carry the unlimited run's bits; over 33 steps the bound on the rates
    holds at every step.  A q_min / q_max box that binds (rate_max infinite): every joint of every step is inside it exactly."""
    torch = torch_mod
    n = 257
    arm = kind_arm("mixed", n)
    rate_only = TW.RATE_LIMIT_ONLY
    d = inputs(pair, n, 1, arm, ("ff",))
    free = launch(torch, pair, "mixed", arm, d, 0.05)
    lim = launch(torch, pair, "mixed", arm, dict(d, limits=rate_only), 0.05)
    fr, lr = free["rates"][0], lim["rates"][0]
    binds = (np.abs(fr) / rate_only[0]).max(axis=1) > 1.0
    print(f"{pair}: the rate limit binds on {int(binds.sum())} of {n} trajectories")
    assert binds.sum() >= n // 4 and (~binds).sum() >= 8
    assert (np.abs(lr) <= rate_only[0] * (1.0 + 2.0 ** -52)).all()
    cos = (lr * fr).sum(axis=1) / (np.linalg.norm(lr, axis=1) * np.linalg.norm(fr, axis=1))
    assert (np.abs(cos - 1.0) <= 1e-12).all(), float(np.abs(cos - 1.0).max())
    for o in OUTS:
        a, b = (x[o][:, ~binds] if x[o].ndim == 3 else x[o][~binds] for x in (lim, free))
        assert np.array_equal(bits(a), bits(b)), (pair, o, "a limit that does not bind changes nothing")
    assert (np.abs(lr[binds]) / rate_only[0]).max(axis=1).min() >= 1.0 - 2.0 ** -51, "a bound trajectory moves at its limit"
    d33 = inputs(pair, n, 33, arm, ("ff",))
    long = launch(torch, pair, "mixed", arm, dict(d33, limits=rate_only), 0.05, want=("rates",))["rates"]
    assert (np.abs(long) <= rate_only[0] * (1.0 + 2.0 ** -52)).all()
    box = np.array([[np.inf] * 7, [-1.5, -1.0, -1.5, -1.9, -0.5, -1.5, -1.0], [1.5, 1.0, 1.5, 0.1, 0.5, 1.5, 1.0]])
    boxed = launch(torch, pair, "mixed", arm, dict(d33, limits=box), 0.05, want=("joints", "final_joints"))
    assert (d33["start"] < box[1]).any() and (d33["start"] > box[2]).any()
    for o in ("joints", "final_joints"):
        assert (boxed[o] >= box[1]).all() and (boxed[o] <= box[2]).all(), (pair, o)
    on_edge = (boxed["joints"] == box[1]) | (boxed["joints"] == box[2])
    print(f"{pair}: {int(on_edge.sum())} of {on_edge.size} joint values sit on the box")
    assert on_edge.any()


# ------------------------------------------------------------------------------------------ 7. rows that are not numbers
PLACES = (0, 63, 64, 256)


@pytest.mark.parametrize("kind", ["r", "mixed"])
def test_trajectories_that_are_not_numbers(torch_mod, kind):
    """A NaN, a +inf and a -inf in start_joints, in the rest_joints row and in the damping entry, and damping values of 0 and -1, at
    trajectories 0, 63, 64 and the last of 257: those trajectories are NaN in every output, every other carries the clean run's bits."""
    torch = torch_mod
    pair, n, steps = "default/default", 257, 3
    arm = kind_arm(kind, n)
    d = inputs(pair, n, steps, arm, ALL)
    lam = np.full(n, 0.05)
    base = launch(torch, pair, kind, arm, d, lam)
    same(launch(torch, pair, kind, arm, d, 0.05), base, "damping array against damping_host")
    hit = np.zeros(n, dtype=bool)
    hit[list(PLACES)] = True
    values = {"start": (np.nan, np.inf, -np.inf), "rest": (np.nan, np.inf, -np.inf), "damping": (np.nan, np.inf, -np.inf, 0.0, -1.0)}
    for target, vals in values.items():
        for turn in range(len(vals)):  # the values rotate over the places: every value stands at every place in some turn
            a = {"start": d["start"].copy(), "rest": d["rest"].copy(), "damping": lam.copy()}
            for i, row in enumerate(PLACES):
                val = vals[(i + turn) % len(vals)]
                if target == "damping":
                    a[target][row] = val
                else:
                    a[target][row, (i + turn) % 7] = val
            for want in (OUTS, ("joints",), ("final_err",)):
                got = launch(torch, pair, kind, arm, dict(d, start=a["start"], rest=a["rest"]), a["damping"], want=want)
                for o in want:
                    g, b = (x[o].reshape(-1, n, x[o].shape[-1]) for x in (got, base))
                    assert np.isnan(g[:, hit]).all(), (kind, target, turn, o, "a trajectory that is not numbers must be NaN everywhere")
                    assert np.array_equal(bits(g[:, ~hit]), bits(b[:, ~hit])), (kind, target, turn, o, "another trajectory's bits changed")


def test_trajectories_that_are_not_numbers_inside_an_infinite_box(torch_mod):
    """With limits whose q_min and q_max are infinite (the ABI allows them) a trajectory whose start holds a NaN, a +inf or a -inf is
    NaN in every output at every step all the same (a clamp would turn a NaN into the bound), and every other trajectory carries the
    clean run's bits."""
    torch = torch_mod
    pair, n, steps = "default/default", 65, 3
    arm = kind_arm("mixed", n)
    d = dict(inputs(pair, n, steps, arm, ("ff",)), limits=np.array([TW.LIMITS[0], [-np.inf] * 7, [np.inf] * 7]))
    base = launch(torch, pair, "mixed", arm, d, 0.05)
    start = d["start"].copy()
    start[0, 3], start[63, 0], start[64, 6] = np.nan, np.inf, -np.inf
    hit = np.zeros(n, dtype=bool)
    hit[[0, 63, 64]] = True
    got = launch(torch, pair, "mixed", arm, dict(d, start=start), 0.05)
    for o in OUTS:
        g, b = (x[o].reshape(-1, n, x[o].shape[-1]) for x in (got, base))
        assert np.isnan(g[:, hit]).all(), (o, "a trajectory that is not numbers must be NaN everywhere")
        assert np.array_equal(bits(g[:, ~hit]), bits(b[:, ~hit])), (o, "another trajectory's bits changed")


@pytest.mark.parametrize("target", ["goal", "feedforward"])
def test_steps_that_are_not_numbers(torch_mod, target):
    """A NaN, a +inf or a -inf in a goal or a feed-forward entry at step 0, at a middle step and at the last step of 5, at trajectories
    0, 63, 64 and the last of 257: the step is held (joints_steps[t] the joints before it, rates_steps[t] = 0, err_steps[t] = NaN), the
    rest of that trajectory has the bits of the same run with that step removed, final_err is NaN exactly where the last goal is bad,
    and every other trajectory carries the clean run's bits."""
    torch = torch_mod
    pair, n, steps = "default/default", 257, 5
    arm = kind_arm("mixed", n)
    d = inputs(pair, n, steps, arm, ALL)
    base = launch(torch, pair, "mixed", arm, d, 0.05)
    hit = np.zeros(n, dtype=bool)
    hit[list(PLACES)] = True
    vals = (np.nan, np.inf, -np.inf)
    for s in (0, 2, steps - 1):
        m12, ff = d["m12"].copy(), d["ff"].copy()
        for i, row in enumerate(PLACES):
            if target == "goal":
                m12[s, (5 * i + s) % 12, row] = vals[(i + s) % 3]
            else:
                ff[s, row, (i + s) % 6] = vals[(i + s) % 3]
        got = launch(torch, pair, "mixed", arm, dict(d, m12=m12, ff=ff), 0.05)
        keep = [t for t in range(steps) if t != s]
        removed = launch(torch, pair, "mixed", arm, dict(d, m12=np.ascontiguousarray(d["m12"][keep]), ff=np.ascontiguousarray(d["ff"][keep])), 0.05)
        what = (target, s)
        before = d["start"] if s == 0 else got["joints"][s - 1]
        assert np.array_equal(bits(got["joints"][s][hit]), bits(np.ascontiguousarray(before[hit]))), (what, "the joints are held")
        assert (got["rates"][s][hit] == 0.0).all() and np.isnan(got["err"][s][hit]).all(), what
        for o in ("joints", "rates", "err"):
            assert np.array_equal(bits(got[o][keep][:, hit]), bits(removed[o][:, hit])), (what, o, "the run with the step removed")
            assert np.array_equal(bits(got[o][:, ~hit]), bits(base[o][:, ~hit])), (what, o, "another trajectory's bits changed")
        assert np.array_equal(bits(got["final_joints"][hit]), bits(removed["final_joints"][hit])), what
        if s == steps - 1 and target == "goal":
            assert np.isnan(got["final_err"][hit]).all(), what
        elif s != steps - 1:
            assert np.array_equal(bits(got["final_err"][hit]), bits(removed["final_err"][hit])), what
        else:  # a bad feed-forward at the last step: the last goal is a goal, final_err is its error at the held joints
            assert np.isfinite(got["final_err"][hit]).all(), what
        for o in ("final_joints", "final_err"):
            assert np.array_equal(bits(got[o][~hit]), bits(base[o][~hit])), (what, o)


# ------------------------------------------------------------------------------------------ 8. refusals and the surface
def test_refusals(torch_mod):
    """Every RSIK_E_INVALID case of include/rsik.h with the function's name in rsik_last_error; RSIK_E_NOT_SET on a context with no
    arm; n == 0 is RSIK_OK; with a damping array damping_host is not read, without rest_joints rest_gain is not read."""
    from reachy2_symbolic_ik_amd import HipSolver
    import ctypes as C

    torch, A = torch_mod, abi()
    solver = solver_of("default/default")
    n, steps = 8, 2
    arm_np = JW.arm_bytes()[:n]
    d = inputs("default/default", n, steps, arm_np, ALL)
    g, q, ff, rest = T(d["m12"], torch), T(d["start"], torch), T(d["ff"], torch), T(d["rest"], torch)
    lam, arm = torch.full((n,), 0.05, dtype=torch.float64, device="cuda"), T(arm_np, torch)
    o = torch.empty((steps, n, 7), dtype=torch.float64, device="cuda")

    def lim(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a, a.ctypes.data_as(C.POINTER(C.c_double))

    def args(**kw):
        a = dict(n=n, n_steps=steps, m12=ptr(g), arm=None, arm_uniform=0, start=ptr(q), dt=0.01, kp=50.0, ko=50.0, ff=ptr(ff), damping_host=0.05,
                 damping=None, rest=ptr(rest), rest_gain=1.0, limits=None, joints=ptr(o), rates=None, err=None, final_joints=None, final_err=None)
        a.update(kw)
        return tuple(a.values())

    keep = []
    cases = [("all outputs NULL", args(joints=None)), ("n < 0", args(n=-1)), ("n_steps 0", args(n_steps=0)), ("n_steps 65537", args(n_steps=65537)),
             ("m12_steps NULL", args(m12=None)), ("start_joints NULL", args(start=None)), ("arm_uniform 2", args(arm_uniform=2))]
    for name in ("dt", "kp", "ko", "rest_gain", "damping_host"):
        cases += [(f"{name} {v}", args(**{name: v})) for v in (-1.0, np.nan, np.inf)]
    cases += [("dt 0", args(dt=0.0)), ("damping_host 0", args(damping_host=0.0))]
    for what, bad in (("rate_max 0", (0, 3, 0.0)), ("rate_max NaN", (0, 0, np.nan)), ("q_min > q_max", (1, 2, 5.0)), ("q_min NaN", (1, 6, np.nan)),
                      ("q_max NaN", (2, 0, np.nan))):
        a = np.array(TW.LIMITS)
        a[bad[0], bad[1]] = bad[2]
        keep.append(lim(a))
        cases.append((what, args(limits=keep[-1][1])))
    for what, cargs in cases:
        assert raw_call(solver, "rsik_track", *cargs) == A.RSIK_E_INVALID, what
        assert "rsik_track" in last_error(solver), (what, last_error(solver))
    assert raw_call(solver, "rsik_track", *args(n=0, m12=None, start=None, joints=None)) == A.RSIK_OK
    assert raw_call(solver, "rsik_track", *args(damping=ptr(lam), damping_host=np.nan, arm=ptr(arm))) == A.RSIK_OK
    assert raw_call(solver, "rsik_track", *args(rest=None, rest_gain=np.nan, kp=0.0, ko=0.0)) == A.RSIK_OK
    inf = lim(np.array([[np.inf] * 7, [-np.inf] * 7, [np.inf] * 7]))
    assert raw_call(solver, "rsik_track", *args(limits=inf[1])) == A.RSIK_OK
    bare = HipSolver(0)
    assert raw_call(bare, "rsik_track", *args()) == A.RSIK_E_NOT_SET
    assert raw_call(bare, "rsik_track", *args(arm=ptr(arm))) == A.RSIK_E_NOT_SET
    torch.cuda.synchronize()
    bare.close()


def test_python_surface(torch_mod):
    """SymbolicIK.track_batch and DualArmIK.track_batch are HipSolver.track on their arms (goals as [T,12,n] or as matrices
    [T,n,4,4]); out= buffers are written in place; a planned launch writes the same bits; the default is the joints alone."""
    from reachy2_symbolic_ik_amd import DualArmIK, SymbolicIK

    torch = torch_mod
    pair, n, steps = "default/default", 130, 4
    solver = solver_of(pair)
    arm = kind_arm("mixed", n)
    with contextlib.redirect_stdout(io.StringIO()):
        ik_l = SymbolicIK("l_arm", solver=solver, **arm_pairs.DEFAULT)
        dual = DualArmIK(solver=solver, **arm_pairs.DEFAULT)
    dl = inputs(pair, n, steps, kind_arm("l", n), ALL)
    kw = dict(feedforward=dl["ff"], rest_joints=dl["rest"], rest_gain=dl["rest_gain"], limits=dl["limits"])
    res = ik_l.track_batch(dl["m12"], dl["start"], TW.DT, TW.KP, TW.KO, 0.05, **kw)
    assert tuple(res) == ("joints",)
    want = launch(torch, pair, "l", kind_arm("l", n), dl, 0.05)
    same({"joints": res["joints"].cpu().numpy()}, {"joints": want["joints"]}, "SymbolicIK.track_batch")
    M = np.zeros((steps, n, 4, 4))
    M[..., :3, :3], M[..., :3, 3], M[..., 3, 3] = dl["R"], dl["p"], 1.0
    res = ik_l.track_batch(M, dl["start"], TW.DT, TW.KP, TW.KO, 0.05, want=OUTS, **kw)
    same({k: a.cpu().numpy() for k, a in res.items()}, want, "SymbolicIK.track_batch on matrices")
    d = inputs(pair, n, steps, arm, NONE)
    got = {k: a.cpu().numpy() for k, a in dual.track_batch(arm, d["m12"], d["start"], TW.DT, TW.KP, TW.KO, 0.05, want=OUTS).items()}
    same(got, launch(torch, pair, "mixed", arm, d, 0.05), "DualArmIK.track_batch")
    out = {"err": torch.full((steps, n, 2), 7.0, dtype=torch.float64, device="cuda")}
    call = dict(damping=0.05, arm=T(arm, torch))
    res = solver.track(T(d["m12"], torch), T(d["start"], torch), TW.DT, TW.KP, TW.KO, want=("err", "final_err"), out=out, **call)
    assert res["err"] is out["err"] and tuple(res) == ("err", "final_err")
    plan = solver.track(T(d["m12"], torch), T(d["start"], torch), TW.DT, TW.KP, TW.KO, want=("err",), plan_only=True, **call)
    plan["launch"]()
    torch.cuda.synchronize()
    assert np.array_equal(bits(plan["err"].cpu().numpy()), bits(out["err"].cpu().numpy()))
    assert np.array_equal(bits(out["err"].cpu().numpy()), bits(got["err"]))
    for bad in (dict(want=()), dict(want=("twist",)), dict(damping=0.0), dict(damping=None), dict(dt=0.0), dict(kp=-1.0),
                dict(limits=np.zeros((3, 7))), dict(rest_gain=float("nan"))):
        a = {"dt": TW.DT, "kp": TW.KP, "ko": TW.KO, "damping": 0.05, **bad}
        with pytest.raises(ValueError):
            solver.track(T(d["m12"], torch), T(d["start"], torch), **a)
    with pytest.raises(ValueError):
        solver.track(T(d["m12"][:, :11], torch), T(d["start"], torch), TW.DT, TW.KP, TW.KO, damping=0.05)


def test_integration_md_snippet(torch_mod):
    """The tracking snippet of INTEGRATION.md as written: the hand moves 5 cm along x in 50 steps, goal t where it is to be when step t
    looks and the feed-forward of step t what carries it to goal t + 1.  Standing still would leave an error of exactly the path's
    length, 0.05 m, and no rotation error; the loop must do better than that on every trajectory that is numbers and end within
    1 mm and 1 mrad on the median trajectory (the damping holds back lambda^2 / (sigma^2 + lambda^2) of the twist, 4 % of 1 mm per step
    at sigma = 0.1, which the feedback at kp dt = 0.2 turns into 0.2 mm), and a start the solve could not give stays NaN."""
    from reachy2_symbolic_ik_amd import SymbolicIK

    torch = torch_mod
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", solver=solver_of("default/default"), **arm_pairs.DEFAULT)
    pos, eul, arm, _ = JW.link_poses()
    poses = np.ascontiguousarray(np.stack([pos[arm == 0], eul[arm == 0]], axis=1))  # [n,2,3]

    q = ik.solve_batch(poses)["joints"]
    n, T_, dt = len(q), 50, 0.01
    p, R = ik.forward_kinematics_batch(q)
    s = torch.arange(T_, dtype=torch.float64, device=q.device) / (T_ - 1)
    step = torch.tensor([0.05, 0.0, 0.0], dtype=torch.float64, device=q.device)
    goals = torch.cat([R.reshape(1, n, 9).expand(T_, n, 9), p[None] + s[:, None, None] * step], dim=2)
    goals = goals.permute(0, 2, 1).contiguous()
    ff = torch.zeros((T_, n, 6), dtype=torch.float64, device=q.device)
    ff[:-1, :, 0] = 0.05 / ((T_ - 1) * dt)
    limits = torch.tensor([[2.0] * 7, [-6.3] * 7, [6.3] * 7])
    run = ik.track_batch(goals, q, dt=dt, kp=20.0, ko=20.0, damping=0.02, feedforward=ff, limits=limits,
                         want=("joints", "err", "final_err"))

    assert tuple(run["joints"].shape) == (T_, n, 7) and tuple(run["err"].shape) == (T_, n, 2) and tuple(run["final_err"].shape) == (n, 2)
    ok = torch.isfinite(q).all(dim=1).cpu().numpy()
    fe = run["final_err"].cpu().numpy()
    assert ok.sum() * 2 >= n and np.isfinite(fe[ok]).all() and np.isnan(fe[~ok]).all()
    print(f"INTEGRATION.md tracking snippet: final position error max {fe[ok, 0].max():.3e} m, median {np.median(fe[ok, 0]):.3e} m, "
          f"rotation max {fe[ok, 1].max():.3e} rad")
    assert (fe[ok, 0] < 0.05).all() and np.median(fe[ok, 0]) <= 1e-3 and np.median(fe[ok, 1]) <= 1e-3
