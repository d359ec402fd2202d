"""GPU tests (-m gpu, MI355X) of rsik_track_avoid (csrc/rsik_kernel_track_avoid.hpp): rsik_track with obstacle avoidance inside the loop,
against rsik_clearance and rsik_track bit for bit, against the NumPy reference and the derived tolerances of
tests/track_avoid_workload.py (pinned on the CPU alone by tests/test_track_avoid_abi.py), against the loop composed of
rsik_forward_kinematics, rsik_clearance, torch and rsik_joint_rates, and against itself bit for bit.

Shapes, small on purpose: n in {1, 63, 64, 65, 257}, n_steps in {1, 2, 33}, arms uniform r, uniform l and a byte per trajectory; scenes of
one sphere, of one capsule, clearance_workload's "open" scene and a full one of 256 spheres and 64 capsules."""
import contextlib
import ctypes as C
import io
import itertools

import numpy as np
import pytest

import arm_pairs
import clearance_workload as CW
import jacobian_workload as JW
import track_avoid_workload as AW
import track_workload as TW
from compare import bits
from gpu_support import T, abi, arm_kwargs, last_error, ptr, raw_call, torch_mod  # noqa: F401
from track_support import ALL, NONE, inputs, kind_arm, row_alone, same, solver_of
from track_support import launch as launch_track
from track_support import solvers_do_not_outlive_the_module  # noqa: F401

pytestmark = pytest.mark.gpu

OUTS = ("joints", "rates", "err", "clearance", "nearest", "final_joints", "final_err", "min_clearance")
SHARED = ("joints", "rates", "err", "final_joints", "final_err")
SIZES = (1, 63, 64, 65, 257)
STEPS = (1, 2, 33)
PLACES = (0, 63, 64, 256)


def scenes(pair):
    sc = CW.scene(pair, "open")
    return {"sphere": dict(spheres=sc["spheres"][:1], capsules=sc["capsules"][:0]), "capsule": dict(spheres=sc["spheres"][:0], capsules=sc["capsules"][:1]),
            "open": sc, "full": AW.full_scene(pair)}


def launch(torch, pair, kind, arm, d, lam, sc, want=OUTS, influence=AW.INFLUENCE, avoid_gain=AW.AVOID_GAIN, radius=AW.LINK_RADIUS, dt=TW.DT,
           kp=TW.KP, ko=TW.KO):
    """One launch through HipSolver.track_avoid on a launch's inputs d (track_support.inputs) and a scene; the results on the host."""
    t = lambda a: None if a is None or not len(a) else T(a, torch)  # noqa: E731
    res = solver_of(pair).track_avoid(T(d["m12"], torch), T(d["start"], torch), dt, kp, ko, damping=lam if isinstance(lam, float) else T(lam, torch),
                                      spheres=t(sc["spheres"]), capsules=t(sc["capsules"]), link_radius=radius, influence=influence,
                                      avoid_gain=avoid_gain, feedforward=t(d["ff"]), rest_joints=t(d["rest"]), rest_gain=d["rest_gain"],
                                      limits=d["limits"], want=want, **arm_kwargs(kind, arm, torch))
    torch.cuda.synchronize()
    assert tuple(res) == tuple(o for o in OUTS if o in want), (tuple(res), want)
    return {k: a.cpu().numpy() for k, a in res.items()}


def clearance_of(torch, pair, kind, arm, q, sc, want=("clearance", "nearest"), radius=AW.LINK_RADIUS):
    """rsik_clearance on joints [n,7] or [T,n,7] with the same obstacles and radii; the results on the host."""
    t = lambda a: None if not len(a) else T(a, torch)  # noqa: E731
    res = solver_of(pair).clearance(T(q, torch), spheres=t(sc["spheres"]), capsules=t(sc["capsules"]), link_radius=radius, want=want,
                                    **arm_kwargs(kind, arm, torch))
    torch.cuda.synchronize()
    return {k: a.cpu().numpy() for k, a in res.items()}


def per_traj(a, n):
    """An output as [*, n, *]: the trajectory on axis 1."""
    return a.reshape(-1, n, a.shape[-1]) if a.ndim >= 2 and a.shape[-2:-1] == (n,) else a.reshape(-1, n, 1)


def pick(got, o, i, n):
    a = got[o]
    return a[i:i + 1] if a.shape[0] == n and o in ("final_joints", "final_err", "min_clearance") else a[:, i:i + 1]


# ------------------------------------------------------------------------------------------ 1. shapes and bits
@pytest.mark.parametrize("terms", [NONE, ALL])
def test_every_shape_and_its_bits(torch_mod, terms):
    """Every n, n_steps and arm form, the four scenes and the pairs rotating over them: the shapes and dtypes of the eight outputs; a
    second launch and each output alone are bit for bit; final_joints has the bits of joints_steps[-1]; trajectories 0, 64 and 256 of
    n = 257 equal the same trajectory launched alone with n = 1; a permutation of the obstacles leaves clearance_steps and min_clearance
    unchanged."""
    torch = torch_mod
    rng = np.random.default_rng(7310)
    for i, (n, n_steps, kind) in enumerate(itertools.product(SIZES, STEPS, ("r", "l", "mixed"))):
        pair = AW.PAIRS[i % len(AW.PAIRS)]
        name = ("sphere", "capsule", "open", "full")[(i // 3 + i) % 4]
        sc = scenes(pair)[name]
        what = f"{pair} n={n} n_steps={n_steps} {kind} scene={name} terms={terms}"
        arm = kind_arm(kind, n)
        d = inputs(pair, n, n_steps, arm, terms)
        got = launch(torch, pair, kind, arm, d, 0.05, sc)
        assert got["joints"].shape == got["rates"].shape == (n_steps, n, 7) and got["err"].shape == (n_steps, n, 2), what
        assert got["clearance"].shape == (n_steps, n) and got["nearest"].shape == (n_steps, n, 2) and got["nearest"].dtype == np.int32, what
        assert got["final_joints"].shape == (n, 7) and got["final_err"].shape == (n, 2) and got["min_clearance"].shape == (n,), what
        assert all(np.isfinite(a).all() for a in got.values()) and (got["nearest"] >= 0).all(), what
        assert np.array_equal(bits(got["final_joints"]), bits(got["joints"][-1])), (what, "final_joints")
        assert (got["min_clearance"] <= got["clearance"].min(axis=0)).all(), what
        same(launch(torch, pair, kind, arm, d, 0.05, sc), got, what + " twice")
        for o in OUTS:
            same(got, launch(torch, pair, kind, arm, d, 0.05, sc, want=(o,)), what + f" {o} alone")
        order_s, order_c = rng.permutation(len(sc["spheres"])), rng.permutation(len(sc["capsules"]))
        mixed_up = launch(torch, pair, kind, arm, d, 0.05, dict(spheres=sc["spheres"][order_s], capsules=sc["capsules"][order_c]),
                          want=("clearance", "min_clearance"), avoid_gain=0.0)
        still = launch(torch, pair, kind, arm, d, 0.05, sc, want=("clearance", "min_clearance"), avoid_gain=0.0)
        same(mixed_up, still, what + " obstacles permuted")
        if n == 257:
            for r in (0, 64, 256):
                alone = launch(torch, pair, kind, arm[r:r + 1], row_alone(d, r), 0.05, sc)
                for o in OUTS:
                    assert np.array_equal(bits(alone[o]), bits(np.ascontiguousarray(pick(got, o, r, n)))), (what, o, f"trajectory {r} launched alone")


@pytest.mark.parametrize("terms", [NONE, ALL])
def test_prefix_property(torch_mod, terms):
    """The n_steps = 33 run equals an n_steps = 16 run followed by an n_steps = 17 run started from its final_joints, bit for bit
    (n = 257, an arm byte per trajectory, the "open" scene), min_clearance being the smaller of the two parts'."""
    torch = torch_mod
    pair, n = "custom/custom", 257
    arm = kind_arm("mixed", n)
    sc = CW.scene(pair, "open")
    d = inputs(pair, n, 33, arm, terms)
    whole = launch(torch, pair, "mixed", arm, d, 0.05, sc)

    def part(lo, hi, start):
        cut = dict(d, m12=np.ascontiguousarray(d["m12"][lo:hi]), start=start, ff=None if d["ff"] is None else np.ascontiguousarray(d["ff"][lo:hi]))
        return launch(torch, pair, "mixed", arm, cut, 0.05, sc)

    a = part(0, 16, d["start"])
    b = part(16, 33, a["final_joints"])
    for o in ("joints", "rates", "err", "clearance", "nearest"):
        assert np.array_equal(bits(np.concatenate([a[o], b[o]])), bits(whole[o])), (terms, o, "16 steps and then 17")
    for o in ("final_joints", "final_err"):
        assert np.array_equal(bits(b[o]), bits(whole[o])), (terms, o)
    assert np.array_equal(bits(np.minimum(a["min_clearance"], b["min_clearance"])), bits(whole["min_clearance"]))
    assert (whole["clearance"] < AW.INFLUENCE).any() and (whole["clearance"] >= AW.INFLUENCE).any()


# ------------------------------------------------------------------------------------------ 2. against rsik_clearance
@pytest.mark.parametrize("name", ["sphere", "capsule", "open", "full"])
def test_clearance_and_nearest_are_rsik_clearance_s_bits(torch_mod, name):
    """clearance_steps[t] and nearest_steps[t] equal, bit for bit, rsik_clearance on start_joints (t = 0) and on joints_steps[t - 1], with
    the same obstacles and radii; min_clearance is the minimum of those and of rsik_clearance(final_joints), bit for bit.  n = 257,
    33 steps, with feed-forward, rest and limits, every arm form."""
    torch = torch_mod
    pair, n, n_steps = "default/ztip", 257, 33
    sc = scenes(pair)[name]
    for kind in ("r", "l", "mixed"):
        arm = kind_arm(kind, n)
        d = inputs(pair, n, n_steps, arm, ALL)
        got = launch(torch, pair, kind, arm, d, 0.05, sc)
        before = np.concatenate([d["start"][None], got["joints"][:-1]])
        ref = clearance_of(torch, pair, kind, arm, before, sc)
        assert np.array_equal(bits(got["clearance"]), bits(ref["clearance"])), (name, kind, "clearance_steps")
        assert np.array_equal(got["nearest"], ref["nearest"]), (name, kind, "nearest_steps")
        last = clearance_of(torch, pair, kind, arm, got["final_joints"], sc)["clearance"]
        assert np.array_equal(bits(got["min_clearance"]), bits(np.minimum(ref["clearance"].min(axis=0), last))), (name, kind, "min_clearance")


# ------------------------------------------------------------------------------------------ 3. against rsik_track
@pytest.mark.parametrize("terms", [NONE, ALL])
def test_without_a_push_the_bits_are_rsik_track_s(torch_mod, terms):
    """With the scene 10 m away, and with influence = 0, the five shared outputs have rsik_track's bits, at both lambdas and in every arm
    form (n = 257, 33 steps, the "open" scene)."""
    torch = torch_mod
    pair, n, n_steps = "default/default", 257, 33
    sc = CW.scene(pair, "open")
    for kind, lam in itertools.product(("r", "l", "mixed"), TW.LAMBDAS):
        arm = kind_arm(kind, n)
        d = inputs(pair, n, n_steps, arm, terms)
        plain = launch_track(torch, pair, kind, arm, d, lam)
        away = launch(torch, pair, kind, arm, d, lam, AW.moved(sc))
        assert (away["clearance"] > 5.0).all()
        same({o: away[o] for o in SHARED}, plain, f"{kind} lambda={lam} terms={terms}: the scene 10 m away")
        # influence = 0.  Radii of zero make every clearance an axis distance, which is never below 0: no trajectory is pushed.
        with np.errstate(invalid="ignore"):  # (the scene's row at infinity)
            thin = dict(spheres=sc["spheres"] * np.array([1.0, 1.0, 1.0, 0.0]), capsules=sc["capsules"] * np.array([1.0] * 6 + [0.0]))
        blind = launch(torch, pair, kind, arm, d, lam, thin, influence=0.0, radius=(0.0, 0.0, 0.0))
        assert (blind["clearance"] >= 0.0).all() and (blind["clearance"] < AW.INFLUENCE).any()
        same({o: blind[o] for o in SHARED}, plain, f"{kind} lambda={lam} terms={terms}: influence = 0, radii of zero")
        # With the scene's own radii a clearance below 0 IS below an influence of 0 (the definition pushes it): the trajectories that
        # never penetrate have rsik_track's bits, the others do not count here.
        blind = launch(torch, pair, kind, arm, d, lam, sc, influence=0.0)
        free = blind["min_clearance"] >= 0.0
        assert free.sum() >= n // 8 and (~free).any()
        for o in SHARED:
            a, b = (per_traj(x[o], n) for x in (blind, plain))
            assert np.array_equal(bits(np.ascontiguousarray(a[:, free])), bits(np.ascontiguousarray(b[:, free]))), (kind, lam, terms, o, "influence = 0")


# ------------------------------------------------------------------------------------------ 4. per step, against the reference
@pytest.mark.parametrize("terms", [NONE, ALL])
@pytest.mark.parametrize("pair", AW.PAIRS)
def test_every_step_against_the_reference(torch_mod, pair, terms):
    """The device's own joints before step t fed into the reference's one step: on the kept pairs joints_steps[t] is within tol_t
    (track_avoid_workload), the clearance within CLEARANCE_BOUND on every pair, at lambda 1e-3 and 0.05 (n = 65, 6 steps, an arm byte
    per trajectory, the "open" scene).  Prints the worst error / tolerance."""
    torch = torch_mod
    n, n_steps = 65, 6
    arm = kind_arm("mixed", n)
    sc = CW.scene(pair, "open")
    d = inputs(pair, n, n_steps, arm, terms)
    for lam in TW.LAMBDAS:
        got = launch(torch, pair, "mixed", arm, d, lam, sc)
        worst, compared, active = 0.0, 0, 0
        for t in range(n_steps):
            before = d["start"] if t == 0 else got["joints"][t - 1]
            ref = AW.one_step(pair, arm, before, d["R"][t], d["p"][t], lam, sc, **AW.terms_of(d, t))
            tol, keep = AW.step_tolerance(ref, before, lam), AW.kept(ref)
            assert (np.abs(got["clearance"][t] - ref["clearance"]) <= CW.CLEARANCE_BOUND).all(), (pair, terms, lam, t, "clearance")
            e = np.linalg.norm(got["joints"][t] - ref["joints"], axis=1)
            worst, compared, active = max(worst, float((e / tol)[keep].max())), compared + int(keep.sum()), active + int((keep & ref["push"]).sum())
            assert (e[keep] <= tol[keep]).all(), (pair, terms, lam, t, float((e / tol)[keep].max()))
            assert np.array_equal((got["clearance"][t] < AW.INFLUENCE)[keep], ref["push"][keep]), (pair, terms, lam, t, "the side of the select")
        print(f"{pair} terms={terms} lambda={lam}: {compared} of {n * n_steps} pairs compared, {active} of them pushed, worst error / tol_t {worst:.3g}")
        assert compared >= 0.8 * n * n_steps and active >= 0.1 * n * n_steps


# ------------------------------------------------------------------------------------------ 5. the composed loop
@pytest.mark.parametrize("pair", AW.PAIRS)
def test_against_the_composed_loop(torch_mod, pair):
    """T = 8 steps, n = 257, an arm byte per trajectory, with feed-forward, rest and limits: each step made of rsik_forward_kinematics,
    rsik_clearance, torch arithmetic and rsik_joint_rates with bias_rates, started from the single launch's own joints before that step,
    lands within track_workload's tol_t (with the full q0) of the single launch's joints after it.  No clearance term: the composed
    step's clearance and gradient are the device's own."""
    torch = torch_mod
    n, steps, lam = 257, 8, 0.05
    arm = kind_arm("mixed", n)
    sc = CW.scene(pair, "open")
    d = inputs(pair, n, steps, arm, ALL)
    got = launch(torch, pair, "mixed", arm, d, lam, sc, want=("joints", "clearance"))
    solver, arm_t = solver_of(pair), T(arm, torch)
    m12, ff, rest, limits = T(d["m12"], torch), T(d["ff"], torch), T(d["rest"], torch), T(d["limits"], torch)
    sp, cp = T(sc["spheres"], torch), T(sc["capsules"], torch)
    worst = 0.0
    for t in range(steps):
        before = d["start"] if t == 0 else got["joints"][t - 1]
        q = T(before, torch)
        p, R = solver.forward_kinematics(q, arm=arm_t)
        near = solver.clearance(q, spheres=sp, capsules=cp, link_radius=AW.LINK_RADIUS, arm=arm_t, want=("clearance", "gradient"))
        assert np.array_equal(bits(near["clearance"].cpu().numpy()), bits(got["clearance"][t])), (pair, t)
        Rg, pg = m12[t][:9].T.reshape(-1, 3, 3), m12[t][9:].T
        D = Rg @ R.transpose(1, 2)
        w = 0.5 * torch.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], dim=1)
        s = w.norm(dim=1)
        angle = torch.atan2(s, 0.5 * (D.diagonal(dim1=1, dim2=2).sum(dim=1) - 1.0))
        big = s * s >= 2.0 ** -52
        e_o = w * torch.where(big, angle / torch.where(big, s, torch.ones_like(s)), torch.ones_like(s))[:, None]
        v = ff[t] + torch.cat([TW.KP * (pg - p), TW.KO * e_o], dim=1)
        q0 = TW.REST_GAIN * (rest - q)
        push = near["clearance"] < AW.INFLUENCE
        q0 = torch.where(push[:, None], q0 + (AW.AVOID_GAIN * (AW.INFLUENCE - near["clearance"]))[:, None] * near["gradient"], q0)
        rates = solver.joint_rates(q, v, damping=lam, bias_rates=q0, arm=arm_t)["rates"]
        m = (rates.abs() / limits[0]).max(dim=1).values
        rates = torch.where((m > 1.0)[:, None], rates / m[:, None], rates)
        composed = torch.minimum(torch.maximum(q + TW.DT * rates, limits[1]), limits[2]).cpu().numpy()
        ref = AW.one_step(pair, arm, before, d["R"][t], d["p"][t], lam, sc, solver="restatement", **AW.terms_of(d, t))
        tol = TW.step_tolerance(ref, before, lam)
        e = np.linalg.norm(composed - got["joints"][t], axis=1)
        worst = max(worst, float((e / tol).max()))
        assert (e <= tol).all(), (pair, t, float((e / tol).max()))
    print(f"{pair}: the composed loop against the single launch, worst difference / tol_t {worst:.3g}")


# ------------------------------------------------------------------------------------------ 6. it avoids
@pytest.mark.parametrize("pair", AW.PAIRS)
def test_it_avoids(torch_mod, pair):
    """The one-sphere elbow case (constant goal, 64 steps), each arm in a uniform launch, on the rows the reference moves away by at
    least 1 cm: the device's min_clearance with avoidance exceeds the device's without by at least half the reference's gain, and
    final_err is within the reference's final_err + 2e-9."""
    torch = torch_mod
    for side, kind in enumerate(("r", "l")):
        e = AW.elbow_case(pair, side)
        rows = e["rows"]
        assert rows.sum() >= 32
        d = dict(m12=TW.m12_of(e["R"], e["p"]), start=e["start"], ff=None, rest=None, rest_gain=0.0, limits=None)
        kw = dict(want=("min_clearance", "final_err"), influence=AW.ELBOW_INFLUENCE, kp=AW.ELBOW_KP, ko=AW.ELBOW_KP)
        arm = kind_arm(kind, AW.N_ELBOW)
        free = launch(torch, pair, kind, arm, d, TW.LAM_RUN, e["scene"], avoid_gain=0.0, **kw)
        avoid = launch(torch, pair, kind, arm, d, TW.LAM_RUN, e["scene"], avoid_gain=AW.ELBOW_GAIN, **kw)
        gain = avoid["min_clearance"] - free["min_clearance"]
        over = avoid["final_err"] - e["avoid"]["final_err"]
        print(f"{pair} {kind}: {int(rows.sum())} rows, device gain / reference gain at least {(gain / e['gain'])[rows].min():.4f}, "
              f"final_err above the reference's by at most {over[rows].max():.3e}")
        assert (gain[rows] >= 0.5 * e["gain"][rows]).all(), (pair, kind, float((gain / e["gain"])[rows].min()))
        assert (over[rows] <= 2e-9).all(), (pair, kind, float(over[rows].max()))


# ------------------------------------------------------------------------------------------ 7. what is not a number
def test_obstacles_that_are_not_numbers(torch_mod):
    """A NaN, a +inf, a -inf in an obstacle row and a negative radius, at the first, a middle and the last obstacle of either kind: the
    clean run's bits with that obstacle removed (the indices of nearest_steps behind it one lower).  Every obstacle unusable:
    clearance_steps and min_clearance +inf, nearest_steps (-1, -1), and rsik_track's bits otherwise."""
    torch = torch_mod
    pair, n, n_steps = "default/default", 65, 5
    arm = kind_arm("mixed", n)
    d = inputs(pair, n, n_steps, arm, ALL)
    open_sc = CW.scene(pair, "open")
    sc = dict(spheres=open_sc["spheres"][CW.usable(open_sc["spheres"])][:9], capsules=open_sc["capsules"][CW.usable(open_sc["capsules"])][:5])
    S = len(sc["spheres"])
    values = (np.nan, np.inf, -np.inf, "radius")
    turn = 0
    for key, width in (("spheres", 4), ("capsules", 7)):
        count = len(sc[key])
        for place in (0, count // 2, count - 1):
            rows = sc[key].copy()
            val = values[turn % 4]
            if val == "radius":
                rows[place, width - 1] = -1e-3
            else:
                rows[place, turn % (width - 1)] = val
            turn += 1
            got = launch(torch, pair, "mixed", arm, d, 0.05, dict(sc, **{key: rows}))
            removed = launch(torch, pair, "mixed", arm, d, 0.05, dict(sc, **{key: np.delete(sc[key], place, axis=0)}))
            at = place + (S if key == "capsules" else 0)
            assert (got["nearest"][..., 1] != at).all(), (key, place, "a skipped obstacle is never the nearest")
            shifted = got["nearest"].copy()
            shifted[..., 1] -= got["nearest"][..., 1] > at
            same(dict(got, nearest=shifted), removed, f"{key} {place} {val}")
    dead = dict(spheres=np.array([[np.nan, 0.0, 0.0, 0.1], [0.3, 0.0, 0.0, -1.0]]), capsules=np.array([[0.0, 0.0, np.inf, 0.1, 0.1, 0.1, 0.05]]))
    got = launch(torch, pair, "mixed", arm, d, 0.05, dead)
    assert np.isposinf(got["clearance"]).all() and np.isposinf(got["min_clearance"]).all() and (got["nearest"] == -1).all()
    same({o: got[o] for o in SHARED}, launch_track(torch, pair, "mixed", arm, d, 0.05), "every obstacle unusable")


@pytest.mark.parametrize("kind", ["r", "mixed"])
def test_trajectories_that_are_not_numbers(torch_mod, kind):
    """A NaN, a +inf and a -inf in start_joints, in the rest_joints row and in the damping entry, and damping values of 0 and -1, at
    trajectories 0, 63, 64 and the last of 257: those trajectories are NaN in every double output and (-1, -1) in nearest_steps, every
    other carries the clean run's bits."""
    torch = torch_mod
    pair, n, steps = "default/default", 257, 3
    arm = kind_arm(kind, n)
    sc = CW.scene(pair, "open")
    d = inputs(pair, n, steps, arm, ALL)
    lam = np.full(n, 0.05)
    base = launch(torch, pair, kind, arm, d, lam, sc)
    same(launch(torch, pair, kind, arm, d, 0.05, sc), base, "damping array against damping_host")
    hit = np.zeros(n, dtype=bool)
    hit[list(PLACES)] = True
    values = {"start": (np.nan, np.inf, -np.inf), "rest": (np.nan, np.inf, -np.inf), "damping": (np.nan, np.inf, -np.inf, 0.0, -1.0)}
    for target, vals in values.items():
        for turn in range(len(vals)):
            a = {"start": d["start"].copy(), "rest": d["rest"].copy(), "damping": lam.copy()}
            for i, row in enumerate(PLACES):
                val = vals[(i + turn) % len(vals)]
                if target == "damping":
                    a[target][row] = val
                else:
                    a[target][row, (i + turn) % 7] = val
            for want in (OUTS, ("clearance",), ("min_clearance", "nearest")):
                got = launch(torch, pair, kind, arm, dict(d, start=a["start"], rest=a["rest"]), a["damping"], sc, want=want)
                for o in want:
                    g, b = (per_traj(x[o], n) for x in (got, base))
                    if o == "nearest":
                        assert (g[:, hit] == -1).all(), (kind, target, turn, o)
                    else:
                        assert np.isnan(g[:, hit]).all(), (kind, target, turn, o, "a trajectory that is not numbers must be NaN everywhere")
                    assert np.array_equal(bits(np.ascontiguousarray(g[:, ~hit])), bits(np.ascontiguousarray(b[:, ~hit]))), (kind, target, turn, o)


@pytest.mark.parametrize("target", ["goal", "feedforward"])
def test_steps_that_are_not_numbers(torch_mod, target):
    """A NaN, a +inf or a -inf in a goal or a feed-forward entry at step 0, at a middle step and at the last step of 5, at trajectories
    0, 63, 64 and the last of 257: the step is held (joints the joints before it, rates 0, err NaN) and clearance_steps and
    nearest_steps ARE written on it, with rsik_clearance's bits at the held joints; the rest of that trajectory has the bits of the
    same run with that step removed, and every other trajectory carries the clean run's bits."""
    torch = torch_mod
    pair, n, steps = "default/default", 257, 5
    arm = kind_arm("mixed", n)
    sc = CW.scene(pair, "open")
    d = inputs(pair, n, steps, arm, ALL)
    base = launch(torch, pair, "mixed", arm, d, 0.05, sc)
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
        got = launch(torch, pair, "mixed", arm, dict(d, m12=m12, ff=ff), 0.05, sc)
        keep = [t for t in range(steps) if t != s]
        removed = launch(torch, pair, "mixed", arm, dict(d, m12=np.ascontiguousarray(d["m12"][keep]), ff=np.ascontiguousarray(d["ff"][keep])), 0.05, sc)
        what = (target, s)
        before = d["start"] if s == 0 else got["joints"][s - 1]
        assert np.array_equal(bits(got["joints"][s][hit]), bits(np.ascontiguousarray(before[hit]))), (what, "the joints are held")
        assert (got["rates"][s][hit] == 0.0).all() and np.isnan(got["err"][s][hit]).all(), what
        held = clearance_of(torch, pair, "mixed", arm, before, sc)
        assert np.array_equal(bits(got["clearance"][s]), bits(held["clearance"])) and np.array_equal(got["nearest"][s], held["nearest"]), (what, "held step")
        assert np.isfinite(got["clearance"][s][hit]).all(), what
        for o in ("joints", "rates", "err", "clearance", "nearest"):
            assert np.array_equal(bits(np.ascontiguousarray(got[o][keep][:, hit])), bits(np.ascontiguousarray(removed[o][:, hit]))), (what, o, "step removed")
            assert np.array_equal(bits(np.ascontiguousarray(got[o][:, ~hit])), bits(np.ascontiguousarray(base[o][:, ~hit]))), (what, o)
        for o in ("final_joints", "min_clearance"):
            assert np.array_equal(bits(got[o][hit]), bits(removed[o][hit])) and np.array_equal(bits(got[o][~hit]), bits(base[o][~hit])), (what, o)
        if s == steps - 1 and target == "goal":
            assert np.isnan(got["final_err"][hit]).all(), what
        assert np.array_equal(bits(got["final_err"][~hit]), bits(base["final_err"][~hit])), what


# ------------------------------------------------------------------------------------------ 8. refusals and the surface
def test_refusals(torch_mod):
    """Every RSIK_E_INVALID case of include/rsik.h with the function's name in rsik_last_error; RSIK_E_NOT_SET on a context with no arm;
    n == 0 is RSIK_OK."""
    from reachy2_symbolic_ik_amd import HipSolver

    torch, A = torch_mod, abi()
    solver = solver_of("default/default")
    n, steps = 8, 2
    arm_np = JW.arm_bytes()[:n]
    d = inputs("default/default", n, steps, arm_np, ALL)
    sc = CW.scene("default/default", "open")
    g, q, ff, rest = T(d["m12"], torch), T(d["start"], torch), T(d["ff"], torch), T(d["rest"], torch)
    sp, cp, arm = T(sc["spheres"], torch), T(sc["capsules"], torch), T(arm_np, torch)
    o = torch.empty((steps, n, 7), dtype=torch.float64, device="cuda")
    near = torch.empty((steps, n, 2), dtype=torch.int32, device="cuda")

    def host(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a, a.ctypes.data_as(C.POINTER(C.c_double))

    def args(**kw):
        a = dict(n=n, n_steps=steps, m12=ptr(g), arm=None, arm_uniform=0, start=ptr(q), dt=0.01, kp=50.0, ko=50.0, ff=ptr(ff), damping_host=0.05,
                 damping=None, rest=ptr(rest), rest_gain=1.0, limits=None, radius=None, n_spheres=len(sc["spheres"]), spheres=ptr(sp),
                 n_capsules=len(sc["capsules"]), capsules=ptr(cp), influence=0.05, avoid_gain=10.0, joints=ptr(o), rates=None, err=None,
                 clearance=None, nearest=None, final_joints=None, final_err=None, min_clearance=None)
        a.update(kw)
        return tuple(a.values())

    keep = []
    cases = [("all outputs NULL", args(joints=None)), ("n < 0", args(n=-1)), ("n_steps 0", args(n_steps=0)), ("n_steps 65537", args(n_steps=65537)),
             ("m12_steps NULL", args(m12=None)), ("start_joints NULL", args(start=None)), ("arm_uniform 2", args(arm_uniform=2)),
             ("n_spheres -1", args(n_spheres=-1)), ("n_spheres 257", args(n_spheres=257)), ("n_capsules -1", args(n_capsules=-1)),
             ("n_capsules 65", args(n_capsules=65)), ("no obstacle", args(n_spheres=0, n_capsules=0)),
             ("no obstacle, arrays given", args(n_spheres=0, n_capsules=0, spheres=ptr(sp), capsules=ptr(cp))),
             ("spheres NULL", args(spheres=None)), ("capsules NULL", args(capsules=None)),
             ("nearest_steps not aligned", args(nearest=near.data_ptr() + 4))]
    for name in ("dt", "kp", "ko", "rest_gain", "damping_host", "influence", "avoid_gain"):
        cases += [(f"{name} {v}", args(**{name: v})) for v in (-1.0, np.nan, np.inf)]
    cases += [("dt 0", args(dt=0.0)), ("damping_host 0", args(damping_host=0.0))]
    for bad in ((0, -0.01), (1, np.nan), (2, np.inf)):
        r = np.array(AW.LINK_RADIUS)
        r[bad[0]] = bad[1]
        keep.append(host(r))
        cases.append((f"link radius {bad}", args(radius=keep[-1][1])))
    lim = np.array(TW.LIMITS)
    lim[0, 3] = 0.0
    keep.append(host(lim))
    cases.append(("rate_max 0", args(limits=keep[-1][1])))
    for what, cargs in cases:
        assert raw_call(solver, "rsik_track_avoid", *cargs) == A.RSIK_E_INVALID, what
        assert "rsik_track_avoid" in last_error(solver), (what, last_error(solver))
    assert raw_call(solver, "rsik_track_avoid", *args(n=0, m12=None, start=None, joints=None)) == A.RSIK_OK
    assert raw_call(solver, "rsik_track_avoid", *args(n_capsules=0, capsules=None, influence=0.0, avoid_gain=0.0)) == A.RSIK_OK
    assert raw_call(solver, "rsik_track_avoid", *args(joints=None, nearest=ptr(near), arm=ptr(arm))) == A.RSIK_OK
    radius = host(AW.LINK_RADIUS)
    assert raw_call(solver, "rsik_track_avoid", *args(radius=radius[1], rest=None, rest_gain=np.nan)) == A.RSIK_OK
    bare = HipSolver(0)
    assert raw_call(bare, "rsik_track_avoid", *args()) == A.RSIK_E_NOT_SET
    assert raw_call(bare, "rsik_track_avoid", *args(arm=ptr(arm))) == A.RSIK_E_NOT_SET
    torch.cuda.synchronize()
    bare.close()


def test_python_surface(torch_mod):
    """SymbolicIK.track_avoid_batch and DualArmIK.track_avoid_batch are HipSolver.track_avoid on their arms (goals as [T,12,n] or as
    matrices [T,n,4,4]); out= buffers are written in place; a planned launch writes the same bits; the default is the joints alone."""
    from reachy2_symbolic_ik_amd import DualArmIK, SymbolicIK

    torch = torch_mod
    pair, n, steps = "default/default", 130, 4
    solver = solver_of(pair)
    sc = CW.scene(pair, "open")
    arm = kind_arm("mixed", n)
    with contextlib.redirect_stdout(io.StringIO()):
        ik_l = SymbolicIK("l_arm", solver=solver, **arm_pairs.DEFAULT)
        dual = DualArmIK(solver=solver, **arm_pairs.DEFAULT)
    dl = inputs(pair, n, steps, kind_arm("l", n), ALL)
    kw = dict(spheres=sc["spheres"], capsules=sc["capsules"], link_radius=AW.LINK_RADIUS, influence=AW.INFLUENCE, avoid_gain=AW.AVOID_GAIN)
    terms = dict(feedforward=dl["ff"], rest_joints=dl["rest"], rest_gain=dl["rest_gain"], limits=dl["limits"])
    res = ik_l.track_avoid_batch(dl["m12"], dl["start"], TW.DT, TW.KP, TW.KO, 0.05, **kw, **terms)
    assert tuple(res) == ("joints",)
    want = launch(torch, pair, "l", kind_arm("l", n), dl, 0.05, sc)
    same({"joints": res["joints"].cpu().numpy()}, {"joints": want["joints"]}, "SymbolicIK.track_avoid_batch")
    M = np.zeros((steps, n, 4, 4))
    M[..., :3, :3], M[..., :3, 3], M[..., 3, 3] = dl["R"], dl["p"], 1.0
    res = ik_l.track_avoid_batch(M, dl["start"], TW.DT, TW.KP, TW.KO, 0.05, want=OUTS, **kw, **terms)
    same({k: a.cpu().numpy() for k, a in res.items()}, want, "SymbolicIK.track_avoid_batch on matrices")
    d = inputs(pair, n, steps, arm, NONE)
    got = {k: a.cpu().numpy() for k, a in dual.track_avoid_batch(arm, d["m12"], d["start"], TW.DT, TW.KP, TW.KO, 0.05, want=OUTS, **kw).items()}
    same(got, launch(torch, pair, "mixed", arm, d, 0.05, sc), "DualArmIK.track_avoid_batch")
    out = {"clearance": torch.full((steps, n), 7.0, dtype=torch.float64, device="cuda")}
    call = dict(damping=0.05, arm=T(arm, torch), **{k: (T(v, torch) if k in ("spheres", "capsules") else v) for k, v in kw.items()})
    res = solver.track_avoid(T(d["m12"], torch), T(d["start"], torch), TW.DT, TW.KP, TW.KO, want=("clearance", "min_clearance"), out=out, **call)
    assert res["clearance"] is out["clearance"] and tuple(res) == ("clearance", "min_clearance")
    plan = solver.track_avoid(T(d["m12"], torch), T(d["start"], torch), TW.DT, TW.KP, TW.KO, want=("clearance",), plan_only=True, **call)
    plan["launch"]()
    torch.cuda.synchronize()
    assert np.array_equal(bits(plan["clearance"].cpu().numpy()), bits(out["clearance"].cpu().numpy()))
    assert np.array_equal(bits(out["clearance"].cpu().numpy()), bits(got["clearance"]))
    for bad in (dict(want=()), dict(want=("witness",)), dict(damping=None), dict(dt=0.0), dict(influence=-1.0), dict(avoid_gain=float("nan")),
                dict(spheres=None, capsules=None), dict(spheres=torch.zeros((257, 4), dtype=torch.float64)),
                dict(capsules=torch.zeros((65, 7), dtype=torch.float64)), dict(link_radius=(0.1, -0.1, 0.1))):
        a = {"dt": TW.DT, "kp": TW.KP, "ko": TW.KO, **call, **bad}
        with pytest.raises(ValueError):
            solver.track_avoid(T(d["m12"], torch), T(d["start"], torch), **a)


def test_integration_md_snippet(torch_mod):
    """The avoidance snippet of INTEGRATION.md as written, on the tracking snippet's goals and the clearance snippet's scene: the shapes;
    clearance is rsik_clearance's at the joints before each step; with the scene 10 m away the joints are track_batch's bits; and on
    the trajectories the push acts on, the clearance at the last step is on the median no smaller than without the push, and
    larger by more than 1 mm on some."""
    from reachy2_symbolic_ik_amd import SymbolicIK

    torch = torch_mod
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", solver=solver_of("default/default"), **arm_pairs.DEFAULT)
    pos, eul, arm, _ = JW.link_poses()
    poses = np.ascontiguousarray(np.stack([pos[arm == 0], eul[arm == 0]], axis=1))[:130]

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
    spheres = torch.tensor([[0.35, -0.25, -0.30, 0.10], [0.10, 0.00, 0.05, 0.15]], dtype=torch.float64)
    table = torch.tensor([[0.2, -0.6, -0.45, 0.2, 0.6, -0.45, 0.05]], dtype=torch.float64)
    radius = (0.05, 0.04, 0.03)
    run = ik.track_avoid_batch(goals, q, dt=dt, kp=20.0, ko=20.0, damping=0.02, spheres=spheres, capsules=table, link_radius=radius,
                               influence=0.10, avoid_gain=20.0, feedforward=ff, limits=limits,
                               want=("joints", "clearance", "nearest", "min_clearance", "final_err"))
    hit = run["min_clearance"] < 0.0

    assert tuple(run["joints"].shape) == (T_, n, 7) and tuple(run["clearance"].shape) == (T_, n) and tuple(run["nearest"].shape) == (T_, n, 2)
    assert tuple(run["min_clearance"].shape) == (n,) and hit.dtype == torch.bool
    ok = torch.isfinite(q).all(dim=1)
    assert int(ok.sum()) * 2 >= n and torch.isnan(run["min_clearance"][~ok]).all() and torch.isfinite(run["min_clearance"][ok]).all()
    before = torch.cat([q[None], run["joints"][:-1]])
    c = ik.clearance_batch(before, spheres, table, radius, want=("clearance",))["clearance"]
    assert torch.equal(c[:, ok].contiguous().view(torch.int64), run["clearance"][:, ok].contiguous().view(torch.int64))
    plain = ik.track_batch(goals, q, dt=dt, kp=20.0, ko=20.0, damping=0.02, feedforward=ff, limits=limits, want=("joints",))["joints"]
    away = torch.tensor([10.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    far = ik.track_avoid_batch(goals, q, dt=dt, kp=20.0, ko=20.0, damping=0.02, spheres=spheres + away, capsules=table + torch.cat([away[:3], away]),
                               link_radius=radius, influence=0.10, avoid_gain=20.0, feedforward=ff, limits=limits, want=("joints",))["joints"]
    assert torch.equal(plain[:, ok].contiguous().view(torch.int64), far[:, ok].contiguous().view(torch.int64))
    pushed = ok & (run["clearance"] < 0.10).any(dim=0)
    blind = ik.track_avoid_batch(goals, q, dt=dt, kp=20.0, ko=20.0, damping=0.02, spheres=spheres, capsules=table, link_radius=radius,
                                 influence=0.10, avoid_gain=0.0, feedforward=ff, limits=limits, want=("clearance",))["clearance"]
    gain = (run["clearance"][-1] - blind[-1])[pushed]
    print(f"INTEGRATION.md avoidance snippet: {int(ok.sum())} trajectories, {int(pushed.sum())} pushed, clearance at the last step against "
          f"the run without the push: median {float(gain.median()):+.4f} m, largest {float(gain.max()):+.4f} m, smallest {float(gain.min()):+.4f} m")
    assert int(pushed.sum()) > 0 and float(gain.median()) >= 0.0 and float(gain.max()) > 1e-3
