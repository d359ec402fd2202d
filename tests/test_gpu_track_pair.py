"""GPU tests (-m gpu, MI355X) of rsik_track_pair (csrc/rsik_kernel_track_pair.hpp): both arms of n_pairs robots tracked in one launch,
each avoiding the static scene and the other arm — against rsik_clearance, rsik_track_avoid and rsik_track bit for bit, against the
NumPy reference and the tolerances of tests/track_pair_workload.py (pinned on the CPU alone by tests/test_track_pair_abi.py), and
against itself bit for bit.

Shapes, small on purpose: n_pairs in {1, 31, 32, 33, 129} (a wave holds 32 pairs), n_steps in {1, 2, 33}; static scenes: none, one sphere,
clearance_workload's "open" scene and a full one of 256 spheres and 64 capsules.  Rows are interleaved: 2i the right arm of robot i,
2i + 1 its left arm."""
import contextlib
import ctypes as C
import io
import itertools

import numpy as np
import pytest

import arm_pairs
import clearance_workload as CW
import track_avoid_workload as AW
import track_pair_workload as PW
import track_workload as TW
from compare import bits
from gpu_support import T, abi, last_error, ptr, raw_call, torch_mod  # noqa: F401
from track_support import ALL, NONE, inputs, same, solver_of
from track_support import launch as launch_track
from track_support import solvers_do_not_outlive_the_module  # noqa: F401

pytestmark = pytest.mark.gpu

OUTS = ("joints", "rates", "err", "clearance", "nearest", "final_joints", "final_err", "min_clearance")
SHARED = ("joints", "rates", "err", "final_joints", "final_err")
PER_ROW = ("final_joints", "final_err", "min_clearance")
N_PAIRS = (1, 31, 32, 33, 129)
STEPS = (1, 2, 33)
PLACES = (0, 31, 32, 128)
SCENES = ("none", "sphere", "open", "full")


def pair_inputs(pair, n_pairs, n_steps, terms):
    return inputs(pair, 2 * n_pairs, n_steps, PW.arm_bytes(n_pairs), terms)


def _scene_kw(sc, torch):
    t = lambda a: None if a is None or not len(a) else T(a, torch)  # noqa: E731
    return dict(spheres=t(sc["spheres"]), capsules=t(sc["capsules"]))


def launch(torch, pair, d, lam, sc, want=OUTS, influence=AW.INFLUENCE, avoid_gain=AW.AVOID_GAIN, radius=AW.LINK_RADIUS, dt=TW.DT, kp=TW.KP,
           ko=TW.KO):
    """One launch through HipSolver.track_pair on a launch's inputs d (interleaved rows) and a static scene; the results on the host."""
    t = lambda a: None if a is None else T(a, torch)  # noqa: E731
    res = solver_of(pair).track_pair(T(d["m12"], torch), T(d["start"], torch), dt, kp, ko, damping=lam if isinstance(lam, float) else T(lam, torch),
                                     link_radius=radius, influence=influence, avoid_gain=avoid_gain, feedforward=t(d["ff"]),
                                     rest_joints=t(d["rest"]), rest_gain=d["rest_gain"], limits=d["limits"], want=want, **_scene_kw(sc, torch))
    torch.cuda.synchronize()
    assert tuple(res) == tuple(o for o in OUTS if o in want), (tuple(res), want)
    return {k: a.cpu().numpy() for k, a in res.items()}


def launch_avoid(torch, pair, d, lam, sc, want=OUTS, influence=AW.INFLUENCE, avoid_gain=AW.AVOID_GAIN, radius=AW.LINK_RADIUS):
    """rsik_track_avoid on the same buffers with the arm bytes 0, 1, 0, 1, ...; the results on the host."""
    t = lambda a: None if a is None else T(a, torch)  # noqa: E731
    n = d["start"].shape[0]
    res = solver_of(pair).track_avoid(T(d["m12"], torch), T(d["start"], torch), TW.DT, TW.KP, TW.KO,
                                      damping=lam if isinstance(lam, float) else T(lam, torch), link_radius=radius, influence=influence,
                                      avoid_gain=avoid_gain, feedforward=t(d["ff"]), rest_joints=t(d["rest"]), rest_gain=d["rest_gain"],
                                      limits=d["limits"], want=want, arm=T(PW.arm_bytes(n // 2), torch), **_scene_kw(sc, torch))
    torch.cuda.synchronize()
    return {k: a.cpu().numpy() for k, a in res.items()}


def rows_of(a, o, rows):
    """The rows (trajectories) `rows` of output o."""
    return np.ascontiguousarray(a[rows] if o in PER_ROW else a[:, rows])


def pairs_alone(d, pairs):
    """The inputs of the robots `pairs` of a launch's inputs d, as a launch of their own."""
    rows = np.stack([2 * np.asarray(pairs), 2 * np.asarray(pairs) + 1], axis=1).reshape(-1)
    return rows, {k: (a if a is None or k in ("rest_gain", "limits") else np.ascontiguousarray(
        a[:, rows] if k in ("R", "p", "ff") else a[..., rows] if k == "m12" else a[rows])) for k, a in d.items()}


def check_against_clearance(torch, pair, d, got, sc, pairs, what, radius=AW.LINK_RADIUS):
    """clearance_steps[t], nearest_steps[t] and min_clearance of the robots `pairs` against rsik_clearance, bit for bit: one batched
    launch gives link_points on the joints before every step and at the end; then, per robot, arm and step, rsik_clearance with n = 1 on
    that row, its capsules the static ones followed by the partner's three, (P_l, P_{l+1}, r_l)."""
    solver = solver_of(pair)
    steps, n = got["joints"].shape[:2]
    before = np.concatenate([d["start"][None], got["joints"]])  # [steps + 1, n, 7]: before step t, and the final joints
    assert np.array_equal(bits(before[-1]), bits(got["final_joints"])), what
    lp = solver.clearance(T(before, torch), spheres=T(np.array([[9.0, 9.0, 9.0, 0.1]]), torch), arm=T(PW.arm_bytes(n // 2), torch),
                          want=("link_points",))["link_points"].cpu().numpy()
    sp = None if not len(sc["spheres"]) else T(sc["spheres"], torch)
    for i, side in itertools.product(pairs, (0, 1)):
        r = 2 * i + side
        seen = np.empty(steps + 1)
        for t in range(steps + 1):
            caps = np.concatenate([sc["capsules"], PW.partner_capsules(lp[t, r ^ 1], radius)])
            one = solver.clearance(T(before[t, r:r + 1], torch), spheres=sp, capsules=T(caps, torch), link_radius=radius, arm_uniform=side,
                                   want=("clearance", "nearest"))
            c, near = one["clearance"].cpu().numpy(), one["nearest"].cpu().numpy()
            seen[t] = c[0]
            if t < steps:
                assert np.array_equal(bits(c), bits(got["clearance"][t, r:r + 1])), (what, "clearance", i, side, t, float(c[0]), float(got["clearance"][t, r]))
                assert np.array_equal(near[0], got["nearest"][t, r]), (what, "nearest", i, side, t, near[0].tolist(), got["nearest"][t, r].tolist())
        assert np.array_equal(bits(np.array([seen.min()])), bits(got["min_clearance"][r:r + 1])), (what, "min_clearance", i, side)


# ------------------------------------------------------------------------------------------ 1. shapes and bits
@pytest.mark.parametrize("terms", [NONE, ALL])
def test_every_shape_and_its_bits(torch_mod, terms):
    """Every n_pairs and n_steps, the four static scenes and the arm pairs rotating over them: the shapes and dtypes of the eight
    outputs; a second launch and each output alone are bit for bit; final_joints has the bits of joints_steps[-1]; a permutation of
    the static obstacles leaves clearance_steps and min_clearance unchanged; robots 0, 31, 32 and 128 of n_pairs = 129 equal the same
    robot launched alone, and a permutation of the robots permutes the outputs."""
    torch = torch_mod
    rng = np.random.default_rng(7311)
    for i, (n_pairs, n_steps) in enumerate(itertools.product(N_PAIRS, STEPS)):
        pair = AW.PAIRS[i % len(AW.PAIRS)]
        name = SCENES[(i // 3 + i) % 4]
        sc = PW.scene_of(pair, name)
        n = 2 * n_pairs
        what = f"{pair} n_pairs={n_pairs} n_steps={n_steps} scene={name} terms={terms}"
        d = pair_inputs(pair, n_pairs, n_steps, terms)
        got = launch(torch, pair, d, 0.05, sc)
        assert got["joints"].shape == got["rates"].shape == (n_steps, n, 7) and got["err"].shape == (n_steps, n, 2), what
        assert got["clearance"].shape == (n_steps, n) and got["nearest"].shape == (n_steps, n, 2) and got["nearest"].dtype == np.int32, what
        assert got["final_joints"].shape == (n, 7) and got["final_err"].shape == (n, 2) and got["min_clearance"].shape == (n,), what
        assert all(np.isfinite(a).all() for a in got.values()) and (got["nearest"] >= 0).all(), what
        assert (got["nearest"][..., 1] < len(sc["spheres"]) + len(sc["capsules"]) + 3).all() and (got["nearest"][..., 0] < 3).all(), what
        assert np.array_equal(bits(got["final_joints"]), bits(got["joints"][-1])), (what, "final_joints")
        assert (got["min_clearance"] <= got["clearance"].min(axis=0)).all(), what
        same(launch(torch, pair, d, 0.05, sc), got, what + " twice")
        for o in OUTS:
            same(got, launch(torch, pair, d, 0.05, sc, want=(o,)), what + f" {o} alone")
        if name != "none":
            order_s, order_c = rng.permutation(len(sc["spheres"])), rng.permutation(len(sc["capsules"]))
            mixed_up = launch(torch, pair, d, 0.05, dict(spheres=sc["spheres"][order_s], capsules=sc["capsules"][order_c]),
                              want=("clearance", "min_clearance"), avoid_gain=0.0)
            same(mixed_up, launch(torch, pair, d, 0.05, sc, want=("clearance", "min_clearance"), avoid_gain=0.0), what + " obstacles permuted")
        if n_pairs == 129:
            for place in PLACES:
                rows, cut = pairs_alone(d, [place])
                alone = launch(torch, pair, cut, 0.05, sc)
                for o in OUTS:
                    assert np.array_equal(bits(alone[o]), bits(rows_of(got[o], o, rows))), (what, o, f"robot {place} launched alone")
            order = rng.permutation(n_pairs)
            rows, cut = pairs_alone(d, order)
            moved = launch(torch, pair, cut, 0.05, sc)
            for o in OUTS:
                assert np.array_equal(bits(moved[o]), bits(rows_of(got[o], o, rows))), (what, o, "the robots permuted")


# ------------------------------------------------------------------------------------------ 2. prefix
@pytest.mark.parametrize("terms", [NONE, ALL])
def test_prefix_property(torch_mod, terms):
    """The n_steps = 33 run equals an n_steps = 16 run followed by an n_steps = 17 run started from its final_joints, bit for bit
    (n_pairs = 129, the "open" scene), min_clearance being the smaller of the two parts'."""
    torch = torch_mod
    pair, n_pairs = "custom/custom", 129
    sc = CW.scene(pair, "open")
    d = pair_inputs(pair, n_pairs, 33, terms)
    whole = launch(torch, pair, d, 0.05, sc)

    def part(lo, hi, start):
        cut = dict(d, m12=np.ascontiguousarray(d["m12"][lo:hi]), start=start, ff=None if d["ff"] is None else np.ascontiguousarray(d["ff"][lo:hi]))
        return launch(torch, pair, cut, 0.05, sc)

    a = part(0, 16, d["start"])
    b = part(16, 33, a["final_joints"])
    for o in ("joints", "rates", "err", "clearance", "nearest"):
        assert np.array_equal(bits(np.concatenate([a[o], b[o]])), bits(whole[o])), (terms, o, "16 steps and then 17")
    for o in ("final_joints", "final_err"):
        assert np.array_equal(bits(b[o]), bits(whole[o])), (terms, o)
    assert np.array_equal(bits(np.minimum(a["min_clearance"], b["min_clearance"])), bits(whole["min_clearance"]))
    assert (whole["clearance"] < AW.INFLUENCE).any() and (whole["clearance"] >= AW.INFLUENCE).any()
    assert (whole["nearest"][..., 1] >= len(sc["spheres"]) + len(sc["capsules"])).any(), "a link of the partner's is the nearest somewhere"


# ------------------------------------------------------------------------------------------ 3. against rsik_clearance
@pytest.mark.parametrize("name", ["none", "open"])
def test_clearance_and_nearest_are_rsik_clearance_s_bits(torch_mod, name):
    """Robots 0, 15, 16 and 32 of n_pairs = 33, 6 steps, with feed-forward, rest and limits: clearance_steps[t], nearest_steps[t] and
    min_clearance are rsik_clearance's bits for the row's joints before step t with the static capsules followed by the partner's
    three links at ITS joints before step t (check_against_clearance).  Both sides occur: the partner the nearest, and not."""
    torch = torch_mod
    pair, n_pairs, n_steps = "default/ztip", 33, 6
    sc = PW.scene_of(pair, name)
    d = pair_inputs(pair, n_pairs, n_steps, ALL)
    got = launch(torch, pair, d, 0.05, sc)
    check_against_clearance(torch, pair, d, got, sc, (0, 15, 16, 32), name)
    partner = got["nearest"][..., 1] >= len(sc["spheres"]) + len(sc["capsules"])
    assert partner.any() and (name == "none" or (~partner).any())
    assert (got["clearance"] < AW.INFLUENCE).any() and (got["clearance"] >= AW.INFLUENCE).any()


# ------------------------------------------------------------------------------------------ 4. against rsik_track_avoid and rsik_track
@pytest.mark.parametrize("terms", [NONE, ALL])
def test_without_a_partner_the_bits_are_rsik_track_avoid_s_and_rsik_track_s(torch_mod, terms):
    """Every left row's start_joints NaN: the right rows of all eight outputs equal rsik_track_avoid on the same buffers (arm bytes 0, 1,
    ..., the same static scene), the left rows are NaN and (-1, -1); the same with the arms the other way round.  Without a static
    scene the five shared outputs equal rsik_track's, clearance is +inf and nearest -1.  A NaN in one robot's rest row or damping
    entry does the same to that robot only: every other robot keeps the clean run's bits."""
    torch = torch_mod
    pair, n_pairs, n_steps = "default/default", 33, 6
    n = 2 * n_pairs
    arm = PW.arm_bytes(n_pairs)
    d = pair_inputs(pair, n_pairs, n_steps, terms)
    sc = CW.scene(pair, "open")
    for side in (0, 1):
        live, dead = np.flatnonzero(arm == side), np.flatnonzero(arm != side)
        start = d["start"].copy()
        start[dead, (3 + side) % 7] = np.nan
        cut = dict(d, start=start)
        got, ref = launch(torch, pair, cut, 0.05, sc), launch_avoid(torch, pair, cut, 0.05, sc)
        assert (ref["clearance"][:, live] < AW.INFLUENCE).any(), "rsik_track_avoid pushes some of the live rows"
        for o in OUTS:
            assert np.array_equal(bits(rows_of(got[o], o, live)), bits(rows_of(ref[o], o, live))), (terms, side, o, "rsik_track_avoid's bits")
            if o == "nearest":
                assert (rows_of(got[o], o, dead) == -1).all(), (terms, side, o)
            else:
                assert np.isnan(rows_of(got[o], o, dead)).all(), (terms, side, o)
        bare = launch(torch, pair, cut, 0.05, PW.NO_SCENE)
        plain = launch_track(torch, pair, "mixed", arm, cut, 0.05)
        for o in SHARED:
            assert np.array_equal(bits(rows_of(bare[o], o, live)), bits(rows_of(plain[o], o, live))), (terms, side, o, "rsik_track's bits")
        assert np.isposinf(bare["clearance"][:, live]).all() and np.isposinf(bare["min_clearance"][live]).all(), (terms, side)
        assert (bare["nearest"] == -1).all() and np.isnan(bare["clearance"][:, dead]).all(), (terms, side)
    if terms == ALL:
        lam = np.full(n, 0.05)
        clean = launch(torch, pair, d, lam, sc)
        same(launch(torch, pair, d, 0.05, sc), clean, "damping array against damping_host")
        hit_rows = (0, 31, 62, 65)  # (robots 0, 15, 31 and 32: the right arm, the left, the right, the left)
        for target, val in (("rest", np.nan), ("rest", -np.inf), ("damping", np.nan), ("damping", 0.0)):
            rest, damping = d["rest"].copy(), lam.copy()
            for r in hit_rows:
                if target == "rest":
                    rest[r, r % 7] = val
                else:
                    damping[r] = val
            cut = dict(d, rest=rest)
            got, ref = launch(torch, pair, cut, damping, sc), launch_avoid(torch, pair, cut, damping, sc)
            touched = np.zeros(n, dtype=bool)
            for r in hit_rows:
                touched[[r, r ^ 1]] = True
                for o in OUTS:
                    g = rows_of(got[o], o, [r])
                    assert (g == -1).all() if o == "nearest" else np.isnan(g).all(), (target, val, r, o)
                    assert np.array_equal(bits(rows_of(got[o], o, [r ^ 1])), bits(rows_of(ref[o], o, [r ^ 1]))), (target, val, r, o, "the partner of a NaN arm")
            for o in OUTS:
                assert np.array_equal(bits(rows_of(got[o], o, ~touched)), bits(rows_of(clean[o], o, ~touched))), (target, val, o, "every other robot")


# ------------------------------------------------------------------------------------------ 5. both arms see each other
def test_both_arms_see_each_other(torch_mod):
    """Where row 2i names the partner's link b with its own link a and row 2i + 1 names the partner's link a with its own link b, the two
    clearances are the same pair of segments with the roles swapped: they differ by at most 2 CLEARANCE_BOUND.  Such cells exist
    (n_pairs = 129, 33 steps, no static scene and the "open" one)."""
    torch = torch_mod
    for pair, name in (("default/default", "none"), ("custom/custom", "open")):
        sc = PW.scene_of(pair, name)
        m = len(sc["spheres"]) + len(sc["capsules"])
        got = launch(torch, pair, pair_inputs(pair, 129, 33, NONE), 0.05, sc, want=("clearance", "nearest"))
        link, obs = got["nearest"][..., 0], got["nearest"][..., 1] - m
        mutual = (obs[:, 0::2] >= 0) & (obs[:, 1::2] >= 0) & (link[:, 0::2] == obs[:, 1::2]) & (link[:, 1::2] == obs[:, 0::2])
        diff = np.abs(got["clearance"][:, 0::2] - got["clearance"][:, 1::2])[mutual]
        print(f"{pair} scene={name}: {int(mutual.sum())} of {mutual.size} cells name each other, largest difference {diff.max():.3e}")
        assert mutual.sum() >= mutual.size // 10, int(mutual.sum())
        assert (diff <= 2 * CW.CLEARANCE_BOUND).all(), float(diff.max())


# ------------------------------------------------------------------------------------------ 6. per step, against the reference
@pytest.mark.parametrize("case", PW.STEP_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{'terms' if c[2] else 'plain'}")
@pytest.mark.parametrize("pair", AW.PAIRS)
def test_every_step_against_the_reference(torch_mod, pair, case):
    """The device's own joints before step t fed into the reference's one step (track_pair_workload.one_step): on the kept cells
    joints_steps[t] is within tol_t (track_avoid_workload.step_tolerance), the clearance within CLEARANCE_BOUND on every cell, and the
    device takes the reference's side of the select, at lambda 1e-3 and 0.05 (N_STEP robots, T_STEP steps).  At least 0.8 of the cells
    are kept and at least 0.1 are kept and pushed with a link of the partner's as the nearest.  Prints the worst error / tolerance."""
    torch = torch_mod
    name, influence, with_terms = case
    n, n_steps = 2 * PW.N_STEP, PW.T_STEP
    sc = PW.scene_of(pair, name)
    m = len(sc["spheres"]) + len(sc["capsules"])
    d = pair_inputs(pair, PW.N_STEP, n_steps, ALL if with_terms else NONE)
    for lam in TW.LAMBDAS:
        got = launch(torch, pair, d, lam, sc, influence=influence)
        worst, compared, partner = 0.0, 0, 0
        for t in range(n_steps):
            before = d["start"] if t == 0 else got["joints"][t - 1]
            ref = PW.one_step(pair, before, d["R"][t], d["p"][t], lam, sc, influence=influence, **AW.terms_of(d, t))
            tol, keep = AW.step_tolerance(ref, before, lam, influence=influence), AW.kept(ref, influence)
            assert (np.abs(got["clearance"][t] - ref["clearance"]) <= CW.CLEARANCE_BOUND).all(), (pair, case, lam, t, "clearance")
            e = np.linalg.norm(got["joints"][t] - ref["joints"], axis=1)
            worst, compared = max(worst, float((e / tol)[keep].max())), compared + int(keep.sum())
            partner += int((keep & ref["push"] & (ref["nearest"][:, 1] >= m)).sum())
            assert (e[keep] <= tol[keep]).all(), (pair, case, lam, t, float((e / tol)[keep].max()))
            assert np.array_equal((got["clearance"][t] < influence)[keep], ref["push"][keep]), (pair, case, lam, t, "the side of the select")
            assert np.array_equal(got["nearest"][t][keep & ref["push"]], ref["nearest"][keep & ref["push"]]), (pair, case, lam, t, "the nearest pair")
        print(f"{pair} {case} lambda={lam}: {compared} of {n * n_steps} cells compared, {partner} pushed by the partner, worst error / tol_t {worst:.3g}")
        assert compared >= 0.8 * n * n_steps and partner >= 0.1 * n * n_steps, (compared, partner)


# ------------------------------------------------------------------------------------------ 7. it avoids
@pytest.mark.parametrize("pair", AW.PAIRS)
def test_it_avoids(torch_mod, pair):
    """The crossing case (constant goals, 64 steps, no static scene), on the robots whose min_clearance (the smaller of the two arms')
    the reference raises by at least 1 cm: the device's with avoidance exceeds the device's without by at least half the reference's
    gain, and final_err is within the reference's final_err + 2e-9."""
    torch = torch_mod
    c = PW.crossing_case(pair)
    pairs = c["pairs"]
    assert pairs.sum() >= 16
    d = dict(m12=TW.m12_of(c["R"], c["p"]), start=c["start"], ff=None, rest=None, rest_gain=0.0, limits=None)
    kw = dict(want=("min_clearance", "final_err"), influence=PW.CROSS_INFLUENCE, kp=PW.CROSS_KP, ko=PW.CROSS_KP)
    free = launch(torch, pair, d, TW.LAM_RUN, PW.NO_SCENE, avoid_gain=0.0, **kw)
    avoid = launch(torch, pair, d, TW.LAM_RUN, PW.NO_SCENE, avoid_gain=PW.CROSS_GAIN, **kw)
    gain = avoid["min_clearance"].reshape(-1, 2).min(axis=1) - free["min_clearance"].reshape(-1, 2).min(axis=1)
    over = (avoid["final_err"] - c["avoid"]["final_err"]).reshape(-1, 2, 2).max(axis=1)
    print(f"{pair}: {int(pairs.sum())} robots, device gain / reference gain at least {(gain / c['gain'])[pairs].min():.4f}, "
          f"final_err above the reference's by at most {over[pairs].max():.3e}")
    assert (gain[pairs] >= 0.5 * c["gain"][pairs]).all(), (pair, float((gain / c["gain"])[pairs].min()))
    assert (over[pairs] <= 2e-9).all(), (pair, float(over[pairs].max()))


# ------------------------------------------------------------------------------------------ 8. steps that are not numbers
@pytest.mark.parametrize("target", ["goal", "feedforward"])
def test_steps_that_are_not_numbers(torch_mod, target):
    """A NaN, a +inf or a -inf in ONE arm's goal or feed-forward at step 0, at a middle step and at the last step of 5, at robots 0, 15,
    16 and 32 of 33 (the right arm and the left in turn): that arm's step is held (joints the joints before it, rates 0, err NaN); its
    partner takes the step and sees the held arm's links, at that step and at the next (rsik_clearance's bits,
    check_against_clearance); every other robot keeps the clean run's bits."""
    torch = torch_mod
    pair, n_pairs, steps = "default/default", 33, 5
    n = 2 * n_pairs
    sc = CW.scene(pair, "open")
    d = pair_inputs(pair, n_pairs, steps, ALL)
    base = launch(torch, pair, d, 0.05, sc)
    robots = (0, 15, 16, 32)
    hit_rows = np.array([2 * i + (k % 2) for k, i in enumerate(robots)])
    touched = np.zeros(n, dtype=bool)
    touched[hit_rows], touched[hit_rows ^ 1] = True, True
    vals = (np.nan, np.inf, -np.inf)
    for s in (0, 2, steps - 1):
        m12, ff = d["m12"].copy(), d["ff"].copy()
        for i, row in enumerate(hit_rows):
            if target == "goal":
                m12[s, (5 * i + s) % 12, row] = vals[(i + s) % 3]
            else:
                ff[s, row, (i + s) % 6] = vals[(i + s) % 3]
        cut = dict(d, m12=m12, ff=ff)
        got = launch(torch, pair, cut, 0.05, sc)
        what = (target, s)
        before = d["start"] if s == 0 else got["joints"][s - 1]
        assert np.array_equal(bits(got["joints"][s][hit_rows]), bits(np.ascontiguousarray(before[hit_rows]))), (what, "the joints are held")
        assert (got["rates"][s][hit_rows] == 0.0).all() and np.isnan(got["err"][s][hit_rows]).all(), what
        assert np.isfinite(got["clearance"][s][hit_rows]).all() and np.isfinite(got["joints"]).all(), what
        assert not np.array_equal(bits(got["joints"][s][hit_rows ^ 1]), bits(np.ascontiguousarray(before[hit_rows ^ 1]))), (what, "the partner moves")
        assert np.isfinite(got["err"][s][hit_rows ^ 1]).all(), what
        check_against_clearance(torch, pair, cut, got, sc, robots, what)
        for o in OUTS:
            assert np.array_equal(bits(rows_of(got[o], o, ~touched)), bits(rows_of(base[o], o, ~touched))), (what, o, "every other robot")
        if s == steps - 1 and target == "goal":
            assert np.isnan(got["final_err"][hit_rows]).all(), what


# ------------------------------------------------------------------------------------------ 9. refusals and the surface
def test_refusals(torch_mod):
    """Every RSIK_E_INVALID case of include/rsik.h with the function's name in rsik_last_error; RSIK_E_NOT_SET on a context with one arm
    and with none; n_pairs == 0 and no static obstacle are RSIK_OK."""
    from reachy2_symbolic_ik_amd import HipSolver

    torch, A = torch_mod, abi()
    solver = solver_of("default/default")
    n_pairs, steps = 4, 2
    n = 2 * n_pairs
    d = pair_inputs("default/default", n_pairs, steps, ALL)
    sc = CW.scene("default/default", "open")
    g, q, ff, rest = T(d["m12"], torch), T(d["start"], torch), T(d["ff"], torch), T(d["rest"], torch)
    sp, cp = T(sc["spheres"], torch), T(sc["capsules"], torch)
    o = torch.empty((steps, n, 7), dtype=torch.float64, device="cuda")
    near = torch.empty((steps, n, 2), dtype=torch.int32, device="cuda")

    def host(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a, a.ctypes.data_as(C.POINTER(C.c_double))

    def args(**kw):
        a = dict(n_pairs=n_pairs, n_steps=steps, m12=ptr(g), start=ptr(q), dt=0.01, kp=50.0, ko=50.0, ff=ptr(ff), damping_host=0.05,
                 damping=None, rest=ptr(rest), rest_gain=1.0, limits=None, radius=None, n_spheres=len(sc["spheres"]), spheres=ptr(sp),
                 n_capsules=len(sc["capsules"]), capsules=ptr(cp), influence=0.05, avoid_gain=10.0, joints=ptr(o), rates=None, err=None,
                 clearance=None, nearest=None, final_joints=None, final_err=None, min_clearance=None)
        a.update(kw)
        return tuple(a.values())

    keep = []
    cases = [("all outputs NULL", args(joints=None)), ("n_pairs < 0", args(n_pairs=-1)), ("n_steps 0", args(n_steps=0)),
             ("n_steps 65537", args(n_steps=65537)), ("m12_steps NULL", args(m12=None)), ("start_joints NULL", args(start=None)),
             ("n_spheres -1", args(n_spheres=-1)), ("n_spheres 257", args(n_spheres=257)), ("n_capsules -1", args(n_capsules=-1)),
             ("n_capsules 65", args(n_capsules=65)), ("spheres NULL", args(spheres=None)), ("capsules NULL", args(capsules=None)),
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
        assert raw_call(solver, "rsik_track_pair", *cargs) == A.RSIK_E_INVALID, what
        assert "rsik_track_pair" in last_error(solver), (what, last_error(solver))
    assert raw_call(solver, "rsik_track_pair", *args(n_pairs=0, m12=None, start=None, joints=None)) == A.RSIK_OK
    assert raw_call(solver, "rsik_track_pair", *args(n_spheres=0, n_capsules=0)) == A.RSIK_OK, "zero static obstacles"
    assert raw_call(solver, "rsik_track_pair", *args(n_spheres=0, n_capsules=0, spheres=None, capsules=None, influence=0.0, avoid_gain=0.0)) == A.RSIK_OK
    assert raw_call(solver, "rsik_track_pair", *args(joints=None, nearest=ptr(near))) == A.RSIK_OK
    radius = host(AW.LINK_RADIUS)
    assert raw_call(solver, "rsik_track_pair", *args(radius=radius[1], rest=None, rest_gain=np.nan)) == A.RSIK_OK
    bare = HipSolver(0)
    assert raw_call(bare, "rsik_track_pair", *args()) == A.RSIK_E_NOT_SET, "no arm set"
    assert "rsik_track_pair" in last_error(bare)
    bare.set_arm(0, arm_pairs.packed_blocks("default/default")[0])
    assert raw_call(bare, "rsik_track_pair", *args()) == A.RSIK_E_NOT_SET, "one arm set"
    torch.cuda.synchronize()
    bare.close()


def test_python_surface(torch_mod):
    """DualArmIK.track_pair_batch is HipSolver.track_pair on interleaved rows, bit for bit, on both input forms (per-arm goals as
    [T,12,n_pairs] and as matrices [T,n_pairs,4,4], and already interleaved arrays), every output split into two views; out= buffers
    are written in place; a planned launch writes the same bits; the default is the joints alone."""
    from reachy2_symbolic_ik_amd import DualArmIK

    torch = torch_mod
    pair, n_pairs, steps = "default/default", 65, 4
    n = 2 * n_pairs
    solver = solver_of(pair)
    sc = CW.scene(pair, "open")
    with contextlib.redirect_stdout(io.StringIO()):
        dual = DualArmIK(solver=solver, **arm_pairs.DEFAULT)
    d = pair_inputs(pair, n_pairs, steps, ALL)
    want = launch(torch, pair, d, 0.05, sc)
    kw = dict(spheres=sc["spheres"], capsules=sc["capsules"], link_radius=AW.LINK_RADIUS, influence=AW.INFLUENCE, avoid_gain=AW.AVOID_GAIN,
              rest_gain=d["rest_gain"], limits=d["limits"])

    def joined(res):
        out = {}
        for k, halves in res.items():
            a = np.stack([halves["r"].cpu().numpy(), halves["l"].cpu().numpy()], axis=1 if k in PER_ROW else 2)
            out[k] = a.reshape(want[k].shape)
        return out

    res = dual.track_pair_batch(d["m12"][..., 0::2], d["m12"][..., 1::2], d["start"][0::2], d["start"][1::2], TW.DT, TW.KP, TW.KO, 0.05,
                                feedforward=(d["ff"][:, 0::2], d["ff"][:, 1::2]), rest_joints=(d["rest"][0::2], d["rest"][1::2]), **kw)
    assert tuple(res) == ("joints",) and tuple(res["joints"]) == ("r", "l") and tuple(res["joints"]["r"].shape) == (steps, n_pairs, 7)
    same(joined(res), {"joints": want["joints"]}, "DualArmIK.track_pair_batch, per arm")
    M = np.zeros((steps, n, 4, 4))
    M[..., :3, :3], M[..., :3, 3], M[..., 3, 3] = d["R"], d["p"], 1.0
    res = dual.track_pair_batch(M[:, 0::2], M[:, 1::2], d["start"][0::2], d["start"][1::2], TW.DT, TW.KP, TW.KO, 0.05, want=OUTS,
                                feedforward=d["ff"], rest_joints=d["rest"], **kw)
    same(joined(res), want, "DualArmIK.track_pair_batch on matrices")
    res = dual.track_pair_batch(d["m12"], None, d["start"], None, TW.DT, TW.KP, TW.KO, np.full(n, 0.05), want=OUTS, feedforward=d["ff"],
                                rest_joints=d["rest"], **kw)
    same(joined(res), want, "DualArmIK.track_pair_batch on interleaved arrays")
    assert res["clearance"]["r"].data_ptr() + 8 == res["clearance"]["l"].data_ptr(), "two views of one tensor"
    out = {"clearance": torch.full((steps, n), 7.0, dtype=torch.float64, device="cuda")}
    call = dict(damping=0.05, feedforward=T(d["ff"], torch), rest_joints=T(d["rest"], torch),
                **{k: (T(v, torch) if k in ("spheres", "capsules") else v) for k, v in kw.items()})
    res = solver.track_pair(T(d["m12"], torch), T(d["start"], torch), TW.DT, TW.KP, TW.KO, want=("clearance", "min_clearance"), out=out, **call)
    assert res["clearance"] is out["clearance"] and tuple(res) == ("clearance", "min_clearance")
    plan = solver.track_pair(T(d["m12"], torch), T(d["start"], torch), TW.DT, TW.KP, TW.KO, want=("clearance",), plan_only=True, **call)
    plan["launch"]()
    torch.cuda.synchronize()
    assert np.array_equal(bits(plan["clearance"].cpu().numpy()), bits(out["clearance"].cpu().numpy()))
    assert np.array_equal(bits(out["clearance"].cpu().numpy()), bits(want["clearance"]))
    res = dual.track_pair_batch(d["m12"], None, d["start"], None, TW.DT, TW.KP, TW.KO, 0.05, want=("min_clearance",), out={"min_clearance": res["min_clearance"]},
                                feedforward=d["ff"], rest_joints=d["rest"], **kw)
    assert np.array_equal(bits(joined(res)["min_clearance"]), bits(want["min_clearance"]))
    for bad in (dict(want=()), dict(want=("witness",)), dict(damping=None), dict(dt=0.0), dict(influence=-1.0), dict(avoid_gain=float("nan")),
                dict(spheres=torch.zeros((257, 4), dtype=torch.float64)), dict(capsules=torch.zeros((65, 7), dtype=torch.float64)),
                dict(link_radius=(0.1, -0.1, 0.1))):
        a = {"dt": TW.DT, "kp": TW.KP, "ko": TW.KO, **call, **bad}
        with pytest.raises(ValueError):
            solver.track_pair(T(d["m12"], torch), T(d["start"], torch), **a)
    with pytest.raises(ValueError):  # an odd number of rows
        solver.track_pair(T(np.ascontiguousarray(d["m12"][..., :3]), torch), T(d["start"][:3], torch), TW.DT, TW.KP, TW.KO, damping=0.05)
    with pytest.raises(ValueError):
        dual.track_pair_batch(d["m12"], None, d["start"][0::2], d["start"][1::2], TW.DT, TW.KP, TW.KO, 0.05)


# ------------------------------------------------------------------------------------------ 10. the INTEGRATION.md snippet
def test_integration_md_snippet(torch_mod):
    """The pair snippet of INTEGRATION.md as written: the shapes of the split outputs; the right arm's clearance is rsik_clearance's at
    its joints before each step with the table followed by arm_capsules of the left arm's link_points at ITS joints before that step
    (three robots, every step); the left arm is the nearest obstacle of the right one somewhere and the table elsewhere; the hands
    reach their goals as they do without the push, and no robot ends nearer to a collision than without it by more than 1 mm."""
    from reachy2_symbolic_ik_amd import DualArmIK
    from reachy2_symbolic_ik_amd.symbolic_ik import arm_capsules

    torch = torch_mod
    with contextlib.redirect_stdout(io.StringIO()):
        dual = DualArmIK(solver=solver_of("default/default"), **arm_pairs.DEFAULT)
    torch.manual_seed(7312)

    n, T_, dt = 64, 60, 0.01
    sway = 0.1 * (torch.rand((n, 7), dtype=torch.float64, device="cuda") - 0.5)
    q_r = torch.tensor([-0.5, -0.1, 0.0, -1.5, 0.0, 0.0, 0.0], dtype=torch.float64, device="cuda") + sway
    q_l = torch.tensor([-0.5, 0.1, 0.0, -1.5, 0.0, 0.0, 0.0], dtype=torch.float64, device="cuda") + sway
    (p_r, R_r), (p_l, R_l) = dual.r_arm.forward_kinematics_batch(q_r), dual.l_arm.forward_kinematics_batch(q_l)
    s = torch.arange(T_, dtype=torch.float64, device="cuda") / (T_ - 1)
    mid = 0.5 * (p_r + p_l)

    def goals_of(p, R):
        return torch.cat([R.reshape(1, n, 9).expand(T_, n, 9), p[None] + s[:, None, None] * 0.8 * (mid - p)], dim=2).permute(0, 2, 1)

    table = torch.tensor([[0.2, -0.6, -0.45, 0.2, 0.6, -0.45, 0.05]], dtype=torch.float64)
    radius = (0.05, 0.04, 0.03)
    run = dual.track_pair_batch(goals_of(p_r, R_r), goals_of(p_l, R_l), q_r, q_l, dt=dt, kp=20.0, ko=20.0, damping=0.02, capsules=table,
                                link_radius=radius, influence=0.10, avoid_gain=20.0,
                                want=("joints", "clearance", "nearest", "min_clearance", "final_err"))
    by_partner = run["nearest"]["r"][..., 1] >= 1
    touched = torch.minimum(run["min_clearance"]["r"], run["min_clearance"]["l"]) < 0.0

    for side in ("r", "l"):
        assert tuple(run["joints"][side].shape) == (T_, n, 7) and tuple(run["clearance"][side].shape) == (T_, n)
        assert tuple(run["nearest"][side].shape) == (T_, n, 2) and tuple(run["min_clearance"][side].shape) == (n,)
        assert torch.isfinite(run["joints"][side]).all() and torch.isfinite(run["min_clearance"][side]).all()
    assert tuple(by_partner.shape) == (T_, n) and by_partner.any() and (~by_partner).any() and touched.dtype == torch.bool
    before_r, before_l = torch.cat([q_r[None], run["joints"]["r"][:-1]]), torch.cat([q_l[None], run["joints"]["l"][:-1]])
    far = torch.tensor([[9.0, 9.0, 9.0, 0.1]], dtype=torch.float64)
    lp_l = dual.l_arm.clearance_batch(before_l, far, None, radius, want=("link_points",))["link_points"]
    for i, t in itertools.product((0, 31, 63), range(T_)):
        caps = torch.cat([table.to(lp_l.device), arm_capsules(lp_l[t, i], radius)])
        one = dual.r_arm.clearance_batch(before_r[t, i:i + 1], None, caps, radius, want=("clearance", "nearest"))
        assert torch.equal(one["clearance"].view(torch.int64), run["clearance"]["r"][t, i:i + 1].contiguous().view(torch.int64)), (i, t)
        assert torch.equal(one["nearest"][0], run["nearest"]["r"][t, i]), (i, t)
    blind = dual.track_pair_batch(goals_of(p_r, R_r), goals_of(p_l, R_l), q_r, q_l, dt=dt, kp=20.0, ko=20.0, damping=0.02, capsules=table,
                                  link_radius=radius, influence=0.10, avoid_gain=0.0, want=("joints", "min_clearance", "final_err"))
    pushed = (run["clearance"]["r"] < 0.10).any(dim=0)
    assert pushed.any() and not torch.equal(run["joints"]["r"][:, pushed], blind["joints"]["r"][:, pushed]), "the push moves the arm"
    for side in ("r", "l"):
        gain = run["min_clearance"][side] - blind["min_clearance"][side]
        print(f"INTEGRATION.md pair snippet, {side}: min_clearance against the run without the push: median {float(gain.median()):+.4f} m, "
              f"smallest {float(gain.min()):+.4f} m; final_err {run['final_err'][side].max(dim=0).values.tolist()}")
        assert float(gain.min()) >= -1e-3
        assert float((run["final_err"][side] - blind["final_err"][side]).abs().max()) <= 1e-3
