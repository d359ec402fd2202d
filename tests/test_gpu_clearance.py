"""GPU tests (-m gpu, MI355X) of rsik_clearance (csrc/rsik_kernel_clearance.hpp): the distance between the arm's three capsules and a
set of sphere and capsule obstacles, the nearest pair, its witness points, its gradient in the joints and the link points, against the
NumPy reference of tests/clearance_workload.py (pinned on the CPU alone by tests/test_clearance_abi.py).

Shapes: N_SET = 1024 rows (four workgroups), 321 rows where the obstacles are many, n in {1, 65, N_SET} for the bits,
n_rep in {1, 3}, a uniform arm and an arm byte per row, on the pairs of jacobian_workload.PAIRS.

Tolerances (clearance_workload): the clearance to CLEARANCE_BOUND and the gradient on the kept rows to GRADIENT_BOUND, each
max(1e-13, 16 x the reference's own float64-against-longdouble error); the link points to 1e-13 like the chain everywhere else."""
import contextlib
import functools
import io
import itertools
import math

import numpy as np
import pytest

import arm_pairs
import clearance_workload as W
import far_inputs as FI
import jacobian_workload as JW
from compare import bits
from gpu_support import T, abi, arm_kwargs, last_error, ptr, raw_call, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

OUTS = ("clearance", "nearest", "gradient", "witness", "link_points")
POINT_TOL = 1e-13
_SOLVERS = {}


def solver_of(pair):
    """The pair's solver, uploaded once for this module (the fixture below closes it when the module is done)."""
    if pair not in _SOLVERS:
        _SOLVERS[pair] = arm_pairs.upload(pair, **({"check": lambda p, b: None} if pair == "default/default" else {}))
    return _SOLVERS[pair]


@pytest.fixture(scope="module", autouse=True)
def _solvers_do_not_outlive_the_module(torch_mod):
    yield
    torch_mod.cuda.synchronize()
    while _SOLVERS:
        _SOLVERS.popitem()[1].close()
    torch_mod.cuda.empty_cache()


def run(torch, pair, q, kind, sc, want=OUTS, arm=None, radius=W.LINK_RADIUS):
    """One launch through HipSolver.clearance on joints [n,7] or [n_rep,n,7]; the results on the host."""
    n = q.shape[-2]
    arm = W.kind_arm(kind, n) if arm is None else arm
    res = solver_of(pair).clearance(T(q, torch), spheres=T(sc["spheres"], torch) if len(sc["spheres"]) else None,
                                    capsules=T(sc["capsules"], torch) if len(sc["capsules"]) else None, link_radius=radius, want=want,
                                    **arm_kwargs(kind, arm, torch))
    torch.cuda.synchronize()
    assert tuple(res) == tuple(o for o in OUTS if o in want)
    return {k: v.cpu().numpy() for k, v in res.items()}


def same(a, b, what):
    for k in b:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def check(got, ref, sc, what, keep=None, radius=W.LINK_RADIUS):
    """The five outputs of n rows against the reference and against each other; returns the figures."""
    n = len(ref["clearance"])
    rows = np.arange(n)
    assert got["nearest"].dtype == np.int32 and got["nearest"].shape == (n, 2), what
    e_c = float(np.abs(got["clearance"] - ref["clearance"]).max())
    link, obs = got["nearest"][:, 0], got["nearest"][:, 1]
    assert (link >= 0).all() and (link < 3).all() and (obs >= 0).all() and (obs < ref["pairs"].shape[1]).all(), what
    decided = ref["runner_up"] - ref["clearance"] > 2 * W.CLEARANCE_BOUND
    wrong = int((got["nearest"][decided] != ref["nearest"][decided]).any(axis=1).sum())
    e_named = float((ref["pairs"][rows, obs, link] - ref["clearance"]).max())
    # the witness: x on the link the device named, y on the obstacle it named, |x - y| - radii = the clearance
    P = ref["link_points"]
    x, y = got["witness"][:, 0], got["witness"][:, 1]
    ends = np.concatenate([np.concatenate([sc["spheres"][:, :3], sc["spheres"][:, :3]], axis=1).reshape(-1, 6), sc["capsules"][:, :6].reshape(-1, 6)])
    rad = np.concatenate([sc["spheres"][:, 3], sc["capsules"][:, 6]])[obs] + np.asarray(radius)[link]
    off_x = float(np.sqrt(W.point_segment(x, P[rows, link], P[rows, link + 1] - P[rows, link])[1]).max())
    off_y = float(np.sqrt(W.point_segment(y, ends[obs, :3], ends[obs, 3:] - ends[obs, :3])[1]).max())
    e_w = float(np.abs(np.linalg.norm(x - y, axis=1) - rad - got["clearance"]).max())
    e_p = float(np.abs(got["link_points"] - P).max())
    keep = np.ones(n, dtype=bool) if keep is None else keep
    agree = keep & (got["nearest"] == ref["nearest"]).all(axis=1)
    e_g = float(np.abs(got["gradient"] - ref["gradient"])[agree].max()) if agree.any() else 0.0
    print(f"{what}: clearance {e_c:.2e} (bound {W.CLEARANCE_BOUND:.1e}), nearest differs on {wrong} of {int(decided.sum())} decided rows, the named "
          f"pair's reference clearance above the minimum by {e_named:.2e}, witness off its link {off_x:.2e} / its obstacle {off_y:.2e}, "
          f"|x - y| - radii against the clearance {e_w:.2e}, gradient on {int(agree.sum())} kept rows {e_g:.2e} (bound {W.GRADIENT_BOUND:.1e}), "
          f"link points {e_p:.2e}")
    assert e_c <= W.CLEARANCE_BOUND, (what, e_c)
    assert wrong == 0, (what, wrong)
    assert e_named <= W.CLEARANCE_BOUND, (what, e_named)
    assert off_x <= POINT_TOL and off_y <= POINT_TOL and e_w <= W.CLEARANCE_BOUND, (what, off_x, off_y, e_w)
    assert (agree == keep).all() and e_g <= W.GRADIENT_BOUND, (what, e_g)
    assert np.isfinite(got["gradient"]).all() and e_p <= POINT_TOL, (what, e_p)
    return e_c, e_g


# ------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("pair", JW.PAIRS)
def test_values_against_the_reference(torch_mod, pair):
    """An arm byte per row: both scenes, n_rep = 1 (the uniform set) and n_rep = 3 (the uniform, the wound and the singular set as the
    three repetitions), every output against the reference, the gradient on the kept rows.  A uniform arm: the open scene, n_rep = 1
    and 3.  The parallel capsule alone: row PAR_ROW answers with the parallel pair."""
    torch = torch_mod
    for kind, scene in (("mixed", "open"), ("mixed", "deep"), ("r", "open")):
        cases = [W.case(pair, name, scene, kind) for name in W.SETS]
        sc = cases[0]["sc"]
        one = run(torch, pair, cases[0]["q"], kind, sc)
        check(one, cases[0]["ref"], sc, f"{pair} {scene} {kind} n_rep=1", cases[0]["keep"])
        three = run(torch, pair, np.stack([c["q"] for c in cases]), kind, sc)
        assert three["clearance"].shape == (3, W.N_SET) and three["nearest"].shape == (3, W.N_SET, 2) and three["witness"].shape == (3, W.N_SET, 2, 3)
        assert three["gradient"].shape == (3, W.N_SET, 7) and three["link_points"].shape == (3, W.N_SET, 4, 3)
        for rep, (name, c) in enumerate(zip(W.SETS, cases)):
            check({k: v[rep] for k, v in three.items()}, c["ref"], sc, f"{pair} {scene} {kind} n_rep=3 [{rep}] {name}", c["keep"])
        same({k: v[0] for k, v in three.items()}, one, f"{pair} {scene} {kind}: repetition 0 of 3 against n_rep = 1")
    alone = W.case(pair, "uniform", "parallel")
    got = run(torch, pair, alone["q"], "mixed", alone["sc"])
    check(got, alone["ref"], alone["sc"], f"{pair} the parallel capsule alone", alone["keep"])
    assert tuple(got["nearest"][W.PAR_ROW]) == (1, 0)
    assert abs(got["clearance"][W.PAR_ROW] - (W.PAR_DISTANCE - W.LINK_RADIUS[1] - 0.02)) <= W.CLEARANCE_BOUND


@pytest.mark.parametrize("pair", ["default/default", "custom/custom"])
def test_wound_and_singular_sets(torch_mod, pair):
    """The wound set (whole turns up to +-6 pi) gives the uniform set's answers to 1e-9; the singular set (a straight elbow) is finite."""
    torch = torch_mod
    sc = W.scene(pair, "open")
    plain, wound = (run(torch, pair, JW.joint_set(name), "mixed", sc) for name in ("uniform", "wound"))
    decided = W.case(pair, "uniform", "open")["keep"]
    for k in OUTS:
        rows = np.ones(W.N_SET, dtype=bool) if k in ("clearance", "link_points") else decided
        err = float(np.abs(wound[k].astype(np.float64) - plain[k])[rows].max())
        print(f"{pair}: wound set against the unwound rows, {k}: {err:.3e}")
        assert err <= 1e-9, (pair, k, err)
    sing = run(torch, pair, JW.joint_set("singular"), "mixed", sc)
    assert all(np.isfinite(sing[k]).all() for k in OUTS if k != "nearest") and (sing["nearest"] >= 0).all()


@functools.lru_cache(maxsize=None)
def far_rows():
    """One joint of a uniform row at a rung of tests/far_inputs.py (2^27, 1e15, 1e300), each joint in turn, and its reduced twin."""
    base = JW.joint_set("uniform")
    far, twin = [], []
    for g, rung in enumerate((2.0 ** 27, 1e15, 1e300)):
        for k in range(7):
            row = base[g * 7 + k].copy()
            sign = 1.0 if k % 2 else -1.0
            x = FI.wind(row[k], rung, sign) if rung < FI.WALKED_FROM else FI.walked(rung, sign, 0.0)[0][k]
            t = row.copy()
            row[k], t[k] = x, FI.reduce_angle(x)
            assert abs(x) >= rung / 2 and abs(t[k]) <= math.pi
            far.append(row); twin.append(t)
    return np.array(far), np.array(twin)


def test_far_angles_are_answered_like_their_reduced_twins(torch_mod):
    """As rsik_jacobian: a joint at 2^27, 1e15 or 1e300 gives the outputs of the angle of [-pi, pi] it is congruent to, to 1e-9."""
    torch = torch_mod
    pair = "custom/custom"
    far, twin = far_rows()
    sc, arm = W.scene(pair, "deep"), JW.arm_bytes()[: len(far)]
    a, b = run(torch, pair, far, "mixed", sc, arm=arm), run(torch, pair, twin, "mixed", sc, arm=arm)
    ref = W.reference(JW.blocks_of(pair), twin, arm, sc)
    assert np.abs(b["clearance"] - ref["clearance"]).max() <= W.CLEARANCE_BOUND
    decided = ref["runner_up"] - ref["clearance"] > 1e-6
    assert decided.sum() >= len(far) - 2
    for k in OUTS:
        err = float(np.abs(a[k].astype(np.float64) - b[k])[decided].max())
        print(f"far rows against their reduced twins, {k}: {err:.3e}")
        assert np.isfinite(a[k]).all() and err <= 1e-9, (k, err)


# ------------------------------------------------------------------------------------------ obstacle counts
def crowd(n_spheres, n_capsules, seed):
    """A seeded scene of that many obstacles inside the arms' reach, radii 0.01 ... 0.08."""
    rng = np.random.default_rng(seed)
    centre = lambda k: rng.uniform(-0.6, 0.6, size=(k, 3)) + [0.2, 0.0, -0.1]  # noqa: E731
    a = centre(n_capsules)
    return dict(spheres=np.concatenate([centre(n_spheres), rng.uniform(0.01, 0.08, size=(n_spheres, 1))], axis=1),
                capsules=np.concatenate([a, a + rng.uniform(-0.2, 0.2, size=(n_capsules, 3)), rng.uniform(0.01, 0.08, size=(n_capsules, 1))], axis=1))


@pytest.mark.parametrize("counts", [(1, 0), (0, 1), (257, 0), (0, 129), (300, 130), (4096, 256)])
def test_obstacle_counts(torch_mod, counts):
    """One sphere alone, one capsule alone, one more than a staged tile of either kind (256 spheres, 128 capsules), both kinds past a
    tile, and the maxima, on 321 rows (a workgroup and a wave and one row): every output against the reference; the last obstacle of
    each kind wins somewhere when it is moved onto a row's wrist."""
    torch = torch_mod
    pair, n = "custom/custom", 321
    q, arm = JW.joint_set("uniform")[:n], JW.arm_bytes()[:n]
    sc = crowd(*counts, seed=7400 + counts[0] + counts[1])
    blocks = JW.blocks_of(pair)
    wrist = W.reference(blocks, q[:2], arm[:2], sc)["link_points"][:, 2]
    if counts[0]:
        sc["spheres"][-1] = np.concatenate([wrist[0] + [0.0, 0.0, 0.01], [0.08]])
    if counts[1]:
        sc["capsules"][-1] = np.concatenate([wrist[1] + [0.0, 0.0, 0.01], wrist[1] + [0.1, 0.0, 0.01], [0.08]])
    ref = W.reference(blocks, q, arm, sc)
    got = run(torch, pair, q, "mixed", sc)
    check(got, ref, sc, f"{counts[0]} spheres, {counts[1]} capsules", keep=np.zeros(n, dtype=bool))
    if counts[0]:
        assert got["nearest"][0, 1] == counts[0] - 1
    if counts[1]:
        assert got["nearest"][1, 1] == counts[0] + counts[1] - 1


def test_permuting_the_obstacles_leaves_the_clearance_bits(torch_mod):
    torch = torch_mod
    pair = "default/ztip"
    sc = crowd(300, 130, seed=7450)
    q = JW.joint_set("uniform")
    base = run(torch, pair, q, "mixed", sc, want=("clearance", "nearest"))
    rng = np.random.default_rng(7451)
    ps, pc = rng.permutation(300), rng.permutation(130)
    got = run(torch, pair, q, "mixed", dict(spheres=sc["spheres"][ps], capsules=sc["capsules"][pc]), want=("clearance", "nearest"))
    assert np.array_equal(bits(got["clearance"]), bits(base["clearance"]))
    back = np.concatenate([ps, 300 + pc])[got["nearest"][:, 1]]
    assert np.array_equal(back, base["nearest"][:, 1]) and np.array_equal(got["nearest"][:, 0], base["nearest"][:, 0])


# ------------------------------------------------------------------------------------------ bits
def test_bits_do_not_depend_on_the_launch(torch_mod):
    """Every output alone and with the others; n = 1, 65 and N_SET on the same rows; a uniform arm against bytes that all say the same;
    the flat call on the tiled rows against n_rep = 3; two launches: bit for bit."""
    torch = torch_mod
    pair = "custom/custom"
    sc = W.scene(pair, "open")
    q = JW.joint_set("uniform")
    for kind in ("l", "mixed"):
        full = run(torch, pair, q, kind, sc)
        same(run(torch, pair, q, kind, sc), full, f"{kind} twice")
        for r in (1, 2, 4):
            for sub in itertools.combinations(OUTS, r):
                same(full, run(torch, pair, q, kind, sc, want=sub), f"{kind} want={sub}")
        for n in (1, 65):
            same({k: v[:n] for k, v in full.items()}, run(torch, pair, q[:n], kind, sc), f"{kind} n={n}")
    l_rows = W.kind_arm("l")
    same(run(torch, pair, q, "l", sc), run(torch, pair, q, "mixed", sc, arm=l_rows), "a uniform arm against bytes that all say l")
    q3 = np.ascontiguousarray(np.stack([JW.joint_set(name) for name in W.SETS]))
    rep = run(torch, pair, q3, "mixed", sc)
    flat = run(torch, pair, q3.reshape(-1, 7), "mixed", sc, arm=np.tile(W.kind_arm("mixed"), 3))
    same({k: v.reshape(flat[k].shape) for k, v in rep.items()}, flat, "n_rep = 3 against the flat call")


# ------------------------------------------------------------------------------------------ rows and obstacles that are not numbers
@pytest.mark.parametrize("kind", ["r", "mixed"])
def test_rows_that_are_not_numbers(torch_mod, kind):
    """A NaN, a +inf and a -inf in single rows — the first row, both sides of a wave boundary, the last row; in the first and in the
    last repetition — make those rows NaN with nearest (-1, -1); every other row carries the bits of the run with ordinary values."""
    torch = torch_mod
    pair, n, n_rep = "default/default", 129, 3
    sc = W.scene(pair, "open")
    q = np.ascontiguousarray(JW.joint_set("uniform")[: n * n_rep].reshape(n_rep, n, 7))
    base = run(torch, pair, q, kind, sc)
    spots = [(0, 0, 0, np.nan), (0, 63, 3, np.inf), (0, 64, 6, -np.inf), (0, 128, 5, np.nan), (2, 0, 1, -np.inf), (2, 63, 2, np.nan), (2, 128, 4, np.inf)]
    bad = q.copy()
    hit = np.zeros((n_rep, n), dtype=bool)
    for rep, row, k, v in spots:
        bad[rep, row, k], hit[rep, row] = v, True
    for subset in (OUTS, ("clearance", "nearest"), ("gradient",)):
        got = run(torch, pair, bad, kind, sc, want=subset)
        for k in subset:
            flat = got[k].reshape(n_rep, n, -1)
            assert (flat[hit] == -1).all() if k == "nearest" else np.isnan(flat[hit]).all(), (kind, k)
            assert np.array_equal(bits(flat[~hit]), bits(base[k].reshape(n_rep, n, -1)[~hit])), (kind, k, "another row's bits changed")


def test_obstacles_that_are_not_numbers(torch_mod):
    """NaN, infinite and negative-radius obstacles: the bits of the scene without them, the obstacle indices shifted.  All obstacles
    bad: clearance +infinity, nearest (-1, -1), gradient 0, witness NaN, the link points as ever."""
    torch = torch_mod
    pair = "custom/custom"
    sc = W.scene(pair, "open")
    ok_s, ok_c = W.usable(sc["spheres"]), W.usable(sc["capsules"])
    assert (~ok_s).sum() == 3 and (~ok_c).sum() == 1
    q = JW.joint_set("uniform")
    dirty = run(torch, pair, q, "mixed", sc)
    clean = run(torch, pair, q, "mixed", dict(spheres=sc["spheres"][ok_s], capsules=sc["capsules"][ok_c]))
    shift = np.concatenate([np.cumsum(ok_s) - 1, ok_s.sum() + np.cumsum(ok_c) - 1])
    assert ok_s[dirty["nearest"][:, 1][dirty["nearest"][:, 1] < len(ok_s)]].all()
    moved = dict(dirty, nearest=np.stack([dirty["nearest"][:, 0], shift[dirty["nearest"][:, 1]]], axis=1).astype(np.int32))
    same(moved, clean, "the scene with its skipped obstacles against the scene without them")
    more = np.array([[0.3, 0.0, 0.0, np.nan], [0.3, 0.0, 0.0, np.inf], [0.3, -np.inf, 0.0, 0.1]])
    none = run(torch, pair, q, "mixed", dict(spheres=np.concatenate([sc["spheres"][~ok_s], more]), capsules=sc["capsules"][~ok_c]))
    assert np.isposinf(none["clearance"]).all() and (none["nearest"] == -1).all() and (none["gradient"] == 0.0).all()
    assert np.isnan(none["witness"]).all()
    assert np.array_equal(bits(none["link_points"]), bits(dirty["link_points"]))


# ------------------------------------------------------------------------------------------ the ABI's refusals
def test_refusals(torch_mod):
    """Counts outside their ranges, no obstacle, a negative, NaN or infinite link radius, all outputs NULL, joints NULL, n < 0,
    n_rep < 1, an obstacle array NULL with a count, a misaligned nearest: RSIK_E_INVALID with the function's name in rsik_last_error;
    n == 0 launches nothing; an arm whose constants were not uploaded is RSIK_E_NOT_SET."""
    import ctypes as C

    from reachy2_symbolic_ik_amd import HipSolver

    torch, A = torch_mod, abi()
    solver = solver_of("default/default")
    q = T(JW.joint_set("uniform")[:8], torch)
    sp = T(np.tile([[0.3, 0.0, 0.0, 0.05]], (4096, 1)), torch)
    cp = T(np.tile([[0.3, 0.0, 0.0, 0.3, 0.1, 0.0, 0.05]], (256, 1)), torch)
    o = torch.empty((8,), dtype=torch.float64, device="cuda")
    near = torch.empty((9, 2), dtype=torch.int32, device="cuda")
    arm = T(JW.arm_bytes()[:8], torch)
    rad = lambda *v: (C.c_double * 3)(*v)  # noqa: E731
    outs = (ptr(o), None, None, None, None)
    for what, args in (("n_spheres 4097", (8, 1, ptr(q), None, 0, None, 4097, ptr(sp), 0, None) + outs),
                       ("n_spheres -1", (8, 1, ptr(q), None, 0, None, -1, ptr(sp), 1, ptr(cp)) + outs),
                       ("n_capsules 257", (8, 1, ptr(q), None, 0, None, 0, None, 257, ptr(cp)) + outs),
                       ("no obstacle", (8, 1, ptr(q), None, 0, None, 0, None, 0, None) + outs),
                       ("a negative radius", (8, 1, ptr(q), None, 0, rad(0.0, -0.01, 0.0), 1, ptr(sp), 0, None) + outs),
                       ("a NaN radius", (8, 1, ptr(q), None, 0, rad(0.0, 0.0, math.nan), 1, ptr(sp), 0, None) + outs),
                       ("an infinite radius", (8, 1, ptr(q), None, 0, rad(math.inf, 0.0, 0.0), 1, ptr(sp), 0, None) + outs),
                       ("all outputs NULL", (8, 1, ptr(q), None, 0, None, 1, ptr(sp), 0, None, None, None, None, None, None)),
                       ("joints NULL", (8, 1, None, None, 0, None, 1, ptr(sp), 0, None) + outs),
                       ("n < 0", (-1, 1, ptr(q), None, 0, None, 1, ptr(sp), 0, None) + outs),
                       ("n_rep < 1", (8, 0, ptr(q), None, 0, None, 1, ptr(sp), 0, None) + outs),
                       ("spheres NULL", (8, 1, ptr(q), None, 0, None, 1, None, 0, None) + outs),
                       ("capsules NULL", (8, 1, ptr(q), None, 0, None, 0, None, 1, None) + outs),
                       ("nearest misaligned", (8, 1, ptr(q), None, 0, None, 1, ptr(sp), 0, None, None, near.data_ptr() + 4, None, None, None)),
                       ("arm_uniform 2", (8, 1, ptr(q), None, 2, None, 1, ptr(sp), 0, None) + outs)):
        assert raw_call(solver, "rsik_clearance", *args) == A.RSIK_E_INVALID, what
        assert "rsik_clearance" in last_error(solver), (what, last_error(solver))
    assert raw_call(solver, "rsik_clearance", 0, 1, None, None, 0, None, 1, None, 0, None, None, None, None, None, None) == A.RSIK_OK
    assert raw_call(solver, "rsik_clearance", 8, 1, ptr(q), ptr(arm), 0, rad(0.0, 0.0, 0.0), 4096, ptr(sp), 256, ptr(cp),
                    None, None, None, None, None) == A.RSIK_E_INVALID
    assert raw_call(solver, "rsik_clearance", 8, 1, ptr(q), ptr(arm), 0, rad(0.0, 0.0, 0.0), 4096, ptr(sp), 256, ptr(cp), *outs) == A.RSIK_OK
    bare = HipSolver(0)
    assert raw_call(bare, "rsik_clearance", 8, 1, ptr(q), None, 0, None, 1, ptr(sp), 0, None, *outs) == A.RSIK_E_NOT_SET
    assert raw_call(bare, "rsik_clearance", 8, 1, ptr(q), ptr(arm), 0, None, 1, ptr(sp), 0, None, *outs) == A.RSIK_E_NOT_SET
    torch.cuda.synchronize()
    bare.close()
    with pytest.raises(ValueError):
        solver.clearance(q)
    with pytest.raises(ValueError):
        solver.clearance(q, spheres=sp[:1], want=())
    with pytest.raises(ValueError):
        solver.clearance(q, spheres=sp[:1], link_radius=(0.0, -1.0, 0.0))


# ------------------------------------------------------------------------------------------ the Python surface
def test_python_surface(torch_mod):
    """SymbolicIK.clearance_batch and DualArmIK.clearance_batch are HipSolver.clearance on their arms; out= buffers are written in
    place; a planned launch writes the same bits; other_arm adds that arm's three capsules behind the caller's."""
    from reachy2_symbolic_ik_amd import DualArmIK, SymbolicIK
    from reachy2_symbolic_ik_amd.symbolic_ik import arm_capsules

    torch = torch_mod
    pair = "default/default"
    solver, sc = solver_of(pair), W.scene(pair, "open")
    q = np.ascontiguousarray(JW.joint_set("uniform")[:390].reshape(3, 130, 7))
    arm = JW.arm_bytes()[:130]
    with contextlib.redirect_stdout(io.StringIO()):
        ik_l = SymbolicIK("l_arm", solver=solver, **arm_pairs.DEFAULT)
        dual = DualArmIK(solver=solver, **arm_pairs.DEFAULT)
    sp, cp = T(sc["spheres"], torch), T(sc["capsules"], torch)
    got = {k: v.cpu().numpy() for k, v in ik_l.clearance_batch(q, sp, cp, W.LINK_RADIUS, want=OUTS).items()}
    same(got, run(torch, pair, q, "l", sc), "SymbolicIK.clearance_batch")
    got = {k: v.cpu().numpy() for k, v in dual.clearance_batch(arm, q, sp, cp, W.LINK_RADIUS).items()}
    assert tuple(got) == ("clearance", "nearest")
    same(got, run(torch, pair, q, "mixed", sc, want=("clearance", "nearest")), "DualArmIK.clearance_batch")
    out = {"gradient": torch.full((3, 130, 7), 7.0, dtype=torch.float64, device="cuda")}
    res = solver.clearance(T(q, torch), sp, cp, W.LINK_RADIUS, arm=T(arm, torch), want=("gradient", "clearance"), out=out)
    assert res["gradient"] is out["gradient"] and tuple(res) == ("clearance", "gradient")
    plan = solver.clearance(T(q, torch), sp, cp, W.LINK_RADIUS, arm=T(arm, torch), want=("gradient",), plan_only=True)
    plan["launch"]()
    torch.cuda.synchronize()
    assert np.array_equal(bits(plan["gradient"].cpu().numpy()), bits(out["gradient"].cpu().numpy()))
    # the right arm's rows against the scene and the left arm at one row of joints
    q_l = JW.joint_set("uniform")[700]
    lp = run(torch, pair, q_l[None], "l", sc, want=("link_points",))["link_points"][0]
    caps = arm_capsules(torch.as_tensor(lp), W.LINK_RADIUS).numpy()
    assert np.array_equal(caps[:, :3], lp[:3]) and np.array_equal(caps[:, 3:6], lp[1:]) and np.array_equal(caps[:, 6], W.LINK_RADIUS)
    r_rows = np.zeros(130, dtype=np.uint8)
    got = {k: v.cpu().numpy() for k, v in dual.clearance_batch(r_rows, q, sp, cp, W.LINK_RADIUS, other_arm=(1, q_l), want=OUTS).items()}
    both = dict(spheres=sc["spheres"], capsules=np.concatenate([sc["capsules"], caps]))
    same(got, run(torch, pair, q, "r", both), "DualArmIK.clearance_batch with the other arm's capsules")


# ------------------------------------------------------------------------------------------ compositions
@pytest.mark.parametrize("pair", JW.PAIRS)
def test_gradient_as_bias_rates_moves_in_the_null_space(torch_mod, pair):
    """rsik_joint_rates with twist 0, lambda = 1e-3 and bias_rates = the gradient, on the kept rows whose manipulability is >= 1e-3: the
    achieved twist is below 1e-4 |gradient| in norm and gradient . rates >= 0 (the clearance does not shrink).  On the deep scene:
    there the exact solve (NumPy, float64, on the reference's Jacobian and gradient) gives at most 2.4e-5 |gradient| on the three
    pairs.  On the open scene of default/default the exact solve itself gives 1.08e-4 on one row of 913 (8.4e-5 and 9.5e-5 on the
    other two pairs), so the bound cannot be asked there.  A row whose witness is the shoulder itself has the zero gradient: zero
    rates and a zero twist, exactly."""
    torch = torch_mod
    c = W.case(pair, "uniform", "deep")
    solver, sc = solver_of(pair), c["sc"]
    q, arm = T(c["q"], torch), T(c["arm"], torch)
    g = solver.clearance(q, T(sc["spheres"], torch), T(sc["capsules"], torch), W.LINK_RADIUS, arm=arm, want=("gradient",))["gradient"]
    res = solver.joint_rates(q, torch.zeros((W.N_SET, 6), dtype=torch.float64, device="cuda"), damping=1e-3, bias_rates=g, arm=arm,
                             want=("rates", "achieved_twist"))
    w = solver.jacobian(q, arm=arm, want=("manipulability",))["manipulability"]
    torch.cuda.synchronize()
    g, rates, twist, w = (t.cpu().numpy() for t in (g, res["rates"], res["achieved_twist"], w))
    rows = c["keep"] & (w >= 1e-3)
    still = rows & (np.abs(g).max(axis=1) == 0.0)
    assert (rates[still] == 0.0).all() and (twist[still] == 0.0).all() and still.sum() * 2 < rows.sum()
    rows &= ~still
    ratio = np.linalg.norm(twist[rows], axis=1) / np.linalg.norm(g[rows], axis=1)
    gain = (g[rows] * rates[rows]).sum(axis=1)
    print(f"{pair}: {int(rows.sum())} rows, achieved twist at most {ratio.max():.3e} |gradient|, gradient . rates at least {gain.min():.3e}")
    assert rows.sum() + still.sum() >= 900
    assert (ratio < 1e-4).all(), (pair, float(ratio.max()))
    assert (gain >= 0.0).all(), (pair, float(gain.min()))


def test_clearance_of_a_sweep_in_place(torch_mod):
    """rsik_clearance on rsik_solve_sweep's joints in place (n_rep = n_theta = 8) equals the flat form row for row, bit for bit; the
    snippet of INTEGRATION.md as written picks, per pose, the sample with the largest clearance."""
    from reachy2_symbolic_ik_amd import SymbolicIK

    torch = torch_mod
    pair = "default/default"
    sc = W.scene(pair, "open")
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", solver=solver_of(pair), **arm_pairs.DEFAULT)
    pos, eul, arm, _ = JW.link_poses()
    poses = np.stack([pos[arm == 0], eul[arm == 0]], axis=1)  # [n,2,3]
    spheres, capsules = T(sc["spheres"], torch), T(sc["capsules"], torch)
    sweep = ik.sweep_batch(poses, n_theta=8)
    got = ik.clearance_batch(sweep["joints"], spheres, capsules, W.LINK_RADIUS, want=OUTS)
    flat = ik.clearance_batch(sweep["joints"].reshape(-1, 7), spheres, capsules, W.LINK_RADIUS, want=OUTS)
    torch.cuda.synchronize()
    assert tuple(got["clearance"].shape) == (8, len(poses))
    same({k: v.cpu().numpy().reshape(flat[k].shape) for k, v in got.items()}, {k: v.cpu().numpy() for k, v in flat.items()}, "a sweep in place")
    c = got["clearance"]
    free = torch.nan_to_num(c, nan=-1.0) > 0.0                       # the samples that keep the arm off every obstacle
    best = torch.nan_to_num(c, nan=-float("inf")).argmax(dim=0)      # per pose: the sample with the most room
    q = sweep["joints"][best, torch.arange(c.shape[1], device=c.device)]
    assert tuple(q.shape) == (len(poses), 7) and bool(free.any()) and bool((~free).any())
    again = ik.clearance_batch(q, spheres, capsules, W.LINK_RADIUS, want=("clearance",))["clearance"]
    ok = torch.isfinite(again)
    assert bool(ok.any()) and torch.equal(again[ok], torch.nan_to_num(c, nan=-float("inf")).max(dim=0).values[ok])
