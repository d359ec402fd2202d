"""GPU tests (-m gpu, MI355X) of rsik_clearance_edges (csrc/rsik_kernel_clearance_edges.hpp): the clearance along the motion between
the waypoints of a path.

The entry point is defined against rsik_clearance and RSIK_STAGE_ANGLE_DIFF: delta comes from the device's own angle_diff, q(s) from
NumPy in the order include/rsik.h fixes (tests/clearance_edges_workload.samples), and ONE rsik_clearance launch over the samples gives
d and the pairs.  edge_clearance and edge_nearest have that launch's bits, edge_sub is the first argmin; edge_bound is the formula,
within ten roundings; the per-path outputs are NumPy's fold of the per-edge ones, exactly.  The joints are the library's own
rsik_solve_path_clear winners (min_clearance 0, (0.05, 100), start rows) on path_clear_workload.TABLE_SHAPES, n = 37, in the scene
clearance_workload.scene("default/default", "open") with LINK_RADIUS."""
import ctypes as C
import functools

import numpy as np
import pytest

import clearance_edges_workload as EW
import path_clear_workload as PC
from clearance_workload import LINK_RADIUS, usable
from compare import as_bits, bits
from gpu_support import T, abi, last_error, make_symbolic, ptr, raw_call, to_np, torch_mod  # noqa: F401
from path_workload import MAIN_SHAPES, N_MAIN, path_fractions, path_poses, path_start
from sampling_support import path_arm_kwargs, path_soa

pytestmark = pytest.mark.gpu

SHAPES = tuple(s for s in MAIN_SHAPES if s[:3] in PC.TABLE_SHAPES)
EDGE = ("edge_clearance", "edge_sub", "edge_nearest", "edge_bound")
PATH = ("path_clearance", "path_edge", "path_bound", "n_below", "first_below")
EVERY = EDGE + PATH
# edge_bound against the formula in NumPy from the returned edge_clearance: the device and NumPy form acc from the same delta with
# the same seven products and six sums, but |tip| is a square root on either side (one rounding apart) inside R, which enters every
# term: at most ten roundings of values below 64 in all, and ulp(64) = 1.4e-14.
BOUND_TOL = 1e-12
assert 10 * np.spacing(64.0) < BOUND_TOL


def scene_tensors(torch, scene=None):
    sc = PC.the_scene() if scene is None else scene
    return dict(spheres=T(sc["spheres"], torch) if len(sc["spheres"]) else None,
                capsules=T(sc["capsules"], torch) if len(sc["capsules"]) else None, link_radius=LINK_RADIUS)


def arm_kw(arm, torch):
    """One byte per path where the arms differ, else the one arm for the launch."""
    arm = np.asarray(arm)
    return dict(arm=T(arm, torch)) if (arm != arm[0]).any() else dict(arm_uniform=int(arm[0]))


def run(solver, joints, arm, torch, n_sub=16, start=None, scene=None, **kw):
    return to_np(solver.clearance_edges(T(joints, torch), None if start is None else T(start, torch), n_sub, **scene_tensors(torch, scene),
                                        **arm_kw(arm, torch), **kw))


def compose(solver, joints, arm, torch, n_sub, start=None, scene=None, min_clearance=-np.inf):
    """The expected value: the device's angle_diff, NumPy's q(s), one rsik_clearance launch over the samples, NumPy's folds."""
    wp, have_a, a = EW.edges_of(joints, start)
    b0 = np.where(wp[..., None], np.nan_to_num(joints, nan=0.0, posinf=0.0, neginf=0.0), 0.0)
    rows = np.ascontiguousarray(np.stack([b0.reshape(-1), a.reshape(-1)], axis=1))
    delta = solver.stage(abi().STAGE_ANGLE_DIFF, T(rows, torch)).cpu().numpy().reshape(b0.shape)
    arm = np.asarray(arm)

    def clearance_of(q, path):
        got = to_np(solver.clearance(T(q, torch), want=("clearance", "nearest"), **scene_tensors(torch, scene), **arm_kw(arm[path], torch)))
        return got["clearance"], got["nearest"]

    return EW.expected(joints, arm, n_sub, clearance_of, start, min_clearance, delta=delta)


def same(got, exp, what, keys=EVERY, paths=None):
    for key in keys:
        x, y = got[key], exp[key]
        if paths is not None:
            x, y = (x[:, paths], y[:, paths]) if key in EDGE else (x[paths], y[paths])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, key, x.dtype, y.dtype, x.shape, y.shape)
        np.testing.assert_array_equal(as_bits(x), as_bits(y), err_msg=f"{what}: {key}")


def check(got, exp, what, min_clearance=-np.inf):
    """The acceptance of one launch against compose()'s expected value."""
    same(got, exp, what, keys=("edge_clearance", "edge_sub", "edge_nearest"))
    wp = exp["wp"]
    assert np.isnan(got["edge_clearance"][~wp]).all() and (got["edge_sub"][~wp] == -1).all() and (got["edge_nearest"][~wp] == -1).all(), what
    assert np.isnan(got["edge_bound"][~wp]).all() and not np.isnan(got["edge_bound"][wp]).any(), what
    formula = EW.bound(got["edge_clearance"], exp["delta"], int(exp["d"].shape[0]) - 1, EW.reach(EW.JW.blocks_of(EW.PAIR), exp["arm"])[None])
    fin = wp & np.isfinite(got["edge_clearance"])
    err = float(np.abs(got["edge_bound"] - formula)[fin].max(initial=0.0))
    assert err <= BOUND_TOL, (what, "edge_bound against the formula", err)
    np.testing.assert_array_equal(got["edge_bound"][wp & ~fin], got["edge_clearance"][wp & ~fin], err_msg=what + ": the bound of an infinite clearance")
    fold = EW.fold_paths(got["edge_clearance"], got["edge_sub"], got["edge_bound"], min_clearance)
    same(got, fold, what + " (the fold of the device's edges)", keys=PATH)
    return err


@functools.lru_cache(maxsize=None)
def shape_case(shape):
    """A shape's rsik_solve_path_clear winners (joints [T,n,7], clearance [T,n]), its arm bytes and start rows: computed once, shared."""
    import torch

    t, k, seed, kind = shape
    n = N_MAIN
    solver, _, _ = make_symbolic(0.03)
    pos, eul, arm = path_poses(seed, n, t, kind)
    start = path_start(seed, n)
    got = to_np(solver.solve_path_clear(path_soa(pos, eul, torch), T(path_fractions(k), torch), T(start, torch), **scene_tensors(torch),
                                        min_clearance=0.0, influence=0.05, clearance_gain=100.0, **path_arm_kwargs(arm, torch)))
    for v in (got["joints"], got["clearance"], arm, start):
        v.setflags(write=False)
    assert (got["index"] >= 0).sum() >= 80 and (got["index"] < 0).sum() >= 5, "solved and skipped waypoints are both needed"
    return solver, got["joints"], got["clearance"], arm, start


# ------------------------------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("shape", SHAPES)
def test_an_edge_is_the_minimum_of_rsik_clearance_over_its_samples(torch_mod, shape):
    torch = torch_mod
    solver, joints, _, arm, start = shape_case(shape)
    for n_sub in (1, 4, 16):
        for st in (None, start):
            what = f"{shape} S {n_sub} start {st is not None}"
            exp = compose(solver, joints, arm, torch, n_sub, st)
            got = run(solver, joints, arm, torch, n_sub, st)
            err = check(got, exp, what)
            wp = exp["wp"]
            print(f"{what}: {int(wp.sum())} edges, {int((got['edge_sub'][wp] % n_sub != 0).sum())} with the minimum strictly inside, "
                  f"|edge_bound - formula| {err:.2e}")
            assert (got["edge_sub"][wp & ~exp["have_a"]] == n_sub).all(), what + ": the one-sample edge is numbered S"
            if n_sub == 16:
                assert (got["edge_sub"][wp] % n_sub != 0).sum() >= 3, what + ": no edge dips between its ends"


# ------------------------------------------------------------------------------------------ 2. S = 1
@pytest.mark.parametrize("shape", SHAPES)
def test_one_sub_step_is_the_smaller_of_the_two_ends(torch_mod, shape):
    """n_sub = 1 without start rows: edge_clearance has the bits of the smaller of rsik_solve_path_clear's `clearance` at the edge's two
    waypoints (the first waypoint: its own)."""
    torch = torch_mod
    solver, joints, clearance, arm, _ = shape_case(shape)
    got = run(solver, joints, arm, torch, 1, want=("edge_clearance", "edge_sub"))
    t, n = clearance.shape
    want = np.full((t, n), np.nan)
    last = np.full(n, np.inf)
    for s in range(t):
        here = ~np.isnan(clearance[s])
        want[s, here] = np.minimum(last, clearance[s])[here]
        last = np.where(here, clearance[s], last)
    np.testing.assert_array_equal(bits(got["edge_clearance"]), bits(want), err_msg=str(shape))
    assert (np.isnan(want) == (got["edge_sub"] == -1)).all()


# ------------------------------------------------------------------------------------------ 3. edge_bound
def test_the_bound_lies_below_a_finer_sampling(torch_mod):
    """(12, 8, 11, r) at S = 4 and 16: edge_bound <= the library's own rsik_clearance minimum over 8 S sub-steps + 1e-9 on every edge."""
    torch = torch_mod
    solver, joints, _, arm, start = shape_case(SHAPES[0])
    for n_sub in (4, 16):
        got = run(solver, joints, arm, torch, n_sub, start, want=("edge_clearance", "edge_bound"))
        fine = compose(solver, joints, arm, torch, 8 * n_sub, start)
        wp = fine["wp"]
        slack = (fine["edge_clearance"] - got["edge_bound"])[wp]
        free = float((got["edge_bound"][wp] > 0).mean())
        print(f"S {n_sub}: {int(wp.sum())} edges, smallest (minimum over {8 * n_sub} sub-steps - edge_bound) {float(slack.min()):.3e} m, "
              f"{100 * free:.1f} % of the edges proven free")
        assert (slack >= -EW.BOUND_SLACK).all(), (n_sub, float(slack.min()))
        assert (got["edge_bound"][wp] <= got["edge_clearance"][wp]).all()
        if n_sub == 16:
            assert free >= 0.5


# ------------------------------------------------------------------------------------------ 4. the path outputs
def test_the_path_outputs_are_the_fold_of_the_edges(torch_mod):
    """min_clearance in {-inf, 0, 0.02}; exact ties (paths that stand still: every sample of every edge has the same d) go to the lowest
    t and the lowest s; a scene in the reverse order gives the same clearances, bounds and counts."""
    torch = torch_mod
    solver, joints, _, arm, start = shape_case(SHAPES[0])
    t, n = joints.shape[:2]
    still = np.broadcast_to(path_start(5, 2)[None], (t, 2, 7))
    J = np.concatenate([joints, still], axis=1)
    A = np.concatenate([arm, [0, 0]]).astype(np.uint8)
    sc = PC.the_scene()
    back = dict(spheres=sc["spheres"][::-1].copy(), capsules=sc["capsules"][::-1].copy())
    for hard in (-np.inf, 0.0, 0.02):
        got = run(solver, J, A, torch, 16, None, min_clearance=hard)
        check(got, compose(solver, J, A, torch, 16, None, min_clearance=hard), f"min_clearance {hard}", hard)
        assert got["path_edge"][n:].tolist() == [[0, 16], [0, 16]] and (got["edge_sub"][1:, n:] == 0).all(), "ties: the lowest t, the lowest s"
        assert (got["edge_clearance"][:, n:] == got["edge_clearance"][0, n:]).all()
        rev = run(solver, J, A, torch, 16, None, scene=back, min_clearance=hard)
        same(rev, got, f"the scene in reverse order, min_clearance {hard}", keys=("edge_clearance", "edge_sub", "edge_bound") + PATH)
        if hard == 0.02:
            assert (got["n_below"] > 0).sum() >= 10 and (got["n_below"] == 0).sum() >= 2 and (got["first_below"] > 0).sum() >= 3
        if hard == -np.inf:
            assert (got["n_below"] == 0).all() and (got["first_below"] == -1).all()


# ------------------------------------------------------------------------------------------ 5. independence
def test_outputs_launches_and_paths_are_independent(torch_mod):
    torch = torch_mod
    solver, joints, _, arm, start = shape_case(SHAPES[1])  # (70, 3, 21, mixed)
    t, n = joints.shape[:2]
    full = run(solver, joints, arm, torch, 16, start, min_clearance=0.0)
    same(run(solver, joints, arm, torch, 16, start, min_clearance=0.0), full, "a second launch")
    for key in EVERY:
        same(run(solver, joints, arm, torch, 16, start, min_clearance=0.0, want=(key,)), full, f"{key} alone", keys=(key,))
    for i in (0, n - 1):
        one = run(solver, joints[:, i:i + 1], arm[i:i + 1], torch, 16, start[i:i + 1], min_clearance=0.0)
        same(one, {k: (v[:, i:i + 1] if k in EDGE else v[i:i + 1]) for k, v in full.items()}, f"path {i} alone")
    perm = np.random.default_rng(3).permutation(n)
    shuffled = run(solver, joints[:, perm], arm[perm], torch, 16, start[perm], min_clearance=0.0)
    same(shuffled, {k: (v[:, perm] if k in EDGE else v[perm]) for k, v in full.items()}, "the paths in another order")
    for side in (0, 1):  # a uniform launch of either arm against the mixed launch's paths of that arm
        rows = np.flatnonzero(arm == side)
        assert len(rows) >= 5
        uni = run(solver, joints[:, rows], arm[rows], torch, 16, start[rows], min_clearance=0.0)
        same(uni, {k: (v[:, rows] if k in EDGE else v[rows]) for k, v in full.items()}, f"arm {side} uniform")
    other = np.ones(n, dtype=np.uint8)  # the same joints on the left arm alone: another answer, and the composition's
    check(run(solver, joints, other, torch, 4, start), compose(solver, joints, other, torch, 4, start), "uniform l")


# ------------------------------------------------------------------------------------------ 6. rows that are not numbers
def test_rows_that_are_not_numbers(torch_mod):
    torch = torch_mod
    solver, joints, _, arm, start = shape_case(SHAPES[0])
    t, n = joints.shape[:2]
    full = run(solver, joints, arm, torch, 16, start)
    J = np.array(joints)
    holes = {3: [0], 8: [t - 1], 12: [5], 20: [6, 7], 25: [0, 1, t - 1]}
    for i, ts in holes.items():
        J[ts, i, 2] = np.nan
    J[4, 30, 6] = np.inf
    touched = sorted(list(holes) + [30])
    rest = np.setdiff1d(np.arange(n), touched)
    for st in (None, start):
        got = run(solver, J, arm, torch, 16, st)
        exp = compose(solver, J, arm, torch, 16, st)
        check(got, exp, f"NaN rows, start {st is not None}")
        for i, ts in holes.items():
            assert (got["edge_sub"][ts, i] == -1).all()
        if st is not None:
            same(got, full, "the other paths", paths=rest)
    wp = np.isfinite(J).all(axis=2)
    bridges = sum(int(wp[s, i] and not wp[s - 1, i] and not wp[s - 2, i] and wp[:s - 2, i].any()) for i in range(n) for s in range(3, t))
    assert bridges >= 3, "edges that bridge two consecutive rows that are not waypoints are needed"
    # an infinity in a start row loses that path only
    st = np.array(start)
    st[7, 0] = np.inf
    got = run(solver, joints, arm, torch, 16, st)
    assert np.isnan(got["edge_clearance"][:, 7]).all() and (got["edge_sub"][:, 7] == -1).all() and (got["edge_nearest"][:, 7] == -1).all()
    assert np.isnan(got["edge_bound"][:, 7]).all() and np.isnan(got["path_clearance"][7]) and np.isnan(got["path_bound"][7])
    assert got["path_edge"][7].tolist() == [-1, -1] and got["n_below"][7] == 0 and got["first_below"][7] == -1
    same(got, full, "the paths beside the lost one", paths=np.setdiff1d(np.arange(n), [7]))
    # the scene's skipped obstacles change nothing but the index
    sc = PC.the_scene()
    ok_s, ok_c = usable(sc["spheres"]), usable(sc["capsules"])
    assert (~ok_s).sum() == 3 and (~ok_c).sum() == 1
    clean = run(solver, joints, arm, torch, 16, start, scene=dict(spheres=sc["spheres"][ok_s], capsules=sc["capsules"][ok_c]))
    same(clean, full, "without the skipped obstacles", keys=("edge_clearance", "edge_sub", "edge_bound", "path_clearance", "path_edge", "path_bound"))
    shift = np.concatenate([np.cumsum(ok_s) - 1, ok_s.sum() + np.cumsum(ok_c) - 1])
    wp = full["edge_sub"] >= 0
    np.testing.assert_array_equal(shift[full["edge_nearest"][wp][:, 1]], clean["edge_nearest"][wp][:, 1])
    # every obstacle skipped
    for st in (None, start):
        none = run(solver, joints, arm, torch, 16, st, scene=dict(spheres=sc["spheres"][~ok_s], capsules=sc["capsules"][~ok_c]))
        wp, have_a, _ = EW.edges_of(joints, st)
        assert np.isposinf(none["edge_clearance"][wp]).all() and np.isposinf(none["edge_bound"][wp]).all() and (none["edge_nearest"] == -1).all()
        np.testing.assert_array_equal(none["edge_sub"], np.where(wp, np.where(have_a, 0, 16), -1))
        has = wp.any(axis=0)
        assert np.isposinf(none["path_clearance"][has]).all() and np.isnan(none["path_clearance"][~has]).all()
        np.testing.assert_array_equal(none["path_edge"][has, 0], np.argmax(wp, axis=0)[has])


# ------------------------------------------------------------------------------------------ 7. the edges of the shape
def test_one_waypoint(torch_mod):
    torch = torch_mod
    solver, joints, _, arm, start = shape_case(SHAPES[0])
    for rows in (slice(3, 4), slice(3, 6)):  # T = 1, and T = 3: the fold's narrowest groups
        row = np.ascontiguousarray(joints[rows])
        for st in (None, start):
            got = run(solver, row, arm, torch, 16, st, min_clearance=0.0)
            check(got, compose(solver, row, arm, torch, 16, st, min_clearance=0.0), f"T = {len(row)}, start {st is not None}", 0.0)
            if st is None and len(row) == 1:
                wp = np.isfinite(row).all(axis=2)
                assert (got["edge_sub"][wp] == 16).all() and np.array_equal(bits(got["edge_bound"]), bits(got["edge_clearance"]))


@pytest.mark.parametrize("n_sub", (1, 63, 64, 65, 256))
def test_sub_steps_on_both_sides_of_a_wave(torch_mod, n_sub):
    torch = torch_mod
    solver, joints, _, arm, start = shape_case(SHAPES[2])  # (5, 64, 31, mixed)
    for rows in (slice(None), slice(0, 1)):  # the whole launch, and one path alone (the widest groups)
        J, a, st = np.ascontiguousarray(joints[:, rows]), arm[rows], start[rows]
        check(run(solver, J, a, torch, n_sub, st), compose(solver, J, a, torch, n_sub, st), f"S {n_sub} paths {rows}")


def test_more_than_one_workgroup_and_the_largest_scenes(torch_mod):
    torch = torch_mod
    solver, joints, _, arm, start = shape_case(SHAPES[0])
    n = joints.shape[1]
    pick = np.random.default_rng(9).integers(0, n, 130)
    J, A, st = np.ascontiguousarray(joints[:, pick]), arm[pick], start[pick]
    full = run(solver, joints, arm, torch, 16, start)
    wide = run(solver, J, A, torch, 16, st)
    same(wide, {k: (v[:, pick] if k in EDGE else v[pick]) for k, v in full.items()}, "n = 130")
    sc = PC.the_scene()
    rng = np.random.default_rng(77)
    pad_s = np.concatenate([rng.uniform(-1, 1, size=(232, 3)) + [20.0, 0.0, 0.0], rng.uniform(0.01, 0.1, size=(232, 1))], axis=1)
    a = rng.uniform(-1, 1, size=(56, 3)) + [0.0, 20.0, 0.0]
    pad_c = np.concatenate([a, a + rng.uniform(-0.3, 0.3, size=(56, 3)), rng.uniform(0.01, 0.1, size=(56, 1))], axis=1)
    big = dict(spheres=np.concatenate([pad_s, sc["spheres"]]), capsules=np.concatenate([pad_c, sc["capsules"]]))
    assert len(big["spheres"]) == 256 and len(big["capsules"]) == 64
    got = run(solver, joints, arm, torch, 16, start, scene=big)
    same(got, full, "256 + 64 obstacles", keys=("edge_clearance", "edge_sub", "edge_bound", "path_clearance", "path_edge", "path_bound"))
    wp = full["edge_sub"] >= 0
    S = len(sc["spheres"])
    moved = full["edge_nearest"][wp][:, 1]
    np.testing.assert_array_equal(got["edge_nearest"][wp][:, 1], np.where(moved < S, moved + 232, moved + 232 + 56))
    for name, scene in (("one sphere", dict(spheres=sc["spheres"][:1], capsules=np.zeros((0, 7)))),
                        ("capsules alone", dict(spheres=np.zeros((0, 4)), capsules=sc["capsules"]))):
        check(run(solver, joints, arm, torch, 4, start, scene=scene), compose(solver, joints, arm, torch, 4, start, scene=scene), name)


@pytest.mark.parametrize("copies", (28, 56, 112, 222, 450))
def test_every_number_of_lanes_per_edge(torch_mod, copies):
    """The host spreads an edge's samples over 32 lanes at this file's sizes and over fewer as the edges grow in number: 16, 8, 4, 2
    and, above 131 072 edges, one lane per edge.  The 37 paths copied `copies` times over give each of them; a path's bits depend
    neither on n nor on its place, so every copy has the small launch's bits."""
    torch = torch_mod
    solver, joints, _, arm, start = shape_case(SHAPES[0])
    t, n = joints.shape[:2]
    full = run(solver, joints, arm, torch, 16, start, min_clearance=0.0)
    wide = run(solver, np.tile(joints, (1, copies, 1)), np.tile(arm, copies), torch, 16, np.tile(start, (copies, 1)), min_clearance=0.0)
    assert wide["edge_clearance"].shape == (t, n * copies)
    same(wide, {k: (np.tile(v, (1, copies) + (1,) * (v.ndim - 2)) if k in EDGE else np.tile(v, (copies,) + (1,) * (v.ndim - 1))) for k, v in full.items()},
         f"{copies} copies")


def test_rows_wound_by_whole_turns(torch_mod):
    """Waypoints wound by whole turns past 2^27 rad, in a start row too: the composition's bits (rsik_clearance answers a finite angle of
    any size, and angle_diff takes the short way round whatever the winding)."""
    torch = torch_mod
    solver, joints, _, arm, start = shape_case(SHAPES[0])
    J, st = np.array(joints), np.array(start)
    turns = 2 * np.pi * 3.0e7
    assert turns > 2.0 ** 27
    J[4, 1:9] += turns
    J[7, 5:12, 3] -= 2 * turns
    st[2, 0] += turns
    got = run(solver, J, arm, torch, 4, st)
    check(got, compose(solver, J, arm, torch, 4, st), "wound rows")
    plain = run(solver, joints, arm, torch, 4, start)
    diff = np.abs(got["edge_clearance"] - plain["edge_clearance"])
    print(f"wound rows: edge_clearance moves by at most {float(np.nanmax(diff)):.3e} m")
    assert np.nanmax(diff) < 1e-6  # (2 pi k is not a whole turn in float64: 3e7 turns are 1e-8 rad off)


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_write_nothing(torch_mod):
    torch = torch_mod
    solver, joints, _, arm, start = shape_case(SHAPES[0])
    _abi = abi()
    t, n = joints.shape[:2]
    sc = PC.the_scene()
    j, sp, cp = T(joints, torch), T(sc["spheres"], torch), T(sc["capsules"], torch)
    rad = (C.c_double * 3)(*LINK_RADIUS)
    ws_bytes = solver.clearance_edges_workspace_bytes(n, t)
    ws = torch.empty(ws_bytes + 8, dtype=torch.uint8, device="cuda")
    shapes = {"edge_clearance": (t, n), "edge_sub": (t, n), "edge_nearest": (t, n, 2), "edge_bound": (t, n), "path_clearance": (n,),
              "path_edge": (n, 2), "path_bound": (n,), "n_below": (n,), "first_below": (n,)}
    ints = ("edge_sub", "edge_nearest", "path_edge", "n_below", "first_below")
    outs = {k: (torch.full(s + (2,), -77, dtype=torch.int32, device="cuda") if k in ints else torch.full(s + (2,), -77.0, dtype=torch.float64, device="cuda"))
            for k, s in shapes.items()}  # (twice the size: room for a pointer 4 bytes off)

    def call(**ch):
        a = dict(n=n, t=t, joints=ptr(j), arm=None, arm_uniform=0, start=None, n_sub=16, rad=rad, ns=len(sc["spheres"]), sp=ptr(sp),
                 nc=len(sc["capsules"]), cp=ptr(cp), hard=0.0, ws=ptr(ws), wsb=ws_bytes, **{k: ptr(v) for k, v in outs.items()})
        a.update(ch)
        return raw_call(solver, "rsik_clearance_edges", a["n"], a["t"], a["joints"], a["arm"], a["arm_uniform"], a["start"], a["n_sub"],
                        a["rad"], a["ns"], a["sp"], a["nc"], a["cp"], a["hard"], a["ws"], a["wsb"], *[a[k] for k in EVERY])

    bad_rad = lambda v: (C.c_double * 3)(0.03, v, 0.04)  # noqa: E731
    refused = {
        "n < 0": dict(n=-1), "n_steps 0": dict(t=0), "n_steps 65537": dict(t=65537), "n_sub 0": dict(n_sub=0), "n_sub 257": dict(n_sub=257),
        "joints NULL": dict(joints=None), "n_spheres -1": dict(ns=-1), "n_spheres 257": dict(ns=257), "n_capsules -1": dict(nc=-1),
        "n_capsules 65": dict(nc=65), "no obstacle": dict(ns=0, nc=0), "spheres NULL": dict(sp=None), "capsules NULL": dict(cp=None),
        "a negative radius": dict(rad=bad_rad(-0.01)), "a NaN radius": dict(rad=bad_rad(float("nan"))), "an infinite radius": dict(rad=bad_rad(float("inf"))),
        "min_clearance NaN": dict(hard=float("nan")), "min_clearance +inf": dict(hard=float("inf")),
        "no workspace": dict(ws=None), "a short workspace": dict(wsb=ws_bytes - 1),
        "edge_nearest 4 bytes off": dict(edge_nearest=ptr(outs["edge_nearest"]) + 4), "path_edge 4 bytes off": dict(path_edge=ptr(outs["path_edge"]) + 4),
        "all nine NULL": {k: None for k in EVERY}, "arm_uniform 2": dict(arm_uniform=2),
    }
    for what, ch in refused.items():
        assert call(**ch) == _abi.RSIK_E_INVALID, (what, last_error(solver))
        assert "rsik_clearance_edges" in last_error(solver), what
    solver.synchronize()
    for k, v in outs.items():
        assert bool((v == -77).all()), f"a refused call wrote {k}"
    # what is NOT refused: no workspace where no path output is asked for; n == 0 with nothing else
    assert call(ws=None, wsb=0, **{k: None for k in PATH}) == _abi.RSIK_OK
    assert call(n=0, joints=None, ws=None, wsb=0) == _abi.RSIK_OK
    solver.synchronize()
    got = {k: outs[k].cpu().numpy().reshape(-1)[:int(np.prod(shapes[k]))].reshape(shapes[k]) for k in EDGE}
    same(got, run(solver, joints, arm, torch, 16, None), "the edge outputs without a workspace", keys=EDGE)
    for k in PATH:
        assert bool((outs[k] == -77).all()), k
