"""GPU tests (-m gpu, MI355X) of rsik_solve_path_pair (csrc/rsik_kernel_path_pair.hpp, solve_path_pair_kernel): rsik_solve_path_clear for
robots of two arms, each arm an obstacle to the other, a state being a pair of samples.

The entry point is defined against rsik_solve_sweep and rsik_clearance: the expected value is tests/path_pair_workload.path_pair_dp on
the library's own sweep over the same T * n poses (arm bytes 0, 1, 0, 1, ...) and a table d [K][K][T][robots][2] from the library's own
rsik_clearance — one launch per (robot, waypoint, partner sample) and view, with n_rep = K rows against the static scene followed by
the partner sample's three capsules, built from rsik_clearance's link_points with track_pair_workload.partner_capsules' construction —
so the mask and the penalty are exact.  The table keeps `nearest` beside the clearance.  A launch is accepted when
  (a) theta / joints / elbow / projected at (t, r) have the BITS of the sweep's sample index[t][r]; the skipped waypoints, n_solved and
      `blocked` are NumPy's exactly; clearance and nearest of both views are the table's bits at the winning pair, which are
      rsik_clearance's on the returned joints (test_clearance_and_nearest_are_rsik_clearance_of_the_returned_joints launches that
      again on the returned rows); no winner lies below min_clearance in either view; interval / reachable / state are the sweep's,
  (b) the cost of the device's path, recomputed by NumPy along `index`, and `cost` itself are within 6 T COST_TOL of NumPy's optimum
      (path_pair_workload.path_pair_tol: its premises asserted), and step_cost^2 per row within the same bound,
  (c) on every robot whose second-best distinct path is more than GAP above the optimum, index is NumPy's exactly."""
import ctypes as C
import functools

import numpy as np
import pytest

import path_pair_workload as PP
from compare import as_bits, bits
from gpu_support import T, abi, cols, last_error, make_symbolic_dual, ptr, raw_call, to_np, torch_mod  # noqa: F401
from path_workload import GAP, path_fractions, path_start
from sampling_support import lib_sweep, path_soa

pytestmark = pytest.mark.gpu

PER_ROW = ("index", "theta", "joints", "elbow", "projected", "step_cost", "interval", "reachable", "state", "clearance", "nearest")
PER_ROBOT = ("cost", "n_solved")
EVERY = PER_ROW + PER_ROBOT + ("blocked",)
FULL = dict(min_clearance=0.0, influence=0.05, clearance_gain=100.0)


def scene_kw(torch, scene):
    sc = PP.NO_SCENE if scene is None else scene
    return dict(spheres=T(sc["spheres"], torch) if len(sc["spheres"]) else None,
                capsules=T(sc["capsules"], torch) if len(sc["capsules"]) else None, link_radius=PP.LINK_RADIUS)


def capsule_lists(solver, joints, arm_rows, torch, scene):
    """For every row of joints [..., rows, 7] the capsule list its PARTNER sees: the scene's capsules followed by the three of that
    row's links, from rsik_clearance's link_points: [..., rows, C + 3, 7] on the device."""
    sc = PP.NO_SCENE if scene is None else scene
    lp = solver.clearance(joints, spheres=torch.tensor([[50.0, 0.0, 0.0, 0.1]], dtype=torch.float64), want=("link_points",),
                          arm=T(arm_rows, torch))["link_points"]
    rad = torch.as_tensor(np.asarray(PP.LINK_RADIUS)).cuda().expand(lp.shape[:-2] + (3,))[..., None]
    own = torch.cat([lp[..., :3, :], lp[..., 1:, :], rad], dim=-1)
    static = T(np.asarray(sc["capsules"], dtype=np.float64).reshape(-1, 7), torch)
    return torch.cat([static.expand(lp.shape[:-2] + static.shape), own], dim=-2).contiguous()


@functools.lru_cache(maxsize=None)
def shape_case(t, k, seed, robots, with_scene=False):
    """A shape's inputs, the library's sweep over them and the library's clearance of every pair of that sweep's samples, in both
    views: computed once, shared.  d [K][K][T][robots][2] and near [K][K][T][robots][2][2]."""
    import torch

    solver, _, dual = make_symbolic_dual(0.03)
    n = 2 * robots
    scene = PP.the_scene() if with_scene else None
    pos, eul, arm = PP.pair_poses(seed, robots, t)
    p, th = path_soa(pos, eul, torch), T(path_fractions(k), torch)
    sw = lib_sweep(solver, p, th, "fraction", arm, torch)
    jt = T(sw["joints"], torch)  # [K, t n, 7]
    caps = capsule_lists(solver, jt, np.tile(arm, t), torch, scene)  # [K, t n, C + 3, 7]
    skw = scene_kw(torch, scene)
    own = jt.reshape(k, t, n, 7).permute(1, 2, 0, 3).contiguous()  # [t, n, K, 7]
    dt = torch.full((t, n, k, k, 1), float("nan"), dtype=torch.float64, device="cuda")      # [t, row, partner sample, own sample]
    nt = torch.full((t, n, k, k, 1, 2), -1, dtype=torch.int32, device="cuda")
    row_ok = (sw["reachable"].reshape(t, n) != 0)[None] & ~np.isnan(sw["joints"]).any(axis=-1).reshape(k, t, n)
    launches = 0
    for s in range(t):
        for r in range(n):
            if not row_ok[:, s, r].any():
                continue
            mine = own[s, r].reshape(k, 1, 7)
            for b in np.flatnonzero(row_ok[:, s, r ^ 1]):
                solver.clearance(mine, spheres=skw["spheres"], capsules=caps[b, s * n + (r ^ 1)], link_radius=PP.LINK_RADIUS, arm_uniform=r & 1,
                                 out={"clearance": dt[s, r, b], "nearest": nt[s, r, b]})
                launches += 1
    dt, nt = dt.cpu().numpy()[..., 0], nt.cpu().numpy()[..., 0, :]
    d = np.empty((k, k, t, robots, 2))
    near = np.empty((k, k, t, robots, 2, 2), dtype=np.int32)
    d[..., 0] = dt[:, 0::2].transpose(3, 2, 0, 1)          # dR(a, b): own a, partner b
    d[..., 1] = dt[:, 1::2].transpose(2, 3, 0, 1)          # dL(a, b): own b, partner a
    near[..., 0, :] = nt[:, 0::2].transpose(3, 2, 0, 1, 4)
    near[..., 1, :] = nt[:, 1::2].transpose(2, 3, 0, 1, 4)
    print(f"T {t} K {k} seed {seed} robots {robots} scene {with_scene}: {launches} rsik_clearance launches for the table")
    for v in list(sw.values()) + [d, near]:
        v.setflags(write=False)
    return solver, dual, p, th, sw, d, near, scene


def run_pair(solver, p, th, start, torch, scene=None, **kw):
    return to_np(solver.solve_path_pair(p, th, None if start is None else T(start, torch), **scene_kw(torch, scene), **kw))


def same_outputs(a, b, what, keys=EVERY, robots=None):
    for key in keys:
        x, y = a[key], b[key]
        if robots is not None:
            rows = np.stack([2 * np.asarray(robots), 2 * np.asarray(robots) + 1], axis=1).reshape(-1)
            x, y = (x[:, rows], y[:, rows]) if key in PER_ROW else (x[robots], y[robots]) if key in PER_ROBOT else (x[:, robots], y[:, robots])
        np.testing.assert_array_equal(as_bits(x), as_bits(y), err_msg=f"{what}: {key}")


def check_pair(got, sw, d, near, t, robots, what, hard, influence, gain, start=None, weights=None, skip=False, need_gap=False):
    """(a) - (c) for one launch `got` against the library's sweep `sw` and its table of the pairs' clearances."""
    n = 2 * robots
    exp = PP.path_pair_dp(sw, d, t, robots, hard, influence, gain, start, weights, skip)
    idx = got["index"]
    k = sw["joints"].shape[0]
    assert idx.dtype == np.int32 and idx.shape == (t, n) and got["n_solved"].dtype == np.int32 and got["n_solved"].shape == (robots,), what
    # (a)
    np.testing.assert_array_equal(idx == -1, np.repeat(~exp["solved"], 2, axis=1), err_msg=what + ": the skipped waypoints")
    np.testing.assert_array_equal(got["n_solved"], exp["n_solved"], err_msg=what)
    assert got["blocked"].shape == (t, robots) and got["blocked"].dtype == np.int16, (what, got["blocked"].dtype)
    np.testing.assert_array_equal(got["blocked"].view(np.uint16), exp["blocked"], err_msg=what + ": blocked")
    assert (idx < k).all(), (what, "index past K", int(idx.max(initial=-1)))
    tt, ii = np.nonzero(idx >= 0)
    pose = tt * n + ii
    for key in ("theta", "joints", "elbow"):
        np.testing.assert_array_equal(bits(got[key][tt, ii]), bits(sw[key][idx[tt, ii], pose]), err_msg=f"{what}: {key} is not the sweep's sample")
        assert np.isnan(got[key][idx < 0]).all(), (what, key)
    np.testing.assert_array_equal(got["projected"][tt, ii], sw["projected"][idx[tt, ii], pose], err_msg=what + ": projected")
    assert (got["projected"][idx < 0] == 0).all() and got["projected"].dtype == np.uint8, (what, "projected")
    assert np.isnan(got["step_cost"][idx < 0]).all() and not np.isnan(got["step_cost"][idx >= 0]).any(), (what, "step_cost NaN pattern")
    for key in ("interval", "reachable", "state"):
        np.testing.assert_array_equal(as_bits(got[key].reshape((t * n,) + got[key].shape[2:])), as_bits(sw[key]), err_msg=f"{what}: {key}")
    assert got["nearest"].dtype == np.int32 and got["nearest"].shape == (t, n, 2), (what, got["nearest"].dtype)
    ts, rs = np.nonzero(idx[:, 0::2] >= 0)
    a, b = idx[ts, 2 * rs], idx[ts, 2 * rs + 1]
    for view in (0, 1):
        np.testing.assert_array_equal(bits(got["clearance"][ts, 2 * rs + view]), bits(d[a, b, ts, rs, view]), err_msg=f"{what}: clearance, view {view}")
        np.testing.assert_array_equal(got["nearest"][ts, 2 * rs + view], near[a, b, ts, rs, view], err_msg=f"{what}: nearest, view {view}")
    assert np.isnan(got["clearance"][idx < 0]).all() and (got["nearest"][idx < 0] == -1).all(), (what, "a skipped waypoint's clearance")
    with np.errstate(invalid="ignore"):
        assert (got["clearance"][idx >= 0] >= hard).all(), (what, "a winner below min_clearance")
    # (b)
    tol = PP.path_pair_tol(t)
    has = exp["n_solved"] > 0
    along, step2 = PP.pair_cost_along(sw, exp["penalty"], idx, t, robots, start, weights)
    assert (along[has] < PP.COST_SUM_MAX).all() and (exp["cost"][has] < PP.COST_SUM_MAX).all(), (what, "the running sum")
    excess = along[has] - exp["cost"][has]
    err_cost = np.abs(got["cost"][has] - along[has])
    err_steps = np.abs(got["step_cost"] ** 2 - step2)[idx >= 0]
    gaps = exp["gap"][exp["n_solved"] > (0 if start is not None else 1)]
    print(f"{what}: {int(has.sum())} robots, device path - optimum in [{float(excess.min(initial=0.0)):.3e}, {float(excess.max(initial=0.0)):.3e}], "
          f"|cost - recomputed| {float(err_cost.max(initial=0.0)):.3e}, |step_cost^2 - recomputed| {float(err_steps.max(initial=0.0)):.3e}, tol {tol:.1e}, "
          f"smallest gap {float(gaps.min(initial=np.inf)):.2e}, blocked cells {int((exp['blocked'] > 0).sum())}")
    assert (np.abs(excess) <= tol).all(), (what, float(np.abs(excess).max(initial=0.0)))
    assert (err_cost <= tol).all() and np.isnan(got["cost"][~has]).all(), (what, float(err_cost.max(initial=0.0)))
    assert (np.abs(got["cost"][has] - exp["cost"][has]) <= tol).all(), what
    assert (err_steps <= tol).all(), (what, float(err_steps.max(initial=0.0)))
    # (c)  (without start rows and without a penalty a path with one solved waypoint is an exact tie at 0: the lowest pair's)
    if need_gap:
        assert (gaps > GAP).all(), (what, float(gaps.min()))
    clear = exp["gap"] > GAP
    if start is None and gain == 0.0:
        clear = clear | (exp["n_solved"] == 1)
    np.testing.assert_array_equal(idx[:, np.repeat(clear, 2)], exp["index"][:, np.repeat(clear, 2)], err_msg=what + ": index where the gap is clear")
    return exp


# ------------------------------------------------------------------------------------------ 1. the three acceptance points
@pytest.mark.parametrize("shape", [s + (False,) for s in PP.MAIN_SHAPES + PP.SMALL_SHAPES] + [PP.MAIN_SHAPES[0] + (True,)])
def test_both_arms_keep_their_clearance_and_the_pair_of_paths_is_the_optimum(torch_mod, shape):
    torch = torch_mod
    t, k, seed, robots, with_scene = shape
    solver, _, p, th, sw, d, near, scene = shape_case(*shape)
    main = shape[:4] in PP.MAIN_SHAPES
    for start in (None, path_start(seed, 2 * robots)):
        exps = {}
        for hard in PP.HARD:
            for influence, gain in PP.SOFT:
                what = f"T {t} K {k} seed {seed} robots {robots} scene {with_scene} start {start is not None} min_clearance {hard} ({influence}, {gain})"
                got = run_pair(solver, p, th, start, torch, scene, min_clearance=hard, influence=influence, clearance_gain=gain)
                exps[hard, gain] = check_pair(got, sw, d, near, t, robots, what, hard, influence, gain, start, need_gap=main)
        if shape == PP.MAIN_SHAPES[0] + (False,):  # the conditions on the inputs: the coupling matters
            free = exps[-np.inf, 0.0]
            differ = lambda e: int((e["index"] != free["index"]).any(axis=0).sum())  # noqa: E731
            lost = int((free["solved"] & ~exps[0.0, 0.0]["solved"]).sum())
            partly = int((exps[0.0, 0.0]["solved"] & (exps[0.0, 0.0]["blocked"] > 0)).sum())
            print(f"start {start is not None}: rows changed by min_clearance 0: {differ(exps[0.0, 0.0])}, by the soft term: {differ(exps[-np.inf, 100.0])}; "
                  f"{lost} solved waypoints lost, {partly} cells partly blocked")
            assert differ(exps[0.0, 0.0]) >= 1 and differ(exps[-np.inf, 100.0]) >= 1 and lost >= 1 and partly >= 10


def test_clearance_and_nearest_are_rsik_clearance_of_the_returned_joints(torch_mod):
    """One rsik_clearance launch per returned row, with the static scene followed by the three capsules built from the PARTNER's
    returned joints: the same bits."""
    torch = torch_mod
    shape = PP.MAIN_SHAPES[0] + (True,)
    t, k, seed, robots, _ = shape
    n = 2 * robots
    solver, _, p, th, sw, d, near, scene = shape_case(*shape)
    got = run_pair(solver, p, th, path_start(seed, n), torch, scene, **FULL)
    arm = np.tile(np.array([0, 1], dtype=np.uint8), robots)
    jt = T(got["joints"], torch)
    caps = capsule_lists(solver, jt, arm, torch, scene)  # [t, n, C + 3, 7]
    skw = scene_kw(torch, scene)
    clr = torch.full((t, n, 1), float("nan"), dtype=torch.float64, device="cuda")
    nr = torch.full((t, n, 1, 2), -1, dtype=torch.int32, device="cuda")
    won = got["index"] >= 0
    assert won.sum() >= 100
    for s, r in zip(*np.nonzero(won)):
        solver.clearance(jt[s, r].reshape(1, 7), spheres=skw["spheres"], capsules=caps[s, r ^ 1], link_radius=PP.LINK_RADIUS, arm_uniform=int(r & 1),
                         out={"clearance": clr[s, r], "nearest": nr[s, r]})
    np.testing.assert_array_equal(bits(got["clearance"]), bits(clr.cpu().numpy()[..., 0]))
    np.testing.assert_array_equal(got["nearest"], nr.cpu().numpy()[:, :, 0])
    partner = got["nearest"][..., 1][won] >= len(scene["spheres"]) + len(scene["capsules"])
    assert partner.any() and (~partner).any(), "winners nearest to the partner and nearest to the scene"


FAR_SHAPE = (6, 4, 239, 12)  # found on the checker: robots 2 and 5 hold their arms further apart than any of their samples is from the scene


def test_a_far_partner_leaves_the_rows_of_rsik_solve_path_clear(torch_mod):
    """With the static scene, on robots whose partner is far — every cross clearance of a pair of row candidates lies above every
    static clearance of a row candidate and above `influence`, asserted on the library's own values — and whose two arms solve the same
    waypoints alone, the index rows are rsik_solve_path_clear's where its gap is clear."""
    import path_clear_workload as PC

    torch = torch_mod
    t, k, seed, robots = FAR_SHAPE
    n = 2 * robots
    solver, _, p, th, sw, cross, _, _ = shape_case(*FAR_SHAPE, False)   # d without a scene: the partner alone
    _, _, _, _, sw2, d, near, scene = shape_case(*FAR_SHAPE, True)
    np.testing.assert_array_equal(as_bits(sw["joints"]), as_bits(sw2["joints"]))
    arm = np.tile(np.array([0, 1], dtype=np.uint8), robots)
    sk = scene_kw(torch, scene)
    static = solver.clearance(T(sw["joints"], torch), spheres=sk["spheres"], capsules=sk["capsules"], link_radius=PP.LINK_RADIUS,
                              arm=T(np.tile(arm, t), torch), want=("clearance",))["clearance"].cpu().numpy()  # [K, t n]
    start = path_start(seed, n)
    alone_exp = PC.path_clear_dp(sw, static, t, n, 0.0, 0.05, 100.0, start)
    row = alone_exp["base"]
    both = row[:, None, :, 0::2] & row[None, :, :, 1::2]
    far = []
    for i in range(robots):
        same_waypoints = (alone_exp["solved"][:, 2 * i] == alone_exp["solved"][:, 2 * i + 1]).all() and alone_exp["solved"][:, 2 * i].sum() >= 3
        nearest_cross = np.where(both[..., i][..., None], cross[:, :, :, i, :], np.inf).min()
        widest_static = np.where(row[:, :, 2 * i:2 * i + 2], static.reshape(k, t, n)[:, :, 2 * i:2 * i + 2], -np.inf).max()
        if same_waypoints and nearest_cross > widest_static and nearest_cross > 0.05 and (alone_exp["gap"][2 * i:2 * i + 2] > GAP).all():
            far.append(i)
    print(f"far robots: {far}")
    assert len(far) >= 2, far
    got = run_pair(solver, p, th, start, torch, scene, **FULL)
    check_pair(got, sw, d, near, t, robots, "the far shape", 0.0, 0.05, 100.0, start)
    alone = to_np(solver.solve_path_clear(p, th, T(start, torch), arm=T(arm, torch), **sk, **FULL))
    rows = np.stack([2 * np.array(far), 2 * np.array(far) + 1], axis=1).reshape(-1)
    np.testing.assert_array_equal(alone["index"][:, rows], alone_exp["index"][:, rows])
    np.testing.assert_array_equal(got["index"][:, rows], alone["index"][:, rows])
    assert (got["index"][:, rows] >= 0).sum() >= 12


# ------------------------------------------------------------------------------------------ 2. the flags and the thetas
def test_unwind_changes_joints_only_and_rows_are_continuous_per_arm(torch_mod):
    torch = torch_mod
    shape = PP.MAIN_SHAPES[0] + (False,)
    t, k, seed, robots, _ = shape
    n = 2 * robots
    solver, _, p, _, _, _, _, _ = shape_case(*shape)
    th = T(np.random.default_rng(seed + 300).uniform(-2 * np.pi, 2 * np.pi, size=(k, t, n)), torch)
    start = path_start(seed, n) + 4.0
    kw = dict(policy="explicit", **FULL)
    plain = run_pair(solver, p, th, start, torch, **kw)
    got = run_pair(solver, p, th, start, torch, unwind=True, **kw)
    same_outputs(got, plain, "everything but joints", keys=tuple(key for key in EVERY if key != "joints"))
    moved = (bits(got["joints"]) != bits(plain["joints"])).any(axis=2)
    assert moved.sum() >= 10
    for r in range(n):
        prev = start[r]
        for s in np.flatnonzero(got["index"][:, r] >= 0):
            want = prev + ((plain["joints"][s, r] - prev + np.pi) % (2 * np.pi) - np.pi)
            assert np.abs(got["joints"][s, r] - want).max() <= 1e-12 and np.abs(got["joints"][s, r] - prev).max() <= np.pi + 1e-12, (s, r)
            prev = got["joints"][s, r]


def test_skip_projected_and_explicit_thetas_per_pose(torch_mod):
    torch = torch_mod
    shape = PP.MAIN_SHAPES[0] + (False,)
    t, k, seed, robots, _ = shape
    n = 2 * robots
    solver, _, p, th, sw, d, near, _ = shape_case(*shape)
    start = path_start(seed, n)
    assert sw["projected"].sum() >= 100
    got = run_pair(solver, p, th, start, torch, skip_projected=True, **FULL)
    e1 = check_pair(got, sw, d, near, t, robots, "the flag", 0.0, 0.05, 100.0, start, skip=True)
    e0 = PP.path_pair_dp(sw, d, t, robots, 0.0, 0.05, 100.0, start)
    assert (got["projected"] == 0).all() and (e1["index"] != e0["index"]).any() and (e1["blocked"] <= e0["blocked"]).all()
    # one angle per waypoint, row and sample: the shared grid's bits where it repeats the grid, and a table of its own where it does not
    per = np.repeat(path_fractions(k)[:, None], t * n, axis=1).reshape(k, t, n)
    same_outputs(run_pair(solver, p, T(per, torch), start, torch, **FULL), run_pair(solver, p, th, start, torch, **FULL), "per pose against the shared grid")


def test_explicit_thetas_against_their_own_table(torch_mod):
    torch = torch_mod
    t, k, seed, robots = 5, 4, 51, 6
    n = 2 * robots
    solver, _, dual = make_symbolic_dual(0.03)
    pos, eul, arm = PP.pair_poses(seed, robots, t)
    p = path_soa(pos, eul, torch)
    th = np.random.default_rng(seed + 200).uniform(-np.pi, np.pi, size=(k, t, n))
    sw = lib_sweep(solver, p, T(th, torch), "explicit", arm, torch)
    exp_free = PP.path_pair_dp(sw, np.ones((k, k, t, robots, 2)), t, robots, -np.inf, 0.0, 0.0, path_start(seed, n))
    got = run_pair(solver, p, T(th, torch), path_start(seed, n), torch, policy="explicit")
    assert (exp_free["n_solved"] > 0).sum() >= 3
    np.testing.assert_array_equal(got["index"] == -1, exp_free["index"] == -1)
    clear = np.repeat(exp_free["gap"] > GAP, 2)
    np.testing.assert_array_equal(got["index"][:, clear], exp_free["index"][:, clear])
    tt, ii = np.nonzero(got["index"] >= 0)
    np.testing.assert_array_equal(bits(got["joints"][tt, ii]), bits(sw["joints"][got["index"][tt, ii], tt * n + ii]))
    np.testing.assert_array_equal(bits(got["theta"][tt, ii]), bits(sw["theta"][got["index"][tt, ii], tt * n + ii]))


# ------------------------------------------------------------------------------------------ 3. rows that are not numbers
def test_rows_that_are_not_numbers_stay_where_they_are(torch_mod):
    torch = torch_mod
    _abi = abi()
    shape = PP.MAIN_SHAPES[0] + (False,)
    t, k, seed, robots, _ = shape
    n = 2 * robots
    solver, _, p, th, _, _, _, _ = shape_case(*shape)
    start = path_start(seed, n)
    clean = run_pair(solver, p, th, start, torch, **FULL)
    busy = np.flatnonzero(clean["n_solved"] >= 4)
    assert len(busy) >= 4
    # a. a NaN start row loses its robot only
    bad = busy[:2]
    st2 = start.copy()
    st2[2 * bad[0], 3] = np.nan
    st2[2 * bad[1] + 1, 6] = np.inf
    got = run_pair(solver, p, th, st2, torch, **FULL)
    same_outputs(got, clean, "bad start rows: the other robots", robots=np.setdiff1d(np.arange(robots), bad))
    same_outputs(got, clean, "bad start rows: is_reachable's outputs", keys=("interval", "reachable", "state"))
    rows = np.stack([2 * bad, 2 * bad + 1], axis=1).reshape(-1)
    assert (got["n_solved"][bad] == 0).all() and (got["index"][:, rows] == -1).all() and np.isnan(got["cost"][bad]).all()
    assert (got["blocked"][:, bad] == 0).all() and np.isnan(got["clearance"][:, rows]).all() and (got["nearest"][:, rows] == -1).all()
    # b. a NaN pose in one arm skips that waypoint for both arms and reports INVALID_INPUT in that row only
    i = int(busy[2])
    s = int(np.flatnonzero(clean["index"][:, 2 * i] >= 0)[1])
    p2 = p.clone()
    p2[4, s, 2 * i + 1] = float("nan")
    got = run_pair(solver, p2, th, start, torch, **FULL)
    same_outputs(got, clean, "a bad pose: the other robots", robots=np.setdiff1d(np.arange(robots), [i]))
    assert got["state"][s, 2 * i + 1] == _abi.STATE_INVALID_INPUT and got["reachable"][s, 2 * i + 1] == 0
    assert got["state"][s, 2 * i] == clean["state"][s, 2 * i] and got["reachable"][s, 2 * i] == clean["reachable"][s, 2 * i] == 1
    assert (got["index"][s, 2 * i:2 * i + 2] == -1).all() and got["blocked"][s, i] == 0 and np.isnan(got["clearance"][s, 2 * i:2 * i + 2]).all()
    assert got["n_solved"][i] == clean["n_solved"][i] - 1


# ------------------------------------------------------------------------------------------ 4. arguments
def raw_pair(solver, n_pairs, t, p, k, policy, thetas, per_pose, start=None, weights=None, flags=0, radius=PP.LINK_RADIUS, n_spheres=None,
             spheres=None, n_capsules=None, capsules=None, hard=0.0, influence=0.05, gain=100.0, workspace=None, workspace_bytes=None,
             nearest_offset=0, **outs):
    """rsik_solve_path_pair on the caller's own buffers: returns the ABI's code."""
    w = None if weights is None else (C.c_double * 7)(*[float(v) for v in weights])
    r = None if radius is None else (C.c_double * 3)(*[float(v) for v in radius])
    if workspace_bytes is None:
        workspace_bytes = 0 if workspace is None else workspace.numel()
    n_spheres = (0 if spheres is None else int(spheres.shape[0])) if n_spheres is None else n_spheres
    n_capsules = (0 if capsules is None else int(capsules.shape[0])) if n_capsules is None else n_capsules
    o = [ptr(outs.get(key)) for key in ("index", "theta", "joints", "elbow", "projected", "step_cost", "cost", "n_solved", "interval",
                                         "reachable", "state", "clearance")]
    near = outs.get("nearest")
    o.append(None if near is None else near.data_ptr() + nearest_offset)
    o.append(ptr(outs.get("blocked")))
    return raw_call(solver, "rsik_solve_path_pair", n_pairs, t, cols(p, 6), int(k), int(policy), ptr(thetas), int(per_pose), ptr(start), w,
                    int(flags), r, int(n_spheres), ptr(spheres), int(n_capsules), ptr(capsules), float(hard), float(influence), float(gain),
                    ptr(workspace), int(workspace_bytes), *o)


def test_arguments(torch_mod):
    """What is refused (RSIK_E_INVALID, the whole text of rsik_last_error, the first fault of a call with two; nothing written),
    n_pairs = 0, a workspace of exactly the helper's size with guard bytes behind it, every output left out in turn, two launches, a
    robot alone and inside a launch of 19 at another place."""
    torch = torch_mod
    _abi = abi()
    shape = PP.MAIN_SHAPES[0] + (True,)
    t, k, seed, robots, _ = shape
    n = 2 * robots
    solver, dual, p3, th, _, _, _, scene = shape_case(*shape)
    p = p3.reshape(6, t * n)
    f64, u8, i32, i16 = torch.float64, torch.uint8, torch.int32, torch.int16
    big = T(np.linspace(0.0, 1.0, 17), torch)
    start = T(path_start(seed, n), torch)
    sc = scene_kw(torch, scene)
    S, Cp = sc["spheres"], sc["capsules"]
    need = solver.solve_path_pair_workspace_bytes(robots, t, k)
    G = 64
    ws = torch.full((need + G,), 0x5A, dtype=u8, device="cuda")
    FR = _abi.THETA_FRACTION
    inf, nan = float("inf"), float("nan")

    def fresh():
        def full(shp, dtype):
            return torch.full(shp, 777.0 if dtype == f64 else 77, dtype=dtype, device="cuda")

        return dict(index=full((t, n), i32), theta=full((t, n), f64), joints=full((t, n, 7), f64), elbow=full((t, n, 3), f64),
                    projected=full((t, n), u8), step_cost=full((t, n), f64), cost=full((robots,), f64), n_solved=full((robots,), i32),
                    interval=full((t, n, 2), f64), reachable=full((t, n), u8), state=full((t, n), u8), clearance=full((t, n), f64),
                    nearest=full((t, n, 2), i32), blocked=full((t, robots), i16))

    def untouched(outs):
        torch.cuda.synchronize()
        for key, v in outs.items():
            assert bool((v == (777.0 if v.dtype == f64 else 77)).all()), key
        assert bool((ws == 0x5A).all()), "the workspace"

    outs = fresh()
    no_main = {key: v for key, v in outs.items() if key not in ("index", "theta", "joints")}

    def call(n_=robots, t_=t, p_=p, k_=k, policy=FR, th_=th, o=outs, **kw):
        kw.setdefault("spheres", S)
        kw.setdefault("capsules", Cp)
        kw.setdefault("workspace", ws)
        return raw_pair(solver, n_, t_, p_, k_, policy, th_, 0, start, **kw, **o)

    calls = {
        "n_pairs -1": (lambda: call(n_=-1), "n_pairs < 0"),
        "n_steps 0": (lambda: call(t_=0), "n_steps must be in [1, 65536]"),
        "n_steps 65537": (lambda: call(t_=65537), "n_steps must be in [1, 65536]"),
        "n_theta 0": (lambda: call(k_=0), "n_theta must be in [1, 16]"),
        "n_theta 17": (lambda: call(k_=17, th_=big), "n_theta must be in [1, 16]"),
        "interval0": (lambda: call(policy=_abi.THETA_INTERVAL0), "theta_policy must be RSIK_THETA_EXPLICIT or RSIK_THETA_FRACTION"),
        "flags 4": (lambda: call(flags=4), "unknown bits in flags"),
        "a negative weight": (lambda: call(weights=(1, 1, 1, -0.5, 1, 1, 1)), "every weight must be finite and >= 0"),
        "a NaN weight": (lambda: call(weights=(1, 1, 1, 1, 1, 1, nan)), "every weight must be finite and >= 0"),
        "n_spheres -1": (lambda: call(n_spheres=-1), "n_spheres must be 0 ... 256"),
        "n_spheres 257": (lambda: call(n_spheres=257), "n_spheres must be 0 ... 256"),
        "n_capsules 65": (lambda: call(n_capsules=65), "n_capsules must be 0 ... 64"),
        "a negative link radius": (lambda: call(radius=(0.03, -0.01, 0.04)), "every link radius must be finite and >= 0"),
        "an infinite influence": (lambda: call(influence=inf), "influence and clearance_gain must be finite and >= 0"),
        "a NaN gain": (lambda: call(gain=nan), "influence and clearance_gain must be finite and >= 0"),
        "min_clearance NaN": (lambda: call(hard=nan), "min_clearance must be finite or -infinity"),
        "min_clearance +inf": (lambda: call(hard=inf), "min_clearance must be finite or -infinity"),
        "pose_soa NULL": (lambda: call(p_=None), "pose_soa is NULL"),
        "theta_in NULL": (lambda: call(th_=None), "theta_in is NULL"),
        "index, theta and joints NULL": (lambda: call(o=no_main), "index, theta and joints are all NULL"),
        "workspace NULL": (lambda: call(workspace=None, workspace_bytes=need), "workspace is NULL or smaller than rsik_solve_path_pair_workspace_bytes"),
        "workspace one byte short": (lambda: call(workspace_bytes=need - 1), "workspace is NULL or smaller than rsik_solve_path_pair_workspace_bytes"),
        "spheres NULL": (lambda: call(spheres=None, n_spheres=3), "spheres or capsules is NULL with a count above 0"),
        "capsules NULL": (lambda: call(capsules=None, n_capsules=1), "spheres or capsules is NULL with a count above 0"),
        "nearest misaligned": (lambda: call(nearest_offset=4), "nearest must be aligned to 8 bytes"),
        # two faults in one call: the one the entry point tests first is the one it reports
        "n_theta 17 and min_clearance NaN": (lambda: call(k_=17, th_=big, hard=nan), "n_theta must be in [1, 16]"),
        "min_clearance NaN and pose_soa NULL": (lambda: call(p_=None, hard=nan), "min_clearance must be finite or -infinity"),
        "workspace NULL and nearest misaligned": (lambda: call(workspace=None, workspace_bytes=need, nearest_offset=4),
                                                  "workspace is NULL or smaller than rsik_solve_path_pair_workspace_bytes"),
    }
    for name, (fn, text) in calls.items():
        rc = fn()
        assert rc == _abi.RSIK_E_INVALID, (name, rc)
        assert last_error(solver) == "rsik_solve_path_pair: " + text, (name, last_error(solver))
    untouched(outs)
    # n_pairs = 0 launches nothing; no obstacle at all is allowed
    assert raw_pair(solver, 0, t, None, k, FR, th, 0, None) == _abi.RSIK_OK
    empty = solver.solve_path_pair(torch.zeros((6, t, 0), dtype=f64, device="cuda"), th)
    assert empty["index"].shape == (t, 0) and empty["blocked"].shape == (t, 0) and empty["cost"].shape == (0,)
    untouched(outs)
    # a workspace of exactly the helper's size: the guard bytes behind it stay
    assert call(workspace_bytes=need) == _abi.RSIK_OK, last_error(solver)
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0x5A).all()), "a store ran past the end of the workspace"
    full = {key: v.cpu().numpy() for key, v in outs.items()}
    assert (full["index"] >= 0).sum() > 100 and (full["blocked"] > 0).sum() > 10
    same_outputs(full, to_np(solver.solve_path_pair(p3, th, start, **sc, **FULL)), "the caller's buffers against solve_path_pair")
    # every output left out in turn: the same bits in the rest
    for left_out in list(EVERY) + [("index", "theta"), ("index", "joints"), ("theta", "joints", "elbow"), ("clearance", "nearest"), ("clearance", "nearest", "blocked")]:
        left_out = (left_out,) if isinstance(left_out, str) else left_out
        for flags in (0, _abi.PATH_UNWIND):
            part = {key: v for key, v in fresh().items() if key not in left_out}
            assert call(o=part, flags=flags) == _abi.RSIK_OK, (left_out, last_error(solver))
            torch.cuda.synchronize()
            keys = tuple(key for key in part if not (flags and key == "joints"))
            same_outputs({key: v.cpu().numpy() for key, v in part.items()}, full, f"without {left_out}, flags {flags}", keys=keys)
    # two launches: the same bits
    again = fresh()
    assert call(o=again) == _abi.RSIK_OK
    torch.cuda.synchronize()
    same_outputs({key: v.cpu().numpy() for key, v in again.items()}, full, "a second launch")
    # a robot's bits are the same alone and inside the launch of 19, at another place
    for i in (5, 18):
        one = to_np(solver.solve_path_pair(p3[:, :, 2 * i:2 * i + 2].contiguous(), th, start[2 * i:2 * i + 2], **sc, **FULL))
        same_outputs(one, {key: (v[:, 2 * i:2 * i + 2] if key in PER_ROW else v[i:i + 1] if key in PER_ROBOT else v[:, i:i + 1]) for key, v in full.items()},
                     f"robot {i} alone")
    order = np.roll(np.arange(robots), 7)
    rows = np.stack([2 * order, 2 * order + 1], axis=1).reshape(-1)
    moved = to_np(solver.solve_path_pair(p3[:, :, T(rows, torch)].contiguous(), th, start[T(rows, torch)], **sc, **FULL))
    same_outputs(moved, {key: (v[:, rows] if key in PER_ROW else v[order] if key in PER_ROBOT else v[:, order]) for key, v in full.items()},
                 "the robots in another order")
    # the Python layers: DualArmIK.path_pair_batch returns the launch's tensors as views per arm
    pos, eul, _ = PP.pair_poses(seed, robots, t)
    res = dual.path_pair_batch(np.stack([pos[:, 0::2], eul[:, 0::2]], axis=2), np.stack([pos[:, 1::2], eul[:, 1::2]], axis=2),
                               start[0::2], start[1::2], thetas=th, **sc, **FULL)
    for key in PER_ROW:
        np.testing.assert_array_equal(as_bits(res[key]["r"].cpu().numpy()), as_bits(full[key][:, 0::2]), err_msg=key)
        np.testing.assert_array_equal(as_bits(res[key]["l"].cpu().numpy()), as_bits(full[key][:, 1::2]), err_msg=key)
    for key in PER_ROBOT + ("blocked",):
        np.testing.assert_array_equal(as_bits(res[key].cpu().numpy()), as_bits(full[key]), err_msg=key)
    with pytest.raises(ValueError):
        solver.solve_path_pair(p3[:, :, :3].contiguous(), th)
