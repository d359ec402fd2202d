"""GPU tests (-m gpu, MI355X) of rsik_solve_path_clear (csrc/rsik_kernel_path.hpp, solve_path_kernel over PathClearArgs): rsik_solve_path
where a sample nearer than min_clearance to a static scene is no candidate and one nearer than `influence` pays a penalty.

The entry point is defined against rsik_solve_sweep and rsik_clearance: the expected value is tests/path_clear_workload.path_clear_dp
on the library's own sweep over the same T * n poses and the library's own rsik_clearance over that sweep's joints ([K][T n][7] is
n_rep = K in place), so the mask and the penalty are exact.  A launch is accepted, as in tests/test_gpu_solve_path.py, when
  (a) theta / joints / elbow / projected at (t, i) have the BITS of the sweep's sample index[t][i]; the skipped waypoints and `blocked`
      are NumPy's exactly; clearance and nearest are rsik_clearance's bits on the returned joints; n_solved / interval / reachable /
      state are as in rsik_solve_path,
  (b) the cost of the device's path, recomputed by NumPy along `index` (penalties included), is within 2 T COST_TOL of NumPy's
      optimum, and `cost` within the same bound of it: per waypoint one transition within COST_TOL and one exactly known penalty added
      to a running sum below 128 (asserted), whose rounding is 1.4e-14 < COST_TOL,
  (c) on every path whose second-best distinct path is more than GAP above the optimum, index is NumPy's exactly.
The scene is clearance_workload.scene("default/default", "open") with LINK_RADIUS; the cases are min_clearance in {0, -inf} crossed with
(influence, gain) in {(0, 0), (0.05, 100)}, with and without start joints; the shapes are path_workload's."""
import ctypes as C
import functools

import numpy as np
import pytest

import path_clear_workload as PC
from clearance_workload import LINK_RADIUS
from compare import as_bits, bits
from gpu_support import T, abi, cols, last_error, make_symbolic, orc, ptr, raw_call, to_np, torch_mod  # noqa: F401
from nearest_workload import skip_projected_case
from path_workload import GAP, MAIN_SHAPES, N_MAIN, SMALL_SHAPES, path_dp, path_fractions, path_poses, path_start, gap_condition
from sampling_support import ALL, PER_WAYPOINT, lib_sweep, path_arm_kwargs, path_soa, same_path_outputs

pytestmark = pytest.mark.gpu

NEW = ("clearance", "nearest", "blocked")
EVERY = ALL + NEW


def scene_tensors(torch, scene=None):
    sc = PC.the_scene() if scene is None else scene
    return dict(spheres=T(sc["spheres"], torch) if len(sc["spheres"]) else None,
                capsules=T(sc["capsules"], torch) if len(sc["capsules"]) else None, link_radius=LINK_RADIUS)


def lib_clearance(solver, joints, arm_rows, torch, scene=None):
    """rsik_clearance of joints [R, rows, 7] (arm_rows [rows]: the arm byte of a row, shared by the repetitions): clearance [R, rows]
    and nearest [R, rows, 2]."""
    got = to_np(solver.clearance(T(np.array(joints), torch), want=("clearance", "nearest"), **scene_tensors(torch, scene), **path_arm_kwargs(arm_rows, torch)))
    return got["clearance"], got["nearest"]


@functools.lru_cache(maxsize=None)
def shape_case(t, k, seed, kind, n):
    """A shape's inputs, the library's sweep over them and the library's clearance of that sweep's joints: computed once, shared."""
    import torch

    solver, _, _ = make_symbolic(0.03)
    pos, eul, arm = path_poses(seed, n, t, kind)
    p, th = path_soa(pos, eul, torch), T(path_fractions(k), torch)
    sw = lib_sweep(solver, p, th, "fraction", arm, torch)
    d, _ = lib_clearance(solver, sw["joints"], np.tile(arm, t), torch)
    for v in list(sw.values()) + [d]:
        v.setflags(write=False)
    return solver, p, th, arm, sw, d


def same_outputs(a, b, what, keys=EVERY, paths=None):
    same_path_outputs(a, b, what, keys=tuple(key for key in keys if key in ALL), paths=paths)
    for key in keys:
        if key in NEW:
            x, y = (a[key], b[key]) if paths is None else (a[key][:, paths], b[key][:, paths])
            np.testing.assert_array_equal(as_bits(x), as_bits(y), err_msg=f"{what}: {key}")


def check_path_clear(got, sw, d, clr_of_joints, t, n, what, hard, influence, gain, start=None, weights=None, skip=False, need_gap=False):
    """(a) - (c) for one launch `got` against the library's sweep `sw`, its clearance table d [K, t n] and rsik_clearance of the
    returned joints clr_of_joints = (clearance [t,n], nearest [t,n,2])."""
    exp = PC.path_clear_dp(sw, d, t, n, hard, influence, gain, start, weights, skip)
    if need_gap:
        gap_condition(exp, what, seeded=start is not None)  # the condition on the inputs, before anything is compared
    idx = got["index"]
    k = sw["joints"].shape[0]
    assert idx.dtype == np.int32 and idx.shape == (t, n) and got["n_solved"].dtype == np.int32, (what, idx.dtype, idx.shape)
    # (a)
    np.testing.assert_array_equal(idx == -1, ~exp["solved"], err_msg=what + ": the skipped waypoints")
    np.testing.assert_array_equal(got["n_solved"], exp["n_solved"], err_msg=what)
    assert got["blocked"].dtype == np.uint8 and got["blocked"].shape == (t, n), (what, got["blocked"].dtype)
    np.testing.assert_array_equal(got["blocked"], exp["blocked"], err_msg=what + ": blocked")
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
    np.testing.assert_array_equal(bits(got["clearance"]), bits(clr_of_joints[0]), err_msg=what + ": clearance is not rsik_clearance's of the joints")
    np.testing.assert_array_equal(got["nearest"], clr_of_joints[1], err_msg=what + ": nearest is not rsik_clearance's of the joints")
    np.testing.assert_array_equal(bits(got["clearance"][tt, ii]), bits(d[idx[tt, ii], pose]), err_msg=what + ": clearance is not d of the sample")
    assert np.isnan(got["clearance"][idx < 0]).all() and (got["nearest"][idx < 0] == -1).all(), (what, "a skipped waypoint's clearance")
    with np.errstate(invalid="ignore"):
        assert (got["clearance"][tt, ii] >= hard).all(), (what, "a winner below min_clearance")
    # (b)
    tol = PC.path_clear_tol(t)
    has = exp["n_solved"] > 0
    along, step2 = PC.clear_cost_along(sw, exp["penalty"], idx, t, n, start, weights)
    assert (along[has] < PC.COST_SUM_MAX).all() and (exp["cost"][has] < PC.COST_SUM_MAX).all(), (what, "the running sum")
    excess = along[has] - exp["cost"][has]
    err_cost = np.abs(got["cost"][has] - along[has])
    err_steps = np.abs(got["step_cost"] ** 2 - step2)[idx >= 0]
    print(f"{what}: {int(has.sum())} paths, device path - optimum in [{float(excess.min(initial=0.0)):.3e}, {float(excess.max(initial=0.0)):.3e}], "
          f"|cost - recomputed| {float(err_cost.max(initial=0.0)):.3e}, |step_cost^2 - recomputed| {float(err_steps.max(initial=0.0)):.3e}, tol {tol:.1e}")
    assert (np.abs(excess) <= tol).all(), (what, float(np.abs(excess).max(initial=0.0)))
    assert (err_cost <= tol).all() and np.isnan(got["cost"][~has]).all(), (what, float(err_cost.max(initial=0.0)))
    assert (np.abs(got["cost"][has] - exp["cost"][has]) <= tol).all(), what
    assert (err_steps <= tol).all(), (what, float(err_steps.max(initial=0.0)))
    # (c)  (without start joints and without a penalty a path with one solved waypoint is an exact tie at 0: the lowest sample's)
    clear = exp["gap"] > GAP
    if start is None and gain == 0.0:
        clear = clear | (exp["n_solved"] == 1)
    np.testing.assert_array_equal(idx[:, clear], exp["index"][:, clear], err_msg=what + ": index where the gap is clear")
    return exp


def run_clear(solver, p, th, start, torch, arm, scene=None, **kw):
    got = to_np(solver.solve_path_clear(p, th, None if start is None else T(start, torch), **scene_tensors(torch, scene), **kw,
                                        **path_arm_kwargs(arm, torch)))
    t = int(p.shape[1])
    plain = got["joints"]
    if kw.get("unwind"):
        plain = to_np(solver.solve_path_clear(p, th, None if start is None else T(start, torch), **scene_tensors(torch, scene),
                                              **{**kw, "unwind": False}, **path_arm_kwargs(arm, torch)))["joints"]
    return got, lib_clearance(solver, plain, arm, torch, scene) if t else None


# ------------------------------------------------------------------------------------------ 1. the three acceptance points
@pytest.mark.parametrize("shape", [s + (N_MAIN,) for s in MAIN_SHAPES] + list(SMALL_SHAPES))
def test_the_path_keeps_its_clearance_and_is_the_optimum(torch_mod, shape):
    torch = torch_mod
    t, k, seed, kind, n = shape
    solver, p, th, arm, sw, d = shape_case(*shape)
    on_table = n == N_MAIN and (t, k, seed) in PC.TABLE_SHAPES
    for start in (None, path_start(seed, n)):
        free = path_dp(sw, t, n, start)
        for hard in PC.HARD:
            exps = []
            for influence, gain in PC.SOFT:
                what = f"T {t} K {k} seed {seed} {kind} n {n} start {start is not None} min_clearance {hard} ({influence}, {gain})"
                got, clr = run_clear(solver, p, th, start, torch, arm, min_clearance=hard, influence=influence, clearance_gain=gain)
                need_gap = n == N_MAIN and gain > 0.0 and k > 1
                exps.append(check_path_clear(got, sw, d, clr, t, n, what, hard, influence, gain, start, need_gap=need_gap))
            if on_table:  # the conditions on the inputs
                PC.soft_condition(exps[0], exps[1], what)
                if hard == 0.0:
                    PC.input_conditions(exps[0], free, what)


# ------------------------------------------------------------------------------------------ 2. identity with rsik_solve_path
@pytest.mark.parametrize("shape", [s + (N_MAIN,) for s in MAIN_SHAPES[:3]])
def test_without_a_constraint_it_is_rsik_solve_path(torch_mod, shape):
    """min_clearance = -inf with gain 0, and the scene 10 m away with min_clearance = 0 and (0.05, 100): every output shared with
    rsik_solve_path has its bits, blocked is 0."""
    torch = torch_mod
    t, k, seed, kind, n = shape
    solver, p, th, arm, sw, d = shape_case(*shape)
    sc = PC.the_scene()
    far = dict(spheres=sc["spheres"] + [10.0, 0.0, 0.0, 0.0], capsules=sc["capsules"] + [10.0, 0.0, 0.0, 10.0, 0.0, 0.0, 0.0])
    for start in (None, path_start(seed, n)):
        st = None if start is None else T(start, torch)
        ref = to_np(solver.solve_path(p, th, st, **path_arm_kwargs(arm, torch)))
        assert (ref["index"] >= 0).sum() >= 20
        a, _ = run_clear(solver, p, th, start, torch, arm, min_clearance=-np.inf, influence=0.05, clearance_gain=0.0)
        b, _ = run_clear(solver, p, th, start, torch, arm, scene=far, min_clearance=0.0, influence=0.05, clearance_gain=100.0)
        for got, what in ((a, "no constraint"), (b, "the scene 10 m away")):
            same_path_outputs(got, ref, f"{what}, start {start is not None}")
            assert (got["blocked"] == 0).all(), what
            assert np.isfinite(got["clearance"][got["index"] >= 0]).all()
        assert (b["clearance"][b["index"] >= 0] > 5.0).all()


# ------------------------------------------------------------------------------------------ 3. the largest scene and its staging
def test_the_largest_scene(torch_mod):
    """232 far spheres and 56 far capsules in front of the open scene's: 256 + 64 obstacles, everything a workgroup can stage.  index,
    cost, clearance, blocked and every other output have the unpadded run's bits; nearest's obstacle index is shifted by the padding."""
    torch = torch_mod
    shape = MAIN_SHAPES[0] + (N_MAIN,)
    t, k, seed, kind, n = shape
    solver, p, th, arm, sw, d = shape_case(*shape)
    sc = PC.the_scene()
    rng = np.random.default_rng(77)
    pad_s = np.concatenate([rng.uniform(-1, 1, size=(232, 3)) + [20.0, 0.0, 0.0], rng.uniform(0.01, 0.1, size=(232, 1))], axis=1)
    a = rng.uniform(-1, 1, size=(56, 3)) + [0.0, 20.0, 0.0]
    pad_c = np.concatenate([a, a + rng.uniform(-0.3, 0.3, size=(56, 3)), rng.uniform(0.01, 0.1, size=(56, 1))], axis=1)
    big = dict(spheres=np.concatenate([pad_s, sc["spheres"]]), capsules=np.concatenate([pad_c, sc["capsules"]]))
    assert len(big["spheres"]) == 256 and len(big["capsules"]) == 64
    start = path_start(seed, n)
    kw = dict(min_clearance=0.0, influence=0.05, clearance_gain=100.0)
    small, _ = run_clear(solver, p, th, start, torch, arm, **kw)
    got, clr = run_clear(solver, p, th, start, torch, arm, scene=big, **kw)
    same_outputs(got, small, "256 + 64 obstacles", keys=tuple(key for key in EVERY if key != "nearest"))
    won = small["index"] >= 0
    assert won.sum() >= 100 and (small["blocked"] > 0).sum() >= 20
    n_s = len(sc["spheres"])
    link, obs = small["nearest"][..., 0], small["nearest"][..., 1]
    shifted = np.where(obs < 0, -1, np.where(obs < n_s, obs + 232, obs + 288))
    assert (obs[won] < n_s).any() and (obs[won] >= n_s).any(), "winners against spheres and against capsules"
    np.testing.assert_array_equal(got["nearest"][..., 0], link)
    np.testing.assert_array_equal(got["nearest"][..., 1], shifted)
    np.testing.assert_array_equal(got["nearest"], clr[1], err_msg="rsik_clearance on the same scene")


# ------------------------------------------------------------------------------------------ 4. every row skipped
def test_a_scene_in_which_every_row_is_skipped(torch_mod):
    torch = torch_mod
    shape = MAIN_SHAPES[1] + (N_MAIN,)
    t, k, seed, kind, n = shape
    solver, p, th, arm, sw, d = shape_case(*shape)
    none = dict(spheres=np.array([[np.nan, 0.0, 0.0, 0.1], [0.3, -0.2, 0.0, -0.05], [np.inf, 0.0, 0.0, 0.1]]),
                capsules=np.array([[0.3, np.nan, 0.0, 0.3, 0.0, 0.2, 0.05]]))
    start = path_start(seed, n)
    ref = to_np(solver.solve_path(p, th, T(start, torch), **path_arm_kwargs(arm, torch)))
    got, clr = run_clear(solver, p, th, start, torch, arm, scene=none, min_clearance=0.0, influence=0.05, clearance_gain=100.0)
    same_path_outputs(got, ref, "every obstacle skipped")
    won = got["index"] >= 0
    assert won.sum() >= 100 and (~won).sum() >= 1
    assert (got["clearance"][won] == np.inf).all() and np.isnan(got["clearance"][~won]).all()
    assert (got["nearest"] == -1).all() and (got["blocked"] == 0).all()
    np.testing.assert_array_equal(bits(got["clearance"]), bits(clr[0]))


# ------------------------------------------------------------------------------------------ 5. the two flags with the constraint
def test_unwind_changes_joints_only(torch_mod):
    torch = torch_mod
    shape = MAIN_SHAPES[0] + (N_MAIN,)
    t, k, seed, kind, n = shape
    solver, p, _, arm, _, _ = shape_case(*shape)
    th = T(np.random.default_rng(seed + 300).uniform(-2 * np.pi, 2 * np.pi, size=(k, t, n)), torch)
    start = path_start(seed, n) + 4.0
    kw = dict(policy="explicit", min_clearance=0.0, influence=0.05, clearance_gain=100.0)
    plain, _ = run_clear(solver, p, th, start, torch, arm, **kw)
    got, clr = run_clear(solver, p, th, start, torch, arm, unwind=True, **kw)
    same_outputs(got, plain, "everything but joints", keys=tuple(key for key in EVERY if key != "joints"))
    moved = (bits(got["joints"]) != bits(plain["joints"])).any(axis=2)
    assert moved.sum() >= 10 and (plain["blocked"] > 0).sum() >= 20
    np.testing.assert_array_equal(bits(got["clearance"]), bits(clr[0]), err_msg="clearance is the plain joints'")


def test_skip_projected_with_the_constraint(torch_mod, orc):
    """skip_projected_case's poses as 75 paths of 4 waypoints: with the flag `blocked` counts only samples the flag leaves in, and the
    expected value is path_clear_dp's with the flag set."""
    torch = torch_mod
    pos, eul, arm, thetas, ref, mixed, allp = skip_projected_case(orc)
    t, n, k = 4, 75, thetas.shape[0]
    p = path_soa(pos.reshape(t, n, 3), eul.reshape(t, n, 3), torch)
    th = T(thetas.reshape(k, t, n), torch)
    start = path_start(33, n)
    solver, _, _ = make_symbolic(0.03)
    arm = arm[:n]
    sw = lib_sweep(solver, p, th, "explicit", arm, torch)
    d, _ = lib_clearance(solver, sw["joints"], np.tile(arm, t), torch)
    kw = dict(policy="explicit", min_clearance=0.0, influence=0.05, clearance_gain=100.0)
    free, clr = run_clear(solver, p, th, start, torch, arm, **kw)
    e0 = check_path_clear(free, sw, d, clr, t, n, "no flag", 0.0, 0.05, 100.0, start)
    got, clr = run_clear(solver, p, th, start, torch, arm, skip_projected=True, **kw)
    e1 = check_path_clear(got, sw, d, clr, t, n, "flag", 0.0, 0.05, 100.0, start, skip=True)
    assert (got["projected"] == 0).all()
    assert (e1["blocked"] <= e0["blocked"]).all() and (e1["blocked"] < e0["blocked"]).sum() >= 5, "projected samples are not counted"
    assert (e1["blocked"] > 0).sum() >= 20


# ------------------------------------------------------------------------------------------ 6. rows that are not numbers
def test_rows_that_are_not_numbers_stay_where_they_are(torch_mod):
    torch = torch_mod
    _abi = abi()
    shape = MAIN_SHAPES[0] + (N_MAIN,)
    t, k, seed, kind, n = shape
    solver, p, _, arm, _, _ = shape_case(*shape)
    start = path_start(seed, n)
    grid = path_fractions(k)
    per = np.repeat(grid[:, None], t * n, axis=1).reshape(k, t, n)
    kw = dict(min_clearance=0.0, influence=0.05, clearance_gain=100.0)

    def run(poses, thetas, st, scene=None):
        return run_clear(solver, poses, T(thetas, torch), st, torch, arm, scene=scene, **kw)[0]

    clean = run(p, per, start)
    same_outputs(run(p, grid, start), clean, "one angle per waypoint and sample against the shared grid")
    busy = np.flatnonzero(clean["n_solved"] >= 6)
    assert len(busy) >= 8
    # a. poses that are not numbers
    bad = busy[:3]
    wp = [int(np.flatnonzero(clean["index"][:, i] >= 0)[1]) for i in bad]
    p2 = p.clone()
    for q, i in enumerate(bad):
        p2[(0, 4, 2)[q], wp[q], i] = (float("nan"), float("inf"), float("-inf"))[q]
    got = run(p2, per, start)
    same_outputs(got, clean, "bad poses: the other paths", paths=np.setdiff1d(np.arange(n), bad))
    for q, i in enumerate(bad):
        s = wp[q]
        assert got["state"][s, i] == _abi.STATE_INVALID_INPUT and got["reachable"][s, i] == 0 and got["index"][s, i] == -1
        assert got["blocked"][s, i] == 0 and np.isnan(got["clearance"][s, i]) and (got["nearest"][s, i] == -1).all()
        assert got["n_solved"][i] == clean["n_solved"][i] - 1
    # b. a theta that is not a number: the sample the clean path used
    i_a = int(busy[3])
    s_a = int(np.flatnonzero(clean["index"][:, i_a] >= 0)[1])
    th2 = per.copy()
    th2[clean["index"][s_a, i_a], s_a, i_a] = np.nan
    got = run(p, th2, start)
    same_outputs(got, clean, "a NaN theta: the other paths", paths=np.setdiff1d(np.arange(n), [i_a]))
    assert got["index"][s_a, i_a] != clean["index"][s_a, i_a]
    sw2 = lib_sweep(solver, p, T(th2, torch), "fraction", arm, torch)
    d2, _ = lib_clearance(solver, sw2["joints"], np.tile(arm, t), torch)
    check_path_clear(got, sw2, d2, lib_clearance(solver, got["joints"], arm, torch), t, n, "a NaN theta", 0.0, 0.05, 100.0, start)
    # c. start rows that are not numbers
    bad = busy[5:8]
    st2 = start.copy()
    for q, i in enumerate(bad):
        st2[i, (0, 3, 6)[q]] = (np.nan, np.inf, np.nan)[q]
    got = run(p, per, st2)
    same_outputs(got, clean, "bad start rows: the other paths", paths=np.setdiff1d(np.arange(n), bad))
    same_path_outputs(got, clean, "bad start rows: is_reachable's outputs", keys=("interval", "reachable", "state"))
    assert (got["n_solved"][bad] == 0).all() and (got["index"][:, bad] == -1).all() and np.isnan(got["cost"][bad]).all()
    assert (got["blocked"][:, bad] == 0).all() and np.isnan(got["clearance"][:, bad]).all() and (got["nearest"][:, bad] == -1).all()
    assert (clean["blocked"][:, bad] > 0).any()
    # d. a sphere row that is not a number, behind the other spheres: nothing changes but the number of every capsule, one higher
    sc = PC.the_scene()
    more = dict(spheres=np.concatenate([sc["spheres"], [[0.3, np.nan, 0.0, 0.05]]]), capsules=sc["capsules"])
    got = run(p, per, start, scene=more)
    same_outputs(got, clean, "a NaN sphere row", keys=tuple(key for key in EVERY if key != "nearest"))
    obs = clean["nearest"][..., 1]
    assert (obs >= len(sc["spheres"])).sum() >= 10, "winners against capsules"
    np.testing.assert_array_equal(got["nearest"][..., 0], clean["nearest"][..., 0])
    np.testing.assert_array_equal(got["nearest"][..., 1], np.where(obs >= len(sc["spheres"]), obs + 1, obs))


# ------------------------------------------------------------------------------------------ 7. arguments
def raw_clear(solver, n, t, p, k, policy, thetas, per_pose, start=None, weights=None, flags=0, arm=None, arm_uniform=0, radius=LINK_RADIUS,
              n_spheres=None, spheres=None, n_capsules=None, capsules=None, hard=0.0, influence=0.05, gain=100.0, workspace=None,
              workspace_bytes=None, nearest_offset=0, **outs):
    """rsik_solve_path_clear on the caller's own buffers: returns the ABI's code."""
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
    return raw_call(solver, "rsik_solve_path_clear", n, t, cols(p, 6), ptr(arm), int(arm_uniform), int(k), int(policy), ptr(thetas),
                    int(per_pose), ptr(start), w, int(flags), r, int(n_spheres), ptr(spheres), int(n_capsules), ptr(capsules),
                    float(hard), float(influence), float(gain), ptr(workspace), int(workspace_bytes), *o)


def test_arguments(torch_mod):
    """What is refused (RSIK_E_INVALID, the whole text of rsik_last_error, the first fault of a call with two; nothing written), n = 0,
    a workspace of exactly the helper's size with guard bytes behind it, every output left out in turn, a misaligned `nearest`."""
    torch = torch_mod
    _abi = abi()
    t, k, n = 12, 8, N_MAIN
    pos, eul, arm = path_poses(11, n, t, "r")
    p = path_soa(pos, eul, torch).reshape(6, t * n)
    solver, _, _ = make_symbolic(0.03)
    f64, u8, i32 = torch.float64, torch.uint8, torch.int32
    th = T(path_fractions(k), torch)
    big = T(np.linspace(0.0, 1.0, 65), torch)
    start = T(path_start(11, n), torch)
    sc = scene_tensors(torch)
    S, Cp = sc["spheres"], sc["capsules"]
    need = solver.solve_path_workspace_bytes(n, t, k)
    G = 64
    ws = torch.full((need + G,), 0x5A, dtype=u8, device="cuda")
    FR = _abi.THETA_FRACTION
    inf, nan = float("inf"), float("nan")

    def fresh():
        def full(shape, dtype):
            return torch.full(shape, 777.0 if dtype == f64 else 77, dtype=dtype, device="cuda")

        return dict(index=full((t, n), i32), theta=full((t, n), f64), joints=full((t, n, 7), f64), elbow=full((t, n, 3), f64),
                    projected=full((t, n), u8), step_cost=full((t, n), f64), cost=full((n,), f64), n_solved=full((n,), i32),
                    interval=full((t, n, 2), f64), reachable=full((t, n), u8), state=full((t, n), u8), clearance=full((t, n), f64),
                    nearest=full((t, n, 2), i32), blocked=full((t, n), u8))

    def untouched(outs):
        torch.cuda.synchronize()
        for key, v in outs.items():
            assert bool((v == (777.0 if v.dtype == f64 else 77)).all()), key
        assert bool((ws == 0x5A).all()), "the workspace"

    outs = fresh()
    no_main = {key: v for key, v in outs.items() if key not in ("index", "theta", "joints")}

    def call(n_=n, t_=t, p_=p, k_=k, policy=FR, th_=th, o=outs, **kw):
        kw.setdefault("spheres", S)
        kw.setdefault("capsules", Cp)
        kw.setdefault("workspace", ws)
        return raw_clear(solver, n_, t_, p_, k_, policy, th_, 0, start, **kw, **o)

    calls = {
        # everything rsik_solve_path refuses
        "n_theta 0": (lambda: call(k_=0), "n_theta must be in [1, 64]"),
        "n_theta 65": (lambda: call(k_=65, th_=big), "n_theta must be in [1, 64]"),
        "interval0": (lambda: call(policy=_abi.THETA_INTERVAL0), "theta_policy must be RSIK_THETA_EXPLICIT or RSIK_THETA_FRACTION"),
        "a negative weight": (lambda: call(weights=(1, 1, 1, -0.5, 1, 1, 1)), "every weight must be finite and >= 0"),
        "a NaN weight": (lambda: call(weights=(1, 1, 1, 1, 1, 1, nan)), "every weight must be finite and >= 0"),
        "flags 4": (lambda: call(flags=4), "unknown bits in flags"),
        "flags -1": (lambda: call(flags=-1), "unknown bits in flags"),
        "arm_uniform 2": (lambda: call(arm_uniform=2), "arm_uniform must be 0 (r) or 1 (l)"),
        "workspace NULL": (lambda: call(workspace=None, workspace_bytes=need), "workspace is NULL or smaller than rsik_solve_path_workspace_bytes"),
        "workspace one byte short": (lambda: call(workspace_bytes=need - 1), "workspace is NULL or smaller than rsik_solve_path_workspace_bytes"),
        "index, theta and joints NULL": (lambda: call(o=no_main), "index, theta and joints are all NULL"),
        "n_steps 0": (lambda: call(t_=0), "n_steps must be in [1, 65536]"),
        "n_steps 65537": (lambda: call(t_=65537), "n_steps must be in [1, 65536]"),
        "theta_in NULL": (lambda: call(th_=None), "theta_in is NULL"),
        "pose_soa NULL": (lambda: call(p_=None), "pose_soa is NULL"),
        "n -1": (lambda: call(n_=-1), "n < 0"),
        # its own
        "n_spheres -1": (lambda: call(n_spheres=-1), "n_spheres must be 0 ... 256"),
        "n_spheres 257": (lambda: call(n_spheres=257), "n_spheres must be 0 ... 256"),
        "n_capsules -1": (lambda: call(n_capsules=-1), "n_capsules must be 0 ... 64"),
        "n_capsules 65": (lambda: call(n_capsules=65), "n_capsules must be 0 ... 64"),
        "no obstacle": (lambda: call(n_spheres=0, n_capsules=0), "at least one obstacle (without obstacles: rsik_solve_path)"),
        "spheres NULL": (lambda: call(spheres=None, n_spheres=3), "spheres or capsules is NULL with a count above 0"),
        "capsules NULL": (lambda: call(capsules=None, n_capsules=1), "spheres or capsules is NULL with a count above 0"),
        "a negative link radius": (lambda: call(radius=(0.03, -0.01, 0.04)), "every link radius must be finite and >= 0"),
        "a NaN link radius": (lambda: call(radius=(nan, 0.05, 0.04)), "every link radius must be finite and >= 0"),
        "an infinite link radius": (lambda: call(radius=(0.03, 0.05, inf)), "every link radius must be finite and >= 0"),
        "a negative influence": (lambda: call(influence=-0.01), "influence and clearance_gain must be finite and >= 0"),
        "an infinite influence": (lambda: call(influence=inf), "influence and clearance_gain must be finite and >= 0"),
        "a negative gain": (lambda: call(gain=-1.0), "influence and clearance_gain must be finite and >= 0"),
        "a NaN gain": (lambda: call(gain=nan), "influence and clearance_gain must be finite and >= 0"),
        "min_clearance NaN": (lambda: call(hard=nan), "min_clearance must be finite or -infinity"),
        "min_clearance +inf": (lambda: call(hard=inf), "min_clearance must be finite or -infinity"),
        "nearest misaligned": (lambda: call(nearest_offset=4), "nearest must be aligned to 8 bytes"),
        # two faults in one call: the one the entry point tests first is the one it reports
        "n_theta 0 and no obstacle": (lambda: call(k_=0, n_spheres=0, n_capsules=0), "n_theta must be in [1, 64]"),
        "no obstacle and min_clearance NaN": (lambda: call(n_spheres=0, n_capsules=0, hard=nan), "at least one obstacle (without obstacles: rsik_solve_path)"),
        "min_clearance NaN and pose_soa NULL": (lambda: call(p_=None, hard=nan), "min_clearance must be finite or -infinity"),
        "workspace NULL and nearest misaligned": (lambda: call(workspace=None, workspace_bytes=need, nearest_offset=4), "workspace is NULL or smaller than rsik_solve_path_workspace_bytes"),
    }
    for name, (fn, text) in calls.items():
        rc = fn()
        assert rc == _abi.RSIK_E_INVALID, (name, rc)
        assert last_error(solver) == "rsik_solve_path_clear: " + text, (name, last_error(solver))
    untouched(outs)
    # n = 0 launches nothing
    assert raw_clear(solver, 0, t, None, k, FR, th, 0, None, spheres=S, capsules=Cp) == _abi.RSIK_OK
    empty = solver.solve_path_clear(torch.zeros((6, t, 0), dtype=f64, device="cuda"), th, **sc)
    assert empty["index"].shape == (t, 0) and empty["nearest"].shape == (t, 0, 2) and empty["blocked"].shape == (t, 0)
    untouched(outs)
    # a workspace of exactly the helper's size: the guard bytes behind it stay
    assert call(workspace_bytes=need) == _abi.RSIK_OK, last_error(solver)
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0x5A).all()), "a store ran past the end of the workspace"
    full = {key: v.cpu().numpy() for key, v in outs.items()}
    assert (full["index"] >= 0).sum() > 100 and (full["blocked"] > 0).sum() > 50
    same_outputs(full, to_np(solver.solve_path_clear(p.reshape(6, t, n), th, start, min_clearance=0.0, influence=0.05, clearance_gain=100.0, **sc)),
                 "the caller's buffers against solve_path_clear")
    # every output left out in turn: the same bits in the rest
    for left_out in list(EVERY) + [("index", "theta"), ("index", "joints"), ("theta", "joints", "elbow"), ("clearance", "nearest"), NEW]:
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
    # a path's bits depend neither on n nor on the other paths
    one = to_np(solver.solve_path_clear(p.reshape(6, t, n)[:, :, 5:6].contiguous(), th, start[5:6], min_clearance=0.0, influence=0.05,
                                        clearance_gain=100.0, **sc))
    same_outputs(one, {key: (v[:, 5:6] if key in PER_WAYPOINT + NEW else v[5:6]) for key, v in full.items()}, "path 5 alone")


# ------------------------------------------------------------------------------------------ 8. the Python layers
def test_python_layers(torch_mod):
    """SymbolicIK.path_clear_batch and DualArmIK.path_clear_batch return the documented shapes and dtypes and the bits of
    HipSolver.solve_path_clear; a plan_only launch launches nothing and, re-issued twice, reproduces the result; the ValueErrors."""
    torch = torch_mod
    from reachy2_symbolic_ik_amd import DualArmIK

    t, k, n = 12, 8, N_MAIN
    pos, eul, arm = path_poses(11, n, t, "r")
    start = path_start(11, n)
    solver, r, _ = make_symbolic(0.03)
    sc = scene_tensors(torch)
    kw = dict(min_clearance=0.0, influence=0.05, clearance_gain=100.0)
    poses = np.stack([pos, eul], axis=2)  # [T,n,2,3]
    res = r.path_clear_batch(poses, start, n_theta=k, **sc, **kw)
    f64 = torch.float64
    want = dict(index=((t, n), torch.int32), theta=((t, n), f64), joints=((t, n, 7), f64), elbow=((t, n, 3), f64),
                projected=((t, n), torch.uint8), step_cost=((t, n), f64), cost=((n,), f64), n_solved=((n,), torch.int32),
                interval=((t, n, 2), f64), reachable=((t, n), torch.uint8), state=((t, n), torch.uint8), clearance=((t, n), f64),
                nearest=((t, n, 2), torch.int32), blocked=((t, n), torch.uint8))
    assert set(res) == set(want)
    for key, (shape, dtype) in want.items():
        assert tuple(res[key].shape) == shape and res[key].dtype == dtype and res[key].is_cuda, key
    res = to_np(res)
    p = path_soa(pos, eul, torch)
    grid = torch.linspace(0.0, 1.0, k, dtype=f64)
    raw = to_np(solver.solve_path_clear(p, grid, T(start, torch), **sc, **kw))
    same_outputs(res, raw, "SymbolicIK.path_clear_batch")
    assert (raw["blocked"] > 0).sum() >= 50 and (raw["index"] >= 0).sum() >= 100
    a = to_np(r.path_clear_batch(p, start, sc["spheres"].cpu().numpy(), sc["capsules"].cpu().numpy(), LINK_RADIUS, 0.0, 0.05, 100.0, n_theta=k))
    same_outputs(a, raw, "SoA poses, NumPy obstacles, positional arguments")
    # plan_only: nothing launched, the re-launch reproduces the result
    out = {key: torch.full(shape, 77, dtype=dtype, device="cuda") for key, (shape, dtype) in want.items()}
    planned = r.path_clear_batch(poses, start, n_theta=k, out=out, plan_only=True, **sc, **kw)
    torch.cuda.synchronize()
    assert all(bool((out[key] == 77).all()) for key in want), "plan_only must not launch"
    for again in ("", ", again"):
        planned["launch"]()
        torch.cuda.synchronize()
        same_outputs({key: out[key].cpu().numpy() for key in want}, raw, "planned launch" + again)
    # both arms
    pos, eul, arm = path_poses(21, n, t, "mixed")
    assert 0 < arm.sum() < n
    dual = DualArmIK(solver=solver, singularity_offset=0.03)
    dd = to_np(dual.path_clear_batch(arm, np.stack([pos, eul], axis=2), start, n_theta=k, **sc, **kw))
    raw = to_np(solver.solve_path_clear(path_soa(pos, eul, torch), grid, T(start, torch), arm=T(arm, torch), **sc, **kw))
    assert dd["joints"].shape == (t, n, 7) and dd["nearest"].dtype == np.int32
    same_outputs(dd, raw, "DualArmIK.path_clear_batch")
    # what the Python driver refuses before any launch, by its whole text
    z = torch.zeros
    refused = {
        "spheres must have shape [S, 4] with S <= 256": lambda: solver.solve_path_clear(p, grid, spheres=z((3, 5), dtype=f64)),
        "capsules must have shape [C, 7] with C <= 64": lambda: solver.solve_path_clear(p, grid, capsules=z((2, 6), dtype=f64)),
        "at least one obstacle: spheres [S, 4] or capsules [C, 7] (without obstacles: solve_path())": lambda: solver.solve_path_clear(p, grid),
        "link_radius must have 3 entries": lambda: solver.solve_path_clear(p, grid, spheres=sc["spheres"], link_radius=(0.1, 0.1)),
    }
    for text, fn in refused.items():
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == text
