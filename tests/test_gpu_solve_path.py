"""GPU tests (-m gpu, MI355X) of rsik_solve_path (csrc/rsik_kernel_path.hpp): n paths of T waypoints, K elbow angles per waypoint,
and the way through them along which the joints move least.

The entry point is defined against rsik_solve_sweep (pinned to the checker by tests/test_gpu_solve_sweep.py): the expected value is
tests/path_workload.path_dp on the library's own sweep over the same T * n poses — NumPy's angle_diff, transition costs and dynamic
programme.  The device's angle_diff and NumPy's can differ in their last bits, so a launch is accepted when
  (a) theta / joints / elbow / projected at (t, i) have the BITS of the sweep's sample index[t][i] (NaN / 0 where index is -1), the
      skipped waypoints are NumPy's, n_solved / interval / reachable / state are the sweep's,
  (b) the cost of the device's path, recomputed by NumPy along `index` from the sweep's joints, is within PATH_TOL = T * 1e-12 of
      NumPy's optimum; `cost` equals it within PATH_TOL, and so does the sum of step_cost ** 2,
  (c) on every path whose second-best distinct path is more than 1e-9 above the optimum, index is NumPy's exactly.
Sizes are the smallest at which the kernel can go wrong: 37 paths (ten workgroups of four, a ragged last one), 70 waypoints (a second,
ragged output trip), K = 64 (every lane), r and l paths in one workgroup."""
import ctypes as C

import numpy as np
import pytest

from compare import bits
from gpu_support import T, abi, cols, last_error, make_symbolic, orc, ptr, raw_call, to_np, torch_mod  # noqa: F401
from nearest_workload import skip_projected_case
from path_workload import GAP, MAIN_SHAPES, N_MAIN, SMALL_SHAPES, cost_along, path_fractions, path_poses, path_start, path_tol
from sampling_support import ALL, check_path, launches, lib_sweep, path_arm_kwargs, path_soa, same_path_outputs

pytestmark = pytest.mark.gpu



# ------------------------------------------------------------------------------------------ 1, 2. sweep samples, and the optimum
@pytest.mark.parametrize("shape", [s + (N_MAIN,) for s in MAIN_SHAPES] + list(SMALL_SHAPES))
def test_the_path_is_made_of_sweep_samples_and_is_the_optimum(torch_mod, shape):
    torch = torch_mod
    t, k, seed, kind, n = shape
    solver, _, _ = make_symbolic(0.03)
    for what, p, th, policy, arm, start in launches(torch, t, k, seed, kind, n):
        sw = lib_sweep(solver, p, th, policy, arm, torch)
        got = to_np(solver.solve_path(p, th, None if start is None else T(start, torch), policy=policy, **path_arm_kwargs(arm, torch)))
        need_gap = n == N_MAIN and policy == "fraction" and k > 1 and (t > 1 or start is not None)
        exp = check_path(got, sw, t, n, what, start, need_gap=need_gap)
        if n == N_MAIN and t >= 5 and policy == "fraction":
            assert 0 < (~exp["solved"]).sum() and exp["solved"].all(axis=0).sum() < n, "the main shapes exercise the skip rule"


# ------------------------------------------------------------------------------------------ 3. the skip rule
@pytest.mark.parametrize("gone", [0, 5, 11])
def test_a_skipped_waypoint_is_as_good_as_absent(torch_mod, gone):
    """(12, 8, 11), every path made unreachable at one waypoint (first, middle, last): the other waypoints carry the bits of the
    same paths without that waypoint, at T and T - 1, with and without start joints."""
    torch = torch_mod
    t, k, n = 12, 8, N_MAIN
    pos, eul, arm = path_poses(11, n, t, "r")
    pos = pos.copy()
    pos[gone] = [2.0, 2.0, 2.0]
    keep = [s for s in range(t) if s != gone]
    th = T(path_fractions(k), torch)
    solver, _, _ = make_symbolic(0.03)
    for start in (None, T(path_start(11, n), torch)):
        a = to_np(solver.solve_path(path_soa(pos, eul, torch), th, start))
        b = to_np(solver.solve_path(path_soa(pos[keep], eul[keep], torch), th, start))
        assert (a["index"][gone] == -1).all() and (a["reachable"][gone] == 0).all() and np.isnan(a["step_cost"][gone]).all()
        assert (b["n_solved"] >= 2).sum() >= 20
        same_path_outputs(a, b, f"waypoint {gone} skipped, start {start is not None}", waypoints=(keep, slice(None)))


# ------------------------------------------------------------------------------------------ 4. against the greedy chain
def test_never_worse_than_the_greedy_chain(torch_mod):
    """(12, 8, 11) without start joints: T chained rsik_solve_nearest launches, each seeded with the winner before it (the first with
    zeros, its own cost not counted; a waypoint without a winner leaves the seed), give a path whose cost — NumPy's, along its
    indices — is never below `cost` - PATH_TOL, and above it by more than GAP on at least 10 paths."""
    torch = torch_mod
    t, k, seed, kind = MAIN_SHAPES[0]
    n = N_MAIN
    pos, eul, arm = path_poses(seed, n, t, kind)
    p, th = path_soa(pos, eul, torch), T(path_fractions(k), torch)
    solver, _, _ = make_symbolic(0.03)
    sw = lib_sweep(solver, p, th, "fraction", arm, torch)
    got = to_np(solver.solve_path(p, th))
    seed_rows = torch.zeros((n, 7), dtype=torch.float64, device="cuda")
    chain = np.full((t, n), -1, dtype=np.int32)
    for s in range(t):
        step = solver.solve_nearest(p[:, s], th, seed_rows)
        won = step["index"] >= 0
        seed_rows = torch.where(won[:, None], step["joints"], seed_rows)
        chain[s] = step["index"].cpu().numpy()
    np.testing.assert_array_equal(chain == -1, got["index"] == -1)
    greedy, _ = cost_along(sw, chain, t, n)
    has = got["n_solved"] > 0
    assert (got["cost"][has] <= greedy[has] + path_tol(t)).all()
    better = int((greedy[has] - got["cost"][has] > GAP).sum())
    print(f"the optimum is below the greedy chain on {better} of {int(has.sum())} paths; median ratio "
          f"{float(np.median(got['cost'][has] / np.maximum(greedy[has], 1e-300))):.2f}")
    assert better >= 10


# ------------------------------------------------------------------------------------------ 5. weights, RSIK_PATH_SKIP_PROJECTED
def test_weights(torch_mod):
    """(12, 8, 11) with (1,1,1,1,0,0,0) and (0.5,0,2,3,5,1,0.25): NumPy's optimum under the same weights, which differs from the unit
    weights' on at least 5 paths; weights of ones are NULL's bits."""
    torch = torch_mod
    t, k, seed, kind = MAIN_SHAPES[0]
    n = N_MAIN
    pos, eul, arm = path_poses(seed, n, t, kind)
    p, th, start = path_soa(pos, eul, torch), T(path_fractions(k), torch), path_start(seed, n)
    solver, _, _ = make_symbolic(0.03)
    sw = lib_sweep(solver, p, th, "fraction", arm, torch)
    unit = to_np(solver.solve_path(p, th, T(start, torch)))
    same_path_outputs(to_np(solver.solve_path(p, th, T(start, torch), weights=(1,) * 7)), unit, "weights of ones against NULL")
    for w in ((1, 1, 1, 1, 0, 0, 0), (0.5, 0, 2, 3, 5, 1, 0.25)):
        got = to_np(solver.solve_path(p, th, T(start, torch), weights=w))
        check_path(got, sw, t, n, f"weights {w}", start, weights=w, need_gap=True)
        differ = int((got["index"] != unit["index"]).any(axis=0).sum())
        print(f"weights {w}: {differ} paths that are not the unit weights'")
        assert differ >= 5


def test_skip_projected(torch_mod, orc):
    """skip_projected_case's 300 steered poses as 75 paths of 4 waypoints, an explicit angle per waypoint and sample (asserted
    before launch: waypoints whose sample 0 projects while a later one does not, and waypoints that project in every sample).
    Without the flag they are solved like any other; with it no winner projects, and a waypoint whose every sample projects is
    skipped: reachable 1, index -1, NaN rows."""
    torch = torch_mod
    pos, eul, arm, thetas, ref, mixed, allp = skip_projected_case(orc)
    t, n, k = 4, 75, thetas.shape[0]
    assert len(pos) == t * n
    p = path_soa(pos.reshape(t, n, 3), eul.reshape(t, n, 3), torch)
    th = T(thetas.reshape(k, t, n), torch)
    start = path_start(33, n)
    solver, _, _ = make_symbolic(0.03)
    sw = lib_sweep(solver, p, th, "explicit", arm[:n], torch)
    np.testing.assert_array_equal(sw["projected"], ref["projected"])
    mixed, allp = mixed.reshape(t, n), allp.reshape(t, n)
    free = to_np(solver.solve_path(p, th, T(start, torch), policy="explicit"))
    check_path(free, sw, t, n, "no flag", start)
    assert (free["index"][allp] >= 0).all() and (free["projected"][allp] == 1).all()
    got = to_np(solver.solve_path(p, th, T(start, torch), policy="explicit", skip_projected=True))
    exp = check_path(got, sw, t, n, "flag", start, skip=True)
    assert (got["projected"] == 0).all() and (got["index"][mixed] >= 1).all()
    assert (got["index"][allp] == -1).all() and (got["reachable"][allp] == 1).all() and np.isnan(got["joints"][allp]).all()
    assert not np.isnan(got["interval"][allp]).any()
    assert (exp["n_solved"] < free["n_solved"]).sum() >= 1 and ((exp["gap"] > GAP) & mixed.any(axis=0)).sum() >= 10


# ------------------------------------------------------------------------------------------ 6. RSIK_PATH_UNWIND
def test_unwind(torch_mod):
    """(12, 8, 11) with explicit angles in [-2 pi, 2 pi] per waypoint and sample, with and without start joints: joints are bit for bit
    T sequential rsik_stage(RSIK_STAGE_ALLOW_MULTITURN) calls over the plain run's rows — each solved row against the solved row
    before it AS WRITTEN, the first against the start row or left alone —, rows cross +-pi (asserted), and nothing else changes."""
    torch = torch_mod
    _abi = abi()
    t, k, seed, kind = MAIN_SHAPES[0]
    n = N_MAIN
    pos, eul, arm = path_poses(seed, n, t, kind)
    p = path_soa(pos, eul, torch)
    th = T(np.random.default_rng(seed + 300).uniform(-2 * np.pi, 2 * np.pi, size=(k, t, n)), torch)
    solver, _, _ = make_symbolic(0.03)
    for start in (None, T(path_start(seed, n) + 4.0, torch)):  # (start rows beyond pi: the first row is carried a turn up)
        plain = solver.solve_path(p, th, start, policy="explicit")
        got = to_np(solver.solve_path(p, th, start, policy="explicit", unwind=True))
        rows = plain["joints"].clone()
        prev = torch.zeros((n, 7), dtype=torch.float64, device="cuda") if start is None else start.clone()
        have = torch.full((n,), start is not None, device="cuda")
        for s in range(t):
            solved = plain["index"][s] >= 0
            out = solver.stage(_abi.STAGE_ALLOW_MULTITURN, torch.cat([rows[s], prev], dim=1).contiguous())
            rows[s] = torch.where((solved & have)[:, None], out, rows[s])
            prev = torch.where(solved[:, None], rows[s], prev)
            have = have | solved
        plain = to_np(plain)
        np.testing.assert_array_equal(bits(got["joints"]), bits(rows.cpu().numpy()), err_msg=f"unwound joints, start {start is not None}")
        moved = (bits(got["joints"]) != bits(plain["joints"])).any(axis=2)
        print(f"start {start is not None}: {int(moved.sum())} of {int((plain['index'] >= 0).sum())} solved rows were unwound")
        assert moved.sum() >= 20 and (np.abs(got["joints"][plain["index"] >= 0]) > np.pi).any()
        same_path_outputs(got, plain, "everything but joints", keys=tuple(key for key in ALL if key != "joints"))


# ------------------------------------------------------------------------------------------ 7. rows that are not numbers
def test_rows_that_are_not_numbers_stay_where_they_are(torch_mod):
    """(12, 8, 11) with start joints.  A NaN / infinity in the pose of one waypoint of three paths: RSIK_STATE_INVALID_INPUT there, the
    waypoint skipped, the path NumPy's optimum without it.  A NaN theta: that sample never wins.  A NaN in three start rows: those
    paths have n_solved 0, index -1, cost NaN, reachable and state unchanged.  Every other path keeps the clean launch's bits."""
    torch = torch_mod
    _abi = abi()
    t, k, seed, kind = MAIN_SHAPES[0]
    n = N_MAIN
    pos, eul, arm = path_poses(seed, n, t, kind)
    p = path_soa(pos, eul, torch)
    start = path_start(seed, n)
    grid = path_fractions(k)
    per = np.repeat(grid[:, None], t * n, axis=1).reshape(k, t, n)
    solver, _, _ = make_symbolic(0.03)

    def run(poses, thetas, st):
        return to_np(solver.solve_path(poses, T(thetas, torch), T(st, torch)))

    clean = run(p, per, start)
    same_path_outputs(run(p, grid, start), clean, "one angle per waypoint and sample against the shared grid")
    whole = np.flatnonzero(clean["n_solved"] == t)
    assert len(whole) >= 9
    # a. poses that are not numbers
    bad = whole[:3]
    p2 = p.clone()
    for q, i in enumerate(bad):
        p2[(0, 4, 2)[q], (0, 6, t - 1)[q], i] = (float("nan"), float("inf"), float("-inf"))[q]
    got = run(p2, per, start)
    others = np.setdiff1d(np.arange(n), bad)
    same_path_outputs(got, clean, "bad poses: the other paths", paths=others)
    for q, i in enumerate(bad):
        s = (0, 6, t - 1)[q]
        assert got["state"][s, i] == _abi.STATE_INVALID_INPUT and got["reachable"][s, i] == 0 and got["index"][s, i] == -1
        assert np.isnan(got["joints"][s, i]).all() and np.isnan(got["interval"][s, i]).all() and got["n_solved"][i] == t - 1
    check_path(got, lib_sweep(solver, p2, T(per, torch), "fraction", arm, torch), t, n, "bad poses", start)
    # b. a theta that is not a number: one the clean path used, one it did not
    i_a, i_b = int(whole[3]), int(whole[4])
    th2 = per.copy()
    th2[clean["index"][5, i_a], 5, i_a] = np.nan
    th2[(clean["index"][5, i_b] + 1) % k, 5, i_b] = np.nan
    got = run(p, th2, start)
    same_path_outputs(got, clean, "a NaN theta: the other paths", paths=np.setdiff1d(np.arange(n), [i_a]))
    assert got["index"][5, i_a] >= 0 and got["index"][5, i_a] != clean["index"][5, i_a] and got["n_solved"][i_a] == t
    check_path(got, lib_sweep(solver, p, T(th2, torch), "fraction", arm, torch), t, n, "a NaN theta", start)
    sh2 = grid.copy()
    sh2[1] = np.nan
    assert (clean["index"] == 1).sum() >= 10
    got = run(p, sh2, start)
    assert not (got["index"] == 1).any() and ((got["index"] >= 0) == (clean["index"] >= 0)).all()
    check_path(got, lib_sweep(solver, p, T(sh2, torch), "fraction", arm, torch), t, n, "a NaN in the shared grid", start)
    # c. start rows that are not numbers
    bad = whole[5:8]
    st2 = start.copy()
    for q, i in enumerate(bad):
        st2[i, (0, 3, 6)[q]] = (np.nan, np.inf, np.nan)[q]
    got = run(p, per, st2)
    same_path_outputs(got, clean, "bad start rows: the other paths", paths=np.setdiff1d(np.arange(n), bad))
    same_path_outputs(got, clean, "bad start rows: is_reachable's outputs", keys=("interval", "reachable", "state"))
    assert (got["n_solved"][bad] == 0).all() and (got["index"][:, bad] == -1).all() and np.isnan(got["cost"][bad]).all()
    assert (got["projected"][:, bad] == 0).all()
    for key in ("theta", "joints", "elbow", "step_cost"):
        assert np.isnan(got[key][:, bad]).all(), key


# ------------------------------------------------------------------------------------------ 8. arguments
def raw_path(solver, n, t, p, k, policy, thetas, per_pose, start=None, weights=None, flags=0, arm=None, arm_uniform=0, workspace=None,
             workspace_bytes=None, **outs):
    """rsik_solve_path on the caller's own buffers: returns the ABI's code."""
    w = None if weights is None else (C.c_double * 7)(*[float(v) for v in weights])
    if workspace_bytes is None:
        workspace_bytes = 0 if workspace is None else workspace.numel()
    o = [ptr(outs.get(key)) for key in ("index", "theta", "joints", "elbow", "projected", "step_cost", "cost", "n_solved", "interval",
                                         "reachable", "state")]
    return raw_call(solver, "rsik_solve_path", n, t, cols(p, 6), ptr(arm), int(arm_uniform), int(k), int(policy), ptr(thetas), int(per_pose),
                    ptr(start), w, int(flags), ptr(workspace), int(workspace_bytes), *o)


def test_arguments(torch_mod):
    """What is refused (RSIK_E_INVALID, the whole text of rsik_last_error, also where a call has two faults; nothing written), n = 0, a workspace of exactly
    the helper's size with guard bytes behind it, and every output left out in turn."""
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
    need = solver.solve_path_workspace_bytes(n, t, k)
    G = 64
    ws = torch.full((need + G,), 0x5A, dtype=u8, device="cuda")
    FR = _abi.THETA_FRACTION

    def fresh():
        def full(shape, dtype):
            return torch.full(shape, 777.0 if dtype == f64 else 77, dtype=dtype, device="cuda")

        return dict(index=full((t, n), i32), theta=full((t, n), f64), joints=full((t, n, 7), f64), elbow=full((t, n, 3), f64),
                    projected=full((t, n), u8), step_cost=full((t, n), f64), cost=full((n,), f64), n_solved=full((n,), i32),
                    interval=full((t, n, 2), f64), reachable=full((t, n), u8), state=full((t, n), u8))

    def untouched(outs):
        torch.cuda.synchronize()
        for key, v in outs.items():
            assert bool((v == (777.0 if v.dtype == f64 else 77)).all()), key
        assert bool((ws == 0x5A).all()), "the workspace"

    outs = fresh()
    no_main = {key: v for key, v in outs.items() if key not in ("index", "theta", "joints")}
    calls = {
        "n_theta 0": (lambda: raw_path(solver, n, t, p, 0, FR, th, 0, start, workspace=ws, **outs), "n_theta must be in [1, 64]"),
        "n_theta 65": (lambda: raw_path(solver, n, t, p, 65, FR, big, 0, start, workspace=ws, **outs), "n_theta must be in [1, 64]"),
        "interval0": (lambda: raw_path(solver, n, t, p, k, _abi.THETA_INTERVAL0, th, 0, start, workspace=ws, **outs), "theta_policy must be RSIK_THETA_EXPLICIT or RSIK_THETA_FRACTION"),
        "a negative weight": (lambda: raw_path(solver, n, t, p, k, FR, th, 0, start, weights=(1, 1, 1, -0.5, 1, 1, 1), workspace=ws, **outs), "every weight must be finite and >= 0"),
        "a NaN weight": (lambda: raw_path(solver, n, t, p, k, FR, th, 0, start, weights=(1, 1, 1, 1, 1, 1, float("nan")), workspace=ws, **outs), "every weight must be finite and >= 0"),
        "flags 4": (lambda: raw_path(solver, n, t, p, k, FR, th, 0, start, flags=4, workspace=ws, **outs), "unknown bits in flags"),
        "flags -1": (lambda: raw_path(solver, n, t, p, k, FR, th, 0, start, flags=-1, workspace=ws, **outs), "unknown bits in flags"),
        "workspace NULL": (lambda: raw_path(solver, n, t, p, k, FR, th, 0, start, workspace=None, workspace_bytes=need, **outs), "workspace is NULL or smaller than rsik_solve_path_workspace_bytes"),
        "workspace one byte short": (lambda: raw_path(solver, n, t, p, k, FR, th, 0, start, workspace=ws, workspace_bytes=need - 1, **outs), "workspace is NULL or smaller than rsik_solve_path_workspace_bytes"),
        "index, theta and joints NULL": (lambda: raw_path(solver, n, t, p, k, FR, th, 0, start, workspace=ws, **no_main), "index, theta and joints are all NULL"),
        "n_steps 0": (lambda: raw_path(solver, n, 0, p, k, FR, th, 0, start, workspace=ws, **outs), "n_steps must be in [1, 65536]"),
        "n_steps 65537": (lambda: raw_path(solver, n, 65537, p, k, FR, th, 0, start, workspace=ws, **outs), "n_steps must be in [1, 65536]"),
        "theta_in NULL": (lambda: raw_path(solver, n, t, p, k, FR, None, 0, start, workspace=ws, **outs), "theta_in is NULL"),
        "pose_soa NULL": (lambda: raw_path(solver, n, t, None, k, FR, th, 0, start, workspace=ws, **outs), "pose_soa is NULL"),
        "n -1": (lambda: raw_path(solver, -1, t, p, k, FR, th, 0, start, workspace=ws, **outs), "n < 0"),
        # two faults in one call: the one the entry point tests first is the one it reports
        "n_theta 0 and interval0": (lambda: raw_path(solver, n, t, p, 0, _abi.THETA_INTERVAL0, th, 0, start, workspace=ws, **outs), "n_theta must be in [1, 64]"),
        "theta_in NULL and pose_soa NULL": (lambda: raw_path(solver, n, t, None, k, FR, None, 0, start, workspace=ws, **outs), "pose_soa is NULL"),
    }
    for name, (call, text) in calls.items():
        rc = call()
        assert rc == _abi.RSIK_E_INVALID, (name, rc)
        assert last_error(solver) == "rsik_solve_path: " + text, (name, last_error(solver))
    untouched(outs)
    # n = 0 launches nothing
    assert raw_path(solver, 0, t, None, k, FR, th, 0, None) == _abi.RSIK_OK
    empty = solver.solve_path(torch.zeros((6, t, 0), dtype=f64, device="cuda"), th)
    assert empty["index"].shape == (t, 0) and empty["joints"].shape == (t, 0, 7) and empty["cost"].shape == (0,)
    untouched(outs)
    # the size helper: monotone in each argument
    size = solver.solve_path_workspace_bytes
    assert need >= n * t * k and size(n + 1, t, k) > need and size(n, t + 1, k) > need and size(n, t, k + 1) > need
    # a workspace of exactly the helper's size: the guard bytes behind it stay
    assert raw_path(solver, n, t, p, k, FR, th, 0, start, workspace=ws, workspace_bytes=need, **outs) == _abi.RSIK_OK, last_error(solver)
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0x5A).all()), "a store ran past the end of the workspace"
    full = {key: v.cpu().numpy() for key, v in outs.items()}
    assert (full["index"] >= 0).sum() > 200
    same_path_outputs(full, to_np(solver.solve_path(p.reshape(6, t, n), th, start)), "the caller's buffers against solve_path")
    # every output left out in turn: the same bits in the rest
    for left_out in list(ALL) + [("index", "theta"), ("index", "joints"), ("theta", "joints", "elbow")]:
        left_out = (left_out,) if isinstance(left_out, str) else left_out
        for flags in (0, _abi.PATH_UNWIND):
            part = {key: v for key, v in fresh().items() if key not in left_out}
            assert raw_path(solver, n, t, p, k, FR, th, 0, start, flags=flags, workspace=ws, **part) == _abi.RSIK_OK, (left_out, last_error(solver))
            torch.cuda.synchronize()
            keys = tuple(key for key in part if not (flags and key == "joints"))
            same_path_outputs({key: v.cpu().numpy() for key, v in part.items()}, full, f"without {left_out}, flags {flags}", keys=keys)
    no_elbow = solver.solve_path(p.reshape(6, t, n), th, start, want_elbow=False)
    assert "elbow" not in no_elbow
    same_path_outputs(to_np(no_elbow), full, "want_elbow=False", keys=tuple(key for key in ALL if key != "elbow"))


# ------------------------------------------------------------------------------------------ 9. the Python layers
def test_python_layers(torch_mod):
    """SymbolicIK.path_batch and DualArmIK.path_batch return the documented shapes and dtypes and the bits of HipSolver.solve_path,
    which are the C call's; the default grid is linspace(0, 1, n_theta); a plan_only launch, re-issued, reproduces the result."""
    torch = torch_mod
    from reachy2_symbolic_ik_amd import DualArmIK

    t, k, n = 12, 8, N_MAIN
    pos, eul, arm = path_poses(11, n, t, "r")
    start = path_start(11, n)
    solver, r, _ = make_symbolic(0.03)
    poses = np.stack([pos, eul], axis=2)  # [T,n,2,3]
    res = r.path_batch(poses, start, n_theta=k)
    want = dict(index=((t, n), torch.int32), theta=((t, n), torch.float64), joints=((t, n, 7), torch.float64), elbow=((t, n, 3), torch.float64),
                projected=((t, n), torch.uint8), step_cost=((t, n), torch.float64), cost=((n,), torch.float64), n_solved=((n,), torch.int32),
                interval=((t, n, 2), torch.float64), reachable=((t, n), torch.uint8), state=((t, n), torch.uint8))
    assert set(res) == set(want)
    for key, (shape, dtype) in want.items():
        assert tuple(res[key].shape) == shape and res[key].dtype == dtype and res[key].is_cuda, key
    res = to_np(res)
    p = path_soa(pos, eul, torch)
    grid = torch.linspace(0.0, 1.0, k, dtype=torch.float64)
    raw = to_np(solver.solve_path(p, grid, T(start, torch)))
    same_path_outputs(res, raw, "SymbolicIK.path_batch")
    check_path(res, lib_sweep(solver, p, grid.cuda(), "fraction", arm, torch), t, n, "path_batch against the sweep over its grid", start)
    same_path_outputs(to_np(r.path_batch(p, start, n_theta=k)), raw, "SoA poses")
    # explicit angles per waypoint, weights, both flags
    th = np.random.default_rng(62).uniform(-np.pi, np.pi, size=(3, t, n))
    w = (1, 2, 3, 4, 0.5, 0.25, 0)
    a = to_np(r.path_batch(poses, start, thetas=th, policy="explicit", weights=w, skip_projected=True, unwind=True))
    b = to_np(solver.solve_path(p, T(th, torch), T(start, torch), policy="explicit", weights=w, skip_projected=True, unwind=True))
    same_path_outputs(a, b, "explicit, weights, skip_projected, unwind")
    # plan_only: nothing launched, the re-launch reproduces the result
    out = {key: torch.full(shape, 77, dtype=dtype, device="cuda") for key, (shape, dtype) in want.items()}
    planned = r.path_batch(poses, start, n_theta=k, out=out, plan_only=True)
    torch.cuda.synchronize()
    assert bool((out["index"] == 77).all()) and bool((out["joints"] == 77).all()), "plan_only must not launch"
    for again in ("", ", again"):
        planned["launch"]()
        torch.cuda.synchronize()
        same_path_outputs({key: out[key].cpu().numpy() for key in want}, raw, "planned launch" + again)
    # both arms
    pos, eul, arm = path_poses(21, n, t, "mixed")
    assert 0 < arm.sum() < n
    dual = DualArmIK(solver=solver, singularity_offset=0.03)
    d = to_np(dual.path_batch(arm, np.stack([pos, eul], axis=2), start, n_theta=k))
    raw = to_np(solver.solve_path(path_soa(pos, eul, torch), grid, T(start, torch), arm=T(arm, torch)))
    assert d["joints"].shape == (t, n, 7) and d["index"].dtype == np.int32
    same_path_outputs(d, raw, "DualArmIK.path_batch")
    # what the Python driver refuses before any launch, by its whole text
    refused = {
        "policy must be 'fraction' or 'explicit'": lambda: solver.solve_path(p, grid, policy="interval0"),
        "thetas must have shape [K] or [K, T, n]": lambda: solver.solve_path(p, torch.zeros((k, n), dtype=torch.float64)),
        "thetas: between 1 and 64 samples per waypoint": lambda: solver.solve_path(p, torch.zeros(65, dtype=torch.float64)),
        f"thetas: expected shape {(k, t, n)}, got {(k, t, n + 1)}": lambda: solver.solve_path(p, torch.zeros((k, t, n + 1), dtype=torch.float64)),
        "weights must have 7 entries": lambda: solver.solve_path(p, grid, weights=(1,) * 6),
    }
    for text, call in refused.items():
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
