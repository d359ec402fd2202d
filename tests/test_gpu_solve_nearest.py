"""GPU tests (-m gpu, MI355X) of rsik_solve_nearest (csrc/rsik_kernel_nearest.hpp): of K elbow angles per pose, the one whose
solution is nearest to the pose's seed joints, one row per pose.

The entry point is defined against rsik_solve_sweep (pinned to the checker by tests/test_gpu_solve_sweep.py): the expected value is
tests/nearest_workload.nearest_from_sweep on the library's own sweep over the same inputs — NumPy's angle_diff, cost and first
argmin.  The device's angle_diff and NumPy's can differ in their last bits, so a row is accepted when
  (a) theta / joints / elbow / projected have the BITS of the sweep's sample index[i] (NaN / 0 where index is -1),
  (b) c_numpy[index[i]] <= c_min + 1e-12 max(1, c_min)   (c <= 7 pi^2, ~25 roundings of 1.1e-16 relative: <= 2e-13, a 5 x margin),
  (c) where the best and second-best candidate are more than 1e-9 apart, index is NumPy's argmin exactly,
  (d) cost is within 1e-12 of sqrt(c_numpy[index]),
and interval / reachable / state have the sweep's bits.  Sizes are the smallest at which the kernel can go wrong: several blocks
with a ragged last block and a ragged last wave, r and l alternating inside every wave, K crossing a lane group."""
import ctypes as C

import numpy as np
import pytest

from checker_support import reachable_rich
from compare import bits
from gpu_support import KINDS, T, abi, cols, last_error, make_symbolic, orc, ptr, raw_call, soa, to_np, torch_mod  # noqa: F401
from nearest_workload import GAP, KS, N_MAIN, main_case, main_thetas, seeds, skip_projected_case
from sampling_support import LANES, ROWS, check_nearest, main_launches, same_nearest_outputs
from sweep_workload import sweep_poses, sweep_thetas

pytestmark = pytest.mark.gpu



def raw_nearest(solver, n, p, k, policy, thetas, per_pose, seed, weights=None, flags=0, arm=None, arm_uniform=0, prev=None,
                index=None, theta=None, joints=None, elbow=None, cost=None, projected=None, interval=None, reachable=None, state=None):
    """rsik_solve_nearest on the caller's own buffers: returns the ABI's code."""
    w = None if weights is None else (C.c_double * 7)(*[float(v) for v in weights])
    return raw_call(solver, "rsik_solve_nearest", n, cols(p, 6), ptr(arm), int(arm_uniform), int(k), int(policy), ptr(thetas), int(per_pose),
                    ptr(prev), ptr(seed), w, int(flags), ptr(index), ptr(theta), ptr(joints), ptr(elbow), ptr(cost), ptr(projected),
                    ptr(interval), ptr(reachable), ptr(state))


# ------------------------------------------------------------------------------------------ 1. the winner is a sweep sample
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", KS)
def test_the_winner_is_a_sample_of_the_sweep(torch_mod, kind, k):
    """n = 1000, K in {1, 3, 8, 70}, both policies, shared and per-pose theta, with and without previous_joints rows, each forced
    L in {1, 8, 64} and the library's own choice: (a) - (d), after the gap condition has been asserted on the library's sweep."""
    torch = torch_mod
    _abi = abi()
    solver, _, _ = make_symbolic(0.03)
    for what, p, th, seedT, kw, seed in main_launches(torch, kind, k):
        sw = to_np(solver.solve_sweep(p, th, **kw))
        ok = sw["reachable"].astype(bool)
        assert ok[0::2].mean() >= 0.04 and ok[1::2].mean() > 0.5, what
        for lanes in LANES:
            solver.set_option(_abi.OPT_NEAREST_LANES, lanes)
            got = to_np(solver.solve_nearest(p, th, seedT, **kw))
            check_nearest(got, sw, seed, f"{what} L {lanes}", need_gap=True)
            assert np.isnan(got["joints"][~ok]).all() and np.isnan(got["elbow"][~ok]).all() and np.isnan(got["theta"][~ok]).all()
            assert np.isnan(got["cost"][~ok]).all() and (got["projected"][~ok] == 0).all()


# ------------------------------------------------------------------------------------------ 2. every L gives the same bits
@pytest.mark.parametrize("kind", KINDS)
def test_every_lane_count_gives_the_same_bits(torch_mod, kind):
    """Test 1's inputs: all outputs, index included, are the same bits under the four values of RSIK_OPT_NEAREST_LANES."""
    torch = torch_mod
    _abi = abi()
    solver, _, _ = make_symbolic(0.03)
    for k in KS:
        for what, p, th, seedT, kw, _ in main_launches(torch, kind, k):
            outs = {}
            for lanes in LANES:
                solver.set_option(_abi.OPT_NEAREST_LANES, lanes)
                outs[lanes] = to_np(solver.solve_nearest(p, th, seedT, **kw))
            assert (outs[1]["index"] >= 0).sum() > 300, what
            for lanes in LANES[1:]:
                same_nearest_outputs(outs[lanes], outs[0], f"{what}: L {lanes} against the library's choice")


# ------------------------------------------------------------------------------------------ 3. ties go to the lowest k
@pytest.mark.parametrize("lanes", LANES)
def test_ties_go_to_the_lowest_sample(torch_mod, lanes):
    """K = 6, per-pose explicit theta whose columns 1 and 4 are equal, seed = the sweep's joints of sample 4: samples 1 and 4 both
    cost exactly 0 (the same function on the same operands), and index is 1 with cost 0 on every reachable row."""
    torch = torch_mod
    _abi = abi()
    n, k = 600, 6
    pos, eul, arm = sweep_poses("mixed", 71, n)
    thetas = sweep_thetas("explicit", True, k, n, 72)
    thetas[4] = thetas[1]
    p, th, armT = soa(pos, eul, torch), T(thetas, torch), T(arm, torch)
    solver, _, _ = make_symbolic(0.03)
    sw = to_np(solver.solve_sweep(p, th, policy="explicit", arm=armT))
    ok = sw["reachable"].astype(bool)
    assert ok.sum() >= 100
    np.testing.assert_array_equal(bits(sw["joints"][1]), bits(sw["joints"][4]))
    seed = np.where(ok[:, None], sw["joints"][4], seeds(n, 73))
    solver.set_option(_abi.OPT_NEAREST_LANES, lanes)
    got = to_np(solver.solve_nearest(p, th, T(seed, torch), policy="explicit", arm=armT))
    assert (got["index"][ok] == 1).all() and (got["cost"][ok] == 0.0).all()
    assert (got["index"][~ok] == -1).all()
    check_nearest(got, sw, seed, f"ties L {lanes}")


# ------------------------------------------------------------------------------------------ 4. RSIK_NEAREST_SKIP_PROJECTED
def test_skip_projected(torch_mod, orc):
    """n = 300, K = 4, theta steered with the checker (asserted before launch: >= 20 poses whose sample 0 projects while a later
    one does not, >= 1 pose that projects in every sample); seed = the projecting sample 0's joints.  Without the flag sample 0
    wins with cost 0; with it the winner has projected == 0 and is NumPy's argmin over the rest; the poses that project in every
    sample give index -1, NaN, reachable 1."""
    torch = torch_mod
    _abi = abi()
    pos, eul, arm, thetas, ref, mixed, allp = skip_projected_case(orc)
    n = len(pos)
    p, th = soa(pos, eul, torch), T(thetas, torch)
    solver, _, _ = make_symbolic(0.03)
    sw = to_np(solver.solve_sweep(p, th, policy="explicit"))
    np.testing.assert_array_equal(sw["projected"], ref["projected"])
    np.testing.assert_array_equal(sw["reachable"], ref["reachable"])
    ok = sw["reachable"].astype(bool)
    seed = np.where(ok[:, None], sw["joints"][0], seeds(n, 33))
    seedT = T(seed, torch)
    for lanes in LANES:
        solver.set_option(_abi.OPT_NEAREST_LANES, lanes)
        free = to_np(solver.solve_nearest(p, th, seedT, policy="explicit"))
        check_nearest(free, sw, seed, f"no flag L {lanes}")
        assert (free["index"][ok] == 0).all() and (free["cost"][ok] == 0.0).all()
        assert (free["projected"][mixed | allp] == 1).all()
        got = to_np(solver.solve_nearest(p, th, seedT, policy="explicit", skip_projected=True))
        exp = check_nearest(got, sw, seed, f"flag L {lanes}", skip=True)
        won = got["index"] >= 0
        assert (got["projected"][won] == 0).all()
        assert (got["index"][mixed] >= 1).all()
        clear = mixed & (exp["gap"] > GAP)
        assert clear.sum() >= 20
        np.testing.assert_array_equal(got["index"][clear], exp["index"][clear])
        assert (got["index"][allp] == -1).all() and (got["reachable"][allp] == 1).all() and (got["projected"][allp] == 0).all()
        for key in ("theta", "joints", "elbow", "cost"):
            assert np.isnan(got[key][allp]).all(), key
        assert not np.isnan(got["interval"][allp]).any()


# ------------------------------------------------------------------------------------------ 5. weights
def test_weights(torch_mod):
    """(1,1,1,1,0,0,0) and (0,0,0,0,2,3,5) against NumPy; a negative, NaN or infinite weight is RSIK_E_INVALID and writes nothing."""
    torch = torch_mod
    _abi = abi()
    k = 8
    pos, eul, arm, seed = main_case("mixed", k)
    p, armT, seedT = soa(pos, eul, torch), T(arm, torch), T(seed, torch)
    th = T(main_thetas("fraction", True, k), torch)
    solver, _, _ = make_symbolic(0.03)
    sw = to_np(solver.solve_sweep(p, th, arm=armT))
    unit = to_np(solver.solve_nearest(p, th, seedT, arm=armT))
    for w in ((1, 1, 1, 1, 0, 0, 0), (0, 0, 0, 0, 2, 3, 5)):
        differ = 0
        for lanes in LANES:
            solver.set_option(_abi.OPT_NEAREST_LANES, lanes)
            got = to_np(solver.solve_nearest(p, th, seedT, weights=w, arm=armT))
            check_nearest(got, sw, seed, f"weights {w} L {lanes}", weights=w, need_gap=True)
            differ = int((got["index"] != unit["index"]).sum())
        print(f"weights {w}: {differ} rows whose winner is not the unit weights'")
        assert differ >= 10
    solver.set_option(_abi.OPT_NEAREST_LANES, 0)
    ones = to_np(solver.solve_nearest(p, th, seedT, weights=(1,) * 7, arm=armT))
    same_nearest_outputs(ones, unit, "weights of ones against NULL")
    index = torch.full((N_MAIN,), 77, dtype=torch.int32, device="cuda")
    for bad in (-1.0, float("nan"), float("inf"), -0.5):
        for q in (0, 6):
            w = [1.0] * 7
            w[q] = bad
            rc = raw_nearest(solver, N_MAIN, p, k, _abi.THETA_FRACTION, th, 1, seedT, weights=w, arm=armT, index=index)
            assert rc == _abi.RSIK_E_INVALID and "rsik_solve_nearest" in last_error(solver), (bad, q, rc)
    torch.cuda.synchronize()
    assert bool((index == 77).all())


# ------------------------------------------------------------------------------------------ 6. ragged sizes and bleed
@pytest.mark.parametrize("lanes", (1, 8, 64))
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257])
def test_ragged_sizes_do_not_bleed(torch_mod, n, lanes):
    """K = 3, r and l mixed; three guard rows behind every output keep their sentinel, and the rows in front are the sweep's."""
    torch = torch_mod
    _abi = abi()
    k, G = 3, 3
    rng = np.random.default_rng(300 + n)
    arm = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    pos, eul = reachable_rich(100 + n, n, arm)
    p, armT = soa(pos, eul, torch), T(arm, torch)
    thetas = sweep_thetas("fraction", True, k, n, 700 + n)
    th = T(thetas, torch)
    seed = seeds(n, 800 + n)
    solver, _, _ = make_symbolic(0.03)
    sw = to_np(solver.solve_sweep(p, th, arm=armT))
    f64, u8 = torch.float64, torch.uint8

    def guarded(width, dtype, fill):
        return torch.full((n + G, width) if width else (n + G,), fill, dtype=dtype, device="cuda")

    outs = dict(index=guarded(0, torch.int32, 77), theta=guarded(0, f64, 777.0), joints=guarded(7, f64, 777.0), elbow=guarded(3, f64, 777.0),
                cost=guarded(0, f64, 777.0), projected=guarded(0, u8, 77), interval=guarded(2, f64, 777.0), reachable=guarded(0, u8, 77),
                state=guarded(0, u8, 77))
    solver.set_option(_abi.OPT_NEAREST_LANES, lanes)
    rc = raw_nearest(solver, n, p, k, _abi.THETA_FRACTION, th, 1, T(seed, torch), arm=armT, **outs)
    assert rc == _abi.RSIK_OK, last_error(solver)
    torch.cuda.synchronize()
    for key, t in outs.items():
        assert bool((t[n:] == (777.0 if t.dtype == f64 else 77)).all()), f"{key}: a store ran past the end of its array"
    got = {key: t[:n].cpu().numpy() for key, t in outs.items()}
    assert sw["reachable"].any() or n < 3
    check_nearest(got, sw, seed, f"n {n} L {lanes}")


# ------------------------------------------------------------------------------------------ 7. rows that are not numbers
def test_rows_that_are_not_numbers_stay_where_they_are(torch_mod):
    """include/rsik.h "Rows that are not numbers", n = 3000, K = 4.  A NaN / +-inf in 12 poses: RSIK_STATE_INVALID_INPUT and index -1
    there, every other row keeps the bits of the clean launch.  A NaN in 12 seed rows: index -1 there only.  A NaN in one entry
    of a per-pose theta array: that row keeps the clean launch's result unless the sample was its winner, then it is NumPy's
    argmin without it.  A NaN in one sample of a shared grid: that k never appears in index."""
    torch = torch_mod
    _abi = abi()
    n, k = 3000, 4
    rng = np.random.default_rng(90)
    arm = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    pos, eul = reachable_rich(91, n, arm)
    p, armT = soa(pos, eul, torch), T(arm, torch)
    solver, _, _ = make_symbolic(0.03)
    per_pose = sweep_thetas("fraction", True, k, n, 92)
    shared = sweep_thetas("fraction", False, k, n, 93)
    seed = seeds(n, 94)

    def run(poses, thetas, sd):
        res = solver.solve_nearest(poses, T(thetas, torch), T(sd, torch), arm=armT)
        torch.cuda.synchronize()
        return to_np(res)

    def sweep(poses, thetas):
        return to_np(solver.solve_sweep(poses, T(thetas, torch), arm=armT))

    clean = run(p, per_pose, seed)
    check_nearest(clean, sweep(p, per_pose), seed, "clean")
    ok = clean["reachable"].astype(bool)
    assert (clean["index"][ok] >= 0).all() and ok.sum() > 1500
    # a. poses that are not numbers
    bad = rng.choice(n, size=12, replace=False)
    p2 = p.clone()
    for q, row in enumerate(bad):
        p2[q % 6, row] = (float("nan"), float("inf"), float("-inf"))[q % 3]
    got = run(p2, per_pose, seed)
    keep = np.ones(n, dtype=bool)
    keep[bad] = False
    same_nearest_outputs(got, clean, "bad poses: the other rows", rows=keep)
    assert (got["state"][bad] == _abi.STATE_INVALID_INPUT).all() and (got["reachable"][bad] == 0).all() and (got["index"][bad] == -1).all()
    assert (got["projected"][bad] == 0).all()
    for key in ("theta", "joints", "elbow", "cost", "interval"):
        assert np.isnan(got[key][bad]).all(), key
    # b. seed rows that are not numbers
    bad = rng.choice(np.flatnonzero(ok), size=12, replace=False)
    seed2 = seed.copy()
    for q, row in enumerate(bad):
        seed2[row, q % 7] = np.nan
    got = run(p, per_pose, seed2)
    keep = np.ones(n, dtype=bool)
    keep[bad] = False
    same_nearest_outputs(got, clean, "bad seed rows: the other rows", rows=keep)
    same_nearest_outputs(got, clean, "bad seed rows: is_reachable's outputs", keys=("interval", "reachable", "state"))
    assert (got["index"][bad] == -1).all() and (got["reachable"][bad] == 1).all() and (got["projected"][bad] == 0).all()
    for key in ("theta", "joints", "elbow", "cost"):
        assert np.isnan(got[key][bad]).all(), key
    # c. one entry of a per-pose theta array: a sample that was not the winner, and one that was
    reach = np.flatnonzero(ok)
    row_a = int(reach[len(reach) // 2])
    row_b = int(reach[len(reach) // 3])
    th2 = per_pose.copy()
    th2[(clean["index"][row_a] + 1) % k, row_a] = np.nan
    th2[clean["index"][row_b], row_b] = np.nan
    got = run(p, th2, seed)
    keep = np.ones(n, dtype=bool)
    keep[row_b] = False
    same_nearest_outputs(got, clean, "a NaN theta beside the winner", rows=keep)
    exp = check_nearest(got, sweep(p, th2), seed, "a NaN theta entry")
    assert got["index"][row_b] >= 0 and got["index"][row_b] != clean["index"][row_b]
    if exp["gap"][row_b] > GAP:
        assert got["index"][row_b] == exp["index"][row_b]
    # d. one sample of a shared grid
    clean_s = run(p, shared, seed)
    assert (clean_s["index"] == 1).sum() > 50
    sh2 = shared.copy()
    sh2[1] = np.nan
    got = run(p, sh2, seed)
    assert not (got["index"] == 1).any() and (got["index"][ok] >= 0).all()
    check_nearest(got, sweep(p, sh2), seed, "a NaN in the shared grid")
    same_nearest_outputs(got, clean_s, "the rows sample 1 did not win", rows=clean_s["index"] != 1)


# ------------------------------------------------------------------------------------------ 8. arguments
def test_arguments(torch_mod):
    """What is refused (with the whole text of rsik_last_error, also where a call has two faults; nothing written) — RSIK_OPT_NEAREST_LANES = 3 is
    refused by rsik_set_option, the entry point that takes it —, a context without an arm, n = 0, and every optional output left
    out in turn."""
    torch = torch_mod
    _abi = abi()
    from reachy2_symbolic_ik_amd import HipSolver

    n, k = 300, 3
    arm = np.zeros(n, dtype=np.uint8)
    pos, eul = reachable_rich(81, n, arm)
    p = soa(pos, eul, torch)
    solver, _, _ = make_symbolic(0.03)
    f64, u8 = torch.float64, torch.uint8
    th = T(np.linspace(0.0, 1.0, k), torch)
    big = T(np.linspace(0.0, 1.0, 4097), torch)
    seed = T(seeds(n, 82), torch)

    def fresh():
        return dict(index=torch.full((n,), 77, dtype=torch.int32, device="cuda"), theta=torch.full((n,), 777.0, dtype=f64, device="cuda"),
                    joints=torch.full((n, 7), 777.0, dtype=f64, device="cuda"), elbow=torch.full((n, 3), 777.0, dtype=f64, device="cuda"),
                    cost=torch.full((n,), 777.0, dtype=f64, device="cuda"), projected=torch.full((n,), 77, dtype=u8, device="cuda"),
                    interval=torch.full((n, 2), 777.0, dtype=f64, device="cuda"), reachable=torch.full((n,), 77, dtype=u8, device="cuda"),
                    state=torch.full((n,), 77, dtype=u8, device="cuda"))

    outs = fresh()
    FR = _abi.THETA_FRACTION
    no_main = {key: v for key, v in outs.items() if key not in ("index", "theta", "joints")}
    calls = {
        "n_theta 0": (lambda: raw_nearest(solver, n, p, 0, FR, th, 0, seed, **outs), "n_theta must be in [1, 4096]"),
        "n_theta 4097": (lambda: raw_nearest(solver, n, p, 4097, FR, big, 0, seed, **outs), "n_theta must be in [1, 4096]"),
        "interval0": (lambda: raw_nearest(solver, n, p, k, _abi.THETA_INTERVAL0, th, 0, seed, **outs), "theta_policy must be RSIK_THETA_EXPLICIT or RSIK_THETA_FRACTION"),
        "none": (lambda: raw_nearest(solver, n, p, k, _abi.THETA_NONE, th, 0, seed, **outs), "theta_policy must be RSIK_THETA_EXPLICIT or RSIK_THETA_FRACTION"),
        "theta_in NULL": (lambda: raw_nearest(solver, n, p, k, FR, None, 0, seed, **outs), "theta_in is NULL"),
        "seed_joints NULL": (lambda: raw_nearest(solver, n, p, k, FR, th, 0, None, **outs), "seed_joints is NULL"),
        "index, theta and joints NULL": (lambda: raw_nearest(solver, n, p, k, FR, th, 0, seed, **no_main), "index, theta and joints are all NULL"),
        "flags 2": (lambda: raw_nearest(solver, n, p, k, FR, th, 0, seed, flags=2, **outs), "unknown bits in flags"),
        "flags 3": (lambda: raw_nearest(solver, n, p, k, FR, th, 0, seed, flags=3, **outs), "unknown bits in flags"),
        "flags -1": (lambda: raw_nearest(solver, n, p, k, FR, th, 0, seed, flags=-1, **outs), "unknown bits in flags"),
        "pose_soa NULL": (lambda: raw_nearest(solver, n, None, k, FR, th, 0, seed, **outs), "pose_soa is NULL"),
        "n -1": (lambda: raw_nearest(solver, -1, p, k, FR, th, 0, seed, **outs), "n < 0"),
        # two faults in one call: the one the entry point tests first is the one it reports
        "n_theta 0 and interval0": (lambda: raw_nearest(solver, n, p, 0, _abi.THETA_INTERVAL0, th, 0, seed, **outs), "n_theta must be in [1, 4096]"),
        "theta_in NULL and pose_soa NULL": (lambda: raw_nearest(solver, n, None, k, FR, None, 0, seed, **outs), "pose_soa is NULL"),
    }
    for name, (call, text) in calls.items():
        rc = call()
        assert rc == _abi.RSIK_E_INVALID, (name, rc)
        assert last_error(solver) == "rsik_solve_nearest: " + text, (name, last_error(solver))
    for value in (3, 2, 7, 9, 63, 65, 128, -1):
        with pytest.raises(_abi.RsikError) as e:
            solver.set_option(_abi.OPT_NEAREST_LANES, value)
        assert e.value.code == _abi.RSIK_E_INVALID and "rsik_set_option" in last_error(solver), value
        assert solver.get_option(_abi.OPT_NEAREST_LANES) == 0
    torch.cuda.synchronize()
    for key, t in outs.items():
        assert bool((t == (777.0 if t.dtype == f64 else 77)).all()), key
    bare = HipSolver(0)  # no arm uploaded
    assert raw_nearest(bare, n, p, k, FR, th, 0, seed, **outs) == _abi.RSIK_E_NOT_SET
    assert last_error(bare) == "rsik_solve_nearest: constants of the requested arm were not uploaded"
    assert raw_nearest(bare, n, p, k, FR, th, 0, seed, arm=T(arm, torch), **outs) == _abi.RSIK_E_NOT_SET
    assert last_error(bare) == "rsik_solve_nearest: per-pose arm ids need both arms' constants (rsik_set_arm)"
    bare.close()
    # n = 0
    assert raw_nearest(solver, 0, None, k, FR, th, 0, None) == _abi.RSIK_OK
    empty = solver.solve_nearest(torch.zeros((6, 0), dtype=f64, device="cuda"), th, torch.zeros((0, 7), dtype=f64, device="cuda"))
    assert empty["index"].shape == (0,) and empty["joints"].shape == (0, 7) and empty["elbow"].shape == (0, 3)
    assert empty["interval"].shape == (0, 2) and empty["state"].shape == (0,)
    torch.cuda.synchronize()
    for key, t in outs.items():
        assert bool((t == (777.0 if t.dtype == f64 else 77)).all()), key
    # every optional output left out in turn: the same bits in the rest
    assert raw_nearest(solver, n, p, k, FR, th, 0, seed, **outs) == _abi.RSIK_OK, last_error(solver)
    torch.cuda.synchronize()
    full = {key: t.cpu().numpy() for key, t in outs.items()}
    assert (full["index"] >= 0).sum() > 100
    for lanes in (1, 8, 64):
        solver.set_option(_abi.OPT_NEAREST_LANES, lanes)
        for left_out in list(ROWS) + [("index", "theta"), ("index", "joints"), ("theta", "joints", "elbow")]:
            left_out = (left_out,) if isinstance(left_out, str) else left_out
            part = {key: t for key, t in fresh().items() if key not in left_out}
            assert raw_nearest(solver, n, p, k, FR, th, 0, seed, **part) == _abi.RSIK_OK, (left_out, last_error(solver))
            torch.cuda.synchronize()
            same_nearest_outputs({key: t.cpu().numpy() for key, t in part.items()}, full, f"without {left_out}, L {lanes}", keys=tuple(part))
    solver.set_option(_abi.OPT_NEAREST_LANES, 0)
    no_elbow = solver.solve_nearest(p, th, seed, want_elbow=False)
    assert "elbow" not in no_elbow
    same_nearest_outputs(to_np(no_elbow), full, "want_elbow=False", keys=tuple(key for key in ROWS if key != "elbow"))


# ------------------------------------------------------------------------------------------ 9. Python surface
def test_python_surface(torch_mod):
    """SymbolicIK.nearest_batch and DualArmIK.nearest_batch return the documented shapes and dtypes and the bits of
    HipSolver.solve_nearest; the default grid is linspace(0, 1, n_theta); a plan_only launch re-issued reproduces the result."""
    torch = torch_mod
    from reachy2_symbolic_ik_amd import DualArmIK

    n, k = 500, 5
    arm = (np.random.default_rng(60).uniform(size=n) < 0.5).astype(np.uint8)
    pos_r, eul_r = reachable_rich(61, n, np.zeros(n, dtype=np.uint8))
    seed = seeds(n, 64)
    solver, r, _ = make_symbolic(0.03)
    poses = np.stack([pos_r, eul_r], axis=1)  # [n,2,3]
    res = r.nearest_batch(poses, seed, n_theta=k)
    want = dict(index=((n,), torch.int32), theta=((n,), torch.float64), joints=((n, 7), torch.float64), elbow=((n, 3), torch.float64),
                cost=((n,), torch.float64), projected=((n,), torch.uint8), interval=((n, 2), torch.float64),
                reachable=((n,), torch.uint8), state=((n,), torch.uint8))
    assert set(res) == set(want)
    for key, (shape, dtype) in want.items():
        assert tuple(res[key].shape) == shape and res[key].dtype == dtype and res[key].is_cuda, key
    res = to_np(res)
    grid = torch.linspace(0.0, 1.0, k, dtype=torch.float64)
    p = soa(pos_r, eul_r, torch)
    raw = to_np(solver.solve_nearest(p, grid, T(seed, torch), policy="fraction", arm_uniform=0))
    same_nearest_outputs(res, raw, "SymbolicIK.nearest_batch")
    check_nearest(res, to_np(solver.solve_sweep(p, grid)), seed, "nearest_batch against sweep_batch's grid")
    assert (res["index"] >= 0).sum() > 250
    default = r.nearest_batch(poses, seed)  # n_theta = 64
    check_nearest(to_np(default), to_np(solver.solve_sweep(p, torch.linspace(0.0, 1.0, 64, dtype=torch.float64))), seed, "default grid")
    # explicit angles, one column per pose, previous_joints rows, weights, the flag
    th = sweep_thetas("explicit", True, 3, n, 62)
    prev = np.random.default_rng(63).uniform(-2, 2, size=(n, 7))
    w = (1, 2, 3, 4, 0.5, 0.25, 0)
    a = to_np(r.nearest_batch(poses, seed, thetas=th, policy="explicit", previous_joints=prev, weights=w, skip_projected=True))
    b = to_np(solver.solve_nearest(p, T(th, torch), T(seed, torch), policy="explicit", previous_joints=T(prev, torch), weights=w,
                                   skip_projected=True))
    same_nearest_outputs(a, b, "explicit, previous_joints, weights, skip_projected")
    sw = to_np(solver.solve_sweep(p, T(th, torch), policy="explicit", previous_joints=T(prev, torch)))
    check_nearest(a, sw, seed, "explicit, previous_joints, weights, skip_projected", weights=w, skip=True)
    # plan_only: nothing launched, the re-launch reproduces the result
    out = {key: torch.full(shape, 77, dtype=dtype, device="cuda") for key, (shape, dtype) in want.items()}
    planned = r.nearest_batch(poses, seed, n_theta=k, out=out, plan_only=True)
    torch.cuda.synchronize()
    assert bool((out["index"] == 77).all()) and bool((out["joints"] == 77).all()), "plan_only must not launch"
    planned["launch"]()
    torch.cuda.synchronize()
    same_nearest_outputs({key: out[key].cpu().numpy() for key in want}, raw, "planned launch")
    planned["launch"]()
    torch.cuda.synchronize()
    same_nearest_outputs({key: out[key].cpu().numpy() for key in want}, raw, "planned launch, again")
    # both arms
    pos, eul = reachable_rich(61, n, arm)
    dual = DualArmIK(solver=solver, singularity_offset=0.03)
    d = to_np(dual.nearest_batch(arm, np.stack([pos, eul], axis=1), seed, n_theta=k))
    raw = to_np(solver.solve_nearest(soa(pos, eul, torch), grid, T(seed, torch), arm=T(arm, torch)))
    assert d["joints"].shape == (n, 7) and d["index"].dtype == np.int32
    same_nearest_outputs(d, raw, "DualArmIK.nearest_batch")
    # what the Python driver refuses before any launch, by its whole text
    seedT = T(seed, torch)
    refused = {
        "policy must be 'fraction' or 'explicit'": lambda: solver.solve_nearest(p, grid, seedT, policy="interval0"),
        "thetas must have shape [K] or [K, n]": lambda: solver.solve_nearest(p, torch.zeros((k, n, 1), dtype=torch.float64), seedT),
        "thetas: between 1 and 4096 samples per pose": lambda: solver.solve_nearest(p, torch.zeros(4097, dtype=torch.float64), seedT),
        f"thetas: expected shape {(k, n)}, got {(k, n + 1)}": lambda: solver.solve_nearest(p, torch.zeros((k, n + 1), dtype=torch.float64), seedT),
        "weights must have 7 entries": lambda: solver.solve_nearest(p, grid, seedT, weights=(1,) * 6),
    }
    for text, call in refused.items():
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
