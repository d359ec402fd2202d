"""GPU tests (-m gpu, MI355X) of rsik_reach_map (csrc/rsik_kernel_reach_map.hpp): is_reachable of n_pos positions x n_rot
orientations, reduced per position on the device.

The entry point is defined against what exists: reachable, state and interval of pose (i, j) are, bit for bit, rsik_solve's under
RSIK_THETA_NONE for position i with orientation j and arm byte arm[i].  So the first reference is the library's own rsik_solve on the
tiled poses (integers and mask exact, the measure within the rounding of a sum in another order); the second the CPU checker
(tests/reach_map_workload.expected_map, pinned on the checker alone by tests/test_reach_map_abi.py).  Shapes are the smallest at
which the kernel can go wrong: one orientation, one short of / exactly / one past a 64-orientation chunk, two chunks and a ragged
third, more than one 1024-orientation tile; one position, fewer and more positions than a workgroup holds, and the position counts at
which the host gives a wave two, four, eight and sixteen positions.
"""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from arm_pairs import checker_arms, upload
from checker_support import default_arms
from compare import TOL, same_bits
from gpu_support import KINDS, T, abi, arm_kwargs, last_error, make_symbolic, orc, ptr, raw_call, soa, torch_mod  # noqa: F401
from reach_map_workload import N_STATES, expected_map, map_case, map_orientations, pack_mask, reduce_map, rounding_bound, tile

pytestmark = pytest.mark.gpu

OUTPUTS = ("count", "state_count", "theta_measure", "mask")
WAVES_PER_BLOCK = 4  # kReachMapWaves: with one position per wave a workgroup holds 4 positions


def default_solver():
    solver, r, l = make_symbolic(0.03)
    r._upload()
    l._upload()
    return solver, r, l


def positions(orc, kind, n_pos, seed):
    """n_pos positions of the test grid's box (and their arm bytes for kind "mixed"): up to 729 a shuffled subset of the grid itself,
    above that uniform in the box around the position's own shoulder."""
    arms = default_arms()
    P, arm_ids, _ = map_case(arms, kind, n_rot=1, seed=seed)
    rng = np.random.default_rng(seed + 1)
    if n_pos <= len(P):
        rows = rng.permutation(len(P))[:n_pos]
        return np.ascontiguousarray(P[rows]), None if arm_ids is None else np.ascontiguousarray(arm_ids[rows])
    ids = rng.integers(0, 2, size=n_pos).astype(np.uint8) if kind == "mixed" else np.full(n_pos, int(kind == "l"), dtype=np.uint8)
    s = np.stack([arms[int(a)].field("shoulder_position") for a in (0, 1)])[ids]
    P = s + rng.uniform([-0.1, -0.5, -0.5], [0.7, 0.5, 0.5], size=(n_pos, 3))
    return np.ascontiguousarray(P), ids if kind == "mixed" else None


def to_map(res):
    """The wrapper's tensors as the ABI's types: count / state_count uint32, mask uint64."""
    out = {}
    for key, v in res.items():
        a = v.cpu().numpy()
        out[key] = a.view(np.uint32) if key in ("count", "state_count") else a.view(np.uint64) if key == "mask" else a
    return out


def solve_tiled(solver, P, kind, arm_ids, E, torch):
    """The reference the entry point is defined against: rsik_solve under RSIK_THETA_NONE on the tiled poses, reduced with NumPy
    (math.fsum per position for the measure)."""
    pos, eul, arm = tile(P, arm_ids if kind == "mixed" else int(kind == "l"), E)
    kw = arm_kwargs(kind, arm, torch)
    res = solver.solve(soa(pos, eul, torch), theta_policy=abi().THETA_NONE, **kw)
    ref = reduce_map(res["reachable"].cpu().numpy(), res["state"].cpu().numpy(), res["interval"].cpu().numpy(), len(P), len(E))
    assert np.isnan(res["interval"].cpu().numpy()[res["reachable"].cpu().numpy() == 0]).all()
    return ref


def check_map(got, ref, n_rot, what, per_pose_tol=0.0):
    np.testing.assert_array_equal(got["count"], ref["count"], err_msg=what + " count")
    np.testing.assert_array_equal(got["state_count"], ref["state_count"], err_msg=what + " state_count")
    np.testing.assert_array_equal(got["mask"], ref["mask"], err_msg=what + " mask")
    assert (got["state_count"].sum(axis=1) == n_rot).all(), what
    err = np.abs(got["theta_measure"] - ref["theta_measure"])
    bound = rounding_bound(n_rot) + per_pose_tol * ref["count"]
    worst = int(np.argmax(err - bound)) if len(err) else 0
    print(f"{what}: measure max err {err.max(initial=0.0):.3e} (bound at that row {bound[worst] if len(err) else 0.0:.3e}), "
          f"reachable share {ref['count'].sum() / max(1, n_rot * len(ref['count'])):.3f}")
    assert np.isfinite(got["theta_measure"]).all(), what
    assert (err <= bound).all(), (what, float(err[worst]), float(bound[worst]))
    assert (got["theta_measure"][ref["count"] == 0] == 0.0).all(), what


def with_options(solver):
    _abi = abi()
    for no_mirror, no_tipz in itertools.product((0, 1), (0, 1)):
        solver.set_option(_abi.OPT_NO_MIRROR, no_mirror)
        solver.set_option(_abi.OPT_NO_TIPZ, no_tipz)
        yield f"no_mirror {no_mirror} no_tipz {no_tipz}"
    solver.set_option(_abi.OPT_NO_MIRROR, 0)
    solver.set_option(_abi.OPT_NO_TIPZ, 0)


def raw_map(solver, n_pos, p, n_rot, e, arm=None, arm_uniform=0, count=None, state_count=None, theta_measure=None, mask=None,
            null_col=None):
    """rsik_reach_map on the caller's own buffers: returns the ABI's code.  p / e: [3, n] tensors or None for a NULL table;
    null_col = ("pos" | "eul", k): that column pointer NULL."""
    def table(t, name):
        if t is None:
            return None
        ptrs = [t[k].data_ptr() for k in range(3)]
        if null_col is not None and null_col[0] == name:
            ptrs[null_col[1]] = None
        return (C.c_void_p * 3)(*ptrs)

    return raw_call(solver, "rsik_reach_map", n_pos, table(p, "pos"), ptr(arm), int(arm_uniform), int(n_rot), table(e, "eul"), ptr(count),
                    ptr(state_count), ptr(theta_measure), ptr(mask))


# ------------------------------------------------------------------------------------------ 1. against the library's own rsik_solve
@pytest.mark.parametrize("kind", KINDS)
def test_map_is_rsik_solve_reduced(torch_mod, orc, kind):
    """n_rot in {1, 63, 64, 65, 130} x n_pos in {1, 2, 3, 5, 729} (3 and 5: one below and one above the 4 positions of a workgroup
    that gives a wave one position), and 5 positions x 4096 orientations (four LDS tiles), under both values of RSIK_OPT_NO_MIRROR
    and of RSIK_OPT_NO_TIPZ: count, state_count and mask equal rsik_solve's reduced; theta_measure within n_rot^2 * 2 pi * 2^-53 of
    the fsum of the widths of rsik_solve's own intervals."""
    torch = torch_mod
    solver, _, _ = default_solver()
    shapes = [(n_pos, n_rot) for n_rot in (1, 63, 64, 65, 130) for n_pos in (1, 2, WAVES_PER_BLOCK - 1, WAVES_PER_BLOCK + 1, 729)]
    shapes.append((5, 4096))
    for n_pos, n_rot in shapes:
        P, arm_ids = positions(orc, kind, n_pos, seed=7 + n_pos)
        E = map_orientations(n_rot, 7)
        ref = solve_tiled(solver, P, kind, arm_ids, E, torch)
        if n_pos == 729 and n_rot == 130:
            assert ((ref["count"] > 0) & (ref["count"] < n_rot)).sum() >= 243
        for opts in with_options(solver):
            got = to_map(solver.reach_map(T(P.T, torch), T(E.T, torch), **arm_kwargs(kind, arm_ids, torch)))
            assert got["mask"].shape == (n_pos, (n_rot + 63) // 64) and got["state_count"].shape == (n_pos, N_STATES)
            check_map(got, ref, n_rot, f"{kind} {n_pos} x {n_rot} {opts}")


@pytest.mark.parametrize("kind", KINDS)
def test_more_positions_per_wave(torch_mod, orc, kind):
    """The host gives a wave q = 2, 4, 8, 16 positions from 8 workgroups of 4 q positions per compute unit on (reach_map_pos_per_wave):
    n_pos a few past each threshold, not a multiple of the positions per workgroup, so the last workgroup has waves with some and waves
    with no positions.  n_rot = 65 (a full chunk and a ragged one) for q = 2 and 4, n_rot = 3 for q = 8 and 16, where the tiled
    reference would otherwise run to 8 M poses.  Same comparison as above."""
    torch = torch_mod
    solver, _, _ = default_solver()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for ppw, extra, n_rot in ((2, 3, 65), (4, 7, 65), (8, 5, 3), (16, 9, 3)):
        E = map_orientations(n_rot, 7)
        n_pos = cus * 8 * WAVES_PER_BLOCK * ppw + extra
        P, arm_ids = positions(orc, kind, n_pos, seed=70 + ppw)
        ref = solve_tiled(solver, P, kind, arm_ids, E, torch)
        got = to_map(solver.reach_map(T(P.T, torch), T(E.T, torch), **arm_kwargs(kind, arm_ids, torch)))
        check_map(got, ref, n_rot, f"{kind} {n_pos} x {n_rot} ({ppw} positions per wave)")


# ------------------------------------------------------------------------------------------ 2. against the checker
@pytest.mark.parametrize("pair", ["default/default", "custom/custom", "custom/default", "default/ztip"])
def test_map_against_the_checker(torch_mod, orc, pair):
    """729 x 130 with a random arm byte per position: integers and mask are the checker's exactly; the measure is within
    2 * TOL * count[i] (TOL = 1e-9 per interval end) plus the rounding bound."""
    torch = torch_mod
    if pair == "default/default":
        arms, solver = default_arms(), default_solver()[0]
    else:
        arms, solver = checker_arms(pair), upload(pair)
    P, arm_ids, E = map_case(arms, "mixed")
    ref = expected_map(orc, arms, P, arm_ids, E, nthreads=4)
    assert ((ref["count"] > 0) & (ref["count"] < 130)).sum() >= 243
    got = to_map(solver.reach_map(T(P.T, torch), T(E.T, torch), arm=T(arm_ids, torch)))
    check_map(got, ref, 130, f"{pair} 729 x 130 against the checker", per_pose_tol=2 * TOL)


# ------------------------------------------------------------------------------------------ 3. optional outputs
def test_optional_outputs_and_guards(torch_mod, orc):
    """Each output alone and every pair of outputs give the same bits as all four together; all four NULL is RSIK_E_INVALID; the
    guard bytes around each buffer are untouched; the padding bits of the last mask word are 0."""
    torch = torch_mod
    _abi = abi()
    solver, _, _ = default_solver()
    n_pos, n_rot, guard = 729, 130, 256
    P, arm_ids, E = map_case(default_arms(), "mixed")
    p, e, arm = T(P.T, torch), T(E.T, torch), T(arm_ids, torch)
    words = (n_rot + 63) // 64
    sizes = {"count": 4 * n_pos, "state_count": 4 * n_pos * N_STATES, "theta_measure": 8 * n_pos, "mask": 8 * n_pos * words}

    def launch(names):
        bufs = {k: torch.full((guard + sizes[k] + guard,), 0xA5, dtype=torch.uint8, device="cuda") for k in names}
        rc = raw_map(solver, n_pos, p, n_rot, e, arm=arm, **{k: bufs[k][guard:guard + sizes[k]] for k in names})
        torch.cuda.synchronize()
        out = {}
        for k, b in bufs.items():
            b = b.cpu().numpy()
            assert (b[:guard] == 0xA5).all() and (b[guard + sizes[k]:] == 0xA5).all(), (names, k, "guard bytes written")
            out[k] = b[guard:guard + sizes[k]].copy()
        return rc, out

    rc, full = launch(OUTPUTS)
    assert rc == _abi.RSIK_OK, last_error(solver)
    mask = full["mask"].view(np.uint64).reshape(n_pos, words)
    assert mask.any() and (mask[:, -1] >> np.uint64(n_rot % 64) == 0).all()
    assert np.array_equal(mask, pack_mask(solve_tiled(solver, P, "mixed", arm_ids, E, torch)["reachable"]))
    for r in (1, 2):
        for names in itertools.combinations(OUTPUTS, r):
            rc, part = launch(names)
            assert rc == _abi.RSIK_OK, (names, last_error(solver))
            for k in names:
                assert np.array_equal(part[k], full[k]), (names, k)
    rc, _ = launch(())
    assert rc == _abi.RSIK_E_INVALID and "all NULL" in last_error(solver)


# ------------------------------------------------------------------------------------------ 4. not numbers, and far inputs
def test_rows_that_are_not_numbers(torch_mod, orc):
    """A NaN or an infinity in one position fills that position's RSIK_STATE_INVALID_INPUT bin with n_rot (count 0, measure 0.0,
    mask 0); in one orientation it moves that one pose of every position to the bin.  Every other output has the bits of a run in
    which the bad value was an ordinary one."""
    torch = torch_mod
    INVALID = abi().STATE_INVALID_INPUT
    solver, _, _ = default_solver()
    P, arm_ids, E = map_case(default_arms(), "mixed")
    n_pos, n_rot = len(P), len(E)
    arm = T(arm_ids, torch)
    clean = to_map(solver.reach_map(T(P.T, torch), T(E.T, torch), arm=arm))
    assert clean["state_count"][:, INVALID].sum() == 0
    rows = np.flatnonzero((clean["count"] > 0) & (clean["count"] < n_rot))
    for q, (bad, col) in enumerate(((np.nan, 0), (np.inf, 1), (-np.inf, 2), (np.nan, 2))):
        i = int(rows[11 * q + 3])
        Pb = P.copy()
        Pb[i, col] = bad
        got = to_map(solver.reach_map(T(Pb.T, torch), T(E.T, torch), arm=arm))
        assert got["count"][i] == 0 and got["theta_measure"][i] == 0.0 and not got["mask"][i].any(), (bad, col)
        assert got["state_count"][i, INVALID] == n_rot and got["state_count"][i].sum() == n_rot, (bad, col)
        others = np.arange(n_pos) != i
        for key in OUTPUTS:
            a, b = got[key][others], clean[key][others]
            assert np.array_equal(a.view(np.uint64) if key == "theta_measure" else a, b.view(np.uint64) if key == "theta_measure" else b), (bad, col, key)
    for q, (bad, col) in enumerate(((np.nan, 0), (np.inf, 1), (-np.inf, 2))):
        j = (5, 64, 129)[q]  # first chunk, first lane of the second, last lane of the ragged one
        Eb = E.copy()
        Eb[j, col] = bad
        got = to_map(solver.reach_map(T(P.T, torch), T(Eb.T, torch), arm=arm))
        # the reference for everything else: the same map without orientation j, from rsik_solve's rows
        ref = solve_tiled(solver, P, "mixed", arm_ids, E, torch)
        ok, st, w = ref["reachable"].copy(), ref["state"].copy(), ref["width"].copy()
        ok[:, j], st[:, j], w[:, j] = False, INVALID, 0.0
        np.testing.assert_array_equal(got["count"], ok.sum(axis=1))
        np.testing.assert_array_equal(got["mask"], pack_mask(ok))
        np.testing.assert_array_equal(got["state_count"], np.stack([(st == c).sum(axis=1) for c in range(N_STATES)], axis=1))
        assert (got["state_count"][:, INVALID] == 1).all()
        want = np.array([math.fsum(r) for r in w])
        assert (np.abs(got["theta_measure"] - want) <= rounding_bound(n_rot)).all(), (bad, col)
        # positions whose pose j was not reachable anyway lose nothing: their measure keeps its bits
        same = ~ref["reachable"][:, j]
        same_bits(got["theta_measure"][same], clean["theta_measure"][same], f"orientation {j} {bad}")


def test_far_inputs_are_answered_as_rsik_solve_answers_them(torch_mod, orc):
    """An orientation of 2^27 + 1.5 rad (reduced by the far-angle branch) and a position at 1e200 (its squared distance overflows)
    are answered as their rsik_solve rows."""
    torch = torch_mod
    solver, _, _ = default_solver()
    P, arm_ids, E = map_case(default_arms(), "mixed")
    P, arm_ids = P[200:264].copy(), arm_ids[200:264].copy()
    E = E.copy()
    E[3, 0] = 2.0 ** 27 + 1.5
    E[70, 2] = -(2.0 ** 27 + 1.5)
    E[129, 1] = 1e300
    P[5] = [1e200, 0.0, 0.0]
    P[6, 2] = -1e200
    ref = solve_tiled(solver, P, "mixed", arm_ids, E, torch)
    assert ref["reachable"][:, [3, 70, 129]].any(), "a far orientation must be reachable somewhere for the comparison to bite"
    got = to_map(solver.reach_map(T(P.T, torch), T(E.T, torch), arm=T(arm_ids, torch)))
    check_map(got, ref, len(E), "far inputs")
    assert got["count"][5] == 0 and got["count"][6] == 0 and got["state_count"][5, abi().STATE_INVALID_INPUT] == 0


# ------------------------------------------------------------------------------------------ 5. reproducible
def test_measure_is_reproducible_and_nothing_accumulates(torch_mod, orc):
    """Two launches on the same inputs give the same bits in theta_measure; a launch into buffers pre-filled with 0xFF gives the
    same result: nothing accumulates into the caller's memory.  n_rot = 2500: three LDS tiles, the totals carried between them."""
    torch = torch_mod
    solver, _, _ = default_solver()
    P, arm_ids, _ = map_case(default_arms(), "mixed")
    for n_rot in (130, 2500):
        E = map_orientations(n_rot, 7)
        p, e, arm = T(P.T, torch), T(E.T, torch), T(arm_ids, torch)
        a = to_map(solver.reach_map(p, e, arm=arm))
        b = to_map(solver.reach_map(p, e, arm=arm))
        words = (n_rot + 63) // 64
        out = {"count": torch.full((729,), -1, dtype=torch.int32, device="cuda"),
               "state_count": torch.full((729, N_STATES), -1, dtype=torch.int32, device="cuda"),
               "theta_measure": torch.full((729,), -1, dtype=torch.int64, device="cuda").view(torch.float64),
               "mask": torch.full((729, words), -1, dtype=torch.int64, device="cuda")}
        c = to_map(solver.reach_map(p, e, arm=arm, out=out))
        assert a["count"].sum() > 0
        for key in OUTPUTS:
            for other in (b, c):
                if key == "theta_measure":
                    same_bits(other[key], a[key], f"{n_rot} {key}")
                else:
                    np.testing.assert_array_equal(other[key], a[key], err_msg=f"{n_rot} {key}")


# ------------------------------------------------------------------------------------------ 6. argument checks
def test_argument_checks(torch_mod, orc):
    torch = torch_mod
    _abi = abi()
    from reachy2_symbolic_ik_amd import HipSolver

    solver, r, _ = default_solver()
    P, arm_ids, E = map_case(default_arms(), "mixed")
    p, e, arm = T(P.T, torch), T(E.T, torch), T(arm_ids, torch)
    sentinel = 0x5A5A5A5A
    count = torch.full((729,), sentinel, dtype=torch.int32, device="cuda")
    big = T(map_orientations(4097, 1).T, torch)
    assert raw_map(solver, 729, p, 0, e, arm=arm, count=count) == _abi.RSIK_E_INVALID and "n_rot" in last_error(solver)
    assert raw_map(solver, 729, p, 4097, big, arm=arm, count=count) == _abi.RSIK_E_INVALID and "n_rot" in last_error(solver)
    assert raw_map(solver, -1, p, 130, e, arm=arm, count=count) == _abi.RSIK_E_INVALID
    assert raw_map(solver, 729, None, 130, e, arm=arm, count=count) == _abi.RSIK_E_INVALID and "pos_soa is NULL" in last_error(solver)
    assert raw_map(solver, 729, p, 130, None, arm=arm, count=count) == _abi.RSIK_E_INVALID and "euler_soa is NULL" in last_error(solver)
    for k in range(3):
        assert raw_map(solver, 729, p, 130, e, arm=arm, count=count, null_col=("pos", k)) == _abi.RSIK_E_INVALID
        assert "a pos_soa column is NULL" in last_error(solver)
        assert raw_map(solver, 729, p, 130, e, arm=arm, count=count, null_col=("eul", k)) == _abi.RSIK_E_INVALID
        assert "a euler_soa column is NULL" in last_error(solver)
    assert raw_map(solver, 729, p, 130, e, arm=None, arm_uniform=2, count=count) == _abi.RSIK_E_INVALID
    assert raw_map(solver, 729, p, 130, e, arm=arm) == _abi.RSIK_E_INVALID
    # n_pos == 0: RSIK_OK, nothing written (NULL tables are fine then)
    assert raw_map(solver, 0, None, 130, None, arm=arm, count=count) == _abi.RSIK_OK, last_error(solver)
    assert raw_map(solver, 0, p, 130, e, count=count) == _abi.RSIK_OK
    torch.cuda.synchronize()
    assert (count.cpu().numpy() == sentinel).all()
    # a missing arm
    lone = HipSolver(0)
    lone.set_arm(0, solver._arm_blocks[0])
    assert raw_map(lone, 729, p, 130, e, arm=None, arm_uniform=1, count=count) == _abi.RSIK_E_NOT_SET
    assert raw_map(lone, 729, p, 130, e, arm=arm, count=count) == _abi.RSIK_E_NOT_SET
    assert raw_map(lone, 729, p, 130, e, arm=None, arm_uniform=0, count=count) == _abi.RSIK_OK, last_error(lone)
    torch.cuda.synchronize()
    assert (count.cpu().numpy() != sentinel).all()
    with pytest.raises(ValueError):
        solver.reach_map(p, big)
    with pytest.raises(ValueError):
        solver.reach_map(p, e, want=())


# ------------------------------------------------------------------------------------------ 7. the Python surface
def test_python_surface(torch_mod, orc):
    """SymbolicIK.reach_map_batch and DualArmIK.reach_map_batch equal the raw call; unpack_reach_mask equals rsik_solve's reachable
    column reshaped; a planned launch re-issues the same map."""
    torch = torch_mod
    import contextlib
    import io

    from reachy2_symbolic_ik_amd import DualArmIK
    from reachy2_symbolic_ik_amd.symbolic_ik import unpack_reach_mask

    solver, r, l = default_solver()
    arms = default_arms()
    for kind, ik in (("r", r), ("l", l)):
        P, _, E = map_case(arms, kind)
        raw = to_map(solver.reach_map(T(P.T, torch), T(E.T, torch), arm_uniform=int(kind == "l")))
        for positions_in, orientations_in in ((P, E), (T(P.T, torch), T(E.T, torch))):  # rows on the host, SoA on the device
            got = ik.reach_map_batch(positions_in, orientations_in)
            ref = solve_tiled(solver, P, kind, None, E, torch)
            assert np.array_equal(unpack_reach_mask(got["mask"], len(E)).cpu().numpy(), ref["reachable"])
            got = to_map(got)
            for key in OUTPUTS:
                assert np.array_equal(got[key].view(np.uint64) if key == "theta_measure" else got[key],
                                      raw[key].view(np.uint64) if key == "theta_measure" else raw[key]), (kind, key)
        only = ik.reach_map_batch(P, E, want=("count",))
        assert set(only) == {"count"} and np.array_equal(only["count"].cpu().numpy().view(np.uint32), raw["count"])
    P, arm_ids, E = map_case(arms, "mixed")
    with contextlib.redirect_stdout(io.StringIO()):
        dual = DualArmIK(device=0)
    raw = to_map(dual.solver.reach_map(T(P.T, torch), T(E.T, torch), arm=T(arm_ids, torch)))
    got = dual.reach_map_batch(arm_ids, P, E)
    ref = solve_tiled(dual.solver, P, "mixed", arm_ids, E, torch)
    assert np.array_equal(unpack_reach_mask(got["mask"], len(E)).cpu().numpy(), ref["reachable"])
    check_map(to_map(got), ref, len(E), "DualArmIK.reach_map_batch")
    for key in OUTPUTS:
        assert np.array_equal(to_map(got)[key].view(np.uint64) if key == "theta_measure" else to_map(got)[key],
                              raw[key].view(np.uint64) if key == "theta_measure" else raw[key]), key
    planned = dual.reach_map_batch(arm_ids, P, E, plan_only=True)
    planned["launch"]()
    torch.cuda.synchronize()
    assert np.array_equal(planned["count"].cpu().numpy().view(np.uint32), raw["count"])
