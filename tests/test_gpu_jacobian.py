"""GPU tests (-m gpu, MI355X) of rsik_jacobian (csrc/rsik_kernel_jacobian.hpp): the 6 x 7 Jacobian of the goal frame, its signed
maximal minors and the manipulability, against the NumPy reference of tests/jacobian_workload.py (pinned on the CPU alone by
tests/test_jacobian_abi.py), against central differences of the device's own rsik_forward_kinematics, and against the solve.

Shapes: n in {1, 63, 64, 65, kBlock - 1, kBlock, kBlock + 1} (one wave short, full, one over; the same for a workgroup), n_rep in
{1, 3}, arms uniform r, uniform l and a byte per row, on the pairs default/default, custom/custom (the tip has x / y components) and
default/ztip (two arms that are no mirror images).

Tolerances.  J against the reference: 1e-13 absolute (device FK is held to 1e-14; an entry is one cross product of such numbers, each
<= 1).  A minor is multilinear in 36 such entries with cofactors bounded by Hadamard at (1 + L^2)^(5/2), L = u + f + |tip|:
tol = 36 (1 + L^2)^(5/2) 1e-13 (jacobian_workload.minor_tol, about 9e-12), absolute, for the null vector, the manipulability and
J . null.  The solver link's two bounds are measured with the CPU checker (jacobian_workload.LINK_*)."""
import contextlib
import functools
import io
import itertools
import math

import numpy as np
import pytest

import arm_pairs
import far_inputs as FI
import jacobian_workload as JW
from compare import bits
from gpu_support import T, abi, arm_kwargs, last_error, ptr, raw_call, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

KBLOCK = 256  # RSIK_BLOCK (csrc/rsik_tables.hpp)
SIZES = (1, 63, 64, 65, KBLOCK - 1, KBLOCK, KBLOCK + 1)
REPS = (1, 3)
OUTS = ("jacobian", "null_vector", "manipulability")
SUBSETS = [c for r in (1, 2) for c in itertools.combinations(OUTS, r)]
J_TOL = 1e-13


_SOLVERS = {}


def solver_of(pair):
    """The pair's solver, uploaded once for this module (the fixture below closes it when the module is done)."""
    if pair not in _SOLVERS:
        _SOLVERS[pair] = arm_pairs.upload(pair, **({"check": lambda p, b: None} if pair == "default/default" else {}))
    return _SOLVERS[pair]


@pytest.fixture(scope="module", autouse=True)
def _solvers_do_not_outlive_the_module(torch_mod):
    """Nothing of these tests stays behind for the files that run after them: the contexts are destroyed, torch's cached blocks freed."""
    yield
    torch_mod.cuda.synchronize()
    while _SOLVERS:
        _SOLVERS.popitem()[1].close()
    torch_mod.cuda.empty_cache()


def kind_arm(kind, n):
    return {"r": np.zeros(n, dtype=np.uint8), "l": np.ones(n, dtype=np.uint8), "mixed": JW.arm_bytes()[:n]}[kind]


def run(torch, pair, q, kind, want=OUTS, arm=None):
    """One launch through HipSolver.jacobian on joints [n,7] or [n_rep,n,7]; the results on the host."""
    n = q.shape[-2]
    arm = kind_arm(kind, n) if arm is None else arm
    res = solver_of(pair).jacobian(T(q, torch), want=want, **arm_kwargs(kind, arm, torch))
    torch.cuda.synchronize()
    assert tuple(res) == tuple(o for o in OUTS if o in want)
    return {k: v.cpu().numpy() for k, v in res.items()}


def same(a, b, what):
    for k in b:
        assert a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def check_values(got, ref, tol, what, rows=None):
    """The three outputs against the reference and against each other."""
    J, null, w = got["jacobian"], got["null_vector"], got["manipulability"]
    assert np.isfinite(J).all() and np.isfinite(null).all() and np.isfinite(w).all(), what
    eJ = float(np.abs(J - ref["jacobian"]).max())
    eN = float(np.abs(null - ref["null_vector"]).max())
    eW = float(np.abs(w - ref["manipulability"]).max())
    exact = np.sqrt((null.astype(np.longdouble) ** 2).sum(axis=-1)).astype(np.float64)
    pos = exact > 0
    eU = float(ulps(w[pos], exact[pos]).max()) if pos.any() else 0.0
    eR = float(np.abs(np.einsum("...ij,...j->...i", J, null)).max())
    print(f"{what}: J {eJ:.2e}, null {eN:.2e}, manipulability {eW:.2e} (tol {tol:.2e}), against |null| {eU:.2f} ulp, |J . null| {eR:.2e}")
    assert eJ <= J_TOL, (what, eJ)
    assert eN <= tol and eW <= tol and eR <= tol, (what, eN, eW, eR, tol)
    assert eU <= 4.0 and (w[~pos] == 0.0).all(), (what, eU)
    return eJ, eN, eW


# ------------------------------------------------------------------------------------------ layout, equivalence and values per shape
@pytest.mark.parametrize("pair", JW.PAIRS)
def test_every_shape_values_and_bits(torch_mod, pair):
    """For every n, n_rep and arm arrangement: the values against the reference; every subset of the outputs, a second launch, the
    flat call on the tiled rows and (arm byte per row) the two uniform launches row by row: all bit for bit."""
    torch = torch_mod
    blocks = JW.blocks_of(pair)
    tol = JW.minor_tol(blocks)
    uniform = JW.joint_set("uniform")
    for n, n_rep in itertools.product(SIZES, REPS):
        q = np.ascontiguousarray(uniform[: n * n_rep].reshape((n_rep, n, 7) if n_rep > 1 else (n, 7)))
        full = {}
        for kind in ("r", "l", "mixed"):
            what = f"{pair} n={n} n_rep={n_rep} {kind}"
            arm = kind_arm(kind, n)
            got = full[kind] = run(torch, pair, q, kind)
            assert got["jacobian"].shape == q.shape[:-1] + (6, 7) and got["manipulability"].shape == q.shape[:-1], what
            check_values(got, JW.reference(blocks, q, arm), tol, what)
            same(run(torch, pair, q, kind), got, what + " twice")
            for sub in SUBSETS:
                same(got, run(torch, pair, q, kind, want=sub), what + f" want={sub}")
            if n_rep > 1:
                flat = run(torch, pair, q.reshape(-1, 7), kind, arm=np.tile(arm, n_rep))
                same({k: v.reshape(flat[k].shape) for k, v in got.items()}, flat, what + " against the flat call")
        rows = kind_arm("mixed", n) == 1
        for k in OUTS:
            is_l = rows.reshape((n,) + (1,) * (full["r"][k].ndim - q.ndim + 1))  # (broadcasts over the repetitions)
            want = np.where(is_l, full["l"][k], full["r"][k])
            assert np.array_equal(bits(full["mixed"][k]), bits(want)), (pair, n, n_rep, k, "arm byte per row against the uniform launches")


def test_refusals(torch_mod):
    """All three outputs NULL, n < 0, n_rep < 1 and joints == NULL are RSIK_E_INVALID with the function's name in rsik_last_error;
    n == 0 launches nothing; an arm whose constants were not uploaded is RSIK_E_NOT_SET, as in rsik_forward_kinematics."""
    from reachy2_symbolic_ik_amd import HipSolver

    torch, A = torch_mod, abi()
    solver = solver_of("default/default")
    q = T(JW.joint_set("uniform")[:8], torch)
    o = torch.empty((8,), dtype=torch.float64, device="cuda")
    arm = T(JW.arm_bytes()[:8], torch)
    for what, args in (("all outputs NULL", (8, 1, ptr(q), None, 0, None, None, None)), ("n < 0", (-1, 1, ptr(q), None, 0, None, None, ptr(o))),
                       ("n_rep < 1", (8, 0, ptr(q), None, 0, None, None, ptr(o))), ("joints NULL", (8, 1, None, None, 0, None, None, ptr(o))),
                       ("arm_uniform 2", (8, 1, ptr(q), None, 2, None, None, ptr(o)))):
        assert raw_call(solver, "rsik_jacobian", *args) == A.RSIK_E_INVALID, what
        assert "rsik_jacobian" in last_error(solver), (what, last_error(solver))
    assert raw_call(solver, "rsik_jacobian", 0, 1, None, None, 0, None, None, None) == A.RSIK_OK
    assert raw_call(solver, "rsik_jacobian", 8, 1, ptr(q), ptr(arm), 0, None, None, ptr(o)) == A.RSIK_OK
    bare = HipSolver(0)
    assert raw_call(bare, "rsik_jacobian", 8, 1, ptr(q), None, 0, None, None, ptr(o)) == A.RSIK_E_NOT_SET
    assert raw_call(bare, "rsik_jacobian", 8, 1, ptr(q), ptr(arm), 0, None, None, ptr(o)) == A.RSIK_E_NOT_SET
    p = torch.empty((8, 3), dtype=torch.float64, device="cuda")
    assert raw_call(bare, "rsik_forward_kinematics", 8, ptr(q), None, 0, ptr(p), None) == A.RSIK_E_NOT_SET
    torch.cuda.synchronize()
    bare.close()


def test_more_repetitions_than_one_grid_holds(torch_mod):
    """n_rep = 65537: the repetition is the grid's y, which holds 65535, so the host issues two launches, each on its slice.  Against
    the flat call, bit for bit."""
    torch = torch_mod
    q = np.ascontiguousarray(np.resize(JW.joint_set("uniform"), (65537, 1, 7)))
    got = run(torch, "default/default", q, "r", arm=np.zeros(1, dtype=np.uint8))
    flat = run(torch, "default/default", q.reshape(-1, 7), "r")
    same({k: v.reshape(flat[k].shape) for k, v in got.items()}, flat, "n_rep = 65537")


def test_python_surface(torch_mod):
    """SymbolicIK.jacobian_batch and DualArmIK.jacobian_batch are HipSolver.jacobian on their arms; out= buffers are written in
    place; a planned launch writes the same bits."""
    from reachy2_symbolic_ik_amd import DualArmIK, SymbolicIK

    torch = torch_mod
    solver = solver_of("default/default")
    q = np.ascontiguousarray(JW.joint_set("uniform")[:390].reshape(3, 130, 7))
    arm = JW.arm_bytes()[:130]
    with contextlib.redirect_stdout(io.StringIO()):
        ik_l = SymbolicIK("l_arm", solver=solver, **arm_pairs.DEFAULT)
        dual = DualArmIK(solver=solver, **arm_pairs.DEFAULT)
    got = {k: v.cpu().numpy() for k, v in ik_l.jacobian_batch(q).items()}
    same(got, run(torch, "default/default", q, "l"), "SymbolicIK.jacobian_batch")
    got = {k: v.cpu().numpy() for k, v in dual.jacobian_batch(arm, q, want=("manipulability",)).items()}
    same(got, {"manipulability": run(torch, "default/default", q, "mixed")["manipulability"]}, "DualArmIK.jacobian_batch")
    out = {"null_vector": torch.full((3, 130, 7), 7.0, dtype=torch.float64, device="cuda")}
    res = solver.jacobian(T(q, torch), arm=T(arm, torch), want=("null_vector", "manipulability"), out=out)
    assert res["null_vector"] is out["null_vector"] and tuple(res) == ("null_vector", "manipulability")
    plan = solver.jacobian(T(q, torch), arm=T(arm, torch), want=("null_vector",), plan_only=True)
    plan["launch"]()
    torch.cuda.synchronize()
    assert np.array_equal(bits(plan["null_vector"].cpu().numpy()), bits(out["null_vector"].cpu().numpy()))
    with pytest.raises(ValueError):
        solver.jacobian(T(q, torch), want=())
    with pytest.raises(ValueError):
        solver.jacobian(T(q[..., :6], torch))


def test_integration_md_snippet(torch_mod):
    """The snippet of INTEGRATION.md as written: a sweep, the manipulability of its joints in place, the argmax over the samples."""
    from reachy2_symbolic_ik_amd import SymbolicIK

    torch = torch_mod
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", solver=solver_of("default/default"), **arm_pairs.DEFAULT)
    pos, eul, arm, _ = JW.link_poses()
    poses = np.stack([pos[arm == 0], eul[arm == 0]], axis=1)  # [n,2,3]
    sweep = ik.sweep_batch(poses, n_theta=16)
    w = ik.jacobian_batch(sweep["joints"], want=("manipulability",))["manipulability"]
    best = torch.nan_to_num(w, nan=-1.0).argmax(dim=0)
    q = sweep["joints"][best, torch.arange(w.shape[1], device=w.device)]
    assert tuple(w.shape) == (16, len(poses)) and tuple(q.shape) == (len(poses), 7) and bool(torch.isfinite(q).all())
    again = ik.jacobian_batch(q)["manipulability"]
    assert torch.equal(again, w.max(dim=0).values)


# ------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("pair", JW.PAIRS)
def test_jacobian_is_the_derivative_of_the_device_fk(torch_mod, pair):
    """Central differences of the device's own rsik_forward_kinematics at h = 1e-6, the angular rows from (R+ - R-) / (2 h) . R^T:
    1e-8.  This settles every sign."""
    torch = torch_mod
    solver = solver_of(pair)
    q, arm = JW.joint_set("uniform")[:512], JW.arm_bytes()[:512]
    arm_t = T(arm, torch)

    def device_fk(x):
        p, R = solver.forward_kinematics(T(x, torch), arm=arm_t)
        return p.cpu().numpy(), R.cpu().numpy()

    J = run(torch, pair, q, "mixed", want=("jacobian",))["jacobian"]
    err = float(np.abs(J - JW.fd_jacobian(device_fk, q)).max())
    print(f"{pair}: J against central differences of rsik_forward_kinematics {err:.3e}")
    assert err <= 1e-8, (pair, err)


@pytest.mark.parametrize("pair", JW.PAIRS)
def test_named_sets_against_the_reference(torch_mod, pair):
    """The golden joints of the reference's solve like the uniform set.  The singular set (a straight elbow): every output finite,
    manipulability <= tol.  The near-singular set: manipulability within tol of the reference's, absolutely.  The wound set (whole
    turns up to +-6 pi): within 1e-13 + tol of the unwound rows' outputs."""
    torch = torch_mod
    blocks = JW.blocks_of(pair)
    tol = JW.minor_tol(blocks)
    arm = JW.arm_bytes()
    gq, ga = JW.golden_joints()
    check_values(run(torch, pair, gq, "mixed", arm=ga), JW.reference(blocks, gq, ga), tol, f"{pair} golden joints")
    got = run(torch, pair, JW.joint_set("singular"), "mixed")
    check_values(got, JW.reference(blocks, JW.joint_set("singular"), arm), tol, f"{pair} singular set")
    print(f"{pair}: singular set manipulability <= {got['manipulability'].max():.3e}")
    assert got["manipulability"].max() <= tol
    got = run(torch, pair, JW.joint_set("near_singular"), "mixed")
    ref = JW.reference(blocks, JW.joint_set("near_singular"), arm)
    check_values(got, ref, tol, f"{pair} near-singular set")
    assert np.abs(got["manipulability"] - ref["manipulability"]).max() <= tol and ref["manipulability"].max() < 1e-3
    wound, plain = run(torch, pair, JW.joint_set("wound"), "mixed"), run(torch, pair, JW.joint_set("uniform"), "mixed")
    for k in OUTS:
        err = float(np.abs(wound[k] - plain[k]).max())
        print(f"{pair}: wound set against the unwound rows, {k}: {err:.3e}")
        assert err <= 1e-13 + tol, (pair, k, err)
    check_values(wound, JW.reference(blocks, JW.joint_set("uniform"), arm), tol + 1e-13, f"{pair} wound set")


# ------------------------------------------------------------------------------------------ rows that are not numbers, far angles
@pytest.mark.parametrize("kind", ["r", "mixed"])
def test_rows_that_are_not_numbers(torch_mod, kind):
    """A NaN, a +inf and a -inf in single rows — the first row, both sides of a wave boundary, the last row; in the first and in the
    last repetition — make those rows NaN in every output; every other row carries the bits of the run with ordinary values there."""
    torch = torch_mod
    n, n_rep = 129, 3
    q = np.ascontiguousarray(JW.joint_set("uniform")[: n * n_rep].reshape(n_rep, n, 7))
    base = run(torch, "default/default", q, kind)
    for subset in (OUTS, ("manipulability",), ("jacobian",)):
        bad = q.copy()
        spots = [(0, 0, 0, np.nan), (0, 63, 3, np.inf), (0, 64, 6, -np.inf), (0, 128, 5, np.nan), (2, 0, 1, -np.inf), (2, 63, 2, np.nan),
                 (2, 128, 4, np.inf)]
        for rep, row, k, v in spots:
            bad[rep, row, k] = v
        got = run(torch, "default/default", bad, kind, want=subset)
        hit = np.zeros((n_rep, n), dtype=bool)
        for rep, row, _, _ in spots:
            hit[rep, row] = True
        for k in subset:
            flat = got[k].reshape(n_rep, n, -1)
            assert np.isnan(flat[hit]).all(), (kind, k, "a row that is not numbers must be NaN in every entry")
            assert np.array_equal(bits(flat[~hit]), bits(base[k].reshape(n_rep, n, -1)[~hit])), (kind, k, "another row's bits changed")


@functools.lru_cache(maxsize=None)
def far_rows():
    """One joint of a uniform row at a rung of tests/far_inputs.py (2^27, 1e15: wound by whole turns; 1e300: the double itself), each
    joint and each sign in turn, and the reduced twin of every row."""
    base = JW.joint_set("uniform")
    far, twin = [], []
    for g, rung in enumerate((2.0 ** 27, 1e15, 1e300)):
        assert rung in FI.RUNGS
        for k in range(7):
            for s, sign in enumerate((1.0, -1.0)):
                row = base[(g * 7 + k) * 2 + s].copy()
                x = FI.wind(row[k], rung, sign) if rung < FI.WALKED_FROM else FI.walked(rung, sign, 0.0)[0][k]
                t = row.copy()
                row[k], t[k] = x, FI.reduce_angle(x)
                assert abs(x) >= rung / 2 and abs(t[k]) <= math.pi
                far.append(row); twin.append(t)
    return np.array(far), np.array(twin)


@pytest.mark.parametrize("pair", ["default/default", "custom/custom"])
def test_far_angles_are_answered_like_their_reduced_twins(torch_mod, pair):
    """One joint at 2^27, 1e15 and 1e300: the row's outputs equal its reduced twin's to 1e-9."""
    torch = torch_mod
    far, twin = far_rows()
    arm = JW.arm_bytes()[: len(far)]
    a, b = run(torch, pair, far, "mixed", arm=arm), run(torch, pair, twin, "mixed", arm=arm)
    for k in OUTS:
        err = float(np.abs(a[k] - b[k]).max())
        print(f"{pair}: far rows against their reduced twins, {k}: {err:.3e}")
        assert np.isfinite(a[k]).all() and err <= 1e-9, (pair, k, err)
    check_values(b, JW.reference(JW.blocks_of(pair), twin, arm), JW.minor_tol(JW.blocks_of(pair)), f"{pair} reduced twins")


# ------------------------------------------------------------------------------------------ the link to the solver
def test_null_vector_is_the_solve_s_self_motion(torch_mod):
    """Reachable rows of the golden pose set G3, both arms: rsik_solve_sweep (EXPLICIT) at theta - h, theta, theta + h, h = 1e-5, theta
    the middle of the row's interval.  Rows kept: not projected at either outer sample, |joints[3]| below the elbow limit at both,
    reference manipulability >= 1e-3 (at least half of the rows).  With dq = angle_diff(q+, q-) / 2h and J, null from rsik_jacobian
    at the middle sample:  max |J . dq| <= 5.8e-9  and  max 1 - |cos(null, dq)| <= 3.4e-15.
    Neither bound can be derived (q''' is unbounded toward singularities): each is 10 x what the CPU checker's get_joints and the NumPy
    reference give on the same poses — 5.78e-10 and 3.33e-16 over 298 kept rows of 512 (tests/test_jacobian_abi.py measures them
    again); the factor covers the device's joints, held to 1e-11 rad, divided by h.  The sign of null . dq/dtheta is negative on every
    kept row of both arms, as include/rsik.h says."""
    from reachy2_symbolic_ik_amd import constants as K

    torch = torch_mod
    solver = solver_of("default/default")
    blocks = JW.blocks_of("default/default")
    pos, eul, arm, theta = JW.link_poses()
    th = np.stack([theta - JW.LINK_H, theta, theta + JW.LINK_H])
    soa = torch.as_tensor(np.ascontiguousarray(np.concatenate([pos.T, eul.T], axis=0))).cuda()
    sw = solver.solve_sweep(soa, T(th, torch), policy="explicit", arm=T(arm, torch), want_elbow=False)
    assert bool(sw["reachable"].all())
    got = solver.jacobian(sw["joints"], arm=T(arm, torch))  # [3, n, 7]: the sweep's output judged in place
    torch.cuda.synchronize()
    q = sw["joints"].cpu().numpy()
    projected = sw["projected"].cpu().numpy()
    keep, dq, ref = JW.link_measure(blocks, q[0], q[2], q[1], projected[0] | projected[2], arm, [b[K.C_ELBOW_LIMIT] for b in blocks])
    J, null = got["jacobian"].cpu().numpy()[1], got["null_vector"].cpu().numpy()[1]
    jdq, cos, signs = JW.link_figures(J, null, dq, keep)
    print(f"solver link: kept {int(keep.sum())} of {len(keep)}, max |J . dq| {jdq:.3e} (bound {JW.LINK_JDQ_BOUND:.1e}), "
          f"max 1 - |cos(null, dq)| {cos:.3e} (bound {JW.LINK_COS_BOUND:.1e}), signs {sorted(set(signs.tolist()))}")
    assert keep.sum() * 2 >= len(keep)
    assert jdq <= JW.LINK_JDQ_BOUND, jdq
    assert cos <= JW.LINK_COS_BOUND, cos
    assert (signs == -1.0).all()
