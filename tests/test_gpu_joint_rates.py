"""GPU tests (-m gpu, MI355X) of rsik_joint_rates (csrc/rsik_kernel_joint_rates.hpp): damped least-squares joint rates from a twist,
against the NumPy reference and the derived per-row tolerance of tests/joint_rates_workload.py (pinned on the CPU alone by
tests/test_joint_rates_abi.py), against central differences of the device's own rsik_forward_kinematics, and against the solve.

Shapes: n in {1, 63, 64, 65, kBlock - 1, kBlock, kBlock + 1}, n_rep in {1, 3}, arms uniform r, uniform l and a byte per row, on the pairs
default/default, custom/custom and default/ztip.  A row's error is the 2-norm of (device - reference) over the row, held to tol_row
(rates) and tol_achieved (achieved_twist)."""
import contextlib
import io
import itertools

import numpy as np
import pytest

import arm_pairs
import jacobian_workload as JW
import joint_rates_workload as W
from compare import bits
from gpu_support import T, abi, arm_kwargs, last_error, ptr, raw_call, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

KBLOCK = 256  # RSIK_BLOCK (csrc/rsik_tables.hpp)
SIZES = (1, 63, 64, 65, KBLOCK - 1, KBLOCK, KBLOCK + 1)
REPS = (1, 3)
OUTS = ("rates", "achieved_twist")

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


def run(torch, pair, q, v, kind, damping, bias=None, want=OUTS, arm=None):
    """One launch through HipSolver.joint_rates on joints [n,7] or [n_rep,n,7]; damping a float or an array; the results on the host."""
    n = q.shape[-2]
    arm = kind_arm(kind, n) if arm is None else arm
    lam = damping if isinstance(damping, float) else T(damping, torch)
    res = solver_of(pair).joint_rates(T(q, torch), T(v, torch), damping=lam, bias_rates=None if bias is None else T(bias, torch),
                                      want=want, **arm_kwargs(kind, arm, torch))
    torch.cuda.synchronize()
    assert tuple(res) == tuple(o for o in OUTS if o in want)
    return {k: a.cpu().numpy() for k, a in res.items()}


def same(a, b, what):
    for k in b:
        assert a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def check_rows(got, ref_rates, ref_achieved, tol_row, tol_achieved, what):
    """Both outputs, flattened to rows, against the reference: the 2-norm of every row's error within its tolerance."""
    r, a = got["rates"].reshape(-1, 7), got["achieved_twist"].reshape(-1, 6)
    assert np.isfinite(r).all() and np.isfinite(a).all(), what
    er, ea = np.linalg.norm(r - ref_rates, axis=1), np.linalg.norm(a - ref_achieved, axis=1)
    worst_r, worst_a = float((er / tol_row).max()), float((ea / tol_achieved).max())
    print(f"{what}: rates max error {er.max():.3e} ({worst_r:.3g} of tol_row, max tol_row {tol_row.max():.3e}), "
          f"achieved_twist max error {ea.max():.3e} ({worst_a:.3g} of its tolerance)")
    assert (er <= tol_row).all(), (what, "rates", worst_r)
    assert (ea <= tol_achieved).all(), (what, "achieved_twist", worst_a)


def check_case(got, case, arm_flat, rows, what):
    check_rows(got, *(W.pick(case, arm_flat, rows, k) for k in ("rates", "achieved_twist", "tol_row", "tol_achieved")), what)


# ------------------------------------------------------------------------------------------ layout, equivalence and values per shape
@pytest.mark.parametrize("pair", W.PAIRS)
def test_every_shape_values_and_bits(torch_mod, pair):
    """For every n, n_rep and arm arrangement, at the three lambdas, with and without bias: the values against the reference within
    tol_row; a second launch, each output alone, the flat call on the tiled rows, a damping array filled with lambda: all bit for bit;
    an arm byte per row equals the two uniform launches row by row; a mixed damping array equals, row by row, the uniform launches at
    each of its values."""
    torch = torch_mod
    uniform, tw, bi = JW.joint_set("uniform"), W.twists(), W.biases()
    lam_pick = np.random.default_rng(7203).integers(0, len(W.LAMBDAS), size=JW.N_SET)
    for n, n_rep in itertools.product(SIZES, REPS):
        N = n * n_rep
        shape = (n_rep, n) if n_rep > 1 else (n,)
        q, v, q0 = (np.ascontiguousarray(a[:N].reshape(shape + (a.shape[1],))) for a in (uniform, tw, bi))
        rows = np.arange(N)
        full = {}
        for kind in ("r", "l", "mixed"):
            arm = kind_arm(kind, n)
            arm_flat = np.tile(arm, n_rep)
            for lam, bias in itertools.product(W.LAMBDAS, (False, True)):
                what = f"{pair} n={n} n_rep={n_rep} {kind} lambda={lam} bias={bias}"
                b = q0 if bias else None
                got = full[kind, lam, bias] = run(torch, pair, q, v, kind, lam, b)
                assert got["rates"].shape == shape + (7,) and got["achieved_twist"].shape == shape + (6,), what
                check_case(got, W.side_case(pair, "uniform", lam, bias), arm_flat, rows, what)
                same(run(torch, pair, q, v, kind, lam, b), got, what + " twice")
                for o in OUTS:
                    same(got, run(torch, pair, q, v, kind, lam, b, want=(o,)), what + f" {o} alone")
                same(run(torch, pair, q, v, kind, np.full(shape, lam), b), got, what + " damping array filled with lambda")
                if n_rep > 1:
                    flat = run(torch, pair, q.reshape(-1, 7), v.reshape(-1, 6), kind, lam, None if b is None else b.reshape(-1, 7), arm=arm_flat)
                    same({k: a.reshape(flat[k].shape) for k, a in got.items()}, flat, what + " against the flat call")
            for bias in (False, True):
                picked = lam_pick[:N].reshape(shape)
                mixed_lam = run(torch, pair, q, v, kind, np.asarray(W.LAMBDAS)[picked], q0 if bias else None)
                for o in OUTS:
                    want = np.select([picked[..., None] == i for i in range(len(W.LAMBDAS))], [full[kind, lam, bias][o] for lam in W.LAMBDAS])
                    assert np.array_equal(bits(mixed_lam[o]), bits(want)), (pair, n, n_rep, kind, bias, o, "a mixed damping array")
        is_l = (kind_arm("mixed", n) == 1)[:, None]  # (broadcasts over the repetitions)
        for lam, bias in itertools.product(W.LAMBDAS, (False, True)):
            for o in OUTS:
                want = np.where(is_l, full["l", lam, bias][o], full["r", lam, bias][o])
                assert np.array_equal(bits(full["mixed", lam, bias][o]), bits(want)), (pair, n, n_rep, lam, bias, o, "arm byte per row")


# ------------------------------------------------------------------------------------------ named sets
@pytest.mark.parametrize("pair", W.PAIRS)
def test_named_sets_against_the_reference(torch_mod, pair):
    """The golden joints of the reference's solve at the three lambdas; the wound set against the unwound rows' reference, J known to
    2e-13 per entry there (the 1e-13 more that test_gpu_jacobian allows the wound set); the singular and the near-singular set at
    lambda 1e-3 and 0.05.  At lambda = 1e-7 the singular and near-singular sets are finite, nothing more; the uniform set is still held
    to tol_row."""
    torch = torch_mod
    blocks = JW.blocks_of(pair)
    arm, rows = JW.arm_bytes(), np.arange(JW.N_SET)
    v, q0 = W.twists(), W.biases()
    gq, ga = JW.golden_joints()
    gJ = W.jacobian_rows(blocks, gq, ga)
    for lam in W.LAMBDAS:
        ref, tol = W.reference(gJ, v[:512], lam, q0[:512]), W.tolerances(gJ, v[:512], lam, q0[:512])
        check_rows(run(torch, pair, gq, v[:512], "mixed", lam, q0[:512], arm=ga), ref["rates"], ref["achieved_twist"], tol["tol_row"],
                   tol["tol_achieved"], f"{pair} golden joints lambda={lam}")
        check_case(run(torch, pair, JW.joint_set("wound"), v, "mixed", lam, q0), W.side_case(pair, "uniform", lam, True, W.WOUND_J_ENTRY),
                   arm, rows, f"{pair} wound set lambda={lam}")
    for name, lam in itertools.product(("singular", "near_singular"), (1e-3, 0.05)):
        check_case(run(torch, pair, JW.joint_set(name), v, "mixed", lam, q0), W.side_case(pair, name, lam, True), arm, rows,
                   f"{pair} {name} set lambda={lam}")
    for name in ("singular", "near_singular"):
        got = run(torch, pair, JW.joint_set(name), v, "mixed", W.TINY_LAMBDA, q0)
        print(f"{pair} {name} set lambda={W.TINY_LAMBDA}: max |rates| {np.abs(got['rates']).max():.3e}")
        assert np.isfinite(got["rates"]).all() and np.isfinite(got["achieved_twist"]).all(), (pair, name)
    check_case(run(torch, pair, JW.joint_set("uniform"), v, "mixed", W.TINY_LAMBDA, q0), W.side_case(pair, "uniform", W.TINY_LAMBDA, True),
               arm, rows, f"{pair} uniform set lambda={W.TINY_LAMBDA}")


# ------------------------------------------------------------------------------------------ frame, order and sign
def _rotation_vectors(Rp, Rm):
    """The rotation vectors of Rp Rm^T [n,3,3] -> [n,3] (angles far below pi)."""
    D = Rp @ Rm.transpose(0, 2, 1)
    w = 0.5 * np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], axis=1)  # sin(angle) axis
    s = np.linalg.norm(w, axis=1)
    scale = np.where(s > 0, np.arcsin(np.minimum(s, 1.0)) / np.where(s > 0, s, 1.0), 1.0)
    return w * scale[:, None]


@pytest.mark.parametrize("pair", W.PAIRS)
def test_achieved_twist_is_the_device_fk_s_velocity_along_the_rates(torch_mod, pair):
    """512 uniform rows, lambda = 0.05, with bias, an arm byte per row.  Central differences of rsik_forward_kinematics along the
    returned rates at h = 1e-6 — (p(q + h q') - p(q - h q')) / 2h and the rotation vector of R+ R-^T over 2h — against achieved_twist:
    1e-8 max(1, |q'|^3) (truncation h^2 |q'|^3, rounding eps / h).  This settles frame, row order and sign.  And
    |achieved - twist| <= |twist - J q0| on every row: damping only shrinks."""
    torch = torch_mod
    solver = solver_of(pair)
    n, h = 512, 1e-6
    q, arm, v, q0 = JW.joint_set("uniform")[:n], JW.arm_bytes()[:n], W.twists()[:n], W.biases()[:n]
    arm_t = T(arm, torch)
    got = run(torch, pair, q, v, "mixed", 0.05, q0)
    rates = got["rates"]

    def device_fk(x):
        p, R = solver.forward_kinematics(T(x, torch), arm=arm_t)
        return p.cpu().numpy(), R.cpu().numpy()

    (pp, Rp), (pm, Rm) = device_fk(q + h * rates), device_fk(q - h * rates)
    fd = np.concatenate([(pp - pm) / (2 * h), _rotation_vectors(Rp, Rm) / (2 * h)], axis=1)
    err = np.abs(fd - got["achieved_twist"]).max(axis=1)
    bound = 1e-8 * np.maximum(1.0, np.linalg.norm(rates, axis=1) ** 3)
    print(f"{pair}: achieved_twist against central differences of rsik_forward_kinematics along the rates: max {err.max():.3e}, "
          f"max error / bound {(err / bound).max():.3g}")
    assert (err <= bound).all(), (pair, float((err / bound).max()))
    residual = W.pick(W.side_case(pair, "uniform", 0.05, True), arm, np.arange(n), "residual_norm")
    short = np.linalg.norm(got["achieved_twist"] - v, axis=1)
    print(f"{pair}: max |achieved - twist| / |twist - J q0| = {(short / residual).max():.4f}")
    assert (short <= residual).all(), pair


# ------------------------------------------------------------------------------------------ the link to the solver
def test_a_self_motion_survives_the_projection(torch_mod):
    """The link_poses rows and filter of jacobian_workload: dq = d joints / d theta from rsik_solve_sweep at theta +- 1e-5.  With
    twist 0, bias dq and lambda = 1e-3, rsik_joint_rates returns dq to within g LINK_JDQ_BOUND + tol_row on the kept rows (J dq is
    within LINK_JDQ_BOUND of zero, and J^T A^-1 has gain g).  With bias 0 and twist 0 every entry is exactly 0.0."""
    from reachy2_symbolic_ik_amd import constants as K

    torch = torch_mod
    solver = solver_of("default/default")
    blocks = JW.blocks_of("default/default")
    pos, eul, arm, theta = JW.link_poses()
    th = np.stack([theta - JW.LINK_H, theta, theta + JW.LINK_H])
    soa = torch.as_tensor(np.ascontiguousarray(np.concatenate([pos.T, eul.T], axis=0))).cuda()
    sw = solver.solve_sweep(soa, T(th, torch), policy="explicit", arm=T(arm, torch), want_elbow=False)
    torch.cuda.synchronize()
    q = sw["joints"].cpu().numpy()
    projected = sw["projected"].cpu().numpy()
    keep, dq, _ = JW.link_measure(blocks, q[0], q[2], q[1], projected[0] | projected[2], arm, [b[K.C_ELBOW_LIMIT] for b in blocks])
    assert keep.sum() * 2 >= len(keep)
    qk, dqk, ak = np.ascontiguousarray(q[1][keep]), np.ascontiguousarray(dq[keep]), np.ascontiguousarray(arm[keep])
    zero = np.zeros((len(qk), 6))
    got = run(torch, "default/default", qk, zero, "mixed", 1e-3, dqk, arm=ak)
    tol = W.tolerances(W.jacobian_rows(blocks, qk, ak), zero, 1e-3, dqk)
    err = np.linalg.norm(got["rates"] - dqk, axis=1)
    bound = tol["g"] * JW.LINK_JDQ_BOUND + tol["tol_row"]
    print(f"solver link: kept {int(keep.sum())} of {len(keep)}, max |rates - dq| {err.max():.3e}, max error / bound {(err / bound).max():.3g}")
    assert (err <= bound).all(), float((err / bound).max())
    still = run(torch, "default/default", qk, zero, "mixed", 1e-3, np.zeros_like(dqk), arm=ak)
    assert (still["rates"] == 0.0).all() and (still["achieved_twist"] == 0.0).all()
    still = run(torch, "default/default", qk, zero, "mixed", 1e-3, None, arm=ak)
    assert (still["rates"] == 0.0).all() and (still["achieved_twist"] == 0.0).all()


# ------------------------------------------------------------------------------------------ rows that are not numbers, far angles
@pytest.mark.parametrize("kind", ["r", "mixed"])
def test_rows_that_are_not_numbers(torch_mod, kind):
    """A NaN, a +inf and a -inf in joints, twist, bias and damping in turn, and a damping entry of 0.0 and of -1.0 — in the first row,
    on both sides of a wave boundary, in the last row; in the first and in the last repetition — make those rows NaN in every output;
    every other row carries the bits of the clean run."""
    torch = torch_mod
    n, n_rep = 129, 3
    N = n * n_rep
    q, v, q0 = (np.ascontiguousarray(a[:N].reshape(n_rep, n, -1)) for a in (JW.joint_set("uniform"), W.twists(), W.biases()))
    lam = np.full((n_rep, n), 0.05)
    base = run(torch, "default/default", q, v, kind, lam, q0)
    same(run(torch, "default/default", q, v, kind, 0.05, q0), base, "damping array against damping_host")
    places = [(0, 0), (0, 63), (0, 64), (0, 128), (2, 0), (2, 63), (2, 64), (2, 128)]
    values = {"joints": (np.nan, np.inf, -np.inf), "twist": (np.nan, np.inf, -np.inf), "bias": (np.nan, np.inf, -np.inf),
              "damping": (np.nan, np.inf, -np.inf, 0.0, -1.0)}
    hit = np.zeros((n_rep, n), dtype=bool)
    for rep, row in places:
        hit[rep, row] = True
    for target, vals in values.items():
        for turn in range(len(vals)):  # the values rotate over the places: every value stands at every place in some turn
            a = {"joints": q.copy(), "twist": v.copy(), "bias": q0.copy(), "damping": lam.copy()}
            for i, (rep, row) in enumerate(places):
                val = vals[(i + turn) % len(vals)]
                if target == "damping":
                    a[target][rep, row] = val
                else:
                    a[target][rep, row, (i + turn) % a[target].shape[-1]] = val
            for want in (OUTS, ("rates",), ("achieved_twist",)):
                got = run(torch, "default/default", a["joints"], a["twist"], kind, a["damping"], a["bias"], want=want)
                for o in want:
                    assert np.isnan(got[o][hit]).all(), (kind, target, turn, o, "a row that is not numbers must be NaN in every entry")
                    assert np.array_equal(bits(got[o][~hit]), bits(base[o][~hit])), (kind, target, turn, o, "another row's bits changed")


@pytest.mark.parametrize("pair", ["default/default", "custom/custom"])
def test_far_angles_are_answered_like_their_reduced_twins(torch_mod, pair):
    """One joint at 2^27, 1e15 and 1e300 (joint_rates_workload.far_rows), lambda = 0.05, with bias: every row within tol_row of its
    reduced twin, tol_row taken with J known to 1e-9 per entry (1e-9 sqrt(42) in place of 6.5e-13), and the twins within the
    ordinary tol_row of the reference."""
    torch = torch_mod
    far, twin = W.far_rows()
    m = len(far)
    arm, v, q0 = JW.arm_bytes()[:m], W.twists()[:m], W.biases()[:m]
    a, b = run(torch, pair, far, v, "mixed", 0.05, q0, arm=arm), run(torch, pair, twin, v, "mixed", 0.05, q0, arm=arm)
    J = W.jacobian_rows(JW.blocks_of(pair), twin, arm)
    loose, ref, tight = W.tolerances(J, v, 0.05, q0, j_entry=W.FAR_J_ENTRY), W.reference(J, v, 0.05, q0), W.tolerances(J, v, 0.05, q0)
    check_rows(a, b["rates"], b["achieved_twist"], loose["tol_row"], loose["tol_achieved"], f"{pair} far rows against their reduced twins")
    check_rows(b, ref["rates"], ref["achieved_twist"], tight["tol_row"], tight["tol_achieved"], f"{pair} reduced twins")


# ------------------------------------------------------------------------------------------ refusals and the Python surface
def test_refusals(torch_mod):
    """Both outputs NULL, n < 0, n_rep < 1, joints == NULL, twist == NULL and a damping_host that is 0, negative, NaN or infinite (with
    damping == NULL) are RSIK_E_INVALID with the function's name in rsik_last_error; with a damping array damping_host is not read;
    n == 0 launches nothing; an arm whose constants were not uploaded is RSIK_E_NOT_SET."""
    from reachy2_symbolic_ik_amd import HipSolver

    torch, A = torch_mod, abi()
    solver = solver_of("default/default")
    q, v = T(JW.joint_set("uniform")[:8], torch), T(W.twists()[:8], torch)
    o = torch.empty((8, 7), dtype=torch.float64, device="cuda")
    lam = torch.full((8,), 0.05, dtype=torch.float64, device="cuda")
    arm = T(JW.arm_bytes()[:8], torch)
    cases = [("both outputs NULL", (8, 1, ptr(q), None, 0, ptr(v), 0.05, None, None, None, None)),
             ("n < 0", (-1, 1, ptr(q), None, 0, ptr(v), 0.05, None, None, ptr(o), None)),
             ("n_rep < 1", (8, 0, ptr(q), None, 0, ptr(v), 0.05, None, None, ptr(o), None)),
             ("joints NULL", (8, 1, None, None, 0, ptr(v), 0.05, None, None, ptr(o), None)),
             ("twist NULL", (8, 1, ptr(q), None, 0, None, 0.05, None, None, ptr(o), None)),
             ("arm_uniform 2", (8, 1, ptr(q), None, 2, ptr(v), 0.05, None, None, ptr(o), None))]
    cases += [(f"damping_host {d}", (8, 1, ptr(q), None, 0, ptr(v), d, None, None, ptr(o), None)) for d in (0.0, -1.0, np.nan, np.inf)]
    for what, args in cases:
        assert raw_call(solver, "rsik_joint_rates", *args) == A.RSIK_E_INVALID, what
        assert "rsik_joint_rates" in last_error(solver), (what, last_error(solver))
    assert raw_call(solver, "rsik_joint_rates", 0, 1, None, None, 0, None, 0.05, None, None, None, None) == A.RSIK_OK
    assert raw_call(solver, "rsik_joint_rates", 8, 1, ptr(q), ptr(arm), 0, ptr(v), np.nan, ptr(lam), None, ptr(o), None) == A.RSIK_OK
    bare = HipSolver(0)
    assert raw_call(bare, "rsik_joint_rates", 8, 1, ptr(q), None, 0, ptr(v), 0.05, None, None, ptr(o), None) == A.RSIK_E_NOT_SET
    assert raw_call(bare, "rsik_joint_rates", 8, 1, ptr(q), ptr(arm), 0, ptr(v), 0.05, None, None, ptr(o), None) == A.RSIK_E_NOT_SET
    torch.cuda.synchronize()
    bare.close()


def test_more_repetitions_than_one_grid_holds(torch_mod):
    """n_rep = 65537 of one row: the repetition is the grid's y, which holds 65535, so the host issues two launches, each on its slice
    of every array.  Against the flat call, bit for bit."""
    torch = torch_mod
    q, v, q0 = (np.ascontiguousarray(np.resize(a, (65537, 1, a.shape[1]))) for a in (JW.joint_set("uniform"), W.twists(), W.biases()))
    lam = np.resize(np.asarray(W.LAMBDAS), (65537, 1))
    got = run(torch, "default/default", q, v, "r", lam, q0, arm=np.zeros(1, dtype=np.uint8))
    flat = run(torch, "default/default", q.reshape(-1, 7), v.reshape(-1, 6), "r", lam.reshape(-1), q0.reshape(-1, 7))
    same({k: a.reshape(flat[k].shape) for k, a in got.items()}, flat, "n_rep = 65537")


def test_python_surface(torch_mod):
    """SymbolicIK.joint_rates_batch and DualArmIK.joint_rates_batch are HipSolver.joint_rates on their arms; out= buffers are written
    in place; a planned launch writes the same bits; the default is the rates alone."""
    from reachy2_symbolic_ik_amd import DualArmIK, SymbolicIK

    torch = torch_mod
    solver = solver_of("default/default")
    q, v, q0 = (np.ascontiguousarray(a[:390].reshape(3, 130, -1)) for a in (JW.joint_set("uniform"), W.twists(), W.biases()))
    arm = JW.arm_bytes()[:130]
    with contextlib.redirect_stdout(io.StringIO()):
        ik_l = SymbolicIK("l_arm", solver=solver, **arm_pairs.DEFAULT)
        dual = DualArmIK(solver=solver, **arm_pairs.DEFAULT)
    res = ik_l.joint_rates_batch(q, v, 0.05, bias_rates=q0)
    assert tuple(res) == ("rates",)
    same({"rates": res["rates"].cpu().numpy()}, run(torch, "default/default", q, v, "l", 0.05, q0, want=("rates",)), "SymbolicIK.joint_rates_batch")
    got = {k: a.cpu().numpy() for k, a in dual.joint_rates_batch(arm, q, v, 0.05, want=OUTS).items()}
    same(got, run(torch, "default/default", q, v, "mixed", 0.05), "DualArmIK.joint_rates_batch")
    out = {"achieved_twist": torch.full((3, 130, 6), 7.0, dtype=torch.float64, device="cuda")}
    res = solver.joint_rates(T(q, torch), T(v, torch), damping=0.05, arm=T(arm, torch), want=OUTS, out=out)
    assert res["achieved_twist"] is out["achieved_twist"] and tuple(res) == OUTS
    plan = solver.joint_rates(T(q, torch), T(v, torch), damping=0.05, arm=T(arm, torch), want=("achieved_twist",), plan_only=True)
    plan["launch"]()
    torch.cuda.synchronize()
    assert np.array_equal(bits(plan["achieved_twist"].cpu().numpy()), bits(out["achieved_twist"].cpu().numpy()))
    assert np.array_equal(bits(out["achieved_twist"].cpu().numpy()), bits(got["achieved_twist"]))
    for bad in (dict(want=()), dict(damping=0.0), dict(damping=None), dict(damping=float("nan"))):
        with pytest.raises(ValueError):
            solver.joint_rates(T(q, torch), T(v, torch), **{"damping": 0.05, **bad})
    with pytest.raises(ValueError):
        solver.joint_rates(T(q, torch), T(v[..., :5], torch), damping=0.05)


def test_integration_md_snippet(torch_mod):
    """The snippet of INTEGRATION.md as written: solve a pose batch, joint rates for a twist with bias_rates = k * null_vector, one
    integration step, fk_residual against the moved poses.  On the rows whose goal the solve reached (the elbow projection moves
    the others' goals before any step is taken) the error is what the damping held back, dt |twist - achieved_twist|,
    plus the second-order terms of the step (dt^2 |q'|^2 times the arm's length and 1: below 2e-5 at |q'| <= 4)."""
    from reachy2_symbolic_ik_amd import SymbolicIK

    torch = torch_mod
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", solver=solver_of("default/default"), **arm_pairs.DEFAULT)
    pos, eul, arm, _ = JW.link_poses()
    poses = np.ascontiguousarray(np.stack([pos[arm == 0], eul[arm == 0]], axis=1))  # [n,2,3]

    q = ik.solve_batch(poses)["joints"]
    null = ik.jacobian_batch(q, want=("null_vector",))["null_vector"]
    twist = torch.zeros((len(q), 6), dtype=torch.float64, device=q.device)
    twist[:, 0] = 0.05
    step = ik.joint_rates_batch(q, twist, damping=0.02, bias_rates=0.5 * null, want=("rates", "achieved_twist"))
    dt = 1e-3
    q_next = q + dt * step["rates"]
    moved = poses.copy()
    moved[:, 0, 0] += dt * 0.05
    err = ik.fk_residual_batch(moved, q_next)
    on_goal = ik.fk_residual_batch(poses, q)[:, 0] < 1e-9

    assert tuple(err.shape) == (len(poses), 2) and bool(torch.isfinite(err).all())
    on_goal = on_goal.cpu().numpy()
    assert on_goal.sum() * 2 >= len(poses)
    held_back = (twist - step["achieved_twist"]).cpu().numpy()[on_goal]
    speed = float(step["rates"].norm(dim=1).max())
    err = err.cpu().numpy()[on_goal]
    print(f"INTEGRATION.md snippet: max position error {err[:, 0].max():.3e} m, rotation {err[:, 1].max():.3e} rad, max |rates| {speed:.3f}")
    assert speed <= 4.0
    assert (err[:, 0] <= dt * np.linalg.norm(held_back[:, :3], axis=1) + 2e-5).all()
    assert (err[:, 1] <= dt * np.linalg.norm(held_back[:, 3:], axis=1) + 2e-5).all()
    assert np.median(err[:, 0]) <= 1e-5
