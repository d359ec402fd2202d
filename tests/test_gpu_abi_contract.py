"""GPU tests (-m gpu, MI355X) of what include/rsik.h promises a C host and the Python driver never asks for: outputs left out
(NULL), optional inputs left out (NULL = a documented explicit value), and rsik_stage with row strides above the minimum and
with rows in pinned host memory.  Everything goes through raw ctypes (solver.lib.rsik_*), on the caller's own buffers.

The reference of every test is the library's own launch with every output present and every input explicit — the form the other
GPU tests hold against the CPU checker and the reference's recordings.  Every assertion is bit equality, an exact status code or
an exact sentinel; no tolerance.  Every kept output buffer has GUARD rows of a sentinel behind it: a store meant for a
neighbouring (dropped) output that landed there changes them.  Shares of reachable / latched rows are conditions on the inputs,
checked on the reference launch; they exclude no row from a comparison.

A NULL output is only safe where every store to it is guarded; the guards were read before these tests first ran:
  solve_kernel                    joints rsik_kernel_solve.hpp:395,398; elbow :347 (371, 378, 387, 396, 399); store_reach (rsik_goal.hpp): interval,
                                  reachable and state, each behind its own test
  control_discrete_kernel         rsik_kernel_discrete.hpp: reachable :354, state :355, emergency :356
  control_continuous_kernel       rsik_kernel_continuous.hpp: reachable :207, state :208 (inputs: timed_out :157, cur_pose :50,
                                  current_joints :44)
  rsik_control_continuous_run     rsik_cont_run.hpp:377-378 (a NULL is not offset per step), :464-467 (no range of a NULL);
                                  cont_prepare_step rsik_kernel_pipeline.hpp:151-152; cont_chain_walk: a latched step :638-639, the
                                  latch fill :694-695
  reach_state_kernel              rsik_kernel_state.hpp: interval :56, reachable :57, state :58
  joints_state_kernel             rsik_kernel_state.hpp: joints :90, elbow :100, previous_joints :86
  theta_from_joints_kernel        rsik_kernel_theta_from_joints.hpp: joints :149, bracket :152, distance :153, state :154;
                                  theta_from_joints_state_kernel: bracket :177
  fk_kernel                       rsik_kernel_state.hpp: position :140, rotation :141 (both NULL refused, rsik_lib.hip:764)
"""
import ctypes as C

import numpy as np
import pytest

import scale_inputs as SC
import theta_workload as W
from checker_support import load, reachable_rich
from compare import bits, same_bits
from gpu_support import T, _eventful_trajectories, abi, last_error, make_control, make_symbolic, ptr, raw_call, soa, torch_mod  # noqa: F401
from gpu_support import cols as table  # (the tests below call the table of a launch `cols`)
from sweep_workload import sweep_poses

pytestmark = pytest.mark.gpu

F64_MARK, U8_MARK, GUARD = -777.0, 0xA5, 3
PREFERRED_THETA = -4 * np.pi / 6
MAX_ANGLE = float(np.deg2rad(42.5))
RUN_SEED = 7126  # trajectories of the continuous run: on the CPU checker 24 of the 96 latch before the last block, 4 inside it, 68 never


# ------------------------------------------------------------------------------------------ helpers
def host_doubles(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


class Outputs:
    """The output buffers of one launch.  spec: name -> (rows, width, "f64" / "u8"), width 0 for a vector.  A kept output is
    `rows` rows of the sentinel with GUARD more behind them; a dropped one is NULL."""

    def __init__(self, torch, spec, drop=()):
        assert set(drop) <= set(spec), drop
        self.spec = spec
        self.buf = {}
        for name, (rows, width, kind) in spec.items():
            if name not in drop:
                shape = (rows + GUARD,) + ((width,) if width else ())
                self.buf[name] = torch.full(shape, F64_MARK if kind == "f64" else U8_MARK, device="cuda",
                                            dtype=torch.float64 if kind == "f64" else torch.uint8)

    def p(self, name):
        return ptr(self.buf.get(name))

    def host(self, what):
        out = {}
        for name, t in self.buf.items():
            rows, _, kind = self.spec[name]
            h = t.cpu().numpy()
            assert (h[rows:] == (F64_MARK if kind == "f64" else U8_MARK)).all(), f"{what}: the guard rows behind {name} were written"
            out[name] = h[:rows]
        return out


def same_outputs(got, ref, what):
    for name, v in got.items():
        same_bits(v, ref[name], f"{what}: {name}")


def rows_that_differ(a, b):
    d = bits(a) != bits(b)
    return np.flatnonzero(d.reshape(len(d), -1).any(axis=1))


def drop_sets(optional, required_to_see=()):
    """Each optional output alone, then all of them at once (but `required_to_see`, where nothing else would be observable)."""
    sets = [(name,) for name in optional]
    rest = tuple(name for name in optional if name not in required_to_see)
    if len(rest) > 1:
        sets.append(rest)
    return sets


def mirror_for_arm(m12, arm_t):
    """Goal matrices of the right arm, rows of the left arm mirrored (M_l = S M S, S = diag(1, -1, 1): sign flips, exact).
    m12: [..., 12, n]."""
    sgn = 1.0 - 2.0 * arm_t.double()
    out = m12.clone()
    for k in (1, 3, 5, 7, 10):
        out[..., k, :] = out[..., k, :] * sgn
    return out.contiguous()


@pytest.fixture(scope="module")
def sym(torch_mod):
    """One context with both arms of singularity_offset 0.03 (the elbow projection can fire)."""
    solver, r, l = make_symbolic(0.03)
    yield solver
    solver.close()


def arm_args(kind, arm, torch):
    return (T(arm, torch), 0) if kind == "mixed" else (None, int(kind == "l"))


# ------------------------------------------------------------------------------------------ 1. optional outputs
SOLVE_OUTPUTS = ("joints", "interval", "elbow", "reachable", "state")


@pytest.mark.parametrize("entry", ["rsik_solve", "rsik_solve_rows"])
@pytest.mark.parametrize("kind", ["mixed", "l"])
def test_solve_outputs_left_out(torch_mod, sym, kind, entry):
    """n = 321 (a full block, a full wave, a ragged wave of one row): each of the five outputs dropped alone, then all but
    joints, then all but state, under RSIK_THETA_FRACTION and RSIK_THETA_INTERVAL0.  RSIK_THETA_NONE with joints and elbow GIVEN
    leaves them untouched and answers the interval, reachable and state of the fraction launch.  rsik_solve: a NULL
    previous_joints_host is seven zeros."""
    torch, A, solver, n = torch_mod, abi(), sym, 321
    pos, eul, arm = sweep_poses(kind, 900, n)
    p = soa(pos, eul, torch)
    cols = table(p, 6)
    arm_t, arm_uniform = arm_args(kind, arm, torch)
    rng = np.random.default_rng(901)
    frac = T(rng.uniform(0.0, 1.0, size=n), torch)
    prev_rows = T(rng.uniform(-2, 2, size=(n, 7)), torch)
    prev_host, prev_host_p = host_doubles(rng.uniform(-2, 2, size=7))
    prev = ptr(prev_rows) if entry == "rsik_solve_rows" else prev_host_p
    spec = dict(joints=(n, 7, "f64"), interval=(n, 2, "f64"), elbow=(n, 3, "f64"), reachable=(n, 0, "u8"), state=(n, 0, "u8"))

    def launch(policy, theta, drop=(), prev=prev):
        what = f"{entry} {kind} policy {policy} without {drop}"
        o = Outputs(torch, spec, drop)
        rc = raw_call(solver, entry, n, cols, ptr(arm_t), arm_uniform, policy, ptr(theta), prev, o.p("joints"), o.p("interval"),
                      o.p("elbow"), o.p("reachable"), o.p("state"))
        assert rc == A.RSIK_OK, (what, rc, last_error(solver))
        solver.synchronize()
        return o.host(what), what

    full = {}
    for policy, theta in ((A.THETA_FRACTION, frac), (A.THETA_INTERVAL0, None)):
        full[policy], _ = launch(policy, theta)
        share = float(full[policy]["reachable"].mean())
        print(f"{entry} {kind} policy {policy}: {share:.3f} of the rows reachable")
        assert 0.2 <= share <= 0.8, "the inputs must hold at least 20 % reachable and 20 % unreachable rows"
        for drop in drop_sets(SOLVE_OUTPUTS, ("joints",)) + [tuple(k for k in SOLVE_OUTPUTS if k != "state")]:
            got, what = launch(policy, theta, drop)
            assert set(got) == set(SOLVE_OUTPUTS) - set(drop)
            same_outputs(got, full[policy], what)
    none, what = launch(A.THETA_NONE, None)
    assert (none["joints"] == F64_MARK).all() and (none["elbow"] == F64_MARK).all(), "RSIK_THETA_NONE writes neither joints nor elbow"
    for name in ("interval", "reachable", "state"):
        same_bits(none[name], full[A.THETA_FRACTION][name], f"{what}: {name} against the fraction launch")
    got, what = launch(A.THETA_NONE, None, drop=("joints", "elbow", "interval", "reachable"))
    same_outputs(got, full[A.THETA_FRACTION], what)
    if entry == "rsik_solve":  # 2. optional input: NULL previous_joints_host = zeros
        zeros, zeros_p = host_doubles(np.zeros(7))
        explicit, _ = launch(A.THETA_FRACTION, frac, prev=zeros_p)
        null, what = launch(A.THETA_FRACTION, frac, prev=None)
        same_outputs(null, explicit, what + " (previous_joints_host NULL against seven zeros)")


DISCRETE_OPTIONAL = ("reachable", "state", "emergency")


@pytest.mark.parametrize("entry", ["rsik_control_discrete", "rsik_control_discrete_rows"])
@pytest.mark.parametrize("kind", ["mixed", "r"])
def test_control_discrete_outputs_left_out(torch_mod, golden_dir, kind, entry):
    """n = 321, 20 search points, previous_sol beyond +-6 pi in joints 0, 2 and 6 (G11's scenario 7, which trips all three limits; test_emergency_reports_discrete
    takes scenario 0 the same way): reachable, state and emergency dropped alone and together; the joints and what is kept keep their bits.
    rsik_control_discrete: a NULL current_joints is the previous_sol_host row of each pose's arm."""
    from reachy2_symbolic_ik_amd.control_ik import matrices_to_m12_soa

    torch, A, n = torch_mod, abi(), 321
    c = make_control()
    solver = c._solver
    c._upload_arms()
    pos, eul, arm = sweep_poses(kind, 910, n)
    m = matrices_to_m12_soa(SC.matrices_from_pose(pos, eul), solver.device)
    cols = table(m, 12)
    arm_t, arm_uniform = arm_args(kind, arm, torch)
    g = load(golden_dir, "g11_emergency.npz")
    ps = np.stack([g["r_arm_discrete_current_joints"][7][0], g["l_arm_discrete_current_joints"][7][1]])
    assert g["r_arm_discrete_cause"][7] == 7 and g["l_arm_discrete_cause"][7] == 7
    ps_host, ps_host_p = host_doubles(ps)
    own = T(ps[arm if kind == "mixed" else np.zeros(n, dtype=np.int64)], torch)  # previous_sol of each pose's arm, [n,7]
    prev = ptr(own) if entry == "rsik_control_discrete_rows" else ps_host_p
    spec = dict(joints=(n, 7, "f64"), reachable=(n, 0, "u8"), state=(n, 0, "u8"), emergency=(n, 0, "u8"))

    def launch(drop=(), current_joints=None):
        what = f"{entry} {kind} without {drop}"
        o = Outputs(torch, spec, drop)
        rc = raw_call(solver, entry, n, cols, ptr(arm_t), arm_uniform, 20, PREFERRED_THETA, A.MODE_UNCONSTRAINED, prev,
                      ptr(current_joints), MAX_ANGLE, o.p("joints"), o.p("reachable"), o.p("state"), o.p("emergency"))
        assert rc == A.RSIK_OK, (what, rc, last_error(solver))
        solver.synchronize()
        return o.host(what), what

    full, _ = launch()
    print(f"{entry} {kind}: reachable {full['reachable'].mean():.3f}, rows that tripped {int((full['emergency'] != 0).sum())}, "
          f"causes {sorted(set(full['emergency'].tolist()))}")
    assert (full["emergency"] != 0).any(), "previous_sol must trip multiturn_safety_check in at least one row"
    for drop in drop_sets(DISCRETE_OPTIONAL):
        got, what = launch(drop)
        same_outputs(got, full, what)
    if entry == "rsik_control_discrete":  # 2. optional input: NULL current_joints = previous_sol of the row's arm
        fallback = full["reachable"] == 0
        assert fallback.any(), "current_joints is only read by a row that finds no theta: the inputs must hold such rows"
        explicit, what = launch(current_joints=own)
        for name in spec:  # the rows that differ, with their inputs
            for i in rows_that_differ(full[name], explicit[name])[:4]:
                print(f"{what}: row {i} arm {arm[i] if kind == 'mixed' else 0} {name} NULL {full[name][i]!r} explicit {explicit[name][i]!r} "
                      f"current_joints {own[i].cpu().numpy()!r} pose {pos[i]!r} {eul[i]!r} reachable {full['reachable'][i]}")
        same_outputs(full, explicit, what + " (current_joints NULL against previous_sol of the row's arm)")


def step_inputs(torch, kind, n, n_steps, seed):
    """Goal matrices [n_steps, 12, n] of the eventful-trajectory builder (right arm; the rows of the left arm mirrored), and how the
    arm reaches the ABI."""
    traj = _eventful_trajectories(torch, n, n_steps, seed, "r_arm")
    if kind != "mixed":
        return traj, None, None, 0
    arm = (np.random.default_rng(seed).uniform(size=n) < 0.5).astype(np.uint8)
    arm_t = T(arm, torch)
    return mirror_for_arm(traj, arm_t), arm, arm_t, 0


@pytest.mark.parametrize("kind", ["mixed", "r"])
def test_control_continuous_step_outputs_and_inputs_left_out(torch_mod, kind):
    """n = 129, three consecutive steps (13 control steps apart, so that some trajectories trip the continuity check and the third
    step finds them latched), the first with timed_out = 1: reachable and state dropped alone and together — cont_state and the
    joints after every step.  Then one input at a time in its explicit form against the NULL form, the same way: current_pose
    (the goal matrix), timed_out (zeros, steps two and three), current_joints (rows 1-7 of cont_state, transposed)."""
    torch, A, n = torch_mod, abi(), 129
    c = make_control()
    solver = c._solver
    c._upload_arms()
    traj, arm, arm_t, arm_uniform = step_inputs(torch, kind, n, 27, 920)
    goals = [traj[s].contiguous() for s in (0, 13, 26)]
    start = c.new_continuous_state("r_arm" if arm is None else arm, n)
    _, pts = host_doubles([c.preferred_theta["r_arm"], c.preferred_theta["l_arm"]])
    ones, zeros = torch.ones(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    spec = dict(joints=(n, 7, "f64"), reachable=(n, 0, "u8"), state=(n, 0, "u8"))

    def three_steps(drop=(), explicit=()):
        what = f"rsik_control_continuous_step {kind} without {drop} explicit {explicit}"
        st = start.clone()
        steps = []
        for s, goal in enumerate(goals):
            timed_out = ones if s == 0 else (zeros if "timed_out" in explicit else None)
            cp = table(goal, 12) if (s == 0 and "current_pose" in explicit) else None
            cj = st[1:8].t().contiguous() if (s == 0 and "current_joints" in explicit) else None
            o = Outputs(torch, spec, drop)
            rc = raw_call(solver, "rsik_control_continuous_step", n, table(goal, 12), cp, ptr(arm_t), arm_uniform, ptr(timed_out),
                          PREFERRED_THETA, pts, A.MODE_UNCONSTRAINED, 0.01, ptr(cj), MAX_ANGLE, ptr(st), o.p("joints"),
                          o.p("reachable"), o.p("state"))
            assert rc == A.RSIK_OK, (what, s, rc, last_error(solver))
            solver.synchronize()
            out = o.host(f"{what} step {s}")
            out["cont_state"] = st.cpu().numpy().copy()
            steps.append(out)
        return steps, what

    full, _ = three_steps()
    print(f"continuous step {kind}: reachable per step {[round(float(s['reachable'].mean()), 3) for s in full]}, "
          f"latched after each {[int((s['cont_state'][9] != 0).sum()) for s in full]}")
    variants = [dict(drop=d) for d in drop_sets(("reachable", "state"))]
    variants += [dict(explicit=(name,)) for name in ("current_pose", "timed_out", "current_joints")]
    for kw in variants:
        got, what = three_steps(**kw)
        for s in range(3):
            same_outputs(got[s], full[s], f"{what} step {s}")


def latch_steps(state_steps, latched_at_the_end):
    """The step at which each trajectory's emergency stop latched (the step before its first RSIK_STATE_EMERGENCY; the last step
    for one that is latched at the end without having reported it), -1 for a trajectory that never latched."""
    n_steps, n = state_steps.shape
    is8 = state_steps == 8
    first8 = np.where(is8.any(axis=0), is8.argmax(axis=0), n_steps)
    trip = np.where(first8 < n_steps, first8 - 1, np.where(latched_at_the_end, n_steps - 1, -1))
    return trip


@pytest.mark.parametrize("form", ["phased", "steps"])
@pytest.mark.parametrize("kind", ["mixed", "r"])
def test_control_continuous_run_outputs_and_inputs_left_out(torch_mod, kind, form):
    """96 trajectories x 40 steps in blocks of 16 (three blocks, the last one ragged), as the phased pipeline and as a launch per step:
    reachable_steps, state_steps and both dropped — joints_steps and the final cont_state have the bits of the run with both, and
    rsik_control_continuous_last_form reports the form asked for.  The reference run must hold trajectories that latch before the
    last block (the latch fill on entry of a later block), inside it (the fill behind a chunk), and a quarter that never latch.
    Then current_pose (the first goal) and current_joints (rows 1-7 of cont_state, transposed) explicit against NULL."""
    torch, A, n, n_steps, block = torch_mod, abi(), 96, 40, 16
    c = make_control()
    solver = c._solver
    c._upload_arms()
    traj, arm, arm_t, arm_uniform = step_inputs(torch, kind, n, n_steps, RUN_SEED)
    start = c.new_continuous_state("r_arm" if arm is None else arm, n)
    _, pts = host_doubles([c.preferred_theta["r_arm"], c.preferred_theta["l_arm"]])
    rows = n_steps * n
    spec = dict(joints=(rows, 7, "f64"), reachable=(rows, 0, "u8"), state=(rows, 0, "u8"))
    run_mode, want_form = {"phased": (A.CONT_RUN_PHASED, A.CONT_FORM_PHASED), "steps": (A.CONT_RUN_STEPS, A.CONT_FORM_STEPS)}[form]

    def run(drop=(), explicit=()):
        what = f"rsik_control_continuous_run {kind} {form} without {drop} explicit {explicit}"
        st = start.clone()
        cp = table(traj[0], 12) if "current_pose" in explicit else None
        cj = st[1:8].t().contiguous() if "current_joints" in explicit else None
        o = Outputs(torch, spec, drop)
        rc = raw_call(solver, "rsik_control_continuous_run", n, n_steps, ptr(traj), cp, ptr(arm_t), arm_uniform, 1, PREFERRED_THETA, pts,
                      A.MODE_UNCONSTRAINED, 0.01, ptr(cj), MAX_ANGLE, ptr(st), o.p("joints"), o.p("reachable"), o.p("state"))
        assert rc == A.RSIK_OK, (what, rc, last_error(solver))
        assert solver.continuous_last_form() == want_form, (what, solver.continuous_last_form())
        solver.synchronize()
        out = o.host(what)
        out["cont_state"] = st.cpu().numpy().copy()
        return out, what

    solver.set_option(A.OPT_CONT_RUN_MODE, run_mode)
    solver.set_option(A.OPT_CONT_BLOCK_STEPS, block)
    try:
        full, _ = run()
        trip = latch_steps(full["state"].reshape(n_steps, n), full["cont_state"][9] != 0)
        last_block = (n_steps - 1) // block * block
        print(f"continuous run {kind} {form}: latched before the last block {int(((trip >= 0) & (trip < last_block)).sum())}, "
              f"inside it {int((trip >= last_block).sum())}, never {int((trip < 0).sum())} of {n}")
        assert ((trip >= 0) & (trip < last_block)).any(), "no trajectory latches before the last block"
        assert (trip >= last_block).any(), "no trajectory latches inside the last block"
        assert (trip < 0).sum() * 4 >= n, "less than a quarter of the trajectories never latch"
        assert ((full["cont_state"][9] != 0) == (trip >= 0)).all()
        for kw in [dict(drop=d) for d in drop_sets(("reachable", "state"))] + [dict(explicit=(name,)) for name in ("current_pose", "current_joints")]:
            got, what = run(**kw)
            same_outputs(got, full, what)
    finally:
        solver.set_option(A.OPT_CONT_RUN_MODE, A.CONT_RUN_AUTO)
        solver.set_option(A.OPT_CONT_BLOCK_STEPS, 0)



def state_rows_inputs(torch, n, seed):
    arm = (np.random.default_rng(seed).uniform(size=n) < 0.5).astype(np.uint8)
    pos, eul = reachable_rich(seed + 1, n, arm)
    return soa(pos, eul, torch), arm, T(arm, torch)


def test_reach_state_outputs_left_out(torch_mod, sym):
    """n = 129, mixed arms, on rows prefilled with a sentinel: interval, reachable and state dropped alone and together — every
    slot of the solver-state rows (20-23 carry the same results) has the bits of the launch with all three."""
    torch, A, solver, n = torch_mod, abi(), sym, 129
    p, arm, arm_t = state_rows_inputs(torch, n, 930)
    cols = table(p, 6)
    prefill = T(np.tile(1000.0 + np.arange(32.0), (n + GUARD, 1)), torch)
    spec = dict(interval=(n, 2, "f64"), reachable=(n, 0, "u8"), state=(n, 0, "u8"))

    def launch(drop=()):
        what = f"rsik_reach_state without {drop}"
        st = prefill.clone()
        o = Outputs(torch, spec, drop)
        rc = raw_call(solver, "rsik_reach_state", n, cols, ptr(arm_t), 0, 0, ptr(st), o.p("interval"), o.p("reachable"), o.p("state"))
        assert rc == A.RSIK_OK, (what, rc, last_error(solver))
        solver.synchronize()
        out = o.host(what)
        out["solver_state"] = st.cpu().numpy()  # (with its guard rows: compared like the rest)
        return out, what

    full, _ = launch()
    S = full["solver_state"]
    same_bits(S[n:], prefill.cpu().numpy()[n:], "the rows behind the last solver-state row")
    same_bits(S[:n, 20:22], full["interval"], "slots 20-21")
    same_bits(S[:n, 22], full["reachable"], "slot 22")
    same_bits(S[:n, 23], full["state"], "slot 23")
    assert 0.2 <= full["reachable"].mean() < 1.0
    for drop in drop_sets(tuple(spec)):
        got, what = launch(drop)
        same_outputs(got, full, what)


def test_joints_from_state_outputs_left_out(torch_mod, sym):
    """n = 129, mixed arms, rows a reach_state left: joints, elbow and both dropped — the rows (16-19 and 24-30 carry the values)
    and what is kept have the bits of the launch with both.  A NULL previous_joints is zeros."""
    torch, A, solver, n = torch_mod, abi(), sym, 129
    p, arm, arm_t = state_rows_inputs(torch, n, 940)
    reached = solver.new_solver_state(n)
    r = solver.reach_state(p, reached, arm=arm_t)
    theta = torch.nan_to_num(r["interval"][:, 0]).contiguous()
    assert float(r["reachable"].double().mean()) > 0.5
    spec = dict(joints=(n, 7, "f64"), elbow=(n, 3, "f64"))
    zeros = torch.zeros((n, 7), dtype=torch.float64, device="cuda")

    def launch(drop=(), prev=None):
        what = f"rsik_joints_from_state without {drop}"
        st = reached.clone()
        o = Outputs(torch, spec, drop)
        rc = raw_call(solver, "rsik_joints_from_state", n, ptr(st), ptr(arm_t), 0, ptr(theta), ptr(prev), o.p("joints"), o.p("elbow"))
        assert rc == A.RSIK_OK, (what, rc, last_error(solver))
        solver.synchronize()
        out = o.host(what)
        out["solver_state"] = st.cpu().numpy()
        return out, what

    full, _ = launch()
    same_bits(full["solver_state"][:, 24:31], full["joints"], "slots 24-30")
    same_bits(full["solver_state"][:, 16:19], full["elbow"], "slots 16-18")
    assert np.isfinite(full["joints"]).mean() > 0.5
    for drop in drop_sets(tuple(spec)):
        got, what = launch(drop)
        same_outputs(got, full, what)
    explicit, what = launch(prev=zeros)
    same_outputs(full, explicit, what + " (previous_joints NULL against zeros)")


def test_theta_from_joints_outputs_left_out(torch_mod, sym):
    """n = 129 rows of tests/theta_workload.py, mixed arms.  rsik_theta_from_joints: joints, bracket, distance and state dropped alone
    and together; rsik_theta_from_joints_state: bracket dropped — theta, what is kept and the solver-state rows keep their bits."""
    torch, A, solver, n = torch_mod, abi(), sym, 129
    pos, eul, arm, cur = W.theta_workload(950, n)
    p, arm_t, cur_t = soa(pos, eul, torch), T(arm, torch), T(cur, torch)
    cols = table(p, 6)
    _, pref = host_doubles(W.PREFERRED)
    spec = dict(theta=(n, 0, "f64"), joints=(n, 7, "f64"), bracket=(n, 2, "f64"), distance=(n, 0, "f64"), state=(n, 0, "u8"))

    def fused(drop=()):
        what = f"rsik_theta_from_joints without {drop}"
        o = Outputs(torch, spec, drop)
        rc = raw_call(solver, "rsik_theta_from_joints", n, A.GOAL_POSE6, cols, ptr(arm_t), 0, ptr(cur_t), pref, o.p("theta"), o.p("joints"),
                      o.p("bracket"), o.p("distance"), o.p("state"))
        assert rc == A.RSIK_OK, (what, rc, last_error(solver))
        solver.synchronize()
        return o.host(what), what

    full, _ = fused()
    assert (full["state"] == 0).all() and np.isfinite(full["theta"]).all()
    assert 0 < np.isnan(full["bracket"][:, 0]).sum() < n, "shortcut rows (no bracket) and searched rows"
    for drop in drop_sets(("joints", "bracket", "distance", "state")):
        got, what = fused(drop)
        same_outputs(got, full, what)

    reached = solver.new_solver_state(n)
    solver.reach_state(p, reached, arm=arm_t, no_limits=True)
    spec_state = dict(theta=(n, 0, "f64"), bracket=(n, 2, "f64"))

    def on_rows(drop=()):
        what = f"rsik_theta_from_joints_state without {drop}"
        st = reached.clone()
        o = Outputs(torch, spec_state, drop)
        rc = raw_call(solver, "rsik_theta_from_joints_state", n, ptr(st), ptr(arm_t), 0, ptr(cur_t), 7, pref, o.p("theta"), o.p("bracket"))
        assert rc == A.RSIK_OK, (what, rc, last_error(solver))
        solver.synchronize()
        out = o.host(what)
        out["solver_state"] = st.cpu().numpy()
        return out, what

    full_rows, _ = on_rows()
    got, what = on_rows(("bracket",))
    same_outputs(got, full_rows, what)


def test_forward_kinematics_outputs_left_out(torch_mod, sym):
    """n = 129, mixed arms: position only and rotation only have the bits of the launch with both; both NULL is refused."""
    torch, A, solver, n = torch_mod, abi(), sym, 129
    rng = np.random.default_rng(960)
    joints = T(rng.uniform(-np.pi, np.pi, size=(n, 7)), torch)
    arm_t = T((rng.uniform(size=n) < 0.5).astype(np.uint8), torch)
    spec = dict(position=(n, 3, "f64"), rotation=(n, 9, "f64"))

    def launch(drop=()):
        what = f"rsik_forward_kinematics without {drop}"
        o = Outputs(torch, spec, drop)
        rc = raw_call(solver, "rsik_forward_kinematics", n, ptr(joints), ptr(arm_t), 0, o.p("position"), o.p("rotation"))
        assert rc == A.RSIK_OK, (what, rc, last_error(solver))
        solver.synchronize()
        return o.host(what), what

    full, _ = launch()
    assert np.isfinite(full["position"]).all() and np.isfinite(full["rotation"]).all()
    for drop in (("rotation",), ("position",)):
        got, what = launch(drop)
        same_outputs(got, full, what)
    assert raw_call(solver, "rsik_forward_kinematics", n, ptr(joints), ptr(arm_t), 0, None, None) == A.RSIK_E_INVALID
    assert "rsik_forward_kinematics" in last_error(solver), last_error(solver)
    solver.synchronize()


# ------------------------------------------------------------------------------------------ 3. rsik_stage: strides, pinned host rows
def stage_rows(golden_dir):
    """The operands of every stage, from the golden sets whose recorded results the existing tests hold the packed call against
    (G15: test_stage_entry_points_against_reference, right arm; G18: test_utils_stages_against_reference; G19: the rate limiter —
    get_best_continuous_theta2 on G18's get_best_discrete_theta operands with G19's d_theta_max values, recycled)."""
    g15, g18, g19 = (load(golden_dir, name) for name in ("g15_stages.npz", "g18_utils.npz", "g19_start_theta.npz"))
    G = lambda k: g15[f"r_arm_{k}"]  # noqa: E731
    have = G("ic_found") != 0
    found = G("na_found")[have] != 0
    lcg, icg = G("lc")[have], G("ic")[have]
    a = g18["bd_args"]
    discrete = np.column_stack([a[:, 0], g18["bd_interval"], a[:, 1:], g18["bd_circle"]])
    rows = {
        0: np.column_stack([G("pos"), G("eul")]),
        1: np.column_stack([G("pos"), G("eul")]),
        2: np.column_stack([G("wrist"), G("pos")]),
        3: G("wrist"),
        4: np.column_stack([G("wrist"), G("ic"), G("lc")])[have],
        5: np.column_stack([lcg[:, 0:3], lcg[:, 4:7], icg[:, 0:3], icg[:, 4:7]]),
        6: np.column_stack([lcg[found, 0:4], G("na_v")[have][found], G("na_q")[have][found]]),
        7: G("lc")[:, 4:7],
        8: np.column_stack([g18["ad_a"], g18["ad_b"]]),
        9: np.column_stack([g18["iv_angle"], g18["iv_interval"]]),
        10: np.column_stack([g18["iv_angle"], g18["iv_prev"], g18["iv_interval"]]),
        11: np.column_stack([g18["eo_elbow"], g18["eo_side"], g18["eo_so"], g18["eo_coeff"], g18["eo_esp"]]),
        12: np.column_stack([g18["mt_new"], g18["mt_prev"]]),
        13: np.column_stack([g18["lo_joints"], g18["lo_max"]]),
        14: np.column_stack([g18["ms_joints"], g18["ms_limits"]]),
        15: np.column_stack([g18["cc_joints"], g18["cc_prev"], np.tile(g18["cc_max"], (len(g18["cc_joints"]), 1))]),
        16: discrete,
        17: g19["tend_in"],
        18: np.column_stack([discrete, np.resize(g19["cont2_in"][:, 3], len(discrete))]),
    }
    return {op: np.ascontiguousarray(v, dtype=np.float64) for op, v in rows.items()}


@pytest.fixture(scope="module")
def stage_inputs(golden_dir):
    return stage_rows(golden_dir)


@pytest.mark.parametrize("op", range(19))
def test_stage_row_strides_and_pinned_host_rows(torch_mod, sym, stage_inputs, op):
    """Every stage at n = 1, 64, 65, 257 (golden rows, recycled where a set is shorter), three times: packed in device memory (what
    HipSolver.stage does); in_stride = need_in + 3 and out_stride = need_out + 5 with NaN in the input padding and a sentinel in the
    output padding — the payload has the bits of the packed call, the padding and the guard rows keep the sentinel; and the same
    padded rows in pinned host memory, read after rsik_sync.  A stride below what the stage reads or writes is refused: nothing
    is written."""
    torch, A, solver = torch_mod, abi(), sym
    need_in, need_out = A.STAGE_ROW[op]
    golden = stage_inputs[op]
    assert golden.shape[1] == need_in and len(golden) >= 64
    pad_in, pad_out = need_in + 3, need_out + 5

    def call(n, src, in_stride, dst, out_stride):
        return raw_call(solver, "rsik_stage", op, n, 0, src.data_ptr(), in_stride, dst.data_ptr(), out_stride)

    for n in (1, 64, 65, 257):
        what = f"stage {op} n {n}"
        x = golden[np.arange(n) % len(golden)]
        # (a) packed
        packed_out = torch.full((n + GUARD, need_out), F64_MARK, dtype=torch.float64, device="cuda")
        assert call(n, T(x, torch), need_in, packed_out, need_out) == A.RSIK_OK, (what, last_error(solver))
        solver.synchronize()
        packed = packed_out.cpu().numpy()
        assert (packed[n:] == F64_MARK).all(), what + ": guard rows of the packed call"
        assert not (packed[:n] == F64_MARK).all(axis=0).any(), what + ": every column of the payload is written"
        # (b) padded, (c) padded in pinned host memory
        xp = np.full((n, pad_in), np.nan)
        xp[:, :need_in] = x
        for where in ("device", "pinned host"):
            src = torch.as_tensor(xp)
            dst = torch.full((n + GUARD, pad_out), F64_MARK, dtype=torch.float64)
            src, dst = (src.cuda(), dst.cuda()) if where == "device" else (src.pin_memory(), dst.pin_memory())
            assert call(n, src, pad_in, dst, pad_out) == A.RSIK_OK, (what, where, last_error(solver))
            solver.synchronize()  # rsik_sync: the host may read the pinned rows now
            out = dst.cpu().numpy()
            same_bits(out[:n, :need_out], packed[:n], f"{what} {where}: payload")
            assert (out[:n, need_out:] == F64_MARK).all(), f"{what} {where}: the padding columns of out were written"
            assert (out[n:] == F64_MARK).all(), f"{what} {where}: the guard rows of out were written"
    # refusals
    n = 65
    src = T(golden[:n], torch)
    dst = torch.full((n, need_out), F64_MARK, dtype=torch.float64, device="cuda")
    for in_stride, out_stride in ((need_in - 1, need_out), (need_in, need_out - 1)):
        assert call(n, src, in_stride, dst, out_stride) == A.RSIK_E_INVALID, (op, in_stride, out_stride)
        assert "rsik_stage" in last_error(solver), last_error(solver)
    solver.synchronize()
    assert bool((dst == F64_MARK).all()), f"stage {op}: a refused call wrote its output"
