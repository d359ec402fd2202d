"""What the GPU tests share: the fixtures, the solvers they launch on, tensors in the ABI's layouts, one way to an entry point of
the C ABI on the caller's own buffers, and the comparisons that several GPU test files hold their launches to.  torch and the
package are imported inside functions and fixtures, so importing this module needs neither.  No test in this file: pytest does not
rewrite its asserts, so every one of them carries its own message."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

import scale_inputs as SC
import theta_workload as W
from checker_support import default_arms
from compare import close
from oracle import oracle as _oracle

URDF = "config_files/reachy2_ik_minimal.urdf"
SIX_PI = 6 * np.pi
EXACT = 1e-12   # theta and bracket of the theta-from-joints search where its decisions agree


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def orc():
    return _oracle


def abi():
    from reachy2_symbolic_ik_amd import _abi

    return _abi


# ------------------------------------------------------------------------------------------ solvers
def make_symbolic(so):
    """(HipSolver, SymbolicIK r, SymbolicIK l) on one context."""
    from reachy2_symbolic_ik_amd import HipSolver, SymbolicIK

    solver = HipSolver(0)
    with contextlib.redirect_stdout(io.StringIO()):
        r = SymbolicIK("r_arm", singularity_offset=so, solver=solver)
        l = SymbolicIK("l_arm", singularity_offset=so, solver=solver)
    return solver, r, l


def make_symbolic_dual(so=0.03):
    """(HipSolver, SymbolicIK r, DualArmIK) on one context, both arms uploaded."""
    from reachy2_symbolic_ik_amd import DualArmIK, HipSolver, SymbolicIK

    solver = HipSolver(0)
    with contextlib.redirect_stdout(io.StringIO()):
        r = SymbolicIK("r_arm", singularity_offset=so, solver=solver)
        r._upload()
        SymbolicIK("l_arm", singularity_offset=so, solver=solver)._upload()
        dual = DualArmIK(solver=solver, singularity_offset=so)
    return solver, r, dual


def make_control(is_dvt=False):
    from reachy2_symbolic_ik_amd import ControlIK

    with contextlib.redirect_stdout(io.StringIO()):
        return ControlIK(urdf_path=URDF, is_dvt=is_dvt)


# ------------------------------------------------------------------------------------------ tensors
def T(a, torch):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def soa(pos, eul, torch):
    return torch.as_tensor(np.ascontiguousarray(np.concatenate([pos.T, eul.T], axis=0))).cuda()


def m12(M, torch):
    from reachy2_symbolic_ik_amd.control_ik import matrices_to_m12_soa

    return matrices_to_m12_soa(M, torch.device("cuda", 0))


def goal_tensor(goal_kind, pos, eul, torch):
    if goal_kind == "pose":
        return soa(pos, eul, torch)
    return m12(SC.matrices_from_pose(pos, eul), torch)


def to_np(res):
    """The tensors of a result on the host (a result may also hold entries that are not tensors: they are left out)."""
    return {k: v.cpu().numpy() for k, v in res.items() if hasattr(v, "cpu")}


KINDS = ("r", "l", "mixed")   # the arrangements of a launch: one arm for all rows, or an arm byte per row


def arm_kwargs(kind, arm, torch):
    """How an arrangement reaches the ABI: arm = NULL + arm_uniform (kernel<false>) or one byte per row (kernel<true>)."""
    if kind == "mixed":
        return dict(arm=T(arm, torch))
    return dict(arm=None, arm_uniform=int(kind == "l"))


# ------------------------------------------------------------------------------------------ the C ABI on the caller's own buffers
def ptr(t):
    return None if t is None else t.data_ptr()


def cols(t, rows):
    """The ABI's column table of an SoA tensor [rows, n]; NULL for None."""
    return None if t is None else (C.c_void_p * rows)(*[t[k].data_ptr() for k in range(rows)])


def raw_call(solver, fn_name, *cargs):
    """One entry point of the C ABI on the caller's own buffers, on the solver's device and stream: returns the ABI's code."""
    import torch

    with torch.cuda.device(solver.device):
        solver._bind_stream()
        return getattr(solver.lib, fn_name)(solver._h, *cargs)


def last_error(solver):
    return (solver.lib.rsik_last_error(solver._h) or b"").decode()


# ------------------------------------------------------------------------------------------ two runs of the same thing
def _bits_equal(torch, a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _rows_except(torch, n, rows):
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[torch.as_tensor(rows, device="cuda")] = False
    return keep


def _same_run(torch, ref, got, tag, joint_tol=1e-9):
    """Two runs of the same trajectories (pipeline vs step kernel, or two block sizes of the pipeline): flags, state codes,
    the carried theta (row 0 of the trajectory state) and its flag rows bit for bit; joints and previous_sol to
    `joint_tol`.  (The pipeline's joints phase writes a quiet step as raw joint + whole turns instead of previous +
    angle_diff(raw, previous) and rebuilds the goal rotation's third row from the other two: both within the last bit of
    their inputs, no accumulation — but where the arm is stretched out the elbow-yaw / wrist-yaw split amplifies a last bit
    2e4 times and more (see test_control_continuous_golden_default_start; 1.2e-10 over 32 M eventful trajectory-steps,
    scripts/soak_pipeline.py), hence 1e-9 and not 1e-14.)"""
    for k in ref:
        a, b = ref[k], got[k]
        if k == "joints":
            assert float((a - b).abs().max()) <= joint_tol, (tag, k, float((a - b).abs().max()))
        elif k == "cont_state":
            assert torch.equal(a[0].view(torch.uint8), b[0].view(torch.uint8)), (tag, "previous_theta")
            assert float((a[1:8] - b[1:8]).abs().max()) <= joint_tol, (tag, "previous_sol")
            assert torch.equal(a[8:11], b[8:11]), (tag, "init / emergency / has_previous_sol")
        else:
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (tag, k)


# ------------------------------------------------------------------------------------------ inputs drawn on the device or per row
def _eventful_trajectories(torch, n_traj, n_steps, seed, arm):
    """[n_steps, 12, n_traj] goal matrices: config 5's sinusoids plus, per trajectory, one of: a jump of the goal, a winding
    wrist (reaches the +-6 pi limit), a stretch far out of reach, a run of exact repeats ("stay" steps) — what makes the
    sequential phases take their rare paths (scripts/soak_pipeline.py's generator, smaller)."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *sh: torch.rand(*sh, generator=g, dtype=torch.float64).to(dev)  # noqa: E731
    k = torch.arange(n_steps, dtype=torch.float64, device=dev)[:, None]
    t = k / 60.0 + 11.0 + r(n_traj)[None, :] * 40.0
    c0 = [0.45, -0.2 if arm == "r_arm" else 0.2, -0.1, 0.0, -np.pi / 2, 0.0]
    amp = [0.3, 0.3, 0.3, np.pi / 4, np.pi / 4, np.pi / 4]
    freq = [0.6, 0.34, 0.78, 0.18, 0.31, 0.47]
    v = [c + a * torch.sin(f * t) for c, a, f in zip(c0, amp, freq)]
    kind = (r(n_traj) * 6).floor()
    at = (r(n_traj) * max(n_steps - 20, 1) + 5).floor()
    after = (k >= at[None, :]).double()
    v[0] = v[0] + after * (kind < 2).double()[None, :] * 0.25 * (r(n_traj)[None, :] - 0.5)
    v[5] = v[5] + (kind == 2).double()[None, :] * k * 0.12 + (kind == 3).double()[None, :] * k * -0.2
    far = ((k >= at[None, :]) & (k < at[None, :] + 25)).double() * (kind == 4).double()[None, :]
    v[0] = v[0] + far * 2.0
    hold = ((k >= at[None, :]) & (k < at[None, :] + 6)).double() * (kind == 5).double()[None, :]
    idx = torch.where(hold.bool(), at[None, :].expand(n_steps, -1), k.expand(-1, n_traj)).long().clamp(max=n_steps - 1)
    v = [torch.gather(x, 0, idx) for x in v]
    ca, sa, cb, sb, cc, sc = torch.cos(v[3]), torch.sin(v[3]), torch.cos(v[4]), torch.sin(v[4]), torch.cos(v[5]), torch.sin(v[5])
    rows = [cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa, sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa,
            -sb, cb * sa, cb * ca, v[0], v[1], v[2]]
    return torch.stack(rows, dim=1).contiguous()


def wrist_pitch(rng, n):
    """Wrist pitch of a previous solution: inside the Orbita3D cone, as every solution is (safety_checks).  A pitch beyond
    +-pi/2 is the other Euler form of the same wrist (roll and yaw turned by pi): a pose that falls back to previous_sol
    then lands exactly between two turns of allow_multiturn, and which one it takes rests on the last ulp of the wrist's
    sin / cos, which the per-row kernels evaluate on the device (include/rsik.h)."""
    return rng.uniform(-0.7, 0.7, size=n)


def bucket_vectors(rng, B):
    """B distinct previous_sol vectors, uniform in +-5 pi per joint; an eighth of them put joints 0, 2 and 6 just inside
    +-6 pi (as G11 does), so that allow_multiturn carries the new joints past the limit and every emergency bit trips."""
    v = rng.uniform(-5 * np.pi, 5 * np.pi, size=(B, 7))
    v[:, 5] = wrist_pitch(rng, B)
    edge = np.arange(B) % 8 == 0
    for k in (0, 2, 6):
        v[edge, k] = rng.choice([-1.0, 1.0], size=int(edge.sum())) * (SIX_PI - rng.uniform(0.05, 1.0, size=int(edge.sum())))
    return v


# ------------------------------------------------------------------------------------------ theta from joints against the checker
def check_against_checker(got, ref, so, pos, eul, arm, cur, what, pref=W.PREFERRED, arms=None):
    """theta / bracket / joints / distance / state of a fused launch against checker_batch's answer; returns the near ties.
    arms: the checker's (r, l) arms of the launch, the default arms with offset `so` where None."""
    n = len(pos)
    assert ref["ok"].all(), (what, "the checker refused rows", np.flatnonzero(~ref["ok"])[:10].tolist())
    np.testing.assert_array_equal(got["state"], np.zeros(n, dtype=np.uint8), err_msg=what)
    dth = np.abs(got["theta"] - ref["theta"])
    print(f"{what}: theta max diff {np.nanmax(dth):.3e}, rows beyond 1e-12: {int((dth > EXACT).sum())} of {n}")
    odd = np.flatnonzero(~(dth <= EXACT))
    assert len(odd) <= n // 10000, (what, len(odd))
    arms = arms or default_arms(so)
    for i in odd:  # a mismatch that is not a near tie fails
        p = pref[int(arm[i])]
        base = W.replay_row(arms, pos[i], eul[i], arm[i], cur[i], p)
        ks = [k for k, m in enumerate(base["margins"]) if m <= W.NEAR_TIE]
        print(f"{what}: row {i} device theta {got['theta'][i]!r} checker {ref['theta'][i]!r} smallest margin {min(base['margins']):.3e}")
        assert ks, (what, i, "theta differs and no comparison of the search is a near tie")
        flipped = [W.replay_row(arms, pos[i], eul[i], arm[i], cur[i], p, flip=k)["theta"] for k in ks]
        assert any(abs(t - got["theta"][i]) <= EXACT for t in flipped), (what, i, got["theta"][i], flipped)
    same = np.ones(n, dtype=bool)
    same[odd] = False
    want_br = W.bracket_of(np.where(ref["shortcut"], np.nan, ref["theta"]), arm)
    assert np.array_equal(np.isnan(want_br[:, 0]), ref["shortcut"]), (what, "brackets and shortcut rows disagree")
    close(got["bracket"][same], want_br[same], what + " bracket", tol=EXACT)
    still = same & ~ref["moved"]
    close(got["joints"][still], ref["joints"][still], what + " joints (state not moved)")
    close(got["distance"][still], ref["distance"][still], what + " distance (state not moved)")
    moved = np.flatnonzero(same & ref["moved"])[:256]  # the rows a projection moved: replayed evaluation by evaluation
    if len(moved):
        rep = [W.replay_row(arms, pos[i], eul[i], arm[i], cur[i], pref[int(arm[i])]) for i in moved]
        close(got["joints"][moved], np.array([r["joints"] for r in rep]), what + " joints (moved rows, replayed)")
        close(got["distance"][moved], np.array([r["distance"] for r in rep]), what + " distance (moved rows, replayed)")
    return odd
