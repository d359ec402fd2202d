"""The closed-form theta interval next to its own guard.

reach_impl forms both interval ends from ONE reciprocal square root of R'^4 disc (R'^2 = |N1 x N2|^2, disc = R'^2 - D'^2,
rsik_device.hpp "reach_line"); the guard in front of it hands over to the reference's arithmetic below R'^2 = 1e-12 and
|disc| = 1e-8.  Random workloads rarely come near either bound, so two families of poses are constructed here, for both arms:

  tangent   the pitch is walked to the reachable / "limited by wrist" boundary (bisection on the checker) and stepped back
            into the reachable side until 1e-8 <= disc <= 1e-6: the radicand of the new operation at its smallest.
  parallel  the hand axis N1 is tilted 1e-6 ... 3e-5 rad off the shoulder-wrist axis N2 of a nearly stretched arm: 1e-12 <= R'^2 <= 1e-9.  There
            disc <= R'^2 < 1e-8, so a reachable row has disc < 0 (the whole circle): |disc| in 1e-8 ... 1e-6 cannot hold
            together with this range of R'^2 on a row whose interval has two ends, which is why the families are separate.

R'^2 and disc of every row are measured with the checker alone (its solver state and its interval): N1 = (wrist - goal) /
|wrist - goal|, N2 = the circle normal, R'^2 = |N1 x N2|^2, and, for an interval of width W, disc = R'^2 sin^2(W / 2).
Bars are those of tests/test_gpu_parity.py (test_interval_closed_form_hands_over_at_decision_boundaries): flags and states
bit-exact, joints and interval ends within TOL = 1e-9, interval ends of arcs narrower than 1e-3 rad within 1e-7."""
import functools

import numpy as np
import pytest

from checker_support import default_arms
from compare import TOL
from oracle import oracle as orc

TIGHT_TOL = 1e-7    # tests/test_gpu_parity.py: interval ends next to tangency (d angle ~ d disc / (2 sqrt(disc)))
ARMS = ("r_arm", "l_arm")


def _solve(o, arm, P, E, **kw):
    ar, al = default_arms()
    aid = np.full(len(P), ARMS.index(arm), dtype=np.uint8)
    return o.solve_batch(ar, al, P, E, arm_id=aid, **kw)


def measure(o, arm, P, E):
    """(R'^2, disc, reachable, state, interval) per row, from the checker alone."""
    A = default_arms()[ARMS.index(arm)]
    sv = o.Solver(A)
    n = len(P)
    R2, disc, ok, st, itv = np.empty(n), np.empty(n), np.empty(n, bool), np.empty(n, int), np.empty((n, 2))
    for k in range(len(P)):
        ok[k], itv[k], st[k] = sv.is_reachable(P[k], E[k])
        goal, wrist, n2 = sv.buf[0:3], sv.buf[6:9], sv.buf[13:16]
        n1 = (wrist - goal) / np.linalg.norm(wrist - goal)
        c = np.cross(n1, n2 / np.linalg.norm(n2))
        R2[k] = c @ c
        width = (itv[k, 1] - itv[k, 0]) % (2 * np.pi) if ok[k] else np.nan
        disc[k] = R2[k] * np.sin(0.5 * width) ** 2
    return R2, disc, ok, st, itv


def tangent_family(o, arm, n_bases=32, per_base=160, seed=5):
    rng = np.random.default_rng(seed + ARMS.index(arm))
    side = -1.0 if arm == "r_arm" else 1.0
    P, E = [], []
    bases = 0
    while bases < n_bases:
        pos = np.array([0.0, 0.2 * side, 0.0]) + rng.uniform(-0.5, 0.5, 3)
        eul = rng.uniform(-np.pi, np.pi, 3)
        pitches = np.linspace(-np.pi, np.pi, 181)
        Pp = np.tile(pos, (len(pitches), 1))
        Ee = np.tile(eul, (len(pitches), 1))
        Ee[:, 1] = pitches
        st = _solve(o, arm, Pp, Ee, theta_policy=3)["state"]
        idx = [k for k in range(len(pitches) - 1) if {int(st[k]), int(st[k + 1])} == {0, 4}]
        if not idx:
            continue
        a, b, sa = pitches[idx[0]], pitches[idx[0] + 1], int(st[idx[0]])
        for _ in range(60):  # the boundary pitch to its last bit
            m = 0.5 * (a + b)
            e = eul.copy(); e[1] = m
            if int(_solve(o, arm, pos[None], e[None], theta_policy=3)["state"][0]) == sa:
                a = m
            else:
                b = m
        # state(a) == sa, state(b) != sa: the reachable end of the bracket, and the direction that leads away from the other end
        inner, sgn = (a, np.sign(a - b)) if sa == 0 else (b, np.sign(b - a))
        # disc grows linearly with the distance from tangency: offsets spread over the decades that can land in 1e-8 ... 1e-6
        for off in 10.0 ** rng.uniform(-9.5, -4.5, per_base):
            e = eul.copy(); e[1] = inner + sgn * off
            P.append(pos); E.append(e)
        bases += 1
    P, E = np.array(P), np.array(E)
    R2, disc, ok, st, itv = measure(o, arm, P, E)
    keep = ok & (st == 0) & (disc >= 1e-8) & (disc <= 1e-6)
    return P[keep], E[keep], R2[keep], disc[keep]


def _rotation_taking(a, b, roll):
    """A rotation R with R a = b (unit vectors), composed with a turn of `roll` about a."""
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)

    def about(axis, ang):
        x, y, z = axis / np.linalg.norm(axis)
        K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
        return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)

    v = np.cross(a, b)
    s, c = np.linalg.norm(v), a @ b
    if s < 1e-12:
        perp = np.cross(a, [1.0, 0.0, 0.0] if abs(a[0]) < 0.9 else [0.0, 1.0, 0.0])
        R = np.eye(3) if c > 0 else about(perp, np.pi)
    else:
        R = about(v, np.arctan2(s, c))
    return R @ about(a, roll)


def parallel_family(o, arm, n=2500, seed=9):
    rng = np.random.default_rng(seed + ARMS.index(arm))
    A = default_arms()[ARMS.index(arm)]
    s = A.field("shoulder_position")
    tip = A.field("tip_position")
    tl = np.array([-tip[0], tip[1], tip[2]])  # the wrist seen from the goal frame (symbolic_ik.py:418-425)
    side = -1.0 if arm == "r_arm" else 1.0
    P, E = [], []
    for _ in range(n):
        # the hand in line with a nearly stretched arm, pointing away from the shoulder (N1 = -N2 tilted by gamma): inside the
        # wrist-limit cone from a shoulder-wrist distance of ~0.42 m on; (u + f = 0.56 m)
        n2 = np.array([1.0, 0.3 * side, -0.3]) + rng.uniform(-0.6, 0.6, 3)
        n2 /= np.linalg.norm(n2)
        wrist = s + rng.uniform(0.44, 0.55) * n2
        perp = np.cross(n2, rng.normal(size=3))
        perp /= np.linalg.norm(perp)
        gamma = 10.0 ** rng.uniform(-5.95, -4.55)  # sin^2 in 1.3e-12 ... 8e-10
        n1 = -(np.cos(gamma) * n2 + np.sin(gamma) * perp)
        R = _rotation_taking(tl, n1, rng.uniform(-np.pi, np.pi))
        E.append(o.euler_from_matrix_xyz(R[None])[0])
        P.append(wrist - R @ tl)
    P, E = np.array(P), np.array(E)
    R2, disc, ok, st, itv = measure(o, arm, P, E)
    keep = ok & (st == 0) & (R2 >= 1e-12) & (R2 <= 1e-9)
    return P[keep], E[keep], R2[keep], disc[keep]


@functools.lru_cache(maxsize=None)
def constructed(arm):
    o = orc
    return tangent_family(o, arm), parallel_family(o, arm)


@pytest.mark.parametrize("arm", ARMS)
def test_constructed_poses_sit_next_to_the_guard(arm):
    """CPU, checker alone: every constructed row is reachable and its R'^2 / disc lies in the range its family is named for."""
    o = orc
    (Pt, Et, R2t, dt), (Pp, Ep, R2p, dp) = constructed(arm)
    print(f"{arm}: tangent rows {len(Pt)} (disc {dt.min():.2e} ... {dt.max():.2e}, R'^2 >= {R2t.min():.2e}), "
          f"parallel rows {len(Pp)} (R'^2 {R2p.min():.2e} ... {R2p.max():.2e})")
    assert len(Pt) >= 1500 and len(Pp) >= 1500
    assert np.all((dt >= 1e-8) & (dt <= 1e-6)) and np.all(R2t >= 1e-12)
    assert np.all((R2p >= 1e-12) & (R2p <= 1e-9))
    # each decade of both ranges is populated
    for lo in (1e-8, 1e-7):
        assert np.sum((dt >= lo) & (dt < 10 * lo)) >= 100
    for lo in (1e-12, 1e-11, 1e-10):
        assert np.sum((R2p >= lo) & (R2p < 10 * lo)) >= 100
    for P, E in ((Pt, Et), (Pp, Ep)):
        ref = _solve(o, arm, P, E)
        assert np.all(ref["reachable"] == 1) and np.all(ref["state"] == 0)
        assert np.all(np.isfinite(ref["interval"])) and np.all(np.isfinite(ref["joints"]))


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ARMS)
def test_interval_ends_next_to_the_guard_match_the_checker(arm):
    import contextlib
    import io

    import torch

    from reachy2_symbolic_ik_amd import HipSolver, SymbolicIK

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    o = orc
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK(arm, singularity_offset=0.03, solver=HipSolver(0))
    for family, (P, E, _, _) in zip(("tangent", "parallel"), constructed(arm)):
        buf = torch.as_tensor(np.ascontiguousarray(np.concatenate([P.T, E.T], axis=0))).cuda()
        res = {k: v.cpu().numpy() for k, v in ik.solve_batch(buf).items()}
        ref = _solve(o, arm, P, E)
        np.testing.assert_array_equal(res["reachable"], ref["reachable"])
        np.testing.assert_array_equal(res["state"], ref["state"])
        assert np.all(ref["reachable"] == 1)  # no row is skipped below
        width = np.abs(((ref["interval"][:, 1] - ref["interval"][:, 0] + np.pi) % (2 * np.pi)) - np.pi)
        tight = width < 1e-3
        # +-pi name the same end of the whole circle
        d_itv = np.abs(res["interval"] - ref["interval"])
        d_itv = np.minimum(d_itv, np.abs(d_itv - 2 * np.pi))
        d_j = np.abs(res["joints"] - ref["joints"])
        print(f"{arm} {family}: rows {len(P)}, tight {int(tight.sum())}, interval err max {d_itv.max():.3e} "
              f"(wide rows {d_itv[~tight].max() if (~tight).any() else 0.0:.3e}), joints err max {d_j.max():.3e} "
              f"(wide rows {d_j[~tight].max() if (~tight).any() else 0.0:.3e})")
        if (~tight).any():
            assert d_itv[~tight].max() < TOL
        if tight.any():
            assert d_itv[tight].max() < TIGHT_TOL
        # the joints are evaluated at theta = interval[0] and inherit that end's conditioning: same split
        if (~tight).any():
            assert d_j[~tight].max() < TOL
        if tight.any():
            assert d_j[tight].max() < TIGHT_TOL
