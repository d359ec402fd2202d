"""Pins, on the CPU checker alone, what tests/test_gpu_far_inputs.py leans on: the workload of tests/far_inputs.py holds every
rung, sign and slot; its wound rows are (nearly all) reachable, so that joints are compared and not only flags; and the checker
answers a wound row exactly as it answers the row's reduced twin — the expected values do not hang on how this host's libm reduces
a huge argument, and no row sits on a decision margin."""
import numpy as np

import far_inputs as F
from checker_support import default_arms
from compare import TOL
from oracle import oracle as orc


def test_every_rung_sign_and_slot_is_present():
    w = F.wound_rows()
    n = len(w["pos"])
    assert n == len(F.RUNGS) * 2 * F.N_BASE * 2 and 2000 <= n <= 5000
    assert F.RUNGS[F.BOUND_RUNG] == 2.0 ** 27 and F.RUNGS[F.FIRST_BROKEN - 1] < 2 ** 26 * np.pi < F.RUNGS[F.FIRST_BROKEN]
    assert list(F.RUNGS) == sorted(F.RUNGS) and F.RUNGS[-1] == np.finfo(np.float64).max
    for g, rung in enumerate(F.RUNGS):
        for arm in (0, 1):
            for slot in range(4):
                for sign in (1.0, -1.0):
                    rows = np.flatnonzero((w["rung"] == g) & (w["arm"] == arm) & (w["slot"] == slot) & (w["sign"] == sign))
                    assert len(rows) >= 4, (rung, arm, slot, sign)
                    for q in ((0, 2) if slot == 3 else (slot,)):
                        v = w["eul"][rows, q]
                        assert (np.sign(v) == sign).all(), (rung, arm, slot, sign)
                        # wound to the rung: within a turn of it below 1e16, within a few hundred doubles of it from there on
                        near = 2 * np.pi + 0.5 if rung < F.WALKED_FROM else 1024 * (rung - np.nextafter(rung, 0.0))
                        assert (np.abs(np.abs(v) - rung) <= near).all(), (rung, arm, slot, sign)
                        # the two rungs at the edge keep to their side of it
                        assert F.SIDE.get(rung, 0) >= 0 or (np.abs(v) <= rung).all(), (rung, arm, slot, sign)
                        assert F.SIDE.get(rung, 0) <= 0 or (np.abs(v) >= rung).all(), (rung, arm, slot, sign)
    # the twin is the row with ordinary angles, and an angle that was not wound is left alone
    assert (np.abs(w["twin_eul"]) <= np.pi).all()
    for slot in range(3):
        others = [q for q in range(3) if q != slot]
        rows = w["slot"] == slot
        assert np.array_equal(w["eul"][rows][:, others], w["twin_eul"][rows][:, others])
    # both arms in every wave of a mixed launch
    assert ((w["arm"][: n - n % 64].reshape(-1, 64).sum(axis=1) == 32)).all()
    th, tw, rg = F.far_thetas()
    assert len(th) == 2 * len(F.RUNGS) and sorted(set(rg)) == list(range(len(F.RUNGS)))
    assert (np.sign(th).reshape(-1, 2) == [1.0, -1.0]).all() and (np.abs(tw) <= np.pi).all()
    assert (np.abs(th[rg == F.FIRST_BROKEN - 1]) < 2 ** 26 * np.pi).all() and (np.abs(th[rg == F.FIRST_BROKEN]) > 2 ** 26 * np.pi).all()
    assert any(2.0 ** 50 < r < 2.0 ** 53 for r in F.RUNGS)
    pos, eul, arm, val, entry = F.far_position_rows()
    assert {(abs(v), np.sign(v), e) for v, e in zip(val, entry)} == {(v, s, e) for v in F.FAR_POSITIONS for s in (1.0, -1.0) for e in range(4)}
    pos, eul, arm, val, entry = F.tiny_position_rows()
    seen = {(abs(v), bool(np.signbit(v)), e) for v, e in zip(val, entry)}
    assert seen == {(v, s, e) for v in F.TINY_POSITIONS for s in (False, True) for e in range(3)}


def test_reduction_is_the_angle():
    """reduce_angle against libm where libm is exact enough to say (moderate angles), and its own precision rule at the top."""
    rng = np.random.default_rng(3)
    x = rng.uniform(-1e6, 1e6, size=2000)
    r = F.reduce_angles(x)
    assert np.max(np.abs(np.sin(r) - np.sin(x))) < 1e-15 and np.max(np.abs(np.cos(r) - np.cos(x))) < 1e-15
    import mpmath as mp

    for v in (1e22, 1e100, 1e300, F.DBL_MAX, -F.DBL_MAX):
        with mp.workdps(700):
            want = mp.mpf(v) - 2 * mp.pi * mp.nint(mp.mpf(v) / (2 * mp.pi))
            assert abs(want - mp.mpf(F.reduce_angle(v))) < mp.mpf(2) ** -51, v


def test_wound_rows_are_reachable_and_equal_their_reduced_twins():
    w = F.wound_rows()
    ar, al = default_arms(F.SINGULARITY_OFFSET)
    th = np.tile(np.array([0.3, -2.0]), len(w["pos"]) // 2)
    for policy, theta_in in ((0, None), (1, th)):
        a = orc.solve_batch(ar, al, w["pos"], w["eul"], arm_id=w["arm"], theta_policy=policy, theta_in=theta_in)
        b = orc.solve_batch(ar, al, w["pos"], w["twin_eul"], arm_id=w["arm"], theta_policy=policy, theta_in=theta_in)
        for k in ("reachable", "state", "projected"):
            assert np.array_equal(a[k], b[k]), (policy, k, np.flatnonzero(a[k] != b[k])[:10])
        for k in ("joints", "interval", "elbow"):
            assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), (policy, k)
            assert np.nanmax(np.abs(a[k] - b[k])) <= TOL, (policy, k, np.nanmax(np.abs(a[k] - b[k])))
    for g, rung in enumerate(F.RUNGS):
        share = a["reachable"][w["rung"] == g].mean()
        assert share >= 0.9, (rung, share)


def test_far_thetas_equal_their_reduced_twins():
    """An explicit theta of any size is the theta it is congruent to (get_joints takes its sine and cosine only)."""
    th, tw, rg = F.far_thetas()
    pos0, eul0 = F.base_poses("r_arm")
    ar, al = default_arms(F.SINGULARITY_OFFSET)
    k = len(th)
    pos, eul = np.repeat(pos0[:8], k, axis=0), np.repeat(eul0[:8], k, axis=0)
    a = orc.solve_batch(ar, al, pos, eul, theta_policy=1, theta_in=np.tile(th, 8))
    b = orc.solve_batch(ar, al, pos, eul, theta_policy=1, theta_in=np.tile(tw, 8))
    assert a["reachable"].mean() > 0.8 and np.array_equal(a["projected"], b["projected"])
    for key in ("joints", "elbow"):
        assert np.nanmax(np.abs(a[key] - b[key])) <= TOL, key


def test_far_positions_are_answered_in_their_row():
    """A position whose squared distance from the shoulder overflows: the norm is infinite, the direction 0 and the goal the
    shoulder itself, which lies behind the backward limit of the default arm; below that it is projected onto the sphere."""
    pos, eul, arm, val, entry = F.far_position_rows()
    ar, al = default_arms(F.SINGULARITY_OFFSET)
    ref = orc.solve_batch(ar, al, pos, eul, arm_id=arm)
    assert (ref["reachable"] == 0).all() and np.isnan(ref["joints"]).all()
    over = np.abs(val) >= 2e154
    both = np.abs(val) == 1e154      # three entries at 1e154 overflow, one does not
    assert (ref["state"][over] == 2).all()
    assert (ref["state"][both & (entry == 3)] == 2).all()
    rest = ~over & ~(both & (entry == 3))
    ahead = rest & ((entry == 0) | (entry == 3)) & (val > 0)
    assert (ref["state"][ahead] == 1).all()                  # projected onto the sphere in front of the torso: out of reach
    assert (ref["state"][rest & ~ahead] == 2).all()          # ... behind it, or sideways with x next to 0: backward
    pos, eul, arm, val, entry = F.tiny_position_rows()
    ref = orc.solve_batch(ar, al, pos, eul, arm_id=arm)
    assert set(ref["state"]) <= {0, 1, 2, 3, 4, 6} and 0 < ref["reachable"].mean()
