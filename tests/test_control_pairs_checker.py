"""Pins what tests/test_gpu_control_arm_pairs.py leans on, on the CPU checker alone: for every control pair of tests/arm_pairs.py and
the threshold family, on exactly the inputs the GPU tests launch, the conditions those tests rely on hold — they are conditions on
the inputs, not measurements, and every count is printed before it is asserted (pytest -s shows them).  The constant blocks of every
pair are what its name says (FORM of rsik_theta_from_joints, PLANE of the control kernels, restated from csrc/rsik_lib.hip), without a
device."""
import numpy as np
import pytest

import control_workload as W
import theta_workload as TW
from arm_pairs import (CONTROL_PAIRS, PAIRS, S3, check_blocks, check_control_blocks, checker_arms, control_expectation, packed_blocks,
                       plane_binds, plane_margin, threshold_family, threshold_offset, threshold_offsets)
from oracle import oracle as orc

ALL_PAIRS = list(CONTROL_PAIRS) + list(threshold_family())


@pytest.fixture(scope="module")
def rows(golden_dir):
    return W.control_rows(golden_dir)


def test_the_control_pairs_launch_what_their_names_say():
    s = threshold_offset()
    assert abs(s - (-0.3705)) < 1e-4, s
    fam = threshold_family()
    assert [plane for _, plane in fam.values()] == [False, True, True] and len(fam) == 3
    for pair in ALL_PAIRS:
        blocks = packed_blocks(pair)
        check_control_blocks(pair, blocks)   # FORM and PLANE of every pair, with singularity_plane_binds restated
        if pair in PAIRS:
            check_blocks(pair, blocks)
        form, plane = control_expectation(pair)
        assert plane_binds(blocks) == plane, pair
        print(f"{pair}: FORM {form}, PLANE {plane}, rhs - reach_max {[round(plane_margin(b), 6) for b in blocks]}")
    # the two offsets the suite had before sit 0.64 m and 0.40 m on either side of the threshold; the family sits 1e-3 on either side
    for so, margin in ((-1.01, 0.64), (0.03, -0.40)):
        b = packed_blocks(f"default@{so}/default@{so}")
        assert abs(plane_margin(b[0]) - margin) < 0.005 and plane_binds(b) == (margin < 0)
    near = [plane_margin(packed_blocks(pair)[0]) for pair in list(fam)[:2]]
    assert abs(near[0] - 1e-3) < 1e-12 and abs(near[1] + 1e-3) < 1e-12, near
    assert [checker_arms(pair)[0].field("singularity_offset") for pair in fam] == [s - 1e-3, s + 1e-3, S3]
    # upload() and checker_arms() read the same dict: the checker's arm carries the override too
    a, b = checker_arms("default@-1.01/default@0.03")
    assert a.field("singularity_offset") == -1.01 and b.field("singularity_offset") == 0.03 and b.field("side") == -1.0
    a, b = checker_arms("default@-1.01/ztip@-1.01")
    assert b.field("singularity_offset") == -1.01 and b.field("singularity_limit_coeff") == 0.8 and b.field("upper_arm_size") == 0.30


@pytest.mark.parametrize("pair", ALL_PAIRS)
def test_discrete_inputs(rows, pair):
    """The 1000 rows: every state rsik_control_discrete can return occurs at least 20 times per arm; after the shortcut failed, both
    "the search found a theta" and "the search failed" occur on each arm; for every nb_search_points and preferred angle the GPU test
    uses, at most 0.5 % of the rows rest on a margin below 1e-9 (only such rows could be set aside on the GPU; these inputs have none, and the GPU test
    compares every row)."""
    M, arm = rows
    assert M.shape == (W.N, 4, 4) and np.array_equal(M[0::2], M[1::2]) and np.array_equal(arm[:4], [0, 1, 0, 1])
    arms = checker_arms(pair)
    ref = W.checker_discrete(arms, M, arm, 64, 0, W.PREFERRED[0])
    s = W.search_rows(arms, M, arm, 64, W.PREFERRED[0])
    np.testing.assert_array_equal(s["reach"] & (s["shortcut"] | s["found"]), ref["reachable"] != 0)   # the replay is the checker's search
    for a in (0, 1):
        m = arm == a
        counts = [int((ref["state"][m] == k).sum()) for k in W.STATES]
        ran = m & s["reach"] & ~s["shortcut"]
        found, failed = int((ran & s["found"]).sum()), int((ran & ~s["found"]).sum())
        print(f"{pair} {'rl'[a]}: states {dict(zip(W.STATES, counts))}, shortcut {int((m & s['shortcut']).sum())}, found {found}, failed {failed}")
        assert min(counts) >= 20 and sum(counts) == m.sum(), (pair, a, counts)
        assert found >= 20 and failed >= 20, (pair, a, found, failed)
        assert W.POPULATIONS[pair][a] == (counts, found, failed), (pair, a)   # the counts the helper module records
    # One search per (nb_search_points, preferred angle) stands for every launch the GPU test makes with them: the search sees
    # neither the constrained mode (the preferred theta an arm searches around is the same in both) nor previous_sol.
    for a in arms:
        for pref in W.PREFERRED:
            assert orc.interval_limit(a, 0, pref)[2] == orc.interval_limit(a, 1, pref)[2]
    for nb in W.NBS:
        for pref in W.PREFERRED:
            hinge = W.search_rows(arms, M, arm, nb, pref)["margin"] < W.HINGE
            print(f"{pair} nb {nb} preferred {pref:.3f}: rows on a margin below {W.HINGE}: {int(hinge.sum())}")
            assert hinge.mean() <= W.HINGE_SHARE, (pair, nb, pref)
    if pair == "default@-1.01/default@0.03":
        differ = int((ref["state"][0::2] != ref["state"][1::2]).sum())
        same_plane = W.checker_discrete(checker_arms("default@0.03/default@0.03"), M, arm, 64, 0, W.PREFERRED[0])
        by_plane = int((ref["state"][0::2] != same_plane["state"][0::2]).sum())
        print(f"{pair}: the r and l rows of a matrix differ in state on {differ} matrices; {by_plane} r rows change state with the r plane")
        assert differ >= 20 and by_plane >= 10


def test_threshold_family(rows):
    """s3: the plane half of is_elbow_ok fails on between 1 % and 10 % of the grid points the search evaluates (arm_pairs.S3 records
    the share).  s* - 1e-3: it fails on none, which is what lets the launch drop it.  s* + 1e-3: on the 1000 rows it decides nothing, so
    the family launches control_workload.cap_rows too, where it decides at least 20 rows per arm for every launch the GPU test makes."""
    M, arm = rows
    below, above, third = list(threshold_family())
    assert third == "default@s3/default@s3" and threshold_offsets()["s3"] == S3 == checker_arms(third)[1].field("singularity_offset")
    s = W.search_rows(checker_arms(third), M, arm, 64, W.PREFERRED[0])
    share = s["plane_fail"].sum() / s["grid"].sum()
    per_arm = [s["plane_fail"][arm == a].sum() / s["grid"][arm == a].sum() for a in (0, 1)]
    print(f"s3 = {S3}: the plane fails on {share:.4f} of the evaluated grid points (r {per_arm[0]:.4f}, l {per_arm[1]:.4f})")
    assert 0.01 <= share <= 0.10 and abs(share - 0.0418) < 5e-5
    s = W.search_rows(checker_arms(below), M, arm, 100, W.PREFERRED[0])
    assert s["plane_fail"].sum() == 0 and s["grid"].sum() > 10000
    # s* + 1e-3: the plane cuts a cap 0.7 mm high and 2 cm in radius off the upper-arm sphere, and no answer on the 1000 rows changes
    from reachy2_symbolic_ik_amd import constants as K
    for b in packed_blocks(above):
        h = -plane_margin(b) / np.sqrt(1.0 + b[K.C_SING_COEFF] ** 2)
        radius = np.sqrt(2.0 * b[K.C_UPPER_ARM] * h - h * h)
        print(f"s* + 1e-3: the plane cuts a cap {h * 1e3:.3f} mm high, {radius * 1e2:.2f} cm in radius")
        assert abs(h - 0.707e-3) < 1e-6 and abs(radius - 0.0199) < 1e-4
    on_rows = [W.checker_discrete(checker_arms(pair), M, arm, 64, 0, W.PREFERRED[0]) for pair in (below, above)]
    for key in on_rows[0]:
        np.testing.assert_array_equal(on_rows[0][key], on_rows[1][key])
    Mc, armc = W.cap_rows()
    no_plane = checker_arms("default@-1.01/default@-1.01")
    for nb in W.NBS:
        for pref in W.PREFERRED:
            with_plane = W.checker_discrete(checker_arms(above), Mc, armc, nb, 0, pref)
            without = W.checker_discrete(no_plane, Mc, armc, nb, 0, pref)
            decided = (with_plane["state"] != without["state"]) | (np.abs(with_plane["joints"] - without["joints"]).max(axis=1) > 1e-6)
            same = W.checker_discrete(checker_arms(below), Mc, armc, nb, 0, pref)
            print(f"s* + 1e-3, nb {nb}, preferred {pref:.3f}: the plane decides {int(decided[armc == 0].sum())} r and {int(decided[armc == 1].sum())} l rows")
            assert decided[armc == 0].sum() >= 20 and decided[armc == 1].sum() >= 20
            for key in same:  # and s* - 1e-3 is the arm without a plane
                np.testing.assert_array_equal(same[key], without[key])


@pytest.mark.parametrize("pair", list(CONTROL_PAIRS) + list(threshold_family())[:2])
def test_trajectory_inputs(pair):
    """The 96 x 25 jumpy trajectories with an arm byte per trajectory: on each arm at least one trajectory latches the emergency stop,
    at least one takes the unreachable fallback without latching, and reachable steps are the majority."""
    Ms, arm, start_j, start_pose = W.trajectories()
    assert Ms.shape == (W.N_TRAJ, W.N_STEPS, 4, 4) and 0 < arm[:64].sum() < 64 and 0 < arm[64:].sum() < 32
    ref = W.checker_trajectories(checker_arms(pair), Ms, arm, start_j, start_pose)
    for a in (0, 1):
        m = arm == a
        latched = ref["latched"][-1][m]
        fallback = ((ref["reachable"] == 0) & ~ref["latched"])[:, m].any(axis=0)
        print(f"{pair} {'rl'[a]}: {int(latched.sum())} trajectories latch, {int(fallback.sum())} take the unreachable fallback, "
              f"reachable steps {ref['reachable'][:, m].mean():.3f}, states {np.unique(ref['state'][:, m]).tolist()}")
        assert latched.sum() >= 1 and fallback.sum() >= 1 and (~latched).sum() >= 1 and ref["reachable"][:, m].mean() > 0.5


THETA_PAIRS = ("default/custom", "ztip/default", "default@-1.01/ztip@-1.01", "default@-1.01/default@0.03", "custom/custom")


@pytest.mark.parametrize("pair", THETA_PAIRS)
def test_theta_from_joints_inputs(pair):
    """theta_workload's rows at n = 300 on the pair's arms: is_reachable_no_limits accepts every row, both arms hold a third of the
    rows at least, shortcut rows and searched rows both occur, and no comparison of any row's search is a near tie."""
    arms = checker_arms(pair)
    pos, eul, arm, cur = TW.theta_workload(TW.SEED + 7, 300, arms=arms)
    ref = TW.checker_batch(None, pos, eul, arm, cur, arms=arms)
    ties = TW.near_ties(arms, pos, eul, arm, cur)
    print(f"{pair}: {int(arm.sum())} l rows, shortcut {int(ref['shortcut'].sum())}, moved {int(ref['moved'].sum())}, near ties {ties}")
    assert ref["ok"].all() and 100 < arm.sum() < 200 and ref["shortcut"].sum() >= 10 and (~ref["shortcut"]).sum() >= 200 and not ties
    assert control_expectation(pair)[0] == (2 if pair == "custom/custom" else 1)
