"""Pins what tests/test_gpu_arm_forms.py leans on, on the CPU checker alone: for every arm pair of tests/arm_pairs.py, and on
exactly the inputs the GPU tests launch, the conditions those tests rely on hold — they are conditions on the inputs, not
measurements, and every share is printed before it is asserted (pytest -s shows them).  The constant blocks of every pair are what
its name says (FORM and TIPZ of the launch, restated from csrc/rsik_lib.hip), without a device."""
import numpy as np
import pytest

import nearest_workload as NW
import path_workload as PW
from arm_pairs import NON_MIRROR, PAIRS, check_blocks, checker_arms, launch_of, packed_blocks
from oracle import oracle as orc
from sweep_workload import expected_tiled, sweep_poses, sweep_thetas

N = 1000
KS = (1, 3, 8, 70)  # 1 and 8: solve and sweep against the checker; 3 and 70: nearest (tests/test_gpu_arm_forms.py)


def test_the_pairs_launch_what_their_names_say():
    assert set(NON_MIRROR) == {"custom/default", "default/custom", "default/ztip", "ztip/default"} and N == NW.N_MAIN
    for pair, (form, form_no_mirror, tipz) in PAIRS.items():
        blocks = packed_blocks(pair)
        check_blocks(pair, blocks)
        print(f"{pair}: FORM {form} ({form_no_mirror} under NO_MIRROR), TIPZ {tipz}")
    default = packed_blocks("default/ztip")[0], packed_blocks("ztip/default")[1]
    assert launch_of(default) == (2, True), "the default pair is a mirror pair with both tips on z"
    a, b = checker_arms("default/ztip")
    assert a.field("upper_arm_size") == 0.28 and b.field("upper_arm_size") == 0.30 and b.field("side") == -1.0


@pytest.mark.parametrize("pair", list(PAIRS))
def test_sweep_and_nearest_inputs(pair):
    """sweep_poses("mixed", 500 + K, 1000) — nearest_workload.main_case's poses — with a theta column per pose, both policies: the
    reachable share is at least 0.04 on the even rows and above 0.5 on the odd ones, all five states occur, between 5 % and 95 % of
    the reachable samples project, one pose has both kinds among its own samples (K > 1), and nearest's gap condition holds."""
    arms = checker_arms(pair)
    for k in KS:
        pos, eul, arm, seed = NW.main_case("mixed", k)
        p2, e2, a2 = sweep_poses("mixed", 500 + k, N)
        assert np.array_equal(pos, p2) and np.array_equal(eul, e2) and np.array_equal(arm, a2) and 0 < arm.sum() < N
        for policy in ("fraction", "explicit"):
            thetas = NW.main_thetas(policy, True, k)
            assert np.array_equal(thetas, sweep_thetas(policy, True, k, N, 600 + k))
            ref = expected_tiled(orc, arms, pos, eul, arm, policy, thetas, nthreads=4)
            ok = ref["reachable"].astype(bool)
            pr = ref["projected"][:, ok]
            both = int(((pr.max(axis=0) == 1) & (pr.min(axis=0) == 0)).sum())
            what = f"{pair} K {k} {policy}"
            print(f"{what}: reachable {ok[0::2].mean():.3f} of the even rows, {ok[1::2].mean():.3f} of the odd rows, states "
                  f"{np.bincount(ref['state'], minlength=5).tolist()}, projected {pr.mean():.3f} of the reachable samples, "
                  f"{both} poses with both kinds")
            assert ok[0::2].mean() >= 0.04 and ok[1::2].mean() > 0.5, what
            assert set(np.unique(ref["state"])) >= {0, 1, 2, 3, 4}, what
            assert 0.05 <= pr.mean() <= 0.95 and (k == 1 or both >= 1), what
            for slot in (0, 1):
                assert ok[arm == slot].sum() >= 100, f"{what}: both slots hold reachable rows"
            if k > 1:
                NW.gap_condition(NW.nearest_from_sweep(ref, seed), ref["reachable"], what)
    assert NW.GAP == 1e-9


@pytest.mark.parametrize("pair", list(PAIRS))
def test_path_inputs(pair):
    """path_workload.MAIN_SHAPES with kind "mixed", the shared grid of fractions and an explicit angle per waypoint and sample: the
    gap condition with and without start joints, at least one skipped waypoint, at least one whole path, fewer than all whole."""
    arms = checker_arms(pair)
    n = PW.N_MAIN
    for t, k, seed, _ in PW.MAIN_SHAPES:
        pos, eul, arm = PW.path_poses(seed, n, t, "mixed")
        assert 0 < arm.sum() < n
        explicit = np.random.default_rng(seed + 200).uniform(-np.pi, np.pi, size=(k, t, n))
        for policy, th in (("fraction", PW.path_fractions(k)), ("explicit", explicit.reshape(k, t * n))):
            ref = expected_tiled(orc, arms, PW.flat(pos), PW.flat(eul), np.tile(arm, t), policy, th, nthreads=4)
            for start in (None, PW.path_start(seed, n)):
                exp = PW.path_dp(ref, t, n, start)
                what = f"{pair} T {t} K {k} seed {seed} {policy} start {start is not None}"
                PW.gap_condition(exp, what, seeded=start is not None)
                whole = int(exp["solved"].all(axis=0).sum())
                assert (~exp["solved"]).sum() >= 1 and 1 <= whole < n, (what, whole)
