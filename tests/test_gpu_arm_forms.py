"""GPU tests (-m gpu, MI355X) of the kernel instantiations launch_form() and tip_on_z() choose (csrc/rsik_lib.hip) for rsik_solve,
rsik_solve_sweep, rsik_solve_nearest and rsik_solve_path: FORM (0 one arm, 1 an arm byte per row with every constant per lane from
LDS, 2 an arm byte per row with the constants that have no handedness read as scalars), TIPZ, PREV_ROWS and nearest's LANES.

A. FORM 1 on two arms that really differ (tests/arm_pairs.NON_MIRROR) against the CPU checker with the pair's two arms: a lane that
   reads the other slot's segment length or limit misses by centimetres and degrees, the bar is TOL = 1e-9.
B. rsik_solve_nearest and rsik_solve_path on all five pairs against the library's own sweep under the same uploaded pair (A ties
   that sweep to the checker): check_nearest and check_path of their own modules, unchanged.
C. Every (RSIK_OPT_NO_MIRROR, RSIK_OPT_NO_TIPZ) form of nearest and path on the default arms, and the forms against each other.
D. custom/custom under RSIK_OPT_NO_MIRROR: FORM 1 on a mirror pair gives the bits of FORM 2.

tests/test_arm_pairs_checker.py asserts the conditions on these inputs on the checker alone; the checker on the two non-default
geometries is pinned to the reference by G9 and G20 (tests/test_oracle_golden.py).  Every tolerance is one the project already has."""
import numpy as np
import pytest

from arm_pairs import NON_MIRROR, PAIRS, checker_arms, solve_fractions, upload
from compare import as_bits, bits, close, joint_error, joints_close, same_bits
from gpu_support import T, abi, make_symbolic, orc, soa, to_np, torch_mod  # noqa: F401
from nearest_workload import GAP, N_MAIN, main_case, main_thetas
from path_workload import MAIN_SHAPES
from path_workload import N_MAIN as N_PATHS
from sampling_support import (LANES, check_against_solve, check_nearest, check_path, launches, lib_sweep, main_launches, path_arm_kwargs,
                              same_nearest_outputs, same_path_outputs, solve_columns)
from sweep_workload import columns, expected_tiled, sweep_poses, sweep_thetas

pytestmark = pytest.mark.gpu

N = 1000  # three full 256-pose blocks, a ragged last one with a ragged last wave; r and l alternate inside every wave
OPTIONS = ((0, 0), (0, 1), (1, 0), (1, 1))  # (RSIK_OPT_NO_MIRROR, RSIK_OPT_NO_TIPZ)
WRIST_YAW_TOL = 2e-15  # test_tip_z_specialisation_matches_general_path's bound on the one output the tip-on-z stage may round differently


def set_options(solver, no_mirror, no_tipz):
    solver.set_option(abi().OPT_NO_MIRROR, no_mirror)
    solver.set_option(abi().OPT_NO_TIPZ, no_tipz)


# ------------------------------------------------------------------------------------------ A. non-mirror pairs against the checker
@pytest.mark.parametrize("pair", NON_MIRROR)
@pytest.mark.parametrize("k", [1, 8])
def test_non_mirror_pairs_against_the_checker(torch_mod, orc, pair, k):
    """n = 1000 mixed rows.  rsik_solve with theta at the interval start and at a fraction per row against orc.solve_batch with the
    pair's arms; rsik_solve_sweep, both policies, a theta column per pose, against sweep_workload.expected_tiled: reachable / state /
    projected exact, interval, theta, joints and elbow within TOL (joints_close); and the sweep is rsik_solve's row per theta column,
    bit for bit."""
    torch = torch_mod
    _abi = abi()
    arms = checker_arms(pair)
    pos, eul, arm = sweep_poses("mixed", 500 + k, N)
    p, armT = soa(pos, eul, torch), T(arm, torch)
    solver = upload(pair)
    worst = 0.0
    u = solve_fractions(k, N)
    for policy, theta_in in ((_abi.THETA_INTERVAL0, None), (_abi.THETA_FRACTION, u)):
        what = f"{pair} K {k} solve policy {policy}"
        ref = orc.solve_batch(arms[0], arms[1], pos, eul, arm_id=arm, theta_policy=policy, theta_in=theta_in, nthreads=4)
        got = to_np(solver.solve(p, arm=armT, theta_policy=policy, theta_in=None if theta_in is None else T(theta_in, torch)))
        for key in ("reachable", "state"):
            np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{what} {key}")
        ok = ref["reachable"].astype(bool)
        assert ok[0::2].mean() >= 0.04 and ok[1::2].mean() > 0.5 and ok[arm == 0].sum() >= 100 and ok[arm == 1].sum() >= 100, what
        close(got["interval"], ref["interval"], what + " interval")
        assert np.isnan(got["joints"][~ok]).all() and np.isnan(got["elbow"][~ok]).all(), what
        joints_close(got["joints"][ok], ref["joints"][ok], what + " joints")
        close(got["elbow"][ok], ref["elbow"][ok], what + " elbow")
        worst = max(worst, joint_error(got["joints"][ok], ref["joints"][ok]))
    for policy in ("fraction", "explicit"):
        what = f"{pair} K {k} sweep {policy}"
        thetas = sweep_thetas(policy, True, k, N, 600 + k)
        ref = expected_tiled(orc, arms, pos, eul, arm, policy, thetas, nthreads=4)
        got = to_np(solver.solve_sweep(p, T(thetas, torch), policy=policy, arm=armT))
        for key in ("reachable", "state", "projected"):
            np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{what} {key}")
        ok = ref["reachable"].astype(bool)
        close(got["interval"], ref["interval"], what + " interval")
        close(got["theta"], ref["theta"], what + " theta")
        for q in range(k):
            assert np.isnan(got["joints"][q][~ok]).all() and np.isnan(got["elbow"][q][~ok]).all(), what
            joints_close(got["joints"][q][ok], ref["joints"][q][ok], f"{what} sample {q} joints")
            close(got["elbow"][q][ok], ref["elbow"][q][ok], f"{what} sample {q} elbow")
            worst = max(worst, joint_error(got["joints"][q][ok], ref["joints"][q][ok]))
        check_against_solve(got, solve_columns(solver, p, policy, columns(thetas, N), torch, arm=armT), what)
    print(f"{pair} K {k}: largest joint difference against the checker {worst:.3e}")


# ------------------------------------------------------------------------------------------ B. nearest and path on the pairs
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("k", [3, 70])
def test_nearest_on_arm_pairs(torch_mod, pair, k):
    """nearest_workload.main_case("mixed", K), a theta column per pose, both policies, with and without previous_joints rows, every
    value of RSIK_OPT_NEAREST_LANES: check_nearest with the gap condition against the library's sweep under the same pair."""
    torch = torch_mod
    _abi = abi()
    pos, eul, arm, seed = main_case("mixed", k)
    p, armT, seedT = soa(pos, eul, torch), T(arm, torch), T(seed, torch)
    prev_rows = T(np.random.default_rng(40 + k).uniform(-2, 2, size=(N_MAIN, 7)), torch)
    solver = upload(pair)
    for policy in ("fraction", "explicit"):
        th = T(main_thetas(policy, True, k), torch)
        for prev in (None, prev_rows):
            kw = dict(policy=policy, previous_joints=prev, arm=armT)
            sw = to_np(solver.solve_sweep(p, th, **kw))
            ok = sw["reachable"].astype(bool)
            assert ok[0::2].mean() >= 0.04 and ok[1::2].mean() > 0.5 and ok[arm == 0].sum() >= 100 and ok[arm == 1].sum() >= 100
            for lanes in LANES:
                solver.set_option(_abi.OPT_NEAREST_LANES, lanes)
                got = to_np(solver.solve_nearest(p, th, seedT, **kw))
                check_nearest(got, sw, seed, f"{pair} K {k} {policy} prev {prev is not None} L {lanes}", need_gap=True)


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("shape", MAIN_SHAPES)
def test_path_on_arm_pairs(torch_mod, pair, shape):
    """path_workload.MAIN_SHAPES with r and l paths in every workgroup, the shared grid of fractions and an explicit angle per waypoint
    and sample, with and without start joints: check_path with the gap condition against the library's sweep over the same T n poses."""
    torch = torch_mod
    t, k, seed, _ = shape
    solver = upload(pair)
    for what, p, th, policy, arm, start in launches(torch, t, k, seed, "mixed"):
        assert 0 < arm.sum() < N_PATHS
        sw = lib_sweep(solver, p, th, policy, arm, torch)
        got = to_np(solver.solve_path(p, th, None if start is None else T(start, torch), policy=policy, arm=T(arm, torch)))
        exp = check_path(got, sw, t, N_PATHS, f"{pair} {what}", start, need_gap=True)
        assert 0 < (~exp["solved"]).sum() and 1 <= exp["solved"].all(axis=0).sum() < N_PATHS, what


# ------------------------------------------------------------------------------------------ C. every option form, default arms
def nearest_rows_agree(a, b, exp, what):
    """Two launches that may differ in the wrist yaw's rounding only (RSIK_OPT_NO_TIPZ 0 against 1): the per-pose outputs are the same
    bits; index is the same wherever the gap is clear; and where index is the same, theta, elbow, projected and the first six joints
    are the same bits and the wrist yaw agrees within WRIST_YAW_TOL."""
    for key in ("interval", "reachable", "state"):
        np.testing.assert_array_equal(as_bits(a[key]), as_bits(b[key]), err_msg=f"{what}: {key}")
    np.testing.assert_array_equal(a["index"] == -1, b["index"] == -1, err_msg=what)
    clear = exp["gap"] > GAP
    np.testing.assert_array_equal(a["index"][clear], b["index"][clear], err_msg=what + ": index where the gap is clear")
    same = a["index"] == b["index"]
    assert same.mean() >= 0.95, what  # (what the gap condition, asserted by check_nearest, and the line above imply)
    for key in ("theta", "elbow", "projected"):
        np.testing.assert_array_equal(as_bits(a[key][same]), as_bits(b[key][same]), err_msg=f"{what}: {key}")
    same_bits(a["joints"][same][:, :6], b["joints"][same][:, :6], what + ": the first six joints")
    won = same & (a["index"] >= 0)
    err = float(np.max(np.abs(a["joints"][won, 6] - b["joints"][won, 6]), initial=0.0))
    assert err < WRIST_YAW_TOL, (what, err)


@pytest.mark.parametrize("kind", ["r", "mixed"])
@pytest.mark.parametrize("k", [3, 70])
@pytest.mark.parametrize("with_prev", [False, True])
def test_nearest_under_every_option_form(torch_mod, kind, k, with_prev):
    """The main launches of tests/test_gpu_solve_nearest.py under the four (RSIK_OPT_NO_MIRROR, RSIK_OPT_NO_TIPZ) settings and the four
    lane settings: each against the library's sweep under the same two options (check_nearest); NO_MIRROR 0 against 1 the same bits in
    every output; NO_TIPZ 0 against 1 as test_tip_z_specialisation_matches_general_path, index equal wherever the gap is clear."""
    torch = torch_mod
    _abi = abi()
    solver, _, _ = make_symbolic(0.03)
    for what, p, th, seedT, kw, seed in main_launches(torch, kind, k):
        if (kw["previous_joints"] is not None) != with_prev:
            continue
        outs, exps = {}, {}
        for no_mirror, no_tipz in OPTIONS:
            set_options(solver, no_mirror, no_tipz)
            sw = to_np(solver.solve_sweep(p, th, **kw))
            for lanes in LANES:
                solver.set_option(_abi.OPT_NEAREST_LANES, lanes)
                got = to_np(solver.solve_nearest(p, th, seedT, **kw))
                exp = check_nearest(got, sw, seed, f"{what} no_mirror {no_mirror} no_tipz {no_tipz} L {lanes}", need_gap=True)
                outs[no_mirror, no_tipz, lanes], exps[no_mirror, no_tipz] = got, exp
        for lanes in LANES:
            for no_tipz in (0, 1):
                same_nearest_outputs(outs[1, no_tipz, lanes], outs[0, no_tipz, lanes], f"{what} no_tipz {no_tipz} L {lanes}: NO_MIRROR 1 against 0")
            for no_mirror in (0, 1):
                nearest_rows_agree(outs[no_mirror, 0, lanes], outs[no_mirror, 1, lanes], exps[no_mirror, 0],
                                   f"{what} no_mirror {no_mirror} L {lanes}: NO_TIPZ 0 against 1")


def paths_agree(a, b, exp, what):
    """nearest_rows_agree for two rsik_solve_path launches: per path."""
    for key in ("interval", "reachable", "state", "n_solved"):
        np.testing.assert_array_equal(as_bits(a[key]), as_bits(b[key]), err_msg=f"{what}: {key}")
    np.testing.assert_array_equal(a["index"] == -1, b["index"] == -1, err_msg=what)
    clear = exp["gap"] > GAP
    np.testing.assert_array_equal(a["index"][:, clear], b["index"][:, clear], err_msg=what + ": index where the gap is clear")
    same = (a["index"] == b["index"]).all(axis=0)
    assert same.any(), what
    for key in ("theta", "elbow", "projected"):
        np.testing.assert_array_equal(as_bits(a[key][:, same]), as_bits(b[key][:, same]), err_msg=f"{what}: {key}")
    same_bits(a["joints"][:, same][..., :6], b["joints"][:, same][..., :6], what + ": the first six joints")
    won = same[None] & (a["index"] >= 0)
    err = float(np.max(np.abs(a["joints"][won][:, 6] - b["joints"][won][:, 6]), initial=0.0))
    assert err < WRIST_YAW_TOL, (what, err)


@pytest.mark.parametrize("shape", MAIN_SHAPES)
def test_path_under_every_option_form(torch_mod, shape):
    """The MAIN_SHAPES launches of tests/test_gpu_solve_path.py under the four option settings: each against the library's sweep under
    the same two options (check_path), and the settings against each other as in test_nearest_under_every_option_form."""
    torch = torch_mod
    t, k, seed, kind = shape
    solver, _, _ = make_symbolic(0.03)
    for what, p, th, policy, arm, start in launches(torch, t, k, seed, kind):
        outs, exps = {}, {}
        for no_mirror, no_tipz in OPTIONS:
            set_options(solver, no_mirror, no_tipz)
            sw = lib_sweep(solver, p, th, policy, arm, torch)
            got = to_np(solver.solve_path(p, th, None if start is None else T(start, torch), policy=policy, **path_arm_kwargs(arm, torch)))
            need_gap = policy == "fraction" and k > 1 and (t > 1 or start is not None)
            exps[no_mirror, no_tipz] = check_path(got, sw, t, N_PATHS, f"{what} no_mirror {no_mirror} no_tipz {no_tipz}", start, need_gap=need_gap)
            outs[no_mirror, no_tipz] = got
        for no_tipz in (0, 1):
            same_path_outputs(outs[1, no_tipz], outs[0, no_tipz], f"{what} no_tipz {no_tipz}: NO_MIRROR 1 against 0")
        for no_mirror in (0, 1):
            paths_agree(outs[no_mirror, 0], outs[no_mirror, 1], exps[no_mirror, 0], f"{what} no_mirror {no_mirror}: NO_TIPZ 0 against 1")


# ------------------------------------------------------------------------------------------ D. custom/custom under NO_MIRROR
def test_form_1_on_a_mirror_pair_gives_the_bits_of_form_2(torch_mod):
    """custom/custom (G9 in both slots: a mirror pair whose tips leave the z axis) launches FORM 2; under RSIK_OPT_NO_MIRROR FORM 1.
    rsik_solve (theta at the interval start and at a fraction per row), rsik_solve_sweep, rsik_solve_nearest (every lane setting) and
    rsik_solve_path give the same bits either way, in every output."""
    torch = torch_mod
    _abi = abi()
    k = 8
    solver = upload("custom/custom")
    pos, eul, arm, seed = main_case("mixed", k)
    p, armT, seedT = soa(pos, eul, torch), T(arm, torch), T(seed, torch)
    u = T(solve_fractions(k, N_MAIN), torch)
    t, kp, pseed, _ = MAIN_SHAPES[1]
    path_launches = list(launches(torch, t, kp, pseed, "mixed"))

    def run():
        out = {"solve i0": to_np(solver.solve(p, arm=armT)),
               "solve fraction": to_np(solver.solve(p, arm=armT, theta_policy=_abi.THETA_FRACTION, theta_in=u))}
        for policy in ("fraction", "explicit"):
            th = T(main_thetas(policy, True, k), torch)
            out[f"sweep {policy}"] = to_np(solver.solve_sweep(p, th, policy=policy, arm=armT))
            for lanes in LANES:
                solver.set_option(_abi.OPT_NEAREST_LANES, lanes)
                out[f"nearest {policy} L {lanes}"] = to_np(solver.solve_nearest(p, th, seedT, policy=policy, arm=armT))
        for what, pp, th, policy, parm, start in path_launches:
            out["path " + what] = to_np(solver.solve_path(pp, th, None if start is None else T(start, torch), policy=policy, arm=T(parm, torch)))
        return out

    form2 = run()
    solver.set_option(_abi.OPT_NO_MIRROR, 1)
    form1 = run()
    assert form2["solve i0"]["reachable"].sum() >= 300 and (form2["nearest fraction L 0"]["index"] >= 0).sum() >= 300
    assert (form2["path " + path_launches[0][0]]["n_solved"] > 0).sum() >= N_PATHS // 2
    for what, a in form2.items():
        b = form1[what]
        assert set(a) == set(b), what
        for key in a:
            x, y = (bits(a[key]), bits(b[key])) if a[key].dtype == np.float64 else (a[key], b[key])
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: {key} under NO_MIRROR")
