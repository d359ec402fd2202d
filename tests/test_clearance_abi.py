"""CPU-side checks of rsik_clearance: declared, exported, bound, ABI version still 8, the Python surface exists, the argument check
that needs no device — and the NumPy reference of the GPU tests (tests/clearance_workload.py) pinned on the CPU alone: against brute
force over a grid of both segments, against its own run in np.longdouble (where the device bounds come from), its gradient against
central differences of its clearance, and what the scenes must contain for tests/test_gpu_clearance.py to mean something."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clearance_workload as W
import jacobian_workload as JW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(sc, st) for sc in W.SCENES for st in W.SETS]


# ------------------------------------------------------------------------------------------ surface
def test_clearance_entry_point_is_part_of_abi_8():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert _abi.ABI_VERSION == 8 == L.rsik_abi_version()
    assert "rsik_clearance" in _abi.PROTOTYPES
    assert isinstance(L.rsik_clearance, C._CFuncPtr)
    hdr = open(os.path.join(ROOT, "include", "rsik.h")).read()
    assert "#define RSIK_ABI_VERSION 8" in hdr
    decl = re.search(r"int rsik_clearance\(([^;]*)\);", hdr)
    assert decl, "include/rsik.h does not declare rsik_clearance"
    assert len(decl.group(1).split(",")) == len(_abi.PROTOTYPES["rsik_clearance"][1]) == 16
    assert int(re.search(r"#define RSIK_OPT_COUNT (\d+)", hdr).group(1)) == 9
    for words in ("g_k = u . (a_k x (x - o_k))", "the first minimum wins", "is skipped"):
        assert words in hdr, words
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`rsik_clearance`" in doc and "clearance_batch" in doc and "bias_rates" in doc


def test_clearance_entry_point_refuses_a_null_context():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert L.rsik_clearance(None, 0, 1, None, None, 0, None, 1, None, 0, None, None, None, None, None, None) == _abi.RSIK_E_INVALID


def test_python_surface_exists():
    from reachy2_symbolic_ik_amd import DualArmIK, HipSolver, SymbolicIK
    from reachy2_symbolic_ik_amd.symbolic_ik import arm_capsules

    for cls, name in ((HipSolver, "clearance"), (SymbolicIK, "clearance_batch"), (DualArmIK, "clearance_batch")):
        fn = getattr(cls, name)
        assert callable(fn), (cls.__name__, name)
        for word in ("nearest", "witness", "gradient", "link_points", "bias_rates"):
            assert word in fn.__doc__, (cls.__name__, name, word)
    assert "other_arm" in DualArmIK.clearance_batch.__doc__ and callable(arm_capsules)
    assert HipSolver.CLEARANCE_OUTPUTS == ("clearance", "nearest", "gradient", "witness", "link_points")


# ------------------------------------------------------------------------------------------ the reference, on the CPU alone
@pytest.mark.parametrize("pair", W.PAIRS)
def test_walk_is_the_jacobian_helper_s_chain(pair):
    """walk() in float64 is jacobian_workload._walk itself; in np.longdouble it is the same chain to 1e-15, and its last link point is
    the position of the helper's FK."""
    q = JW.joint_set("wound")[:128]
    for block in JW.blocks_of(pair):
        p, _, axes, origins = JW._walk(block, q)
        pts, ax, og = W.walk(block, q)
        assert np.array_equal(pts[:, 3], p) and np.array_equal(ax, axes) and np.array_equal(og, origins)
        assert np.array_equal(pts[:, 0], origins[:, 1]) and np.array_equal(pts[:, 1], origins[:, 3]) and np.array_equal(pts[:, 2], origins[:, 6])
        lp, la, lo = W.walk(block, q, np.longdouble)
        assert lp.dtype == np.longdouble
        err = max(float(np.abs(lp - pts).max()), float(np.abs(la - ax).max()), float(np.abs(lo - og).max()))
        print(f"{pair}: walk in longdouble against float64 {err:.3e}")
        assert err < 1e-15


@pytest.mark.parametrize("pair", W.PAIRS)
def test_reference_distance_against_brute_force(pair):
    """Every (link, obstacle) pair of 24 rows against the smallest distance over a 65 x 65 grid of (s, t): the reference is never
    above a sampled distance, and the best sample is within one grid step x (the sum of the two segments' lengths) of it."""
    blocks, sc = JW.blocks_of(pair), W.scene(pair, "open")
    q, arm = JW.joint_set("uniform")[:24], JW.arm_bytes()[:24]
    ref = W.reference(blocks, q, arm, sc, radius=(0.0, 0.0, 0.0))
    sp, cp = sc["spheres"], sc["capsules"]
    ok = np.concatenate([W.usable(sp), W.usable(cp)])
    a = np.concatenate([sp[:, :3], cp[:, :3]])[ok]
    b = np.concatenate([sp[:, :3], cp[:, 3:6]])[ok]
    rad = np.concatenate([sp[:, 3], cp[:, 6]])[ok]
    grid = np.linspace(0.0, 1.0, 65)
    worst_above, worst_gap = 0.0, 0.0
    for i in range(len(q)):
        P = ref["link_points"][i]
        x = P[:3, None, :] + grid[None, :, None] * (P[1:] - P[:3])[:, None, :]              # [3, 65, 3]
        y = a[:, None, :] + grid[None, :, None] * (b - a)[:, None, :]                        # [m, 65, 3]
        d = np.linalg.norm(x[None, :, :, None, :] - y[:, None, None, :, :], axis=-1)          # [m, 3, 65, 65]
        sampled = d.reshape(len(a), 3, -1).min(axis=-1) - rad[:, None]
        got = ref["pairs"][i][ok]
        lengths = np.linalg.norm(P[1:] - P[:3], axis=1)[None, :] + np.linalg.norm(b - a, axis=1)[:, None]
        worst_above = max(worst_above, float((got - sampled).max()))
        assert (got <= sampled + 1e-15).all(), (pair, i, float((got - sampled).max()))
        assert (sampled - got <= lengths / 64).all(), (pair, i, float((sampled - got).max()))
        worst_gap = max(worst_gap, float((sampled - got).max()))
    print(f"{pair}: reference above the best of 65 x 65 samples by at most {worst_above:.3e}, below it by at most {worst_gap:.3e}")
    assert np.isinf(ref["pairs"][:, ~ok]).all()


@pytest.mark.parametrize("pair", W.PAIRS)
def test_reference_outputs_are_what_the_header_defines(pair):
    """The witness points lie on their segments and are the distance apart that the clearance says; `nearest` is the first minimum of
    the pair table in the order (obstacle, link); the gradient is zero for the joints above the link."""
    c = W.case(pair, "uniform", "open")
    ref, sc = c["ref"], c["sc"]
    x, y = ref["witness"][:, 0], ref["witness"][:, 1]
    link, obs = ref["nearest"][:, 0], ref["nearest"][:, 1]
    rows = np.arange(len(link))
    rad = np.concatenate([sc["spheres"][:, 3], sc["capsules"][:, 6]])[obs] + np.asarray(W.LINK_RADIUS)[link]
    assert np.abs(np.linalg.norm(x - y, axis=1) - rad - ref["clearance"]).max() < 1e-15
    flat = ref["pairs"].reshape(len(link), -1)
    assert np.array_equal(flat.argmin(axis=1), obs * 3 + link) and np.array_equal(flat.min(axis=1), ref["clearance"])
    P = ref["link_points"]
    e = P[rows, link + 1] - P[rows, link]
    s = ((x - P[rows, link]) * e).sum(axis=1) / (e * e).sum(axis=1)
    assert (s > -1e-15).all() and (s < 1 + 1e-15).all()
    assert np.abs(np.cross(x - P[rows, link], e)).max() < 1e-16
    above = np.arange(7)[None, :] >= np.asarray(W.LINK_JOINTS)[link][:, None]
    at_shoulder = (link == 0) & (s < 1e-15)  # the witness is the shoulder itself, which no joint moves
    assert (ref["gradient"][above] == 0.0).all() and (np.abs(ref["gradient"]).max(axis=1) > 0)[~at_shoulder].all()


def _measure(pair):
    """(E_d, E_g, FD, kept share) per (scene, set) of a pair: the reference in float64 against itself in np.longdouble, its gradient
    against central differences of its clearance."""
    out = {}
    for scene, name in CASES:
        c = W.case(pair, name, scene)
        ref, keep = c["ref"], c["keep"]
        ld = W.reference(JW.blocks_of(pair), c["q"], c["arm"], c["sc"], dtype=np.longdouble)
        assert ld["clearance"].dtype == np.longdouble
        out[scene, name] = (float(np.abs(ref["clearance"] - ld["clearance"]).max()), float(np.abs(ref["gradient"] - ld["gradient"])[keep].max()),
                            float(np.abs(ref["gradient"] - c["fd"])[keep].max()), float(keep.mean()))
        print(f"{pair} {scene} {name}: E_d {out[scene, name][0]:.3e}, E_g {out[scene, name][1]:.3e}, gradient against central "
              f"differences {out[scene, name][2]:.3e}, kept {out[scene, name][3]:.3f}")
    return out


def test_device_bounds_come_from_the_reference():
    """The bounds of tests/test_gpu_clearance.py are max(1e-13, 16 x E) with E the largest |float64 - longdouble| of the reference,
    for the clearance over all rows and for the gradient over the kept rows, of every pair, scene and set.  Measured here again: the
    constants in clearance_workload must be that, rounded up (no more than twice it: the last bits of the measurement may differ
    between libm builds).  The same for the gradient against central differences of the clearance at h = 1e-6 on the kept rows, whose
    bound is 10 x the value observed.  The filter keeps at least 90 % of the rows of every scene and set."""
    figures = [v for pair in W.PAIRS for v in _measure(pair).values()]
    e_d, e_g, fd = (max(f[k] for f in figures) for k in range(3))
    print(f"E_d {e_d:.3e} (recorded {W.E_CLEARANCE:.1e}), E_g {e_g:.3e} (recorded {W.E_GRADIENT:.1e}), central differences {fd:.3e} "
          f"(recorded {W.FD_OBSERVED:.1e}), smallest kept share {min(f[3] for f in figures):.3f}")
    assert e_d <= W.E_CLEARANCE <= 2 * e_d, (e_d, W.E_CLEARANCE)
    assert e_g <= W.E_GRADIENT <= 2 * e_g, (e_g, W.E_GRADIENT)
    assert W.CLEARANCE_BOUND == max(1e-13, 16 * W.E_CLEARANCE) and W.GRADIENT_BOUND == max(1e-13, 16 * W.E_GRADIENT)
    assert fd <= W.FD_OBSERVED <= 2 * fd and W.FD_BOUND == 10 * W.FD_OBSERVED, (fd, W.FD_OBSERVED)
    assert min(f[3] for f in figures) >= 0.9


@pytest.mark.parametrize("pair", W.PAIRS)
def test_scenes_hold_the_cases_the_gpu_tests_need(pair):
    """Penetrated rows, skipped obstacles and exact ties are present; every row penetrates the deep scene; every link and both kinds
    of obstacle win somewhere; one capsule has a == b; one capsule is parallel to link 1 of row PAR_ROW and wins there."""
    for scene in W.SCENES:
        c = W.case(pair, "uniform", scene)
        ref, sc = c["ref"], c["sc"]
        S = len(sc["spheres"])
        skipped = int((~W.usable(sc["spheres"])).sum()), int((~W.usable(sc["capsules"])).sum())
        penetrated = int((ref["clearance"] < 0).sum())
        tied = int((ref["runner_up"] - ref["clearance"] <= 2 * W.CLEARANCE_BOUND).sum())
        print(f"{pair} {scene}: {penetrated} rows penetrate, {tied} tied, skipped obstacles {skipped}, winners by link "
              f"{np.bincount(ref['nearest'][:, 0], minlength=3).tolist()}, capsule winners {int((ref['nearest'][:, 1] >= S).sum())}")
        assert skipped == (3, 1) and penetrated > 0
        assert (sc["capsules"][:, :3] == sc["capsules"][:, 3:6]).all(axis=1).sum() == 1
        assert np.isfinite(ref["clearance"]).all() and S <= 4096 and len(sc["capsules"]) <= 256
        radii = np.concatenate([sc["spheres"][:, 3], sc["capsules"][:, 6]])
        assert np.nanmin(radii[radii >= 0]) >= 0.01 and np.sort(radii[radii >= 0])[-3] <= 0.08
        if scene == "deep":
            assert penetrated == W.N_SET
        else:
            assert tied > 0 and (np.bincount(ref["nearest"][:, 0], minlength=3) > 0).all() and (ref["nearest"][:, 1] >= S).any()
            assert (ref["nearest"][:, 1] < S).any()
    sc = W.scene(pair, "open")
    P = W.case(pair, "uniform", "open")["ref"]["link_points"][W.PAR_ROW]
    cap = sc["capsules"][sc["par"]]
    assert np.abs(np.cross(P[2] - P[1], cap[3:6] - cap[:3])).max() < 1e-16  # (of two vectors of 0.3 m)
    alone = W.case(pair, "uniform", "parallel")  # the scene that holds nothing else: there the parallel pair is row PAR_ROW's answer
    assert np.array_equal(alone["sc"]["capsules"][0], cap) and len(alone["sc"]["spheres"]) == 0
    assert tuple(alone["ref"]["nearest"][W.PAR_ROW]) == (1, 0) and not alone["keep"][W.PAR_ROW]
    assert abs(alone["ref"]["clearance"][W.PAR_ROW] - (W.PAR_DISTANCE - W.LINK_RADIUS[1] - 0.02)) < 1e-15


def test_reference_rows_and_obstacles_that_are_not_numbers():
    pair = "default/default"
    sc = W.scene(pair, "open")
    q = JW.joint_set("uniform")[:8].copy()
    q[2, 5], q[5, 0] = np.nan, -np.inf
    ref = W.reference(JW.blocks_of(pair), q, JW.arm_bytes()[:8], sc)
    for key in ("clearance", "gradient", "witness", "link_points"):
        rows = np.isnan(ref[key].reshape(8, -1))
        assert rows[[2, 5]].all() and not rows[[0, 1, 3, 4, 6, 7]].any(), key
    assert (ref["nearest"][[2, 5]] == -1).all() and (ref["nearest"][[0, 1, 3, 4, 6, 7]] >= 0).all()
    ok_s, ok_c = W.usable(sc["spheres"]), W.usable(sc["capsules"])
    clean = dict(spheres=sc["spheres"][ok_s], capsules=sc["capsules"][ok_c])
    ref2 = W.reference(JW.blocks_of(pair), q, JW.arm_bytes()[:8], clean)
    shift = np.concatenate([np.cumsum(ok_s) - 1, ok_s.sum() + np.cumsum(ok_c) - 1])
    good = [0, 1, 3, 4, 6, 7]
    assert np.array_equal(ref["clearance"][good], ref2["clearance"][good])
    assert np.array_equal(shift[ref["nearest"][good, 1]], ref2["nearest"][good, 1])
    none = W.reference(JW.blocks_of(pair), q, JW.arm_bytes()[:8], dict(spheres=sc["spheres"][~ok_s], capsules=sc["capsules"][~ok_c]))
    assert np.isposinf(none["clearance"][good]).all() and (none["nearest"] == -1).all()
    assert (none["gradient"][good] == 0).all() and np.isnan(none["witness"][good]).all() and np.isfinite(none["link_points"][good]).all()
