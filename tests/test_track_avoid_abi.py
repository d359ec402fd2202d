"""CPU-side checks of rsik_track_avoid: declared, exported, bound, ABI version still 8, the Python surface exists, the argument check
that needs no device — and the NumPy reference of the GPU tests (tests/track_avoid_workload.py) pinned on the CPU alone, with the
conditions that tests/test_gpu_track_avoid.py relies on asserted here, on the reference, so that no filter can hide a failure."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import clearance_workload as CW
import jacobian_workload as JW
import track_avoid_workload as AW
import track_workload as TW
from compare import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ surface
def test_track_avoid_entry_point_is_part_of_abi_8():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert _abi.ABI_VERSION == 8 == L.rsik_abi_version()
    assert "rsik_track_avoid" in _abi.PROTOTYPES
    assert isinstance(L.rsik_track_avoid, C._CFuncPtr)
    hdr = open(os.path.join(ROOT, "include", "rsik.h")).read()
    assert "#define RSIK_ABI_VERSION 8" in hdr
    decl = re.search(r"int rsik_track_avoid\(([^;]*)\);", hdr)
    assert decl, "include/rsik.h does not declare rsik_track_avoid"
    assert len(decl.group(1).split(",")) == len(_abi.PROTOTYPES["rsik_track_avoid"][1]) == 31
    assert int(re.search(r"#define RSIK_OPT_COUNT (\d+)", hdr).group(1)) == 9
    for words in ("a select, not a multiplication by zero", "0 ... 256 spheres", "0 ... 64 capsules", "has rsik_track's bits"):
        assert words in hdr, words
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`rsik_track_avoid`" in doc and "track_avoid_batch" in doc


def test_track_avoid_entry_point_refuses_a_null_context():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    args = (None, 0, 1, None, None, 0, None, 0.01, 1.0, 1.0, None, 0.05, None, None, 0.0, None, None, 1, None, 0, None, 0.1, 1.0) + (None,) * 8
    assert L.rsik_track_avoid(*args) == _abi.RSIK_E_INVALID


def test_python_surface_exists():
    from reachy2_symbolic_ik_amd import DualArmIK, HipSolver, SymbolicIK

    for cls, name in ((HipSolver, "track_avoid"), (SymbolicIK, "track_avoid_batch"), (DualArmIK, "track_avoid_batch")):
        fn = getattr(cls, name)
        assert callable(fn), (cls.__name__, name)
        for word in ("influence", "avoid_gain", "spheres", "capsules", "min_clearance", "nearest"):
            assert word in fn.__doc__, (cls.__name__, name, word)
    assert HipSolver.TRACK_AVOID_OUTPUTS == ("joints", "rates", "err", "clearance", "nearest", "final_joints", "final_err", "min_clearance")
    assert (HipSolver.TRACK_AVOID_MAX_SPHERES, HipSolver.TRACK_AVOID_MAX_CAPSULES) == (256, 64)


# ------------------------------------------------------------------------------------------ the reference, on the CPU alone
@pytest.mark.parametrize("with_terms", [False, True])
def test_without_a_push_the_reference_is_track_workload_s(with_terms):
    """With avoid_gain = 0, and with the scene moved 10 m away, the reference equals track_workload.run bit for bit in the five outputs
    the two share (lstsq rates, each arm on its own block), without and with feed-forward, rest and limits; with avoid_gain = 0 the
    clearance is still the scene's, and 10 m away no pair is inside the influence distance."""
    pair, n, T = "custom/custom", 24, 3
    sc = CW.scene(pair, "open")
    for side in (0, 1):
        arm = np.full(n, side, dtype=np.uint8)
        d = AW.inputs(pair, n, T, arm, with_terms)
        plain = TW.run(JW.blocks_of(pair)[side], d["start"], d["R"], d["p"], 0.05, **AW.terms_of(d))
        zero = AW.run(pair, arm, d["start"], d["R"], d["p"], 0.05, sc, avoid_gain=0.0, **AW.terms_of(d))
        away = AW.run(pair, arm, d["start"], d["R"], d["p"], 0.05, AW.moved(sc), **AW.terms_of(d))
        for o in ("joints", "rates", "err", "final_joints", "final_err"):
            assert np.array_equal(bits(zero[o]), bits(plain[o])), (side, o, "avoid_gain = 0")
            assert np.array_equal(bits(away[o]), bits(plain[o])), (side, o, "the scene 10 m away")
        assert zero["push"].any() and not away["push"].any() and (away["clearance"] > 5.0).all()
        first = CW.reference(JW.blocks_of(pair), d["start"], arm, sc)
        assert np.array_equal(bits(zero["clearance"][0]), bits(first["clearance"])) and np.array_equal(zero["nearest"][0], first["nearest"])


def test_the_push_is_the_clearance_gradient_times_a():
    """One step of the reference with a push, without a rest posture: q0 is avoid_gain (influence - d) times clearance_workload's
    gradient on the rows where d < influence and zero elsewhere; with a rest posture it is that on top of rest_gain (rest - q)."""
    pair, n = "default/default", 64
    arm = JW.arm_bytes()[:n]
    d = AW.inputs(pair, n, 1, arm, True)
    sc = CW.scene(pair, "open")
    c = CW.reference(JW.blocks_of(pair), d["start"], arm, sc)
    push = c["clearance"] < AW.INFLUENCE
    assert push.any() and (~push).any()
    a = AW.AVOID_GAIN * (AW.INFLUENCE - c["clearance"])
    s = AW.one_step(pair, arm, d["start"], d["R"][0], d["p"][0], 0.05, sc, solver="restatement")
    assert np.array_equal(s["push"], push)
    assert np.array_equal(bits(s["q0"][push]), bits(0.0 + a[push, None] * c["gradient"][push])) and (s["q0"][~push] == 0.0).all()
    rest = d["rest"]
    s = AW.one_step(pair, arm, d["start"], d["R"][0], d["p"][0], 0.05, sc, rest=rest, rest_gain=TW.REST_GAIN, solver="restatement")
    base = TW.REST_GAIN * (rest - d["start"])
    assert np.array_equal(bits(s["q0"]), bits(np.where(push[:, None], base + a[:, None] * c["gradient"], base)))


def test_the_tolerance_is_track_workload_s_plus_the_clearance_terms():
    """tol_t is track_workload.step_tolerance evaluated with the full q0, plus dt avoid_gain (sqrt(7) GRADIENT_BOUND (influence - d) +
    CLEARANCE_BOUND |g|) where the push acts and nothing where it does not; the two bounds are clearance_workload's."""
    pair, n = "default/default", 64
    arm = JW.arm_bytes()[:n]
    d = AW.inputs(pair, n, 1, arm, False)
    s = AW.one_step(pair, arm, d["start"], d["R"][0], d["p"][0], 0.05, CW.scene(pair, "open"), solver="restatement")
    tol = AW.step_tolerance(s, d["start"], 0.05)
    base = TW.step_tolerance(s, d["start"], 0.05)
    g = np.linalg.norm(s["gradient"], axis=1)
    extra = TW.DT * AW.AVOID_GAIN * (math.sqrt(7.0) * CW.GRADIENT_BOUND * (AW.INFLUENCE - s["clearance"]) + CW.CLEARANCE_BOUND * g)
    assert np.array_equal(tol[~s["push"]], base[~s["push"]])
    assert np.allclose(tol[s["push"]], (base + extra)[s["push"]], rtol=1e-15, atol=0.0) and (extra[s["push"]] > 0.0).all()
    assert CW.CLEARANCE_BOUND == max(1e-13, 16 * CW.E_CLEARANCE) and CW.GRADIENT_BOUND == max(1e-13, 16 * CW.E_GRADIENT)


@pytest.mark.parametrize("pair", AW.PAIRS)
def test_the_seeded_run_has_both_sides_of_the_select_and_the_bounds_hold_on_its_joints(pair):
    """The seeded run with the "open" scene (N_OPEN trajectories, T_OPEN steps): the push acts on at least 20 % of the (trajectory, step)
    pairs and does not on at least 20 %; at least 80 % of the active pairs are kept.  The device bounds of clearance_workload were
    measured on other joints, so E (float64 against longdouble) is measured again on the joints this run visits — the clearance on
    every pair, the gradient on the kept active pairs — and max(1e-13, 16 E) must not exceed them."""
    r = AW.open_run(pair)
    active = r["push"]
    kept_active = (r["keep"] & active).sum() / active.sum()
    print(f"{pair}: push active on {active.mean():.3f} of {active.size} pairs, {kept_active:.3f} of them kept, {r['keep'].mean():.3f} kept in all")
    assert active.mean() >= 0.2 and (~active).mean() >= 0.2, float(active.mean())
    assert kept_active >= 0.8, float(kept_active)
    assert np.isfinite(r["joints"]).all() and (r["err"][:, :, 1] < 1.0).all()
    arm = JW.arm_bytes()[:AW.N_OPEN]
    blocks, sc = JW.blocks_of(pair), CW.scene(pair, "open")
    before = np.concatenate([TW.starts()[None, :AW.N_OPEN], r["joints"][:-1]]).reshape(-1, 7)
    arms = np.tile(arm, AW.T_OPEN)
    f64 = CW.reference(blocks, before, arms, sc)
    ld = CW.reference(blocks, before, arms, sc, dtype=np.longdouble)
    assert np.array_equal(bits(f64["clearance"].reshape(AW.T_OPEN, -1)), bits(r["clearance"]))
    keep = (r["keep"] & active).reshape(-1)
    e_d = float(np.abs(f64["clearance"] - ld["clearance"]).max())
    e_g = float(np.abs(f64["gradient"] - ld["gradient"])[keep].max())
    print(f"{pair}: on the run's joints E_d {e_d:.3e}, E_g {e_g:.3e} (bounds {CW.CLEARANCE_BOUND:.1e}, {CW.GRADIENT_BOUND:.1e})")
    assert max(1e-13, 16 * e_d) <= CW.CLEARANCE_BOUND, e_d
    assert max(1e-13, 16 * e_g) <= CW.GRADIENT_BOUND, e_g


@pytest.mark.parametrize("pair", AW.PAIRS)
def test_the_elbow_case_has_rows_that_the_reference_moves_away(pair):
    """The one-sphere elbow case on both blocks: at least 32 rows whose min_clearance with avoidance exceeds the one without by at
    least 1 cm in the reference; the sphere is inside the influence distance of every row at some step, and without avoidance every
    row ends with the elbow inside it."""
    for side in (0, 1):
        e = AW.elbow_case(pair, side)
        print(f"{pair} side {side}: {int(e['rows'].sum())} of {AW.N_ELBOW} rows gain at least {AW.MIN_GAIN} m, largest gain {e['gain'].max():.4f} m, "
              f"final_err with avoidance at most {e['avoid']['final_err'].max(axis=0).tolist()}")
        assert e["rows"].sum() >= 32, int(e["rows"].sum())
        assert e["avoid"]["push"].any(axis=0).all() and (e["free"]["min_clearance"] < 0.0).all()
        assert len(e["scene"]["spheres"]) == 1 and len(e["scene"]["capsules"]) == 0


def test_the_full_scene_is_the_open_scene_repeated():
    """256 spheres and 64 capsules; clearance is the "open" scene's and the nearest pair the same obstacle at its index in the longer
    lists."""
    pair = "default/default"
    sc, full = CW.scene(pair, "open"), AW.full_scene(pair)
    assert full["spheres"].shape == (256, 4) and full["capsules"].shape == (64, 7)
    q, arm = TW.starts()[:65], JW.arm_bytes()[:65]
    a, b = (CW.reference(JW.blocks_of(pair), q, arm, s, full=False) for s in (sc, full))
    assert np.array_equal(bits(a["clearance"]), bits(b["clearance"])) and np.array_equal(a["nearest"][:, 0], b["nearest"][:, 0])
    S = len(sc["spheres"])
    assert np.array_equal(np.where(a["nearest"][:, 1] >= S, a["nearest"][:, 1] - S + 256, a["nearest"][:, 1]), b["nearest"][:, 1])
