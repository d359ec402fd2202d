"""CPU-side checks of rsik_track_pair: declared, exported, bound, ABI version still 8, the Python surface exists, the argument check
that needs no device — and the NumPy reference of the GPU tests (tests/track_pair_workload.py) pinned on the CPU alone, with the
conditions that tests/test_gpu_track_pair.py relies on asserted here, on the reference, so that no filter can hide a failure."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clearance_workload as CW
import jacobian_workload as JW
import track_avoid_workload as AW
import track_pair_workload as PW
import track_workload as TW
from compare import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ surface
def test_track_pair_entry_point_is_part_of_abi_8():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    assert _abi.ABI_VERSION == 8 == L.rsik_abi_version()
    assert "rsik_track_pair" in _abi.PROTOTYPES
    assert isinstance(L.rsik_track_pair, C._CFuncPtr)
    hdr = open(os.path.join(ROOT, "include", "rsik.h")).read()
    assert "#define RSIK_ABI_VERSION 8" in hdr
    decl = re.search(r"int rsik_track_pair\(([^;]*)\);", hdr)
    assert decl, "include/rsik.h does not declare rsik_track_pair"
    assert len(decl.group(1).split(",")) == len(_abi.PROTOTYPES["rsik_track_pair"][1]) == 29
    assert "arm" not in decl.group(1), "there is no arm argument"
    assert int(re.search(r"#define RSIK_OPT_COUNT (\d+)", hdr).group(1)) == 9
    for words in ("row 2i is the right arm of robot i", "indices n_spheres + n_capsules + l", "NO static obstacle is allowed here",
                  "has rsik_track_avoid's bits"):
        assert words in hdr, words
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`rsik_track_pair`" in doc and "track_pair_batch" in doc


def test_track_pair_entry_point_refuses_a_null_context():
    from reachy2_symbolic_ik_amd import _abi

    L = _abi.load()
    args = (None, 0, 1, None, None, 0.01, 1.0, 1.0, None, 0.05, None, None, 0.0, None, None, 0, None, 0, None, 0.1, 1.0) + (None,) * 8
    assert L.rsik_track_pair(*args) == _abi.RSIK_E_INVALID


def test_python_surface_exists():
    from reachy2_symbolic_ik_amd import DualArmIK, HipSolver

    for cls, name in ((HipSolver, "track_pair"), (DualArmIK, "track_pair_batch")):
        fn = getattr(cls, name)
        assert callable(fn), (cls.__name__, name)
        for word in ("influence", "avoid_gain", "spheres", "capsules", "min_clearance", "nearest", "right arm", "left arm", "partner"):
            assert word in fn.__doc__, (cls.__name__, name, word)
    assert HipSolver.TRACK_PAIR_OUTPUTS is HipSolver.TRACK_AVOID_OUTPUTS


# ------------------------------------------------------------------------------------------ the reference, on the CPU alone
@pytest.mark.parametrize("with_terms", [False, True])
def test_without_a_partner_and_without_a_push_the_reference_is_track_avoid_workload_s(with_terms):
    """With one arm's rows NaN the other arm's rows equal track_avoid_workload.run (rows of that arm alone, the same static scene) bit
    for bit in every output, and the NaN rows are NaN in joints, err and clearance with nearest (-1, -1); with avoid_gain = 0 both arms' rows equal it in the five
    outputs the two share, while their clearance is the partner's where the partner is nearer than the scene."""
    pair, n_pairs, T = "custom/custom", 12, 3
    sc = CW.scene(pair, "open")
    d = PW.inputs(pair, n_pairs, T, with_terms)
    terms = AW.terms_of(d)
    arm = PW.arm_bytes(n_pairs)
    shared = ("joints", "rates", "err", "final_joints", "final_err")

    def rows_of(x, idx):  # (per step [T, n, ...] or per row [n, ...])
        return x[idx] if x.shape[0] == 2 * n_pairs else x[:, idx]

    for side in (0, 1):
        live = np.flatnonzero(arm == side)
        start = d["start"].copy()
        start[arm != side] = np.nan
        got = PW.run(pair, start, d["R"], d["p"], 0.05, sc, **terms)
        sub = dict(ff=None if terms["ff"] is None else terms["ff"][:, live], rest=None if terms["rest"] is None else terms["rest"][live],
                   rest_gain=terms["rest_gain"], limits=terms["limits"])
        alone = AW.run(pair, arm[live], d["start"][live], d["R"][:, live], d["p"][:, live], 0.05, sc, **sub)
        assert alone["push"].any(), "the live rows are pushed by the scene somewhere"
        for o in shared + ("clearance", "min_clearance"):
            assert np.array_equal(bits(rows_of(got[o], live)), bits(alone[o])), (side, o)
        assert np.array_equal(got["nearest"][:, live], alone["nearest"]), side
        dead = np.flatnonzero(arm != side)
        for o in ("joints", "err", "final_joints", "clearance"):  # (the reference holds such a row: its rates are 0, the device's NaN)
            assert np.isnan(rows_of(got[o], dead)).all(), (side, o)
        assert (got["nearest"][:, dead] == -1).all() and np.isnan(got["min_clearance"][dead]).all()
    zero = PW.run(pair, d["start"], d["R"], d["p"], 0.05, sc, avoid_gain=0.0, **terms)
    both = AW.run(pair, arm, d["start"], d["R"], d["p"], 0.05, sc, avoid_gain=0.0, **terms)
    for o in shared:
        assert np.array_equal(bits(zero[o]), bits(both[o])), (o, "avoid_gain = 0")
    assert (zero["clearance"] <= both["clearance"]).all() and zero["partner"].any() and (~zero["partner"]).any()
    assert np.array_equal(bits(zero["clearance"][~zero["partner"]]), bits(both["clearance"][~zero["partner"]]))


def test_without_a_scene_and_without_a_partner_nothing_is_near():
    """No static obstacle and the partner NaN: clearance +infinity, nearest (-1, -1), no push, and the five shared outputs are
    track_workload.run's bit for bit."""
    pair, n_pairs, T = "default/ztip", 8, 3
    d = PW.inputs(pair, n_pairs, T, True)
    terms = AW.terms_of(d)
    start = d["start"].copy()
    start[1::2] = np.nan
    got = PW.run(pair, start, d["R"], d["p"], 0.05, PW.NO_SCENE, **terms)
    plain = TW.run(JW.blocks_of(pair)[0], d["start"][0::2], d["R"][:, 0::2], d["p"][:, 0::2], 0.05, ff=terms["ff"][:, 0::2],
                   rest=terms["rest"][0::2], rest_gain=terms["rest_gain"], limits=terms["limits"])
    assert np.isposinf(got["clearance"][:, 0::2]).all() and (got["nearest"] == -1).all() and not got["push"].any()
    assert np.isposinf(got["min_clearance"][0::2]).all()
    for o in ("joints", "rates", "err"):
        assert np.array_equal(bits(got[o][:, 0::2]), bits(plain[o])), o
    for o in ("final_joints", "final_err"):
        assert np.array_equal(bits(got[o][0::2]), bits(plain[o])), o


def test_the_partner_s_capsules_are_what_clearance_workload_makes_of_them():
    """clearance() of a pair equals clearance_workload.reference of each row alone with the static capsules followed by
    partner_capsules(the partner's link points): clearance and gradient bit for bit, nearest the same, both arms, with and without a
    static scene; and both arms see the same axis distance where each names the other's link with its own."""
    pair = "default/default"
    blocks = JW.blocks_of(pair)
    q = TW.starts()[:16]
    for sc in (PW.NO_SCENE, CW.scene(pair, "open")):
        got = PW.clearance(blocks, q, sc)
        for r in range(len(q)):
            pts = CW.walk(blocks[(r ^ 1) & 1], q[(r ^ 1):(r ^ 1) + 1])[0][0]
            one = dict(spheres=sc["spheres"], capsules=np.concatenate([sc["capsules"], PW.partner_capsules(pts)]))
            ref = CW.reference(blocks, q[r:r + 1], np.array([r & 1], dtype=np.uint8), one)
            assert np.array_equal(bits(got["clearance"][r:r + 1]), bits(ref["clearance"])), r
            assert np.array_equal(got["nearest"][r], ref["nearest"][0]), r
            assert np.array_equal(bits(got["gradient"][r:r + 1]), bits(ref["gradient"])), r
    got = PW.clearance(blocks, q, PW.NO_SCENE)
    link, obs = got["nearest"][:, 0], got["nearest"][:, 1]
    mutual = (link[0::2] == obs[1::2]) & (link[1::2] == obs[0::2])
    assert mutual.any()
    assert (np.abs(got["clearance"][0::2] - got["clearance"][1::2])[mutual] <= 2 * CW.CLEARANCE_BOUND).all()


@pytest.mark.parametrize("pair", PW.PAIRS)
def test_the_seeded_pair_run_has_the_shares_and_the_bounds_hold_on_its_joints(pair):
    """The seeded pair run without a static scene (N_SEED robots, T_SEED steps, influence AW.INFLUENCE): at least 0.8 of the (row, step)
    cells pass the `kept` filter and at least 0.1 are kept and pushed with a link of the partner's as the nearest — the conditions the
    GPU per-step test relies on.  E (float64 against longdouble, BOTH arms' link points in the respective precision) is measured on
    the joints this run visits — the clearance on every cell, the gradient on the kept and pushed ones — and max(1e-13, 16 E) must
    not exceed clearance_workload's two bounds, which track_avoid_workload.step_tolerance uses."""
    r = PW.seeded_run(pair)
    n = r["keep"].size
    kept, partner = r["keep"].sum() / n, (r["keep"] & r["push"] & r["partner"]).sum() / n
    print(f"{pair}: {kept:.3f} of {n} cells kept, {partner:.3f} kept and pushed by the partner, the push acts on {r['push'].mean():.3f}")
    assert kept >= 0.8, float(kept)
    assert partner >= 0.1, float(partner)
    assert r["push"].any() and (~r["push"]).any()
    assert np.isfinite(r["joints"]).all() and (r["err"][:, :, 1] < 1.0).all()
    blocks = JW.blocks_of(pair)
    d = PW.inputs(pair, PW.N_SEED, PW.T_SEED, False)
    before = np.concatenate([d["start"][None], r["joints"][:-1]]).reshape(-1, 7)
    f64 = PW.clearance(blocks, before, PW.NO_SCENE)
    ld = PW.clearance(blocks, before, PW.NO_SCENE, dtype=np.longdouble)
    assert np.array_equal(bits(f64["clearance"].reshape(PW.T_SEED, -1)), bits(r["clearance"]))
    keep = (r["keep"] & r["push"]).reshape(-1)
    e_d = float(np.abs(f64["clearance"] - ld["clearance"]).max())
    e_g = float(np.abs(f64["gradient"] - ld["gradient"])[keep].max())
    print(f"{pair}: on the run's joints E_d {e_d:.3e}, E_g {e_g:.3e} (bounds {CW.CLEARANCE_BOUND:.1e}, {CW.GRADIENT_BOUND:.1e})")
    assert max(1e-13, 16 * e_d) <= CW.CLEARANCE_BOUND, e_d
    assert max(1e-13, 16 * e_g) <= CW.GRADIENT_BOUND, e_g


@pytest.mark.parametrize("pair", PW.PAIRS)
def test_the_per_step_cases_have_the_shares(pair):
    """The shapes and cases of the GPU per-step test (PW.STEP_CASES, N_STEP robots, T_STEP steps, both lambdas), on the reference's own
    run: at least 0.8 of the cells kept, at least 0.1 kept and pushed with a link of the partner's as the nearest."""
    for (name, influence, with_terms), lam in ((c, lam) for c in PW.STEP_CASES for lam in TW.LAMBDAS):
        d = PW.inputs(pair, PW.N_STEP, PW.T_STEP, with_terms)
        r = PW.run(pair, d["start"], d["R"], d["p"], lam, PW.scene_of(pair, name), influence=influence, **AW.terms_of(d))
        n = r["keep"].size
        kept, partner = r["keep"].sum() / n, (r["keep"] & r["push"] & r["partner"]).sum() / n
        print(f"{pair} scene={name} influence={influence} terms={with_terms} lambda={lam}: kept {kept:.3f}, pushed by the partner {partner:.3f}")
        assert kept >= 0.8 and partner >= 0.1, (name, influence, with_terms, lam, float(kept), float(partner))


@pytest.mark.parametrize("pair", PW.PAIRS)
def test_the_crossing_case_has_pairs_that_the_reference_moves_apart(pair):
    """The crossing case: without avoidance the two forearms end up through each other on every robot, and on at least 16 robots the
    reference's min_clearance (the smaller of the two arms') gains at least AW.MIN_GAIN with avoidance; the nearest pair at the end
    of the unobstructed run is forearm against forearm."""
    c = PW.crossing_case(pair)
    print(f"{pair}: {int(c['pairs'].sum())} of {PW.N_CROSS} robots gain at least {AW.MIN_GAIN} m, largest gain {c['gain'].max():.4f} m, "
          f"final_err with avoidance at most {c['avoid']['final_err'].max(axis=0).tolist()}")
    assert c["pairs"].sum() >= 16, int(c["pairs"].sum())
    assert (c["free"]["min_clearance"] < 0.0).all() and c["avoid"]["push"].any(axis=0).all()
    last = c["free"]["nearest"][-1]
    assert (last[:, 0] == 1).all() and (last[:, 1] == 1).all(), "link 1 against the partner's link 1 (no static obstacle: index 0 + 1)"
