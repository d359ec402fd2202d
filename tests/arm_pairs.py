"""Arm pairs for the launches that read an arm byte per row (tests/test_arm_pairs_checker.py pins their inputs on the checker alone,
tests/test_gpu_arm_forms.py launches them on the GPU).  No test in this file.  The control launches (rsik_control_discrete(_rows),
rsik_control_continuous_step / _run) and rsik_theta_from_joints have pairs of their own further down: CONTROL_PAIRS and threshold_family()
(tests/test_control_pairs_checker.py on the checker alone, tests/test_gpu_control_arm_pairs.py on the GPU).

rsik_solve / rsik_solve_rows, rsik_solve_sweep, rsik_solve_nearest and rsik_solve_path pick their kernel with launch_form() and
tip_on_z() (csrc/rsik_lib.hip): FORM 0 one arm for the launch; FORM 2 an arm byte per row and every constant without a handedness
read once as a scalar, legal only when the two uploaded blocks are mirror images; FORM 1 an arm byte per row and every constant read
per lane from LDS; TIPZ when both tips lie on the goal z axis.  A pair is named "<r slot>/<l slot>" after the geometry uploaded into
each slot; PAIRS says what each must launch, and upload() asserts it on the uploaded blocks before anything runs."""
import contextlib
import io

import numpy as np

from checker_support import CUSTOM_GEOMETRY
from oracle import oracle as orc

DEFAULT = dict(singularity_offset=0.03)
CUSTOM = CUSTOM_GEOMETRY  # G9 (tests/checker_support.py): the tip has x / y components, u != f, other shoulder offsets and limits
ZTIP = dict(  # G20 (must match oracle/gen_golden.py ZTIP_GEOMETRY): other segment lengths and limits, the tip still on z
    ik_parameters={
        "r_shoulder_position": np.array([0.0, -0.2, 0.0]), "r_shoulder_orientation": [-15, 0, 10],
        "r_upper_arm_size": 0.30, "r_forearm_size": 0.26, "r_tip_position": np.array([0.0, 0.0, 0.09]),
        "l_shoulder_position": np.array([0.0, 0.2, 0.0]), "l_shoulder_orientation": [15, 0, -10],
        "l_upper_arm_size": 0.30, "l_forearm_size": 0.26, "l_tip_position": np.array([0.0, 0.0, 0.09]),
    },
    elbow_limit=115, wrist_limit=38.0, backward_limit=0.035, singularity_offset=0.05, singularity_limit_coeff=0.8)
GEOMETRY = {"default": DEFAULT, "custom": CUSTOM, "ztip": ZTIP}

# pair -> (FORM, FORM under RSIK_OPT_NO_MIRROR, TIPZ); RSIK_OPT_NO_TIPZ makes every TIPZ false
PAIRS = {
    "custom/custom": (2, 1, False),
    "custom/default": (1, 1, False),
    "default/custom": (1, 1, False),
    "default/ztip": (1, 1, True),
    "ztip/default": (1, 1, True),
}
NON_MIRROR = tuple(pair for pair, (form, _, _) in PAIRS.items() if form == 1)
ARM_NAMES = ("r_arm", "l_arm")


def geometry_of(name):
    """The geometry of a slot name: a key of GEOMETRY, or "<key>@<offset>" for that geometry with another singularity_offset, the
    offset a number ("default@-1.01") or a label of threshold_offsets() ("default@s*-1e-3")."""
    base, at, so = name.partition("@")
    if not at:
        return GEOMETRY[base]
    return dict(GEOMETRY[base], singularity_offset=threshold_offsets()[so] if so in THRESHOLD_LABELS else float(so))


def checker_arms(pair):
    """The checker's two arms of a pair: (orc.Arm of the r slot, orc.Arm of the l slot)."""
    r, l = pair.split("/")
    return orc.Arm("r_arm", **geometry_of(r)), orc.Arm("l_arm", **geometry_of(l))


def is_sided(i):
    """arm_const_is_sided (csrc/rsik_tables.hpp) restated: the entries a mirror-image pair may differ in."""
    from reachy2_symbolic_ik_amd import constants as K

    return (i in (K.C_SHOULDER + 1, K.C_TIPL + 1, K.C_ES + 1, K.C_SIDE) or K.C_MST <= i < K.C_TSH + 3
            or K.C_PLANE_P <= i < K.C_PROJ_CENTER + 3)


def launch_of(blocks, no_mirror=0, no_tipz=0):
    """(FORM, TIPZ) of a launch with an arm byte per row on these two constant blocks: launch_form and tip_on_z restated."""
    from reachy2_symbolic_ik_amd import constants as K

    r, l = (np.ascontiguousarray(b, dtype=np.float64) for b in blocks)
    same = all(r[i:i + 1].tobytes() == l[i:i + 1].tobytes() for i in range(K.ARM_CONSTS_COUNT) if not is_sided(i))
    tipz = all(b[K.C_TIPL] == 0.0 and b[K.C_TIPL + 1] == 0.0 for b in (r, l))
    return (2 if same and not no_mirror else 1), (tipz and not no_tipz)


def packed_blocks(pair):
    """The constant blocks SymbolicIK packs for the two slots of a pair, without a device."""
    from reachy2_symbolic_ik_amd.constants import ArmGeometry, default_ik_parameters

    out = []
    for arm, name in zip(ARM_NAMES, pair.split("/")):
        kw = dict(geometry_of(name))
        out.append(ArmGeometry(arm, kw.pop("ik_parameters", None) or default_ik_parameters(), **kw).pack())
    return out


def check_blocks(pair, blocks):
    """The pair is what its name says, on the constant blocks themselves."""
    from reachy2_symbolic_ik_amd import constants as K

    form, form_no_mirror, tipz = PAIRS[pair]
    r, l = blocks
    assert r is not None and l is not None and r.shape == l.shape == (K.ARM_CONSTS_COUNT,), pair
    assert r[K.C_SIDE] == 1.0 and l[K.C_SIDE] == -1.0, pair
    if form == 1:
        assert r[K.C_UPPER_ARM] != l[K.C_UPPER_ARM], f"{pair}: the upper arms of a non-mirror pair must differ"
        assert abs(r[K.C_UPPER_ARM] - l[K.C_UPPER_ARM]) > 0.01 and r[K.C_ELBOW_LIMIT] != l[K.C_ELBOW_LIMIT], pair
    else:
        assert r[K.C_UPPER_ARM] == l[K.C_UPPER_ARM] != 0.28, f"{pair}: a mirror pair that is not the default one"
    on_z = [b[K.C_TIPL] == 0.0 and b[K.C_TIPL + 1] == 0.0 for b in (r, l)]
    assert all(on_z) == tipz, f"{pair}: tip x / y entries {r[K.C_TIPL:K.C_TIPL + 2]}, {l[K.C_TIPL:K.C_TIPL + 2]}"
    assert launch_of(blocks) == (form, tipz) and launch_of(blocks, no_mirror=1) == (form_no_mirror, tipz), pair
    assert launch_of(blocks, no_tipz=1) == (form, False), pair


def upload(pair, check=check_blocks):
    """A fresh HipSolver with the pair's two geometries uploaded, each slot from a SymbolicIK(arm, solver=..., **geometry)._upload();
    the uploaded blocks are checked against the pair's name before the solver is handed out."""
    from reachy2_symbolic_ik_amd import HipSolver, SymbolicIK

    solver = HipSolver(0)
    with contextlib.redirect_stdout(io.StringIO()):
        for arm, name in zip(ARM_NAMES, pair.split("/")):
            SymbolicIK(arm, solver=solver, **geometry_of(name))._upload()
    blocks = list(solver._arm_blocks)
    check(pair, blocks)
    for got, want in zip(blocks, packed_blocks(pair)):
        assert got.tobytes() == want.tobytes(), f"{pair}: the uploaded block is not the geometry's"
    return solver


def solve_fractions(k, n):
    """One fraction of the interval per row for rsik_solve(RSIK_THETA_FRACTION): uniform in [0, 1]."""
    return np.random.default_rng(650 + k).uniform(0.0, 1.0, size=n)


# ------------------------------------------------------------------------------------------ the control launches
# rsik_control_discrete(_rows), rsik_control_continuous_step / _run and rsik_theta_from_joints on arm pairs (tests/test_control_pairs_checker.py
# pins their inputs on the checker alone, tests/test_gpu_control_arm_pairs.py launches them).  The control kernels compile the singularity-plane
# half of is_elbow_ok out of a launch (PLANE = false) when singularity_plane_binds (csrc/rsik_lib.hip) says it cannot fail on either arm;
# rsik_theta_from_joints picks its kernel with launch_form().  pair -> (FORM of rsik_theta_from_joints, PLANE of the control kernels):
CONTROL_PAIRS = {
    "default/custom": (1, True),              # both planes bind, non-mirror, the l tip off the z axis
    "ztip/default": (1, True),                # both planes bind, non-mirror, both tips on z
    "custom/custom": (2, True),               # mirror, non-default: slope 0.8, offset 0.05, other shoulder offsets, tip with x / y
    "default@-1.01/ztip@-1.01": (1, False),   # non-mirror, no plane on either arm
    "default@-1.01/default@0.03": (1, True),  # the same arm but for the plane: PLANE = true although r never binds
}


def plane_margin(block):
    """rhs - reach_max of singularity_plane_binds (csrc/rsik_lib.hip) for one constant block: the plane half of is_elbow_ok cannot
    fail on this arm when this exceeds 1e-6."""
    from reachy2_symbolic_ik_amd import constants as K

    c = np.asarray(block, dtype=np.float64)
    sc = c[K.C_SING_COEFF]
    rhs = c[K.C_ES + 2] - c[K.C_SING_OFFSET] - sc * c[K.C_ES]
    reach_max = c[K.C_SHOULDER + 2] - sc * c[K.C_SHOULDER] + c[K.C_UPPER_ARM] * np.sqrt(1.0 + sc * sc)
    return float(rhs - reach_max)


def plane_binds(blocks):
    """singularity_plane_binds restated: PLANE of a control launch on these two constant blocks."""
    return any(not (plane_margin(b) > 1e-6) for b in blocks)


def threshold_offset():
    """s*: the singularity_offset of the default mirror pair at which rhs == reach_max in singularity_plane_binds, from the packed
    blocks (the smaller of the two slots' values: they agree to rounding).  About -0.3705."""
    from reachy2_symbolic_ik_amd import constants as K

    return float(min(b[K.C_SING_OFFSET] + plane_margin(b) for b in packed_blocks("default/default")))


S3 = -0.30
THRESHOLD_LABELS = ("s*-1e-3", "s*+1e-3", "s3")


def threshold_offsets():
    """The offsets behind THRESHOLD_LABELS: s* - 1e-3, s* + 1e-3 and S3, s* resolved from the packed blocks when asked for."""
    s = threshold_offset()
    return dict(zip(THRESHOLD_LABELS, (s - 1e-3, s + 1e-3, S3)))


def threshold_family():
    """The default mirror pair at the three offsets of THRESHOLD_LABELS, pair name -> (FORM, PLANE): s* - 1e-3 must come out
    PLANE = false, s* + 1e-3 PLANE = true, and s3 = S3 = -0.30 PLANE = true.  s3 was chosen on the checker alone so that the plane half
    of is_elbow_ok fails on between 1 % and 10 % of the grid points the discrete search evaluates on control_workload's 1000 rows
    (nb_search_points 64, preferred angle -4 pi / 6).  Measured share: 0.0418 (r rows 0.0462, l rows 0.0375);
    tests/test_control_pairs_checker.py::test_threshold_family measures it again and asserts it."""
    return {f"default@{label}/default@{label}": (2, plane) for label, plane in zip(THRESHOLD_LABELS, (False, True, True))}


def control_expectation(pair):
    return CONTROL_PAIRS[pair] if pair in CONTROL_PAIRS else threshold_family()[pair]


def upload_control(pair):
    """upload() for a pair of CONTROL_PAIRS or threshold_family(): the uploaded blocks are checked with check_control_blocks, and with
    check_blocks too where the pair is also one of PAIRS."""
    def check(pair, blocks):
        check_control_blocks(pair, blocks)
        if pair in PAIRS:
            check_blocks(pair, blocks)

    return upload(pair, check=check)


def check_control_blocks(pair, blocks):
    """A control pair is what its name says, on the constant blocks themselves: FORM, PLANE, and what the slots differ in."""
    from reachy2_symbolic_ik_amd import constants as K

    form, plane = control_expectation(pair)
    r, l = blocks
    assert r is not None and l is not None and r.shape == l.shape == (K.ARM_CONSTS_COUNT,), pair
    assert r[K.C_SIDE] == 1.0 and l[K.C_SIDE] == -1.0, pair
    assert launch_of(blocks)[0] == form and launch_of(blocks, no_mirror=1)[0] == 1, pair
    assert plane_binds(blocks) == plane, (pair, [plane_margin(b) for b in blocks])
    differ = {i for i in range(K.ARM_CONSTS_COUNT) if not is_sided(i) and r[i:i + 1].tobytes() != l[i:i + 1].tobytes()}
    if pair == "default@-1.01/default@0.03":
        # the same arm but for the plane: the offset, and the two constants without a handedness that are derived from it
        assert {K.C_SING_OFFSET, K.C_PLANE_K} <= differ <= {K.C_SING_OFFSET, K.C_PLANE_K, K.C_PROJ_RADIUS}, (pair, sorted(differ))
        assert plane_margin(r) > 0.5 and plane_margin(l) < -0.3, pair  # r never binds, l does
    elif pair == "default@-1.01/ztip@-1.01":
        assert min(plane_margin(b) for b in blocks) > 0.5 and r[K.C_UPPER_ARM] != l[K.C_UPPER_ARM], pair
    elif form == 1:
        assert abs(r[K.C_UPPER_ARM] - l[K.C_UPPER_ARM]) > 0.01 and r[K.C_ELBOW_LIMIT] != l[K.C_ELBOW_LIMIT], pair
        assert r[K.C_SING_COEFF] != l[K.C_SING_COEFF] and r[K.C_SING_OFFSET] != l[K.C_SING_OFFSET], pair
    else:
        assert not differ, (pair, sorted(differ))
    if pair in threshold_family():
        so = geometry_of(pair.split("/")[0])["singularity_offset"]
        assert r[K.C_SING_OFFSET] == l[K.C_SING_OFFSET] == so and r[K.C_UPPER_ARM] == 0.28, (pair, so)
    if pair == "custom/custom":
        assert r[K.C_SING_COEFF] == 0.8 and r[K.C_SING_OFFSET] == 0.05 and r[K.C_TIPL] != 0.0 and r[K.C_SHOULDER] != 0.0, pair
