"""Arm pairs for the launches that read an arm byte per row (tests/test_arm_pairs_checker.py pins their inputs on the checker alone,
tests/test_gpu_arm_forms.py launches them on the GPU).  No test in this file.

rsik_solve / rsik_solve_rows, rsik_solve_sweep, rsik_solve_nearest and rsik_solve_path pick their kernel with launch_form() and
tip_on_z() (csrc/rsik_lib.hip): FORM 0 one arm for the launch; FORM 2 an arm byte per row and every constant without a handedness
read once as a scalar, legal only when the two uploaded blocks are mirror images; FORM 1 an arm byte per row and every constant read
per lane from LDS; TIPZ when both tips lie on the goal z axis.  A pair is named "<r slot>/<l slot>" after the geometry uploaded into
each slot; PAIRS says what each must launch, and upload() asserts it on the uploaded blocks before anything runs."""
import contextlib
import io

import numpy as np

from oracle import oracle as orc
from test_oracle_golden import CUSTOM_GEOMETRY

DEFAULT = dict(singularity_offset=0.03)
CUSTOM = CUSTOM_GEOMETRY  # G9: the tip has x / y components, u != f, other shoulder offsets and limits
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


def checker_arms(pair):
    """The checker's two arms of a pair: (orc.Arm of the r slot, orc.Arm of the l slot)."""
    r, l = pair.split("/")
    return orc.Arm("r_arm", **GEOMETRY[r]), orc.Arm("l_arm", **GEOMETRY[l])


def is_sided(i):
    """arm_const_is_sided (csrc/rsik_kernel_solve.hpp) restated: the entries a mirror-image pair may differ in."""
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
        kw = dict(GEOMETRY[name])
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


def upload(pair):
    """A fresh HipSolver with the pair's two geometries uploaded, each slot from a SymbolicIK(arm, solver=..., **geometry)._upload();
    the uploaded blocks are checked against the pair's name before the solver is handed out."""
    from reachy2_symbolic_ik_amd import HipSolver, SymbolicIK

    solver = HipSolver(0)
    with contextlib.redirect_stdout(io.StringIO()):
        for arm, name in zip(ARM_NAMES, pair.split("/")):
            SymbolicIK(arm, solver=solver, **GEOMETRY[name])._upload()
    blocks = list(solver._arm_blocks)
    check_blocks(pair, blocks)
    for got, want in zip(blocks, packed_blocks(pair)):
        assert got.tobytes() == want.tobytes(), f"{pair}: the uploaded block is not the geometry's"
    return solver


def solve_fractions(k, n):
    """One fraction of the interval per row for rsik_solve(RSIK_THETA_FRACTION): uniform in [0, 1]."""
    return np.random.default_rng(650 + k).uniform(0.0, 1.0, size=n)
