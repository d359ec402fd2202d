"""Inputs and the checker-side expected values of the rsik_reach_map tests (tests/test_reach_map_abi.py pins the helper and the
inputs' conditions on the checker alone, tests/test_gpu_reach_map.py uses them on the GPU).  No test in this file."""
import math

import numpy as np

N_STATES = 11
THETA_NONE = 3
TWO_PI = 2 * math.pi


def map_positions(arm):
    """The 9 x 9 x 9 grid around the arm's shoulder s (an orc.Arm): s_x + linspace(-0.1, 0.7, 9), s_y + linspace(-0.5, 0.5, 9),
    s_z + linspace(-0.5, 0.5, 9); x varies slowest.  [729, 3]."""
    s = arm.field("shoulder_position")
    gx, gy, gz = np.meshgrid(s[0] + np.linspace(-0.1, 0.7, 9), s[1] + np.linspace(-0.5, 0.5, 9), s[2] + np.linspace(-0.5, 0.5, 9),
                             indexing="ij")
    return np.ascontiguousarray(np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1))


def map_orientations(n_rot, seed):
    """[n_rot, 3] Euler angles, uniform in [-pi, pi]^3."""
    return np.random.default_rng(seed).uniform(-np.pi, np.pi, size=(n_rot, 3))


def map_case(arms, kind, n_rot=130, seed=7):
    """The named test grid: (P [729,3], arm_ids [729] uint8 or None, E [n_rot,3]).  kind "r" / "l": every voxel around that arm's
    shoulder, no arm bytes; "mixed": a random arm byte per position, each voxel taken around its own arm's shoulder."""
    E = map_orientations(n_rot, seed)
    if kind != "mixed":
        return map_positions(arms[int(kind == "l")]), None, E
    arm_ids = np.random.default_rng(seed + 1000).integers(0, 2, size=729).astype(np.uint8)
    P = np.where(arm_ids[:, None] != 0, map_positions(arms[1]), map_positions(arms[0]))
    return np.ascontiguousarray(P), arm_ids, E


def tile(P, arm_ids, E):
    """The n_pos * n_rot poses of a map, position-major (pose (i, j) is row i * n_rot + j): pos, eul, arm byte per pose."""
    n_pos, n_rot = len(P), len(E)
    arm_ids = np.zeros(n_pos, dtype=np.uint8) if arm_ids is None else np.asarray(arm_ids, dtype=np.uint8)
    if arm_ids.ndim == 0:  # one arm for every position (arm_uniform)
        arm_ids = np.full(n_pos, arm_ids, dtype=np.uint8)
    return np.repeat(P, n_rot, axis=0), np.tile(E, (n_pos, 1)), np.repeat(arm_ids, n_rot)


def widths(interval, reachable):
    """Per pose: i1 - i0, plus 2 pi where i0 > i1; 0.0 where the pose is not reachable."""
    i0, i1 = interval[..., 0], interval[..., 1]
    ok = np.asarray(reachable).astype(bool)
    w = np.where(i0 > i1, (i1 - i0) + TWO_PI, i1 - i0)
    return np.where(ok, w, 0.0)


def pack_mask(reachable):
    """[n_pos, n_rot] flags -> [n_pos, ceil(n_rot / 64)] uint64: bit (j % 64) of word (j // 64) is flag (i, j), padding bits 0."""
    r = np.asarray(reachable).astype(bool)
    n_pos, n_rot = r.shape
    words = (n_rot + 63) // 64
    padded = np.zeros((n_pos, words * 64), dtype=np.uint64)
    padded[:, :n_rot] = r
    shifts = np.arange(64, dtype=np.uint64)
    return (padded.reshape(n_pos, words, 64) << shifts).sum(axis=2, dtype=np.uint64)


def reduce_map(reachable, state, interval, n_pos, n_rot):
    """The four arrays of rsik_reach_map from per-pose results laid out position-major: NumPy counts, math.fsum per position."""
    ok = np.asarray(reachable).reshape(n_pos, n_rot).astype(bool)
    st = np.asarray(state).reshape(n_pos, n_rot)
    w = widths(np.asarray(interval).reshape(n_pos, n_rot, 2), ok)
    return {
        "count": ok.sum(axis=1).astype(np.uint32),
        "state_count": np.stack([(st == c).sum(axis=1) for c in range(N_STATES)], axis=1).astype(np.uint32),
        "theta_measure": np.array([math.fsum(row) for row in w], dtype=np.float64).reshape(n_pos),
        "mask": pack_mask(ok),
        "reachable": ok, "state": st, "width": w,
    }


def expected_map(orc, arms, P, arm_ids, E, nthreads=1):
    """What the checker says a map holds: ONE orc.solve_batch(theta_policy = 3, is_reachable only) over the tiled poses, reduced
    with reduce_map.  arms: (orc.Arm r, orc.Arm l); arm_ids: [n_pos] bytes, one arm id (0 / 1) for every
    position, or None for the r slot."""
    pos, eul, arm = tile(P, arm_ids, E)
    ref = orc.solve_batch(arms[0], arms[1], pos, eul, arm_id=arm, theta_policy=THETA_NONE, nthreads=nthreads)
    return reduce_map(ref["reachable"], ref["state"], ref["interval"], len(P), len(E))


def rounding_bound(n_rot):
    """rsik.h: the order of the sum is the kernel's own, so theta_measure is defined to n_rot^2 * 2 pi * 2^-53."""
    return float(n_rot) ** 2 * TWO_PI * 2.0 ** -53
