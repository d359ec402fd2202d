"""Inputs and the expected values of the rsik_solve_nearest tests (tests/test_solve_nearest_abi.py pins the helper on the checker
alone, tests/test_gpu_solve_nearest.py uses it on the GPU).  No test in this file.

The entry point is defined against rsik_solve_sweep: its answer for pose i is sample index[i] of the sweep over the same inputs.  So
the expected value is built from a sweep's outputs (the library's own on the GPU, the checker's tiled batch on the CPU) with NumPy:
d = (a - b + pi) % 2 pi - pi, c = sum_q w_q d_q d_q, the first argmin over the candidates."""
import numpy as np

from checker_support import reachable_rich
from sweep_workload import expected_tiled, sweep_poses, sweep_thetas  # noqa: F401  (the poses and theta arrays are the sweep tests')

GAP = 1e-9          # best and second-best cost further apart than this: the device's argmin must be NumPy's
COST_TOL = 1e-12    # c <= 7 pi^2; about 25 roundings of 1.1e-16 relative give <= 2e-13: a 5 x margin
KS = (1, 3, 8, 70)  # samples per pose of the main GPU tests: 70 gives 64 lanes a second, ragged round; 3 leaves lanes of 8 idle
N_MAIN = 1000       # three full 256-pose blocks, a ragged last one with a ragged last wave


def seeds(n, seed):
    """The joints each row wants to stay near: uniform in [-2, 2] per joint."""
    return np.random.default_rng(seed).uniform(-2.0, 2.0, size=(n, 7))


def main_case(kind, k):
    """Poses, arm bytes and seed rows of the main tests for one (kind, K)."""
    pos, eul, arm = sweep_poses(kind, 500 + k, N_MAIN)
    return pos, eul, arm, seeds(N_MAIN, 900 + k)


def main_thetas(policy, per_pose, k):
    return sweep_thetas(policy, per_pose, k, N_MAIN, 600 + k)


def costs(joints, seed, weights=None):
    """c [K, n] of sweep joints [K, n, 7] against seed [n, 7]: angle_diff as utils.py:486-490, summed q = 0 ... 6 in that order."""
    w = np.ones(7) if weights is None else np.asarray(weights, dtype=np.float64)
    d = (joints - seed[None] + np.pi) % (2 * np.pi) - np.pi
    c = np.zeros(joints.shape[:2])
    for q in range(7):
        c = c + (w[q] * d[..., q]) * d[..., q]
    return c


def nearest_from_sweep(sweep_out, seed, weights=None, skip_projected=False):
    """What rsik_solve_nearest must return, from a sweep's outputs (joints [K,n,7], projected [K,n], reachable [n]).  Returns
    c [K,n]; candidate [K,n]; index [n] (first argmin over the candidates, -1 without one); c_min [n] (inf without a candidate);
    gap [n]: second-best minus best candidate cost (inf with fewer than two candidates)."""
    with np.errstate(invalid="ignore"):
        c = costs(np.asarray(sweep_out["joints"]), np.asarray(seed), weights)
    cand = (np.asarray(sweep_out["reachable"]) != 0)[None] & ~np.isnan(c)
    if skip_projected:
        cand = cand & (np.asarray(sweep_out["projected"]) == 0)
    masked = np.where(cand, c, np.inf)
    index = np.argmin(masked, axis=0).astype(np.int32)  # (the first of equal minima)
    index[~cand.any(axis=0)] = -1
    ordered = np.sort(masked, axis=0)
    c_min = ordered[0]
    with np.errstate(invalid="ignore"):
        gap = ordered[1] - ordered[0] if len(ordered) > 1 else np.full(c_min.shape, np.inf)
    gap = np.where(np.isnan(gap), np.inf, gap)  # inf - inf: fewer than two candidates
    return dict(c=c, candidate=cand, index=index, c_min=c_min, gap=gap)


def gap_condition(expected, reachable, what=""):
    """The condition on the inputs (not a measurement): at least 95 % of the reachable rows have their best and second-best
    candidates more than GAP apart, so that on them the device's index must equal NumPy's argmin exactly."""
    ok = np.asarray(reachable) != 0
    clear = expected["gap"][ok] > GAP
    share = float(clear.mean()) if ok.any() else 1.0
    print(f"{what}: {int(ok.sum())} reachable rows, {share:.4f} of them with a gap above {GAP}")
    assert share >= 0.95, (what, share)
    return share


def skip_projected_case(orc, n=300, k=4):
    """The inputs of the RSIK_NEAREST_SKIP_PROJECTED tests, steered with the checker: per-pose explicit thetas such that sample 0
    of at least 20 poses projects while a later sample of the same pose does not (`mixed`), and at least one pose projects in
    every sample (`all_projected`).  Returns pos, eul, arm, thetas [k, n], the checker's tiled sweep, and the two row masks."""
    arm = np.zeros(n, dtype=np.uint8)
    pos, eul = reachable_rich(31, n, arm)
    arms = (orc.Arm("r_arm", 0.03), orc.Arm("l_arm", 0.03))
    probe = expected_tiled(orc, arms, pos, eul, arm, "fraction", np.linspace(0.0, 1.0, 33))
    thetas = np.random.default_rng(32).uniform(-np.pi, np.pi, size=(k, n))
    for i in np.flatnonzero(probe["reachable"]):
        yes, no = np.flatnonzero(probe["projected"][:, i] == 1), np.flatnonzero(probe["projected"][:, i] == 0)
        if len(yes) >= k and i % 3 == 0:
            thetas[:, i] = probe["theta"][yes[:k], i]
        elif len(yes) and len(no):
            thetas[0, i] = probe["theta"][yes[0], i]
            m = min(len(no), k - 1)  # (distinct angles: a repeated one would be an exact tie)
            thetas[1:1 + m, i] = probe["theta"][no[:m], i]
    ref = expected_tiled(orc, arms, pos, eul, arm, "explicit", thetas)
    ok = ref["reachable"].astype(bool)
    mixed = ok & (ref["projected"][0] == 1) & (ref["projected"][1:].min(axis=0) == 0)
    all_projected = ok & (ref["projected"].min(axis=0) == 1)
    print(f"{int(mixed.sum())} poses whose sample 0 projects and a later one does not, {int(all_projected.sum())} that project in every sample")
    assert mixed.sum() >= 20 and all_projected.sum() >= 1
    return pos, eul, arm, thetas, ref, mixed, all_projected
