"""Inputs and the checker-side expected values of the rsik_solve_sweep tests (tests/test_solve_sweep_abi.py pins the helper on
the checker alone, tests/test_gpu_solve_sweep.py uses it on the GPU).  No test in this file."""
import numpy as np

from checker_support import reachable_rich, state_workload

THETA_EXPLICIT, THETA_FRACTION = 1, 2
POLICY = {"explicit": THETA_EXPLICIT, "fraction": THETA_FRACTION}


def sweep_poses(kind, seed, n):
    """Even rows: state_workload (every outcome of is_reachable); odd rows: reachable_rich.  kind "r" / "l" / "mixed" (a random
    arm byte per row, so r and l alternate inside every wave).  Returns pos [n,3], eul [n,3], arm [n] uint8."""
    pos, eul, arm = state_workload(seed, n, arm={"r": 0, "l": 1, "mixed": None}[kind])
    p2, e2 = reachable_rich(seed + 1, n, arm)
    odd = np.arange(n) % 2 == 1
    pos[odd], eul[odd] = p2[odd], e2[odd]
    if kind == "mixed" and n >= 512:
        waves = arm[: n - n % 64].reshape(-1, 64).sum(axis=1)
        assert ((waves > 0) & (waves < 64)).all(), "r and l must alternate inside every wave"
    return pos, eul, arm


def sweep_thetas(policy, per_pose, k, n, seed):
    """[k] (shared) or [k, n] (per pose).  Fractions: 0.0 first and 1.0 last (when k > 1), uniform in [0, 1] between; explicit
    angles: uniform in [-2 pi, 2 pi], so they also lie outside the interval."""
    rng = np.random.default_rng(seed)
    shape = (k, n) if per_pose else (k,)
    if policy == "explicit":
        return rng.uniform(-2 * np.pi, 2 * np.pi, size=shape)
    u = rng.uniform(0.0, 1.0, size=shape)
    u[0] = 0.0
    if k > 1:
        u[-1] = 1.0
    return u


def columns(thetas, n):
    """The [k, n] form of either form of thetas."""
    thetas = np.asarray(thetas, dtype=np.float64)
    return np.ascontiguousarray(thetas if thetas.ndim == 2 else np.repeat(thetas[:, None], n, axis=1))


def fraction_theta(interval, u):
    """theta of RSIK_THETA_FRACTION: i0 + u * (i1' - i0), i1' = i1 + 2 pi where the interval wraps; unfused, as the kernels."""
    a, b = interval[:, 0], interval[:, 1].copy()
    b[a > b] += 2 * np.pi
    return a + u * (b - a)


def expected_tiled(orc, arms, pos, eul, arm, policy, thetas, nthreads=1):
    """What the checker says a sweep returns: the poses tiled k times and the theta columns laid end to end go through ONE
    orc.solve_batch(theta_policy, theta_in) — every row a fresh is_reachable followed by one get_joints — and come back
    sample-major: joints [k,n,7], elbow [k,n,3], projected [k,n], theta [k,n]; interval / reachable / state [n] of sample 0."""
    n = len(pos)
    th = columns(thetas, n)
    k = th.shape[0]
    ref = orc.solve_batch(arms[0], arms[1], np.tile(pos, (k, 1)), np.tile(eul, (k, 1)), arm_id=np.tile(arm, k),
                          theta_policy=POLICY[policy], theta_in=th.reshape(-1), nthreads=nthreads)
    out = {key: ref[key].reshape((k, n) + ref[key].shape[1:]) for key in ("joints", "elbow", "projected")}
    for key in ("interval", "reachable", "state"):
        full = ref[key].reshape((k, n) + ref[key].shape[1:])
        assert all(np.array_equal(full[0], full[q], equal_nan=True) for q in range(k)), key
        out[key] = full[0]
    theta = np.stack([fraction_theta(out["interval"], th[q]) for q in range(k)]) if policy == "fraction" else th.copy()
    theta[:, out["reachable"] == 0] = np.nan
    out["theta"] = theta
    return out
