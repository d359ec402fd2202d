#!/usr/bin/env python3
"""Cost of rsik_joint_rates on n rows of joints uniform in [-2, 2]^7 (right arm), twists and biases uniform in [-1, 1], lambda = 0.05:
  (a) rates only, no bias: 56 + 48 B read, 56 B written per row;
  (b) both outputs with bias: 56 + 48 + 56 B read, 56 + 48 B written per row;
  (c) the n_rep form on a sweep's output: rsik_solve_sweep of n / 16 reachable poses at 16 fractions of the interval, then
      rsik_joint_rates on its joints [16, n / 16, 7] in place, rates only (the sweep itself is not timed);
against what the library offered for the same rows before it:
  (d) rsik_jacobian writing the Jacobian only: 56 B read, 336 B written per row — the one launch a caller had to make before their
      solve could begin;
  (e) (d), then the torch chain on J: bmm (J J^T) + lambda^2 I, linalg.cholesky + cholesky_solve or linalg.solve, whichever is faster
      here (both are timed, the faster one is reported as (e)), bmm (J^T y).
Before anything is timed, (a) and (e) must agree: per row within the tolerance of tests/joint_rates_workload.py evaluated with torch
(sqrt(42) 1e-13 (|y| + g (2 |J| |y|)) + 128 * 2^-53 kappa(A) |z|), on the first 65 536 rows.
One process: untimed launches first, then rounds with the forms interleaved; HIP events on the stream; median [min, max] of the
rounds.  Prints one JSON line.

    python scripts/joint_rates_cost.py [--sizes 65536 1048576 4194304] [--launches 3] [--rounds 7]
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from reachy2_symbolic_ik_amd import SymbolicIK  # noqa: E402

LAMBDA = 0.05
BYTES = {"rates": 56 + 48 + 56, "both_bias": 56 + 48 + 56 + 56 + 48, "sweep_rates": 56 + 48 + 56, "jacobian": 56 + 336}


def time_launch(launch, k):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(k):
        launch()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / k  # us per call of `launch`


def torch_chain(jac_launch, J, v, how):
    """Form (e) as a callable: the Jacobian launch, then A = J J^T + lambda^2 I, the 6 x 6 solve, J^T y."""
    eye = (LAMBDA * LAMBDA) * torch.eye(6, dtype=torch.float64, device=J.device)
    rhs = v.unsqueeze(-1)

    def run():
        jac_launch()
        A = torch.bmm(J, J.transpose(1, 2)) + eye
        y = torch.cholesky_solve(rhs, torch.linalg.cholesky(A)) if how == "cholesky" else torch.linalg.solve(A, rhs)
        return torch.bmm(J.transpose(1, 2), y).squeeze(-1)

    return run


def tolerance(J, v):
    """tol_row of tests/joint_rates_workload.py (no bias), in torch."""
    U, s, _ = torch.linalg.svd(J, full_matrices=False)
    l2 = LAMBDA * LAMBDA
    c = torch.einsum("nji,nj->ni", U, v)
    yn = (c / (s * s + l2)).norm(dim=1)
    zn = (s * c / (s * s + l2)).norm(dim=1)
    g = (s / (s * s + l2)).max(dim=1).values
    kappa = (s[:, 0] ** 2 + l2) / (s[:, 5] ** 2 + l2)
    return 42 ** 0.5 * 1e-13 * (yn + g * 2.0 * s[:, 0] * yn) + 128.0 * 2.0 ** -53 * kappa * zn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[65536, 1048576, 4194304])
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", device=0)
    ik._upload()
    sv = ik.solver
    out = {"lambda": LAMBDA}
    for n in args.sizes:
        rng = np.random.default_rng(11)
        q = torch.as_tensor(rng.uniform(-2.0, 2.0, size=(n, 7))).to(dev)
        v = torch.as_tensor(rng.uniform(-1.0, 1.0, size=(n, 6))).to(dev)
        q0 = torch.as_tensor(rng.uniform(-1.0, 1.0, size=(n, 7))).to(dev)
        a = sv.joint_rates(q, v, damping=LAMBDA, plan_only=True)
        b = sv.joint_rates(q, v, damping=LAMBDA, bias_rates=q0, want=("rates", "achieved_twist"), plan_only=True)
        d = sv.jacobian(q, want=("jacobian",), plan_only=True)
        # a sweep's output: n / 16 reachable poses in front of the right shoulder, 16 fractions of the interval each
        m = max(n // 16, 1)
        pose = np.concatenate([np.array([[0.30], [-0.2], [-0.25]]) + rng.uniform(-0.08, 0.08, size=(3, m)),
                               np.array([[0.0], [-np.pi / 2], [0.0]]) + rng.uniform(-0.4, 0.4, size=(3, m))])
        sw = sv.solve_sweep(torch.as_tensor(np.ascontiguousarray(pose)).to(dev), torch.linspace(0.0, 1.0, 16, dtype=torch.float64), want_elbow=False)
        c = sv.joint_rates(sw["joints"], v[: 16 * m].reshape(16, m, 6), damping=LAMBDA, plan_only=True)
        forms = {"rates": a["launch"], "both_bias": b["launch"], "sweep_rates": c["launch"], "jacobian": d["launch"],
                 "chain_cholesky": torch_chain(d["launch"], d["jacobian"], v, "cholesky"),
                 "chain_solve": torch_chain(d["launch"], d["jacobian"], v, "solve")}
        for f in forms.values():  # untimed launches first: warm-up, settled clock
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        res = {"sweep_rows": 16 * m, "sweep_reachable_share": round(float(sw["reachable"].double().mean()), 4)}
        # the forms must agree before anything is timed
        k = min(n, 65536)  # (the tolerance takes a batched SVD: the first 65 536 rows)
        tol = tolerance(d["jacobian"][:k], v[:k])
        for how in ("cholesky", "solve"):
            err = (forms[f"chain_{how}"]()[:k] - a["rates"][:k]).norm(dim=1)
            res[f"rates_vs_chain_{how}_max_err"] = float(err.max())
            res[f"rates_vs_chain_{how}_max_err_over_tol"] = round(float((err / tol).max()), 4)
            assert bool((err <= tol).all()), res
        del tol, err
        t = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, f in forms.items():
                t[k].append(time_launch(f, args.launches))
        med = {k: float(np.median(x)) for k, x in t.items()}
        for k, x in t.items():
            res[f"{k}_us"] = round(med[k], 1)
            res[f"{k}_us_min_max"] = [round(float(np.min(x)), 1), round(float(np.max(x)), 1)]
        for k, rows in (("rates", n), ("both_bias", n), ("sweep_rates", 16 * m), ("jacobian", n)):
            res[f"{k}_GB_per_s"] = round(rows * BYTES[k] / (med[k] * 1e-6) / 1e9, 1)
        chain = min(("chain_cholesky", "chain_solve"), key=lambda k: med[k])
        res["chain"] = chain
        res["rates_over_jacobian"] = round(med["rates"] / med["jacobian"], 3)
        res["rates_over_chain"] = round(med["rates"] / med[chain], 5)
        res["both_bias_over_jacobian"] = round(med["both_bias"] / med["jacobian"], 3)
        res["sweep_rates_per_row_over_rates_per_row"] = round((med["sweep_rates"] / (16 * m)) / (med["rates"] / n), 3)
        out[str(n)] = res
        del a, b, c, d, sw, q, v, q0, forms
        torch.cuda.empty_cache()
    out["launches_per_median"] = args.launches * args.rounds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
