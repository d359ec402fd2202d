#!/usr/bin/env python3
"""Cost of rsik_jacobian on n rows of joints uniform in [-2, 2]^7 (right arm), three forms:
  (a) all three outputs (jacobian, null_vector, manipulability): 56 B read, 336 + 56 + 8 B written per row;
  (b) manipulability only: 56 B read, 8 B written per row;
  (c) the n_rep form on a sweep's output: rsik_solve_sweep of n / 16 reachable poses at 16 fractions of the interval, then
      rsik_jacobian on its joints [16, n / 16, 7] in place, manipulability only and all three outputs (the sweep itself is not timed);
against what the library offered for the same rows before it:
  (d) one rsik_forward_kinematics launch (position and rotation: 56 B read, 96 B written per row);
  (e) the central-difference construction: 14 rsik_forward_kinematics launches on joints +- h e_k (the perturbed rows are built ahead
      and not timed), the torch assembly of J from the differences, torch.linalg.det on the seven 6 x 6 sub-matrices and the norm;
      sizes up to --fd-max-rows only (it holds about 1.3 KB per row).
HIP events on the stream, the forms interleaved in rounds in one process, medians and the spread of the rounds.  For form (b) the
fraction of the fp64 issue rate: the kernel's fp64 vector instructions per row (counted in its gfx950 assembly: --fp64-instr) over the
rate rsik_debug_math op 6 sustains in this process (scripts/valu_peak.py's calibration; profiles/r01/fp64_valu_calibration.txt has
5.03e11 wave-instructions/s).  Prints one JSON line.

    python scripts/jacobian_cost.py [--sizes 65536 1048576 4194304 16777216] [--launches 3] [--rounds 7]
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

BYTES = {"all": (56, 336 + 56 + 8), "manipulability": (56, 8), "fk": (56, 96)}
FP64_INSTR = 876  # v_*_f64 in jacobian_kernel<false, false, false, true> (hipcc -S --offload-arch=gfx950; the rare far-angle branch included)


def time_launch(launch, k):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(k):
        launch()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / k  # us per call of `launch`


def valu_rate(sv, n=1 << 22, reps=10):
    """fp64 wave-instructions per second of rsik_debug_math op 6 (8 x 2048 dependent v_fma_f64 per lane), as scripts/valu_peak.py."""
    a = torch.rand(n, dtype=torch.float64, device="cuda")
    b = torch.full((n,), 0.999, dtype=torch.float64, device="cuda")
    for _ in range(3):
        sv.debug_math(6, a, b)
    torch.cuda.synchronize()
    us = time_launch(lambda: sv.debug_math(6, a, b), reps)
    return (n / 64) * 8 * 2048 / (us * 1e-6)


def fd_form(sv, q, h=1e-6):
    """Form (e) as a callable: J by central differences of rsik_forward_kinematics, the signed minors with torch.linalg.det, the norm."""
    n = q.shape[0]
    eye = torch.eye(7, dtype=torch.float64, device=q.device) * h
    plus = [(q + eye[k]).contiguous() for k in range(7)]
    minus = [(q - eye[k]).contiguous() for k in range(7)]
    J = torch.empty((n, 6, 7), dtype=torch.float64, device=q.device)
    cols = [[c for c in range(7) if c != i] for i in range(7)]

    def run():
        _, R0 = sv.forward_kinematics(q)
        for k in range(7):
            pp, Rp = sv.forward_kinematics(plus[k])
            pm, Rm = sv.forward_kinematics(minus[k])
            J[:, :3, k] = (pp - pm) / (2 * h)
            W = torch.bmm((Rp - Rm) / (2 * h), R0.transpose(1, 2))
            J[:, 3, k], J[:, 4, k], J[:, 5, k] = W[:, 2, 1], W[:, 0, 2], W[:, 1, 0]
        null = torch.stack([(-1.0) ** i * torch.linalg.det(J[:, :, cols[i]]) for i in range(7)], dim=1)
        return J, null, null.norm(dim=1)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[65536, 1048576, 4194304, 16777216])
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--fd-max-rows", type=int, default=4194304)
    ap.add_argument("--fp64-instr", type=int, default=FP64_INSTR)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", device=0)
    ik._upload()
    sv = ik.solver
    out = {"fp64_wave_instr_per_s": float(f"{valu_rate(sv):.4g}"), "fp64_instr_per_row": args.fp64_instr}
    for n in args.sizes:
        q = torch.as_tensor(np.random.default_rng(11).uniform(-2.0, 2.0, size=(n, 7))).to(dev)
        a = sv.jacobian(q, plan_only=True)
        b = sv.jacobian(q, want=("manipulability",), plan_only=True)
        fk_out = (torch.empty((n, 3), dtype=torch.float64, device=dev), torch.empty((n, 3, 3), dtype=torch.float64, device=dev))
        d = sv.plan("rsik_forward_kinematics", n, q.data_ptr(), None, 0, fk_out[0].data_ptr(), fk_out[1].data_ptr())
        # a sweep's output: n / 16 reachable poses in front of the right shoulder, 16 fractions of the interval each
        m = max(n // 16, 1)
        rng = np.random.default_rng(12)
        pose = np.concatenate([np.array([[0.30], [-0.2], [-0.25]]) + rng.uniform(-0.08, 0.08, size=(3, m)),
                               np.array([[0.0], [-np.pi / 2], [0.0]]) + rng.uniform(-0.4, 0.4, size=(3, m))])
        sw = sv.solve_sweep(torch.as_tensor(np.ascontiguousarray(pose)).to(dev), torch.linspace(0.0, 1.0, 16, dtype=torch.float64), want_elbow=False)
        c1 = sv.jacobian(sw["joints"], want=("manipulability",), plan_only=True)
        c3 = sv.jacobian(sw["joints"], plan_only=True)
        forms = {"all": a["launch"], "manipulability": b["launch"], "sweep_manipulability": c1["launch"], "sweep_all": c3["launch"], "fk": d}
        if n <= args.fd_max_rows:
            forms["fd_and_det"] = fd_form(sv, q)
        for f in forms.values():  # warm-up, settled clock
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        res = {"sweep_rows": 16 * m, "sweep_reachable_share": round(float(sw["reachable"].double().mean()), 4)}
        if "fd_and_det" in forms:  # the forms must agree (section 6 of the measuring guide): J to 1e-8, the minors to 1e-7
            Jf, nf, wf = forms["fd_and_det"]()
            res["fd_J_max_diff"] = float((Jf - a["jacobian"]).abs().max())
            res["fd_null_max_diff"] = float((nf - a["null_vector"]).abs().max())
            assert res["fd_J_max_diff"] < 1e-8 and res["fd_null_max_diff"] < 1e-7, res
            del Jf, nf, wf
        assert torch.equal(a["manipulability"], b["manipulability"])
        t = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, f in forms.items():
                t[k].append(time_launch(f, args.launches if k != "fd_and_det" else 1))
        med = {k: float(np.median(v)) for k, v in t.items()}
        for k, v in t.items():
            res[f"{k}_us"] = round(med[k], 1)
            res[f"{k}_us_min_max"] = [round(float(np.min(v)), 1), round(float(np.max(v)), 1)]
        for k, rows in (("all", n), ("manipulability", n), ("fk", n), ("sweep_manipulability", 16 * m), ("sweep_all", 16 * m)):
            rd, wr = BYTES["fk" if k == "fk" else "all" if k.endswith("all") else "manipulability"]
            res[f"{k}_GB_per_s"] = round(rows * (rd + wr) / (med[k] * 1e-6) / 1e9, 1)
            res[f"{k}_rows_per_s"] = float(f"{rows / (med[k] * 1e-6):.4g}")
        res["all_over_fk"] = round(med["all"] / med["fk"], 3)
        res["all_over_14_fk"] = round(med["all"] / (14 * med["fk"]), 4)
        res["manipulability_over_fk"] = round(med["manipulability"] / med["fk"], 3)
        if "fd_and_det" in med:
            res["all_over_fd_and_det"] = round(med["all"] / med["fd_and_det"], 5)
            res["manipulability_over_fd_and_det"] = round(med["manipulability"] / med["fd_and_det"], 5)
        for k, rows in (("manipulability", n), ("sweep_manipulability", 16 * m)):
            res[f"{k}_fp64_issue_share"] = round((rows / 64) * args.fp64_instr / (med[k] * 1e-6) / out["fp64_wave_instr_per_s"], 3)
        out[str(n)] = res
        del a, b, c1, c3, d, sw, q, fk_out, forms
        torch.cuda.empty_cache()
    out["launches_per_median"] = args.launches * args.rounds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
