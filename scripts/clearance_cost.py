#!/usr/bin/env python3
"""Cost of rsik_clearance on the sample-major joints of a sweep (right arm: n / 16 reachable poses at 16 fractions of the interval, the
sweep itself not timed), against S spheres with and without 8 capsules, three forms:
  (a) clearance only (the mask of INTEGRATION.md): 56 B read, 8 B written per row;
  (b) clearance, nearest and gradient (what a null-space bias needs): 56 B read, 8 + 8 + 56 B written per row;
  (c) all five outputs: 56 B read, 8 + 8 + 56 + 48 + 96 B written per row;
against what a caller composed for the same rows before it:
  (d) the sweep's own elbow output, the wrist with torch from the joints (the chain's first four joints on the arm's constant block),
      the goal origin from rsik_forward_kinematics, and broadcast [rows, links, spheres] distances in torch, reduced to the minimum;
      the capsules likewise with the closest-point formula for two segments.  In chunks of --chunk-rows rows, so that the broadcast fits;
      it answers the clearance only.
HIP events on the stream, the forms interleaved in rounds in one process, medians and the spread of the rounds.  Prints one JSON line.

    python scripts/clearance_cost.py [--sizes 1048576 4194304] [--spheres 64 1024] [--launches 3] [--rounds 7]
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
from reachy2_symbolic_ik_amd import constants as K  # noqa: E402

RADIUS = (0.05, 0.04, 0.03)
OUT_BYTES = {"clearance": 8, "clearance_nearest_gradient": 8 + 8 + 56, "all": 8 + 8 + 56 + 48 + 96}


def time_launch(launch, k):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(k):
        launch()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / k  # us per call of `launch`


def scene(n_spheres, n_capsules, dev):
    """Obstacles in front of the right shoulder, radii 0.01 ... 0.08."""
    rng = np.random.default_rng(21)
    centre = lambda k: rng.uniform(-0.5, 0.5, size=(k, 3)) + [0.3, -0.2, -0.2]  # noqa: E731
    a = centre(n_capsules)
    sp = np.concatenate([centre(n_spheres), rng.uniform(0.01, 0.08, size=(n_spheres, 1))], axis=1)
    cp = np.concatenate([a, a + rng.uniform(-0.2, 0.2, size=(n_capsules, 3)), rng.uniform(0.01, 0.08, size=(n_capsules, 1))], axis=1)
    return torch.as_tensor(sp).to(dev), (torch.as_tensor(cp).to(dev) if n_capsules else None)


def composed_form(sv, consts, joints, elbow, spheres, capsules, chunk):
    """Form (d) as a callable on joints [K,m,7] and the sweep's elbow [K,m,3]: the clearance [K,m]."""
    dev = joints.device
    b = torch.as_tensor(np.asarray(consts, dtype=np.float64)).to(dev)
    sh, u, f = b[K.C_SHOULDER:K.C_SHOULDER + 3], b[K.C_UPPER_ARM], b[K.C_FOREARM]
    Ms = b[K.C_MST:K.C_MST + 9].reshape(3, 3).t()
    rad = torch.tensor(RADIUS, dtype=torch.float64, device=dev)
    q = joints.reshape(-1, 7)
    el = elbow.reshape(-1, 3)
    out = torch.empty(q.shape[0], dtype=torch.float64, device=dev)

    def seg_point(P0, e, C):
        s = (((C[None, None] - P0[:, :, None]) * e[:, :, None]).sum(-1) / (e * e).sum(-1)[:, :, None]).clamp(0.0, 1.0)
        return (P0[:, :, None] + s[..., None] * e[:, :, None] - C[None, None]).norm(dim=-1)  # [rows, 3, S]

    def seg_seg(P0, e, Q0, g):
        """Closest points of two segments (the clamped solution of the 2 x 2 system, then each parameter re-solved for the other)."""
        r = P0[:, :, None] - Q0[None, None]
        a, c = (e * e).sum(-1)[:, :, None], (g * g).sum(-1)[None, None]
        bb, er, gr = (e[:, :, None] * g[None, None]).sum(-1), (e[:, :, None] * r).sum(-1), (g[None, None] * r).sum(-1)
        den = a * c - bb * bb
        s = torch.where(den > 1e-14 * a * c, (bb * gr - c * er) / den.clamp_min(1e-300), torch.zeros_like(den)).clamp(0.0, 1.0)
        t = torch.where(c > 0, (bb * s + gr) / c.clamp_min(1e-300), torch.zeros_like(den)).clamp(0.0, 1.0)
        s = ((bb * t - er) / a).clamp(0.0, 1.0)
        t = torch.where(c > 0, (bb * s + gr) / c.clamp_min(1e-300), torch.zeros_like(den)).clamp(0.0, 1.0)
        return (r + s[..., None] * e[:, :, None] - t[..., None] * g[None, None]).norm(dim=-1)  # [rows, 3, Cp]

    def run():
        for lo in range(0, q.shape[0], chunk):
            j = q[lo:lo + chunk]
            c0, s0, c1, s1, c2, s2, c3, s3 = (fn(j[:, k]) for k in range(4) for fn in (torch.cos, torch.sin))
            zero = torch.zeros_like(c0)
            Gt = torch.stack([c0 * c1, -c0 * s1, s0, s1, c1, zero, -s0 * c1, s0 * s1, c0], dim=1).reshape(-1, 3, 3)
            MG = Ms @ Gt
            H0 = torch.stack([c3, -s2 * s3, -c2 * s3], dim=1)
            wrist = el[lo:lo + chunk] + f * (MG @ H0[..., None])[..., 0]
            tip, _ = sv.forward_kinematics(j.contiguous())
            P = torch.stack([sh.expand_as(wrist), el[lo:lo + chunk], wrist, tip], dim=1)  # [rows, 4, 3]
            P0, e = P[:, :3], P[:, 1:] - P[:, :3]
            best = (seg_point(P0, e, spheres[:, :3]) - rad[None, :, None] - spheres[None, None, :, 3]).amin(dim=(1, 2))
            if capsules is not None:
                d = seg_seg(P0, e, capsules[:, :3], capsules[:, 3:6] - capsules[:, :3]) - rad[None, :, None] - capsules[None, None, :, 6]
                best = torch.minimum(best, d.amin(dim=(1, 2)))
            out[lo:lo + chunk] = best
        return out.reshape(joints.shape[:-1])

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1048576, 4194304])
    ap.add_argument("--spheres", type=int, nargs="*", default=[64, 1024])
    ap.add_argument("--capsules", type=int, nargs="*", default=[0, 8])
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--chunk-rows", type=int, default=65536)
    ap.add_argument("--composed-max-pairs", type=float, default=5e9, help="rows x spheres above which form (d) is not timed")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        ik = SymbolicIK("r_arm", device=0)
    ik._upload()
    sv = ik.solver
    out = {}
    for n in args.sizes:
        m = max(n // 16, 1)
        rng = np.random.default_rng(12)
        pose = np.concatenate([np.array([[0.30], [-0.2], [-0.25]]) + rng.uniform(-0.08, 0.08, size=(3, m)),
                               np.array([[0.0], [-np.pi / 2], [0.0]]) + rng.uniform(-0.4, 0.4, size=(3, m))])
        sw = sv.solve_sweep(torch.as_tensor(np.ascontiguousarray(pose)).to(dev), torch.linspace(0.0, 1.0, 16, dtype=torch.float64), want_elbow=True)
        q = sw["joints"]
        for n_s in args.spheres:
            for n_c in args.capsules:
                sp, cp = scene(n_s, n_c, dev)
                wants = {"clearance": ("clearance",), "clearance_nearest_gradient": ("clearance", "nearest", "gradient"),
                         "all": sv.CLEARANCE_OUTPUTS}
                plans = {k: sv.clearance(q, sp, cp, RADIUS, want=w, plan_only=True) for k, w in wants.items()}
                forms = {k: p["launch"] for k, p in plans.items()}
                if 16 * m * n_s <= args.composed_max_pairs:
                    chunk = max(1024, min(args.chunk_rows, int(2e8 // (3 * max(n_s, 8 * n_c, 1)))))
                    forms["composed"] = composed_form(sv, ik.consts, q, sw["elbow"], sp, cp, chunk)
                for f in forms.values():  # warm-up, settled clock
                    for _ in range(2):
                        f()
                torch.cuda.synchronize()
                res = {"rows": 16 * m, "reachable_share": round(float(sw["reachable"].double().mean()), 4)}
                if "composed" in forms:  # the forms must agree on the rows that are numbers
                    a, b = plans["clearance"]["clearance"], forms["composed"]()
                    ok = torch.isfinite(a)
                    res["composed_max_diff"] = float((a[ok] - b[ok]).abs().max())
                    assert res["composed_max_diff"] < 1e-9 and bool(torch.isnan(b[~ok]).all()), res
                assert torch.equal(torch.nan_to_num(plans["all"]["clearance"]), torch.nan_to_num(plans["clearance"]["clearance"]))
                t = {k: [] for k in forms}
                for _ in range(args.rounds):
                    for k, f in forms.items():
                        t[k].append(time_launch(f, args.launches if k != "composed" else 1))
                med = {k: float(np.median(v)) for k, v in t.items()}
                for k, v in t.items():
                    res[f"{k}_us"] = round(med[k], 1)
                    res[f"{k}_us_min_max"] = [round(float(np.min(v)), 1), round(float(np.max(v)), 1)]
                for k in wants:
                    res[f"{k}_GB_per_s"] = round(16 * m * (56 + OUT_BYTES[k]) / (med[k] * 1e-6) / 1e9, 1)
                    res[f"{k}_pairs_per_s"] = float(f"{16 * m * 3 * (n_s + n_c) / (med[k] * 1e-6):.4g}")
                if "composed" in med:
                    res["clearance_over_composed"] = round(med["clearance"] / med["composed"], 5)
                out[f"{n}x{n_s}s{n_c}c"] = res
                del plans, forms, sp, cp
                torch.cuda.empty_cache()
        del sw, q
        torch.cuda.empty_cache()
    out["launches_per_median"] = args.launches * args.rounds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
