"""Device-side driver: owns one rsik context per GPU and hands torch-owned HBM buffers to the C ABI.

PyTorch is used for device memory, streams and torch.distributed only; all arithmetic happens in
the hand-written HIP kernels behind include/rsik.h.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Optional, Sequence

import numpy as np
import torch

from . import _abi
from .constants import ARM_CONSTS_COUNT

_F64 = torch.float64
_U8 = torch.uint8


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


class ContinuousRunResult(dict):
    """What control_continuous_run returns: the dict of output tensors (joints, reachable, state) with one attribute beside it,
    `run_form` = how the library issued the run (_abi.CONT_FORM_*; `run_form_name` in words)."""

    run_form: int = _abi.CONT_FORM_NONE

    @property
    def run_form_name(self) -> str:
        return _abi.CONT_FORM_NAMES.get(self.run_form, str(self.run_form))


class HipSolver:
    """One context = one GPU.  Methods enqueue on torch's current stream and return torch tensors."""

    def __init__(self, device: int | torch.device | None = None) -> None:
        self.lib = _abi.load()
        if self.lib.rsik_device_count() <= 0 or not torch.cuda.is_available():
            raise RuntimeError(
                "reachy2_symbolic_ik_amd: no MI355X/HIP device visible — this package has no CPU fallback"
            )
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", index)
        h = C.c_void_p()
        rc = self.lib.rsik_create(index, C.byref(h))
        if rc != _abi.RSIK_OK:
            raise _abi.RsikError(rc, (self.lib.rsik_last_error(None) or b"").decode())
        self._h = h
        self._arms_set = [False, False]
        self._arm_blocks = [None, None]
        self._arm_gen = 0  # bumped whenever an arm's constants really change: plans made before are then stale

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.lib.rsik_destroy(self._h)
            self._h = None

    def __del__(self) -> None:  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        if rc != _abi.RSIK_OK:
            raise _abi.RsikError(rc, (self.lib.rsik_last_error(self._h) or b"").decode())

    def _bind_stream(self) -> None:
        s = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self.lib.rsik_set_stream(self._h, C.c_void_p(s)))

    def _call(self, fn_name: str, *cargs) -> None:
        """One C-ABI call of this context on its device and torch's current stream, checked."""
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(getattr(self.lib, fn_name)(self._h, *cargs))

    def _finish(self, res: Dict[str, Any], fn_name: str, cargs: tuple, plan_only: bool, keepalive: tuple) -> Dict[str, Any]:
        """Launches, or (plan_only) adds res["launch"] (see plan()) and what the planned launch points into."""
        if plan_only:
            res["launch"] = self.plan(fn_name, *cargs)
            res["_keepalive"] = keepalive
        else:
            self._call(fn_name, *cargs)
        return res

    @staticmethod
    def _cols(t: torch.Tensor, rows: int):
        """The ABI's column table of an SoA tensor [rows, n]: one pointer per row."""
        return (C.c_void_p * rows)(*[t[k].data_ptr() for k in range(rows)])

    @staticmethod
    def _pair(v: Sequence[float], name: str):
        """A per-arm launch constant: 2 float64 values (r, l), and the pointer the ABI takes."""
        pts = np.ascontiguousarray(v, dtype=np.float64)
        if pts.shape != (2,):
            raise ValueError(f"{name} must have 2 entries (r, l)")
        return pts, pts.ctypes.data_as(C.POINTER(C.c_double))

    def set_arm(self, arm_id: int, consts: np.ndarray) -> None:
        c = np.ascontiguousarray(consts, dtype=np.float64)
        if c.shape != (ARM_CONSTS_COUNT,):
            raise ValueError(f"expected {ARM_CONSTS_COUNT} constants, got {c.shape}")
        old = self._arm_blocks[arm_id]
        if old is not None and old.tobytes() == c.tobytes():
            return
        self._check(self.lib.rsik_set_arm(self._h, int(arm_id), c.ctypes.data_as(C.POINTER(C.c_double)), c.size))
        self._arms_set[arm_id] = True
        self._arm_blocks[arm_id] = c.copy()
        self._arm_gen += 1

    def synchronize(self) -> None:
        """Waits for the work on the CURRENT torch stream of this device (the stream every non-planned call uses)."""
        self._call("rsik_sync")  # (binds the stream first: a planned launch may have left the context on another, possibly destroyed, one)

    def control_continuous_reserve(self, n: int, n_steps: int) -> None:
        """rsik_control_continuous_reserve: workspace, side streams and events of a control_continuous_run(n, n_steps), so
        that the run allocates nothing — needed before such a run is captured into a hipGraph on a fresh context."""
        self._call("rsik_control_continuous_reserve", int(n), int(n_steps))

    def control_continuous_release(self) -> None:
        """rsik_control_continuous_release: waits for the device and frees the workspace(s) continuous runs keep in the context
        (hipGraphs captured from such runs must not be replayed afterwards)."""
        with torch.cuda.device(self.device):
            self._check(self.lib.rsik_control_continuous_release(self._h))

    # ------------------------------------------------------------------ checks
    def _dev_f64(self, t: torch.Tensor, shape: Sequence[int], name: str) -> torch.Tensor:
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t, dtype=np.float64))
        t = t.to(device=self.device, dtype=_F64)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t.contiguous()

    def _dev_cols(self, t: torch.Tensor, rows: int, n: int, name: str) -> torch.Tensor:
        """SoA input [rows, n]: the ABI takes one pointer per column array, so any view whose rows are unit-stride
        (e.g. a column slice columns[:, lo:hi] of a larger batch) is passed as it is, without a copy."""
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t, dtype=np.float64))
        t = t.to(device=self.device, dtype=_F64)
        if tuple(t.shape) != (rows, n):
            raise ValueError(f"{name}: expected shape {(rows, n)}, got {tuple(t.shape)}")
        if n > 1 and t.stride(1) != 1:
            t = t.contiguous()
        return t

    def _dev_u8(self, t, n: int, name: str) -> torch.Tensor:
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t, dtype=np.uint8))
        t = t.to(device=self.device, dtype=_U8)
        if tuple(t.shape) != (n,):
            raise ValueError(f"{name}: expected shape ({n},), got {tuple(t.shape)}")
        return t.contiguous()

    def _out_buf(self, out: Optional[Dict[str, torch.Tensor]], name: str, shape: Sequence[int], dtype: torch.dtype) -> torch.Tensor:
        """The caller's `out[name]` if given — it must be exactly what the kernel writes (this device, dtype, shape,
        contiguous: the kernels get a raw pointer) — else a fresh buffer."""
        t = None if out is None else out.get(name, None)
        shape = tuple(int(v) for v in shape)
        if t is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"out[{name!r}] must be a torch tensor")
        if t.device != self.device or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor of shape {shape} on {self.device}; got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}{'' if t.is_contiguous() else ' (not contiguous)'}")
        return t

    def _arm_ids(self, arm, n: int) -> Optional[torch.Tensor]:
        """The optional per-row arm ids [n] u8 of every entry point (None: the launch's arm_uniform holds)."""
        return None if arm is None else self._dev_u8(arm, n, "arm")

    # what solve_sweep, solve_nearest and solve_path share: the policy, the theta grid, the weights, the per-pose outputs
    @staticmethod
    def _policy_code(policy: str) -> int:
        codes = {"fraction": _abi.THETA_FRACTION, "explicit": _abi.THETA_EXPLICIT}
        if policy not in codes:
            raise ValueError("policy must be 'fraction' or 'explicit'")
        return codes[policy]

    def _theta_grid(self, thetas, pose_shape: Sequence[int], pose_dims: str, k_max: int, per: str):
        """thetas [K], shared, or [K, *pose_shape], one column per pose (`pose_dims`: that shape in words) -> (device tensor, K,
        per_pose); K is 1 ... k_max samples per `per`."""
        if not isinstance(thetas, torch.Tensor):
            thetas = torch.as_tensor(np.asarray(thetas, dtype=np.float64))
        if thetas.dim() not in (1, 1 + len(pose_shape)):
            raise ValueError(f"thetas must have shape [K] or [K, {pose_dims}]")
        k = int(thetas.shape[0])
        per_pose = thetas.dim() != 1
        if not 1 <= k <= k_max:
            raise ValueError(f"thetas: between 1 and {k_max} samples per {per}")
        return self._dev_f64(thetas, (k, *pose_shape) if per_pose else (k,), "thetas"), k, per_pose

    @staticmethod
    def _weights7(weights: Optional[Sequence[float]]):
        """The 7 joint weights (None: the library's ones) -> (array to keep alive, the pointer the ABI takes)."""
        if weights is None:
            return None, None
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (7,):
            raise ValueError("weights must have 7 entries")
        return w, w.ctypes.data_as(C.POINTER(C.c_double))

    def _reach_outs(self, res: Dict[str, torch.Tensor], out: Optional[Dict[str, torch.Tensor]], lead: Sequence[int]) -> None:
        """The tail of a sampling result: is_reachable's interval, reachable and state for poses of shape `lead`."""
        res["interval"] = self._out_buf(out, "interval", (*lead, 2), _F64)
        res["reachable"] = self._out_buf(out, "reachable", lead, _U8)
        res["state"] = self._out_buf(out, "state", lead, _U8)

    # ------------------------------------------------------------------ rsik_solve
    def solve(
        self,
        pose_soa: torch.Tensor,
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        theta_policy: int = _abi.THETA_INTERVAL0,
        theta_in: Optional[torch.Tensor] = None,
        previous_joints: Optional[Sequence[float]] = None,
        want_elbow: bool = True,
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
        previous_joints_rows: Optional[torch.Tensor] = None,
    ) -> Dict[str, torch.Tensor]:
        """pose_soa: [6, n] float64 (rows px,py,pz,roll,pitch,yaw).  Returns joints [n,7], interval [n,2],
        elbow [n,3], reachable [n] u8, state [n] u8 (device tensors, asynchronous on the current stream).
        previous_joints: 7 values for every pose (rsik_solve); previous_joints_rows: [n,7], one row per pose
        (rsik_solve_rows: n independent callers in one launch).  Not both.
        plan_only=True launches nothing and adds res["launch"], a zero-overhead re-launch callable (see plan())."""
        if pose_soa.dim() != 2 or pose_soa.shape[0] != 6:
            raise ValueError("pose_soa must have shape [6, n]")
        n = int(pose_soa.shape[1])
        pose_soa = self._dev_cols(pose_soa, 6, n, "pose_soa")
        arm = self._arm_ids(arm, n)
        if theta_policy in (_abi.THETA_EXPLICIT, _abi.THETA_FRACTION):
            if theta_in is None:
                raise ValueError("theta_in is required for this theta policy")
            theta_in = self._dev_f64(theta_in, (n,), "theta_in")
        else:
            theta_in = None
        none = theta_policy == _abi.THETA_NONE
        joints = None if none else self._out_buf(out, "joints", (n, 7), _F64)
        elbow = self._out_buf(out, "elbow", (n, 3), _F64) if (not none and want_elbow) else None
        interval = self._out_buf(out, "interval", (n, 2), _F64)
        reachable = self._out_buf(out, "reachable", (n,), _U8)
        state = self._out_buf(out, "state", (n,), _U8)
        cols = self._cols(pose_soa, 6)
        prev = None
        fn_name = "rsik_solve"
        if previous_joints_rows is not None:
            if previous_joints is not None:
                raise ValueError("previous_joints and previous_joints_rows cannot be combined")
            previous_joints_rows = self._dev_f64(previous_joints_rows, (n, 7), "previous_joints_rows")
            prev = _ptr(previous_joints_rows)
            fn_name = "rsik_solve_rows"
        elif previous_joints is not None:
            pj = np.ascontiguousarray(previous_joints, dtype=np.float64)
            if pj.shape != (7,):
                raise ValueError("previous_joints must have 7 entries")
            prev = pj.ctypes.data_as(C.POINTER(C.c_double))
        cargs = (n, cols, _ptr(arm), int(arm_uniform), int(theta_policy), _ptr(theta_in), prev,
                 _ptr(joints), _ptr(interval), _ptr(elbow), _ptr(reachable), _ptr(state))
        res = {"interval": interval, "reachable": reachable, "state": state}
        self._finish(res, fn_name, cargs, plan_only, (pose_soa, arm, theta_in, cols, prev, previous_joints_rows))
        if joints is not None:
            res["joints"] = joints
        if elbow is not None:
            res["elbow"] = elbow
        return res

    # ------------------------------------------------------------------ rsik_solve_sweep
    def solve_sweep(
        self,
        pose_soa: torch.Tensor,
        thetas: torch.Tensor,
        policy: str = "fraction",
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        previous_joints: Optional[torch.Tensor] = None,
        want_elbow: bool = True,
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """K elbow angles per pose from one launch (rsik_solve_sweep): is_reachable once per pose, then get_joints at every
        sample, each sample bit for bit what solve() returns for that theta — independent of the other samples and their order.
        pose_soa: [6, n] float64.  thetas: 1-D [K], shared by every pose, or 2-D [K, n], one column per pose; `policy`
        "fraction" (of the pose's interval, 0 ... 1 from interval[0] to interval[1]) or "explicit" (angles).
        previous_joints: [n, 7] or None for zeros, one row per pose.
        Returns device tensors, sample-major: joints [K, n, 7], elbow [K, n, 3] (want_elbow), projected [K, n] u8 (1 where the
        elbow projection moved the goal for that sample), theta [K, n] (the angle evaluated), and interval [n, 2],
        reachable [n] u8, state [n] u8 as solve().  Sample k is the contiguous array joints[k];
        joints.permute(1, 0, 2) is the per-pose view [n, K, 7].
        plan_only=True launches nothing and adds res["launch"], a zero-overhead re-launch callable (see plan())."""
        if pose_soa.dim() != 2 or pose_soa.shape[0] != 6:
            raise ValueError("pose_soa must have shape [6, n]")
        code = self._policy_code(policy)
        n = int(pose_soa.shape[1])
        pose_soa = self._dev_cols(pose_soa, 6, n, "pose_soa")
        thetas, k, per_pose = self._theta_grid(thetas, (n,), "n", 4096, "pose")
        arm = self._arm_ids(arm, n)
        if previous_joints is not None:
            previous_joints = self._dev_f64(previous_joints, (n, 7), "previous_joints")
        res = {"joints": self._out_buf(out, "joints", (k, n, 7), _F64)}
        if want_elbow:
            res["elbow"] = self._out_buf(out, "elbow", (k, n, 3), _F64)
        res["projected"] = self._out_buf(out, "projected", (k, n), _U8)
        res["theta"] = self._out_buf(out, "theta", (k, n), _F64)
        self._reach_outs(res, out, (n,))
        cols = self._cols(pose_soa, 6)
        cargs = (n, cols, _ptr(arm), int(arm_uniform), k, code, _ptr(thetas), int(per_pose),
                 _ptr(previous_joints), _ptr(res["joints"]), _ptr(res.get("elbow")), _ptr(res["projected"]), _ptr(res["theta"]),
                 _ptr(res["interval"]), _ptr(res["reachable"]), _ptr(res["state"]))
        return self._finish(res, "rsik_solve_sweep", cargs, plan_only, (pose_soa, arm, thetas, cols, previous_joints))

    # ------------------------------------------------------------------ rsik_solve_nearest
    def solve_nearest(
        self,
        pose_soa: torch.Tensor,
        thetas: torch.Tensor,
        seed_joints: torch.Tensor,
        policy: str = "fraction",
        weights: Optional[Sequence[float]] = None,
        skip_projected: bool = False,
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        previous_joints: Optional[torch.Tensor] = None,
        want_elbow: bool = True,
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """Of K elbow angles per pose, the one whose solution is nearest to the pose's seed joints, from one launch
        (rsik_solve_nearest): solve_sweep's samples, the weighted squared angle_diff to seed_joints as the cost, the smallest cost
        wins, the lowest sample among equal costs — one row per pose comes back instead of K.
        pose_soa, thetas ([K] or [K, n]), policy, previous_joints, arm: as solve_sweep.  seed_joints: [n, 7].  weights: 7 values,
        finite and >= 0, None for ones.  skip_projected: samples whose elbow projection moved the goal are no candidates.
        Returns device tensors: index [n] int32 (the winning sample, -1 where the pose has no candidate), theta [n], joints [n,7],
        elbow [n,3] (want_elbow), projected [n] u8 — the bits of solve_sweep's sample index[i] of pose i, NaN / 0 without a
        candidate —, cost [n] (sqrt of the winner's weighted sum), and interval [n,2], reachable [n] u8, state [n] u8 as solve():
        a pose can be reachable and have index -1.
        plan_only=True launches nothing and adds res["launch"], a zero-overhead re-launch callable (see plan())."""
        if pose_soa.dim() != 2 or pose_soa.shape[0] != 6:
            raise ValueError("pose_soa must have shape [6, n]")
        code = self._policy_code(policy)
        n = int(pose_soa.shape[1])
        pose_soa = self._dev_cols(pose_soa, 6, n, "pose_soa")
        thetas, k, per_pose = self._theta_grid(thetas, (n,), "n", 4096, "pose")
        seed_joints = self._dev_f64(seed_joints, (n, 7), "seed_joints")
        arm = self._arm_ids(arm, n)
        if previous_joints is not None:
            previous_joints = self._dev_f64(previous_joints, (n, 7), "previous_joints")
        w, wp = self._weights7(weights)
        res = {"index": self._out_buf(out, "index", (n,), torch.int32), "theta": self._out_buf(out, "theta", (n,), _F64),
               "joints": self._out_buf(out, "joints", (n, 7), _F64)}
        if want_elbow:
            res["elbow"] = self._out_buf(out, "elbow", (n, 3), _F64)
        res["cost"] = self._out_buf(out, "cost", (n,), _F64)
        res["projected"] = self._out_buf(out, "projected", (n,), _U8)
        self._reach_outs(res, out, (n,))
        cols = self._cols(pose_soa, 6)
        cargs = (n, cols, _ptr(arm), int(arm_uniform), k, code, _ptr(thetas), int(per_pose), _ptr(previous_joints),
                 _ptr(seed_joints), wp, _abi.NEAREST_SKIP_PROJECTED if skip_projected else 0,
                 _ptr(res["index"]), _ptr(res["theta"]), _ptr(res["joints"]), _ptr(res.get("elbow")), _ptr(res["cost"]),
                 _ptr(res["projected"]), _ptr(res["interval"]), _ptr(res["reachable"]), _ptr(res["state"]))
        return self._finish(res, "rsik_solve_nearest", cargs, plan_only, (pose_soa, arm, thetas, cols, previous_joints, seed_joints, w))

    # ------------------------------------------------------------------ rsik_solve_path
    def solve_path_workspace_bytes(self, n: int, n_steps: int, n_theta: int) -> int:
        """rsik_solve_path_workspace_bytes: the device workspace a solve_path of this shape needs."""
        b = C.c_size_t(0)
        rc = self.lib.rsik_solve_path_workspace_bytes(int(n), int(n_steps), int(n_theta), C.byref(b))
        if rc != _abi.RSIK_OK:
            raise _abi.RsikError(rc, "rsik_solve_path_workspace_bytes: n >= 0, n_steps 1 ... 65536, n_theta 1 ... 64")
        return int(b.value)

    def solve_path(
        self,
        pose_soa: torch.Tensor,
        thetas: torch.Tensor,
        start_joints: Optional[torch.Tensor] = None,
        policy: str = "fraction",
        weights: Optional[Sequence[float]] = None,
        skip_projected: bool = False,
        unwind: bool = False,
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        want_elbow: bool = True,
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """The least-motion way through K elbow angles per waypoint, for n paths of T waypoints, from one launch (rsik_solve_path):
        solve_sweep's samples at every waypoint, the weighted squared angle_diff between consecutive waypoints' joints as the
        transition cost, and the sequence of samples with the smallest sum, found by dynamic programming on the device.
        pose_soa: [6, T, n] float64, waypoint-major.  thetas: [K], shared by every waypoint, or [K, T, n]; K <= 64; policy
        "fraction" or "explicit".  start_joints: [n, 7] or None, the joints each path starts from.  weights: 7 values, finite and
        >= 0, None for ones.  skip_projected: samples whose elbow projection moved the goal are no candidates.  unwind: joints are
        made continuous along the path (allow_multiturn against the row before), index and the costs do not change.  arm: [n], one
        byte per path.
        Returns device tensors: index [T, n] int32 (the winning sample, -1 at a waypoint without a candidate: the path skips it),
        theta [T, n], joints [T, n, 7], elbow [T, n, 3] (want_elbow), projected [T, n] u8 — the bits of solve_sweep's sample
        index[t, i] —, step_cost [T, n] (sqrt of the transition cost into the waypoint), cost [n] (the minimal sum, not its root),
        n_solved [n] int32, and interval [T, n, 2], reachable [T, n] u8, state [T, n] u8 as solve().
        The workspace is allocated here, with torch, from rsik_solve_path_workspace_bytes; a plan keeps it alive.
        plan_only=True launches nothing and adds res["launch"], a zero-overhead re-launch callable (see plan())."""
        return self._solve_path(None, pose_soa, thetas, start_joints, policy, weights, skip_projected, unwind, arm, arm_uniform,
                                want_elbow, out, plan_only)

    def _solve_path(self, scene, pose_soa, thetas, start_joints, policy, weights, skip_projected, unwind, arm, arm_uniform, want_elbow,
                    out, plan_only):
        """What solve_path() and solve_path_clear() share: the checks, the workspace, the buffers and the call.  scene: None
        (rsik_solve_path), or (tensors to keep alive, the C arguments between flags and the workspace) for rsik_solve_path_clear, which
        has three outputs more."""
        if pose_soa.dim() != 3 or pose_soa.shape[0] != 6:
            raise ValueError("pose_soa must have shape [6, T, n]")
        code = self._policy_code(policy)
        t, n = int(pose_soa.shape[1]), int(pose_soa.shape[2])
        if not 1 <= t <= 65536:
            raise ValueError("pose_soa: between 1 and 65536 waypoints per path")
        pose_soa = self._dev_cols(pose_soa.reshape(6, t * n), 6, t * n, "pose_soa")
        thetas, k, per_pose = self._theta_grid(thetas, (t, n), "T, n", 64, "waypoint")
        if start_joints is not None:
            start_joints = self._dev_f64(start_joints, (n, 7), "start_joints")
        arm = self._arm_ids(arm, n)
        w, wp = self._weights7(weights)
        ws_bytes = self.solve_path_workspace_bytes(n, t, k)
        workspace = torch.empty((max(ws_bytes, 1),), dtype=_U8, device=self.device)
        res = {"index": self._out_buf(out, "index", (t, n), torch.int32), "theta": self._out_buf(out, "theta", (t, n), _F64),
               "joints": self._out_buf(out, "joints", (t, n, 7), _F64)}
        if want_elbow:
            res["elbow"] = self._out_buf(out, "elbow", (t, n, 3), _F64)
        res["projected"] = self._out_buf(out, "projected", (t, n), _U8)
        res["step_cost"] = self._out_buf(out, "step_cost", (t, n), _F64)
        res["cost"] = self._out_buf(out, "cost", (n,), _F64)
        res["n_solved"] = self._out_buf(out, "n_solved", (n,), torch.int32)
        self._reach_outs(res, out, (t, n))
        cols = self._cols(pose_soa, 6)
        flags = (_abi.PATH_SKIP_PROJECTED if skip_projected else 0) | (_abi.PATH_UNWIND if unwind else 0)
        cargs = (n, t, cols, _ptr(arm), int(arm_uniform), k, code, _ptr(thetas), int(per_pose), _ptr(start_joints), wp, flags)
        keep, symbol = (pose_soa, arm, thetas, cols, start_joints, w, workspace), "rsik_solve_path"
        if scene is not None:
            res["clearance"] = self._out_buf(out, "clearance", (t, n), _F64)
            res["nearest"] = self._out_buf(out, "nearest", (t, n, 2), torch.int32)
            res["blocked"] = self._out_buf(out, "blocked", (t, n), _U8)
            cargs, keep, symbol = cargs + scene[1], keep + scene[0], "rsik_solve_path_clear"
        cargs += (_ptr(workspace), ws_bytes,
                  _ptr(res["index"]), _ptr(res["theta"]), _ptr(res["joints"]), _ptr(res.get("elbow")), _ptr(res["projected"]),
                  _ptr(res["step_cost"]), _ptr(res["cost"]), _ptr(res["n_solved"]),
                  _ptr(res["interval"]), _ptr(res["reachable"]), _ptr(res["state"]))
        if scene is not None:
            cargs += (_ptr(res["clearance"]), _ptr(res["nearest"]), _ptr(res["blocked"]))
        # (the workspace: torch allocated it on the launch's stream and hands it out again in stream order; a plan keeps it)
        return self._finish(res, symbol, cargs, plan_only, keep)

    def _path_scene(self, spheres, capsules, link_radius, need_obstacle: bool):
        """The static scene of solve_path_clear() and solve_path_pair(): (tensors to keep alive, the C arguments link_radius_host,
        n_spheres, spheres, n_capsules, capsules).  need_obstacle: solve_path_clear() refuses a call without one."""

        def rows(t, width, most, message):
            if t is None:
                return None, 0
            if not isinstance(t, torch.Tensor):
                t = torch.as_tensor(np.asarray(t, dtype=np.float64))
            if t.dim() != 2 or t.shape[1] != width or t.shape[0] > most:
                raise ValueError(message)
            count = int(t.shape[0])
            return (self._dev_f64(t, (count, width), message.split()[0]) if count else None), count

        spheres, n_spheres = rows(spheres, 4, self.TRACK_AVOID_MAX_SPHERES, "spheres must have shape [S, 4] with S <= 256")
        capsules, n_capsules = rows(capsules, 7, self.TRACK_AVOID_MAX_CAPSULES, "capsules must have shape [C, 7] with C <= 64")
        if need_obstacle and n_spheres + n_capsules < 1:
            raise ValueError("at least one obstacle: spheres [S, 4] or capsules [C, 7] (without obstacles: solve_path())")
        rad, rad_p = None, None
        if link_radius is not None:
            rad = np.ascontiguousarray(link_radius.cpu().numpy() if isinstance(link_radius, torch.Tensor) else link_radius, dtype=np.float64)
            if rad.shape != (3,):
                raise ValueError("link_radius must have 3 entries")
            rad_p = rad.ctypes.data_as(C.POINTER(C.c_double))
        return (spheres, capsules, rad), (rad_p, n_spheres, _ptr(spheres), n_capsules, _ptr(capsules))

    # ------------------------------------------------------------------ rsik_solve_path_clear
    def solve_path_clear(
        self,
        pose_soa: torch.Tensor,
        thetas: torch.Tensor,
        start_joints: Optional[torch.Tensor] = None,
        *,
        spheres: Optional[torch.Tensor] = None,
        capsules: Optional[torch.Tensor] = None,
        link_radius: Any = None,
        min_clearance: float = -float("inf"),
        influence: float = 0.0,
        clearance_gain: float = 0.0,
        policy: str = "fraction",
        weights: Optional[Sequence[float]] = None,
        skip_projected: bool = False,
        unwind: bool = False,
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        want_elbow: bool = True,
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """solve_path() among obstacles, from one launch (rsik_solve_path_clear): the least-motion way through the samples that keep
        the arm at least min_clearance away from a static scene.  Every argument of solve_path() means what it means there;
        spheres [S, 4], capsules [C, 7] and link_radius are track_avoid()'s (S <= 256, C <= 64, at least one obstacle, shared by
        every path, waypoint and sample).
        d of a sample is clearance()'s `clearance` of its joints.  A sample with d < min_clearance (m; -inf: no constraint) is no
        candidate; a waypoint left without one is skipped, index -1.  A sample with d < influence (m) adds
        clearance_gain (influence - d)^2 (rad^2 per m^2) to the cost of every path through it; cost includes these penalties,
        step_cost does not.  With min_clearance = -inf and clearance_gain = 0 the result is solve_path()'s, bit for bit.
        Returns solve_path()'s dict and clearance [T, n], nearest [T, n, 2] int32 (link, obstacle index) — clearance()'s bits for
        the returned joints (without unwind); NaN and (-1, -1) at a skipped waypoint — and blocked [T, n] u8: how many of the K
        samples solve_path() would have taken as candidates fail d >= min_clearance.
        The workspace is handled as in solve_path(); a plan keeps it and the obstacle tensors alive.
        plan_only=True launches nothing and adds res["launch"], a zero-overhead re-launch callable (see plan())."""

        keep, scene_args = self._path_scene(spheres, capsules, link_radius, True)
        scene = (keep, scene_args + (float(min_clearance), float(influence), float(clearance_gain)))
        return self._solve_path(scene, pose_soa, thetas, start_joints, policy, weights, skip_projected, unwind, arm, arm_uniform,
                                want_elbow, out, plan_only)

    # ------------------------------------------------------------------ rsik_solve_path_pair
    PATH_PAIR_MAX_THETA = 16

    def solve_path_pair_workspace_bytes(self, n_pairs: int, n_steps: int, n_theta: int) -> int:
        """rsik_solve_path_pair_workspace_bytes: the device workspace a solve_path_pair of this shape needs."""
        b = C.c_size_t(0)
        rc = self.lib.rsik_solve_path_pair_workspace_bytes(int(n_pairs), int(n_steps), int(n_theta), C.byref(b))
        if rc != _abi.RSIK_OK:
            raise _abi.RsikError(rc, "rsik_solve_path_pair_workspace_bytes: n_pairs >= 0, n_steps 1 ... 65536, n_theta 1 ... 16")
        return int(b.value)

    def solve_path_pair(
        self,
        pose_soa: torch.Tensor,
        thetas: torch.Tensor,
        start_joints: Optional[torch.Tensor] = None,
        *,
        spheres: Optional[torch.Tensor] = None,
        capsules: Optional[torch.Tensor] = None,
        link_radius: Any = None,
        min_clearance: float = -float("inf"),
        influence: float = 0.0,
        clearance_gain: float = 0.0,
        policy: str = "fraction",
        weights: Optional[Sequence[float]] = None,
        skip_projected: bool = False,
        unwind: bool = False,
        want_elbow: bool = True,
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """solve_path_clear() for robots of two arms that keep out of each other, from one launch (rsik_solve_path_pair): the
        elbow angles of both arms chosen together, a state being a pair of samples (a of the right arm, b of the left).
        pose_soa: [6, T, n] with n = 2 n_pairs rows, row 2 i the right arm of robot i and row 2 i + 1 its left arm (track_pair()'s
        rows; there is no arm argument).  thetas: [K] or [K, T, n], K <= 16.  start_joints: [n, 7] or None.  spheres [S, 4],
        capsules [C, 7] (both may be missing: the partner is always an obstacle), link_radius and every other keyword as in
        solve_path_clear().
        A pair whose right arm's clearance() to the static scene and the left arm's three links, or the left arm's to the scene and
        the right arm's links, is below min_clearance is no candidate; a waypoint without a candidate pair is skipped for both arms.
        Each view nearer than influence adds clearance_gain (influence - d)^2 to the cost.
        Returns solve_path_clear()'s dict with index, theta, joints ... [T, n, ...] per row, clearance [T, n] and nearest [T, n, 2]
        int32 (link, obstacle index: S + C + l is the partner's link l) per view, and per robot cost [n_pairs], n_solved [n_pairs]
        int32 and blocked [T, n_pairs] int16 (the count of a uint16: pairs of row candidates that are no candidate pair).
        plan_only=True launches nothing and adds res["launch"], a zero-overhead re-launch callable (see plan())."""
        if pose_soa.dim() != 3 or pose_soa.shape[0] != 6:
            raise ValueError("pose_soa must have shape [6, T, n]")
        code = self._policy_code(policy)
        t, n = int(pose_soa.shape[1]), int(pose_soa.shape[2])
        if n % 2:
            raise ValueError("pose_soa: an even number of rows, row 2 i the right arm of robot i and row 2 i + 1 its left arm")
        if not 1 <= t <= 65536:
            raise ValueError("pose_soa: between 1 and 65536 waypoints per path")
        n_pairs = n // 2
        pose_soa = self._dev_cols(pose_soa.reshape(6, t * n), 6, t * n, "pose_soa")
        thetas, k, per_pose = self._theta_grid(thetas, (t, n), "T, n", self.PATH_PAIR_MAX_THETA, "waypoint")
        if start_joints is not None:
            start_joints = self._dev_f64(start_joints, (n, 7), "start_joints")
        scene_keep, scene_args = self._path_scene(spheres, capsules, link_radius, False)
        w, wp = self._weights7(weights)
        ws_bytes = self.solve_path_pair_workspace_bytes(n_pairs, t, k)
        workspace = torch.empty((max(ws_bytes, 1),), dtype=_U8, device=self.device)
        res = {"index": self._out_buf(out, "index", (t, n), torch.int32), "theta": self._out_buf(out, "theta", (t, n), _F64),
               "joints": self._out_buf(out, "joints", (t, n, 7), _F64)}
        if want_elbow:
            res["elbow"] = self._out_buf(out, "elbow", (t, n, 3), _F64)
        res["projected"] = self._out_buf(out, "projected", (t, n), _U8)
        res["step_cost"] = self._out_buf(out, "step_cost", (t, n), _F64)
        res["cost"] = self._out_buf(out, "cost", (n_pairs,), _F64)
        res["n_solved"] = self._out_buf(out, "n_solved", (n_pairs,), torch.int32)
        self._reach_outs(res, out, (t, n))
        res["clearance"] = self._out_buf(out, "clearance", (t, n), _F64)
        res["nearest"] = self._out_buf(out, "nearest", (t, n, 2), torch.int32)
        res["blocked"] = self._out_buf(out, "blocked", (t, n_pairs), torch.int16)
        cols = self._cols(pose_soa, 6)
        flags = (_abi.PATH_SKIP_PROJECTED if skip_projected else 0) | (_abi.PATH_UNWIND if unwind else 0)
        cargs = (n_pairs, t, cols, k, code, _ptr(thetas), int(per_pose), _ptr(start_joints), wp, flags,
                 *scene_args, float(min_clearance), float(influence), float(clearance_gain), _ptr(workspace), ws_bytes,
                 _ptr(res["index"]), _ptr(res["theta"]), _ptr(res["joints"]), _ptr(res.get("elbow")), _ptr(res["projected"]),
                 _ptr(res["step_cost"]), _ptr(res["cost"]), _ptr(res["n_solved"]),
                 _ptr(res["interval"]), _ptr(res["reachable"]), _ptr(res["state"]),
                 _ptr(res["clearance"]), _ptr(res["nearest"]), _ptr(res["blocked"]))
        return self._finish(res, "rsik_solve_path_pair", cargs, plan_only,
                            (pose_soa, thetas, cols, start_joints, w, workspace) + scene_keep)

    # ------------------------------------------------------------------ rsik_reach_map
    REACH_MAP_OUTPUTS = ("count", "state_count", "theta_measure", "mask")

    def reach_map(
        self,
        pos_soa: torch.Tensor,
        euler_soa: torch.Tensor,
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        want: Sequence[str] = REACH_MAP_OUTPUTS,
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """A reachability map from one launch (rsik_reach_map): every position of pos_soa [3, n_pos] with every orientation of
        euler_soa [3, n_rot] (rows roll, pitch, yaw; 1 ... 4096 of them), reduced per position on the device.  Pose (i, j) is judged
        bit for bit as solve() judges it under THETA_NONE with arm byte arm[i] (`arm`: [n_pos] u8, one per POSITION, or None
        with arm_uniform).
        `want`: which of the four outputs to compute, at least one.  Returns device tensors, one row per position:
        count [n_pos] int32 (reachable orientations), state_count [n_pos, 11] int32 (orientations per state code),
        theta_measure [n_pos] float64 (summed interval width of the reachable ones, 0.0 where there is none),
        mask [n_pos, ceil(n_rot / 64)] int64 (the words' bits: bit j % 64 of word j // 64 is pose (i, j)'s flag; see
        unpack_reach_mask).  The parallelism comes from the positions: few positions with many orientations are correct, not fast.
        plan_only=True launches nothing and adds res["launch"], a zero-overhead re-launch callable (see plan())."""
        if pos_soa.dim() != 2 or pos_soa.shape[0] != 3:
            raise ValueError("pos_soa must have shape [3, n_pos]")
        if euler_soa.dim() != 2 or euler_soa.shape[0] != 3:
            raise ValueError("euler_soa must have shape [3, n_rot]")
        n_pos, n_rot = int(pos_soa.shape[1]), int(euler_soa.shape[1])
        if not 1 <= n_rot <= 4096:
            raise ValueError("euler_soa: between 1 and 4096 orientations")
        want = tuple(want)
        if not want or any(name not in self.REACH_MAP_OUTPUTS for name in want):
            raise ValueError(f"want must name at least one of {self.REACH_MAP_OUTPUTS}")
        pos_soa = self._dev_cols(pos_soa, 3, n_pos, "pos_soa")
        euler_soa = self._dev_cols(euler_soa, 3, n_rot, "euler_soa")
        arm = self._arm_ids(arm, n_pos)
        shapes = {"count": ((n_pos,), torch.int32), "state_count": ((n_pos, 11), torch.int32),
                  "theta_measure": ((n_pos,), _F64), "mask": ((n_pos, (n_rot + 63) // 64), torch.int64)}
        res = {name: self._out_buf(out, name, *shapes[name]) for name in self.REACH_MAP_OUTPUTS if name in want}
        pcols, ecols = self._cols(pos_soa, 3), self._cols(euler_soa, 3)
        cargs = (n_pos, pcols, _ptr(arm), int(arm_uniform), n_rot, ecols,
                 _ptr(res.get("count")), _ptr(res.get("state_count")), _ptr(res.get("theta_measure")), _ptr(res.get("mask")))
        return self._finish(res, "rsik_reach_map", cargs, plan_only, (pos_soa, euler_soa, arm, pcols, ecols))

    def plan(self, fn_name: str, *args):
        """Binds one C-ABI call with all its arguments once; the returned callable re-issues exactly that launch (a few
        microseconds of host time per call — the hot loop of a caller that re-solves resident buffers, e.g. bench.py).
        `launch()` enqueues on the stream that was current at PLANNING time, whatever other calls have done to the
        context's stream since; `launch(stream=handle)` enqueues on another hipStream_t (a capture stream when the
        launches are recorded into a hipGraph).  The plan is tied to the arm constants uploaded at planning time: it
        raises if set_arm() has changed them since.  Keep the tensors alive while the plan is used."""
        fn = getattr(self.lib, fn_name)
        set_stream = self.lib.rsik_set_stream
        with torch.cuda.device(self.device):
            planned = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        h, check, gen = self._h, self._check, self._arm_gen

        def launch(stream: Optional[int] = None) -> None:
            if self._arm_gen != gen:
                raise RuntimeError("HipSolver.plan: the arm constants were changed after this launch was planned")
            set_stream(h, planned if stream is None else C.c_void_p(stream))
            rc = fn(h, *args)
            if stream is not None:  # a caller's (capture) stream may not outlive the call: never leave the context on it
                set_stream(h, planned)
            if rc != _abi.RSIK_OK:
                check(rc)

        return launch

    # ------------------------------------------------------------------ rsik_control_discrete
    def control_discrete(
        self,
        m12_soa: torch.Tensor,
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        nb_search_points: int = 20,
        preferred_theta: float = -4 * np.pi / 6,
        constrained_mode: int = _abi.MODE_UNCONSTRAINED,
        previous_sol: Optional[np.ndarray] = None,
        current_joints: Optional[torch.Tensor] = None,
        orbita3d_max_angle: float = float(np.deg2rad(42.5)),
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
        previous_sol_rows: Optional[torch.Tensor] = None,
    ) -> Dict[str, torch.Tensor]:
        """m12_soa: [12, n] float64 (R row-major, then translation).  previous_sol: (2, 7), ControlIK.previous_sol of r and
        l for the whole launch (rsik_control_discrete); previous_sol_rows: [n,7], the previous_sol of the caller that owns
        each goal, for that row's own arm (rsik_control_discrete_rows: n independent callers in one launch).  Not both."""
        if m12_soa.dim() != 2 or m12_soa.shape[0] != 12:
            raise ValueError("m12_soa must have shape [12, n]")
        n = int(m12_soa.shape[1])
        m12_soa = self._dev_cols(m12_soa, 12, n, "m12_soa")
        if nb_search_points < 2:
            raise ValueError("nb_search_points must be >= 2")
        arm = self._arm_ids(arm, n)
        if current_joints is not None:
            current_joints = self._dev_f64(current_joints, (n, 7), "current_joints")
        if previous_sol_rows is not None:
            if previous_sol is not None:
                raise ValueError("previous_sol and previous_sol_rows cannot be combined")
            ps = self._dev_f64(previous_sol_rows, (n, 7), "previous_sol_rows")
            prev, fn_name = _ptr(ps), "rsik_control_discrete_rows"
        else:
            ps = np.ascontiguousarray(previous_sol, dtype=np.float64)
            if ps.shape != (2, 7):
                raise ValueError("previous_sol must have shape (2, 7)")
            prev, fn_name = ps.ctypes.data_as(C.POINTER(C.c_double)), "rsik_control_discrete"
        joints = self._out_buf(out, "joints", (n, 7), _F64)
        reachable = self._out_buf(out, "reachable", (n,), _U8)
        state = self._out_buf(out, "state", (n,), _U8)
        emergency = self._out_buf(out, "emergency", (n,), _U8)
        cols = self._cols(m12_soa, 12)
        cargs = (n, cols, _ptr(arm), int(arm_uniform), int(nb_search_points), float(preferred_theta), int(constrained_mode),
                 prev, _ptr(current_joints), float(orbita3d_max_angle), _ptr(joints), _ptr(reachable), _ptr(state), _ptr(emergency))
        res = {"joints": joints, "reachable": reachable, "state": state, "emergency": emergency}
        return self._finish(res, fn_name, cargs, plan_only, (m12_soa, arm, current_joints, cols, ps))

    # ------------------------------------------------------------------ rsik_control_continuous_step
    def new_continuous_state(self, n: int) -> torch.Tensor:
        return torch.zeros((_abi.CONT_STATE_ROWS, n), dtype=_F64, device=self.device)

    def control_continuous_step(
        self,
        m12_soa: torch.Tensor,
        cont_state: torch.Tensor,
        preferred_theta_self: Sequence[float],
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        timed_out: Optional[torch.Tensor] = None,
        preferred_theta: float = -4 * np.pi / 6,
        constrained_mode: int = _abi.MODE_UNCONSTRAINED,
        d_theta_max: float = 0.01,
        current_joints: Optional[torch.Tensor] = None,
        current_pose_m12: Optional[torch.Tensor] = None,
        orbita3d_max_angle: float = float(np.deg2rad(42.5)),
        out: Optional[Dict[str, torch.Tensor]] = None,
    ) -> Dict[str, torch.Tensor]:
        """One control step for n trajectories; `cont_state` ([RSIK_CONT_STATE_ROWS, n], see include/rsik.h) is updated in place."""
        if m12_soa.dim() != 2 or m12_soa.shape[0] != 12:
            raise ValueError("m12_soa must have shape [12, n]")
        n = int(m12_soa.shape[1])
        m12_soa = self._dev_f64(m12_soa, (12, n), "m12_soa")
        self._check_cont_state(cont_state, n)
        arm = self._arm_ids(arm, n)
        if timed_out is not None:
            timed_out = self._dev_u8(timed_out, n, "timed_out")
        if current_joints is not None:
            current_joints = self._dev_f64(current_joints, (n, 7), "current_joints")
        cp = None
        if current_pose_m12 is not None:
            current_pose_m12 = self._dev_f64(current_pose_m12, (12, n), "current_pose_m12")
            cp = self._cols(current_pose_m12, 12)
        pref_self, pts = self._pair(preferred_theta_self, "preferred_theta_self")  # (pref_self: alive until the call returns)
        joints = self._out_buf(out, "joints", (n, 7), _F64)
        reachable = self._out_buf(out, "reachable", (n,), _U8)
        state = self._out_buf(out, "state", (n,), _U8)
        self._call("rsik_control_continuous_step", n, self._cols(m12_soa, 12), cp, _ptr(arm), int(arm_uniform), _ptr(timed_out),
                   float(preferred_theta), pts, int(constrained_mode), float(d_theta_max), _ptr(current_joints),
                   float(orbita3d_max_angle), _ptr(cont_state), _ptr(joints), _ptr(reachable), _ptr(state))
        return {"joints": joints, "reachable": reachable, "state": state}

    def control_continuous_run(
        self,
        m12_steps: torch.Tensor,
        cont_state: torch.Tensor,
        preferred_theta_self: Sequence[float],
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        first_step_timed_out: bool = True,
        preferred_theta: float = -4 * np.pi / 6,
        constrained_mode: int = _abi.MODE_UNCONSTRAINED,
        d_theta_max: float = 0.01,
        current_joints: Optional[torch.Tensor] = None,
        current_pose_m12: Optional[torch.Tensor] = None,
        orbita3d_max_angle: float = float(np.deg2rad(42.5)),
        out: Optional[Dict[str, torch.Tensor]] = None,
        goals_resident: Optional[bool] = None,
    ) -> "ContinuousRunResult":
        """m12_steps: [n_steps, 12, n] float64 on the device.  All steps of all trajectories from one C call (the phased
        trajectory pipeline of rsik_control_continuous_run, or a launch of the step kernel per control step under
        RSIK_CONT_RUN_STEPS); returns joints [n_steps, n, 7], reachable / state [n_steps, n]; `cont_state` is updated in place.
        The result's attribute `run_form` says how the run was issued (rsik_control_continuous_last_form: _abi.CONT_FORM_*) — in particular
        when the library fell back to a launch per step because the arm's projection margin lets is_reachable_no_limits fail.
        `goals_resident` (None: RSIK_OPT_CONT_GOALS_RESIDENT as set on the context): the caller's promise that lets this run's
        prepare phase start beside the previous run's tail — include/rsik.h."""
        if m12_steps.dim() != 3 or m12_steps.shape[1] != 12:
            raise ValueError("m12_steps must have shape [n_steps, 12, n]")
        n_steps, _, n = (int(v) for v in m12_steps.shape)
        if m12_steps.dtype != _F64 or m12_steps.device != self.device or not m12_steps.is_contiguous():
            m12_steps = m12_steps.to(device=self.device, dtype=_F64).contiguous()
        self._check_cont_state(cont_state, n)
        arm = self._arm_ids(arm, n)
        if current_joints is not None:
            current_joints = self._dev_f64(current_joints, (n, 7), "current_joints")
        cp = None
        if current_pose_m12 is not None:
            current_pose_m12 = self._dev_f64(current_pose_m12, (12, n), "current_pose_m12")
            cp = self._cols(current_pose_m12, 12)
        # (not _pair: this entry point has never refused a preferred_theta_self of another shape, and does not start to here)
        pts = np.ascontiguousarray(preferred_theta_self, dtype=np.float64)
        joints = self._out_buf(out, "joints", (n_steps, n, 7), _F64)
        reachable = self._out_buf(out, "reachable", (n_steps, n), _U8)
        state = self._out_buf(out, "state", (n_steps, n), _U8)
        before = None
        if goals_resident is not None:
            before = self.get_option(_abi.OPT_CONT_GOALS_RESIDENT)
            self.set_option(_abi.OPT_CONT_GOALS_RESIDENT, int(bool(goals_resident)))
        try:
            self._call("rsik_control_continuous_run", n, n_steps, _ptr(m12_steps), cp, _ptr(arm), int(arm_uniform),
                       int(bool(first_step_timed_out)), float(preferred_theta), pts.ctypes.data_as(C.POINTER(C.c_double)),
                       int(constrained_mode), float(d_theta_max), _ptr(current_joints), float(orbita3d_max_angle),
                       _ptr(cont_state), _ptr(joints), _ptr(reachable), _ptr(state))
        finally:
            if before is not None:
                self.set_option(_abi.OPT_CONT_GOALS_RESIDENT, before)
        res = ContinuousRunResult({"joints": joints, "reachable": reachable, "state": state})
        res.run_form = self.continuous_last_form()
        return res

    def continuous_last_form(self) -> int:
        """How the last control_continuous_run of this context was issued: _abi.CONT_FORM_* (names: _abi.CONT_FORM_NAMES)."""
        return int(self.lib.rsik_control_continuous_last_form(self._h))

    # ------------------------------------------------------------------ solver-state entry points
    def new_solver_state(self, n: int) -> torch.Tensor:
        return torch.zeros((n, _abi.SOLVER_STATE_STRIDE), dtype=_F64, device=self.device)

    def reach_state(self, pose_soa: torch.Tensor, solver_state: torch.Tensor, arm: Optional[torch.Tensor] = None,
                    arm_uniform: int = 0, no_limits: bool = False) -> Dict[str, torch.Tensor]:
        n = int(pose_soa.shape[1])
        pose_soa = self._dev_f64(pose_soa, (6, n), "pose_soa")
        self._check_state(solver_state, n)
        arm = self._arm_ids(arm, n)
        interval = torch.empty((n, 2), dtype=_F64, device=self.device)
        reachable = torch.empty((n,), dtype=_U8, device=self.device)
        state = torch.empty((n,), dtype=_U8, device=self.device)
        self._call("rsik_reach_state", n, self._cols(pose_soa, 6), _ptr(arm), int(arm_uniform), int(bool(no_limits)),
                   _ptr(solver_state), _ptr(interval), _ptr(reachable), _ptr(state))
        return {"interval": interval, "reachable": reachable, "state": state}

    def joints_from_state(self, solver_state: torch.Tensor, theta: torch.Tensor, arm: Optional[torch.Tensor] = None,
                          arm_uniform: int = 0, previous_joints: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        n = int(solver_state.shape[0])
        self._check_state(solver_state, n)
        theta = self._dev_f64(theta, (n,), "theta")
        arm = self._arm_ids(arm, n)
        if previous_joints is not None:
            previous_joints = self._dev_f64(previous_joints, (n, 7), "previous_joints")
        joints = torch.empty((n, 7), dtype=_F64, device=self.device)
        elbow = torch.empty((n, 3), dtype=_F64, device=self.device)
        self._call("rsik_joints_from_state", n, _ptr(solver_state), _ptr(arm), int(arm_uniform),
                   _ptr(theta), _ptr(previous_joints), _ptr(joints), _ptr(elbow))
        return {"joints": joints, "elbow": elbow}

    def elbow_from_state(self, solver_state: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
        n = int(solver_state.shape[0])
        self._check_state(solver_state, n)
        theta = self._dev_f64(theta, (n,), "theta")
        elbow = torch.empty((n, 3), dtype=_F64, device=self.device)
        self._call("rsik_elbow_from_state", n, _ptr(solver_state), _ptr(theta), _ptr(elbow))
        return elbow

    # ------------------------------------------------------------------ rsik_theta_from_joints
    def theta_from_joints(
        self,
        goal_soa: torch.Tensor,
        current_joints: torch.Tensor,
        preferred_theta: Sequence[float],
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        want: Sequence[str] = ("joints", "bracket", "distance", "state"),
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """For n independent rows, the theta of the elbow circle whose solution is closest to the row's measured joints
        (utils.get_best_theta_to_current_joints after is_reachable_no_limits: what a caller of the reference does when it
        starts or restarts an arm).  goal_soa: [6, n] poses (px,py,pz,roll,pitch,yaw) or [12, n] matrices (R row-major, t):
        the pose each arm is in.  current_joints: [n, 7].  preferred_theta: 2 values, r and l, used as given.
        Returns theta [n] and, as named in `want`, joints [n,7] (of the last evaluation), bracket [n,2] (the final low, high;
        NaN where the preferred theta itself matched), distance [n] (the objective at theta), state [n] u8.  Asynchronous on
        the current stream; nothing is allocated when every output is in `out`, so the call can be captured into a graph."""
        if not isinstance(goal_soa, torch.Tensor) or goal_soa.dim() != 2 or goal_soa.shape[0] not in (6, 12):
            raise ValueError("goal_soa must have shape [6, n] or [12, n]")
        rows, n = int(goal_soa.shape[0]), int(goal_soa.shape[1])
        if goal_soa.dtype != _F64:
            raise ValueError(f"goal_soa must be float64, got {goal_soa.dtype}")
        goal_soa = self._dev_cols(goal_soa, rows, n, "goal_soa")
        if isinstance(current_joints, torch.Tensor) and current_joints.dtype != _F64:
            raise ValueError(f"current_joints must be float64, got {current_joints.dtype}")
        current_joints = self._dev_f64(current_joints, (n, 7), "current_joints")
        arm = self._arm_ids(arm, n)
        pref, pts = self._pair(preferred_theta, "preferred_theta")
        unknown = set(want) - {"joints", "bracket", "distance", "state"}
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        res = {"theta": self._out_buf(out, "theta", (n,), _F64)}
        for key, shape, dt in (("joints", (n, 7), _F64), ("bracket", (n, 2), _F64), ("distance", (n,), _F64), ("state", (n,), _U8)):
            if key in want:
                res[key] = self._out_buf(out, key, shape, dt)
        cols = self._cols(goal_soa, rows)
        kind = _abi.GOAL_M12 if rows == 12 else _abi.GOAL_POSE6
        cargs = (n, kind, cols, _ptr(arm), int(arm_uniform), _ptr(current_joints), pts,
                 _ptr(res["theta"]), _ptr(res.get("joints")), _ptr(res.get("bracket")), _ptr(res.get("distance")), _ptr(res.get("state")))
        return self._finish(res, "rsik_theta_from_joints", cargs, plan_only, (goal_soa, current_joints, arm, cols, pref))

    def theta_from_joints_state(self, solver_state: torch.Tensor, current_joints: torch.Tensor, preferred_theta: Sequence[float],
                                arm: Optional[torch.Tensor] = None, arm_uniform: int = 0) -> Dict[str, torch.Tensor]:
        """The same search on stored solver-state rows (after reach_state), each row left as the reference leaves `self`
        (rsik_theta_from_joints_state).  current_joints: [n, 7], or [n, 14] for the list-of-both-arms form of ControlIK.__init__.
        Returns theta [n], bracket [n, 2]."""
        n = int(solver_state.shape[0]) if isinstance(solver_state, torch.Tensor) and solver_state.dim() == 2 else -1
        self._check_state(solver_state, n)
        width = int(current_joints.shape[1]) if getattr(current_joints, "ndim", 0) == 2 else -1
        if width not in (7, 14):
            raise ValueError("current_joints must have shape [n, 7] or [n, 14]")
        current_joints = self._dev_f64(current_joints, (n, width), "current_joints")
        arm = self._arm_ids(arm, n)
        pref, pts = self._pair(preferred_theta, "preferred_theta")  # (pref: alive until the call returns)
        theta = torch.empty((n,), dtype=_F64, device=self.device)
        bracket = torch.empty((n, 2), dtype=_F64, device=self.device)
        self._call("rsik_theta_from_joints_state", n, _ptr(solver_state), _ptr(arm), int(arm_uniform),
                   _ptr(current_joints), width, pts, _ptr(theta), _ptr(bracket))
        return {"theta": theta, "bracket": bracket}

    def stage(self, op: int, rows: torch.Tensor, arm_uniform: int = 0) -> torch.Tensor:
        """rsik_stage: one stage of SymbolicIK.is_reachable (include/rsik.h RSIK_STAGE_*) on explicit operands, row by row.
        rows: [n, doubles the stage reads] float64 on the device (or pinned host memory); returns [n, doubles it writes]."""
        need_in, need_out = _abi.STAGE_ROW[int(op)]
        if (not isinstance(rows, torch.Tensor) or rows.dtype != _F64 or rows.dim() != 2 or rows.shape[1] != need_in or not rows.is_contiguous()
                or not (rows.device == self.device or (rows.device.type == "cpu" and rows.is_pinned()))):
            raise ValueError(f"stage {op} takes a contiguous float64 [n, {need_in}] tensor on {self.device} (or in pinned host memory)")
        n = int(rows.shape[0])
        out = torch.empty((n, need_out), dtype=_F64, device=self.device)
        self._call("rsik_stage", int(op), n, int(arm_uniform), _ptr(rows), need_in, _ptr(out), need_out)
        return out

    def _check_cont_state(self, cont_state: torch.Tensor, n: int) -> None:
        if (not isinstance(cont_state, torch.Tensor) or cont_state.dtype != _F64 or cont_state.device != self.device
                or tuple(cont_state.shape) != (_abi.CONT_STATE_ROWS, n) or not cont_state.is_contiguous()):
            raise ValueError(f"cont_state must be a contiguous float64 [{_abi.CONT_STATE_ROWS}, {n}] tensor on {self.device}")

    def _check_state(self, solver_state: torch.Tensor, n: int) -> None:
        if (not isinstance(solver_state, torch.Tensor) or solver_state.dtype != _F64 or solver_state.device != self.device
                or tuple(solver_state.shape) != (n, _abi.SOLVER_STATE_STRIDE) or not solver_state.is_contiguous()):
            raise ValueError(f"solver_state must be a contiguous float64 [{n}, {_abi.SOLVER_STATE_STRIDE}] tensor on {self.device}")

    # ------------------------------------------------------------------ goal matrix <-> Euler pose
    def set_option(self, option: int, value: int) -> None:
        """rsik_set_option, e.g. (_abi.OPT_EULER_ROUNDTRIP, 1): the control kernels run goal matrices through the
        reference's matrix -> Euler -> matrix round trip instead of consuming M[:3,:3] directly."""
        self._check(self.lib.rsik_set_option(self._h, int(option), int(value)))

    def get_option(self, option: int) -> int:
        v = C.c_int(0)
        self._check(self.lib.rsik_get_option(self._h, int(option), C.byref(v)))
        return int(v.value)

    def matrix_to_pose(self, m12_soa: torch.Tensor, identity_shortcut: bool = False) -> torch.Tensor:
        """Goal matrices [12,n] (R row-major, t) -> poses [6,n] (px,py,pz,roll,pitch,yaw): a batched
        utils.get_euler_from_homogeneous_matrix (utils.py:84-90); `identity_shortcut` adds control_ik.py:212-214."""
        if m12_soa.dim() != 2 or m12_soa.shape[0] != 12:
            raise ValueError("m12_soa must have shape [12, n]")
        n = int(m12_soa.shape[1])
        m12_soa = self._dev_f64(m12_soa, (12, n), "m12_soa")
        out = torch.empty((6, n), dtype=_F64, device=self.device)
        self._call("rsik_matrix_to_pose", n, self._cols(m12_soa, 12), 1 if identity_shortcut else 0, self._cols(out, 6))
        return out

    # ------------------------------------------------------------------ forward kinematics
    def forward_kinematics(self, joints: torch.Tensor, arm: Optional[torch.Tensor] = None, arm_uniform: int = 0):
        """joints [n,7] -> (goal position [n,3], goal rotation [n,3,3]) in the torso frame (rsik_forward_kinematics)."""
        n = int(joints.shape[0])
        joints = self._dev_f64(joints, (n, 7), "joints")
        arm = self._arm_ids(arm, n)
        pos = torch.empty((n, 3), dtype=_F64, device=self.device)
        rot = torch.empty((n, 3, 3), dtype=_F64, device=self.device)
        self._call("rsik_forward_kinematics", n, _ptr(joints), _ptr(arm), int(arm_uniform), _ptr(pos), _ptr(rot))
        return pos, rot

    def fk_residual(self, goal_soa: torch.Tensor, joints: torch.Tensor, arm: Optional[torch.Tensor] = None,
                    arm_uniform: int = 0) -> torch.Tensor:
        """FK(joints) against the goals they were solved for: err [n,2] = (position error m, rotation error rad).
        goal_soa: [6,n] poses (px,py,pz,roll,pitch,yaw) or [12,n] matrices (R row-major, t)."""
        if goal_soa.dim() != 2 or goal_soa.shape[0] not in (6, 12):
            raise ValueError("goal_soa must have shape [6, n] or [12, n]")
        rows, n = int(goal_soa.shape[0]), int(goal_soa.shape[1])
        goal_soa = self._dev_f64(goal_soa, (rows, n), "goal_soa")
        joints = self._dev_f64(joints, (n, 7), "joints")
        arm = self._arm_ids(arm, n)
        err = torch.empty((n, 2), dtype=_F64, device=self.device)
        kind = _abi.GOAL_M12 if rows == 12 else _abi.GOAL_POSE6
        self._call("rsik_fk_residual", n, kind, self._cols(goal_soa, rows), _ptr(joints), _ptr(arm), int(arm_uniform), _ptr(err))
        return err

    # ------------------------------------------------------------------ rsik_jacobian
    JACOBIAN_OUTPUTS = ("jacobian", "null_vector", "manipulability")

    def jacobian(
        self,
        joints: torch.Tensor,
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        want: Sequence[str] = JACOBIAN_OUTPUTS,
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """How the goal frame moves with the joints, from one launch (rsik_jacobian).  joints: [n, 7], or [n_rep, n, 7] — the
        sample-major joints of solve_sweep, the waypoint-major joints of solve_path — in the convention solve() returns and
        forward_kinematics() reads.  arm: [n] u8, one byte per row, shared by every repetition, or None with arm_uniform.
        `want`: which of the three outputs to compute, at least one; the bits of one do not depend on the others.  Returns device
        tensors shaped like the joints' leading dimensions:
        jacobian [..., 6, 7]: column k is the goal frame's velocity per unit rate of joint k in the torso frame, rows 0-2 the
        derivative of forward_kinematics' position (tip offset included), rows 3-5 the angular velocity w_k, dR/dq_k = [w_k]x R;
        null_vector [..., 7]: the signed minors of J, null[i] = (-1)^i det(J without column i): J . null = 0, the sign is defined,
        the vector is continuous, not normalised, and the zero vector at a singularity; away from singularities and from the
        elbow projection and the elbow-limit clamp it is parallel to d joints / d theta of solve();
        manipulability [...]: |null| = sqrt(det(J J^T)), Yoshikawa's measure; 0, not NaN, at a singular row.
        A row that holds a NaN or an infinity gives NaN in all three.
        plan_only=True launches nothing and adds res["launch"], a zero-overhead re-launch callable (see plan())."""
        if not isinstance(joints, torch.Tensor):
            joints = torch.as_tensor(np.asarray(joints, dtype=np.float64))
        if joints.dim() not in (2, 3) or joints.shape[-1] != 7:
            raise ValueError("joints must have shape [n, 7] or [n_rep, n, 7]")
        lead = tuple(int(v) for v in joints.shape[:-1])
        n_rep, n = (1, lead[0]) if len(lead) == 1 else lead
        if n_rep < 1:
            raise ValueError("joints: at least one repetition")
        want = tuple(want)
        if not want or any(name not in self.JACOBIAN_OUTPUTS for name in want):
            raise ValueError(f"want must name at least one of {self.JACOBIAN_OUTPUTS}")
        joints = self._dev_f64(joints, lead + (7,), "joints")
        arm = self._arm_ids(arm, n)
        shapes = {"jacobian": lead + (6, 7), "null_vector": lead + (7,), "manipulability": lead}
        res = {name: self._out_buf(out, name, shapes[name], _F64) for name in self.JACOBIAN_OUTPUTS if name in want}
        cargs = (n, n_rep, _ptr(joints), _ptr(arm), int(arm_uniform),
                 _ptr(res.get("jacobian")), _ptr(res.get("null_vector")), _ptr(res.get("manipulability")))
        return self._finish(res, "rsik_jacobian", cargs, plan_only, (joints, arm))

    # ------------------------------------------------------------------ rsik_joint_rates
    JOINT_RATES_OUTPUTS = ("rates", "achieved_twist")

    def joint_rates(
        self,
        joints: torch.Tensor,
        twist: torch.Tensor,
        damping: Any = None,
        bias_rates: Optional[torch.Tensor] = None,
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        want: Sequence[str] = ("rates",),
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """The joint rates that give the goal frame a wanted twist, damped least squares on the Jacobian of jacobian(), from one
        launch in which J stays in registers (rsik_joint_rates).  joints: [n, 7] or [n_rep, n, 7] as jacobian() takes them; twist:
        the same leading shape, [..., 6], in the row order of the Jacobian (entries 0-2 the linear velocity of the goal-frame origin,
        3-5 the angular velocity, torso frame); damping: lambda, a float (finite, > 0) for every row or a tensor [..., n] with one
        lambda per row (e.g. derived from jacobian()'s manipulability); bias_rates: [..., 7] or None for zeros, the rates q0 the arm
        would like to have (joint centring, or a self-motion command k * null_vector); arm / arm_uniform as jacobian().
        Per row, rates minimises |J q' - twist|^2 + lambda^2 |q' - q0|^2; it is computed as q0 + J^T y with
        (J J^T + lambda^2 I) y = twist - J q0, an L D L^T factorisation in natural order in which every pivot is clamped from below
        at lambda^2 (the exact pivots are never smaller, so the pivot clamp changes no exact result; it keeps a finite row finite at a
        straight elbow and with a tiny lambda).  lambda = 0 is not offered: 1e-6 is the pseudo-inverse to every digit that survives.
        `want`: which of rates [..., 7] and achieved_twist [..., 6] (= J . rates, short of twist by the damping) to compute, at least
        one; the bits of one do not depend on the other.  A row with a NaN or an infinity in joints, twist or bias, or with a lambda
        that is NaN, infinite or <= 0, is NaN in both.
        plan_only=True launches nothing and adds res["launch"], a zero-overhead re-launch callable (see plan())."""
        if not isinstance(joints, torch.Tensor):
            joints = torch.as_tensor(np.asarray(joints, dtype=np.float64))
        if joints.dim() not in (2, 3) or joints.shape[-1] != 7:
            raise ValueError("joints must have shape [n, 7] or [n_rep, n, 7]")
        lead = tuple(int(v) for v in joints.shape[:-1])
        n_rep, n = (1, lead[0]) if len(lead) == 1 else lead
        if n_rep < 1:
            raise ValueError("joints: at least one repetition")
        want = tuple(want)
        if not want or any(name not in self.JOINT_RATES_OUTPUTS for name in want):
            raise ValueError(f"want must name at least one of {self.JOINT_RATES_OUTPUTS}")
        if damping is None:
            raise ValueError("damping: a float > 0 or a tensor with one lambda per row")
        joints = self._dev_f64(joints, lead + (7,), "joints")
        twist = self._dev_f64(twist, lead + (6,), "twist")
        bias_rates = None if bias_rates is None else self._dev_f64(bias_rates, lead + (7,), "bias_rates")
        if isinstance(damping, (int, float)):
            damping_host, damping = float(damping), None
            if not (np.isfinite(damping_host) and damping_host > 0.0):
                raise ValueError("damping must be finite and > 0")
        else:
            damping_host, damping = 0.0, self._dev_f64(damping, lead, "damping")
        arm = self._arm_ids(arm, n)
        shapes = {"rates": lead + (7,), "achieved_twist": lead + (6,)}
        res = {name: self._out_buf(out, name, shapes[name], _F64) for name in self.JOINT_RATES_OUTPUTS if name in want}
        cargs = (n, n_rep, _ptr(joints), _ptr(arm), int(arm_uniform), _ptr(twist), damping_host, _ptr(damping), _ptr(bias_rates),
                 _ptr(res.get("rates")), _ptr(res.get("achieved_twist")))
        return self._finish(res, "rsik_joint_rates", cargs, plan_only, (joints, twist, damping, bias_rates, arm))

    # ------------------------------------------------------------------ rsik_track
    TRACK_OUTPUTS = ("joints", "rates", "err", "final_joints", "final_err")

    def track(
        self,
        m12_steps: torch.Tensor,
        start_joints: torch.Tensor,
        dt: float,
        kp: float,
        ko: float,
        damping: Any = None,
        feedforward: Optional[torch.Tensor] = None,
        rest_joints: Optional[torch.Tensor] = None,
        rest_gain: float = 0.0,
        limits: Any = None,
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        want: Sequence[str] = ("joints",),
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """Closed-loop tracking of n goal trajectories over T steps at the velocity level, every step in one launch in which the
        joints stay in registers (rsik_track).  m12_steps: [T, 12, n] goal matrices (R row-major, then t: the layout of
        control_continuous_run; R must be a rotation, it is consumed as it comes); start_joints: [n, 7]; dt > 0; kp, ko >= 0 the
        gains on the position and orientation error; damping: lambda of joint_rates(), a float or a tensor [n], one per trajectory;
        feedforward: [T, n, 6] or None for zeros, a twist in the row order of the Jacobian; rest_joints: [n, 7] or None, with
        rest_gain >= 0; limits: [3, 7] on the host (rows rate_max > 0, q_min <= q_max; infinities allowed) or None for none;
        arm / arm_uniform as jacobian().
        Per trajectory, q := start_joints, then for every step t: (p, R) = forward_kinematics(q); e_p = p_g - p, e_o the rotation
        vector of R_g R^T (close to 0, its direction undefined, at a rotation by pi); v = feedforward[t] + (kp e_p, ko e_o);
        q0 = rest_gain (rest_joints - q); q' = joint_rates(q, v, lambda, q0) exactly; with limits q' is scaled by one factor so that
        no |q'_k| exceeds rate_max_k; q := q + dt q', clamped to [q_min, q_max] with limits.
        `want`: which of TRACK_OUTPUTS to compute, at least one; the bits of one do not depend on the others.  Returns device
        tensors: joints [T, n, 7] (after every step), rates [T, n, 7] (after the limit), err [T, n, 2] (|e_p| in m and the rotation
        angle in rad each step saw, before it moved), final_joints [n, 7], final_err [n, 2] (the last goal at the last joints).
        A trajectory with a NaN or an infinity in its start or rest row, or an unusable lambda, is NaN everywhere; a step whose
        goal or feed-forward is not numbers is skipped (joints held, rates 0, err NaN) and the trajectory goes on.
        plan_only=True launches nothing and adds res["launch"], a zero-overhead re-launch callable (see plan())."""
        if not isinstance(m12_steps, torch.Tensor):
            m12_steps = torch.as_tensor(np.asarray(m12_steps, dtype=np.float64))
        if m12_steps.dim() != 3 or m12_steps.shape[1] != 12:
            raise ValueError("m12_steps must have shape [n_steps, 12, n]")
        n_steps, n = int(m12_steps.shape[0]), int(m12_steps.shape[2])
        if not 1 <= n_steps <= 65536:
            raise ValueError("m12_steps: between 1 and 65536 steps")
        want = tuple(want)
        if not want or any(name not in self.TRACK_OUTPUTS for name in want):
            raise ValueError(f"want must name at least one of {self.TRACK_OUTPUTS}")
        if damping is None:
            raise ValueError("damping: a float > 0 or a tensor with one lambda per trajectory")
        dt, kp, ko, rest_gain = float(dt), float(kp), float(ko), float(rest_gain)
        if not (np.isfinite(dt) and dt > 0.0):
            raise ValueError("dt must be finite and > 0")
        for name, gain in (("kp", kp), ("ko", ko), ("rest_gain", rest_gain)):
            if not (np.isfinite(gain) and gain >= 0.0):
                raise ValueError(f"{name} must be finite and >= 0")
        m12_steps = self._dev_f64(m12_steps, (n_steps, 12, n), "m12_steps")
        start_joints = self._dev_f64(start_joints, (n, 7), "start_joints")
        feedforward = None if feedforward is None else self._dev_f64(feedforward, (n_steps, n, 6), "feedforward")
        rest_joints = None if rest_joints is None else self._dev_f64(rest_joints, (n, 7), "rest_joints")
        if isinstance(damping, (int, float)):
            damping_host, damping = float(damping), None
            if not (np.isfinite(damping_host) and damping_host > 0.0):
                raise ValueError("damping must be finite and > 0")
        else:
            damping_host, damping = 0.0, self._dev_f64(damping, (n,), "damping")
        lim, lim_p = None, None
        if limits is not None:
            lim = np.ascontiguousarray(limits.cpu().numpy() if isinstance(limits, torch.Tensor) else limits, dtype=np.float64)
            if lim.shape != (3, 7) or np.isnan(lim).any() or not (lim[0] > 0.0).all() or not (lim[1] <= lim[2]).all():
                raise ValueError("limits must be [3, 7]: rate_max > 0, q_min <= q_max, no NaN")
            lim_p = lim.ctypes.data_as(C.POINTER(C.c_double))
        arm = self._arm_ids(arm, n)
        shapes = {"joints": (n_steps, n, 7), "rates": (n_steps, n, 7), "err": (n_steps, n, 2), "final_joints": (n, 7), "final_err": (n, 2)}
        res = {name: self._out_buf(out, name, shapes[name], _F64) for name in self.TRACK_OUTPUTS if name in want}
        cargs = (n, n_steps, _ptr(m12_steps), _ptr(arm), int(arm_uniform), _ptr(start_joints), dt, kp, ko, _ptr(feedforward),
                 damping_host, _ptr(damping), _ptr(rest_joints), rest_gain, lim_p) + tuple(_ptr(res.get(name)) for name in self.TRACK_OUTPUTS)
        return self._finish(res, "rsik_track", cargs, plan_only, (m12_steps, start_joints, feedforward, damping, rest_joints, arm, lim))

    # ------------------------------------------------------------------ rsik_track_avoid
    TRACK_AVOID_OUTPUTS = ("joints", "rates", "err", "clearance", "nearest", "final_joints", "final_err", "min_clearance")
    TRACK_AVOID_MAX_SPHERES, TRACK_AVOID_MAX_CAPSULES = 256, 64

    def track_avoid(
        self,
        m12_steps: torch.Tensor,
        start_joints: torch.Tensor,
        dt: float,
        kp: float,
        ko: float,
        damping: Any = None,
        spheres: Optional[torch.Tensor] = None,
        capsules: Optional[torch.Tensor] = None,
        link_radius: Any = None,
        influence: float = 0.0,
        avoid_gain: float = 0.0,
        feedforward: Optional[torch.Tensor] = None,
        rest_joints: Optional[torch.Tensor] = None,
        rest_gain: float = 0.0,
        limits: Any = None,
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        want: Sequence[str] = ("joints",),
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """track() with obstacle avoidance inside the loop, every step in one launch (rsik_track_avoid).  Every argument of track()
        means what it means there; spheres [S, 4], capsules [Cp, 7] and link_radius are clearance()'s, static and shared by every
        trajectory and step, with S <= 256, Cp <= 64 and at least one obstacle (without obstacles: track()).
        Per step, (d, nearest, g) = clearance, nearest and gradient of clearance() at the current joints; the bias is
        q0 = rest_gain (rest_joints - q), and where d < influence (m, >= 0) q0 += avoid_gain (influence - d) g; the rates are
        joint_rates(q, v, lambda, q0) as in track().  The push is a bias: it acts in the null space of the task first.
        `want`: which of TRACK_AVOID_OUTPUTS to compute, at least one; the bits of one do not depend on the others.  Beside track()'s
        five: clearance [T, n] and nearest [T, n, 2] int32 (link, obstacle index) that each step saw before it moved, bit for bit
        clearance()'s at those joints, and min_clearance [n], the minimum of clearance over the steps and at the final joints.
        A trajectory the push never acts on has track()'s bits.
        plan_only=True launches nothing and adds res["launch"], a zero-overhead re-launch callable (see plan())."""
        return self._track_avoid("rsik_track_avoid", m12_steps, start_joints, dt, kp, ko, damping, spheres, capsules, link_radius, influence,
                                 avoid_gain, feedforward, rest_joints, rest_gain, limits, arm, arm_uniform, want, out, plan_only)

    def _track_avoid(self, symbol, m12_steps, start_joints, dt, kp, ko, damping, spheres, capsules, link_radius, influence, avoid_gain,
                     feedforward, rest_joints, rest_gain, limits, arm, arm_uniform, want, out, plan_only):
        """What track_avoid() and track_pair() share: the checks, the buffers and the call.  rsik_track_pair takes no arm arguments,
        an even number of rows, and no static obstacle is allowed."""
        pairs = symbol == "rsik_track_pair"
        if not isinstance(m12_steps, torch.Tensor):
            m12_steps = torch.as_tensor(np.asarray(m12_steps, dtype=np.float64))
        if m12_steps.dim() != 3 or m12_steps.shape[1] != 12:
            raise ValueError("m12_steps must have shape [n_steps, 12, n]")
        n_steps, n = int(m12_steps.shape[0]), int(m12_steps.shape[2])
        if not 1 <= n_steps <= 65536:
            raise ValueError("m12_steps: between 1 and 65536 steps")
        if pairs and n % 2:
            raise ValueError("m12_steps: an even number of rows, the right arm of robot i in row 2 i and its left arm in row 2 i + 1")
        want = tuple(want)
        if not want or any(name not in self.TRACK_AVOID_OUTPUTS for name in want):
            raise ValueError(f"want must name at least one of {self.TRACK_AVOID_OUTPUTS}")
        if damping is None:
            raise ValueError("damping: a float > 0 or a tensor with one lambda per trajectory")
        dt, kp, ko, rest_gain, influence, avoid_gain = float(dt), float(kp), float(ko), float(rest_gain), float(influence), float(avoid_gain)
        if not (np.isfinite(dt) and dt > 0.0):
            raise ValueError("dt must be finite and > 0")
        for name, gain in (("kp", kp), ("ko", ko), ("rest_gain", rest_gain), ("influence", influence), ("avoid_gain", avoid_gain)):
            if not (np.isfinite(gain) and gain >= 0.0):
                raise ValueError(f"{name} must be finite and >= 0")

        def rows(t, width, most, name):
            if t is None:
                return None, 0
            if not isinstance(t, torch.Tensor):
                t = torch.as_tensor(np.asarray(t, dtype=np.float64))
            if t.dim() != 2 or t.shape[1] != width or t.shape[0] > most:
                raise ValueError(f"{name} must have shape [k, {width}] with k <= {most}")
            count = int(t.shape[0])
            return (self._dev_f64(t, (count, width), name) if count else None), count

        spheres, n_spheres = rows(spheres, 4, self.TRACK_AVOID_MAX_SPHERES, "spheres")
        capsules, n_capsules = rows(capsules, 7, self.TRACK_AVOID_MAX_CAPSULES, "capsules")
        if not pairs and n_spheres + n_capsules < 1:
            raise ValueError("at least one obstacle: spheres [k, 4] or capsules [k, 7] (without obstacles: track())")
        rad, rad_p = None, None
        if link_radius is not None:
            rad = np.ascontiguousarray(link_radius.cpu().numpy() if isinstance(link_radius, torch.Tensor) else link_radius, dtype=np.float64)
            if rad.shape != (3,) or not np.isfinite(rad).all() or not (rad >= 0.0).all():
                raise ValueError("link_radius must be 3 finite values >= 0")
            rad_p = rad.ctypes.data_as(C.POINTER(C.c_double))
        m12_steps = self._dev_f64(m12_steps, (n_steps, 12, n), "m12_steps")
        start_joints = self._dev_f64(start_joints, (n, 7), "start_joints")
        feedforward = None if feedforward is None else self._dev_f64(feedforward, (n_steps, n, 6), "feedforward")
        rest_joints = None if rest_joints is None else self._dev_f64(rest_joints, (n, 7), "rest_joints")
        if isinstance(damping, (int, float)):
            damping_host, damping = float(damping), None
            if not (np.isfinite(damping_host) and damping_host > 0.0):
                raise ValueError("damping must be finite and > 0")
        else:
            damping_host, damping = 0.0, self._dev_f64(damping, (n,), "damping")
        lim, lim_p = None, None
        if limits is not None:
            lim = np.ascontiguousarray(limits.cpu().numpy() if isinstance(limits, torch.Tensor) else limits, dtype=np.float64)
            if lim.shape != (3, 7) or np.isnan(lim).any() or not (lim[0] > 0.0).all() or not (lim[1] <= lim[2]).all():
                raise ValueError("limits must be [3, 7]: rate_max > 0, q_min <= q_max, no NaN")
            lim_p = lim.ctypes.data_as(C.POINTER(C.c_double))
        arm = None if pairs else self._arm_ids(arm, n)
        shapes = {"joints": (n_steps, n, 7), "rates": (n_steps, n, 7), "err": (n_steps, n, 2), "clearance": (n_steps, n),
                  "nearest": (n_steps, n, 2), "final_joints": (n, 7), "final_err": (n, 2), "min_clearance": (n,)}
        res = {name: self._out_buf(out, name, shapes[name], torch.int32 if name == "nearest" else _F64)
               for name in self.TRACK_AVOID_OUTPUTS if name in want}
        rows = (n // 2, n_steps, _ptr(m12_steps)) if pairs else (n, n_steps, _ptr(m12_steps), _ptr(arm), int(arm_uniform))
        cargs = rows + (_ptr(start_joints), dt, kp, ko, _ptr(feedforward),
                        damping_host, _ptr(damping), _ptr(rest_joints), rest_gain, lim_p, rad_p, n_spheres, _ptr(spheres), n_capsules,
                        _ptr(capsules), influence, avoid_gain) + tuple(_ptr(res.get(name)) for name in self.TRACK_AVOID_OUTPUTS)
        return self._finish(res, symbol, cargs, plan_only,
                            (m12_steps, start_joints, feedforward, damping, rest_joints, arm, lim, spheres, capsules, rad))

    # ------------------------------------------------------------------ rsik_track_pair
    TRACK_PAIR_OUTPUTS = TRACK_AVOID_OUTPUTS

    def track_pair(
        self,
        m12_steps: torch.Tensor,
        start_joints: torch.Tensor,
        dt: float,
        kp: float,
        ko: float,
        damping: Any = None,
        spheres: Optional[torch.Tensor] = None,
        capsules: Optional[torch.Tensor] = None,
        link_radius: Any = None,
        influence: float = 0.0,
        avoid_gain: float = 0.0,
        feedforward: Optional[torch.Tensor] = None,
        rest_joints: Optional[torch.Tensor] = None,
        rest_gain: float = 0.0,
        limits: Any = None,
        want: Sequence[str] = ("joints",),
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """track_avoid() for robots of two arms that avoid each other, every step of both arms in one launch (rsik_track_pair).
        The n = 2 n_pairs rows of every array are interleaved: row 2 i is the right arm of robot i, row 2 i + 1 its left arm; there
        is no arm argument, and both arms' constants must be set.  Every other argument means what it means in track_avoid():
        m12_steps [T, 12, n], start_joints [n, 7], damping a float or [n], feedforward [T, n, 6], rest_joints [n, 7], limits [3, 7],
        spheres [S, 4] and capsules [Cp, 7] with S <= 256, Cp <= 64 — and here no static obstacle at all is allowed, because the
        partner is always one.
        Per step each arm's obstacles are the spheres, the capsules, and then the other arm's three links as capsules (its
        link_points of clearance() at the joints it has reached, with link_radius), obstacle indices S + Cp + l; both arms look at
        each other's joints from before the step.  influence, avoid_gain and the push are track_avoid()'s; the gradient is with
        respect to the row's own joints.
        `want`: which of TRACK_PAIR_OUTPUTS (= TRACK_AVOID_OUTPUTS) to compute, at least one; the bits of one do not depend on the
        others: joints, rates [T, n, 7], err [T, n, 2], clearance [T, n], nearest [T, n, 2] int32, final_joints [n, 7], final_err
        [n, 2], min_clearance [n].  clearance and nearest are bit for bit clearance()'s for the row's joints before the step with
        the static capsules followed by the partner's three.  An arm that is NaN (start, rest, damping) is NaN in its own outputs and
        no obstacle for its partner, which then has track_avoid()'s bits for the static scene.
        plan_only=True launches nothing and adds res["launch"], a zero-overhead re-launch callable (see plan())."""
        return self._track_avoid("rsik_track_pair", m12_steps, start_joints, dt, kp, ko, damping, spheres, capsules, link_radius, influence,
                                 avoid_gain, feedforward, rest_joints, rest_gain, limits, None, 0, want, out, plan_only)

    # ------------------------------------------------------------------ rsik_clearance
    CLEARANCE_OUTPUTS = ("clearance", "nearest", "gradient", "witness", "link_points")
    CLEARANCE_MAX_SPHERES, CLEARANCE_MAX_CAPSULES = 4096, 256

    def clearance(
        self,
        joints: torch.Tensor,
        spheres: Optional[torch.Tensor] = None,
        capsules: Optional[torch.Tensor] = None,
        link_radius: Any = None,
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        want: Sequence[str] = ("clearance", "nearest"),
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """How far the arm is from a set of obstacles, from one launch (rsik_clearance).  The arm is three capsules — link 0
        shoulder -> elbow, link 1 elbow -> wrist, link 2 wrist -> goal origin (forward_kinematics' position) — with the radii
        link_radius (3 values on the host, or None for zeros).  joints: [n, 7] or [n_rep, n, 7] as jacobian() takes them (a sweep's
        or a path's joints in place); spheres: [S, 4] rows (x, y, z, r), S <= 4096, or None; capsules: [Cp, 7] rows (a, b, r),
        Cp <= 256, a == b allowed, or None; torso frame, shared by every row; at least one obstacle.  arm / arm_uniform as jacobian().
        `want`: which of CLEARANCE_OUTPUTS to compute, at least one; the bits of one do not depend on the others.  Returns device
        tensors shaped like the joints' leading dimensions:
        clearance [...]: the minimum over links and obstacles of (distance between the axis segments) - link radius - obstacle
        radius; negative where the radii penetrate;
        nearest [..., 2] int32: (link, obstacle index) of the pair that gives it — spheres are 0 ... S - 1, capsule j is S + j; the
        first minimum in the order (obstacle 0, link 0), (obstacle 0, link 1), (obstacle 0, link 2), (obstacle 1, link 0) ...;
        witness [..., 2, 3]: x on the link's axis and y on the obstacle's axis, a pair that attains the distance;
        gradient [..., 7]: d clearance / d joints of that pair, u . (a_k x (x - o_k)) for the joints that move the link, 0 for the
        others and the zero vector where the axes touch: k * gradient is a bias_rates for joint_rates() and track();
        link_points [..., 4, 3]: shoulder, elbow, wrist, goal origin.
        A row with a NaN or an infinity among its joints is NaN with nearest (-1, -1).  An obstacle row with a NaN, an infinity or a
        negative radius is skipped; if all are: clearance +inf, nearest (-1, -1), gradient 0, witness NaN.
        plan_only=True launches nothing and adds res["launch"], a zero-overhead re-launch callable (see plan())."""
        if not isinstance(joints, torch.Tensor):
            joints = torch.as_tensor(np.asarray(joints, dtype=np.float64))
        if joints.dim() not in (2, 3) or joints.shape[-1] != 7:
            raise ValueError("joints must have shape [n, 7] or [n_rep, n, 7]")
        lead = tuple(int(v) for v in joints.shape[:-1])
        n_rep, n = (1, lead[0]) if len(lead) == 1 else lead
        if n_rep < 1:
            raise ValueError("joints: at least one repetition")
        want = tuple(want)
        if not want or any(name not in self.CLEARANCE_OUTPUTS for name in want):
            raise ValueError(f"want must name at least one of {self.CLEARANCE_OUTPUTS}")

        def rows(t, width, most, name):
            if t is None:
                return None, 0
            if not isinstance(t, torch.Tensor):
                t = torch.as_tensor(np.asarray(t, dtype=np.float64))
            if t.dim() != 2 or t.shape[1] != width or t.shape[0] > most:
                raise ValueError(f"{name} must have shape [k, {width}] with k <= {most}")
            count = int(t.shape[0])
            return (self._dev_f64(t, (count, width), name) if count else None), count

        spheres, n_spheres = rows(spheres, 4, self.CLEARANCE_MAX_SPHERES, "spheres")
        capsules, n_capsules = rows(capsules, 7, self.CLEARANCE_MAX_CAPSULES, "capsules")
        if n_spheres + n_capsules < 1:
            raise ValueError("at least one obstacle: spheres [k, 4] or capsules [k, 7]")
        rad, rad_p = None, None
        if link_radius is not None:
            rad = np.ascontiguousarray(link_radius.cpu().numpy() if isinstance(link_radius, torch.Tensor) else link_radius, dtype=np.float64)
            if rad.shape != (3,) or not np.isfinite(rad).all() or not (rad >= 0.0).all():
                raise ValueError("link_radius must be 3 finite values >= 0")
            rad_p = rad.ctypes.data_as(C.POINTER(C.c_double))
        joints = self._dev_f64(joints, lead + (7,), "joints")
        arm = self._arm_ids(arm, n)
        shapes = {"clearance": lead, "nearest": lead + (2,), "gradient": lead + (7,), "witness": lead + (2, 3), "link_points": lead + (4, 3)}
        res = {name: self._out_buf(out, name, shapes[name], torch.int32 if name == "nearest" else _F64)
               for name in self.CLEARANCE_OUTPUTS if name in want}
        cargs = (n, n_rep, _ptr(joints), _ptr(arm), int(arm_uniform), rad_p, n_spheres, _ptr(spheres), n_capsules, _ptr(capsules)) \
            + tuple(_ptr(res.get(name)) for name in self.CLEARANCE_OUTPUTS)
        return self._finish(res, "rsik_clearance", cargs, plan_only, (joints, arm, spheres, capsules, rad))

    # ------------------------------------------------------------------ rsik_clearance_edges
    CLEARANCE_EDGES_OUTPUTS = ("edge_clearance", "edge_sub", "edge_nearest", "edge_bound",
                               "path_clearance", "path_edge", "path_bound", "n_below", "first_below")
    CLEARANCE_EDGES_MAX_SUB = 256

    def clearance_edges_workspace_bytes(self, n: int, n_steps: int) -> int:
        """rsik_clearance_edges_workspace_bytes: the device workspace the per-path outputs of a clearance_edges of this shape need."""
        b = C.c_size_t(0)
        rc = self.lib.rsik_clearance_edges_workspace_bytes(int(n), int(n_steps), C.byref(b))
        if rc != _abi.RSIK_OK:
            raise _abi.RsikError(rc, "rsik_clearance_edges_workspace_bytes: n >= 0, n_steps 1 ... 65536")
        return int(b.value)

    def clearance_edges(
        self,
        joints: torch.Tensor,
        start_joints: Optional[torch.Tensor] = None,
        n_sub: int = 16,
        *,
        spheres: Optional[torch.Tensor] = None,
        capsules: Optional[torch.Tensor] = None,
        link_radius: Any = None,
        arm: Optional[torch.Tensor] = None,
        arm_uniform: int = 0,
        min_clearance: float = -float("inf"),
        want: Sequence[str] = CLEARANCE_EDGES_OUTPUTS,
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """The clearance of n paths ALONG the motion between their waypoints, from one call (rsik_clearance_edges): solve_path_clear()
        and solve_path_pair() keep min_clearance at the waypoints only; this verifies the way between them.
        joints: [T, n, 7], waypoint-major, the `joints` of solve_path(), solve_path_clear() or solve_path_pair() (with or without
        unwind) or joints_steps of the track calls, in place; a row with a NaN or an infinity is not a waypoint (a skipped one) and
        the edge bridges it.  start_joints: [n, 7] or None.  n_sub: S, 1 ... 256 sub-steps per edge.  spheres [k, 4], k <= 256,
        capsules [k, 7], k <= 64, link_radius: solve_path_clear()'s scene, at least one obstacle.  arm: [n], one byte per path.
        The edge into waypoint (t, i) runs from the waypoint before it (or the start row) joint by joint the short way round:
        q(s) = a + angle_diff(b, a) * (s / S), s = 0 ... S, q(S) = b; a first waypoint without a start row is the one sample s = S.
        `want`: which of CLEARANCE_EDGES_OUTPUTS to compute, at least one; the bits of one do not depend on the others.  Returns
        device tensors:
        edge_clearance [T, n]: the least clearance()'s `clearance` over the samples; edge_sub [T, n] int32: the lowest s that attains
        it; edge_nearest [T, n, 2] int32: that sample's (link, obstacle index);
        edge_bound [T, n]: edge_clearance - sum_k |delta_k| R_k / (2 S), R_k the arm's reach beyond joint k — a certified lower bound
        on the clearance of the whole continuous motion of the edge (include/rsik.h derives it): edge_bound > 0 proves the edge free;
        NaN, -1, (-1, -1), NaN where row t is not a waypoint; +inf, the first s, (-1, -1), +inf where every obstacle is skipped;
        path_clearance [n], path_edge [n, 2] int32 (t, s) of it, path_bound [n]: the minima over a path's edges; n_below [n] int32:
        the edges with edge_clearance < min_clearance (m; -inf: none), first_below [n] int32: the first such t or -1.  A path
        without a waypoint, or whose start row is not numbers: NaN, (-1, -1), NaN, 0, -1.
        The workspace the per-path outputs need is allocated here, with torch; a plan keeps it and the obstacle tensors alive.
        plan_only=True launches nothing and adds res["launch"], a zero-overhead re-launch callable (see plan())."""
        if not isinstance(joints, torch.Tensor):
            joints = torch.as_tensor(np.asarray(joints, dtype=np.float64))
        if joints.dim() != 3 or joints.shape[-1] != 7:
            raise ValueError("joints must have shape [T, n, 7]")
        t, n = int(joints.shape[0]), int(joints.shape[1])
        if not 1 <= t <= 65536:
            raise ValueError("joints: between 1 and 65536 waypoints per path")
        n_sub = int(n_sub)
        if not 1 <= n_sub <= self.CLEARANCE_EDGES_MAX_SUB:
            raise ValueError(f"n_sub must be 1 ... {self.CLEARANCE_EDGES_MAX_SUB}")
        want = tuple(want)
        if not want or any(name not in self.CLEARANCE_EDGES_OUTPUTS for name in want):
            raise ValueError(f"want must name at least one of {self.CLEARANCE_EDGES_OUTPUTS}")
        keep, scene_args = self._path_scene(spheres, capsules, link_radius, True)
        joints = self._dev_f64(joints, (t, n, 7), "joints")
        if start_joints is not None:
            start_joints = self._dev_f64(start_joints, (n, 7), "start_joints")
        arm = self._arm_ids(arm, n)
        shapes = {"edge_clearance": ((t, n), _F64), "edge_sub": ((t, n), torch.int32), "edge_nearest": ((t, n, 2), torch.int32),
                  "edge_bound": ((t, n), _F64), "path_clearance": ((n,), _F64), "path_edge": ((n, 2), torch.int32),
                  "path_bound": ((n,), _F64), "n_below": ((n,), torch.int32), "first_below": ((n,), torch.int32)}
        res = {name: self._out_buf(out, name, *shapes[name]) for name in self.CLEARANCE_EDGES_OUTPUTS if name in want}
        workspace, ws_bytes = None, 0
        if any(name in want for name in self.CLEARANCE_EDGES_OUTPUTS[4:]):
            ws_bytes = self.clearance_edges_workspace_bytes(n, t)
            workspace = torch.empty((max(ws_bytes, 8) // 8,), dtype=_F64, device=self.device)
        cargs = (n, t, _ptr(joints), _ptr(arm), int(arm_uniform), _ptr(start_joints), n_sub) + scene_args \
            + (float(min_clearance), _ptr(workspace), ws_bytes) + tuple(_ptr(res.get(name)) for name in self.CLEARANCE_EDGES_OUTPUTS)
        return self._finish(res, "rsik_clearance_edges", cargs, plan_only, (joints, start_joints, arm, workspace) + keep)

    # ------------------------------------------------------------------ measurement hooks
    def clock_monitor(self, seconds: float, n_waves: int = 64, stream: Optional[torch.cuda.Stream] = None):
        """Starts rsik_debug_math op 8 on `stream` (a side stream, so that it runs BESIDE whatever the main stream is
        doing): n_waves one-wave workgroups each wait `seconds` (clamped to 5 s) and report shader-clock and 100 MHz
        ticks.  Returns (core_ticks, real_ticks) device tensors, valid once `stream` has been synchronised;
        core clock in GHz = core_ticks / real_ticks * 0.1."""
        ticks = torch.tensor([float(seconds) * 1e8], dtype=_F64, device=self.device)
        o0 = torch.zeros((n_waves,), dtype=_F64, device=self.device)
        o1 = torch.zeros((n_waves,), dtype=_F64, device=self.device)
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        st.wait_stream(torch.cuda.current_stream(self.device))  # the tick count must have been written
        with torch.cuda.device(self.device):
            self._check(self.lib.rsik_set_stream(self._h, C.c_void_p(st.cuda_stream)))
            self._check(self.lib.rsik_debug_math(self._h, 8, int(n_waves), _ptr(ticks), None, _ptr(o0), _ptr(o1)))
            self._bind_stream()
        for t in (ticks, o0, o1):
            t.record_stream(st)
        return o0, o1

    def build_id(self) -> str:
        return (self.lib.rsik_build_id() or b"").decode()

    # ------------------------------------------------------------------ test hook
    def debug_math(self, op: int, a: torch.Tensor, b: Optional[torch.Tensor] = None):
        """Evaluates the kernels' own elementary functions (csrc/rsik_math.hpp) on device arrays (rsik_debug_math)."""
        n = int(a.numel())
        a = self._dev_f64(a, (n,), "a")
        if b is not None:
            b = self._dev_f64(b, (n,), "b")
        o0 = torch.empty((n,), dtype=_F64, device=self.device)
        o1 = torch.empty((n,), dtype=_F64, device=self.device)
        self._call("rsik_debug_math", int(op), n, _ptr(a), _ptr(b), _ptr(o0), _ptr(o1))
        return o0, o1
