"""SymbolicIK — drop-in for reachy2_symbolic_ik.symbolic_ik.SymbolicIK (symbolic_ik.py:25-863) on MI355X.

Same constructor signature, public attributes, return tuples and state strings as the reference;
every solve runs in the HIP kernels behind include/rsik.h (no CPU path).  The scalar methods
(`is_reachable`, `get_joints`, ...) are batch-of-one calls that keep the reference's per-instance
state semantics in a one-row device state array; the `*_batch` methods are the
MI355X-native interface for pose batches laid out SoA in HBM.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import numpy.typing as npt
import torch

from . import _abi
from .backend import HipSolver
from .constants import ARM_IDS, STATE_STRINGS, ArmGeometry, default_ik_parameters

_THETA_POLICIES = {"interval0": _abi.THETA_INTERVAL0, "explicit": _abi.THETA_EXPLICIT, "fraction": _abi.THETA_FRACTION,
                   "none": _abi.THETA_NONE}


def poses_to_soa(poses: Any, device: torch.device) -> torch.Tensor:
    """[n,2,3] (position, xyz-euler) or [6,n] -> [6,n] float64 on `device` with unit-stride rows (a column slice of a
    larger SoA batch is passed through as a view: the ABI takes one pointer per column array)."""
    t = poses if isinstance(poses, torch.Tensor) else torch.as_tensor(np.asarray(poses, dtype=np.float64))
    t = t.to(device=device, dtype=torch.float64)
    if t.dim() == 3 and tuple(t.shape[1:]) == (2, 3):
        t = t.reshape(t.shape[0], 6).t()
    elif not (t.dim() == 2 and t.shape[0] == 6):
        raise ValueError("poses must have shape [n,2,3] or [6,n]")
    return t if (t.shape[1] <= 1 or t.stride(1) == 1) else t.contiguous()


def _path_soa(poses: Any, device: Any) -> torch.Tensor:
    """Waypoint-major path poses as SoA [6, T, n]: [T,n,2,3] (position, Euler angles per waypoint), or SoA [6,T,n] as it is."""
    if isinstance(poses, torch.Tensor):
        t = poses.to(device=device, dtype=torch.float64)
    else:
        t = torch.as_tensor(np.asarray(poses, dtype=np.float64)).to(device)
    if t.dim() == 3 and t.shape[0] == 6:
        return t
    if t.dim() == 4 and tuple(t.shape[2:]) == (2, 3):
        return t.reshape(t.shape[0], t.shape[1], 6).permute(2, 0, 1).contiguous()
    raise ValueError("poses must have shape [T,n,2,3] or SoA [6,T,n]")


class SymbolicIK:
    def __init__(
        self,
        arm: str = "r_arm",
        ik_parameters: Dict[str, Any] = {},
        elbow_limit: int = 127,
        wrist_limit: np.float64 = np.float64(42.5),
        projection_margin: float = 1e-8,
        backward_limit: float = 0.02,
        normal_vector_margin: float = 1e-7,
        singularity_offset: float = 0.03,
        singularity_limit_coeff: float = 1.0,
        device: Any = None,
        solver: Optional[HipSolver] = None,
    ) -> None:
        if ik_parameters == {}:
            print("Using default parameters")
            ik_parameters = default_ik_parameters()
        self._geom = ArmGeometry(arm, ik_parameters, elbow_limit, wrist_limit, projection_margin, backward_limit,
                                 normal_vector_margin, singularity_offset, singularity_limit_coeff)
        g = self._geom
        # public attributes of the reference (symbolic_ik.py:55-83)
        self.arm = arm
        self.shoulder_position = g.shoulder_position
        self.shoulder_orientation_offset = g.shoulder_orientation_offset
        self.upper_arm_size = g.upper_arm_size
        self.forearm_size = g.forearm_size
        self.tip_position = g.tip_position
        self.gripper_size = g.gripper_size
        self.max_arm_length = g.max_arm_length
        self.torso_pose = np.array([0.0, 0.0, 0.0])
        self.projection_margin = projection_margin
        self.normal_vector_margin = normal_vector_margin
        self.backward_limit = backward_limit
        self.elbow_limit = elbow_limit
        self.shoulder_wrist_min_distance = g.shoulder_wrist_min_distance
        self.wrist_limit = wrist_limit
        self.singularity_offset = singularity_offset
        self.singularity_limit_coeff = singularity_limit_coeff
        self.elbow_singularity_position = g.elbow_singularity_position
        self.wrist_singularity_position = g.wrist_singularity_position

        self.arm_id = ARM_IDS[arm]
        self.consts = g.pack()
        self._solver = solver if solver is not None else HipSolver(device)
        self._solver.set_arm(self.arm_id, self.consts)

    # ------------------------------------------------------------------ scalar drop-in API
    @property
    def solver(self) -> HipSolver:
        return self._solver

    def _upload(self) -> None:
        # several SymbolicIK objects may share one context; make sure *this* arm's constants are current
        self._solver.set_arm(self.arm_id, self.consts)

    # One scalar call = one launch and one stream synchronisation: the kernel reads its arguments from, and keeps this
    # object's row of solver state (which carries the call's results, include/rsik.h RSIK_SOLVER_STATE_STRIDE) in,
    # pinned host memory, which the device addresses directly — no upload, no download (is_reachable 32 -> 23 us,
    # get_elbow_position 27 -> 20 us, get_joints 30 -> 27 us per call against staging copies on both sides).
    def _scalar_io(self):
        io = getattr(self, "_io", None)
        if io is None:
            import ctypes as C

            h_in = torch.empty(8, dtype=torch.float64).pin_memory()
            h_state = torch.zeros(_abi.SOLVER_STATE_STRIDE, dtype=torch.float64).pin_memory()  # one instance = one row
            h_elbow = torch.empty(3, dtype=torch.float64).pin_memory()
            base = h_in.data_ptr()
            io = self._io = {
                "h_in": h_in, "h_in_np": h_in.numpy(), "h_state": h_state, "h_state_np": h_state.numpy(),
                "h_elbow": h_elbow, "h_elbow_np": h_elbow.numpy(),
                "cols": (C.c_void_p * 6)(*[base + 8 * k for k in range(6)]),
                "theta": C.c_void_p(base), "prev": C.c_void_p(base + 8), "state": C.c_void_p(h_state.data_ptr()),
                "elbow": C.c_void_p(h_elbow.data_ptr()),
            }
        return io

    def _finish(self, io) -> np.ndarray:
        torch.cuda.current_stream(self._solver.device).synchronize()
        s = io["h_state_np"]
        self.goal_pose = np.array([s[0:3], s[3:6]])
        self.wrist_position = s[6:9].copy()
        self.intersection_circle = (s[9:12].copy(), float(s[12]), s[13:16].copy())
        return s

    def _reach_scalar(self, goal_pose: Any, no_limits: bool):
        io = self._scalar_io()
        io["h_in_np"][0:3] = goal_pose[0]
        io["h_in_np"][3:6] = goal_pose[1]
        sv = self._solver
        self._upload()
        with torch.cuda.device(sv.device):
            sv._bind_stream()
            sv._check(sv.lib.rsik_reach_state(sv._h, 1, io["cols"], None, self.arm_id, 1 if no_limits else 0, io["state"],
                                              None, None, None))
            s = self._finish(io)
        if int(s[23]) == _abi.STATE_INVALID_INPUT:
            # include/rsik.h "Rows that are not numbers": the batch API reports the row; the scalar drop-in does what the reference
            # does with a NaN in the pose (symbolic_ik.py:580, np.linalg.lstsq on a system full of NaN) — the solver object is untouched
            raise np.linalg.LinAlgError("SVD did not converge in Linear Least Squares")
        return bool(s[22] != 0.0), s[20:22].copy(), int(s[23])

    def is_reachable(self, goal_pose: npt.NDArray[np.float64]) -> Tuple[bool, npt.NDArray[np.float64], Optional[Any], str]:
        """symbolic_ik.py:121-282."""
        ok, interval, code = self._reach_scalar(goal_pose, no_limits=False)
        if not ok:
            return False, np.array([]), None, STATE_STRINGS[code]
        return True, interval, self.get_joints, STATE_STRINGS[code]

    def is_reachable_no_limits(self, goal_pose: npt.NDArray[np.float64]) -> Tuple[bool, npt.NDArray[np.float64], Optional[Any]]:
        """symbolic_ik.py:85-119."""
        ok, interval, _ = self._reach_scalar(goal_pose, no_limits=True)
        if not ok:
            return False, np.array([]), None
        return True, np.array([-np.pi, np.pi]), self.get_joints

    def get_joints(
        self, theta: float, previous_joints: Sequence[float] = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    ) -> Tuple[npt.NDArray[np.float64], npt.NDArray[np.float64]]:
        """symbolic_ik.py:697-863 — reads and (when the elbow projection fires) updates the state left by the
        last is_reachable*() call, exactly like the reference's bound method."""
        io = self._scalar_io()
        io["h_in_np"][0] = theta
        io["h_in_np"][1:8] = previous_joints
        sv = self._solver
        self._upload()
        with torch.cuda.device(sv.device):
            sv._bind_stream()
            sv._check(sv.lib.rsik_joints_from_state(sv._h, 1, io["state"], None, self.arm_id, io["theta"], io["prev"], None, None))
            s = self._finish(io)
        joints = s[24:31].copy()
        if s[19] != 0.0:  # Q2: 3 components after a projection, [x, y, z, 1] otherwise
            self.elbow_position = s[16:19].copy()
        else:
            self.elbow_position = np.array([s[16], s[17], s[18], 1.0])
        return joints, self.elbow_position

    def _theta_from_joints_scalar(self, current_joints: Any, preferred_theta: float) -> Tuple[float, float, float]:
        """utils.get_best_theta_to_current_joints on this object's state row, one launch (rsik_theta_from_joints_state): the
        row, and with it goal_pose / wrist_position / elbow_position, end up as the reference's ~35 get_joints calls leave them.
        current_joints: 7 values, or the two lists of 7 that ControlIK.__init__ hands over (Q15).  Returns (theta, low, high);
        low and high are NaN when the preferred theta itself matched."""
        cj = np.asarray(current_joints, dtype=np.float64)
        if cj.shape not in ((7,), (2, 7)):
            raise ValueError("current_joints must hold 7 joints, or two lists of 7 (the constructor's form)")
        io = self._scalar_io()
        tj = io.get("tj")
        if tj is None:
            import ctypes as C

            tj = io["tj"] = torch.zeros(14 + 3, dtype=torch.float64).pin_memory()
            io["tj_np"] = tj.numpy()
            io["tj_cur"], io["tj_theta"], io["tj_bracket"] = (C.c_void_p(tj.data_ptr()), C.c_void_p(tj.data_ptr() + 8 * 14),
                                                              C.c_void_p(tj.data_ptr() + 8 * 15))
            io["tj_pref"] = np.zeros(2)
            io["tj_pref_p"] = io["tj_pref"].ctypes.data_as(C.POINTER(C.c_double))
        io["tj_np"][:cj.size] = cj.reshape(-1)
        io["tj_pref"][:] = preferred_theta
        sv = self._solver
        self._upload()
        with torch.cuda.device(sv.device):
            sv._bind_stream()
            sv._check(sv.lib.rsik_theta_from_joints_state(
                sv._h, 1, io["state"], None, self.arm_id, io["tj_cur"], int(cj.size),
                io["tj_pref_p"], io["tj_theta"], io["tj_bracket"]))
            s = self._finish(io)
        self.elbow_position = s[16:19].copy() if s[19] != 0.0 else np.array([s[16], s[17], s[18], 1.0])
        o = io["tj_np"]
        return float(o[14]), float(o[15]), float(o[16])

    def get_elbow_position(self, theta: float) -> npt.NDArray[np.float64]:
        """symbolic_ik.py:684-695."""
        io = self._scalar_io()
        io["h_in_np"][0] = theta
        sv = self._solver
        with torch.cuda.device(sv.device):
            sv._bind_stream()
            sv._check(sv.lib.rsik_elbow_from_state(sv._h, 1, io["state"], io["theta"], io["elbow"]))
            torch.cuda.current_stream(sv.device).synchronize()
        e = io["h_elbow_np"]
        return np.array([e[0], e[1], e[2], 1.0])

    # ---- the stages of is_reachable as public methods (the reference's own harness times them one by one,
    # src/benchmark/ik_benchmarks.py:36-130): each is one rsik_stage launch on the operands it is given — the fused kernels never
    # form these intermediates.  `self.wrist_position` is read where the reference reads it (a caller may assign it).
    def _stage(self, op: int, *operands: Any) -> np.ndarray:
        need_in, need_out = _abi.STAGE_ROW[op]
        io = getattr(self, "_stage_io", None)
        if io is None:
            io = self._stage_io = {"in": torch.empty((1, _abi.STAGE_IN_MAX), dtype=torch.float64).pin_memory(),
                                   "out": torch.empty((1, _abi.STAGE_OUT_MAX), dtype=torch.float64).pin_memory()}
            io["in_np"], io["out_np"] = io["in"].numpy(), io["out"].numpy()
        flat = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in operands])
        if flat.size != need_in:
            raise ValueError(f"stage {op} takes {need_in} numbers, got {flat.size}")
        io["in_np"][0, :need_in] = flat
        sv = self._solver
        self._upload()
        with torch.cuda.device(sv.device):
            sv._bind_stream()
            sv._check(sv.lib.rsik_stage(sv._h, int(op), 1, self.arm_id, io["in"].data_ptr(), _abi.STAGE_IN_MAX, io["out"].data_ptr(), _abi.STAGE_OUT_MAX))
            torch.cuda.current_stream(sv.device).synchronize()
        return io["out_np"][0, :need_out].copy()

    def is_pose_in_robot_reach(self, goal_pose: npt.NDArray[np.float64]) -> Tuple[bool, npt.NDArray[np.float64], str]:
        """symbolic_ik.py:284-307."""
        o = self._stage(_abi.STAGE_POSE_IN_REACH, goal_pose[0], goal_pose[1])
        code = int(o[4])
        return bool(o[0] != 0.0), np.array([o[1:4], np.asarray(goal_pose[1], dtype=np.float64)]), STATE_STRINGS[code]

    def get_wrist_position(self, goal_pose: npt.NDArray[np.float64]) -> npt.NDArray[np.float64]:
        """symbolic_ik.py:418-425."""
        return self._stage(_abi.STAGE_WRIST_POSITION, goal_pose[0], goal_pose[1])

    def get_limitation_wrist_circle(self, goal_pose: npt.NDArray[np.float64]) -> Tuple[npt.NDArray[np.float64], float, npt.NDArray[np.float64]]:
        """symbolic_ik.py:401-416 (reads self.wrist_position)."""
        o = self._stage(_abi.STAGE_LIMITATION_CIRCLE, self.wrist_position, goal_pose[0])
        return o[0:3], float(o[3]), o[4:7]

    def get_intersection_circle(self, goal_pose: npt.NDArray[np.float64]) -> Optional[Tuple[npt.NDArray[np.float64], float, npt.NDArray[np.float64]]]:
        """symbolic_ik.py:366-399 (reads self.wrist_position; the argument is not looked at, as in the reference)."""
        o = self._stage(_abi.STAGE_INTERSECTION_CIRCLE, self.wrist_position)
        return None if o[0] == 0.0 else (o[1:4], float(o[4]), o[5:8])

    def are_circles_linked(self, intersection_circle: Any, limitation_wrist_circle: Any) -> npt.NDArray[np.float64]:
        """symbolic_ik.py:427-509: the interval of valid elbow angles, or an empty array (reads self.wrist_position)."""
        o = self._stage(_abi.STAGE_CIRCLES_LINKED, self.wrist_position, intersection_circle[0], [intersection_circle[1]], intersection_circle[2],
                        limitation_wrist_circle[0], [limitation_wrist_circle[1]], limitation_wrist_circle[2])
        return np.array([]) if o[0] == 0.0 else o[1:3]

    def points_of_nearest_approach(self, p1: Any, V_torso_normal1: Any, p2: Any, V_torso_normal2: Any) -> Tuple[npt.NDArray[np.float64], npt.NDArray[np.float64]]:
        """symbolic_ik.py:588-606: (a point of, the direction of) the line in which the two circles' planes meet."""
        o = self._stage(_abi.STAGE_NEAREST_APPROACH, p1, V_torso_normal1, p2, V_torso_normal2)
        return (o[1:4] if o[0] != 0.0 else np.array([])), o[4:7]

    def intersection_circle_line_3d_vd(self, center: Any, radius: float, direction: Any, point_on_line: Any) -> Optional[npt.NDArray[np.float64]]:
        """symbolic_ik.py:608-645."""
        o = self._stage(_abi.STAGE_CIRCLE_LINE, center, [radius], direction, point_on_line)
        k = int(o[0])
        return None if k == 0 else (np.array([o[1:4]]) if k == 1 else np.vstack((o[1:4], o[4:7])))

    # ------------------------------------------------------------------ batched API (MI355X-native)
    def solve_batch(
        self,
        poses: Any,
        theta: Any = "interval0",
        previous_joints: Optional[Sequence[float]] = None,
        want_elbow: bool = True,
        out: Optional[Dict[str, torch.Tensor]] = None,
        plan_only: bool = False,
    ) -> Dict[str, torch.Tensor]:
        """Fused is_reachable + get_joints for a batch of poses of this arm.

        poses: [n,2,3] or SoA [6,n].  theta: "interval0" (the reference's README/benchmark convention),
        "none" (reachability only), ("explicit", tensor[n]) or ("fraction", tensor[n]).
        previous_joints: (7,) for every pose, or (n, 7): one get_joints previous_joints per pose (n independent callers in
        one launch, rsik_solve_rows).
        Returns device tensors: joints [n,7], interval [n,2], elbow [n,3], reachable [n] u8, state [n] u8.
        """
        return _solve_batch(self, {"arm_uniform": self.arm_id}, poses, theta, previous_joints, want_elbow, out, plan_only)

    def sweep_batch(self, poses: Any, thetas: Any = None, n_theta: int = 16, policy: str = "fraction",
                    previous_joints: Any = None, want_elbow: bool = True,
                    out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """The arm's redundant degree of freedom sampled for a batch of poses of this arm, in one launch: is_reachable once per
        pose, then the closure it returns (theta_to_joints_func) at K elbow angles — every sample a fresh get_joints on the
        goal asked for, whatever the other samples did (HipSolver.solve_sweep, rsik_solve_sweep).

        poses: [n,2,3] or SoA [6,n].  thetas: [K] shared by every pose, or [K, n]; None: `n_theta` evenly spaced fractions
        from 0 to 1 inclusive (interval[0] ... interval[1]).  policy: "fraction" or "explicit".  previous_joints: (n, 7) or None.
        Returns device tensors, sample-major: joints [K,n,7], elbow [K,n,3], projected [K,n] u8 (1: the elbow projection moved
        the goal, the joints reach the moved goal), theta [K,n], interval [n,2], reachable [n] u8, state [n] u8.
        joints.permute(1, 0, 2) is the per-pose view [n,K,7]."""
        return _sweep_batch(self, {"arm_uniform": self.arm_id}, poses, thetas, n_theta, policy, previous_joints, want_elbow, out)

    def nearest_batch(self, poses: Any, seed_joints: Any, n_theta: int = 64, thetas: Any = None, policy: str = "fraction",
                      weights: Optional[Sequence[float]] = None, skip_projected: bool = False, previous_joints: Any = None,
                      want_elbow: bool = True, out: Optional[Dict[str, torch.Tensor]] = None,
                      plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """For every pose of this arm, the elbow angle — of K sampled ones — whose solution is nearest to that row's seed joints,
        in one launch: sweep_batch's samples, judged on the device, one row per pose back (HipSolver.solve_nearest,
        rsik_solve_nearest).  What a planner or a trajectory optimiser asks with the joints it has.

        poses: [n,2,3] or SoA [6,n].  seed_joints: [n,7].  thetas: [K] shared by every pose, or [K, n]; None: `n_theta` evenly
        spaced fractions from 0 to 1 inclusive, as sweep_batch.  policy: "fraction" or "explicit".  weights: 7 values >= 0 for the
        squared joint differences (None: ones).  skip_projected: samples whose elbow projection moved the goal cannot win.
        Returns device tensors: index [n] int32 (-1: no candidate), theta [n], joints [n,7], elbow [n,3], projected [n] u8,
        cost [n], interval [n,2], reachable [n] u8, state [n] u8."""
        return _nearest_batch(self, {"arm_uniform": self.arm_id}, poses, seed_joints, n_theta, thetas, policy, weights, skip_projected,
                              previous_joints, want_elbow, out, plan_only)

    def path_batch(self, poses: Any, start_joints: Any = None, n_theta: int = 16, thetas: Any = None, policy: str = "fraction",
                   weights: Optional[Sequence[float]] = None, skip_projected: bool = False, unwind: bool = False,
                   want_elbow: bool = True, out: Optional[Dict[str, torch.Tensor]] = None,
                   plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """For n paths of T waypoints of this arm, the sequence of elbow angles — one of K sampled ones per waypoint — along which
        the joints move least, in one launch: sweep_batch's samples at every waypoint, the best way through them found on the
        device (HipSolver.solve_path, rsik_solve_path).  Not the greedy chain of nearest_batch calls: the optimum over all K ^ T.

        poses: [T,n,2,3] or SoA [6,T,n], waypoint-major.  start_joints: [n,7] or None.  thetas: [K] shared by every waypoint, or
        [K,T,n]; None: `n_theta` evenly spaced fractions from 0 to 1 inclusive; K <= 64.  policy: "fraction" or "explicit".
        weights: 7 values >= 0 (None: ones).  skip_projected: samples whose elbow projection moved the goal cannot win.  unwind:
        joints continuous along the path (allow_multiturn against the row before).
        Returns device tensors: index [T, n] int32 (-1: a waypoint without a candidate, skipped), theta [T,n], joints [T,n,7],
        elbow [T,n,3], projected [T,n] u8, step_cost [T,n], cost [n], n_solved [n] int32, interval [T,n,2], reachable [T,n] u8,
        state [T,n] u8."""
        return _path_batch(self, {"arm_uniform": self.arm_id}, poses, start_joints, n_theta, thetas, policy, weights, skip_projected,
                           unwind, want_elbow, out, plan_only)

    def path_clear_batch(self, poses: Any, start_joints: Any = None, spheres: Any = None, capsules: Any = None, link_radius: Any = None,
                         min_clearance: float = -float("inf"), influence: float = 0.0, clearance_gain: float = 0.0, n_theta: int = 16,
                         thetas: Any = None, policy: str = "fraction", weights: Optional[Sequence[float]] = None,
                         skip_projected: bool = False, unwind: bool = False, want_elbow: bool = True,
                         out: Optional[Dict[str, torch.Tensor]] = None, plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """path_batch among obstacles, in one launch (HipSolver.solve_path_clear, rsik_solve_path_clear): the least-motion sequence
        of elbow angles among the samples whose arm stays at least min_clearance (m; -inf: no constraint) away from the static
        scene spheres [S,4] (S <= 256), capsules [Cp,7] (Cp <= 64) with link_radius (3 values), clearance_batch's obstacle
        arguments, at least one obstacle in all.  A sample nearer than influence (m) adds clearance_gain (influence - d)^2 to the
        cost of the paths through it.  Every other argument is path_batch's.
        Returns path_batch's tensors and clearance [T,n], nearest [T,n,2] int32 — clearance_batch's for the returned joints — and
        blocked [T,n] u8, the samples of a waypoint that only the constraint excluded."""
        return _path_clear_batch(self, {"arm_uniform": self.arm_id}, poses, start_joints, spheres, capsules, link_radius, min_clearance,
                                 influence, clearance_gain, n_theta, thetas, policy, weights, skip_projected, unwind, want_elbow, out,
                                 plan_only)

    def reach_map_batch(self, positions: Any, orientations: Any, want: Sequence[str] = HipSolver.REACH_MAP_OUTPUTS,
                        out: Optional[Dict[str, torch.Tensor]] = None, plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """A reachability map (capability map) of this arm in one launch: every position with every orientation of one set,
        is_reachable per pair, reduced per position on the device — a few bytes back per position instead of a row per pose
        (HipSolver.reach_map, rsik_reach_map).  Pose (i, j) is judged bit for bit as solve_batch(theta="none") judges it.

        positions: [n_pos,3] or SoA [3,n_pos].  orientations: [n_rot,3] or SoA [3,n_rot] (roll, pitch, yaw), 1 ... 4096 of them.
        want: which outputs to compute.
        Returns device tensors, one row per position: count [n_pos] int32 (reachable orientations), state_count [n_pos,11] int32
        (orientations per state code), theta_measure [n_pos] (summed interval width of the reachable ones: elbow freedom left),
        mask [n_pos, ceil(n_rot/64)] int64 (bit j % 64 of word j // 64: pose (i, j) reachable; unpack_reach_mask gives the
        bool [n_pos,n_rot] view).  The parallelism comes from the positions: few positions with many orientations are not fast."""
        return _reach_map_batch(self, {"arm_uniform": self.arm_id}, positions, orientations, want, out, plan_only)

    def theta_from_joints_batch(self, poses: Any, current_joints: Any, preferred_theta: Optional[float] = None,
                                out: Optional[Dict[str, torch.Tensor]] = None, plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """For every row, the theta whose solution is closest to that row's measured joints: is_reachable_no_limits(pose),
        then utils.get_best_theta_to_current_joints — what a caller does before it starts or restarts an arm, for n arms in
        one launch.  poses: [n,2,3] or SoA [6,n] (the pose each arm is in); current_joints: [n,7]; preferred_theta: tried
        first (default: ControlIK's for this arm, -4 pi / 6 for r and its mirror image for l).
        Returns device tensors theta [n], joints [n,7], bracket [n,2], distance [n], state [n] u8 (HipSolver.theta_from_joints)."""
        if preferred_theta is None:
            preferred_theta = default_preferred_theta(self.arm_id)
        return _theta_from_joints_batch(self, {"arm_uniform": self.arm_id}, poses, current_joints, [float(preferred_theta)] * 2, out, plan_only)

    def is_reachable_batch(self, poses: Any) -> Dict[str, torch.Tensor]:
        return self.solve_batch(poses, theta="none")

    def solve_batch_host(self, poses_soa_host: Any, chunk: Optional[int] = None, slots: int = 3,
                         out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """solve_batch for a batch that lives in HOST memory (what a caller of the reference's NumPy API has).
        poses_soa_host: [6,n] float64 (pinned memory gives the full PCIe rate: torch.Tensor.pin_memory()).  Returns HOST
        tensors (pinned): joints [n,7], interval [n,2], reachable [n], state [n] (theta = interval[0]).

        chunk = None: one upload, one launch, one download.  With a chunk size the batch is cut into chunks whose
        upload / solve / download are queued round-robin on `slots` HIP streams (device buffers of `chunk` poses instead
        of n).  Measured on MI355X (scripts/host_pipeline.py, 4 M poses, pinned): 0.455 G solves/s either way — the
        122 B/pose cross PCIe at 55 GB/s in total, uploads and downloads do not overlap each other on this platform, and
        the kernel is 60x faster than the link; chunks of 1 M / 256 k / 64 k poses cost 6 / 17 / 35 % in launch overhead."""
        dev = self._solver.device
        src = poses_soa_host if isinstance(poses_soa_host, torch.Tensor) else torch.as_tensor(np.asarray(poses_soa_host, dtype=np.float64))
        if src.dim() != 2 or src.shape[0] != 6 or src.dtype != torch.float64 or src.is_cuda:
            raise ValueError("poses_soa_host must be a host float64 tensor/array of shape [6, n]")
        n = int(src.shape[1])
        if out is None:
            out = {
                "joints": torch.empty((n, 7), dtype=torch.float64).pin_memory(),
                "interval": torch.empty((n, 2), dtype=torch.float64).pin_memory(),
                "reachable": torch.empty((n,), dtype=torch.uint8).pin_memory(),
                "state": torch.empty((n,), dtype=torch.uint8).pin_memory(),
            }
        if n == 0:
            return out
        chunk = n if chunk is None else max(1, min(int(chunk), n))
        self._upload()
        cache = getattr(self, "_host_pipeline", None)
        if cache is None or cache["chunk"] != chunk or len(cache["slots"]) != slots:
            cache = {"chunk": chunk, "slots": [
                {"stream": torch.cuda.Stream(device=dev),
                 "in": torch.empty((6, chunk), dtype=torch.float64, device=dev),
                 "joints": torch.empty((chunk, 7), dtype=torch.float64, device=dev),
                 "interval": torch.empty((chunk, 2), dtype=torch.float64, device=dev),
                 "reachable": torch.empty((chunk,), dtype=torch.uint8, device=dev),
                 "state": torch.empty((chunk,), dtype=torch.uint8, device=dev)} for _ in range(slots)]}
            self._host_pipeline = cache
        start = torch.cuda.current_stream(dev).record_event()
        for k, a in enumerate(range(0, n, chunk)):
            b = min(a + chunk, n)
            m = b - a
            sl = cache["slots"][k % slots]
            with torch.cuda.stream(sl["stream"]):
                if k < slots:
                    sl["stream"].wait_event(start)
                for c in range(6):  # one contiguous copy per column (a strided [6, m] copy is staged through pageable memory)
                    sl["in"][c, :m].copy_(src[c, a:b], non_blocking=True)
                dev_out = {key: sl[key][:m] for key in ("joints", "interval", "reachable", "state")}
                self._solver.solve(sl["in"][:, :m] if m == chunk else sl["in"][:, :m].contiguous(), arm_uniform=self.arm_id,
                                   theta_policy=_THETA_POLICIES["interval0"], want_elbow=False, out=dev_out)
                for key in ("joints", "interval", "reachable", "state"):
                    out[key][a:b].copy_(dev_out[key], non_blocking=True)
        for sl in cache["slots"]:
            torch.cuda.current_stream(dev).wait_stream(sl["stream"])
        torch.cuda.current_stream(dev).synchronize()
        return out

    def forward_kinematics_batch(self, joints: Any):
        """joints [n,7] -> (goal position [n,3], goal rotation [n,3,3]): the chain get_joints inverts
        (symbolic_ik.py:728-848).  The reference itself has no FK; this is the on-device self-check of SURVEY 8 f-4."""
        self._upload()
        j = torch.as_tensor(joints, dtype=torch.float64).to(self._solver.device)
        return self._solver.forward_kinematics(j.reshape(-1, 7).contiguous(), arm_uniform=self.arm_id)

    def jacobian_batch(self, joints: Any, want: Sequence[str] = HipSolver.JACOBIAN_OUTPUTS,
                       out: Optional[Dict[str, torch.Tensor]] = None, plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """How this arm's goal frame moves when its joints move, in one launch (HipSolver.jacobian, rsik_jacobian).
        joints: [n,7], or [K,n,7] as sweep_batch and path_batch return them (judged in place), in the convention solve_batch returns
        and forward_kinematics_batch reads.  want: which outputs to compute; the bits of one do not depend on the others.
        Returns device tensors:
        jacobian [...,6,7]: column k is the velocity of the goal frame per unit rate of joint k in the torso frame; rows 0-2 are
        d position / d q_k of the position forward_kinematics_batch returns (the goal-frame origin, tip offset included, not the
        wrist), rows 3-5 the angular velocity w_k, d R / d q_k = [w_k]x R; the signs are those of the caller's joint convention.
        null_vector [...,7]: the signed minors of J, null[i] = (-1)^i det(J without column i) — the generalised cross product of J's
        six rows: J . null = 0, the sign is defined and the vector is continuous in the joints; it is not normalised and is the
        zero vector at a singularity.  Away from singularities, where neither the elbow projection nor the elbow-limit clamp is
        active, it is parallel to d joints / d theta of solve_batch: the arm's self-motion.
        manipulability [...]: sqrt(sum null[i]^2) = sqrt(det(J J^T)), Yoshikawa's measure, without forming J J^T; 0, not NaN, at a
        singular row such as a straight elbow (joints[3] == 0).
        A row with a NaN or an infinity among its joints is NaN in every output; a finite angle of any size is answered like the
        angle of [-pi, pi] it is congruent to."""
        return _jacobian_batch(self, {"arm_uniform": self.arm_id}, joints, want, out, plan_only)

    def joint_rates_batch(self, joints: Any, twist: Any, damping: Any, bias_rates: Any = None, want: Sequence[str] = ("rates",),
                          out: Optional[Dict[str, torch.Tensor]] = None, plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """The joint rates that give this arm's goal frame the twist [...,6] (linear velocity of the goal-frame origin, then angular
        velocity, torso frame: the row order of jacobian_batch's J), in one launch (HipSolver.joint_rates, rsik_joint_rates).
        joints: [n,7] or [K,n,7] as jacobian_batch takes them; damping: lambda > 0, a float or a tensor [...] with one per row;
        bias_rates: [...,7] or None for zeros, the rates q0 the arm would like to have, e.g. k * null_vector.
        Per row, rates [...,7] minimises |J q' - twist|^2 + lambda^2 |q' - q0|^2: rates = q0 + J^T y with
        (J J^T + lambda^2 I) y = twist - J q0, solved by L D L^T in natural order with every pivot clamped from below at lambda^2
        (the pivot clamp changes no exact result and keeps a finite row finite at a straight elbow).  achieved_twist [...,6] =
        J . rates.  want: which of the two to compute; the bits of one do not depend on the other.  A row with a NaN or an infinity
        in joints, twist or bias, or a lambda that is NaN, infinite or <= 0, is NaN in every output."""
        return _joint_rates_batch(self, {"arm_uniform": self.arm_id}, joints, twist, damping, bias_rates, want, out, plan_only)

    def track_batch(self, goals: Any, start_joints: Any, dt: float, kp: float, ko: float, damping: Any, feedforward: Any = None,
                    rest_joints: Any = None, rest_gain: float = 0.0, limits: Any = None, want: Sequence[str] = ("joints",),
                    out: Optional[Dict[str, torch.Tensor]] = None, plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """This arm follows n goal trajectories over T steps in closed loop, every step in one launch (HipSolver.track, rsik_track).
        goals: [T,12,n] (R row-major, then t: what control_continuous_run takes) or matrices [T,n,4,4]; start_joints [n,7]: any
        joints.  Per step: forward kinematics, e_p = p_g - p and e_o the rotation vector of R_g R^T, the twist
        feedforward[t] + (kp e_p, ko e_o), the rates of joint_rates_batch for it with bias rest_gain (rest_joints - q), one common
        factor so that no rate exceeds limits[0], q := q + dt q' clamped to [limits[1], limits[2]].  Returns the outputs named in
        want, of HipSolver.TRACK_OUTPUTS: joints [T,n,7], rates [T,n,7], err [T,n,2] (m, rad; what each step saw before it moved),
        final_joints [n,7], final_err [n,2].  Where solve_batch answers NaN (a goal out of reach, the wrist limit) the loop goes as
        near as the damping lets it; a step whose goal is not numbers is skipped."""
        return _track_batch(self, {"arm_uniform": self.arm_id}, goals, start_joints, dt, kp, ko, damping, feedforward, rest_joints,
                            rest_gain, limits, want, out, plan_only)

    def track_avoid_batch(self, goals: Any, start_joints: Any, dt: float, kp: float, ko: float, damping: Any, spheres: Any = None,
                          capsules: Any = None, link_radius: Any = None, influence: float = 0.0, avoid_gain: float = 0.0,
                          feedforward: Any = None, rest_joints: Any = None, rest_gain: float = 0.0, limits: Any = None,
                          want: Sequence[str] = ("joints",), out: Optional[Dict[str, torch.Tensor]] = None,
                          plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """track_batch with obstacle avoidance inside the loop, every step in one launch (HipSolver.track_avoid, rsik_track_avoid).
        goals, start_joints, dt, kp, ko, damping, feedforward, rest_joints, rest_gain and limits are track_batch's; spheres [S,4]
        (S <= 256), capsules [Cp,7] (Cp <= 64) and link_radius are clearance_batch's, static, at least one in all.  Per step the
        clearance d of the current joints and its gradient g are clearance_batch's, and where d < influence the bias of the rates
        gains avoid_gain (influence - d) g: the arm moves away in the null space of the task.  Returns the outputs named in want, of
        HipSolver.TRACK_AVOID_OUTPUTS: track_batch's five, clearance [T,n] and nearest [T,n,2] int32 (what each step saw before it
        moved) and min_clearance [n] (over the steps and at the final joints)."""
        return _track_avoid_batch(self, {"arm_uniform": self.arm_id}, goals, start_joints, dt, kp, ko, damping, spheres, capsules,
                                  link_radius, influence, avoid_gain, feedforward, rest_joints, rest_gain, limits, want, out, plan_only)

    def clearance_batch(self, joints: Any, spheres: Any = None, capsules: Any = None, link_radius: Any = None,
                        want: Sequence[str] = ("clearance", "nearest"), out: Optional[Dict[str, torch.Tensor]] = None,
                        plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """How far this arm is from a set of obstacles, in one launch (HipSolver.clearance, rsik_clearance).  The arm is three
        capsules (shoulder -> elbow -> wrist -> goal origin) of the radii link_radius (3 values, None for zeros); joints: [n,7], or
        [K,n,7] as sweep_batch and path_batch return them (judged in place); spheres [S,4] rows (x, y, z, r), capsules [Cp,7] rows
        (a, b, r), in the torso frame, shared by every row, at least one in all.  Returns the outputs named in want, of
        HipSolver.CLEARANCE_OUTPUTS: clearance [...] (axis distance minus both radii of the nearest pair, negative inside),
        nearest [...,2] int32 (link, obstacle index; capsule j is S + j), witness [...,2,3] (the point on the link's axis and the point
        on the obstacle's), gradient [...,7] (d clearance / d joints of that pair, zero where the axes touch; k * gradient is a
        bias_rates for joint_rates_batch and track_batch), link_points [...,4,3] (shoulder, elbow, wrist, goal origin).  A row of
        joints that is not numbers is NaN with nearest (-1, -1); an obstacle that is not numbers or has a negative radius is skipped."""
        return _clearance_batch(self, {"arm_uniform": self.arm_id}, joints, spheres, capsules, link_radius, want, out, plan_only)

    def clearance_edges_batch(self, joints: Any, start_joints: Any = None, n_sub: int = 16, spheres: Any = None, capsules: Any = None,
                              link_radius: Any = None, min_clearance: float = -float("inf"), want: Optional[Sequence[str]] = None,
                              out: Optional[Dict[str, torch.Tensor]] = None, plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """The clearance of this arm ALONG the motion between the waypoints of n paths, in one call (HipSolver.clearance_edges,
        rsik_clearance_edges): path_clear_batch keeps min_clearance at the waypoints only.  joints: [T,n,7] as path_batch and
        path_clear_batch return them (in place; a NaN row is a skipped waypoint, bridged), start_joints [n,7] or None, n_sub: the
        sub-steps S per edge, 1 ... 256; spheres, capsules, link_radius as path_clear_batch.  Every edge is sampled at
        a + angle_diff(b, a) * (s / S), s = 0 ... S.  Returns the outputs named in want (None: all of
        HipSolver.CLEARANCE_EDGES_OUTPUTS): edge_clearance [T,n] (the least clearance_batch `clearance` over the samples), edge_sub
        [T,n] int32 (the s that attains it), edge_nearest [T,n,2] int32 (link, obstacle index), edge_bound [T,n] (a certified lower
        bound on the clearance of the whole continuous motion: above 0 the edge is proven free), and per path path_clearance [n],
        path_edge [n,2] int32 (t, s), path_bound [n], n_below [n] int32 (edges with edge_clearance < min_clearance) and first_below
        [n] int32 (the first such t, or -1)."""
        return _clearance_edges_batch(self, {"arm_uniform": self.arm_id}, joints, start_joints, n_sub, spheres, capsules, link_radius,
                                      min_clearance, want, out, plan_only)

    def fk_residual_batch(self, poses: Any, joints: Any) -> torch.Tensor:
        """err [n,2] = (position error m, rotation error rad) of FK(joints) against the poses they were solved for."""
        self._upload()
        soa = poses_to_soa(poses, self._solver.device)
        j = torch.as_tensor(joints, dtype=torch.float64).to(self._solver.device)
        return self._solver.fk_residual(soa, j.reshape(-1, 7).contiguous(), arm_uniform=self.arm_id)

    @staticmethod
    def state_strings(codes: Any) -> list:
        c = codes.cpu().numpy() if isinstance(codes, torch.Tensor) else np.asarray(codes)
        return [STATE_STRINGS[int(k)] for k in c]


def default_preferred_theta(arm_id: int) -> float:
    """ControlIK.preferred_theta of an arm (control_ik.py:133-139): -4 pi / 6 for r, -pi + 4 pi / 6 for l."""
    base = -4 * np.pi / 6
    return base if arm_id == 0 else -np.pi - base


def _split_previous_joints(previous_joints: Any):
    """solve_batch's previous_joints: None or (7,) -> the launch-uniform vector; a 2-D (n, 7) array -> one row per pose
    (the backend checks n and raises ValueError before anything is launched).  Returns (uniform, rows)."""
    if previous_joints is None:
        return None, None
    shape = tuple(previous_joints.shape) if hasattr(previous_joints, "shape") else np.shape(previous_joints)
    if len(shape) == 2:
        return None, previous_joints
    return previous_joints, None


# ---- the batch methods of SymbolicIK and DualArmIK: one implementation each.  `ik` is either object (its solver, its _upload());
# `arm` is what tells the backend whose rows these are: {"arm_uniform": id} for one arm, {"arm": arm_ids} for rows of both.
def _default_grid(thetas: Any, n_theta: int, single: Optional[float]) -> Any:
    """The caller's thetas, or `n_theta` evenly spaced fractions from 0 to 1 inclusive.  `single`: what stands for a grid of fewer
    than two samples (path_batch: the middle of the interval); None: linspace's own answer (sweep_batch, nearest_batch)."""
    if thetas is not None:
        return thetas
    if single is None or int(n_theta) > 1:
        return torch.linspace(0.0, 1.0, int(n_theta), dtype=torch.float64)
    return torch.tensor([single], dtype=torch.float64)


def _solve_batch(ik, arm, poses, theta, previous_joints, want_elbow, out, plan_only):
    soa = poses_to_soa(poses, ik._solver.device)
    name, theta_in = (theta, None) if isinstance(theta, str) else (theta[0], theta[1])  # a policy name, or (name, tensor[n])
    policy = _THETA_POLICIES[name]
    ik._upload()
    previous_joints, rows = _split_previous_joints(previous_joints)
    return ik._solver.solve(soa, theta_policy=policy, theta_in=theta_in, previous_joints=previous_joints, want_elbow=want_elbow,
                            out=out, plan_only=plan_only, previous_joints_rows=rows, **arm)


def _sweep_batch(ik, arm, poses, thetas, n_theta, policy, previous_joints, want_elbow, out):
    soa = poses_to_soa(poses, ik._solver.device)
    thetas = _default_grid(thetas, n_theta, None)
    ik._upload()
    return ik._solver.solve_sweep(soa, thetas, policy=policy, previous_joints=previous_joints, want_elbow=want_elbow, out=out, **arm)


def _nearest_batch(ik, arm, poses, seed_joints, n_theta, thetas, policy, weights, skip_projected, previous_joints, want_elbow, out,
                   plan_only):
    soa = poses_to_soa(poses, ik._solver.device)
    thetas = _default_grid(thetas, n_theta, None)
    ik._upload()
    return ik._solver.solve_nearest(soa, thetas, seed_joints, policy=policy, weights=weights, skip_projected=skip_projected,
                                    previous_joints=previous_joints, want_elbow=want_elbow, out=out, plan_only=plan_only, **arm)


def _path_batch(ik, arm, poses, start_joints, n_theta, thetas, policy, weights, skip_projected, unwind, want_elbow, out, plan_only):
    soa = _path_soa(poses, ik._solver.device)
    thetas = _default_grid(thetas, n_theta, 0.5)
    ik._upload()
    return ik._solver.solve_path(soa, thetas, start_joints, policy=policy, weights=weights, skip_projected=skip_projected,
                                 unwind=unwind, want_elbow=want_elbow, out=out, plan_only=plan_only, **arm)


def _path_clear_batch(ik, arm, poses, start_joints, spheres, capsules, link_radius, min_clearance, influence, clearance_gain, n_theta,
                      thetas, policy, weights, skip_projected, unwind, want_elbow, out, plan_only):
    soa = _path_soa(poses, ik._solver.device)
    thetas = _default_grid(thetas, n_theta, 0.5)
    ik._upload()
    return ik._solver.solve_path_clear(soa, thetas, start_joints, spheres=spheres, capsules=capsules, link_radius=link_radius,
                                       min_clearance=min_clearance, influence=influence, clearance_gain=clearance_gain, policy=policy,
                                       weights=weights, skip_projected=skip_projected, unwind=unwind, want_elbow=want_elbow, out=out,
                                       plan_only=plan_only, **arm)


def _xyz_soa(rows: Any, device: Any, name: str) -> torch.Tensor:
    """[n,3] rows or SoA [3,n] -> SoA [3,n] float64 on the device (a [3,3] input is taken as rows)."""
    t = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(np.asarray(rows, dtype=np.float64))
    t = t.to(device=device, dtype=torch.float64)
    if t.dim() != 2 or 3 not in t.shape:
        raise ValueError(f"{name} must have shape [n,3] or [3,n]")
    return t.t().contiguous() if t.shape[1] == 3 else t


def _reach_map_batch(ik, arm, positions, orientations, want, out, plan_only):
    pos = _xyz_soa(positions, ik._solver.device, "positions")
    eul = _xyz_soa(orientations, ik._solver.device, "orientations")
    ik._upload()
    return ik._solver.reach_map(pos, eul, want=want, out=out, plan_only=plan_only, **arm)


def _jacobian_batch(ik, arm, joints, want, out, plan_only):
    ik._upload()
    return ik._solver.jacobian(joints, want=want, out=out, plan_only=plan_only, **arm)


def _joint_rates_batch(ik, arm, joints, twist, damping, bias_rates, want, out, plan_only):
    ik._upload()
    return ik._solver.joint_rates(joints, twist, damping=damping, bias_rates=bias_rates, want=want, out=out, plan_only=plan_only, **arm)


def _track_batch(ik, arm, goals, start_joints, dt, kp, ko, damping, feedforward, rest_joints, rest_gain, limits, want, out, plan_only):
    g = goals if isinstance(goals, torch.Tensor) else torch.as_tensor(np.asarray(goals, dtype=np.float64))
    g = g.to(device=ik._solver.device, dtype=torch.float64)
    if g.dim() == 4 and tuple(g.shape[2:]) == (4, 4):  # [T,n,4,4] -> [T,12,n]
        g = torch.cat([g[..., :3, :3].reshape(g.shape[0], g.shape[1], 9), g[..., :3, 3]], dim=2).permute(0, 2, 1).contiguous()
    ik._upload()
    return ik._solver.track(g, start_joints, dt, kp, ko, damping=damping, feedforward=feedforward, rest_joints=rest_joints,
                            rest_gain=rest_gain, limits=limits, want=want, out=out, plan_only=plan_only, **arm)


def _track_avoid_batch(ik, arm, goals, start_joints, dt, kp, ko, damping, spheres, capsules, link_radius, influence, avoid_gain,
                       feedforward, rest_joints, rest_gain, limits, want, out, plan_only):
    g = goals if isinstance(goals, torch.Tensor) else torch.as_tensor(np.asarray(goals, dtype=np.float64))
    g = g.to(device=ik._solver.device, dtype=torch.float64)
    if g.dim() == 4 and tuple(g.shape[2:]) == (4, 4):  # [T,n,4,4] -> [T,12,n]
        g = torch.cat([g[..., :3, :3].reshape(g.shape[0], g.shape[1], 9), g[..., :3, 3]], dim=2).permute(0, 2, 1).contiguous()
    ik._upload()
    return ik._solver.track_avoid(g, start_joints, dt, kp, ko, damping=damping, spheres=spheres, capsules=capsules,
                                  link_radius=link_radius, influence=influence, avoid_gain=avoid_gain, feedforward=feedforward,
                                  rest_joints=rest_joints, rest_gain=rest_gain, limits=limits, want=want, out=out, plan_only=plan_only,
                                  **arm)


def _m12_steps(goals, device):
    """Goals [T,12,n] or matrices [T,n,4,4] -> [T,12,n] float64 on the device."""
    g = goals if isinstance(goals, torch.Tensor) else torch.as_tensor(np.asarray(goals, dtype=np.float64))
    g = g.to(device=device, dtype=torch.float64)
    if g.dim() == 4 and tuple(g.shape[2:]) == (4, 4):
        g = torch.cat([g[..., :3, :3].reshape(g.shape[0], g.shape[1], 9), g[..., :3, 3]], dim=2).permute(0, 2, 1)
    return g


def _interleave(r, l, dim, device):
    """Two per-arm arrays -> one with row 2 i from r and row 2 i + 1 from l along `dim`."""
    r, l = ((t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t, dtype=np.float64))).to(device=device, dtype=torch.float64)
            for t in (r, l))
    if r.shape != l.shape:
        raise ValueError("the right and the left arm's arrays must have the same shape")
    dim = dim % r.dim()
    return torch.stack([r, l], dim=dim + 1).reshape(r.shape[:dim] + (2 * r.shape[dim],) + r.shape[dim + 1:]).contiguous()


def _clearance_batch(ik, arm, joints, spheres, capsules, link_radius, want, out, plan_only):
    ik._upload()
    return ik._solver.clearance(joints, spheres=spheres, capsules=capsules, link_radius=link_radius, want=want, out=out,
                                plan_only=plan_only, **arm)


def _clearance_edges_batch(ik, arm, joints, start_joints, n_sub, spheres, capsules, link_radius, min_clearance, want, out, plan_only):
    ik._upload()
    return ik._solver.clearance_edges(joints, start_joints, n_sub, spheres=spheres, capsules=capsules, link_radius=link_radius,
                                      min_clearance=min_clearance, want=ik._solver.CLEARANCE_EDGES_OUTPUTS if want is None else want,
                                      out=out, plan_only=plan_only, **arm)


def arm_capsules(link_points: torch.Tensor, link_radius: Any = None) -> torch.Tensor:
    """The three capsules [3,7] (a, b, r) of an arm from ONE row of clearance_batch's link_points [4,3] and its link radii (3
    values, None for zeros): what the other arm takes as obstacles.  Stays on link_points' device; nothing waits."""
    p = link_points.reshape(4, 3)
    if link_radius is None:
        r = torch.zeros(3, dtype=p.dtype)
    else:
        r = link_radius if isinstance(link_radius, torch.Tensor) else torch.as_tensor(np.asarray(link_radius, dtype=np.float64))
    return torch.cat([p[:3], p[1:], r.to(device=p.device, dtype=p.dtype).reshape(3, 1)], dim=1)


def unpack_reach_mask(mask: torch.Tensor, n_rot: int) -> torch.Tensor:
    """The `mask` of reach_map_batch / HipSolver.reach_map, [n_pos, ceil(n_rot/64)] int64, as a bool tensor [n_pos, n_rot]:
    entry (i, j) is pose (i, j)'s reachable flag."""
    if mask.dim() != 2 or mask.shape[1] != (int(n_rot) + 63) // 64:
        raise ValueError("mask must have shape [n_pos, ceil(n_rot / 64)]")
    bits = torch.arange(64, dtype=torch.int64, device=mask.device)
    return (((mask.unsqueeze(-1) >> bits) & 1) != 0).reshape(mask.shape[0], -1)[:, : int(n_rot)]


def _theta_from_joints_batch(ik, arm, poses, current_joints, preferred_theta, out, plan_only):
    soa = poses_to_soa(poses, ik._solver.device)
    ik._upload()
    return ik._solver.theta_from_joints(soa, current_joints, preferred_theta, out=out, plan_only=plan_only, **arm)


class DualArmIK:
    """Mixed r/l batches in one launch (BASELINE config 4): two SymbolicIK objects sharing one device context, the arm
    of every pose given by a uint8 array (0 = r_arm, 1 = l_arm)."""

    def __init__(self, device: Any = None, solver: Optional[HipSolver] = None, **symbolic_ik_kwargs: Any) -> None:
        self._solver = solver if solver is not None else HipSolver(device)
        self.r_arm = SymbolicIK("r_arm", solver=self._solver, **symbolic_ik_kwargs)
        self.l_arm = SymbolicIK("l_arm", solver=self._solver, **symbolic_ik_kwargs)

    @property
    def solver(self) -> HipSolver:
        return self._solver

    def _upload(self) -> None:
        self.r_arm._upload()
        self.l_arm._upload()

    def solve_batch(self, arm_ids: Any, poses: Any, theta: Any = "interval0", previous_joints: Optional[Sequence[float]] = None,
                    want_elbow: bool = True, out: Optional[Dict[str, torch.Tensor]] = None,
                    plan_only: bool = False) -> Dict[str, torch.Tensor]:
        return _solve_batch(self, {"arm": arm_ids}, poses, theta, previous_joints, want_elbow, out, plan_only)

    def sweep_batch(self, arm_ids: Any, poses: Any, thetas: Any = None, n_theta: int = 16, policy: str = "fraction",
                    previous_joints: Any = None, want_elbow: bool = True,
                    out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """SymbolicIK.sweep_batch for rows of both arms (arm_ids [n] uint8): K elbow angles per pose in one launch.  Returns
        sample-major tensors (joints [K,n,7] ...); joints.permute(1, 0, 2) is the per-pose view [n,K,7]."""
        return _sweep_batch(self, {"arm": arm_ids}, poses, thetas, n_theta, policy, previous_joints, want_elbow, out)

    def nearest_batch(self, arm_ids: Any, poses: Any, seed_joints: Any, n_theta: int = 64, thetas: Any = None, policy: str = "fraction",
                      weights: Optional[Sequence[float]] = None, skip_projected: bool = False, previous_joints: Any = None,
                      want_elbow: bool = True, out: Optional[Dict[str, torch.Tensor]] = None,
                      plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """SymbolicIK.nearest_batch for rows of both arms (arm_ids [n] uint8): of K elbow angles per pose, the one whose solution
        is nearest to the row's seed joints, one row per pose (index [n] int32, theta, joints [n,7] ...)."""
        return _nearest_batch(self, {"arm": arm_ids}, poses, seed_joints, n_theta, thetas, policy, weights, skip_projected,
                              previous_joints, want_elbow, out, plan_only)

    def path_batch(self, arm_ids: Any, poses: Any, start_joints: Any = None, n_theta: int = 16, thetas: Any = None,
                   policy: str = "fraction", weights: Optional[Sequence[float]] = None, skip_projected: bool = False,
                   unwind: bool = False, want_elbow: bool = True, out: Optional[Dict[str, torch.Tensor]] = None,
                   plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """SymbolicIK.path_batch for paths of both arms (arm_ids [n] uint8, one byte per path): the least-motion sequence of elbow
        angles along every path (index [T, n] int32, theta, joints [T,n,7], step_cost, cost [n] ...)."""
        return _path_batch(self, {"arm": arm_ids}, poses, start_joints, n_theta, thetas, policy, weights, skip_projected, unwind,
                           want_elbow, out, plan_only)

    def path_clear_batch(self, arm_ids: Any, poses: Any, start_joints: Any = None, spheres: Any = None, capsules: Any = None,
                         link_radius: Any = None, min_clearance: float = -float("inf"), influence: float = 0.0,
                         clearance_gain: float = 0.0, n_theta: int = 16, thetas: Any = None, policy: str = "fraction",
                         weights: Optional[Sequence[float]] = None, skip_projected: bool = False, unwind: bool = False,
                         want_elbow: bool = True, out: Optional[Dict[str, torch.Tensor]] = None,
                         plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """SymbolicIK.path_clear_batch for paths of both arms (arm_ids [n] uint8, one byte per path): path_batch among the static
        obstacles spheres [S,4] and capsules [Cp,7] of clearance_batch, samples nearer than min_clearance excluded and those nearer
        than influence charged clearance_gain (influence - d)^2; path_batch's tensors and clearance [T,n], nearest [T,n,2] int32,
        blocked [T,n] u8."""
        return _path_clear_batch(self, {"arm": arm_ids}, poses, start_joints, spheres, capsules, link_radius, min_clearance, influence,
                                 clearance_gain, n_theta, thetas, policy, weights, skip_projected, unwind, want_elbow, out, plan_only)

    def reach_map_batch(self, arm_ids: Any, positions: Any, orientations: Any, want: Sequence[str] = HipSolver.REACH_MAP_OUTPUTS,
                        out: Optional[Dict[str, torch.Tensor]] = None, plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """SymbolicIK.reach_map_batch for positions of both arms (arm_ids [n_pos] uint8, one byte per POSITION): every position
        with every orientation, reduced per position (count [n_pos] int32, state_count [n_pos,11], theta_measure, mask)."""
        return _reach_map_batch(self, {"arm": arm_ids}, positions, orientations, want, out, plan_only)

    def jacobian_batch(self, arm_ids: Any, joints: Any, want: Sequence[str] = HipSolver.JACOBIAN_OUTPUTS,
                       out: Optional[Dict[str, torch.Tensor]] = None, plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """SymbolicIK.jacobian_batch for rows of both arms (arm_ids [n] uint8, one byte per row, shared by every repetition of
        joints [K,n,7]): jacobian [...,6,7] (column k: the goal frame's velocity per unit rate of joint k, rows 0-2 d position /
        d q_k, rows 3-5 the angular velocity, torso frame), null_vector [...,7] (the signed minors of J, (-1)^i det(J without column
        i): J . null = 0, signed, continuous, not normalised, zero at a singularity, parallel to d joints / d theta of the solve),
        manipulability [...] (its norm = sqrt(det(J J^T)); 0, not NaN, at a singular row)."""
        return _jacobian_batch(self, {"arm": arm_ids}, joints, want, out, plan_only)

    def joint_rates_batch(self, arm_ids: Any, joints: Any, twist: Any, damping: Any, bias_rates: Any = None,
                          want: Sequence[str] = ("rates",), out: Optional[Dict[str, torch.Tensor]] = None,
                          plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """SymbolicIK.joint_rates_batch for rows of both arms (arm_ids [n] uint8, one byte per row, shared by every repetition of
        joints [K,n,7]): rates [...,7], the minimiser of |J q' - twist|^2 + lambda^2 |q' - q0|^2 (q0 = bias_rates or zero), from
        (J J^T + lambda^2 I) y = twist - J q0 by L D L^T with the pivot clamp at lambda^2, and achieved_twist [...,6] = J . rates."""
        return _joint_rates_batch(self, {"arm": arm_ids}, joints, twist, damping, bias_rates, want, out, plan_only)

    def track_batch(self, arm_ids: Any, goals: Any, start_joints: Any, dt: float, kp: float, ko: float, damping: Any,
                    feedforward: Any = None, rest_joints: Any = None, rest_gain: float = 0.0, limits: Any = None,
                    want: Sequence[str] = ("joints",), out: Optional[Dict[str, torch.Tensor]] = None,
                    plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """SymbolicIK.track_batch for trajectories of both arms (arm_ids [n] uint8, one byte per trajectory): closed-loop tracking of
        goals [T,12,n] from start_joints [n,7] in one launch: joints [T,n,7], rates [T,n,7], err [T,n,2], final_joints [n,7],
        final_err [n,2], as named in want."""
        return _track_batch(self, {"arm": arm_ids}, goals, start_joints, dt, kp, ko, damping, feedforward, rest_joints, rest_gain,
                            limits, want, out, plan_only)

    def track_avoid_batch(self, arm_ids: Any, goals: Any, start_joints: Any, dt: float, kp: float, ko: float, damping: Any,
                          spheres: Any = None, capsules: Any = None, link_radius: Any = None, influence: float = 0.0,
                          avoid_gain: float = 0.0, feedforward: Any = None, rest_joints: Any = None, rest_gain: float = 0.0,
                          limits: Any = None, want: Sequence[str] = ("joints",), out: Optional[Dict[str, torch.Tensor]] = None,
                          plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """SymbolicIK.track_avoid_batch for trajectories of both arms (arm_ids [n] uint8, one byte per trajectory): track_batch with
        the static obstacles spheres [S,4] and capsules [Cp,7] of clearance_batch pushed away from inside the loop (the bias gains
        avoid_gain (influence - clearance) gradient where the clearance is below influence), in one launch: track_batch's outputs, clearance [T,n], nearest [T,n,2] int32 and min_clearance [n], as named in want."""
        return _track_avoid_batch(self, {"arm": arm_ids}, goals, start_joints, dt, kp, ko, damping, spheres, capsules, link_radius,
                                  influence, avoid_gain, feedforward, rest_joints, rest_gain, limits, want, out, plan_only)

    def track_pair_batch(self, goals_r: Any, goals_l: Any, start_r: Any, start_l: Any, dt: float, kp: float, ko: float, damping: Any,
                         spheres: Any = None, capsules: Any = None, link_radius: Any = None, influence: float = 0.0,
                         avoid_gain: float = 0.0, feedforward: Any = None, rest_joints: Any = None, rest_gain: float = 0.0,
                         limits: Any = None, want: Sequence[str] = ("joints",), out: Optional[Dict[str, torch.Tensor]] = None,
                         plan_only: bool = False) -> Dict[str, Any]:
        """Both arms of n_pairs robots tracked in one launch, avoiding each other (HipSolver.track_pair, rsik_track_pair):
        track_avoid_batch in which every arm has, beside the static spheres [S,4] and capsules [Cp,7] (none at all is allowed),
        the other arm's three links as obstacles at every step, at the joints that arm has reached; influence, avoid_gain and
        link_radius as in track_avoid_batch.
        goals_r, goals_l: [T,12,n_pairs] or matrices [T,n_pairs,4,4], per arm; start_r, start_l: [n_pairs,7].  They are interleaved
        (row 2 i the right arm of robot i, row 2 i + 1 its left arm).  With goals_l = None and start_l = None, goals_r and start_r are
        taken as already interleaved arrays of 2 n_pairs rows.  damping, feedforward and rest_joints: a float (damping), an
        interleaved array ([2 n_pairs], [T, 2 n_pairs, 6], [2 n_pairs, 7]), or a pair (right, left) of per-arm arrays.
        Returns HipSolver.TRACK_PAIR_OUTPUTS as named in want — joints, rates [T,n_pairs,7], err [T,n_pairs,2], clearance
        [T,n_pairs], nearest [T,n_pairs,2] int32 (link, obstacle index: S + Cp + l is the partner's link l), final_joints
        [n_pairs,7], final_err [n_pairs,2], min_clearance [n_pairs] — each as {"r": ..., "l": ...}, two strided views of the
        launch's interleaved tensor, which `out` takes as HipSolver.track_pair does.  plan_only adds "launch"."""
        dev = self._solver.device
        if (goals_l is None) != (start_l is None):
            raise ValueError("goals_l and start_l: both per arm, or both None for interleaved goals_r and start_r")
        if goals_l is None:
            goals, start = _m12_steps(goals_r, dev), start_r
        else:
            goals, start = _interleave(_m12_steps(goals_r, dev), _m12_steps(goals_l, dev), 2, dev), _interleave(start_r, start_l, 0, dev)

        def rows(x, dim):
            return _interleave(x[0], x[1], dim, dev) if isinstance(x, (tuple, list)) and len(x) == 2 else x

        self._upload()
        res = self._solver.track_pair(goals.contiguous(), start, dt, kp, ko, damping=rows(damping, 0), spheres=spheres, capsules=capsules,
                                      link_radius=link_radius, influence=influence, avoid_gain=avoid_gain,
                                      feedforward=rows(feedforward, 1), rest_joints=rows(rest_joints, 0), rest_gain=rest_gain,
                                      limits=limits, want=want, out=out, plan_only=plan_only)
        split = {}
        for name, x in res.items():
            if name not in HipSolver.TRACK_PAIR_OUTPUTS:
                split[name] = x
            elif name in ("final_joints", "final_err", "min_clearance"):
                split[name] = {"r": x[0::2], "l": x[1::2]}
            else:
                split[name] = {"r": x[:, 0::2], "l": x[:, 1::2]}
        return split

    def path_pair_batch(self, poses_r: Any, poses_l: Any, start_r: Any = None, start_l: Any = None, spheres: Any = None,
                        capsules: Any = None, link_radius: Any = None, min_clearance: float = -float("inf"), influence: float = 0.0,
                        clearance_gain: float = 0.0, n_theta: int = 8, thetas: Any = None, policy: str = "fraction",
                        weights: Optional[Sequence[float]] = None, skip_projected: bool = False, unwind: bool = False,
                        want_elbow: bool = True, out: Optional[Dict[str, torch.Tensor]] = None,
                        plan_only: bool = False) -> Dict[str, Any]:
        """The elbow angles of both arms of n_pairs robots along two hand paths, chosen together in one launch so that the arms keep
        out of each other (HipSolver.solve_path_pair, rsik_solve_path_pair): path_clear_batch in which every arm has, beside the
        static spheres [S,4] and capsules [Cp,7] (none at all is allowed), the other arm's three links as obstacles, at the sample
        that arm takes at the same waypoint.  A pair of samples nearer than min_clearance in either arm's view is excluded, one
        nearer than influence is charged clearance_gain (influence - d)^2 per view; n_theta <= 16 samples per arm and waypoint.
        poses_r, poses_l: [T,n_pairs,2,3] or SoA [6,T,n_pairs], per arm; start_r, start_l: [n_pairs,7] or None.  They are
        interleaved (row 2 i the right arm of robot i, row 2 i + 1 its left arm).  With poses_l = None, poses_r and start_r are
        taken as already interleaved arrays of 2 n_pairs rows.
        Returns index, theta, joints, elbow, projected, step_cost, interval, reachable, state, clearance and nearest [T,n_pairs,2]
        int32 (link, obstacle index: S + Cp + l is the partner's link l), each as {"r": ..., "l": ...}, two strided views of the
        launch's interleaved tensor, which `out` takes as HipSolver.solve_path_pair does; and per robot cost [n_pairs], n_solved
        [n_pairs] and blocked [T,n_pairs] (the pairs of samples the clearance excludes).  plan_only adds "launch"."""
        dev = self._solver.device
        if poses_l is None:
            if start_l is not None:
                raise ValueError("poses_l and start_l: both per arm, or both None for interleaved poses_r and start_r")
            soa, start = _path_soa(poses_r, dev), start_r
        else:
            if (start_r is None) != (start_l is None):
                raise ValueError("start_r and start_l: both or neither")
            soa = _interleave(_path_soa(poses_r, dev), _path_soa(poses_l, dev), 2, dev)
            start = None if start_r is None else _interleave(start_r, start_l, 0, dev)
        thetas = _default_grid(thetas, n_theta, 0.5)
        self._upload()
        res = self._solver.solve_path_pair(soa, thetas, start, spheres=spheres, capsules=capsules, link_radius=link_radius,
                                           min_clearance=min_clearance, influence=influence, clearance_gain=clearance_gain,
                                           policy=policy, weights=weights, skip_projected=skip_projected, unwind=unwind,
                                           want_elbow=want_elbow, out=out, plan_only=plan_only)
        per_robot = ("cost", "n_solved", "blocked", "launch", "_keepalive")
        return {name: x if name in per_robot else {"r": x[:, 0::2], "l": x[:, 1::2]} for name, x in res.items()}

    def clearance_batch(self, arm_ids: Any, joints: Any, spheres: Any = None, capsules: Any = None, link_radius: Any = None,
                        other_arm: Optional[Tuple[int, Any]] = None, want: Sequence[str] = ("clearance", "nearest"),
                        out: Optional[Dict[str, torch.Tensor]] = None, plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """SymbolicIK.clearance_batch for rows of both arms (arm_ids [n] uint8, one byte per row, shared by every repetition of
        joints [K,n,7]): clearance [...], nearest [...,2] int32 (link, obstacle index), witness [...,2,3], gradient [...,7] (k *
        gradient is a bias_rates for joint_rates_batch and track_batch), link_points [...,4,3], as named in want.
        other_arm = (arm_id, joints7): adds the three capsules of that arm (0 = r, 1 = l) at the one row of joints [7] to the obstacle
        list, behind the caller's capsules (their obstacle indices are S + Cp ... S + Cp + 2, link 0 first), with the radii
        link_radius.  They are built on the device from that arm's link_points (one launch more, nothing waits) and meet EVERY row, so
        the rows should be the opposite arm's: a row of the same arm finds itself at distance 0."""
        if other_arm is not None:
            side, q = other_arm
            self._upload()
            dev = self._solver.device
            q = (q if isinstance(q, torch.Tensor) else torch.as_tensor(np.asarray(q, dtype=np.float64))).to(device=dev, dtype=torch.float64)
            lp = self._solver.clearance(q.reshape(1, 7), spheres=torch.zeros((1, 4), dtype=torch.float64, device=dev),
                                        arm_uniform=int(side), want=("link_points",))["link_points"]
            extra = arm_capsules(lp[0], link_radius)
            if capsules is None:
                capsules = extra
            else:
                given = capsules if isinstance(capsules, torch.Tensor) else torch.as_tensor(np.asarray(capsules, dtype=np.float64))
                capsules = torch.cat([given.to(device=dev, dtype=torch.float64).reshape(-1, 7), extra], dim=0)
        return _clearance_batch(self, {"arm": arm_ids}, joints, spheres, capsules, link_radius, want, out, plan_only)

    def clearance_edges_batch(self, arm_ids: Any, joints: Any, start_joints: Any = None, n_sub: int = 16, spheres: Any = None,
                              capsules: Any = None, link_radius: Any = None, min_clearance: float = -float("inf"),
                              want: Optional[Sequence[str]] = None, out: Optional[Dict[str, torch.Tensor]] = None,
                              plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """SymbolicIK.clearance_edges_batch for paths of both arms (arm_ids [n] uint8, one byte per path): the clearance along the
        motion between the waypoints of joints [T,n,7], sampled at n_sub + 1 sub-steps per edge against the static scene.  Returns
        edge_clearance, edge_sub, edge_nearest, edge_bound [T,n,...] (edge_bound: the certified lower bound on the continuous
        motion) and path_clearance, path_edge, path_bound, n_below, first_below [n,...], as named in want (None: all).  The joints
        of path_pair_batch are 2 n_pairs paths of their own here (row 2 i right, 2 i + 1 left) against the static scene; the other
        arm in motion is not among the obstacles."""
        return _clearance_edges_batch(self, {"arm": arm_ids}, joints, start_joints, n_sub, spheres, capsules, link_radius,
                                      min_clearance, want, out, plan_only)

    def theta_from_joints_batch(self, arm_ids: Any, poses: Any, current_joints: Any, preferred_theta: Optional[Sequence[float]] = None,
                                out: Optional[Dict[str, torch.Tensor]] = None, plan_only: bool = False) -> Dict[str, torch.Tensor]:
        """SymbolicIK.theta_from_joints_batch for rows of both arms (arm_ids [n] uint8).  preferred_theta: (r, l), default
        ControlIK's pair."""
        if preferred_theta is None:
            preferred_theta = (default_preferred_theta(0), default_preferred_theta(1))
        return _theta_from_joints_batch(self, {"arm": arm_ids}, poses, current_joints, preferred_theta, out, plan_only)
