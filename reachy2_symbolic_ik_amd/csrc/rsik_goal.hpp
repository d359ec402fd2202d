// rsik_goal.hpp — from a kernel's inputs to its goal and out with the reach outputs: the head the pose kernels share (goal_of_pose,
// reach_invalid_input, store_reach: solve, sweep, nearest, path, reach_map under the rule stated in rsik_tables.hpp) and the goal-matrix
// conversion of the kernels that take matrices (goal_from_m12, load_m12)
#pragma once

#include "rsik_device.hpp"
#include "rsik_rows.hpp"

namespace rsik {

__device__ __forceinline__ void reach_invalid_input(Reach& r) {  // rsik.h "Rows that are not numbers": the reference raises (S:580) or projects an infinity
    r.ok = false; r.state = RSIK_STATE_INVALID_INPUT; r.i0 = r.i1 = __builtin_nan("");
}
// The goal stage of the sweep, nearest and path kernels: the goal's three vectors from the pose's Euler angles.  (solve_kernel spells
// the same two forms out, for the RSIK_MARKs between their halves.)
template <bool TIPZ, class ACC>
__device__ __forceinline__ Goal goal_of_pose(const ACC& A, double roll, double pitch, double yaw) {
    if constexpr (TIPZ) return goal_from_euler_tipz(A, roll, pitch, yaw);
    else return make_goal(A, rot_from_euler(roll, pitch, yaw));
}
// the per-pose outputs of is_reachable: interval, reachable, state (each optional)
template <class ARGS>
__device__ __forceinline__ void store_reach(const ARGS& K, bool live, int64_t tile0, unsigned t, const Reach& r) {
    if (!live) return;
    if (K.interval) {
        const f64x2 iv = {r.i0, r.i1};  // one 16-B store per lane
        st_stream(reinterpret_cast<f64x2*>(K.interval + 2 * tile0) + t, iv);
    }
    if (K.reachable) st_stream(K.reachable + tile0 + t, (uint8_t)(r.ok ? 1 : 0));
    if (K.state) st_stream(K.state + tile0 + t, (uint8_t)r.state);
}

// C:212-217: M -> goal pose.  np.allclose(R, I) snaps to the identity.  Otherwise the reference converts R to
// extrinsic xyz Euler angles (U:84-90) and the solver rebuilds the rotation from them (S:420).  For a proper rotation
// away from gimbal lock that round trip reproduces R to rounding, so R is consumed directly (Q6); the round trip is
// really made (euler_xyz_from_matrix + rot_from_euler) exactly where it changes the result:
//   - R is not orthonormal to 1e-12 (SciPy then substitutes the nearest rotation), or
//   - the pitch is within ~1e-5 of +-pi/2 (inside 1e-7 of the lock SciPy sets yaw := 0, which moves the joints by up
//     to ~4e-6 rad: measured on the G8 goldens).
// mode (RSIK_OPT_EULER_ROUNDTRIP): 0 = as above, 1 = always, 2 = never.
// `special` (optional): set when the matrix did not go through as it came — the identity shortcut, the Euler round trip —
// or is not a proper rotation whose third row is the cross product of the other two: the trajectory pipeline's joints
// phase re-reads all twelve entries only for those (cont_joints_kernel).
// Returns true for a block that is no right-handed frame (det <= 0, det_not_positive: SciPy raises ValueError where the reference
// converts it, U:89): the caller answers RSIK_STATE_INVALID_INPUT; Rg is then the block as it came, or NaN.  Tested in AUTO and ALWAYS —
// in AUTO also where the Gramian is the identity: a reflection has an identity Gramian — and not in NEVER, which makes no
// conversion and consumes the block as it came.
__device__ __forceinline__ bool goal_from_m12(const double (&m)[12], Rot& Rg, V3& pos, int mode, bool* special = nullptr) {
#pragma unroll
    for (int k = 0; k < 9; k++) Rg.m[k] = m[k];
    double c6, c7, c8;
    row0_cross_row1(m, c6, c7, c8);
    const bool bad = mode != 2 && det_not_positive(m, c6, c7, c8);
    if (special) {
        // row 2 against row 0 x row 1, entry by entry, to 1e-14: a few roundings of the entries themselves.  (A looser test — 1e-9
        // until round 4 — let the joints phase rebuild the third row of a matrix that is NOT orthonormal to rounding, and where
        // the arm is stretched out the elbow-yaw / wrist-yaw split amplifies such a difference 2e4 times and more: the pipeline
        // and the step kernel could then differ by ~1e-5 rad under RSIK_EULER_NEVER.  Anything else re-reads the three entries.)
        *special = !(fabs(c6 - m[6]) <= 1e-14 && fabs(c7 - m[7]) <= 1e-14 && fabs(c8 - m[8]) <= 1e-14);
    }
    // np.allclose(R, I) needs all nine entries close; R00 alone rules it out for nearly every goal
    bool eye = RSIK_RARE(np_isclose(Rg.m[0], 1.0));
    if (eye) {
#pragma unroll
        for (int k = 1; k < 9; k++) eye = eye && np_isclose(Rg.m[k], (k % 4 == 0) ? 1.0 : 0.0);
    }
    if (eye) {  // C:212-214 np.allclose(R, I)
        if (special) *special = true;
#pragma unroll
        for (int k = 0; k < 9; k++) Rg.m[k] = (k % 4 == 0) ? 1.0 : 0.0;
    } else {
        bool rt = mode == 1;
        // (1e-12 on the diagonal too: SciPy's own test lets a block scaled by 1 + 5e-6 pass as a rotation, and then normalises
        // its quaternion — consumed as it came, such a block moves the wrist by 5e-7 m)
        if (mode == 0) rt = (fabs(Rg.m[6]) > 1.0 - 1e-10) || !gram_is_identity(Rg.m, 1e-12);
        if (special && rt) *special = true;
        if (RSIK_RARE(rt)) {  // (a block with det <= 0 comes back as NaN: the row is invalid either way)
            double eul[3];
            euler_xyz_from_matrix(Rg.m, eul);
            Rg = rot_from_euler(eul[0], eul[1], eul[2]);
        }
    }
    pos = {m[9], m[10], m[11]};
    return bad;
}
__device__ __forceinline__ bool load_m12(const double* const* in, int64_t i, Rot& Rg, V3& pos, int mode) {
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = in[k][i];
    return goal_from_m12(m, Rg, pos, mode);
}

}  // namespace rsik
