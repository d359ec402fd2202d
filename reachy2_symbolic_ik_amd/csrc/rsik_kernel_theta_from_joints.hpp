// rsik_kernel_theta_from_joints.hpp — rsik_theta_from_joints / rsik_theta_from_joints_state: for n independent rows, the theta of
// the elbow circle whose solution is closest to the row's measured joints (utils.get_best_theta_to_current_joints, U:267-331), and
// the two rate-limiter stages of rsik_stage (U:115-127, U:220-264)
#pragma once

#include "rsik_goal.hpp"
#include "rsik_kernel_stages.hpp"
#include "rsik_kernel_state.hpp"
#include "rsik_rows.hpp"
#include "rsik_tables.hpp"

namespace rsik {

// ------------------------------------------------------------------------------------------
// What every caller of the reference does when it starts or restarts an arm (C:142-158, C:306-325): is_reachable_no_limits on the
// pose the arm is in, then a ternary search over the whole circle — one get_joints at the preferred theta, two per iteration for
// 16 iterations, one more at the end.  cont_init_kernel does the same for the few lone waves of a run's start; this is the
// throughput form: one row per lane, chip-filling launches.
//
// The search is about 35 DEPENDENT joints_from_theta evaluations per lane, so the kernel is fp64-VALU and latency bound (130 B in,
// 90 B out per row).  What it is built around:
//   - the two mid points of an iteration stand side by side in the loop body.  They depend on each other only through the rare
//     projection branch, so the scheduler interleaves the two evaluations: two independent chains per lane is what hides the fp64
//     latency at 2 waves per SIMD.  (A form with ONE inlined evaluation walked by a per-lane state machine — a quarter of the
//     code, 178-184 VGPRs — serialises them and measured 0.98-1.24 x the timed-out step kernel: dropped, docs/experiments.md T.1.)
//   - what does not depend on theta is formed once per row: the goal's three vectors (make_goal), the measured joints, the
//     bracket ends.  The compiler moves the rest of the loop-invariant part of the evaluation (the goal x axis in the shoulder
//     frame, the arm constants) out of the loop by itself, since the evaluation is inlined into it.
//   - the evaluation order is the reference's, one after the other, because each get_joints can move the solver's state where the
//     elbow projection fires (Q1): no two-lanes-per-row form here (cont_init_kernel's PAIR is only valid where no projection can
//     fire, and at full occupancy the second lane is not idle silicon but another row's).
// The numbers compared are bit for bit those of best_theta_to_current_joints (same functions, same order; the translation unit is
// compiled without contraction), so a theta found here is the theta a timed-out continuous step finds.
// ------------------------------------------------------------------------------------------
struct ThetaSearchOut {
    double theta, low, high, distance;
    double j[7];
    V3 elbow;
    bool projected;
};

// n14: the constructor's list-of-both-arms form (Q15, C:152-158): joints 0 and 1, each against all seven entries of its list.
template <class Acc>
__device__ __forceinline__ ThetaSearchOut theta_search(const Acc& A, Reach& r, const Goal& G, const double* cur, bool n14, double pref) {
    const double zeros[7] = {0, 0, 0, 0, 0, 0, 0};
    const double tolerance = 0.01;
    ThetaSearchOut S;
    auto eval = [&](double th, bool keep) -> double {
        double st, ct;
        fast_sincos(near_angle(th), &st, &ct);  // (th can be the caller's preferred theta: any finite double)
        const JointsOut o = joints_from_theta_g<false>(A, r, G, ct, st, zeros);
        double acc = 0.0;
        if (RSIK_RARE(n14)) {
#pragma unroll
            for (int q = 0; q < 2; q++)
#pragma unroll
                for (int k = 0; k < 7; k++) { const double d = angle_diff(o.j[q], cur[7 * q + k]); acc += d * d; }
        } else {
#pragma unroll
            for (int k = 0; k < 7; k++) { const double d = angle_diff(o.j[k], cur[k]); acc += d * d; }
        }
        const double dist = sqrt(acc);
        if (keep) {
#pragma unroll
            for (int k = 0; k < 7; k++) S.j[k] = o.j[k];
            S.elbow = o.elbow; S.projected = o.projected; S.distance = dist; S.theta = th;
        }
        return dist;
    };
    double low = -kPi, high = kPi;
    if (A(RSIK_C_SIDE) < 0) { low = 0; high = kTwoPi; }
    S.low = S.high = __builtin_nan("");
    if (eval(pref, true) < tolerance) return S;  // U:296-300
    // (bounded whatever the data: the bracket is arithmetic on constants and shrinks by a third per iteration — 16 iterations)
    while ((high - low) > tolerance) {
        const double mid1 = low + (high - low) / 3;
        const double mid2 = high - (high - low) / 3;
        const double f1 = eval(mid1, false);
        const double f2 = eval(mid2, false);
        if (f1 < f2) high = mid2; else low = mid1;
    }
    (void)eval((low + high) / 2, true);  // U:323-324: evaluated once more (the call's side effect on the solver state, Q1)
    S.low = low; S.high = high;
    return S;
}

struct ThetaFromJointsArgs {
    int64_t n;
    const double* goal[12];        // pose_soa[6] or m12_soa[12]
    const uint8_t* arm;
    int euler_roundtrip;           // RSIK_OPT_EULER_ROUNDTRIP (matrix goals)
    const double* current_joints;  // [n,7]; the state entry: [n, n_current]
    int n_current;                 // the state entry: 7 or 14
    double pref[2];                // preferred theta per arm slot
    double* solver_state;          // the state entry
    double* theta;                 // [n]
    double* joints;                // [n,7] or NULL
    double* bracket;               // [n,2] or NULL
    double* distance;              // [n] or NULL
    uint8_t* state;                // [n] or NULL
    ArmC arms[2];
};

// MIXED as in solve_kernel: 0 = one arm for the whole launch (constants are scalar loads from the argument block), 1 = an arm byte per
// row, every constant from the lane's LDS copy, 2 = an arm byte per row and the two blocks mirror images of each other (checked by
// the host): only the constants with a handedness come from LDS.  The evaluation reads ~60 constants, 35 times over: with form 1
// they are LDS reads inside the loop (there are no registers left to keep them in), with form 2 two thirds of them are scalar again.
template <int MIXED, bool M12>
__global__ __launch_bounds__(kBlock) void theta_from_joints_kernel(const ThetaFromJointsArgs K) {
    __shared__ double lds_out[kBlock / 64][64 * 7];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t wave_base = (int64_t)blockIdx.x * kBlock + wave * 64;
    const bool live = i < K.n;
    const int64_t ii = live ? i : (K.n - 1);

    __shared__ SharedTables lds_tab;
    stage_tables<(MIXED != 0), (MIXED == 1 ? 0 : (int)offsetof(ThetaFromJointsArgs, arms) + (int)sizeof(ArmC))>(lds_tab, K.arms);
    const int slot = (MIXED != 0 && K.arm[ii] != 0) ? 1 : 0;
    const AccK<MIXED> A = kernarg_acc<AccK<MIXED>, ThetaFromJointsArgs>(lds_tab, slot);

    double cur[7];
#pragma unroll
    for (int k = 0; k < 7; k++) cur[k] = K.current_joints[ii * 7 + k];
    Rot Rg;
    V3 pos;
    bool invalid = !all_finite(cur);
    if constexpr (M12) {
        double m[12];
#pragma unroll
        for (int k = 0; k < 12; k++) m[k] = K.goal[k][ii];
        invalid = invalid || !all_finite(m);
        invalid = goal_from_m12(m, Rg, pos, K.euler_roundtrip) || invalid;  // ... or no right-handed frame
    } else {
        double p[6];
#pragma unroll
        for (int k = 0; k < 6; k++) p[k] = K.goal[k][ii];
        invalid = invalid || !all_finite(p);
        pos = {p[0], p[1], p[2]};
        Rg = rot_from_caller_euler(p[3], p[4], p[5]);
    }
    const Goal G = make_goal(A, Rg);
    Reach r = reach_g<true>(A, pos, G.woff);  // is_reachable_no_limits (S:85-119)
    ThetaSearchOut S = theta_search(A, r, G, cur, false, K.pref[slot]);
    int code = RSIK_STATE_REACHABLE;
    if (RSIK_RARE(invalid || !r.ok)) {  // rsik.h "Rows that are not numbers"; C:385-387
        code = invalid ? RSIK_STATE_INVALID_INPUT : RSIK_STATE_NOT_REACHABLE_NO_LIMITS;
        const double nan = __builtin_nan("");
        S.theta = S.low = S.high = S.distance = nan;
#pragma unroll
        for (int k = 0; k < 7; k++) S.j[k] = nan;
    }
    if (K.joints) store_rows<7>(K.joints, wave_base, K.n, lane, lds_out[wave], S.j);
    if (live) {
        K.theta[i] = S.theta;
        if (K.bracket) { K.bracket[2 * i] = S.low; K.bracket[2 * i + 1] = S.high; }
        if (K.distance) K.distance[i] = S.distance;
        if (K.state) K.state[i] = (uint8_t)code;
    }
}

// The drop-in call shape: the same search on stored solver-state rows (rsik_kernel_state.hpp), each row left as the reference
// leaves `self` after those get_joints calls.  Not a hot path (the scalar API calls it with n = 1, on pinned host rows).
template <bool MIXED>
__global__ __launch_bounds__(kBlock) void theta_from_joints_state_kernel(const ThetaFromJointsArgs K) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    __shared__ SharedTables lds_tab;
    stage_tables<MIXED, (int)offsetof(ThetaFromJointsArgs, arms) + (MIXED ? 0 : (int)sizeof(ArmC))>(lds_tab, K.arms);
    if (i >= K.n) return;
    const Acc<MIXED> A = make_acc<MIXED>(K.arms, MIXED ? (K.arm[i] != 0) : false, lds_tab);
    const int slot = MIXED ? (A.isl ? 1 : 0) : 0;
    double* Sr = K.solver_state + i * RSIK_SOLVER_STATE_STRIDE;
    Reach r = reach_from_state(Sr);
    const Goal G = make_goal(A, rot_from_caller_euler(Sr[3], Sr[4], Sr[5]));
    const bool n14 = K.n_current == 14;
    double cur[14];
#pragma unroll
    for (int k = 0; k < 14; k++) cur[k] = (k < 7 || n14) ? K.current_joints[i * K.n_current + k] : 0.0;
    const ThetaSearchOut S = theta_search(A, r, G, cur, n14, K.pref[slot]);
    K.theta[i] = S.theta;
    if (K.bracket) { K.bracket[2 * i] = S.low; K.bracket[2 * i + 1] = S.high; }
#pragma unroll
    for (int k = 0; k < 7; k++) Sr[24 + k] = S.j[k];
    Sr[0] = r.pos.x; Sr[1] = r.pos.y; Sr[2] = r.pos.z;
    Sr[6] = r.w.x; Sr[7] = r.w.y; Sr[8] = r.w.z;
    Sr[16] = S.elbow.x; Sr[17] = S.elbow.y; Sr[18] = S.elbow.z;
    Sr[19] = S.projected ? 1.0 : 0.0;
}

// rsik_stage, the rate limiter as utils.py exposes it (today only inside the continuous kernels: continuous_next_theta_goal).  A
// kernel of its own, so that stage_kernel stays the code it was.  Row-major in and out like stage_kernel:
//   RSIK_STAGE_TEND_TO_PREFERRED_THETA  U:115-127.  in: previous_theta, d_theta_max, goal_theta; out: reached 0/1, theta
//   RSIK_STAGE_BEST_CONTINUOUS_THETA2   U:220-264.  in: the 18 operands of RSIK_STAGE_BEST_DISCRETE_THETA, d_theta_max;
//                                       out: reachable 0/1, theta, which text (0 nothing found, 1 "ok et proche", 2 "ok mais loin"),
//                                       "preferred_theta worked" 0/1 of the search inside
__device__ __forceinline__ bool tend_to_theta_ref(double previous_theta, double d_theta_max, double goal, double& theta) {
    const double ad = angle_diff(goal, previous_theta);
    if (fabs(ad) < d_theta_max) { theta = goal; return true; }
    const double sign = ad / fabs(ad);  // U:126, U:258
    theta = previous_theta + sign * d_theta_max;
    return false;
}
__global__ __launch_bounds__(kBlock) void stage_limiter_kernel(const StageArgs K) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= K.n) return;
    const double* x = K.in + i * K.in_stride;
    double* o = K.out + i * K.out_stride;
    if (K.op == RSIK_STAGE_TEND_TO_PREFERRED_THETA) {
        double th;
        const bool reached = tend_to_theta_ref(x[0], x[1], x[2], th);
        o[0] = reached ? 1.0 : 0.0; o[1] = th;
    } else {  // RSIK_STAGE_BEST_CONTINUOUS_THETA2
        double in[19];
        for (int k = 0; k < 19; k++) in[k] = x[k];
        double goal = in[0], th = in[0];
        bool worked = false;
        const int nb = (in[3] >= 0.0 && in[3] <= 1048576.0) ? (int)in[3] : 0;
        const bool found = best_discrete_theta_ref(in[0], in[1], in[2], nb, in[4], in[5], in[6], in[7], V3{in[8], in[9], in[10]},
                                                   V3{in[11], in[12], in[13]}, in[14], V3{in[15], in[16], in[17]}, goal, worked);
        double which = 0.0;
        if (found) which = tend_to_theta_ref(in[0], in[18], goal, th) ? 1.0 : 2.0;  // U:252-264
        o[0] = found ? 1.0 : 0.0; o[1] = found ? th : in[0]; o[2] = which; o[3] = worked ? 1.0 : 0.0;
    }
}

}  // namespace rsik
