// rsik_kernel_track.hpp — rsik_track: closed-loop tracking of a goal trajectory at the velocity level, one trajectory per lane, every
// step of it in one launch (track_kernel).  A step is forward kinematics of the current joints, the pose error against the step's goal,
// a twist from that error, the damped least-squares rates of rsik_joint_rates, the rate limit and one integration step; the joints
// stay in the lane's registers from the first step to the last.
//
// The chain (track_chain) is jr_columns of rsik_kernel_joint_rates.hpp restated a third time, with the position and the rotation of
// forward_kinematics (rsik_device.hpp) formed from the same partial products, and the solve is joint_rates_kernel's, expression for
// expression.  Restated and not shared, for the reason written above jr_columns: a function that jacobian_kernel, joint_rates_kernel and
// this kernel all call changes how the first two are scheduled, and their code is to stay what it is.  The expressions are the same
// ones under -ffp-contract=off, so a step's rates are rsik_joint_rates' to the bit for the same (q, v, lambda, q0), and far angles and
// rows that are not numbers are answered as rsik_jacobian answers them.
#pragma once

#include "rsik_kernel_joint_rates.hpp"  // damping_usable, jr_tri
#include "rsik_rows.hpp"
#include "rsik_tables.hpp"

namespace rsik {

constexpr int kTrackBlock = 64;  // one wave per workgroup: see track_kernel

struct TrackArgs {
    int64_t n, n_steps;
    const double* m12_steps;      // [n_steps][12][n]: R row-major, then t
    const uint8_t* arm;           // [n] or NULL
    const double* start_joints;   // [n][7]
    const double* feedforward;    // [n_steps][n][6] or NULL (FF)
    const double* damping;        // [n] or NULL: then damping_host for every trajectory
    const double* rest_joints;    // [n][7] or NULL (REST)
    double* joints_steps;         // [n_steps][n][7] or NULL (OUTS & kTrackJoints)
    double* rates_steps;          // [n_steps][n][7] or NULL (OUTS & kTrackRates)
    double* err_steps;            // [n_steps][n][2] or NULL (OUTS & kTrackErr)
    double* final_joints;         // [n][7] or NULL
    double* final_err;            // [n][2] or NULL
    double damping_host, dt, kp, ko, rest_gain;
    double rate_max[7], q_min[7], q_max[7];  // (LIM)
    ArmC arms[2];                 // as FkArgs.arms
};
constexpr int kTrackJoints = 1, kTrackRates = 2, kTrackErr = 4;  // the bits of OUTS: which per-step outputs exist

// What one step needs of the arm at joints j: the columns of J as jr_columns forms them, column k = (lin[k], ang[k]), and the goal
// frame (pos, R row-major) as forward_kinematics forms it.  The far angles of j are reduced in place.
template <bool MIXED>
__device__ __forceinline__ void track_chain(const Acc<MIXED>& A, double (&j)[7], V3 (&ang)[7], V3 (&lin)[7], V3& pos, double (&R)[9]) {
    {
        double far = fabs(j[0]);
#pragma unroll
        for (int k = 1; k < 7; k++) far = fmax(far, fabs(j[k]));
        if (RSIK_RARE(far >= kFarAngle)) {  // one copy of the reduction: the seven values rotate through it
#pragma clang loop unroll(disable)
            for (int q = 0; q < 7; q++) {
                const double t = j[0];
                j[0] = j[1]; j[1] = j[2]; j[2] = j[3]; j[3] = j[4]; j[4] = j[5]; j[5] = j[6];
                j[6] = near_angle(t);
            }
        }
    }
    double sn[7], cs[7];
    {
        const double a[4] = {j[0], j[1], j[2], j[3]}, b[3] = {j[4], j[5], j[6]};
        double s1[4], c1[4], s2[3], c2[3];
        fast_sincos_n<4>(a, s1, c1);
        fast_sincos_n<3>(b, s2, c2);
#pragma unroll
        for (int k = 0; k < 4; k++) { sn[k] = s1[k]; cs[k] = c1[k]; }
#pragma unroll
        for (int k = 0; k < 3; k++) { sn[4 + k] = s2[k]; cs[4 + k] = c2[k]; }
    }
    auto mul = [](const double (&X)[9], const double (&Y)[9], double (&Z)[9]) {
#pragma unroll
        for (int rr = 0; rr < 3; rr++)
#pragma unroll
            for (int c = 0; c < 3; c++) Z[3 * rr + c] = fma(X[3 * rr], Y[c], fma(X[3 * rr + 1], Y[3 + c], X[3 * rr + 2] * Y[6 + c]));
    };
    const double c0 = cs[0], s0 = sn[0], c1 = cs[1], s1 = sn[1], c2 = cs[2], s2 = sn[2], c3 = cs[3], s3 = sn[3];
    const double c4 = cs[4], s4 = sn[4], c5 = cs[5], s5 = sn[5], c6 = cs[6], s6 = sn[6];
    const double Gt[9] = {c0 * c1, -c0 * s1, s0, s1, c1, 0.0, -s0 * c1, s0 * s1, c0};
    const double H[9] = {c3, 0.0, s3, -s2 * s3, c2, s2 * c3, -c2 * s3, -s2, c2 * c3};
    const double Kt[9] = {c4 * c5, -s4, c4 * s5, s4 * c5, c4, s4 * s5, -s5, 0.0, c5};
    double Ms[9];
#pragma unroll
    for (int rr = 0; rr < 3; rr++)
#pragma unroll
        for (int c = 0; c < 3; c++) Ms[3 * rr + c] = A(RSIK_C_MST + 3 * c + rr);
    double MG[9], MGH[9], Rt[9];
    mul(Ms, Gt, MG);
    mul(MG, H, MGH);
    mul(MGH, Kt, Rt);
    const auto column = [](const double (&M)[9], int c) { return V3{M[c], M[3 + c], M[6 + c]}; };
    // goal axes as forward_kinematics forms them: x = Rt . (0, s6, c6), z = -Rt[:,0], y = z x x
    const V3 xg = {fma(Rt[1], s6, Rt[2] * c6), fma(Rt[4], s6, Rt[5] * c6), fma(Rt[7], s6, Rt[8] * c6)};
    const V3 zg = column(Rt, 0) * -1.0;
    const V3 yg = cross(zg, xg);
    const V3 tl = cvec(A, RSIK_C_TIPL);
    const double u = A(RSIK_C_UPPER_ARM), f = A(RSIK_C_FOREARM);
    const V3 ux = column(MG, 0), fx = column(MGH, 0);
    const V3 dw = {-fma(xg.x, tl.x, fma(yg.x, tl.y, zg.x * tl.z)), -fma(xg.y, tl.x, fma(yg.y, tl.y, zg.y * tl.z)),
                   -fma(xg.z, tl.x, fma(yg.z, tl.y, zg.z * tl.z))};  // goal origin - wrist
    const V3 de = madd(fx, f, dw);                                  // goal origin - elbow
    const V3 ds = madd(ux, u, de);                                  // goal origin - shoulder
    ang[0] = column(Ms, 1); ang[1] = column(MG, 2); ang[2] = ux * -1.0; ang[3] = column(MGH, 1);
    ang[4] = column(MGH, 2); ang[5] = column(Rt, 1); ang[6] = zg;
#pragma unroll
    for (int k = 0; k < 7; k++) lin[k] = cross(ang[k], k < 2 ? ds : k < 4 ? de : dw);
    // forward_kinematics' goal frame: wrist = s + u MG[:,0] + f MGH[:,0], pos = wrist - R . tip_local (a - t and a + (-t) are one value)
    const V3 sh = cvec(A, RSIK_C_SHOULDER);
    const V3 w = {fma(u, MG[0], fma(f, MGH[0], sh.x)), fma(u, MG[3], fma(f, MGH[3], sh.y)), fma(u, MG[6], fma(f, MGH[6], sh.z))};
    pos = w + dw;
    R[0] = xg.x; R[1] = yg.x; R[2] = zg.x;
    R[3] = xg.y; R[4] = yg.y; R[5] = zg.y;
    R[6] = xg.z; R[7] = yg.z; R[8] = zg.z;
}

// One trajectory per lane, sequentially over the steps; the definition of a step is in include/rsik.h (rsik_track).
//   shape      The work is latency-bound and sequential, and a launch is small: 4096 trajectories are 64 waves.  Workgroups of ONE
//              wave, so that those waves can go to 64 compute units and not 16 (the intent: not measured against 256 threads), and
//              one wave per SIMD asked for, so that the compiler has every register: the Jacobian, the triangle, the joints, the rest
//              joints and the next step's goal and feed-forward all stay in registers and nothing spills (DESIGN.md section 4 has
//              the counts).
//   loads      start, rest and damping once.  The 12 goal columns of step t + 1 (coalesced as they lie: 512 contiguous bytes per wave
//              and column) and the wave's 6 x 64 feed-forward doubles of step t + 1 (one contiguous slab, each lane takes 6 of its
//              doubles as they lie) are issued before step t's arithmetic and wait in registers: a step never begins with a trip to
//              memory.  The slab goes through LDS at the start of its own step, where each lane picks up its row.
//   step       track_chain; pose error (D = Rg R^T, its rotation vector); twist; bias; the solve of joint_rates_kernel (normal
//              matrix, L D L^T with the pivot clamp, two triangular solves, q0 + J^T y); rate limit (LIM: IEEE divisions, so that the
//              binding joint comes out at its limit to the last bit or one beside it); integration and clamp.
//   stores     every [*,7] and [*,2] row through store_rows (LDS): a wave writes contiguous memory, streaming.  The stores of step t are
//              issued at the head of trip t + 1, after the wait for that step's inputs and before the loads of step t + 2: see there.
//   variants   MIXED as the other kernels; OUTS: which of the per-step outputs exist; FF, REST, LIM: whether the feed-forward, the
//              rest posture and the limits exist.  A variant holds no register and issues no instruction for a term it does not
//              have.  final_joints and final_err cost nothing per step: they are a uniform test of the pointer in the trip after the
//              last step (final_err: the chain and the pose error once more).
// A skipped step (goal or feed-forward not numbers, or rates that do not come out finite) selects: joints held, rates 0, err NaN; no branch depends on data but the far-angle
// one of the chain, the order of every sum is fixed, so a trajectory's bits depend on the trajectory alone, and those of an output
// do not depend on which others exist.
template <bool MIXED, int OUTS, bool FF, bool REST, bool LIM>
__global__ __launch_bounds__(kTrackBlock, 1) void track_kernel(const TrackArgs K) {
    __shared__ SharedTables lds_tab;
    __shared__ double lds_rows[64 * 7];
    const int lane = threadIdx.x;
    const int64_t wave_row = (int64_t)blockIdx.x * kTrackBlock;  // < n: the grid has ceil(n / 64) workgroups
    stage_tables<MIXED, 0, kTrackBlock>(lds_tab, K.arms);
    const int64_t row = wave_row + lane;
    const bool live = row < K.n;
    const int64_t r = live ? row : K.n - 1;  // a lane past the end works on the last trajectory and stores nothing
    const Acc<MIXED> A = make_acc<MIXED>(K.arms, MIXED ? (K.arm[r] != 0) : false, lds_tab);
    const int64_t w_end = K.n;
    int64_t rows_here = K.n - wave_row;
    if (rows_here > 64) rows_here = 64;
    const int ff_total = (int)rows_here * 6;

    double q[7], rest[7];
#pragma unroll
    for (int k = 0; k < 7; k++) q[k] = K.start_joints[r * 7 + k];
    if constexpr (REST) {
#pragma unroll
        for (int k = 0; k < 7; k++) rest[k] = K.rest_joints[r * 7 + k];
    }
    const double lambda = K.damping ? ld_stream(K.damping + r) : K.damping_host;
    // the first step's goal and feed-forward; from here on step t + 1's are loaded while step t computes
    double g[12], ffs[6];
    const double* goal_col = K.m12_steps + r;
#pragma unroll
    for (int k = 0; k < 12; k++) g[k] = ld_stream(goal_col + k * K.n);
    if constexpr (FF) {
#pragma unroll
        for (int k = 0; k < 6; k++) ffs[k] = (k * 64 + lane < ff_total) ? ld_stream(K.feedforward + wave_row * 6 + k * 64 + lane) : 0.0;
    }

    const double nan = __builtin_nan("");
    const double l2 = lambda * lambda;
    bool bad = !all_finite(q) || !damping_usable(lambda);
    if constexpr (REST) bad = bad || !all_finite(rest);
    if (bad) {  // (a trajectory that is NaN everywhere: NaN from the start, and every step of it is held, since its rates are NaN; also
                // so that an infinity does not walk the far-angle path every step)
#pragma unroll
        for (int k = 0; k < 7; k++) q[k] = nan;
    }

    const bool want_final_err = K.final_err != nullptr;
    double qd_out[7], err_out[2];  // what the step before leaves for the head of the next trip to store
#pragma clang loop unroll(disable)
    for (int64_t t = 0; t <= K.n_steps; t++) {
        const bool last_look = t == K.n_steps;  // (uniform) the trip after the last step: its stores, final_joints, final_err
        double gc[12], ffc[6];
#pragma unroll
        for (int k = 0; k < 12; k++) gc[k] = g[k];
        if constexpr (FF) {
#pragma unroll
            for (int k = 0; k < 6; k++) ffc[k] = ffs[k];
        }
        // The wave waits HERE for this step's goal and feed-forward, which were issued a whole step ago, behind the stores of the step
        // before that: everything the counter still holds is old, and the wait costs nothing.  (gfx9 counts loads and stores in one
        // counter and the compiler waits for all of it: with the stores at the END of a step this wait would sit behind stores issued
        // a moment ago, a trip to memory at the start of every step.)  The empty asm is the first use of the loaded registers.
        asm volatile("" ::"v"(gc[0]), "v"(gc[1]), "v"(gc[2]), "v"(gc[3]), "v"(gc[4]), "v"(gc[5]), "v"(gc[6]), "v"(gc[7]), "v"(gc[8]),
                     "v"(gc[9]), "v"(gc[10]), "v"(gc[11]) : "memory");
        if constexpr (FF) asm volatile("" ::"v"(ffc[0]), "v"(ffc[1]), "v"(ffc[2]), "v"(ffc[3]), "v"(ffc[4]), "v"(ffc[5]) : "memory");
        // 8. the stores of the step before, then the loads of the step after: both have this step's arithmetic to complete in
        if (t > 0) {
            if constexpr ((OUTS & kTrackErr) != 0) store_rows<2>(K.err_steps + (t - 1) * K.n * 2, wave_row, w_end, lane, lds_rows, err_out);
            if constexpr ((OUTS & kTrackRates) != 0) store_rows<7>(K.rates_steps + (t - 1) * K.n * 7, wave_row, w_end, lane, lds_rows, qd_out);
            if ((OUTS & kTrackJoints) != 0 || (last_look && K.final_joints != nullptr)) {
                double out[7];
#pragma unroll
                for (int k = 0; k < 7; k++) out[k] = bad ? nan : q[k];
                if constexpr ((OUTS & kTrackJoints) != 0) store_rows<7>(K.joints_steps + (t - 1) * K.n * 7, wave_row, w_end, lane, lds_rows, out);
                if (last_look && K.final_joints != nullptr) store_rows<7>(K.final_joints, wave_row, w_end, lane, lds_rows, out);
            }
        }
        if (last_look && !want_final_err) break;
        if (t + 1 < K.n_steps) {  // (uniform) the next step's inputs: issued here, used a step later
            const double* next = goal_col + (t + 1) * 12 * K.n;
#pragma unroll
            for (int k = 0; k < 12; k++) g[k] = ld_stream(next + k * K.n);
            if constexpr (FF) {
                const double* slab = K.feedforward + ((t + 1) * K.n + wave_row) * 6;
#pragma unroll
                for (int k = 0; k < 6; k++) ffs[k] = (k * 64 + lane < ff_total) ? ld_stream(slab + k * 64 + lane) : 0.0;
            }
        }
        bool skip = !all_finite(gc);
        double v[6];
        if constexpr (FF) {  // the wave's slab of this step -> LDS -> each lane's row
            if (!last_look) {
#pragma unroll
                for (int k = 0; k < 6; k++) lds_rows[k * 64 + lane] = ffc[k];
                rows_staged();
                staged_row<6>(lds_rows, wave_row, w_end, lane, v);
                rows_staged();
                skip = skip || !all_finite(v);
            }
        }

        // 1. forward kinematics and the columns of J
        double qa[7];
#pragma unroll
        for (int k = 0; k < 7; k++) qa[k] = q[k];
        V3 ang[7], lin[7], pos;
        double R[9];
        track_chain<MIXED>(A, qa, ang, lin, pos, R);

        // 2. pose error: e_p = p_g - p, e_o the rotation vector of D = Rg R^T
        const V3 ep = {gc[9] - pos.x, gc[10] - pos.y, gc[11] - pos.z};
        const auto D = [&](int i, int j) { return fma(gc[3 * i], R[3 * j], fma(gc[3 * i + 1], R[3 * j + 1], gc[3 * i + 2] * R[3 * j + 2])); };
        const V3 w = {0.5 * (D(2, 1) - D(1, 2)), 0.5 * (D(0, 2) - D(2, 0)), 0.5 * (D(1, 0) - D(0, 1))};
        const double c = 0.5 * (((D(0, 0) + D(1, 1)) + D(2, 2)) - 1.0);
        const double s2 = dot(w, w), ep2 = dot(ep, ep);
        const double s = s2 > 0.0 ? sqrt_cr(s2) : 0.0;
        const double angle = fast_atan2(s, c);
        // (|e_p|^2 overflows from |e_p| = 1.34e154 on: sqrt_cr is for finite arguments, the answer there is +infinity)
        const double ep_norm = ep2 < __builtin_inf() ? sqrt_cr(ep2) : __builtin_inf();
        double err[2] = {ep2 > 0.0 ? ep_norm : 0.0, angle};
        if (last_look) {
#pragma unroll
            for (int k = 0; k < 2; k++) err[k] = (bad || skip) ? nan : err[k];
            store_rows<2>(K.final_err, wave_row, w_end, lane, lds_rows, err);
            break;
        }
        const double scale = s2 >= 0x1p-52 ? angle * fast_rcp(s) : 1.0;
        const V3 eo = w * scale;

        // 3. twist, 4. bias
        if constexpr (FF) {
            v[0] = fma(K.kp, ep.x, v[0]); v[1] = fma(K.kp, ep.y, v[1]); v[2] = fma(K.kp, ep.z, v[2]);
            v[3] = fma(K.ko, eo.x, v[3]); v[4] = fma(K.ko, eo.y, v[4]); v[5] = fma(K.ko, eo.z, v[5]);
        } else {
            v[0] = K.kp * ep.x; v[1] = K.kp * ep.y; v[2] = K.kp * ep.z;
            v[3] = K.ko * eo.x; v[4] = K.ko * eo.y; v[5] = K.ko * eo.z;
        }
        double q0[7];
        if constexpr (REST) {
#pragma unroll
            for (int k = 0; k < 7; k++) q0[k] = K.rest_gain * (rest[k] - q[k]);
        }

        // 5. rates: joint_rates_kernel's residual, normal matrix, factorisation, solves and last sum
        const auto J = [&](int i, int k) {
            return i == 0 ? lin[k].x : i == 1 ? lin[k].y : i == 2 ? lin[k].z : i == 3 ? ang[k].x : i == 4 ? ang[k].y : ang[k].z;
        };
        double y[6];  // the residual, then z, then y
#pragma unroll
        for (int i = 0; i < 6; i++) {
            y[i] = v[i];
            if constexpr (REST) {
#pragma unroll
                for (int k = 0; k < 7; k++) y[i] = fma(-J(i, k), q0[k], y[i]);
            }
        }
        double a[21];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
                double sum = i == j ? l2 : 0.0;
#pragma unroll
                for (int k = 0; k < 7; k++) sum = fma(J(i, k), J(j, k), sum);
                a[jr_tri(i, j)] = sum;
            }
        double inv[6];
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double d = a[jr_tri(j, j)];
            double wk[5];  // wk[k] = L[j][k] d_k
#pragma unroll
            for (int k = 0; k < j; k++) {
                wk[k] = a[jr_tri(j, k)] * a[jr_tri(k, k)];
                d = fma(-a[jr_tri(j, k)], wk[k], d);
            }
            d = fmax(d, l2);
            a[jr_tri(j, j)] = d;
            inv[j] = fast_rcp(d);
#pragma unroll
            for (int i = j + 1; i < 6; i++) {
                double sum = a[jr_tri(i, j)];
#pragma unroll
                for (int k = 0; k < j; k++) sum = fma(-a[jr_tri(i, k)], wk[k], sum);
                a[jr_tri(i, j)] = sum * inv[j];
            }
        }
#pragma unroll
        for (int i = 1; i < 6; i++)
#pragma unroll
            for (int k = 0; k < i; k++) y[i] = fma(-a[jr_tri(i, k)], y[k], y[i]);
#pragma unroll
        for (int i = 0; i < 6; i++) y[i] *= inv[i];
#pragma unroll
        for (int i = 4; i >= 0; i--)
#pragma unroll
            for (int k = i + 1; k < 6; k++) y[i] = fma(-a[jr_tri(k, i)], y[k], y[i]);
        double qd[7];
#pragma unroll
        for (int k = 0; k < 7; k++) {
            double sum = REST ? q0[k] : 0.0;
#pragma unroll
            for (int i = 0; i < 6; i++) sum = fma(J(i, k), y[i], sum);
            qd[k] = sum;
        }

        // Rates that are not numbers (a finite goal or feed-forward so large that the twist or the solve overflows): the step is held
        // like a skipped one.  Without this the clamp of step 7 would turn a NaN into q_min (fmin and fmax drop a NaN), and without
        // a box the joints would be NaN from here on.  A trajectory that is NaN (bad) is held here at every step, and stays NaN.
        skip = skip || !all_finite(qd);

        // 6. rate limit: one factor for the seven joints, so the direction is kept
        if constexpr (LIM) {
            double m = fabs(qd[0]) / K.rate_max[0];
#pragma unroll
            for (int k = 1; k < 7; k++) m = fmax(m, fabs(qd[k]) / K.rate_max[k]);
            if (m > 1.0) {
#pragma unroll
                for (int k = 0; k < 7; k++) qd[k] = qd[k] / m;
            }
        }
        // 7. integration; a skipped step holds the joints and reports no motion
#pragma unroll
        for (int k = 0; k < 7; k++) {
            double moved = fma(K.dt, qd[k], q[k]);
            // (fmin and fmax drop a NaN for the bound, but rates that are NaN never come here: the step is held, and a trajectory that
            // is NaN, whose rates are NaN at every step, keeps its NaN joints)
            if constexpr (LIM) moved = fmin(fmax(moved, K.q_min[k]), K.q_max[k]);
            q[k] = skip ? q[k] : moved;
            qd[k] = skip ? 0.0 : qd[k];
        }
        // (8. the stores: at the head of the next trip)
#pragma unroll
        for (int k = 0; k < 2; k++) err_out[k] = (bad || skip) ? nan : err[k];
#pragma unroll
        for (int k = 0; k < 7; k++) qd_out[k] = bad ? nan : qd[k];
    }
}

}  // namespace rsik
