// rsik_kernel_track_avoid.hpp — rsik_track_avoid: rsik_track with obstacle avoidance inside the loop (track_avoid_kernel).  A step is
// track_kernel's step (rsik_kernel_track.hpp) with one term more in its bias: the clearance of the current joints against a static
// set of obstacles, as clearance_kernel (rsik_kernel_clearance.hpp) defines it, and, where that clearance is below `influence`, the
// gradient of the winning pair times avoid_gain (influence - clearance) added to the bias rates.
//
// The chain (avoid_chain) is track_chain restated, with the four link points of clearance_kernel formed beside the goal frame from
// the same partial products: the link points with clearance_kernel's expressions (P[l + 1] = P[l] + e[l]), so that a step's clearance
// and nearest pair are rsik_clearance's to the bit for the same joints, the goal frame and the columns of J with track_chain's, so
// that a trajectory the push never acts on has rsik_track's bits.  Restated and not shared, for the reason written above jr_columns.
// The pair tests themselves (clr_point, clr_segment, clr_take and the tiny-value guards) are clearance_kernel's functions, called.
#pragma once

#include "rsik_kernel_clearance.hpp"    // clr_point, clr_segment, clr_take, ClrBest, kClrTiny
#include "rsik_kernel_joint_rates.hpp"  // damping_usable, jr_tri
#include "rsik_kernel_track.hpp"        // kTrackBlock
#include "rsik_rows.hpp"
#include "rsik_tables.hpp"

namespace rsik {

constexpr int kAvoidMaxSpheres = 256, kAvoidMaxCapsules = 64;  // what a workgroup stages ONCE: 256 x 4 + 64 x 8 doubles = 12 KiB

struct TrackAvoidArgs {
    int64_t n, n_steps;
    const double* m12_steps;      // [n_steps][12][n]: R row-major, then t
    const uint8_t* arm;           // [n] or NULL
    const double* start_joints;   // [n][7]
    const double* feedforward;    // [n_steps][n][6] or NULL (FF)
    const double* damping;        // [n] or NULL: then damping_host for every trajectory
    const double* rest_joints;    // [n][7] or NULL
    const double* spheres;        // [n_spheres][4]: x, y, z, r
    const double* capsules;       // [n_capsules][7]: a, b, r
    double* joints_steps;         // [n_steps][n][7] or NULL
    double* rates_steps;          // [n_steps][n][7] or NULL
    double* err_steps;            // [n_steps][n][2] or NULL
    double* clearance_steps;      // [n_steps][n] or NULL
    int32_t* nearest_steps;       // [n_steps][n][2] or NULL: (link, obstacle)
    double* final_joints;         // [n][7] or NULL
    double* final_err;            // [n][2] or NULL
    double* min_clearance;        // [n] or NULL
    int n_spheres, n_capsules;
    double damping_host, dt, kp, ko, rest_gain, influence, avoid_gain;
    double link_radius[3];
    double rate_max[7], q_min[7], q_max[7];  // (LIM)
    ArmC arms[2];                 // as FkArgs.arms
};

// What one step needs of the arm at joints j: the joint axes ang[k], the forearm's direction fx (from it, from ang[2] = -(the upper
// arm's direction) and from e[2] = goal origin - wrist, avoid_levers forms the three levers whose cross products with the axes are the
// columns of J as track_chain forms them: AFTER the pair loop, so that six registers fewer are live across it), the goal frame (pos, R
// row-major) as forward_kinematics forms it, and the links P[l] + s e[l] as clearance_kernel forms them.  The far angles of j are
// reduced in place.
template <bool MIXED>
__device__ __forceinline__ void avoid_chain(const Acc<MIXED>& A, double (&j)[7], V3 (&ang)[7], V3& fx_out, V3& pos, double (&R)[9],
                                            V3 (&P)[4], V3 (&e)[3]) {
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
    // track_chain's axes and goal frame
    fx_out = fx;
    ang[0] = column(Ms, 1); ang[1] = column(MG, 2); ang[2] = ux * -1.0; ang[3] = column(MGH, 1);
    ang[4] = column(MGH, 2); ang[5] = column(Rt, 1); ang[6] = zg;
    const V3 sh = cvec(A, RSIK_C_SHOULDER);
    const V3 w = {fma(u, MG[0], fma(f, MGH[0], sh.x)), fma(u, MG[3], fma(f, MGH[3], sh.y)), fma(u, MG[6], fma(f, MGH[6], sh.z))};
    pos = w + dw;
    R[0] = xg.x; R[1] = yg.x; R[2] = zg.x;
    R[3] = xg.y; R[4] = yg.y; R[5] = zg.y;
    R[6] = xg.z; R[7] = yg.z; R[8] = zg.z;
    // clearance_kernel's links: start point and direction, P[3] the goal origin
    e[0] = ux * u;
    e[1] = fx * f;
    e[2] = dw;
    P[0] = sh;
#pragma unroll
    for (int l = 0; l < 3; l++) P[l + 1] = P[l] + e[l];
}

// track_chain's levers: goal origin - shoulder, - elbow, - wrist.  (ang2 * -1.0 is the upper arm's direction to the bit: ang[2] is
// that direction times -1.0.)
template <bool MIXED>
__device__ __forceinline__ void avoid_levers(const Acc<MIXED>& A, V3 ang2, V3 fx, V3 dw, V3 (&lever)[3]) {
    const double u = A(RSIK_C_UPPER_ARM), f = A(RSIK_C_FOREARM);
    lever[2] = dw;
    lever[1] = madd(fx, f, dw);
    lever[0] = madd(ang2 * -1.0, u, lever[1]);
}

// The link's start point or direction: a select of VALUES.  (Written in place as `link == 0 ? P[0] : link == 1 ? P[1] : P[2]` the
// conditional is a choice between array elements, that is of an address, and inside the step loop the compiler answers it with the
// three points in scratch memory and an indexed load.  Arguments by value are loaded before the choice.)
__device__ __forceinline__ double avoid_pick(int link, double a, double b, double c) { return link == 0 ? a : link == 1 ? b : c; }
__device__ __forceinline__ V3 avoid_pick(int link, V3 a, V3 b, V3 c) {
    return V3{avoid_pick(link, a.x, b.x, c.x), avoid_pick(link, a.y, b.y, c.y), avoid_pick(link, a.z, b.z, c.z)};
}

// track_kernel (its comment describes the shape, the loads, the step and the stores; all of that is kept) with step 4 of
// include/rsik.h (rsik_track_avoid) in place of the rest bias alone.
//   obstacles  staged ONCE per workgroup, before the loop, with clearance_kernel's validity test (a NaN, an infinity or a negative radius
//              puts NaN in the radius: such an obstacle's clearance is NaN against every link and clr_take never takes it).  They stay in
//              LDS for every step; every lane reads the same obstacle: a broadcast.
//   per step   avoid_chain; the pose error and the twist (the goal, the position and the rotation end there); the pair loop in
//              clearance_kernel's order, keeping (c, s, t, code) of the best pair — it runs BEFORE the levers, the linear columns of J
//              and the triangle are formed, so that they are not live across it (with one wave per SIMD the kernel has every
//              register, and this order is what keeps all eight forms free of spills); after the loop the winner's row is read
//              again from LDS, its witness points, the unit vector between them and the gradient are formed as clearance_kernel forms
//              them; then the select of step 4b and track_kernel's solve, limit and integration.
//   stores     clearance_steps (one double per lane, coalesced as it lies) and nearest_steps (one 8-byte word per lane) directly, with
//              the other stores of step t at the head of trip t + 1.  min_clearance is a running minimum in one register; the
//              clearance at the final joints is one more chain and pair loop in the trip after the last step, and only when
//              min_clearance is asked for.
//   variants   MIXED, FF, LIM as track_kernel.  The rest posture and which outputs exist are uniform tests of their pointers at run
//              time and selects: 8 instantiations, not 128.  Where neither a rest posture nor a push is there the bias is left out of
//              the residual by a select (not multiplied in as zeros), which is what keeps rsik_track's bits on such a trajectory.
// As in track_kernel, no branch depends on data but the far-angle one of the chain, and the order of every sum is fixed.
template <bool MIXED, bool FF, bool LIM>
__global__ __launch_bounds__(kTrackBlock, 1) void track_avoid_kernel(const TrackAvoidArgs K) {
    __shared__ SharedTables lds_tab;
    __shared__ double lds_rows[64 * 7];
    __shared__ __attribute__((aligned(16))) double lds_sph[kAvoidMaxSpheres * 4];
    __shared__ __attribute__((aligned(16))) double lds_cap[kAvoidMaxCapsules * 8];
    const int lane = threadIdx.x;
    const int64_t wave_row = (int64_t)blockIdx.x * kTrackBlock;  // < n: the grid has ceil(n / 64) workgroups
    // the obstacles, once: n_spheres <= kAvoidMaxSpheres and n_capsules <= kAvoidMaxCapsules (the host refuses anything else)
    for (int o = lane; o < K.n_spheres; o += kTrackBlock) {
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = K.spheres[(int64_t)o * 4 + k];
        if (!(all_finite(v) && v[3] >= 0.0)) v[3] = __builtin_nan("");
#pragma unroll
        for (int k = 0; k < 4; k++) lds_sph[o * 4 + k] = v[k];
    }
    for (int o = lane; o < K.n_capsules; o += kTrackBlock) {
        double v[7];
#pragma unroll
        for (int k = 0; k < 7; k++) v[k] = K.capsules[(int64_t)o * 7 + k];
        if (!(all_finite(v) && v[6] >= 0.0)) v[6] = __builtin_nan("");
#pragma unroll
        for (int k = 0; k < 7; k++) lds_cap[o * 8 + k] = v[k];
        lds_cap[o * 8 + 7] = 0.0;
    }
    stage_tables<MIXED, 0, kTrackBlock>(lds_tab, K.arms);  // (ends with the barrier that also stands behind the obstacles)
    const int64_t row = wave_row + lane;
    const bool live = row < K.n;
    const int64_t r = live ? row : K.n - 1;  // a lane past the end works on the last trajectory and stores nothing
    const Acc<MIXED> A = make_acc<MIXED>(K.arms, MIXED ? (K.arm[r] != 0) : false, lds_tab);
    const int64_t w_end = K.n;
    int64_t rows_here = K.n - wave_row;
    if (rows_here > 64) rows_here = 64;
    const int ff_total = (int)rows_here * 6;
    const bool has_rest = K.rest_joints != nullptr;  // (uniform)

    double q[7], rest[7];
#pragma unroll
    for (int k = 0; k < 7; k++) q[k] = K.start_joints[r * 7 + k];
#pragma unroll
    for (int k = 0; k < 7; k++) rest[k] = has_rest ? K.rest_joints[r * 7 + k] : 0.0;
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
    const bool bad = !all_finite(q) || !damping_usable(lambda) || !all_finite(rest);
    if (bad) {  // (as track_kernel: NaN from the start, every step held)
#pragma unroll
        for (int k = 0; k < 7; k++) q[k] = nan;
    }

    const bool want_final_err = K.final_err != nullptr, want_min = K.min_clearance != nullptr;
    double qd_out[7], err_out[2], clr_out = nan;  // what the step before leaves for the head of the next trip to store
    unsigned long long near_out = ~0ull;
    double min_clr = __builtin_inf();
#pragma clang loop unroll(disable)
    for (int64_t t = 0; t <= K.n_steps; t++) {
        const bool last_look = t == K.n_steps;  // (uniform) the trip after the last step: its stores and the final outputs
        double gc[12], ffc[6];
#pragma unroll
        for (int k = 0; k < 12; k++) gc[k] = g[k];
        if constexpr (FF) {
#pragma unroll
            for (int k = 0; k < 6; k++) ffc[k] = ffs[k];
        }
        // the wave waits HERE for this step's goal and feed-forward, issued a whole step ago: see track_kernel
        asm volatile("" ::"v"(gc[0]), "v"(gc[1]), "v"(gc[2]), "v"(gc[3]), "v"(gc[4]), "v"(gc[5]), "v"(gc[6]), "v"(gc[7]), "v"(gc[8]),
                     "v"(gc[9]), "v"(gc[10]), "v"(gc[11]) : "memory");
        if constexpr (FF) asm volatile("" ::"v"(ffc[0]), "v"(ffc[1]), "v"(ffc[2]), "v"(ffc[3]), "v"(ffc[4]), "v"(ffc[5]) : "memory");
        // 8. the stores of the step before, then the loads of the step after: both have this step's arithmetic to complete in
        if (t > 0) {
            if (K.clearance_steps != nullptr && live) st_stream(K.clearance_steps + (t - 1) * K.n + row, clr_out);
            if (K.nearest_steps != nullptr && live) st_stream((unsigned long long*)K.nearest_steps + (t - 1) * K.n + row, near_out);
            if (K.err_steps != nullptr) store_rows<2>(K.err_steps + (t - 1) * K.n * 2, wave_row, w_end, lane, lds_rows, err_out);
            if (K.rates_steps != nullptr) store_rows<7>(K.rates_steps + (t - 1) * K.n * 7, wave_row, w_end, lane, lds_rows, qd_out);
            if (K.joints_steps != nullptr || (last_look && K.final_joints != nullptr)) {
                double out[7];
#pragma unroll
                for (int k = 0; k < 7; k++) out[k] = bad ? nan : q[k];
                if (K.joints_steps != nullptr) store_rows<7>(K.joints_steps + (t - 1) * K.n * 7, wave_row, w_end, lane, lds_rows, out);
                if (last_look && K.final_joints != nullptr) store_rows<7>(K.final_joints, wave_row, w_end, lane, lds_rows, out);
            }
        }
        if (last_look && !want_final_err && !want_min) break;
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

        // 1. forward kinematics, the joint axes and the links
        double qa[7];
#pragma unroll
        for (int k = 0; k < 7; k++) qa[k] = q[k];
        V3 ang[7], fx, pos, P[4], e[3];
        double R[9];
        avoid_chain<MIXED>(A, qa, ang, fx, pos, R, P, e);

        // 2. pose error: e_p = p_g - p, e_o the rotation vector of D = Rg R^T.  (2 and 3 stand AHEAD of the pair loop: the goal, the
        // position and the rotation end here, and the loop has their registers.)
        const V3 ep = {gc[9] - pos.x, gc[10] - pos.y, gc[11] - pos.z};
        const auto D = [&](int i, int j) { return fma(gc[3 * i], R[3 * j], fma(gc[3 * i + 1], R[3 * j + 1], gc[3 * i + 2] * R[3 * j + 2])); };
        const V3 w = {0.5 * (D(2, 1) - D(1, 2)), 0.5 * (D(0, 2) - D(2, 0)), 0.5 * (D(1, 0) - D(0, 1))};
        const double c = 0.5 * (((D(0, 0) + D(1, 1)) + D(2, 2)) - 1.0);
        const double s2 = dot(w, w), ep2 = dot(ep, ep);
        const double s = s2 > 0.0 ? sqrt_cr(s2) : 0.0;
        const double angle = fast_atan2(s, c);
        const double ep_norm = ep2 < __builtin_inf() ? sqrt_cr(ep2) : __builtin_inf();
        double err[2] = {ep2 > 0.0 ? ep_norm : 0.0, angle};
        if (last_look && want_final_err) {  // (uniform)
            double fe[2];
#pragma unroll
            for (int k = 0; k < 2; k++) fe[k] = (bad || skip) ? nan : err[k];
            store_rows<2>(K.final_err, wave_row, w_end, lane, lds_rows, fe);
        }
        const double scale = s2 >= 0x1p-52 ? angle * fast_rcp(s) : 1.0;
        const V3 eo = w * scale;

        // 3. twist
        if constexpr (FF) {
            v[0] = fma(K.kp, ep.x, v[0]); v[1] = fma(K.kp, ep.y, v[1]); v[2] = fma(K.kp, ep.z, v[2]);
            v[3] = fma(K.ko, eo.x, v[3]); v[4] = fma(K.ko, eo.y, v[4]); v[5] = fma(K.ko, eo.z, v[5]);
        } else {
            v[0] = K.kp * ep.x; v[1] = K.kp * ep.y; v[2] = K.kp * ep.z;
            v[3] = K.ko * eo.x; v[4] = K.ko * eo.y; v[5] = K.ko * eo.z;
        }
        // 4a. the clearance of q, its pair and its gradient: clearance_kernel's loop over the staged obstacles, and its winner
        double grad[7] = {}, clr = nan;
        if (!last_look || want_min) {  // (uniform)
            double ee[3], inv_ee[3];
#pragma unroll
            for (int l = 0; l < 3; l++) { ee[l] = dot(e[l], e[l]); inv_ee[l] = clr_rcp(ee[l]); }
            ClrBest B = {__builtin_inf(), 0.0, 0.0, -1};
#pragma unroll 4  // (four spheres' chains in flight: -7 ... -9 % of a launch, the same bits; the capsule loop unrolled spills)
            for (int o = 0; o < K.n_spheres; o++) {
                const V3 C = {lds_sph[o * 4], lds_sph[o * 4 + 1], lds_sph[o * 4 + 2]};
                const double ro = lds_sph[o * 4 + 3];
#pragma unroll
                for (int l = 0; l < 3; l++) clr_point<true>(B, P[l], e[l], inv_ee[l], K.link_radius[l], C, ro, 4 * o + l);
            }
#pragma clang loop unroll(disable)
            for (int o = 0; o < K.n_capsules; o++) {
                const V3 Q0 = {lds_cap[o * 8], lds_cap[o * 8 + 1], lds_cap[o * 8 + 2]};
                const V3 Q1 = {lds_cap[o * 8 + 3], lds_cap[o * 8 + 4], lds_cap[o * 8 + 5]};
                const double ro = lds_cap[o * 8 + 6];
                const V3 fq = Q1 - Q0;
                const double ff = dot(fq, fq), inv_ff = clr_rcp(ff);
#pragma unroll
                for (int l = 0; l < 3; l++)
                    clr_segment<true>(B, P[l], e[l], ee[l], inv_ee[l], K.link_radius[l], Q0, fq, ff, inv_ff, ro, 4 * (K.n_spheres + o) + l);
            }
            const bool none = B.code < 0;  // every obstacle was skipped
            const int link = none ? 0 : (B.code & 3), obs = none ? 0 : (B.code >> 2);
            clr = bad ? nan : B.c;
            min_clr = B.c < min_clr ? B.c : min_clr;
            if (last_look) {
                if (live) st_stream(K.min_clearance + row, bad ? nan : min_clr);  // (want_min holds here)
            } else {
                clr_out = clr;
                near_out = (bad || none) ? ~0ull : ((unsigned long long)(unsigned)obs << 32) | (unsigned)link;  // (link, obstacle)
                // the winner's obstacle again, from LDS: a sphere's centre, or a capsule's point at t (a winner is never a skipped row,
                // so what LDS holds of it is what global memory holds)
                const bool is_sphere = obs < K.n_spheres;
                const int so = is_sphere ? obs : 0, co = is_sphere ? 0 : obs - K.n_spheres;
                const V3 C = {lds_sph[so * 4], lds_sph[so * 4 + 1], lds_sph[so * 4 + 2]};
                const V3 Q0 = {lds_cap[co * 8], lds_cap[co * 8 + 1], lds_cap[co * 8 + 2]};
                const V3 Q1 = {lds_cap[co * 8 + 3], lds_cap[co * 8 + 4], lds_cap[co * 8 + 5]};
                const V3 yc = madd(Q1 - Q0, B.t, Q0);
                const V3 y = {is_sphere ? C.x : yc.x, is_sphere ? C.y : yc.y, is_sphere ? C.z : yc.z};
                const V3 Pl = avoid_pick(link, P[0], P[1], P[2]), el = avoid_pick(link, e[0], e[1], e[2]);
                const V3 x = madd(el, B.s, Pl);
                const V3 d = x - y;
                const double d2 = dot(d, d);
                const double inv_d = (!none && d2 >= kClrTiny) ? fast_rcp(sqrt_cr(d2)) : 0.0;  // touching axes, or no pair: the zero vector
                const V3 un = {none ? 0.0 : d.x * inv_d, none ? 0.0 : d.y * inv_d, none ? 0.0 : d.z * inv_d};
#pragma unroll
                for (int k = 0; k < 7; k++) {
                    const bool moves = !none && k < (link == 0 ? 2 : link == 1 ? 4 : 7);
                    const V3 arm_k = (none ? Pl : x) - (k < 2 ? P[0] : k < 4 ? P[1] : P[2]);
                    const double gk = dot(un, cross(ang[k], arm_k));
                    grad[k] = moves ? gk : 0.0;
                }
            }
        }

        if (last_look) break;

        // 4b. bias: the rest term, and the push where the clearance is below the influence distance (a select: +infinity, "no
        // obstacle usable", and a NaN trajectory never push)
        const bool push = clr < K.influence;
        const double gain = K.avoid_gain * (K.influence - clr);
        const bool biased = has_rest || push;
        double q0[7];
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const double rest_k = has_rest ? K.rest_gain * (rest[k] - q[k]) : 0.0;
            const double pushed = rest_k + gain * grad[k];
            q0[k] = push ? pushed : rest_k;
        }

        // 5. rates: joint_rates_kernel's residual, normal matrix, factorisation, solves and last sum
        V3 lin[7], lever[3];
        avoid_levers<MIXED>(A, ang[2], fx, e[2], lever);
#pragma unroll
        for (int k = 0; k < 7; k++) lin[k] = cross(ang[k], k < 2 ? lever[0] : k < 4 ? lever[1] : lever[2]);
        const auto J = [&](int i, int k) {
            return i == 0 ? lin[k].x : i == 1 ? lin[k].y : i == 2 ? lin[k].z : i == 3 ? ang[k].x : i == 4 ? ang[k].y : ang[k].z;
        };
        double y[6];  // the residual, then z, then y
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double res = v[i];
#pragma unroll
            for (int k = 0; k < 7; k++) res = fma(-J(i, k), q0[k], res);
            y[i] = biased ? res : v[i];
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
            double sum = q0[k];
#pragma unroll
            for (int i = 0; i < 6; i++) sum = fma(J(i, k), y[i], sum);
            qd[k] = sum;
        }

        // rates that are not numbers: the step is held like a skipped one (see track_kernel)
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
