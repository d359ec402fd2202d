// rsik_kernel_joint_rates.hpp — rsik_joint_rates: damped least-squares joint rates from a twist of the goal frame, one (repetition, row)
// per lane (joint_rates_kernel).  The Jacobian never leaves the lane's registers.
#pragma once

#include "rsik_rows.hpp"
#include "rsik_tables.hpp"

namespace rsik {

struct JointRatesArgs {
    int64_t n;
    const double* joints;      // [n_rep][n][7]
    const uint8_t* arm;        // [n] or NULL: shared by every repetition
    const double* twist;       // [n_rep][n][6]
    const double* damping;     // [n_rep][n] or NULL: then damping_host for every row
    const double* bias_rates;  // [n_rep][n][7] or NULL (BIAS)
    double* rates;             // [n_rep][n][7] or NULL (WR)
    double* achieved_twist;    // [n_rep][n][6] or NULL (WA)
    double damping_host;
    ArmC arms[2];              // as FkArgs.arms
};

// The squares of the damping the entry point answers: lambda > 0 whose square is a normal double.  (A lambda below 1.5e-154 or above
// 1.3e154 has no usable square; such a row is answered like lambda <= 0.)
__host__ __device__ inline bool damping_usable(double lambda) {
    const double l2 = lambda * lambda;
    return lambda > 0.0 && l2 >= 2.2250738585072014e-308 && l2 <= 1.7976931348623157e308;
}

// Entry (i, j), i >= j, of a symmetric 6 x 6 matrix kept as its lower triangle, row by row: 0 ... 20
__host__ __device__ constexpr int jr_tri(int i, int j) { return i * (i + 1) / 2 + j; }

// The chain of jacobian_kernel (rsik_kernel_jacobian.hpp; its comment describes the joints and chain steps), restated: joints ->
// sincos -> Gt, H, Kt, MG, MGH, Rt -> the columns of J, column k = (lin[k], ang[k]), for the seven joints j (reduced in place where far) on the arm A.
// Restated and not shared: with the chain moved into a function both kernels call, the compiler schedules jacobian_kernel's 14
// instantiations differently (13-17 instructions fewer each, other registers), and their assembly is to stay what it was.  The
// expressions are the same ones, under -ffp-contract=off, so the far-angle and NaN behaviour are rsik_jacobian's.
// Returns whether the row holds a NaN or an infinity.
template <bool MIXED>
__device__ __forceinline__ bool jr_columns(const Acc<MIXED>& A, double (&j)[7], V3 (&ang)[7], V3 (&lin)[7]) {
    const bool bad = !all_finite(j);
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
    return bad;
}

// One (repetition, row) per lane; the repetition is blockIdx.y, as jacobian_kernel.
//   loads      joints as jacobian_kernel, the row's damping directly; twist [*,6] and bias_rates [*,7] go to LDS (stage_rows: a wave reads
//              its 64 rows as one contiguous slab) and wait there while the chain runs: every load is issued before anything waits,
//              and the chain does not hold 26 registers for operands it does not use; the bias is read a second time for the last sum
//   chain      jr_columns: column k of J = (lin[k], ang[k]).  These 42 doubles are the only copy of J.
//   residual   r = twist - J q0                                                  (BIAS; 6 x 7 fused multiply-adds, k = 0 ... 6)
//   normal     A = J J^T + lambda^2 I, lower triangle: entry (i, j) starts from lambda^2 (i == j) or 0 and takes seven fused
//              multiply-adds, k = 0 ... 6
//   factor     A = L D L^T in natural order, no square root, in place: column j holds L[i][j] d_j until the pivot is known.  Every pivot
//              d_j is clamped from below at lambda^2 (exactly it is a Schur complement of J J^T plus lambda^2, so never smaller: the
//              clamp changes no exact result and keeps 1 / d_j finite where rounding would not).  Six fast_rcp.
//   solves     L z = r, z_i /= d_i, L^T y = z
//   rates      q0 + J^T y                                                        (7 x 6 fused multiply-adds, i = 0 ... 5)
//   achieved   J rates                                                           (WA; 6 x 7 fused multiply-adds, k = 0 ... 6)
//   stores     both through store_rows (LDS): a wave writes contiguous memory
// The order of every sum is fixed and no branch depends on data (but the far-angle one of jr_columns), so a row's bits depend on the
// row alone.  The rates are computed the same way whether they are stored or not: the bits of an output do not depend on the other.
// A row with a NaN or an infinity in joints, twist or bias, or whose damping is not usable, stores NaN in everything it stores.
// Waves per SIMD: the rates-only form without bias is asked to fit three (168 registers; it needs 170 when left alone and fits without
// a spill); every other form spills 2-21 registers when asked the same and stays at two.
template <bool MIXED, bool BIAS, bool WR, bool WA>
__global__ __launch_bounds__(kBlock, (!BIAS && !WA) ? 3 : 2) void joint_rates_kernel(const JointRatesArgs K) {
    static_assert(WR || WA, "at least one output");
    __shared__ SharedTables lds_tab;
    __shared__ double lds_rows[kBlock / 64][64 * (BIAS ? 13 : 7)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t wave_row = (int64_t)blockIdx.x * kBlock + wave * 64;
    stage_tables<MIXED>(lds_tab, K.arms);
    if (wave_row >= K.n) return;  // (the whole wave)
    const int64_t row = wave_row + lane;
    const bool live = row < K.n;
    const int64_t r = live ? row : K.n - 1;              // a lane past the end works on the last row and stores nothing
    const int64_t rep_base = (int64_t)blockIdx.y * K.n;  // first row of this repetition in the flat [n_rep * n] numbering
    const Acc<MIXED> A = make_acc<MIXED>(K.arms, MIXED ? (K.arm[r] != 0) : false, lds_tab);
    double* lt = lds_rows[wave];   // the twist rows, later the achieved twist or the rates (without bias)
    double* lb = lt + 64 * 6;      // the bias rows, later the rates (only with BIAS)
    const int64_t w0 = rep_base + wave_row, w_end = rep_base + K.n;

    // every global load of the lane is issued here, before anything waits: one trip to memory
    double j[7];
#pragma unroll
    for (int k = 0; k < 7; k++) j[k] = K.joints[(rep_base + r) * 7 + k];
    const double lambda = K.damping ? ld_stream(K.damping + rep_base + r) : K.damping_host;
    stage_rows<6>(K.twist, w0, w_end, lane, lt);
    if constexpr (BIAS) stage_rows<7>(K.bias_rates, w0, w_end, lane, lb);

    V3 ang[7], lin[7];
    bool bad = jr_columns<MIXED>(A, j, ang, lin);
    // entry (i, k) of J, i and k compile-time constants once the loops are unrolled
    const auto J = [&](int i, int k) {
        return i == 0 ? lin[k].x : i == 1 ? lin[k].y : i == 2 ? lin[k].z : i == 3 ? ang[k].x : i == 4 ? ang[k].y : ang[k].z;
    };
    const double l2 = lambda * lambda;
    bad = bad || !damping_usable(lambda);

    // twist and bias have waited in LDS while the chain held the registers
    rows_staged();
    double v[6], q0[7];
    staged_row<6>(lt, w0, w_end, lane, v);
    bad = bad || !all_finite(v);
    if constexpr (BIAS) {
        staged_row<7>(lb, w0, w_end, lane, q0);
        bad = bad || !all_finite(q0);
    }

    double y[6];  // the residual, then z, then y
#pragma unroll
    for (int i = 0; i < 6; i++) {
        y[i] = v[i];
        if constexpr (BIAS) {
#pragma unroll
            for (int k = 0; k < 7; k++) y[i] = fma(-J(i, k), q0[k], y[i]);
        }
    }
    double a[21];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) {
            double s = i == j ? l2 : 0.0;
#pragma unroll
            for (int k = 0; k < 7; k++) s = fma(J(i, k), J(j, k), s);
            a[jr_tri(i, j)] = s;
        }
    double inv[6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        // a(j, k), k < j, holds L[j][k]; a(i, j), i > j, is reduced to L[i][j] d_j, then scaled
        double d = a[jr_tri(j, j)];
        double w[5];  // w[k] = L[j][k] d_k
#pragma unroll
        for (int k = 0; k < j; k++) {
            w[k] = a[jr_tri(j, k)] * a[jr_tri(k, k)];
            d = fma(-a[jr_tri(j, k)], w[k], d);
        }
        d = fmax(d, l2);
        a[jr_tri(j, j)] = d;
        inv[j] = fast_rcp(d);
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double s = a[jr_tri(i, j)];
#pragma unroll
            for (int k = 0; k < j; k++) s = fma(-a[jr_tri(i, k)], w[k], s);
            a[jr_tri(i, j)] = s * inv[j];
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

    const double nan = __builtin_nan("");
    if constexpr (BIAS) {  // read again instead of kept: seven register pairs the factorisation does not have to hold
        asm volatile("" ::: "memory");
        staged_row<7>(lb, w0, w_end, lane, q0);
    }
    rows_staged();  // (every lane has read its inputs: the slabs are free for the outputs)
    double qd[7];
#pragma unroll
    for (int k = 0; k < 7; k++) {
        double s = BIAS ? q0[k] : 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++) s = fma(J(i, k), y[i], s);
        qd[k] = s;
    }
    if constexpr (WA) {
        double at[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 7; k++) s = fma(J(i, k), qd[k], s);
            at[i] = bad ? nan : s;
        }
        store_rows<6>(K.achieved_twist, w0, w_end, lane, lt, at);
    }
    if constexpr (WR) {
#pragma unroll
        for (int k = 0; k < 7; k++) qd[k] = bad ? nan : qd[k];
        store_rows<7>(K.rates, w0, w_end, lane, BIAS ? lb : lt, qd);
    }
}

}  // namespace rsik
