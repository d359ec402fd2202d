// rsik_kernel_jacobian.hpp — rsik_jacobian: the 6 x 7 geometric Jacobian of the goal frame, its signed maximal minors (the self-motion vector) and
// Yoshikawa's manipulability, one (repetition, row) per lane (jacobian_kernel)
#pragma once

#include "rsik_rows.hpp"
#include "rsik_tables.hpp"

namespace rsik {

struct JacobianArgs {
    int64_t n;
    const double* joints;   // [n_rep][n][7]
    const uint8_t* arm;     // [n] or NULL: shared by every repetition
    double* jacobian;       // [n_rep][n][6][7] or NULL
    double* null_vector;    // [n_rep][n][7] or NULL
    double* manipulability; // [n_rep][n] or NULL
    ArmC arms[2];           // as FkArgs.arms
};

// Rows of the Jacobian a wave stages in LDS at a time: 32 rows x 42 doubles = 10.5 KiB per wave, 42 KiB per workgroup, so that three
// workgroups still share a compute unit's 160 KiB with the tables.  A wave writes its 64 rows as two contiguous slabs of 32 x 336 B.
constexpr int kJacRowsStaged = 32;

// Columns b < c of seven in lexicographic order: (0,1) ... (0,6), (1,2) ... (5,6) -> 0 ... 20
__host__ __device__ constexpr int jac_pair(int b, int c) { return b * (13 - b) / 2 + (c - b - 1); }
// Columns a < b < c of seven in lexicographic order -> 0 ... 34: the triples that start below a, then the rank of (b, c) among the pairs above a
__host__ __device__ constexpr int jac_triple(int a, int b, int c) {
    return 35 - (7 - a) * (6 - a) * (5 - a) / 6 + jac_pair(b, c) - (a + 1) * (12 - a) / 2;
}

// The 35 minors of a 3 x 7 block, one per column triple a < b < c: v_a . (v_b x v_c), from the 21 cross products v_b x v_c every triple
// above them shares.  Every index is a compile-time constant once the loops are unrolled.
__device__ __forceinline__ void jac_minors3(const V3 (&v)[7], double (&m)[35]) {
    V3 x[21];
#pragma unroll
    for (int b = 0; b < 6; b++)
#pragma unroll
        for (int c = b + 1; c < 7; c++) x[jac_pair(b, c)] = cross(v[b], v[c]);
#pragma unroll
    for (int a = 0; a < 5; a++)
#pragma unroll
        for (int b = a + 1; b < 6; b++)
#pragma unroll
            for (int c = b + 1; c < 7; c++) m[jac_triple(a, b, c)] = dot(v[a], x[jac_pair(b, c)]);
}

// (-1)^I det(J without column I): the Laplace expansion of the 6 x 6 determinant across its linear (top) and angular (bottom) three
// rows.  The six columns left are numbered 0 ... 5 in place; each of the 20 triples p < q < r of them takes the top minor of its columns
// times the bottom minor of the other three, with the sign (-1)^(p + q + r + 1).  Twenty fused multiply-adds in that order, no branch,
// no division: the value does not depend on anything but the two sets of minors.
template <int I>
__device__ __forceinline__ double jac_null_entry(const double (&top)[35], const double (&bot)[35]) {
    double acc = 0.0;
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = p + 1; q < 5; q++)
#pragma unroll
            for (int r = q + 1; r < 6; r++) {
                int rest[3] = {0, 0, 0}, m = 0;
#pragma unroll
                for (int x = 0; x < 6; x++)
                    if (x != p && x != q && x != r) rest[m++] = x;
                const auto col = [](int x) { return x + (x >= I ? 1 : 0); };  // the column of J that stands at place x
                const double t = top[jac_triple(col(p), col(q), col(r))];
                const double b = bot[jac_triple(col(rest[0]), col(rest[1]), col(rest[2]))];
                const bool minus = (((p + q + r + 1) & 1) != 0) != ((I & 1) != 0);
                acc = minus ? fma(-t, b, acc) : fma(t, b, acc);
            }
    return acc;
}

// One (repetition, row) per lane; the repetition is blockIdx.y, the rows of a workgroup are kBlock consecutive rows of that repetition.
//   joints     seven loads per lane; an angle of magnitude >= 2^27 goes through near_angle first (rare: skipped by a wave that holds none)
//   chain      forward_kinematics' own partial products (rsik_device.hpp): Gt, H, Kt, MG = Ms Gt, MGH = MG H, Rt = MGH Kt.  The joint
//              axes in the torso frame are columns of them:  a0 = Ms[:,1], a1 = MG[:,2], a2 = -MG[:,0] (the elbow yaw is Rx(-j2)),
//              a3 = MGH[:,1], a4 = MGH[:,2], a5 = Rt[:,1], a6 = -Rt[:,0] (the goal frame turns about its own z = -x_tip with j6).
//              Axes 0, 1 pass through the shoulder, 2, 3 through the elbow, 4, 5, 6 through the wrist; the lever arms p - o_k are
//              built from the goal end: p - wrist = -R tip_local, + f MGH[:,0] to the elbow, + u MG[:,0] to the shoulder.
//              Column k = (a_k x (p - o_k), a_k).
//   minors     jac_minors3 on the linear and on the angular columns, jac_null_entry per column, sqrt of the sum of squares
//   stores     the Jacobian through LDS, 32 rows at a time (flush_rows over half-rows of 21 doubles), the null vector through
//              store_rows, the manipulability directly: a wave writes contiguous memory in all three
// A row that holds a NaN or an infinity stores NaN in everything it stores; no other row sees it.
// WJ / WN / WM: the outputs requested.  The arithmetic of an output is the same instructions in every instantiation that has it.
template <bool MIXED, bool WJ, bool WN, bool WM>
__global__ __launch_bounds__(kBlock) void jacobian_kernel(const JacobianArgs K) {
    __shared__ SharedTables lds_tab;
    __shared__ double lds_out[kBlock / 64][WJ ? kJacRowsStaged * 42 : WN ? 64 * 7 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t wave_row = (int64_t)blockIdx.x * kBlock + wave * 64;
    stage_tables<MIXED>(lds_tab, K.arms);
    if (wave_row >= K.n) return;  // (the whole wave)
    const int64_t row = wave_row + lane;
    const bool live = row < K.n;
    const int64_t r = live ? row : K.n - 1;              // a lane past the end works on the last row and stores nothing
    const int64_t rep_base = (int64_t)blockIdx.y * K.n;  // first row of this repetition in the flat [n_rep * n] numbering
    const Acc<MIXED> A = make_acc<MIXED>(K.arms, MIXED ? (K.arm[r] != 0) : false, lds_tab);
    double j[7];
#pragma unroll
    for (int k = 0; k < 7; k++) j[k] = K.joints[(rep_base + r) * 7 + k];
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
    V3 ang[7], lin[7];
    ang[0] = column(Ms, 1); ang[1] = column(MG, 2); ang[2] = ux * -1.0; ang[3] = column(MGH, 1);
    ang[4] = column(MGH, 2); ang[5] = column(Rt, 1); ang[6] = zg;
#pragma unroll
    for (int k = 0; k < 7; k++) lin[k] = cross(ang[k], k < 2 ? ds : k < 4 ? de : dw);
    const double nan = __builtin_nan("");

    if constexpr (WJ) {
        double* lw = lds_out[wave];
        // in half-rows of 21 doubles, which is what flush_rows<21> counts: 64 of them are the 32 staged rows
        const int64_t h0 = 2 * (rep_base + wave_row), h_end = 2 * (rep_base + K.n);
#pragma unroll
        for (int half = 0; half < 64 / kJacRowsStaged; half++) {
            if (lane / kJacRowsStaged == half) {
                double* mine = lw + (lane % kJacRowsStaged) * 42;
#pragma unroll
                for (int k = 0; k < 7; k++) {
                    mine[k] = bad ? nan : lin[k].x; mine[7 + k] = bad ? nan : lin[k].y; mine[14 + k] = bad ? nan : lin[k].z;
                    mine[21 + k] = bad ? nan : ang[k].x; mine[28 + k] = bad ? nan : ang[k].y; mine[35 + k] = bad ? nan : ang[k].z;
                }
            }
            flush_rows<21>(K.jacobian, h0 + 2 * kJacRowsStaged * half, h_end, lane, lw);
        }
    }
    if constexpr (WN || WM) {
        double top[35], bot[35];
        jac_minors3(lin, top);
        jac_minors3(ang, bot);
        double nv[7];
        nv[0] = jac_null_entry<0>(top, bot); nv[1] = jac_null_entry<1>(top, bot); nv[2] = jac_null_entry<2>(top, bot);
        nv[3] = jac_null_entry<3>(top, bot); nv[4] = jac_null_entry<4>(top, bot); nv[5] = jac_null_entry<5>(top, bot);
        nv[6] = jac_null_entry<6>(top, bot);
        if constexpr (WM) {
            double ss = nv[0] * nv[0];
#pragma unroll
            for (int k = 1; k < 7; k++) ss = fma(nv[k], nv[k], ss);
            const double w = ::sqrt(ss);  // (IEEE: 0 at an exactly singular row, where sqrt_cr has no answer)
            if (live) st_stream(K.manipulability + rep_base + row, bad ? nan : w);
        }
        if constexpr (WN) {
#pragma unroll
            for (int k = 0; k < 7; k++) nv[k] = bad ? nan : nv[k];
            store_rows<7>(K.null_vector, rep_base + wave_row, rep_base + K.n, lane, lds_out[wave], nv);
        }
    }
}

}  // namespace rsik
