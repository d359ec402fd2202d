// rsik_kernel_clearance.hpp — rsik_clearance: the distance between the arm (three capsules: shoulder - elbow - wrist - goal origin) and a
// set of sphere and capsule obstacles, the pair that gives it, its witness points and its gradient in the joints, one (repetition, row)
// per lane (clearance_kernel)
#pragma once

#include "rsik_rows.hpp"
#include "rsik_tables.hpp"

namespace rsik {

struct ClearanceArgs {
    int64_t n;
    const double* joints;    // [n_rep][n][7]
    const uint8_t* arm;      // [n] or NULL: shared by every repetition
    const double* spheres;   // [n_spheres][4]: x, y, z, r
    const double* capsules;  // [n_capsules][7]: a, b, r
    double* clearance;       // [n_rep][n] or NULL
    int32_t* nearest;        // [n_rep][n][2] or NULL: (link, obstacle)
    double* gradient;        // [n_rep][n][7] or NULL
    double* witness;         // [n_rep][n][2][3] or NULL: x on the link axis, y on the obstacle axis
    double* link_points;     // [n_rep][n][4][3] or NULL: shoulder, elbow, wrist, goal origin
    int n_spheres, n_capsules;
    double link_radius[3];
    ArmC arms[2];            // as FkArgs.arms
};

constexpr int kClrMaxSpheres = 4096, kClrMaxCapsules = 256;
// Obstacles a workgroup stages in LDS at a time.  One buffer of 1024 doubles (8 KiB) holds a tile of either kind: 256 spheres of 4
// doubles (one per thread) or 128 capsules of 8 (the seven of the row and a pad, so that a capsule is read as four 16-byte words).
constexpr int kClrSphereTile = 256, kClrCapsuleTile = 128;
static_assert(kClrSphereTile * 4 == kClrCapsuleTile * 8 && kClrSphereTile <= kBlock && kClrCapsuleTile <= kBlock, "one buffer, one obstacle per thread");

// A squared length below this counts as zero: sqrt_cr and fast_rcp are for normal numbers well inside the range.  2^-900 is the
// square of 1.1e-136 m.
constexpr double kClrTiny = 0x1p-900;
__device__ __forceinline__ double clr_rcp(double x) { return x >= kClrTiny ? fast_rcp(x) : 0.0; }
__device__ __forceinline__ double clr_sqrt(double x) { return x >= kClrTiny ? sqrt_cr(x) : 0.0; }
__device__ __forceinline__ double clr_clamp01(double v) { return fmin(fmax(v, 0.0), 1.0); }

// The best pair so far.  code = 4 * obstacle + link; s, t: where the witness points lie on the link's and on the obstacle's segment.
struct ClrBest {
    double c, s, t;
    int code;
};
// Strictly less: the first minimum wins, and a NaN (an obstacle that is skipped) never does.
template <bool WIT>
__device__ __forceinline__ void clr_take(ClrBest& B, double c, double s, double t, int code) {
    const bool win = c < B.c;
    B.c = win ? c : B.c;
    B.code = win ? code : B.code;
    if constexpr (WIT) { B.s = win ? s : B.s; B.t = win ? t : B.t; }
}

// A link P0 + s e, s in [0, 1] (ee = e . e, inv_ee = 1 / ee or 0 for a link without length), against the point C.
template <bool WIT>
__device__ __forceinline__ void clr_point(ClrBest& B, V3 P0, V3 e, double inv_ee, double rl, V3 C, double ro, int code) {
    const V3 r = P0 - C;
    const double s = clr_clamp01(-dot(r, e) * inv_ee);
    const V3 v = madd(e, s, r);
    const double d = clr_sqrt(dot(v, v));
    clr_take<WIT>(B, (d - rl) - ro, s, 0.0, code);
}

// A link against the segment Q0 + t f, t in [0, 1]: the smallest of five candidates, each a pair of points ON the two segments, so
// that the result is never below the true distance and equals it when the minimum is among them — and it is: either it is attained
// with s or t at an end (candidates 1-4: each end point against the other segment) or at the interior critical point (candidate 5).
// No branch, no special case for parallel or degenerate segments: where the 2 x 2 system has no usable determinant candidate 5
// repeats candidate 1.  The five are compared on the squared distance (one pair: the radii are the same), then one square root.
template <bool WIT>
__device__ __forceinline__ void clr_segment(ClrBest& B, V3 P0, V3 e, double ee, double inv_ee, double rl, V3 Q0, V3 f, double ff,
                                            double inv_ff, double ro, int code) {
    const V3 r = P0 - Q0;
    const double b = dot(e, f), c = dot(e, r), fr = dot(f, r);
    const double den = fma(ee, ff, -(b * b));
    double s[5], t[5];
    s[0] = 0.0; t[0] = clr_clamp01(fr * inv_ff);
    s[1] = 1.0; t[1] = clr_clamp01((fr + b) * inv_ff);
    t[2] = 0.0; s[2] = clr_clamp01(-c * inv_ee);
    t[3] = 1.0; s[3] = clr_clamp01((b - c) * inv_ee);
    s[4] = clr_clamp01(fma(b, fr, -(c * ff)) * clr_rcp(den));
    t[4] = clr_clamp01(fma(b, s[4], fr) * inv_ff);
    double d2 = 0.0, sb = 0.0, tb = 0.0;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const V3 v = madd(f, -t[k], madd(e, s[k], r));
        const double q = dot(v, v);
        const bool less = k == 0 || q < d2;
        d2 = less ? q : d2;
        sb = less ? s[k] : sb;
        tb = less ? t[k] : tb;
    }
    clr_take<WIT>(B, (clr_sqrt(d2) - rl) - ro, sb, tb, code);
}

// One (repetition, row) per lane; the repetition is blockIdx.y, the rows of a workgroup are kBlock consecutive rows of that repetition.
//   chain      jacobian_kernel's (rsik_kernel_jacobian.hpp; its comment describes the joints and the chain steps), restated like
//              jr_columns and for the same reason: joints -> sincos -> Gt, H, Kt, MG, MGH, Rt.  From it the four link points — shoulder,
//              elbow = shoulder + u MG[:,0], wrist = elbow + f MGH[:,0], goal origin = wrist - R tip_local — and the seven joint axes.
//   obstacles  staged in LDS tile by tile by the whole workgroup (one obstacle per thread), spheres first, then capsules.  The thread
//              that stages an obstacle tests it: a NaN, an infinity or a negative radius puts NaN in the radius, so that its clearance is
//              NaN against every link and clr_take never takes it.  Every lane reads the same obstacle: an LDS broadcast.
//   pairs      in the order (obstacle 0, link 0), (obstacle 0, link 1), (obstacle 0, link 2), (obstacle 1, link 0) ...; the strict
//              compare of clr_take keeps the first minimum.  The minimum itself does not depend on the order.
//   the winner its witness points from (s, t) and the obstacle's row, read again from global memory; the unit vector between them; the
//              gradient g_k = u . (a_k x (x - o_k)) for the joints below the link
//   stores     clearance and nearest (one 8-byte word per row) directly, the rest through store_rows: contiguous per wave
// No wave leaves before the last barrier: a wave past the end of the rows helps staging, works on the last row and stores nothing.
// WIT: the gradient or the witness is wanted, so (s, t) of the best pair are kept.  Which outputs are stored is decided by their
// pointers at run time; the arithmetic of an output is the same instructions whatever else is stored.
template <bool MIXED, bool WIT>
__global__ __launch_bounds__(kBlock) void clearance_kernel(const ClearanceArgs K) {
    __shared__ SharedTables lds_tab;
    __shared__ __attribute__((aligned(16))) double lds_obs[kClrSphereTile * 4];
    __shared__ double lds_out[kBlock / 64][64 * 12];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t wave_row = (int64_t)blockIdx.x * kBlock + wave * 64;
    stage_tables<MIXED>(lds_tab, K.arms);
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
    // the links as start point and direction: P[l] + s e[l], s in [0, 1]; P[3] is the goal origin
    V3 P[4], e[3];
    e[0] = ux * u;
    e[1] = fx * f;
    e[2] = {-fma(xg.x, tl.x, fma(yg.x, tl.y, zg.x * tl.z)), -fma(xg.y, tl.x, fma(yg.y, tl.y, zg.y * tl.z)),
            -fma(xg.z, tl.x, fma(yg.z, tl.y, zg.z * tl.z))};  // goal origin - wrist
    P[0] = cvec(A, RSIK_C_SHOULDER);
#pragma unroll
    for (int l = 0; l < 3; l++) P[l + 1] = P[l] + e[l];
    double ee[3], inv_ee[3];
#pragma unroll
    for (int l = 0; l < 3; l++) { ee[l] = dot(e[l], e[l]); inv_ee[l] = clr_rcp(ee[l]); }

    ClrBest B = {__builtin_inf(), 0.0, 0.0, -1};
    const int tid = threadIdx.x;
    for (int base = 0; base < K.n_spheres; base += kClrSphereTile) {
        const int count = min(kClrSphereTile, K.n_spheres - base);
        __syncthreads();  // the tile before this one has been read by every wave
        if (tid < count) {
            double v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = K.spheres[(int64_t)(base + tid) * 4 + k];
            if (!(all_finite(v) && v[3] >= 0.0)) v[3] = __builtin_nan("");
#pragma unroll
            for (int k = 0; k < 4; k++) lds_obs[tid * 4 + k] = v[k];
        }
        __syncthreads();
        for (int o = 0; o < count; o++) {
            const V3 C = {lds_obs[o * 4], lds_obs[o * 4 + 1], lds_obs[o * 4 + 2]};
            const double ro = lds_obs[o * 4 + 3];
#pragma unroll
            for (int l = 0; l < 3; l++) clr_point<WIT>(B, P[l], e[l], inv_ee[l], K.link_radius[l], C, ro, 4 * (base + o) + l);
        }
    }
    for (int base = 0; base < K.n_capsules; base += kClrCapsuleTile) {
        const int count = min(kClrCapsuleTile, K.n_capsules - base);
        __syncthreads();
        if (tid < count) {
            double v[7];
#pragma unroll
            for (int k = 0; k < 7; k++) v[k] = K.capsules[(int64_t)(base + tid) * 7 + k];
            if (!(all_finite(v) && v[6] >= 0.0)) v[6] = __builtin_nan("");
#pragma unroll
            for (int k = 0; k < 7; k++) lds_obs[tid * 8 + k] = v[k];
            lds_obs[tid * 8 + 7] = 0.0;
        }
        __syncthreads();
        for (int o = 0; o < count; o++) {
            const V3 Q0 = {lds_obs[o * 8], lds_obs[o * 8 + 1], lds_obs[o * 8 + 2]};
            const V3 Q1 = {lds_obs[o * 8 + 3], lds_obs[o * 8 + 4], lds_obs[o * 8 + 5]};
            const double ro = lds_obs[o * 8 + 6];
            const V3 fq = Q1 - Q0;
            const double ff = dot(fq, fq), inv_ff = clr_rcp(ff);
#pragma unroll
            for (int l = 0; l < 3; l++)
                clr_segment<WIT>(B, P[l], e[l], ee[l], inv_ee[l], K.link_radius[l], Q0, fq, ff, inv_ff, ro,
                                 4 * (K.n_spheres + base + o) + l);
        }
    }
    if (wave_row >= K.n) return;  // (the whole wave, behind the last barrier)

    const double nan = __builtin_nan("");
    const bool none = B.code < 0;  // every obstacle was skipped
    const int link = none ? 0 : (B.code & 3), obs = none ? 0 : (B.code >> 2);
    if (K.clearance != nullptr && live) st_stream(K.clearance + rep_base + row, bad ? nan : B.c);
    if (K.nearest != nullptr && live) {
        const bool no_pair = bad || none;
        const unsigned long long word = no_pair ? ~0ull : ((unsigned long long)(unsigned)obs << 32) | (unsigned)link;  // (link, obstacle)
        st_stream((unsigned long long*)K.nearest + rep_base + row, word);
    }
    if constexpr (WIT) {
        // the winner's obstacle again, from global memory: a sphere's centre, or a capsule's point at t
        V3 y = {nan, nan, nan};
        if (!none) {
            if (obs < K.n_spheres) {
                const double* sp = K.spheres + (int64_t)obs * 4;
                y = {sp[0], sp[1], sp[2]};
            } else {
                const double* cp = K.capsules + (int64_t)(obs - K.n_spheres) * 7;
                const V3 Q0 = {cp[0], cp[1], cp[2]}, Q1 = {cp[3], cp[4], cp[5]};
                y = madd(Q1 - Q0, B.t, Q0);
            }
        }
        const V3 Pl = link == 0 ? P[0] : link == 1 ? P[1] : P[2];
        const V3 el = link == 0 ? e[0] : link == 1 ? e[1] : e[2];
        const V3 x = none ? V3{nan, nan, nan} : madd(el, B.s, Pl);
        if (K.witness != nullptr) {
            const double w[6] = {bad ? nan : x.x, bad ? nan : x.y, bad ? nan : x.z, bad ? nan : y.x, bad ? nan : y.y, bad ? nan : y.z};
            store_rows<6>(K.witness, rep_base + wave_row, rep_base + K.n, lane, lds_out[wave], w);
        }
        if (K.gradient != nullptr) {
            const V3 v = x - y;
            const double d2 = dot(v, v);
            const double inv_d = (!none && d2 >= kClrTiny) ? fast_rcp(sqrt_cr(d2)) : 0.0;  // touching axes, or no pair: the zero vector
            const V3 un = {none ? 0.0 : v.x * inv_d, none ? 0.0 : v.y * inv_d, none ? 0.0 : v.z * inv_d};
            V3 ang[7];
            ang[0] = column(Ms, 1); ang[1] = column(MG, 2); ang[2] = ux * -1.0; ang[3] = column(MGH, 1);
            ang[4] = column(MGH, 2); ang[5] = column(Rt, 1); ang[6] = zg;
            double g[7];
#pragma unroll
            for (int k = 0; k < 7; k++) {
                const bool moves = !none && k < (link == 0 ? 2 : link == 1 ? 4 : 7);
                const V3 lever = (none ? Pl : x) - (k < 2 ? P[0] : k < 4 ? P[1] : P[2]);
                const double gk = dot(un, cross(ang[k], lever));
                g[k] = bad ? nan : moves ? gk : 0.0;
            }
            store_rows<7>(K.gradient, rep_base + wave_row, rep_base + K.n, lane, lds_out[wave], g);
        }
    }
    if (K.link_points != nullptr) {
        double lp[12];
#pragma unroll
        for (int l = 0; l < 4; l++) { lp[3 * l] = bad ? nan : P[l].x; lp[3 * l + 1] = bad ? nan : P[l].y; lp[3 * l + 2] = bad ? nan : P[l].z; }
        store_rows<12>(K.link_points, rep_base + wave_row, rep_base + K.n, lane, lds_out[wave], lp);
    }
}

}  // namespace rsik
