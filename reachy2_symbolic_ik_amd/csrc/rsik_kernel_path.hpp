// rsik_kernel_path.hpp — rsik_solve_path: n paths of n_steps waypoints, n_theta elbow angles per waypoint, and of the n_theta ^ n_steps
// ways through them the one whose joints move least (solve_path_kernel); rsik_solve_path_clear: the same kernel over PathClearArgs,
// where a sample too close to a static set of obstacles is no candidate and one inside the influence distance pays a penalty
#pragma once

#include <type_traits>

#include "rsik_goal.hpp"
#include "rsik_kernel_clearance.hpp"    // clr_point, clr_segment, ClrBest
#include "rsik_kernel_nearest.hpp"
#include "rsik_kernel_track_avoid.hpp"  // kAvoidMaxSpheres, kAvoidMaxCapsules
#include "rsik_rows.hpp"
#include "rsik_tables.hpp"

namespace rsik {

struct PathArgs {
    int64_t n;           // paths
    int64_t n_steps;     // waypoints per path; every per-waypoint array is [n_steps][n], waypoint-major
    const double* in[6];
    const uint8_t* arm;  // [n], one byte per path, or NULL
    int theta_policy;    // RSIK_THETA_EXPLICIT or RSIK_THETA_FRACTION
    int n_theta;         // samples per waypoint, 1 ... 64
    int theta_per_pose;  // 0: theta_in[n_theta], one value per sample for every waypoint; else theta_in[n_theta][n_steps * n]
    int skip_projected;  // RSIK_PATH_SKIP_PROJECTED: a sample whose elbow projection fired is no candidate
    int unwind;          // RSIK_PATH_UNWIND
    const double* theta_in;
    double prev[7];      // get_joints' previous_joints: zeros
    const double* start; // [n,7] or NULL: the joints each path starts from
    double weights[7];   // of the squared joint differences
    uint8_t* back;       // workspace: [n][n_steps][n_theta] backpointers, then [n][n_steps] winners
    int32_t* index;      // [n_steps][n] or NULL: the winning sample, -1 at a skipped waypoint
    double* theta;       // [n_steps][n] or NULL
    double* joints;      // [n_steps][n][7] or NULL
    double* elbow;       // [n_steps][n][3] or NULL
    uint8_t* projected;  // [n_steps][n] or NULL
    double* step_cost;   // [n_steps][n] or NULL: sqrt of the transition cost into the waypoint
    double* cost;        // [n] or NULL: the minimal sum
    int32_t* n_solved;   // [n] or NULL
    double* interval;    // [n_steps][n][2] or NULL
    uint8_t* reachable;  // [n_steps][n] or NULL
    uint8_t* state;      // [n_steps][n] or NULL
    ArmC arms[2];        // as SolveArgs.arms
};

// rsik_solve_path_clear's argument block: PathArgs' fields by the same names (solve_path_kernel reads either), then the scene, the
// constraint and the three outputs that go with it.
struct PathClearArgs {
    int64_t n;
    int64_t n_steps;
    const double* in[6];
    const uint8_t* arm;
    int theta_policy;
    int n_theta;
    int theta_per_pose;
    int skip_projected;
    int unwind;
    const double* theta_in;
    double prev[7];
    const double* start;
    double weights[7];
    uint8_t* back;
    int32_t* index;
    double* theta;
    double* joints;
    double* elbow;
    uint8_t* projected;
    double* step_cost;
    double* cost;
    int32_t* n_solved;
    double* interval;
    uint8_t* reachable;
    uint8_t* state;
    const double* spheres;   // [n_spheres][4]: x, y, z, r
    const double* capsules;  // [n_capsules][7]: a, b, r
    double* clearance;       // [n_steps][n] or NULL: d of the winning sample
    int32_t* nearest;        // [n_steps][n][2] or NULL: (link, obstacle) of the winning sample
    uint8_t* blocked;        // [n_steps][n] or NULL: candidates of rsik_solve_path that fail d >= min_clearance
    int n_spheres, n_capsules;
    double min_clearance, influence, clearance_gain;
    double link_radius[3];
    ArmC arms[2];
};

// This kernel's own constant accessor, for AccSweep's reason.
template <int MIXED>
struct AccPath : AccK<MIXED> {};

constexpr unsigned kPathNone = 0xffu;   // a backpointer / winner byte: no candidate in this lane, a skipped waypoint
constexpr unsigned kPathFirst = 0xfeu;  // a backpointer byte: a candidate of the path's first solved waypoint
constexpr int kPathRow = 8;             // doubles of a sample's LDS row: 7 joints and A, the least cost of a path that ends in it
constexpr int kPathLds = 2 * 64 * kPathRow + 8;  // doubles per wave: two row sets (previous, current) and the start / carry row

// c(a, b) of rsik.h, b the sample's joints and a the row they are measured against (both in registers): the operations of
// solve_nearest_kernel's cost on the same operands, so the same bits — d_q = angle_diff(b_q, a_q), c = sum_q (w_q d_q) d_q, q = 0 ... 6 in
// that order, unfused — with the seven angle_diffs side by side: pymod_2pi's rare fix-up (the quotient rounded across an integer) is
// tested ONCE for all seven, on their minimum and maximum, instead of as seven branches on seven compare masks.  Applied to a value
// already in [0, 2 pi), or to a NaN (which the minimum and maximum let through), the fix-up changes nothing.
__device__ __forceinline__ double path_cost(const double (&w)[7], const double (&b)[7], const double (&a)[7]) {
    double m[7];
#pragma unroll
    for (int q = 0; q < 7; q++) {
        const double x = (b[q] - a[q]) + kPi;
        m[q] = fma(-floor(x * 0.15915494309189535), kTwoPi, x);
    }
    double lo = m[0], hi = m[0];
#pragma unroll
    for (int q = 1; q < 7; q++) { lo = __builtin_fmin(lo, m[q]); hi = __builtin_fmax(hi, m[q]); }
    if (RSIK_RARE(!(lo >= 0 && hi < kTwoPi))) {
#pragma unroll
        for (int q = 0; q < 7; q++) {
            if (m[q] < 0) m[q] += kTwoPi;
            if (m[q] >= kTwoPi) m[q] -= kTwoPi;
        }
    }
    double c = 0.0;
#pragma unroll
    for (int q = 0; q < 7; q++) {
        const double d = m[q] - kPi;
        c = c + (w[q] * d) * d;
    }
    return c;
}
// A row of 8 doubles in LDS (16-byte aligned): four 16-byte reads, issued together
struct PathRow { f64x2 v[4]; };
__device__ __forceinline__ PathRow path_row(const double* p) {
    const f64x2* p2 = reinterpret_cast<const f64x2*>(p);
    return PathRow{{p2[0], p2[1], p2[2], p2[3]}};
}
__device__ __forceinline__ double path_cost(const double (&w)[7], const double (&b)[7], const PathRow& r) {
    const double a[7] = {r.v[0].x, r.v[0].y, r.v[1].x, r.v[1].y, r.v[2].x, r.v[2].y, r.v[3].x};
    return path_cost(w, b, a);
}
// the same against 7 doubles anywhere in LDS (the start row, a staged output row)
__device__ __forceinline__ double path_cost_at(const double (&w)[7], const double (&b)[7], const double* p) {
    double a[7];
#pragma unroll
    for (int q = 0; q < 7; q++) a[q] = p[q];
    return path_cost(w, b, a);
}
// The links of the arm at joints j as clearance_kernel forms them (its chain, restated as avoid_chain restates it and for the reason
// written above jr_columns: the same expressions on the same operands, so the same bits): start points P[0 ... 2], directions e.
template <class ACC>
__device__ __forceinline__ void path_links(const ACC& A, double (&j)[7], V3 (&P)[4], V3 (&e)[3]) {
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
    e[0] = ux * u;
    e[1] = fx * f;
    e[2] = {-fma(xg.x, tl.x, fma(yg.x, tl.y, zg.x * tl.z)), -fma(xg.y, tl.x, fma(yg.y, tl.y, zg.y * tl.z)),
            -fma(xg.z, tl.x, fma(yg.z, tl.y, zg.z * tl.z))};  // goal origin - wrist
    P[0] = cvec(A, RSIK_C_SHOULDER);
#pragma unroll
    for (int l = 0; l < 3; l++) P[l + 1] = P[l] + e[l];
}

// clearance_kernel's pair loop over the obstacles a workgroup staged (track_avoid_kernel's layout), in its order: the clearance and
// the code 4 * obstacle + link of the first minimum, -1 where every obstacle is skipped.  No witness: (s, t) are not kept.
__device__ __forceinline__ ClrBest path_pairs(const V3 (&P)[4], const V3 (&e)[3], const double (&rl)[3], int n_spheres, int n_capsules,
                                              const double* lds_sph, const double* lds_cap) {
    double ee[3], inv_ee[3];
#pragma unroll
    for (int l = 0; l < 3; l++) { ee[l] = dot(e[l], e[l]); inv_ee[l] = clr_rcp(ee[l]); }
    ClrBest B = {__builtin_inf(), 0.0, 0.0, -1};
#pragma unroll 4  // (as track_avoid_kernel: four spheres' chains in flight; the capsule loop stays rolled)
    for (int o = 0; o < n_spheres; o++) {
        const V3 C = {lds_sph[o * 4], lds_sph[o * 4 + 1], lds_sph[o * 4 + 2]};
        const double ro = lds_sph[o * 4 + 3];
#pragma unroll
        for (int l = 0; l < 3; l++) clr_point<false>(B, P[l], e[l], inv_ee[l], rl[l], C, ro, 4 * o + l);
    }
#pragma clang loop unroll(disable)
    for (int o = 0; o < n_capsules; o++) {
        const V3 Q0 = {lds_cap[o * 8], lds_cap[o * 8 + 1], lds_cap[o * 8 + 2]};
        const V3 Q1 = {lds_cap[o * 8 + 3], lds_cap[o * 8 + 4], lds_cap[o * 8 + 5]};
        const double ro = lds_cap[o * 8 + 6];
        const V3 fq = Q1 - Q0;
        const double ff = dot(fq, fq), inv_ff = clr_rcp(ff);
#pragma unroll
        for (int l = 0; l < 3; l++)
            clr_segment<false>(B, P[l], e[l], ee[l], inv_ee[l], rl[l], Q0, fq, ff, inv_ff, ro, 4 * (n_spheres + o) + l);
    }
    return B;
}

__device__ __forceinline__ void path_lds_fence() {  // the wave's LDS writes are done before any lane reads another lane's
    wave_lds_fence();
    branch_stores_stay();
}

// One wave = one path, kBlock / 64 paths per workgroup.  ONE loop runs both passes, so that a sample is the same instructions in both
// (solve_nearest_kernel's last trip, generalised): the head of solve_sweep_kernel (loads, goal stage, reach_g) and one sample
// (joints_from_theta_g on a copy of the wrist reach_g left), then what the pass does with it.
//
// Trips 0 ... n_steps - 1, the forward pass: every lane holds waypoint t of the path, lane k takes sample k.  Lane k puts its joints
// into row k of the current LDS row set, walks the candidates i of the previous solved waypoint (a scalar loop over the set bits of
// their ballot; the rows are broadcast reads), keeps the least A(i) + c(J_prev[i], J[k]) — the lowest i among equal values, the loop
// ascends — and writes A into its row and i into its byte of the backpointer table (workspace).  A waypoint without a candidate in any lane
// (one ballot) leaves the previous rows as they are.
// Trip n_steps starts with the backtrack: the least (A, k) of the last solved waypoint (nearest_of_group), then down the table, eight rows'
// bytes loaded ahead of the eight cross-lane reads that depend on each other.  Lane t & 63 keeps waypoint t's winner and the wave
// writes 64 of them at a time to the workspace, where the output pass's lane — the same lane — finds it.
// Trips n_steps ..., the output pass: lane l holds waypoint 64 (trip - n_steps) + l and runs its one winning sample again: the sweep's
// bits, 1 / n_theta of the forward pass's samples.  Rows are staged in LDS; the step costs are measured between a row and the solved
// row before it (in the slab, or the carry row a trip leaves for the next); RSIK_PATH_UNWIND then walks the slab's solved rows in
// order, lane q < 7 joint q; the rows leave as runs of 7 (3) doubles, 64 addresses per store.
#ifndef RSIK_PATH_MIN_WAVES
#define RSIK_PATH_MIN_WAVES 1
#endif
//
// ARGS = PathClearArgs (rsik_solve_path_clear; `if constexpr (CLEAR)` below, nothing of it in rsik_solve_path's instantiations):
//   obstacles  staged ONCE per workgroup ahead of the tables' barrier, as track_avoid_kernel stages them and with its validity test (a NaN
//              in the radius of a skipped row, capsules padded to 8 doubles): 12 KiB beside the four waves' row sets.
//   per trip   where some lane holds a candidate (forward pass), or a winner and clearance / nearest are asked for (output pass), a
//              wave-uniform test: path_links and path_pairs on the lane's joints, d = the clearance rsik_clearance returns for them.
//   forward    a candidate with !(d >= min_clearance) is none; `blocked` is the difference of the two ballots, stored by lane 0; the
//              penalty p = (gain u) u, u = influence - d where d < influence, is added to A AFTER the minimum over the previous rows.
//   output     d and the (link, obstacle) word of the winning sample, one store each per lane; NaN and (-1, -1) at a skipped waypoint.
template <int MIXED, bool TIPZ, class ARGS = PathArgs>
__global__ __launch_bounds__(kBlock, RSIK_PATH_MIN_WAVES) void solve_path_kernel(const ARGS K) {
    constexpr bool CLEAR = std::is_same<ARGS, PathClearArgs>::value;
    constexpr int PB = kBlock / 64;  // paths per workgroup
    __shared__ SharedTables lds_tab;
    __shared__ __attribute__((aligned(16))) double lds[PB][kPathLds];
    __shared__ __attribute__((aligned(16))) double lds_sph[CLEAR ? kAvoidMaxSpheres * 4 : 1];
    __shared__ __attribute__((aligned(16))) double lds_cap[CLEAR ? kAvoidMaxCapsules * 8 : 1];
    static_assert(sizeof(SharedTables) + sizeof(g_sincos_tab) + sizeof(double) * (PB * kPathLds + (kAvoidMaxSpheres * 4 + kAvoidMaxCapsules * 8)) <= 64 * 1024,
                  "the static LDS of a workgroup: tables, row sets and the staged scene");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t path = (int64_t)blockIdx.x * PB + wave;
    const int64_t pc = path < K.n ? path : K.n - 1;  // (a wave past the end stages the tables with the others, then leaves)

    if constexpr (CLEAR) {  // the scene, once: n_spheres <= kAvoidMaxSpheres and n_capsules <= kAvoidMaxCapsules (the host refuses anything else)
        for (int o = threadIdx.x; o < K.n_spheres; o += kBlock) {
            double v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = K.spheres[(int64_t)o * 4 + k];
            if (!(all_finite(v) && v[3] >= 0.0)) v[3] = __builtin_nan("");
#pragma unroll
            for (int k = 0; k < 4; k++) lds_sph[o * 4 + k] = v[k];
        }
        for (int o = threadIdx.x; o < K.n_capsules; o += kBlock) {
            double v[7];
#pragma unroll
            for (int k = 0; k < 7; k++) v[k] = K.capsules[(int64_t)o * 7 + k];
            if (!(all_finite(v) && v[6] >= 0.0)) v[6] = __builtin_nan("");
#pragma unroll
            for (int k = 0; k < 7; k++) lds_cap[o * 8 + k] = v[k];
            lds_cap[o * 8 + 7] = 0.0;
        }
    }
    warm_and_stage_tables<MIXED>(K, lds_tab);  // (ends with the barrier that also stands behind the scene)
    const AccPath<MIXED> A = kernarg_acc<AccPath<MIXED>, ARGS>(lds_tab, (MIXED != 0 && K.arm[pc] != 0) ? 1 : 0);
    if (path >= K.n) return;  // (wave-uniform; no workgroup barrier follows)

    double* lds_wave = lds[wave];
    double* carry = lds_wave + 2 * 64 * kPathRow;  // the start row; in the output pass the last solved row of the trips before
    const int T = (int)K.n_steps;
    const int NT = K.n_theta;
    const int64_t n = K.n;
    const bool want_elbow = K.elbow != nullptr;
    const bool fraction = K.theta_policy != RSIK_THETA_EXPLICIT;
    const bool per_pose = K.theta_per_pose != 0;
    const bool skip_projected = K.skip_projected != 0;
    const bool has_start = K.start != nullptr;
    uint8_t* back = K.back + path * T * NT;          // [T][NT]
    uint8_t* winners = K.back + n * T * NT + path * T;  // [T]
    double w[7];
#pragma unroll
    for (int q = 0; q < 7; q++) w[q] = K.weights[q];

    // the start row: lane q < 7 keeps entry q (what RSIK_PATH_UNWIND measures the first solved row against) and puts it into LDS
    double uprev = 0.0;
    bool lost = false;  // rsik.h: a start row that holds something that is not a number loses its path
    if (has_start) {
        if (lane < 7) {
            uprev = K.start[path * 7 + lane];
            carry[lane] = uprev;
        }
        lost = __builtin_amdgcn_ballot_w64(lane < 7 && !(fabs(uprev) < __builtin_inf())) != 0;
        path_lds_fence();
    }

    unsigned long long pmask = 0;  // the candidates of the last solved waypoint (scalar)
    int cs = 0;                    // the row set the next solved waypoint writes
    int solved = 0;                // solved waypoints so far
    double last_a = __builtin_inf();  // this lane's A at the last solved waypoint, inf where it was no candidate there
    bool have_carry = has_start;      // output pass: there is a row (start, or a solved one) in front of this trip's rows
    bool have_uprev = has_start;
    const int trips = (T + 63) >> 6;
#pragma clang loop unroll(disable)
    for (int it = 0; it < T + trips; it++) {
        const bool out = it >= T;  // scalar
        if (it == T) {
            // ---- the end of the forward pass: the path's cost and its last sample, then the winners by backtracking
            double end_a = last_a;
            int end_k = (pmask >> lane) & 1 ? lane : kNoSample;
            nearest_of_group<64>(end_a, end_k);
            if (lane == 0) {
                if (K.cost) st_stream(K.cost + path, solved ? end_a : __builtin_nan(""));
                if (K.n_solved) st_stream(K.n_solved + path, (int32_t)solved);
            }
            int cur = __builtin_amdgcn_readfirstlane(end_k);
            unsigned mine = kPathNone;
            for (int tb = T - 1; tb >= 0; tb -= 8) {
                unsigned b[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int t = tb - u;
                    b[u] = (t >= 0 && lane < NT) ? (unsigned)back[(int64_t)t * NT + lane] : kPathNone;
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int t = tb - u;
                    if (t >= 0) {
                        const bool was_solved = __builtin_amdgcn_ballot_w64(b[u] != kPathNone) != 0;
                        if ((t & 63) == lane) mine = was_solved ? (unsigned)cur : kPathNone;
                        if (was_solved) cur = __builtin_amdgcn_readlane((int)b[u], cur & 63);
                        if ((t & 63) == 0 && t + lane < T) winners[t + lane] = (uint8_t)mine;
                    }
                }
            }
        }
        // ---- which waypoint and which sample this lane takes
        const int wp_raw = out ? ((it - T) << 6) + lane : it;
        const bool live = wp_raw < T;                       // (the forward pass: every lane)
        const int wp = live ? wp_raw : T - 1;
        int k = lane;
        if (out) k = live ? (int)winners[wp] : (int)kPathNone;
        const int64_t row = (int64_t)wp * n + path;  // of every [n_steps][n] array

        double in[6];
#pragma unroll
        for (int c = 0; c < 6; c++) in[c] = ld_stream(K.in[c] + row);
        const bool invalid = settle_pose(in);  // rsik.h "Rows that are not numbers"
        const V3 pos = {in[0], in[1], in[2]};
        const Goal G = goal_of_pose<TIPZ>(A, in[3], in[4], in[5]);
        Reach r = reach_g<false, false>(A, pos, G.woff);
        if (RSIK_RARE(invalid)) reach_invalid_input(r);
        if (out) store_reach(K, live, row, 0u, r);

        // ---- the sample
        const bool run = r.ok && k < NT && !lost;
        JointsOut o;
        double theta = __builtin_nan("");
        bool cand = false;
        if (run) {
            const double th_in = per_pose ? K.theta_in[(int64_t)k * T * n + row] : K.theta_in[k];
            theta = th_in;
            if (fraction) {
                const double fa = r.i0;
                double fb = r.i1;
                if (fa > fb) fb += kTwoPi;
                theta = fa + th_in * (fb - fa);
            }
            double ct, st;
            fast_sincos(near_angle(theta), &st, &ct);
            o = joints_from_theta_g<true, TIPZ>(A, r, G, ct, st, (const double*)K.prev);
            cand = !(skip_projected && o.projected);
#pragma unroll
            for (int q = 0; q < 7; q++) cand = cand && o.j[q] == o.j[q];  // "its joints are numbers"
        }
        double pen = 0.0, clr = __builtin_nan("");  // CLEAR: p and d of this lane's sample
        unsigned long long near_word = ~0ull;
        if constexpr (CLEAR) {
            const bool want_clr = K.clearance != nullptr || K.nearest != nullptr;
            const bool sel = out ? (run && live) : cand;  // the lanes whose d is used
            const unsigned long long pre = __builtin_amdgcn_ballot_w64(sel);
            if (pre != 0 && (!out || want_clr)) {  // (scalar)
                double jc[7];
#pragma unroll
                for (int q = 0; q < 7; q++) jc[q] = sel ? o.j[q] : 0.0;
                const bool bad = !all_finite(jc);  // rsik_clearance: such a row is NaN
                V3 P[4], e[3];
                path_links(A, jc, P, e);
                const ClrBest B = path_pairs(P, e, K.link_radius, K.n_spheres, K.n_capsules, lds_sph, lds_cap);
                const bool none = B.code < 0;  // every obstacle was skipped
                const int link = none ? 0 : (B.code & 3), obs = none ? 0 : (B.code >> 2);
                clr = (bad || !sel) ? __builtin_nan("") : B.c;
                near_word = (bad || none || !sel) ? ~0ull : ((unsigned long long)(unsigned)obs << 32) | (unsigned)link;  // (link, obstacle)
            }
            if (!out) {
                cand = cand && clr >= K.min_clearance;  // (false for a NaN)
                const double u = K.influence - clr;
                const double p = (K.clearance_gain * u) * u;
                pen = clr < K.influence ? p : 0.0;
                const int n_blocked = __builtin_popcountll(pre) - __builtin_popcountll(__builtin_amdgcn_ballot_w64(cand));
                if (K.blocked != nullptr && lane == 0) K.blocked[row] = (uint8_t)n_blocked;
            }
        }

        if (!out) {
            // ---- forward pass: A of this lane's sample, its backpointer
            const unsigned long long cmask = __builtin_amdgcn_ballot_w64(cand);
            unsigned bp = kPathNone;
            if (cmask != 0) {  // (scalar) a solved waypoint
                double* cur_rows = lds_wave + cs * (64 * kPathRow);
                const double* prev_rows = lds_wave + (cs ^ 1) * (64 * kPathRow);
                double a = __builtin_inf();
                if (cand) {
                    double* mine = cur_rows + lane * kPathRow;
#pragma unroll
                    for (int q = 0; q < 7; q++) mine[q] = o.j[q];
                    if (solved == 0) {
                        a = has_start ? path_cost_at(w, o.j, carry) : 0.0;
                        if constexpr (CLEAR) a = a + pen;
                        bp = kPathFirst;
                    } else {
                        // scalar: the candidates of the previous solved waypoint, ascending; the next one's row is read while this
                        // one's is worked on (the last trip reads its own row again rather than branch)
                        unsigned long long m = pmask;  // != 0
                        int i = __builtin_ctzll(m);
                        m &= m - 1;
                        PathRow pr = path_row(prev_rows + i * kPathRow);
                        for (;;) {
                            const bool more = m != 0;
                            const int i_next = more ? __builtin_ctzll(m) : i;
                            m &= m - 1;
                            const PathRow pr_next = path_row(prev_rows + i_next * kPathRow);
                            const double v = pr.v[3].y + path_cost(w, o.j, pr);
                            if (v < a) { a = v; bp = (unsigned)i; }
                            if (!more) break;
                            pr = pr_next;
                            i = i_next;
                        }
                        if constexpr (CLEAR) a = a + pen;  // the minimum first, then one more sum
                    }
                    mine[7] = a;
                }
                last_a = a;
                pmask = cmask;
                cs ^= 1;
                solved++;
                path_lds_fence();
            }
            if (lane < NT) back[(int64_t)it * NT + lane] = (uint8_t)bp;
        } else {
            // ---- output pass: the winning sample's row
            double* jrow = lds_wave + lane * 7;
            double* erow = lds_wave + 64 * 7 + lane * 3;
            const int t0 = (it - T) << 6;
            const bool won = run && live;
            bool win_projected = false;
            if (won) {
#pragma unroll
                for (int q = 0; q < 7; q++) jrow[q] = o.j[q];
                if (want_elbow) { erow[0] = o.elbow.x; erow[1] = o.elbow.y; erow[2] = o.elbow.z; }
                win_projected = o.projected;
                branch_stores_stay();
            } else {  // a skipped waypoint, a lane past the path's end: NaN
                const double nan = opaque(__builtin_nan(""));
#pragma unroll
                for (int q = 0; q < 7; q++) jrow[q] = nan;
                if (want_elbow) { erow[0] = nan; erow[1] = nan; erow[2] = nan; }
                theta = nan;
                branch_stores_stay();
            }
            path_lds_fence();
            const unsigned long long smask = __builtin_amdgcn_ballot_w64(won);
            double step = __builtin_nan("");
            if (won) {
                const unsigned long long below = smask & ((1ull << lane) - 1ull);
                const double* pr = below ? lds_wave + (63 - __builtin_clzll(below)) * 7 : carry;
                step = (below || have_carry) ? sqrt(path_cost_at(w, o.j, pr)) : 0.0;
            }
            if (live) {
                if (K.index) st_stream(K.index + row, (int32_t)(won ? k : -1));
                if (K.theta) st_stream(K.theta + row, theta);
                if (K.projected) st_stream(K.projected + row, (uint8_t)(win_projected ? 1 : 0));
                if (K.step_cost) st_stream(K.step_cost + row, step);
                if constexpr (CLEAR) {
                    if (K.clearance) st_stream(K.clearance + row, clr);
                    if (K.nearest) st_stream((unsigned long long*)K.nearest + row, near_word);
                }
            }
            path_lds_fence();  // (the carry row has been read)
            if (smask != 0) {
                const int last = 63 - __builtin_clzll(smask);
                if (lane < 7) carry[lane] = lds_wave[last * 7 + lane];
                have_carry = true;
                if (K.unwind && K.joints && lane < 7) {  // sequential along the path: joint `lane` of every solved row, in order
                    unsigned long long m = smask;
                    while (m) {
                        const int rr = __builtin_ctzll(m);
                        m &= m - 1;
                        double v = lds_wave[rr * 7 + lane];
                        if (have_uprev) {
                            v = uprev + angle_diff(v, uprev);  // RSIK_STAGE_ALLOW_MULTITURN's line
                            lds_wave[rr * 7 + lane] = v;
                        }
                        uprev = v;
                        have_uprev = true;
                    }
                }
                if (K.unwind && K.joints) have_uprev = true;
                path_lds_fence();
            }
            // the slab's rows, each to its own waypoint: element e of the slab is entry e % W of waypoint t0 + e / W
            if (K.joints) {
#pragma unroll
                for (int c = 0; c < 7; c++) {
                    const int e = c * 64 + lane;
                    const int rr = e / 7;
                    if (t0 + rr < T) st_stream(K.joints + ((int64_t)(t0 + rr) * n + path) * 7 + (e - rr * 7), lds_wave[e]);
                }
            }
            if (want_elbow) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int e = c * 64 + lane;
                    const int rr = e / 3;
                    if (t0 + rr < T) st_stream(K.elbow + ((int64_t)(t0 + rr) * n + path) * 3 + (e - rr * 3), lds_wave[64 * 7 + e]);
                }
            }
            path_lds_fence();  // (the slabs have been read: the next trip stages its own)
        }
    }
}

}  // namespace rsik
