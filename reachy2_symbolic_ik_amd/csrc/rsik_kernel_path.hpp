// rsik_kernel_path.hpp — rsik_solve_path: n paths of n_steps waypoints, n_theta elbow angles per waypoint, and of the n_theta ^ n_steps
// ways through them the one whose joints move least (solve_path_kernel)
#pragma once

#include "rsik_goal.hpp"
#include "rsik_kernel_nearest.hpp"
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
template <int MIXED, bool TIPZ>
__global__ __launch_bounds__(kBlock, RSIK_PATH_MIN_WAVES) void solve_path_kernel(const PathArgs K) {
    constexpr int PB = kBlock / 64;  // paths per workgroup
    __shared__ SharedTables lds_tab;
    __shared__ __attribute__((aligned(16))) double lds[PB][kPathLds];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t path = (int64_t)blockIdx.x * PB + wave;
    const int64_t pc = path < K.n ? path : K.n - 1;  // (a wave past the end stages the tables with the others, then leaves)

    warm_and_stage_tables<MIXED>(K, lds_tab);
    const AccPath<MIXED> A = kernarg_acc<AccPath<MIXED>, PathArgs>(lds_tab, (MIXED != 0 && K.arm[pc] != 0) ? 1 : 0);
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
