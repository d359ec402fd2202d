// rsik_kernel_path_pair.hpp — rsik_solve_path_pair: rsik_solve_path_clear for robots of two arms whose forearms keep out of each other
// (solve_path_pair_kernel).  Row 2i is the right arm of robot i, row 2i + 1 its left arm (rsik_track_pair's rows); a state of the
// dynamic programme is a PAIR of samples (a of the right arm, b of the left), n_theta^2 <= 256 of them per waypoint, and the
// arm-to-arm distances of those pairs never leave the wave.
//
// path_cost, path_links, path_pairs (rsik_kernel_path.hpp), clr_segment (rsik_kernel_clearance.hpp), pair_swap
// (rsik_kernel_track_pair.hpp) and the sample of solve_path_kernel are called, not restated.
#pragma once

#include "rsik_kernel_path.hpp"
#include "rsik_kernel_track_pair.hpp"  // pair_swap, avoid_pick

namespace rsik {

struct PathPairArgs {
    int64_t n;           // rows: 2 n_pairs
    int64_t n_steps;     // waypoints; every per-waypoint array is [n_steps][n]
    const double* in[6];
    const uint8_t* arm;  // not read: the arm of a row is its parity (kept so that the host's fill_samples serves)
    int theta_policy;
    int n_theta;         // samples per waypoint and arm, 1 ... 16
    int theta_per_pose;
    int skip_projected;
    int unwind;
    const double* theta_in;
    double prev[7];      // zeros
    const double* start; // [n,7] or NULL
    double weights[7];
    uint8_t* back;       // workspace: [n_pairs][n_steps][n_theta^2] backpointers, [n_pairs][n_steps] flags, [n_pairs][n_steps][2] winners
    int32_t* index;
    double* theta;
    double* joints;
    double* elbow;
    uint8_t* projected;
    double* step_cost;
    double* cost;        // [n_pairs]
    int32_t* n_solved;   // [n_pairs]
    double* interval;
    uint8_t* reachable;
    uint8_t* state;
    const double* spheres;
    const double* capsules;
    double* clearance;   // [n_steps][n]
    int32_t* nearest;    // [n_steps][n][2]
    uint16_t* blocked;   // [n_steps][n_pairs]
    int n_spheres, n_capsules;
    double min_clearance, influence, clearance_gain;
    double link_radius[3];
    ArmC arms[2];        // slot 0 = r, slot 1 = l
};

// This kernel's own constant accessor, for AccSweep's reason.  Both arms sit in one wave: every constant comes from LDS.
struct AccPathPair : AccK<1> {};

constexpr int kPairMaxTheta = 16;                         // samples per arm: a backpointer byte holds (a, b), 4 bits each
constexpr int kPairStates = kPairMaxTheta * kPairMaxTheta;
constexpr unsigned kPairSkipped = 0, kPairFirst = 1, kPairLater = 2;  // a waypoint's flag byte: the sentinels a backpointer byte has no room for
// A wave's LDS, in doubles.  The forward pass: the A table, then a region of 2 kPairStates that holds the samples' links and static
// clearances while the states are judged and the B and c tables afterwards, the argmin of stage 1 (ints; the first waypoint's start
// costs before that), two sets of 2 x 16 joint rows (previous, current), the start / carry rows.  The output pass stages its 64 rows
// of 7 + 3 doubles over the front.
constexpr int kPairOffA = 0, kPairOffB = kPairStates, kPairOffC = 2 * kPairStates, kPairOffArg = 3 * kPairStates;
constexpr int kPairOffJ = kPairOffArg + kPairStates / 2, kPairOffCarry = kPairOffJ + 2 * 32 * 7, kPairLds = kPairOffCarry + 16;
constexpr int kPairLink = 12;  // doubles of a sample's links: P[0] and e[0 .. 2]
static_assert(32 * kPairLink + 32 + 16 <= 2 * kPairStates, "links, static clearances and codes fit the B and c tables' place");
static_assert(64 * 10 <= kPairOffCarry, "the output pass's slabs end before the carry rows");

// One view of a pair of samples: the arm (P, e) against the partner's three links as capsules (Q[l], Q[l + 1], rl[l]), obstacle
// indices n_static + l, in clearance_kernel's order and after the static obstacles B already holds — track_pair_kernel's
// construction: the direction is Q1 - Q0, a link with an end that is not a number gets a NaN radius.
__device__ __forceinline__ void pair_view(ClrBest& B, const V3 (&P)[4], const V3 (&e)[3], const V3 (&Q)[4], const double (&rl)[3], int n_static) {
    double ee[3], inv_ee[3];
#pragma unroll
    for (int l = 0; l < 3; l++) { ee[l] = dot(e[l], e[l]); inv_ee[l] = clr_rcp(ee[l]); }
#pragma clang loop unroll(disable)
    for (int lp = 0; lp < 3; lp++) {
        const V3 Q0 = avoid_pick(lp, Q[0], Q[1], Q[2]), Q1 = avoid_pick(lp, Q[1], Q[2], Q[3]);
        const double ends[6] = {Q0.x, Q0.y, Q0.z, Q1.x, Q1.y, Q1.z};
        const double ro = all_finite(ends) ? avoid_pick(lp, rl[0], rl[1], rl[2]) : __builtin_nan("");
        const V3 fq = Q1 - Q0;
        const double ff = dot(fq, fq), inv_ff = clr_rcp(ff);
#pragma unroll
        for (int l = 0; l < 3; l++) clr_segment<false>(B, P[l], e[l], ee[l], inv_ee[l], rl[l], Q0, fq, ff, inv_ff, ro, 4 * (n_static + lp) + l);
    }
}
// a sample's links back from LDS: P[0] and e as path_links left them, P[l + 1] = P[l] + e[l] as it forms them
__device__ __forceinline__ void pair_links_at(const double* p, V3 (&P)[4], V3 (&e)[3]) {
    P[0] = {p[0], p[1], p[2]};
#pragma unroll
    for (int l = 0; l < 3; l++) { e[l] = {p[3 + 3 * l], p[4 + 3 * l], p[5 + 3 * l]}; P[l + 1] = P[l] + e[l]; }
}
__device__ __forceinline__ void pair_joints_at(const double* p, double (&j)[7]) {
#pragma unroll
    for (int q = 0; q < 7; q++) j[q] = p[q];
}

// One wave = one robot, kBlock / 64 robots per workgroup; one loop runs both passes, as in solve_path_kernel, so that a sample is the
// same instructions in both and has rsik_solve_sweep's bits.
//
// Trips 0 ... n_steps - 1, the forward pass, waypoint t:
//   samples   lane 16 s + k (s = 0 right, 1 left; k < n_theta) runs sample k of row 2i + s: solve_path_kernel's sample, the row
//             candidate rule, path_links and path_pairs over the staged static scene.  Joints, links, static clearance and code go to LDS.
//   states    state a n_theta + b sits in lane s & 63, slot s >> 6.  Where both samples are row candidates the lane forms both views
//             (pair_view on top of the sample's static result: the minimum is exact and the static obstacles come first, so this is
//             rsik_clearance's pair loop cut in two), the mask and the penalty pR + pL.  `blocked` is a difference of ballots.
//   tables    a waypoint with a candidate pair (one ballot; without one the tables stay): c of the left arm, n_theta^2 path_costs, one
//             per state; stage 1, B(a, b') = min_b A(a, b) + cL(b, b'); c of the right arm in the same place; stage 2,
//             A'(a', b') = (min_a B(a, b') + cR(a, a')) + p.  Ascending loops and strict compares: ties go to the lowest index.  A pair
//             that is no candidate holds +infinity and never wins.  One backpointer byte per state, one flag byte per waypoint.
// Trip n_steps starts with the end of the path (nearest_of_group over the A table) and the backtrack, one dependent byte per waypoint.
// Trips n_steps ..., the output pass: lane 2 v + s holds row 2i + s of waypoint 32 (trip - n_steps) + v and runs its winning sample
// again; the two lanes of a waypoint swap their link points in registers (pair_swap) for clearance and nearest; step costs, the
// unwinding and the stores are solve_path_kernel's with two rows per waypoint.
// Every sum has a fixed order, there is no atomic, and every branch is wave-uniform but the far-angle one of path_links and the
// rare fix-up of path_cost.
template <bool TIPZ>
__global__ __launch_bounds__(kBlock, 1) void solve_path_pair_kernel(const PathPairArgs K) {
    constexpr int PB = kBlock / 64;  // robots per workgroup
    __shared__ SharedTables lds_tab;
    __shared__ __attribute__((aligned(16))) double lds[PB][kPairLds];
    __shared__ __attribute__((aligned(16))) double lds_sph[kAvoidMaxSpheres * 4];
    __shared__ __attribute__((aligned(16))) double lds_cap[kAvoidMaxCapsules * 8];
    static_assert(sizeof(SharedTables) + sizeof(g_sincos_tab) + sizeof(double) * (PB * kPairLds + kAvoidMaxSpheres * 4 + kAvoidMaxCapsules * 8) <= 64 * 1024,
                  "the static LDS of a workgroup: tables, the waves' regions and the staged scene");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n = K.n, n_pairs = K.n >> 1;
    const int64_t robot = (int64_t)blockIdx.x * PB + wave;

    for (int o = threadIdx.x; o < K.n_spheres; o += kBlock) {  // the scene, once, as solve_path_kernel stages it
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
    stage_tables<true>(lds_tab, K.arms);  // (ends with the barrier that also stands behind the scene)
    if (robot >= n_pairs) return;         // (wave-uniform; no workgroup barrier follows)

    double* L = lds[wave];
    double* tabA = L + kPairOffA;
    double* tabB = L + kPairOffB;
    double* tabC = L + kPairOffC;
    double* links = L + kPairOffB;                   // [32][kPairLink], while the states are judged
    double* sclr = links + 32 * kPairLink;           // [32]
    int* scode = reinterpret_cast<int*>(sclr + 32);  // [32]
    int* argB = reinterpret_cast<int*>(L + kPairOffArg);
    double* c0 = L + kPairOffArg;                    // [32]: the start costs, at the first solved waypoint only
    double* jsets = L + kPairOffJ;                   // [2][32][7]
    double* carry = L + kPairOffCarry;               // [2][7]
    const int T = (int)K.n_steps;
    const int NT = K.n_theta, KK = NT * NT;
    const bool want_elbow = K.elbow != nullptr;
    const bool fraction = K.theta_policy != RSIK_THETA_EXPLICIT;
    const bool per_pose = K.theta_per_pose != 0;
    const bool skip_projected = K.skip_projected != 0;
    const bool has_start = K.start != nullptr;
    const int n_static = K.n_spheres + K.n_capsules;
    uint8_t* back = K.back + robot * T * KK;                              // [T][KK]
    uint8_t* flags = K.back + n_pairs * T * KK + robot * T;               // [T]
    uint8_t* winners = K.back + n_pairs * T * (KK + 1) + robot * T * 2;   // [T][2]
    double w[7];
#pragma unroll
    for (int q = 0; q < 7; q++) w[q] = K.weights[q];

    // the two start rows: lane 7 s + q keeps entry q of row 2i + s
    double uprev = 0.0;
    bool lost = false;  // rsik.h: a start row that holds something that is not a number loses the robot
    if (has_start) {
        if (lane < 14) {
            uprev = K.start[robot * 14 + lane];
            carry[lane] = uprev;
        }
        lost = __builtin_amdgcn_ballot_w64(lane < 14 && !(fabs(uprev) < __builtin_inf())) != 0;
        path_lds_fence();
    }

    int cs = 0;      // the joint set the next solved waypoint writes
    int solved = 0;  // solved waypoints so far
    bool have_carry = has_start, have_uprev = has_start;
    const int trips = (T + 31) >> 5;
#pragma clang loop unroll(disable)
    for (int it = 0; it < T + trips; it++) {
        const bool out = it >= T;  // scalar
        if (it == T) {
            // ---- the end of the forward pass: the least A, ties to the lowest state; then the winners, backwards
            double end_a = __builtin_inf();
            int end_s = kNoSample;
            if (solved) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int s = lane + 64 * j;
                    const double a = s < KK ? tabA[s] : __builtin_inf();
                    if (a < end_a) { end_a = a; end_s = s; }
                }
            }
            nearest_of_group<64>(end_a, end_s);
            if (lane == 0) {
                if (K.cost) st_stream(K.cost + robot, solved ? end_a : __builtin_nan(""));
                if (K.n_solved) st_stream(K.n_solved + robot, (int32_t)solved);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");  // the table's bytes, written by other lanes of this wave
            int cur = __builtin_amdgcn_readfirstlane(end_s);
            for (int t = T - 1; t >= 0; t--) {
                const unsigned fl = (unsigned)__builtin_amdgcn_readfirstlane((int)flags[t]);
                unsigned wa = 0xffu, wb = 0xffu;
                if (fl != kPairSkipped && cur < KK) {
                    wa = (unsigned)cur / (unsigned)NT;
                    wb = (unsigned)cur - wa * (unsigned)NT;
                    if (fl == kPairLater) {
                        const unsigned bp = (unsigned)__builtin_amdgcn_readfirstlane((int)back[(int64_t)t * KK + cur]);
                        cur = (int)((bp >> 4) * (unsigned)NT + (bp & 15u));
                    }
                }
                if (lane < 2) winners[t * 2 + lane] = (uint8_t)(lane ? wb : wa);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
            path_lds_fence();
        }
        // ---- which row, waypoint and sample this lane takes
        const int side = out ? (lane & 1) : ((lane >> 4) & 1);
        const int wp_raw = out ? ((it - T) << 5) + (lane >> 1) : it;
        const bool live = wp_raw < T;  // (the forward pass: every lane)
        const int wp = live ? wp_raw : T - 1;
        int k = lane < 32 ? (lane & 15) : (int)kPathNone;
        if (out) k = live ? (int)winners[wp * 2 + side] : (int)kPathNone;
        const int64_t row = (int64_t)wp * n + 2 * robot + side;  // of every [n_steps][n] array
        AccPathPair A = kernarg_acc<AccPathPair, PathPairArgs>(lds_tab, 0);
        A.lds = (LdsConst)lds_tab.arm[side];

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
        // ---- its links and its clearance to the static scene
        const bool want_clr = K.clearance != nullptr || K.nearest != nullptr;
        const bool sel = out ? (run && live) : cand;  // the lanes whose links are used
        const unsigned long long pre = __builtin_amdgcn_ballot_w64(sel);
        V3 P[4] = {}, e[3] = {};
        ClrBest B = {__builtin_inf(), 0.0, 0.0, -1};
        bool bad = false;
        const bool links_wanted = pre != 0 && (!out || want_clr);  // (scalar)
        if (links_wanted) {
            double jc[7];
#pragma unroll
            for (int q = 0; q < 7; q++) jc[q] = sel ? o.j[q] : 0.0;
            bad = !all_finite(jc);  // rsik_clearance: such a row is NaN, and so are its link points
            path_links(A, jc, P, e);
            B = path_pairs(P, e, K.link_radius, K.n_spheres, K.n_capsules, lds_sph, lds_cap);
        }

        if (!out) {
            // ---- forward pass.  The samples' rows into LDS
            double* cur_j = jsets + cs * (32 * 7);
            const double* prev_j = jsets + (cs ^ 1) * (32 * 7);
            if (lane < 32 && k < NT) {
#pragma unroll
                for (int q = 0; q < 7; q++) cur_j[lane * 7 + q] = cand ? o.j[q] : 0.0;
                if (links_wanted) {
                    double* lp = links + lane * kPairLink;
                    lp[0] = P[0].x; lp[1] = P[0].y; lp[2] = P[0].z;
#pragma unroll
                    for (int l = 0; l < 3; l++) { lp[3 + 3 * l] = e[l].x; lp[4 + 3 * l] = e[l].y; lp[5 + 3 * l] = e[l].z; }
                    sclr[lane] = bad ? __builtin_nan("") : B.c;
                    scode[lane] = B.code;
                }
                if (solved == 0 && has_start) c0[lane] = cand ? path_cost_at(w, o.j, carry + side * 7) : 0.0;
                branch_stores_stay();
            }
            path_lds_fence();
            // the states
            const unsigned long long rmask = pre;  // row candidates: bits 0 ... 15 right, 16 ... 31 left
            double pen0 = 0.0, pen1 = 0.0, pen2 = 0.0, pen3 = 0.0;
            unsigned cpm = 0;  // bit j: state lane + 64 j is a candidate pair
            int n_row = 0, n_cand = 0;
#pragma clang loop unroll(disable)
            for (int j = 0; j < 4; j++) {
                const int s = lane + 64 * j;
                const bool valid = s < KK;
                const unsigned sa = valid ? (unsigned)s / (unsigned)NT : 0u;
                const unsigned sb = valid ? (unsigned)s - sa * (unsigned)NT : 0u;
                const bool rc = valid && ((rmask >> sa) & 1ull) != 0 && ((rmask >> (16 + sb)) & 1ull) != 0;
                const unsigned long long rcm = __builtin_amdgcn_ballot_w64(rc);
                if (rcm == 0) continue;  // (scalar)
                V3 PR[4], eR[3], PL[4], eL[3];
                pair_links_at(links + sa * kPairLink, PR, eR);
                pair_links_at(links + (16 + sb) * kPairLink, PL, eL);
                const double sR = sclr[sa], sL = sclr[16 + sb];
                const double nan = __builtin_nan("");
                V3 QR[4], QL[4];  // what rsik_clearance returns as link_points: NaN for a row that is not numbers
#pragma unroll
                for (int l = 0; l < 4; l++) {
                    QR[l] = {sR == sR ? PR[l].x : nan, sR == sR ? PR[l].y : nan, sR == sR ? PR[l].z : nan};
                    QL[l] = {sL == sL ? PL[l].x : nan, sL == sL ? PL[l].y : nan, sL == sL ? PL[l].z : nan};
                }
                ClrBest BR = {sR, 0.0, 0.0, scode[sa]}, BL = {sL, 0.0, 0.0, scode[16 + sb]};
                pair_view(BR, PR, eR, QL, K.link_radius, n_static);
                pair_view(BL, PL, eL, QR, K.link_radius, n_static);
                const double dR = BR.c, dL = BL.c;  // (a NaN static part stays a NaN: clr_take never replaces it)
                const bool cp = rc && dR >= K.min_clearance && dL >= K.min_clearance;  // (false for a NaN)
                const double uR = K.influence - dR, uL = K.influence - dL;
                const double pR = dR < K.influence ? (K.clearance_gain * uR) * uR : 0.0;
                const double pL = dL < K.influence ? (K.clearance_gain * uL) * uL : 0.0;
                const double p = pR + pL;
                pen0 = j == 0 ? p : pen0; pen1 = j == 1 ? p : pen1; pen2 = j == 2 ? p : pen2; pen3 = j == 3 ? p : pen3;
                cpm |= cp ? (1u << j) : 0u;
                n_row += __builtin_popcountll(rcm);
                n_cand += __builtin_popcountll(__builtin_amdgcn_ballot_w64(cp));
            }
            if (K.blocked != nullptr && lane == 0) K.blocked[(int64_t)it * n_pairs + robot] = (uint16_t)(n_row - n_cand);
            path_lds_fence();  // (the links have been read: the tables take their place)

            unsigned fl = kPairSkipped;
            unsigned bp0 = 0, bp1 = 0, bp2 = 0, bp3 = 0;
            if (n_cand != 0) {  // (scalar) a solved waypoint
                double a0 = __builtin_inf(), a1 = a0, a2 = a0, a3 = a0;
                if (solved == 0) {
                    fl = kPairFirst;
#pragma clang loop unroll(disable)
                    for (int j = 0; j < 4; j++) {
                        const int s = lane + 64 * j;
                        const bool valid = s < KK;
                        const unsigned sa = valid ? (unsigned)s / (unsigned)NT : 0u;
                        const unsigned sb = valid ? (unsigned)s - sa * (unsigned)NT : 0u;
                        const double p = j == 0 ? pen0 : j == 1 ? pen1 : j == 2 ? pen2 : pen3;
                        double a = has_start ? (c0[sa] + c0[16 + sb]) + p : p;
                        a = ((cpm >> j) & 1u) ? a : __builtin_inf();
                        a0 = j == 0 ? a : a0; a1 = j == 1 ? a : a1; a2 = j == 2 ? a : a2; a3 = j == 3 ? a : a3;
                    }
                    path_lds_fence();  // (the start costs have been read)
                } else {
                    fl = kPairLater;
                    // the left arm's transitions into tabC: entry b NT + b' = cL(JLprev[b], JL[b'])
#pragma clang loop unroll(disable)
                    for (int j = 0; j < 4; j++) {
                        const int s = lane + 64 * j;
                        if (s < KK) {
                            const unsigned sa = (unsigned)s / (unsigned)NT, sb = (unsigned)s - sa * (unsigned)NT;
                            double jb[7], ja[7];
                            pair_joints_at(cur_j + (16 + sb) * 7, jb);
                            pair_joints_at(prev_j + (16 + sa) * 7, ja);
                            tabC[s] = path_cost(w, jb, ja);
                        }
                    }
                    path_lds_fence();
                    // stage 1: B(a, b') = min_b A(a, b) + cL(b, b')
#pragma clang loop unroll(disable)
                    for (int j = 0; j < 4; j++) {
                        const int s = lane + 64 * j;
                        if (s < KK) {
                            const unsigned sa = (unsigned)s / (unsigned)NT, sb = (unsigned)s - sa * (unsigned)NT;
                            double best = __builtin_inf();
                            int arg = 0;
                            for (int b = 0; b < NT; b++) {
                                const double v = tabA[sa * NT + b] + tabC[b * NT + sb];
                                if (v < best) { best = v; arg = b; }
                            }
                            tabB[s] = best;
                            argB[s] = arg;
                        }
                    }
                    path_lds_fence();
                    // the right arm's transitions in the same place: entry a NT + a' = cR(JRprev[a], JR[a'])
#pragma clang loop unroll(disable)
                    for (int j = 0; j < 4; j++) {
                        const int s = lane + 64 * j;
                        if (s < KK) {
                            const unsigned sa = (unsigned)s / (unsigned)NT, sb = (unsigned)s - sa * (unsigned)NT;
                            double jb[7], ja[7];
                            pair_joints_at(cur_j + sb * 7, jb);
                            pair_joints_at(prev_j + sa * 7, ja);
                            tabC[s] = path_cost(w, jb, ja);
                        }
                    }
                    path_lds_fence();
                    // stage 2: A'(a', b') = (min_a B(a, b') + cR(a, a')) + p(a', b')
#pragma clang loop unroll(disable)
                    for (int j = 0; j < 4; j++) {
                        const int s = lane + 64 * j;
                        const bool valid = s < KK;
                        const unsigned sa = valid ? (unsigned)s / (unsigned)NT : 0u;
                        const unsigned sb = valid ? (unsigned)s - sa * (unsigned)NT : 0u;
                        double best = __builtin_inf();
                        int arg = 0;
                        for (int a = 0; a < NT; a++) {
                            const double v = tabB[a * NT + sb] + tabC[a * NT + sa];
                            if (v < best) { best = v; arg = a; }
                        }
                        const double p = j == 0 ? pen0 : j == 1 ? pen1 : j == 2 ? pen2 : pen3;
                        const double a = ((cpm >> j) & 1u) ? best + p : __builtin_inf();
                        const unsigned bp = ((unsigned)arg << 4) | (unsigned)argB[arg * NT + sb];
                        a0 = j == 0 ? a : a0; a1 = j == 1 ? a : a1; a2 = j == 2 ? a : a2; a3 = j == 3 ? a : a3;
                        bp0 = j == 0 ? bp : bp0; bp1 = j == 1 ? bp : bp1; bp2 = j == 2 ? bp : bp2; bp3 = j == 3 ? bp : bp3;
                    }
                    path_lds_fence();  // (every read of the old A table is done)
                }
                if (lane < KK) tabA[lane] = a0;
                if (lane + 64 < KK) tabA[lane + 64] = a1;
                if (lane + 128 < KK) tabA[lane + 128] = a2;
                if (lane + 192 < KK) tabA[lane + 192] = a3;
                cs ^= 1;
                solved++;
                path_lds_fence();
            }
            uint8_t* brow = back + (int64_t)it * KK;
            if (lane < KK) brow[lane] = (uint8_t)bp0;
            if (lane + 64 < KK) brow[lane + 64] = (uint8_t)bp1;
            if (lane + 128 < KK) brow[lane + 128] = (uint8_t)bp2;
            if (lane + 192 < KK) brow[lane + 192] = (uint8_t)bp3;
            if (lane == 0) flags[it] = (uint8_t)fl;
        } else {
            // ---- output pass: the winning sample's row; its clearance with the partner's links behind the static scene
            const bool won = run && live;
            double clr = __builtin_nan("");
            unsigned long long near_word = ~0ull;
            if (want_clr) {  // (scalar; every lane is here: pair_swap)
                const double nan = __builtin_nan("");
                const bool shown = links_wanted && !bad && won;
                V3 Q[4], Pn[4];
#pragma unroll
                for (int l = 0; l < 4; l++) {
                    Pn[l] = {shown ? P[l].x : nan, shown ? P[l].y : nan, shown ? P[l].z : nan};
                    Q[l] = pair_swap(Pn[l]);
                }
                if (links_wanted) {
                    pair_view(B, P, e, Q, K.link_radius, n_static);
                    const bool none = B.code < 0;  // every obstacle was skipped
                    const int link = none ? 0 : (B.code & 3), obs = none ? 0 : (B.code >> 2);
                    clr = (bad || !won) ? nan : B.c;
                    near_word = (bad || none || !won) ? ~0ull : ((unsigned long long)(unsigned)obs << 32) | (unsigned)link;  // (link, obstacle)
                }
            }
            double* jrow = L + lane * 7;
            double* erow = L + 64 * 7 + lane * 3;
            const int t0 = (it - T) << 5;
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
            const unsigned long long mine_side = 0x5555555555555555ull << side;  // the lanes of this lane's arm
            double step = __builtin_nan("");
            if (won) {
                const unsigned long long below = smask & mine_side & ((1ull << lane) - 1ull);
                const double* pr = below ? L + (63 - __builtin_clzll(below)) * 7 : carry + side * 7;
                step = (below || have_carry) ? sqrt(path_cost_at(w, o.j, pr)) : 0.0;
            }
            if (live) {
                if (K.index) st_stream(K.index + row, (int32_t)(won ? k : -1));
                if (K.theta) st_stream(K.theta + row, theta);
                if (K.projected) st_stream(K.projected + row, (uint8_t)(win_projected ? 1 : 0));
                if (K.step_cost) st_stream(K.step_cost + row, step);
                if (K.clearance) st_stream(K.clearance + row, clr);
                if (K.nearest) st_stream((unsigned long long*)K.nearest + row, near_word);
            }
            path_lds_fence();  // (the carry rows have been read)
            const unsigned long long rmask_r = smask & 0x5555555555555555ull;  // solved waypoints of this trip, by their right arm's lane
            if (rmask_r != 0) {
                const int last = 63 - __builtin_clzll(rmask_r);  // the right arm's lane of the last solved waypoint
                if (lane < 14) carry[lane] = L[(last + (lane >= 7 ? 1 : 0)) * 7 + (lane >= 7 ? lane - 7 : lane)];
                have_carry = true;
                if (K.unwind && K.joints && lane < 14) {  // sequential along the path: lane 7 s + q walks joint q of arm s
                    const int us = lane >= 7 ? 1 : 0, uq = lane - 7 * us;
                    unsigned long long m = rmask_r;
                    while (m) {
                        const int rr = __builtin_ctzll(m) + us;
                        m &= m - 1;
                        double v = L[rr * 7 + uq];
                        if (have_uprev) {
                            v = uprev + angle_diff(v, uprev);  // RSIK_STAGE_ALLOW_MULTITURN's line
                            L[rr * 7 + uq] = v;
                        }
                        uprev = v;
                        have_uprev = true;
                    }
                }
                if (K.unwind && K.joints) have_uprev = true;
                path_lds_fence();
            }
            // the slab's rows: element x of the slab is entry x % W of row 2i + (x / W & 1) of waypoint t0 + x / W / 2
            if (K.joints) {
#pragma unroll
                for (int c = 0; c < 7; c++) {
                    const int x = c * 64 + lane;
                    const int rr = x / 7;
                    if (t0 + (rr >> 1) < T) st_stream(K.joints + ((int64_t)(t0 + (rr >> 1)) * n + 2 * robot + (rr & 1)) * 7 + (x - rr * 7), L[x]);
                }
            }
            if (want_elbow) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int x = c * 64 + lane;
                    const int rr = x / 3;
                    if (t0 + (rr >> 1) < T) st_stream(K.elbow + ((int64_t)(t0 + (rr >> 1)) * n + 2 * robot + (rr & 1)) * 3 + (x - rr * 3), L[64 * 7 + x]);
                }
            }
            path_lds_fence();  // (the slabs have been read: the next trip stages its own)
        }
    }
}

}  // namespace rsik
