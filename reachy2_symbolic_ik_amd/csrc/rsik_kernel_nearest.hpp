// rsik_kernel_nearest.hpp — rsik_solve_nearest: is_reachable once per pose, get_joints at n_theta elbow angles, and of those the one
// solution nearest to the pose's seed joints (solve_nearest_kernel)
#pragma once

#include "rsik_goal.hpp"
#include "rsik_rows.hpp"
#include "rsik_tables.hpp"

namespace rsik {

struct NearestArgs {
    int64_t n;
    const double* in[6];
    const uint8_t* arm;
    int theta_policy;    // RSIK_THETA_EXPLICIT or RSIK_THETA_FRACTION
    int n_theta;         // samples per pose, >= 1
    int theta_per_pose;  // 0: theta_in[n_theta], one value per sample for every pose; else theta_in[n_theta][n]
    int skip_projected;  // RSIK_NEAREST_SKIP_PROJECTED: a sample whose elbow projection fired is no candidate
    const double* theta_in;
    union {
        double prev[7];           // previous_joints == NULL: zeros
        const double* prev_rows;  // PREV_ROWS kernels: [n,7] device, one row per pose, shared by the pose's samples
    };
    const double* seed;  // [n,7]: the joints each pose wants to stay near
    double weights[7];   // of the squared joint differences
    int32_t* index;      // [n] or NULL: the winning sample, -1 without a candidate
    double* theta;       // [n] or NULL
    double* joints;      // [n,7] or NULL
    double* elbow;       // [n,3] or NULL
    double* cost;        // [n] or NULL: sqrt of the winner's weighted sum
    uint8_t* projected;  // [n] or NULL
    double* interval;    // [n][2] or NULL
    uint8_t* reachable;  // [n] or NULL
    uint8_t* state;      // [n] or NULL
    ArmC arms[2];        // as SolveArgs.arms
};

// This kernel's own constant accessor, for AccSweep's reason: the device functions templated on the accessor get instantiations of
// their own here, and the ones the other kernels use keep their callers.
template <int MIXED>
struct AccNearest : AccK<MIXED> {};

constexpr int kNoSample = 0x7fffffff;  // the k of a lane (a pose) that holds no candidate: beyond every n_theta

// (c, k) < (bc, bk), lexicographically: the smaller cost, the lower sample among equal costs.  A NaN c is never nearer.
__device__ __forceinline__ bool nearer(double c, int k, double bc, int bk) { return c < bc || (c == bc && k < bk); }

// The minimum of (c, k) under `nearer` over the L consecutive lanes of a pose, left in every one of them: a total order, so the
// result does not depend on how the samples were dealt to the lanes.
template <int L>
__device__ __forceinline__ void nearest_of_group(double& c, int& k) {
#pragma unroll
    for (int off = L / 2; off >= 1; off >>= 1) {
        const double oc = __shfl_xor(c, off, 64);
        const int ok = __shfl_xor(k, off, 64);
        if (nearer(oc, ok, c, k)) { c = oc; k = ok; }
    }
}

// solve_sweep_kernel's head (loads, goal stage, reach_g once per pose) and its sample (get_joints on a copy of the wrist reach_g left,
// so a sample is, bit for bit, what rsik_solve_sweep writes for it), but nothing is stored per sample: each sample's joints go into
//     c = sum_q w_q d_q d_q,   d_q = angle_diff(joints_q, seed_q),   q = 0 ... 6 in that order, unfused,
// and a lane carries only the nearest (c, k) it has seen.  The winner's row is not carried (28 registers): the loop's LAST trip
// evaluates the winning sample once more — the same function on the same operands, the sweep's bits again, 1 / n_theta of the work —
// and stages the one row per pose, which leaves through the LDS slabs as solve_kernel's does.
//
// L lanes per pose (1, 8 or 64; kBlock / L poses per workgroup, 64 / L per wave): the L lanes of a pose hold the same pose (each
// runs the head), lane l takes the samples k = l, l + L, ..., the group reduces its (c, k) with nearest_of_group and every lane of
// it runs the last trip on the same k; lane 0 of the group stores.  Every sample's c comes from the same instructions whatever L
// is and the order is total, so all outputs, index included, are the same bits for every L.
//
// The pose's seed row waits in LDS, in the slab its joints row later takes: read back per sample (7 ds_reads against the thousand
// instructions of a sample), it costs no registers across the loop.
#ifndef RSIK_NEAREST_MIN_WAVES
#define RSIK_NEAREST_MIN_WAVES 1
#endif
template <int MIXED, bool TIPZ, bool PREV_ROWS, int L>
__global__ __launch_bounds__(kBlock, RSIK_NEAREST_MIN_WAVES) void solve_nearest_kernel(const NearestArgs K) {
    static_assert(L == 1 || L == 8 || L == 64, "lanes per pose");
    constexpr int PW = 64 / L;      // poses per wave
    constexpr int PB = kBlock / L;  // poses per workgroup
    __shared__ SharedTables lds_tab;
    __shared__ double lds[kBlock / 64][64 * 10];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile0 = (int64_t)blockIdx.x * PB;
    const int64_t left = K.n - tile0;                               // >= 1 (grid = ceil(n / PB))
    const unsigned rows = left < PB ? (unsigned)left : (unsigned)PB;
    const unsigned sub = (unsigned)lane & (L - 1);                  // this lane's place among the L lanes of its pose
    const unsigned pw = (unsigned)lane / L;                         // the pose's place in the wave
    const unsigned t = (unsigned)wave * PW + pw;                    // and in the tile
    const unsigned tt = (t < rows ? t : rows - 1) & (PB - 1);       // clamped pose index inside the tile
    const bool lead = sub == 0;
    const bool live = t < rows && lead;                             // the lanes that store

    double in[6];
#pragma unroll
    for (int k = 0; k < 6; k++) in[k] = ld_stream(K.in[k] + tile0 + tt);
    warm_and_stage_tables<MIXED>(K, lds_tab);
    const AccNearest<MIXED> A = kernarg_acc<AccNearest<MIXED>, NearestArgs>(lds_tab, (MIXED != 0 && K.arm[tile0 + tt] != 0) ? 1 : 0);
    double* lds_wave = lds[wave];

    const bool invalid = settle_pose(in);  // rsik.h "Rows that are not numbers"
    const V3 pos = {in[0], in[1], in[2]};
    const Goal G = goal_of_pose<TIPZ>(A, in[3], in[4], in[5]);
    Reach r = reach_g<false, false>(A, pos, G.woff);
    if (RSIK_RARE(invalid)) reach_invalid_input(r);
    store_reach(K, live, tile0, t, r);
    if (rows <= (unsigned)(wave * PW)) return;  // a wave past the end of the batch (wave-uniform; no barrier follows)

    const int wave_rows = rows - wave * PW < PW ? (int)(rows - wave * PW) : PW;  // poses of this wave that exist (scalar), >= 1
    const int64_t wave_base = tile0 + wave * PW;
    // the wave's seed rows: one contiguous run of wave_rows x 7 doubles into the joints slab
    {
        const double* src = K.seed + wave_base * 7;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            if (k * 64 < PW * 7) {
                const int idx = k * 64 + lane;
                if (idx < wave_rows * 7) lds_wave[idx] = ld_stream(src + idx);
            }
        }
        wave_lds_fence();
    }
    const double* seed = lds_wave + (tt - wave * PW) * 7;  // (clamped: a lane past the end reads the last pose's row, as it solves that pose)
    double* jrow = lds_wave + pw * 7;
    double* erow = lds_wave + 64 * 7 + pw * 3;

    const bool want_elbow = K.elbow != nullptr;
    const bool fraction = K.theta_policy != RSIK_THETA_EXPLICIT;
    const bool per_pose = K.theta_per_pose != 0;
    const bool skip_projected = K.skip_projected != 0;
    // the fraction arithmetic's two operands, as solve_kernel forms them per launch: theta = a + u * (b - a)
    const double fa = r.i0;
    double fb = r.i1;
    if (fa > fb) fb += kTwoPi;
    const double fspan = fb - fa;
    const V3 wrist = r.w;
    const double* th_col = K.theta_in + tile0 + tt;  // per-pose form: this pose's entry of sample 0

    double best_c = __builtin_inf();
    int best_k = kNoSample;
    double win_theta = __builtin_nan("");
    bool win_projected = false, won = false;
    const int rounds = (K.n_theta + L - 1) / L;  // trips that deal samples to the lanes; trip `rounds` is the winner's
#pragma clang loop unroll(disable)
    for (int it = 0; it <= rounds; it++) {
        const bool last = it == rounds;
        if (last) {
            if constexpr (L > 1) nearest_of_group<L>(best_c, best_k);
        }
        const int k = last ? best_k : it * L + (int)sub;
        if (r.ok && k < K.n_theta) {  // (a lane the samples do not reach; a pose without a candidate: kNoSample)
            const double th_in = per_pose ? th_col[(int64_t)k * K.n] : K.theta_in[k];
            double theta = th_in;
            if (fraction) theta = fa + th_in * fspan;
            double ct, st;
            fast_sincos(near_angle(theta), &st, &ct);
            r.w = wrist;
            JointsOut o;
            if constexpr (PREV_ROWS) o = joints_from_theta_g<true, TIPZ>(A, r, G, ct, st, (GConst)(K.prev_rows + (tile0 + tt) * 7));
            else o = joints_from_theta_g<true, TIPZ>(A, r, G, ct, st, (const double*)K.prev);
            if (!last) {
                double c = 0.0;
#pragma unroll
                for (int q = 0; q < 7; q++) {
                    const double d = angle_diff(o.j[q], seed[q]);
                    c = c + (K.weights[q] * d) * d;
                }
                if (!(skip_projected && o.projected) && nearer(c, k, best_c, best_k)) { best_c = c; best_k = k; }
            } else {
                won = true;
                win_theta = theta;
                win_projected = o.projected;
                if (lead) {  // (the seed rows have been read for the last time: every lane of the wave is in this trip)
#pragma unroll
                    for (int q = 0; q < 7; q++) jrow[q] = o.j[q];
                    if (want_elbow) { erow[0] = o.elbow.x; erow[1] = o.elbow.y; erow[2] = o.elbow.z; }
                }
            }
        }
        branch_stores_stay();  // (also keeps the seed row's reads inside the loop: hoisted, they are 14 registers carried through it)
    }
    if (!won && lead) {  // no candidate: NaN — staged once
        const double nan = opaque(__builtin_nan(""));
#pragma unroll
        for (int q = 0; q < 7; q++) jrow[q] = nan;
        if (want_elbow) { erow[0] = nan; erow[1] = nan; erow[2] = nan; }
        branch_stores_stay();
    }
    if (L == 1 && wave_rows == 64) {
        if (K.joints) flush_rows_full<7>(K.joints, wave_base, lane, lds_wave);
        if (want_elbow) flush_rows_full<3>(K.elbow, wave_base, lane, lds_wave + 64 * 7);
    } else {
        if (K.joints) flush_pose_rows<7, PW>(K.joints, wave_base, wave_rows, lane, lds_wave);
        if (want_elbow) flush_pose_rows<3, PW>(K.elbow, wave_base, wave_rows, lane, lds_wave + 64 * 7);
    }
    if (live) {
        if (K.index) st_stream(K.index + tile0 + t, (int32_t)(won ? best_k : -1));
        if (K.theta) st_stream(K.theta + tile0 + t, win_theta);
        if (K.cost) st_stream(K.cost + tile0 + t, won ? sqrt(best_c) : __builtin_nan(""));
        if (K.projected) st_stream(K.projected + tile0 + t, (uint8_t)(win_projected ? 1 : 0));
    }
}

}  // namespace rsik
