// rsik_kernel_sweep.hpp — rsik_solve_sweep: is_reachable once per pose, then get_joints at n_theta elbow angles (solve_sweep_kernel)
#pragma once

#include "rsik_goal.hpp"
#include "rsik_rows.hpp"
#include "rsik_tables.hpp"

namespace rsik {

struct SweepArgs {
    int64_t n;
    const double* in[6];
    const uint8_t* arm;
    int theta_policy;    // RSIK_THETA_EXPLICIT or RSIK_THETA_FRACTION
    int n_theta;         // samples per pose, >= 1
    int theta_per_pose;  // 0: theta_in[n_theta], one value per sample for every pose; else theta_in[n_theta][n]
    const double* theta_in;
    union {
        double prev[7];           // previous_joints == NULL: zeros
        const double* prev_rows;  // PREV_ROWS kernels: [n,7] device, one row per pose, shared by the pose's samples
    };
    double* joints;      // [n_theta][n][7]
    double* elbow;       // [n_theta][n][3] or NULL
    uint8_t* projected;  // [n_theta][n] or NULL
    double* theta;       // [n_theta][n] or NULL
    double* interval;    // [n][2] or NULL
    uint8_t* reachable;  // [n] or NULL
    uint8_t* state;      // [n] or NULL
    ArmC arms[2];        // as SolveArgs.arms
};

// The sweep's own constant accessor: AccK's behaviour under another type, so that every device function templated on the accessor
// (reach_g, joints_from_theta_g, the goal stage ...) gets an instantiation of its own here and the ones solve_kernel, the discrete
// kernel and the pipeline kernels use keep their single caller — sharing one changes how those kernels are compiled.
template <int MIXED>
struct AccSweep : AccK<MIXED> {};

// One workgroup = one tile of kBlock consecutive poses, one pose per lane: solve_kernel's geometry, loads and reachability stage,
// run ONCE per pose; then a loop over the n_theta samples, each of them solve_kernel's get_joints stage on the wrist reach_g left
// (joints_from_theta_g<true> moves r.w where the elbow projection fires: every sample starts from a copy, so that a projected
// sample leaves nothing behind for the next one and the samples do not depend on their order).  Sample k of pose i is, bit for
// bit, what solve_kernel writes for pose i with theta_in = that sample's value: the same functions on the same operands, and
// the library is compiled without contraction.
// Outputs are sample-major: sample k's joints are the contiguous [n,7] array at joints + k n 7, written slab by slab per wave
// exactly as solve_kernel writes its one array.  The per-pose outputs (interval, reachable, state) are written once, ahead of
// the loop, which ends their registers' lives there.
// Every sample's cos / sin come from fast_sincos(theta) — also at fraction 0, where solve_kernel's RSIK_THETA_INTERVAL0 would
// take them from the intersection point: RSIK_THETA_FRACTION with 0 does the same there.
#ifndef RSIK_SWEEP_MIN_WAVES
#define RSIK_SWEEP_MIN_WAVES 1
#endif
template <int MIXED, bool TIPZ, bool PREV_ROWS>
__global__ __launch_bounds__(kBlock, RSIK_SWEEP_MIN_WAVES) void solve_sweep_kernel(const SweepArgs K) {
    __shared__ SharedTables lds_tab;
    __shared__ double lds[kBlock / 64][64 * 10];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile0 = (int64_t)blockIdx.x * kBlock;
    const int64_t left = K.n - tile0;                                   // >= 1 (grid = ceil(n / kBlock))
    const unsigned rows = left < kBlock ? (unsigned)left : (unsigned)kBlock;
    const unsigned t = threadIdx.x & (kBlock - 1);
    const unsigned tt = (t < rows ? t : rows - 1) & (kBlock - 1);       // clamped pose index inside the tile
    const bool live = t < rows;

    double in[6];
#pragma unroll
    for (int k = 0; k < 6; k++) in[k] = ld_stream(K.in[k] + tile0 + tt);
    warm_and_stage_tables<MIXED>(K, lds_tab);
    const AccSweep<MIXED> A = kernarg_acc<AccSweep<MIXED>, SweepArgs>(lds_tab, (MIXED != 0 && K.arm[tile0 + tt] != 0) ? 1 : 0);
    double* lds_wave = lds[wave];

    const bool invalid = settle_pose(in);  // rsik.h "Rows that are not numbers"
    const V3 pos = {in[0], in[1], in[2]};
    const Goal G = goal_of_pose<TIPZ>(A, in[3], in[4], in[5]);
    Reach r = reach_g<false, false>(A, pos, G.woff);
    if (RSIK_RARE(invalid)) reach_invalid_input(r);
    store_reach(K, live, tile0, t, r);
    if (rows <= (unsigned)(wave * 64)) return;  // a wave past the end of the batch (wave-uniform; no barrier follows)

    const bool want_elbow = K.elbow != nullptr;
    const bool full = rows >= (unsigned)(wave * 64 + 64);  // the wave's 64 rows all exist (wave-uniform, scalar)
    const bool fraction = K.theta_policy != RSIK_THETA_EXPLICIT;
    const bool per_pose = K.theta_per_pose != 0;
    const int64_t wave_base = tile0 + wave * 64;
    double* jrow = lds_wave + lane * 7;
    double* erow = lds_wave + 64 * 7 + lane * 3;
    // the fraction arithmetic's two operands, as solve_kernel forms them per launch: theta = a + u * (b - a)
    const double fa = r.i0;
    double fb = r.i1;
    if (fa > fb) fb += kTwoPi;
    const double fspan = fb - fa;
    const V3 wrist = r.w;
    if (!r.ok) {  // rows of a pose that is not reachable: NaN in every sample — staged once, no sample of this lane rewrites them
        const double nan = opaque(__builtin_nan(""));
#pragma unroll
        for (int k = 0; k < 7; k++) jrow[k] = nan;
        erow[0] = nan; erow[1] = nan; erow[2] = nan;
        branch_stores_stay();
    }
    // the shared grid is read through the constant address space: one scalar load per sample and wave
    const __attribute__((address_space(4))) double* grid = (const __attribute__((address_space(4))) double*)K.theta_in;
    const double* th_col = K.theta_in + tile0 + tt;  // per-pose form: this pose's entry of sample 0
    double* jout = K.joints;
    double* eout = K.elbow;
    uint8_t* pout = K.projected ? K.projected + tile0 + t : nullptr;
    double* tout = K.theta ? K.theta + tile0 + t : nullptr;
#pragma clang loop unroll(disable)
    for (int k = 0; k < K.n_theta; k++) {
        const double th_in = per_pose ? *th_col : grid[k];
        double theta = th_in;
        if (fraction) theta = fa + th_in * fspan;
        bool projected = false;
        if (r.ok) {
            double ct, st;
            fast_sincos(near_angle(theta), &st, &ct);
            r.w = wrist;
            if constexpr (PREV_ROWS) {
                JointsOut o = joints_from_theta_g<true, TIPZ>(A, r, G, ct, st, (GConst)(K.prev_rows + (tile0 + tt) * 7));
#pragma unroll
                for (int q = 0; q < 7; q++) jrow[q] = o.j[q];
                if (want_elbow) { erow[0] = o.elbow.x; erow[1] = o.elbow.y; erow[2] = o.elbow.z; }
                projected = o.projected;
                branch_stores_stay();
            } else {
                JointsOut o = joints_from_theta_g<true, TIPZ>(A, r, G, ct, st, (const double*)K.prev);
#pragma unroll
                for (int q = 0; q < 7; q++) jrow[q] = o.j[q];
                if (want_elbow) { erow[0] = o.elbow.x; erow[1] = o.elbow.y; erow[2] = o.elbow.z; }
                projected = o.projected;
                branch_stores_stay();
            }
        } else {
            theta = __builtin_nan("");
        }
        if (full) {
            flush_rows_full<7>(jout, wave_base, lane, lds_wave);
            if (want_elbow) flush_rows_full<3>(eout, wave_base, lane, lds_wave + 64 * 7);
        } else {
            flush_rows<7>(jout, wave_base, K.n, lane, lds_wave);
            if (want_elbow) flush_rows<3>(eout, wave_base, K.n, lane, lds_wave + 64 * 7);
        }
        if (live) {
            if (pout) st_stream(pout, (uint8_t)(projected ? 1 : 0));
            if (tout) st_stream(tout, theta);
        }
        // next sample's slabs: n rows further on
        jout += K.n * 7;
        if (want_elbow) eout += K.n * 3;
        if (pout) pout += K.n;
        if (tout) tout += K.n;
        th_col += K.n;
    }
}

}  // namespace rsik
