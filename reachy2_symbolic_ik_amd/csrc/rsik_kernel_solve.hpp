// rsik_kernel_solve.hpp — rsik_solve: its argument block and solve_kernel; rsik_matrix_to_pose: matrix_to_pose_kernel
#pragma once

#include "rsik_goal.hpp"
#include "rsik_tables.hpp"

namespace rsik {

struct SolveArgs {
    int64_t n;
    const double* in[6];
    const uint8_t* arm;
    int theta_policy;
    const double* theta_in;
    union {
        double prev[7];         // rsik_solve: get_joints' previous_joints, the same for every pose
        const double* prev_rows;  // rsik_solve_rows (PREV_ROWS kernels): [n,7] device, one row per pose
    };
    double* joints;
    double* interval;
    double* elbow;
    uint8_t* reachable;
    uint8_t* state;
    ArmC arms[2];  // uniform launch: arms[0] is the arm; mixed launch: arms[0] = r, arms[1] = l
};

#ifndef RSIK_SOLVE_MIN_WAVES
#define RSIK_SOLVE_MIN_WAVES 1
#endif

// One workgroup = one tile of kBlock consecutive poses, one pose per lane.  Every global address is a scalar base
// (column pointer + tile offset, computed on the SALU) plus a small per-lane offset, so the six loads and all the
// stores share one or two address registers.  Lanes past the end of the batch recompute the last pose; their stores
// are masked.  (A persistent variant that walks several tiles per workgroup with the next tile prefetched was
// measured slower at every depth: 46.0 / 47.7 / 52.5 us for 2 / 4 / 8 tiles against 45.5 us, see
// profiles/r01/timeline/: under the power-managed clock it is the executed instruction count that sets the time, not
// how well the waves overlap.)
// TIPZ: every arm of the launch has tip_x = tip_y = 0 (goal_from_euler_tipz: -24 fp64 operations per pose).
// PREV_ROWS: previous_joints is the pose's own row of K.prev_rows (rsik_solve_rows), not the launch constant K.prev.
// joints_from_theta_g reads it only on an exact singularity, so a pose that is not singular loads none of it.
template <int MIXED, bool TIPZ, bool PREV_ROWS = false>
__global__ __launch_bounds__(kBlock, RSIK_SOLVE_MIN_WAVES) void solve_kernel(const SolveArgs K) {
    __shared__ SharedTables lds_tab;
    __shared__ double lds[kBlock / 64][64 * 10];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // scalar: wave-level tests stay on the SALU
    const int64_t tile0 = (int64_t)blockIdx.x * kBlock;
    const int64_t left = K.n - tile0;                                   // >= 1 (grid = ceil(n / kBlock))
    const unsigned rows = left < kBlock ? (unsigned)left : (unsigned)kBlock;
    const unsigned t = threadIdx.x & (kBlock - 1);                      // (tells the compiler t < kBlock)
    const unsigned tt = (t < rows ? t : rows - 1) & (kBlock - 1);       // clamped pose index inside the tile
    const bool live = t < rows;

#ifdef RSIK_CLOCK_PROBE
    const uint64_t probe_c0 = __builtin_readcyclecounter(), probe_r0 = __builtin_amdgcn_s_memrealtime();
#endif
#ifdef RSIK_TIMELINE_PROBE
    const uint64_t probe_t0 = __builtin_amdgcn_s_memrealtime();
#endif
    // the six pose loads are issued before the table staging so that their latency overlaps it
    double in[6];
#pragma unroll
    for (int k = 0; k < 6; k++) in[k] = ld_stream(K.in[k] + tile0 + tt);
    warm_and_stage_tables<MIXED>(K, lds_tab);
#ifdef RSIK_TIMELINE_PROBE
    const uint64_t probe_t1 = __builtin_amdgcn_s_memrealtime();
    uint64_t probe_mid = 0, probe_goal = 0, probe_reach = 0;
#define RSIK_SOLVE_PROBE(v) do { __builtin_amdgcn_sched_barrier(0); v = __builtin_amdgcn_s_memrealtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define RSIK_SOLVE_PROBE(v) do { } while (0)
#endif
    const AccK<MIXED> A = kernarg_acc<AccK<MIXED>, SolveArgs>(lds_tab, (MIXED != 0 && K.arm[tile0 + tt] != 0) ? 1 : 0);
    double* lds_wave = lds[wave];

    // rsik.h "Rows that are not numbers": judged here, while the six values are at hand (further down it would keep them all alive)
    const bool invalid = settle_pose(in);
    const V3 pos = {in[0], in[1], in[2]};
    Goal G;
    if constexpr (TIPZ) {
        G = goal_from_euler_tipz(A, in[3], in[4], in[5]);
    } else {
        RSIK_MARK("euler");
        const Rot Rg = rot_from_euler(in[3], in[4], in[5]);
        RSIK_MARK("goal");
        G = make_goal(A, Rg);
    }
    RSIK_MARK("reach_start");
    RSIK_SOLVE_PROBE(probe_goal);
    Reach r = reach_g<false, false>(A, pos, G.woff);
    RSIK_SOLVE_PROBE(probe_reach);
    if (RSIK_RARE(invalid)) reach_invalid_input(r);
    RSIK_MARK("after_reach");

    // joints [64,7] and elbow [64,3] of the wave are staged in LDS (row-major, as they go to HBM) by whichever branch
    // the lane takes, then written out with coalesced rows: failed poses only cost their NaN fill when one exists
    // (the elbow rows only when the caller asked for them: a launch constant, every test of it a scalar branch)
    const bool want_elbow = K.elbow != nullptr;
    if (K.theta_policy != RSIK_THETA_NONE) {
        double* jrow = lds_wave + lane * 7;
        double* erow = lds_wave + 64 * 7 + lane * 3;
        if (r.ok) {
            double ct = r.ct0, st = r.st0;  // theta = interval[0]: cos/sin come straight from the intersection point
            if (K.theta_policy != RSIK_THETA_INTERVAL0) {
                const double th_in = K.theta_in[tile0 + tt];
                double theta = th_in;
                if (K.theta_policy != RSIK_THETA_EXPLICIT) {
                    double a = r.i0, b = r.i1;
                    if (a > b) b += kTwoPi;
                    theta = a + th_in * (b - a);
                }
                fast_sincos(near_angle(theta), &st, &ct);
            }
            // Two statements chosen at compile time: a pointer that could be either the kernarg array or a global row would
            // turn the uniform kernels' loads into flat loads, and any shared local changes how the uniform kernels are
            // scheduled.  tt is clamped, so dead lanes read a row in bounds.
            if constexpr (PREV_ROWS) {
                JointsOut o = joints_from_theta_g<true, TIPZ>(A, r, G, ct, st, (GConst)(K.prev_rows + (tile0 + tt) * 7));
                RSIK_MARK("stores");
#pragma unroll
                for (int k = 0; k < 7; k++) jrow[k] = o.j[k];
                if (want_elbow) { erow[0] = o.elbow.x; erow[1] = o.elbow.y; erow[2] = o.elbow.z; }
                branch_stores_stay();
            } else {
                JointsOut o = joints_from_theta_g<true, TIPZ>(A, r, G, ct, st, (const double*)K.prev);
                RSIK_MARK("stores");
#pragma unroll
                for (int k = 0; k < 7; k++) jrow[k] = o.j[k];
                if (want_elbow) { erow[0] = o.elbow.x; erow[1] = o.elbow.y; erow[2] = o.elbow.z; }
                branch_stores_stay();
            }
        } else {
            // (`opaque`: the value is made inside this branch — otherwise the compiler merges the two branches' LDS writes and
            // every wave, reachable or not, first fills ten registers pairs with NaN: 20 v_mov in the all-reachable config 2)
            const double nan = opaque(__builtin_nan(""));
#pragma unroll
            for (int k = 0; k < 7; k++) jrow[k] = nan;
            if (want_elbow) { erow[0] = nan; erow[1] = nan; erow[2] = nan; }
            branch_stores_stay();
        }
#ifdef RSIK_TIMELINE_PROBE
        probe_mid = __builtin_amdgcn_s_memrealtime();  // all arithmetic done, outputs staged in LDS
#endif
        const int64_t wave_base = tile0 + wave * 64;
        if (rows >= (unsigned)(wave * 64 + 64)) {  // the wave's 64 rows all exist (wave-uniform, scalar)
            if (K.joints) flush_rows_full<7>(K.joints, wave_base, lane, lds_wave);
            if (want_elbow) flush_rows_full<3>(K.elbow, wave_base, lane, lds_wave + 64 * 7);
        } else if (rows > (unsigned)(wave * 64)) {
            if (K.joints) flush_rows<7>(K.joints, wave_base, K.n, lane, lds_wave);
            if (want_elbow) flush_rows<3>(K.elbow, wave_base, K.n, lane, lds_wave + 64 * 7);
        }
    }
    store_reach(K, live, tile0, t, r);
#ifdef RSIK_TIMELINE_PROBE
    // diagnostic build only (scripts/timeline_probe.py): lanes 0-2 of every wave overwrite their interval rows with
    // (start, tables staged), (outputs staged, stores issued), (HW_ID, XCC_ID)
    if (lane < 4 && K.interval && live) {
        __builtin_amdgcn_s_waitcnt(0);
        const uint64_t t3 = __builtin_amdgcn_s_memrealtime();
        const uint32_t hw = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));   // HW_REG_HW_ID
        const uint32_t xcc = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)); // HW_REG_XCC_ID
        double2 iv;
        if (lane == 0) iv = {(double)probe_t0, (double)probe_t1};
        else if (lane == 1) iv = {(double)probe_mid, (double)t3};
        else if (lane == 2) iv = {(double)hw, (double)xcc};
        else iv = {(double)probe_goal, (double)probe_reach};  // (the stage timers' extra stamps: goal vectors done, is_reachable done)
        reinterpret_cast<double2*>(K.interval)[tile0 + t] = iv;
    }
#endif
#ifdef RSIK_CLOCK_PROBE
    // diagnostic build only (scripts/clock_probe.py): lane 0 of every wave overwrites its interval row with the wave's
    // lifetime in core-clock ticks (s_memtime) and in 100 MHz ticks (s_memrealtime)
    if (lane == 0 && K.interval && live) {
        const uint64_t c1 = __builtin_readcyclecounter(), r1 = __builtin_amdgcn_s_memrealtime();
        double2 iv = {(double)(c1 - probe_c0), (double)(r1 - probe_r0)};
        reinterpret_cast<double2*>(K.interval)[tile0 + t] = iv;
    }
#endif
}

// utils.get_euler_from_homogeneous_matrix for a batch (U:84-90), optionally with ControlIK's identity shortcut
// (C:212-214): m12 SoA -> pose SoA (px, py, pz, roll, pitch, yaw), the input layout of rsik_solve.
struct MatrixToPoseArgs {
    int64_t n;
    const double* in[12];
    double* out[6];
    int identity_shortcut;
};
__global__ __launch_bounds__(kBlock) void matrix_to_pose_kernel(const MatrixToPoseArgs K) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= K.n) return;
    double m[9], eul[3];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = K.in[k][i];
    bool eye = K.identity_shortcut != 0;
#pragma unroll
    for (int k = 0; k < 9; k++) eye = eye && np_isclose(m[k], (k % 4 == 0) ? 1.0 : 0.0);
    if (eye) { eul[0] = 0.0; eul[1] = 0.0; eul[2] = 0.0; }
    else euler_xyz_from_matrix(m, eul);
#pragma unroll
    for (int k = 0; k < 3; k++) { K.out[k][i] = K.in[9 + k][i]; K.out[3 + k][i] = eul[k]; }
}

}  // namespace rsik
