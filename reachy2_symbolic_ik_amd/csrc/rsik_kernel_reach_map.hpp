// rsik_kernel_reach_map.hpp — rsik_reach_map: is_reachable of n_pos positions x n_rot orientations, reduced per position on the device (reach_map_kernel)
#pragma once

#include "rsik_goal.hpp"
#include "rsik_tables.hpp"

namespace rsik {

constexpr int kReachMapTile = 1024;        // orientations whose wrist offsets a workgroup holds in LDS at a time (a multiple of 64)
constexpr int kReachMapMaxPosPerWave = 16;  // positions a wave owns, at the most (the host picks 1, 2, 4, 8 or 16: reach_map_pos_per_wave)
constexpr int kReachMapWaves = kBlock / 64;

struct ReachMapArgs {
    int64_t n_pos;
    const double* pos[3];
    const uint8_t* arm;   // [n_pos] or NULL
    int n_rot;            // 1 ... 4096
    int tile;             // min(n_rot rounded up to 64, kReachMapTile): the stride of the wrist-offset columns in LDS
    int pos_per_wave;     // 1 ... kReachMapMaxPosPerWave
    const double* eul[3];
    uint32_t* count;         // [n_pos] or NULL
    uint32_t* state_count;   // [n_pos][RSIK_REACH_MAP_STATES] or NULL
    double* theta_measure;   // [n_pos] or NULL
    uint64_t* mask;          // [n_pos][ceil(n_rot / 64)] or NULL
    ArmC arms[2];            // as SolveArgs.arms
};
// dynamic LDS of a launch: the wrist offsets of one tile, three columns per arm slot, and one "not numbers" byte per orientation
__host__ __device__ constexpr size_t reach_map_lds_bytes(int slots, int tile) { return (size_t)slots * 3 * tile * sizeof(double) + (size_t)tile; }

// The map's own constant accessor (see AccSweep): reach_g and the goal stage get instantiations of their own here.
template <int MIXED>
struct AccReachMap : AccK<MIXED> {};

// The sum of a double over the 64 lanes in a fixed order, with DPP moves instead of six dependent trips through the LDS crossbar
// (__shfl_xor): shifts by 1, 2, 4 and 8 inside each row of 16 lanes leave the row's sum in its last lane, row_bcast:15 adds it to the
// next row (rows 1 and 3), row_bcast:31 adds lane 31 to rows 2 and 3; lane 63 then holds the wave's sum, which comes back as a scalar.
// A lane without a source, or in a row the mask leaves out, adds 0.0.  Needs all 64 lanes active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_or_zero_f64(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, ROW_MASK, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, ROW_MASK, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum_f64(double x) {
    x += dpp_or_zero_f64<0x111, 0xF>(x);  // row_shr:1
    x += dpp_or_zero_f64<0x112, 0xF>(x);  // row_shr:2
    x += dpp_or_zero_f64<0x114, 0xF>(x);  // row_shr:4
    x += dpp_or_zero_f64<0x118, 0xF>(x);  // row_shr:8
    x += dpp_or_zero_f64<0x142, 0xA>(x);  // row_bcast:15 into rows 1 and 3
    x += dpp_or_zero_f64<0x143, 0xC>(x);  // row_bcast:31 into rows 2 and 3
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), 63), __builtin_amdgcn_readlane(__double2loint(x), 63));
}

// Pose (i, j) = position i with orientation j.  Lanes are orientations, a position is wave-uniform.
//
// A workgroup owns kReachMapWaves * pos_per_wave consecutive positions, pos_per_wave of them per wave.  It walks the orientations in
// tiles of at most kReachMapTile:
//   stage    every thread takes orientations t, t + kBlock, ... of the tile: settle_pose on (0, 0, 0, roll, pitch, yaw) — far angles
//            reduced, "not numbers" judged — and goal_of_pose<TIPZ> per arm slot; the wrist offset goes to LDS (column-wise, 24 B per
//            orientation and slot), the verdict to a byte.  The three sincos and the rotation are paid once per orientation and
//            workgroup, not once per pose.
//   reach    each wave, for each of its positions: the position comes through scalar loads (constant address space) and is settled
//            with (x, y, z, 0, 0, 0), so "Pose out of reach" and "Backward pose" are scalar branches inside reach_g; then one
//            reach_g<false, false> per 64-orientation chunk on (position, wrist offset from LDS), reach_invalid_input where either
//            half is not numbers.  These are solve_kernel's functions on solve_kernel's operands (settle_pose judges and reduces the
//            two halves of a row independently; the library is compiled without contraction): reachable, state and interval of
//            pose (i, j) are rsik_solve's under RSIK_THETA_NONE bit for bit, whatever pos_per_wave and the tile are.
//   reduce   the chunk's mask word is __ballot(reachable), the counts are popcounts of ballots per state code (scalar adds), the
//            width goes into a per-lane sum (lane l adds chunks in rising order); at the end of the tile wave_sum_f64 gives
//            the wave's sum, in a fixed order, as a scalar.
// The per-position totals live in LDS between tiles (each lane reads and writes only its own word: no barrier); the tile sums are
// added in rising tile order.  Nothing crosses a wave and nothing is an atomic: the measure is the same bits on every launch.
// After the last tile lanes 0 ... 11 write the position's row with ordinary vector stores; the mask words of a tile are stored
// by the lanes that hold them, 8 B each, side by side.
// Every wave reaches every barrier: a wave without positions (the last workgroup) stages and waits like the others.
template <int MIXED, bool TIPZ>
__global__ __launch_bounds__(kBlock) void reach_map_kernel(const ReachMapArgs K) {
    constexpr int SLOTS = MIXED != 0 ? 2 : 1;
    __shared__ SharedTables lds_tab;
    __shared__ uint32_t acc_n[kReachMapWaves][kReachMapMaxPosPerWave][12];  // [..][s < 11]: poses in state s; [..][11]: reachable poses
    __shared__ double acc_w[kReachMapWaves][kReachMapMaxPosPerWave];
    extern __shared__ double woff_lds[];  // [SLOTS][3][tile] doubles, then [tile] bytes
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & (kReachMapWaves - 1);
    const int n_rot = K.n_rot, tile = K.tile;
    uint8_t* bad_lds = reinterpret_cast<uint8_t*>(woff_lds + SLOTS * 3 * tile);
    const int ppw = K.pos_per_wave < kReachMapMaxPosPerWave ? K.pos_per_wave : kReachMapMaxPosPerWave;
    const int64_t p0 = ((int64_t)blockIdx.x * kReachMapWaves + wave) * ppw;
    const int64_t p_left = K.n_pos - p0;
    const int np = p_left <= 0 ? 0 : (p_left < ppw ? (int)p_left : ppw);  // this wave's positions (wave-uniform)
    const int64_t words = ((int64_t)n_rot + 63) >> 6;                      // mask words per position

    warm_and_stage_tables<MIXED>(K, lds_tab);  // (ends in a barrier)
    if (lane < 12) {
#pragma unroll
        for (int k = 0; k < kReachMapMaxPosPerWave; k++) acc_n[wave][k][lane] = 0;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kReachMapMaxPosPerWave; k++) acc_w[wave][k] = 0.0;
    }
    typedef const __attribute__((address_space(4))) double* ScalarCol;
    const ScalarCol px = (ScalarCol)K.pos[0], py = (ScalarCol)K.pos[1], pz = (ScalarCol)K.pos[2];

#pragma clang loop unroll(disable)
    for (int r0 = 0; r0 < n_rot; r0 += tile) {
        const int nr = n_rot - r0 < tile ? n_rot - r0 : tile;  // orientations of this tile, >= 1
        const bool last_tile = r0 + tile >= n_rot;
        if (r0 != 0) __syncthreads();                         // every wave has read the tile before
        // ---- stage: orientation -> wrist offset per arm slot
#pragma clang loop unroll(disable)
        for (int j = threadIdx.x; j < nr; j += kBlock) {
            double in[6] = {0.0, 0.0, 0.0, K.eul[0][r0 + j], K.eul[1][r0 + j], K.eul[2][r0 + j]};
            const bool bad = settle_pose(in);  // rsik.h "Rows that are not numbers", the orientation's half
#pragma unroll
            for (int s = 0; s < SLOTS; s++) {
                const AccReachMap<MIXED> As = kernarg_acc<AccReachMap<MIXED>, ReachMapArgs>(lds_tab, s);
                const Goal G = goal_of_pose<TIPZ>(As, in[3], in[4], in[5]);
                double* col = woff_lds + s * 3 * tile + j;
                col[0] = G.woff.x; col[tile] = G.woff.y; col[2 * tile] = G.woff.z;
            }
            bad_lds[j] = bad ? 1 : 0;
        }
        __syncthreads();
        // ---- reach and reduce: this wave's positions over the tile's chunks
        const int chunks = (nr + 63) >> 6;  // <= kReachMapTile / 64 = 16 <= 64 lanes
#pragma clang loop unroll(disable)
        for (int k = 0; k < np; k++) {
            const int64_t p = p0 + k;
            double pin[6] = {px[p], py[p], pz[p], 0.0, 0.0, 0.0};
            const bool pos_bad = settle_pose(pin);  // the position's half
            const V3 pos = {pin[0], pin[1], pin[2]};
            int slot = 0;
            if constexpr (MIXED != 0) slot = __builtin_amdgcn_readfirstlane(K.arm[p] != 0 ? 1 : 0);
            const AccReachMap<MIXED> A = kernarg_acc<AccReachMap<MIXED>, ReachMapArgs>(lds_tab, slot);
            const double* wcol = woff_lds + slot * 3 * tile;
            uint32_t n_ok = 0, n_st[RSIK_REACH_MAP_STATES];
#pragma unroll
            for (int s = 0; s < RSIK_REACH_MAP_STATES; s++) n_st[s] = 0;
            double wsum = 0.0;
            uint64_t my_word = 0;
#pragma clang loop unroll(disable)
            for (int c = 0; c < chunks; c++) {
                const int j = c * 64 + lane;
                const bool live = j < nr;
                const int jj = live ? j : nr - 1;  // lanes past the ragged end recompute the last orientation; their votes are masked
                const V3 woff = {wcol[jj], wcol[tile + jj], wcol[2 * tile + jj]};
                Reach r = reach_g<false, false>(A, pos, woff);
                if (RSIK_RARE(pos_bad || bad_lds[jj] != 0)) reach_invalid_input(r);
                const uint64_t okb = __ballot(live && r.ok);
                n_ok += (uint32_t)__builtin_popcountll(okb);
#pragma unroll
                for (int s = 0; s < RSIK_REACH_MAP_STATES; s++) n_st[s] += (uint32_t)__builtin_popcountll(__ballot(live && r.state == s));
                double w = r.i1 - r.i0;
                if (r.i0 > r.i1) w += kTwoPi;
                wsum += (live && r.ok) ? w : 0.0;
                if (lane == c) my_word = okb;
            }
            wsum = wave_sum_f64(wsum);
            uint32_t mine = n_ok;  // lane 11
#pragma unroll
            for (int s = 0; s < RSIK_REACH_MAP_STATES; s++)
                if (lane == s) mine = n_st[s];
            if (K.mask && lane < chunks) K.mask[p * words + (r0 >> 6) + lane] = my_word;
            if (lane < 12) {
                const uint32_t tot = acc_n[wave][k][lane] + mine;
                acc_n[wave][k][lane] = tot;
                if (last_tile) {
                    if (lane < RSIK_REACH_MAP_STATES) {
                        if (K.state_count) K.state_count[p * RSIK_REACH_MAP_STATES + lane] = tot;
                    } else if (K.count) {
                        K.count[p] = tot;
                    }
                }
            }
            if (lane == 0) {
                const double tot = acc_w[wave][k] + wsum;
                acc_w[wave][k] = tot;
                if (last_tile && K.theta_measure) K.theta_measure[p] = tot;
            }
        }
    }
}

}  // namespace rsik
