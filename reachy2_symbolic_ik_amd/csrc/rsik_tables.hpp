// rsik_tables.hpp — what every kernel's start shares: the workgroup size, per-arm constant access (Acc, AccK), the workgroup's tables in
// LDS (SharedTables, stage_tables), the warm-up of the argument block (warm_kernarg, warm_and_stage_tables)
#pragma once

#include <stddef.h>

#include "rsik_device.hpp"

namespace rsik {

#ifndef RSIK_BLOCK
#define RSIK_BLOCK 256
#endif
constexpr int kBlock = RSIK_BLOCK;

// Per-arm constant access.  Uniform launches read the block from the kernarg segment (scalar loads).  Mixed r/l
// launches stage both blocks in LDS once per workgroup and every lane reads its own arm's value with one ds_read
// (selecting between two scalar values would cost two v_cndmask per use and spill the scalar file).
typedef const __attribute__((address_space(3))) double* LdsConst;
template <bool MIXED>
struct Acc {
    const ArmC* a;
    bool isl;
    LdsConst lds;  // MIXED only: this lane's arm block in LDS
    UnitAtanTab utab;  // LDS copy of the unit-vector atan2 table (rsik_math.hpp)
    __device__ __forceinline__ double operator()(int i) const {
        if constexpr (MIXED) return lds[i];
        else return a[0].v[i];
    }
};
// Same, with the uniform block addressed through an explicit kernarg-segment (constant address space) pointer.
typedef const __attribute__((address_space(4))) double* KConst;
// Entries of the constant block that can differ between a right and a left arm that are mirror images of each other
// (everything with a y component or a handedness: shoulder y, tip y, the shoulder frame, the elbow singularity y, the
// side sign, the projection plane).  In a mixed launch whose two blocks agree everywhere else (checked by the host:
// SolveArgs.mirror) only these come from the per-lane LDS copy; the rest are the same scalar loads as in a
// uniform launch (a mixed launch reads ~85 constants per wave, ~35 of them from this shared set).
__host__ __device__ constexpr bool arm_const_is_sided(int i) {
    return i == RSIK_C_SHOULDER + 1 || i == RSIK_C_TIPL + 1 || (i >= RSIK_C_MST && i < RSIK_C_TSH + 3) || i == RSIK_C_ES + 1 ||
           i == RSIK_C_SIDE || (i >= RSIK_C_PLANE_P && i < RSIK_C_PROJ_CENTER + 3);
}
// MIXED: 0 = one arm for the whole launch, 1 = per-lane arm, every constant from LDS, 2 = per-lane arm, mirrored blocks
template <int MIXED>
struct AccK {
    KConst k;
    LdsConst lds;
    UnitAtanTab utab;
    __device__ __forceinline__ double operator()(int i) const {
        if constexpr (MIXED == 1) return lds[i];
        else if constexpr (MIXED == 2) return arm_const_is_sided(i) ? lds[i] : k[i];
        else return k[i];
    }
};
// Workgroup-shared read-only data: the per-arm blocks (mixed launches) and the unit-vector atan2 table.
struct SharedTables {
    double arm[2][RSIK_ARM_CONSTS_COUNT];
    double utab[3][kUnitAtanRows];  // column-major, see unit_atan2_n
};
// The kernels read their ~1 KB argument block (pointers, launch constants, the arm constants) with scalar loads that the
// compiler places where the values are first needed — a dozen first touches of different 64-byte lines, spread over the
// whole kernel, and the scalar cache starts every launch cold: every wave of a launch's first round stalls on each of them
// (measured: RSIK_WARM_KERNARG 0 vs 1).  warm_kernarg<BYTES>() touches every line of the block once, after the wave
// has issued its input loads and ahead of the table-staging loads (warm_and_stage_tables): the misses overlap each other and
// the input loads' latency, later reads hit.
// (The values are discarded: all loads target one clobbered scalar register and are waited for inside the block.)
#ifndef RSIK_WARM_KERNARG
#define RSIK_WARM_KERNARG 1
#endif
template <int BYTES>
__device__ __forceinline__ void warm_kernarg() {
#if RSIK_WARM_KERNARG
    const unsigned long long ka = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
#define RSIK_TOUCH(off) if constexpr (BYTES > (off)) asm volatile("s_load_dword s90, %0, " #off ::"s"(ka) : "s90", "memory")
    RSIK_TOUCH(0x40); RSIK_TOUCH(0x80); RSIK_TOUCH(0xc0); RSIK_TOUCH(0x100); RSIK_TOUCH(0x140); RSIK_TOUCH(0x180);
    RSIK_TOUCH(0x1c0); RSIK_TOUCH(0x200); RSIK_TOUCH(0x240); RSIK_TOUCH(0x280); RSIK_TOUCH(0x2c0); RSIK_TOUCH(0x300);
    RSIK_TOUCH(0x340); RSIK_TOUCH(0x380); RSIK_TOUCH(0x3c0); RSIK_TOUCH(0x400); RSIK_TOUCH(0x440); RSIK_TOUCH(0x480);
    RSIK_TOUCH(0x4c0); RSIK_TOUCH(0x500); RSIK_TOUCH(0x540); RSIK_TOUCH(0x580); RSIK_TOUCH(0x5c0); RSIK_TOUCH(0x600);
#undef RSIK_TOUCH
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "s90", "memory");
#endif
}

// All global reads of the staging are issued first and the LDS writes follow, so a workgroup pays ONE memory round trip
// before its barrier (a copy loop per table serialises one round trip per table: +0.6 us on every wave's start-up).
// It does not warm the argument block: a kernel that calls it directly (every kernel but the five of warm_and_stage_tables) runs
// with no warm-up at all.
// WARM: NOT USED, and never was.  Commit 83758e1 added it as "bytes of the argument block to warm while the staging loads fly" and
// took the warm_kernarg call out of its ten callers; the call that was to use it here was never committed.  It stays, with the
// arguments those callers pass, only because it decides which callers share an instantiation, and the order in which the compiler
// emits those changes how two kernels compile: without it stage_kernel comes out 6 instructions longer and
// theta_from_joints_state_kernel<true> 40 shorter (one generic-to-LDS null test folded or not, the arithmetic the same), and the
// kernels are to stay what they were (the rule above warm_and_stage_tables; docs/experiments.md part H).  A new caller leaves it out.
// NB: threads of the workgroup (a power of two)
template <bool MIXED, int WARM = 0, int NB = kBlock>
__device__ __forceinline__ void stage_tables(SharedTables& S, const ArmC* arms) {
    constexpr int NA = kUnitAtanRows * 3, NS = kSinCosRows * 2, NC = 2 * RSIK_ARM_CONSTS_COUNT;
    constexpr int RA = (NA + NB - 1) / NB, RS = (NS + NB - 1) / NB, RC = (NC + NB - 1) / NB;
    const unsigned t = threadIdx.x & (NB - 1);  // the launch uses NB threads: tells the compiler t < NB
    const double* ga = &c_unit_atan_tab[0][0];
    const double* gs = &c_sincos_tab[0][0];
    double va[RA], vs[RS], vc[RC];
    // chunk r of a table covers elements [r NB, (r+1) NB): only a table's last chunk can be partial
#pragma unroll
    for (int r = 0; r < RA; r++) va[r] = ((r + 1) * NB <= NA || t + r * NB < NA) ? ga[t + r * NB] : 0.0;
#pragma unroll
    for (int r = 0; r < RS; r++) vs[r] = ((r + 1) * NB <= NS || t + r * NB < NS) ? gs[t + r * NB] : 0.0;
    if constexpr (MIXED) {
#pragma unroll
        for (int r = 0; r < RC; r++) {
            const unsigned k = t + r * NB;
            vc[r] = ((r + 1) * NB <= NC || k < NC) ? arms[k / RSIK_ARM_CONSTS_COUNT].v[k % RSIK_ARM_CONSTS_COUNT] : 0.0;
        }
    }
    double* la = &S.utab[0][0];
    double* ls = &g_sincos_tab[0][0];
#pragma unroll
    for (int r = 0; r < RA; r++)
        if ((r + 1) * NB <= NA || t + r * NB < NA) la[t + r * NB] = va[r];
#pragma unroll
    for (int r = 0; r < RS; r++)
        if ((r + 1) * NB <= NS || t + r * NB < NS) ls[t + r * NB] = vs[r];
    if constexpr (MIXED) {
        double* lc = &S.arm[0][0];
#pragma unroll
        for (int r = 0; r < RC; r++)
            if ((r + 1) * NB <= NC || t + r * NB < NC) lc[t + r * NB] = vc[r];
    }
    __syncthreads();
}
template <bool MIXED>
__device__ __forceinline__ Acc<MIXED> make_acc(const ArmC* arms, bool isl, SharedTables& S) {
    Acc<MIXED> A{arms, isl, (LdsConst)S.arm[isl ? 1 : 0], (UnitAtanTab)&S.utab[0][0]};
    return A;
}

// ---- what solve_kernel and solve_sweep_kernel (rsik_kernel_sweep.hpp) share — here and in rsik_goal.hpp — templated on the argument
// block and the accessor type: each keeps instantiations of its own (see AccSweep).  Not the tile indices and the six pose loads: in a
// function both kernels compile differently.
// Nor, for the sweep and nearest kernels, the body of their sample loop: one "joints at this sample" function in place of the
// `if constexpr (PREV_ROWS)` pair, with one "stage the row / stage a NaN row" function, compiled 48 instantiations differently (every
// sweep and every nearest kernel: sweep PREV_ROWS 10 instructions shorter, nearest 1 to 14 longer).  What is shared is what
// scripts/compare_kernel_asm.py showed to leave every instantiation instruction for instruction as it was; a further helper goes
// through the same comparison, one at a time.
// The kernarg warm-up and the table staging of the solve, sweep, nearest, path and reach_map kernels.  (MIXED == 1 takes every constant
// from LDS: nothing to warm.)  The warm-up goes BEFORE the staging loads are issued.  The other kernels call stage_tables alone and
// warm nothing.  The two forms were measured against each other per kernel (commit 83758e1, which recorded the second as "between
// their issue and their use"; as committed it is no warm-up at all): config 2 (the solve kernel) 31.1 us warmed before the staging
// loads against 31.9 us, config 3 (the discrete kernel) 15.9 us against 15.7 us.  A warm-up between the issue and the use of the
// staging loads has not been run in any kernel (docs/experiments.md part H).
template <int MIXED, class ARGS>
__device__ __forceinline__ void warm_and_stage_tables(const ARGS& K, SharedTables& S) {
    warm_kernarg<(MIXED == 1 ? 0 : (int)offsetof(ARGS, arms) + (int)sizeof(ArmC))>();
    stage_tables<(MIXED != 0)>(S, K.arms);
}
// An AccK (or a type derived from it) over the arms of the kernel's own argument block ARGS, read through the kernarg segment
template <class ACC, class ARGS>
__device__ __forceinline__ ACC kernarg_acc(SharedTables& S, int slot) {
    ACC A;
    A.k = (KConst)&((const __attribute__((address_space(4))) ARGS*)__builtin_amdgcn_kernarg_segment_ptr())->arms[0].v[0];
    A.lds = (LdsConst)S.arm[slot]; A.utab = (UnitAtanTab)&S.utab[0][0];
    return A;
}

}  // namespace rsik
