// rsik_rows.hpp — streaming global accesses and row-major rows through a wave's LDS slab: the wave-level LDS fences, st_stream / ld_stream,
// store_rows / flush_rows* (rows out), stage_rows / staged_row (rows in), branch_stores_stay
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rsik {

// What stands between a wave's LDS writes and its lanes' reads of each other's values.  The s_waitcnt operand is gfx9's encoding of
// lgkmcnt(0) alone: bits 11:8 (lgkmcnt) zero, vmcnt (bits 15:14 and 3:0) and expcnt (bits 6:4) at their maxima, so the wave waits for
// its LDS operations and for no global load or store.  A wave-level barrier is enough because only this wave's lanes touch the slab and
// the wave executes in lock-step: wave_barrier is no instruction, it keeps the compiler from moving LDS accesses across this point.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
}
// The same between release / acquire fences of wavefront scope.  wave_lds_fence serves where all the writes stand before and all the
// reads after one point of straight-line code (every helper below); this one is for an exchange in both directions around a loop
// whose trips depend on data (the discrete kernel's cooperative sweep, where a group's leader writes over a row the others have read).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    wave_lds_fence();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Batch inputs are read once and outputs written once: streaming (non-temporal) accesses keep them from displacing
// each other in L2 and leave fewer dirty lines for the end-of-kernel write-back.
#ifndef RSIK_NT_STORE
#define RSIK_NT_STORE 1  // config 2: 45.2 -> 44.7 us per 1 M poses; non-temporal LOADS cost 0.5 us (inputs of back-to-back launches sit in the 256 MB Infinity Cache)
#endif
#ifndef RSIK_NT_LOAD
#define RSIK_NT_LOAD 0
#endif
typedef double f64x2 __attribute__((ext_vector_type(2)));
// kStoreStream: non-temporal.  kStoreThrough: written through to system scope (sc0 sc1) — nothing of the kernel's output is left dirty in
// the eight L2s for the write-back at its end, which the next launch of a stream (and every launch that waits for this one) sits behind.
// Round 6, same box, interleaved: the discrete kernel 15.0 -> 14.6 us per 262 144 matrices, the trajectory pipeline -1.3 ... -1.5 % per pass
// in every launch form (its kernels' ends are what its hand-overs wait for); the solve kernel, four rounds of waves long, 31.3 -> 31.7 us
// with it: that one keeps the non-temporal form (docs/experiments.md R6.8).
constexpr int kStoreStream = 1, kStoreThrough = 2;
template <int POLICY = kStoreStream, class T>
__device__ __forceinline__ void st_stream(T* p, T v) {
#if RSIK_NT_STORE
    if constexpr (POLICY == kStoreThrough && sizeof(T) <= 8) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}
template <class T>
__device__ __forceinline__ T ld_stream(const T* p) {
#if RSIK_NT_LOAD
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

// Writes ROWxW doubles per lane as a contiguous [64*W] slab per wave (row-major [n,W] output).
template <int W, int POLICY = kStoreStream>
__device__ __forceinline__ void store_rows(double* __restrict__ out, int64_t wave_base, int64_t n, int lane,
                                           double* __restrict__ lds_wave, const double (&vals)[W]) {
#pragma unroll
    for (int k = 0; k < W; k++) lds_wave[lane * W + k] = vals[k];
    wave_lds_fence();
    int64_t rows = n - wave_base;
    if (rows > 64) rows = 64;
    double* dst = out + wave_base * W;
    if (__builtin_amdgcn_readfirstlane((int)rows) == 64) {  // every wave but the last: no per-row bounds test
        double v[W];
#pragma unroll
        for (int k = 0; k < W; k++) v[k] = lds_wave[k * 64 + lane];
#pragma unroll
        for (int k = 0; k < W; k++) st_stream<POLICY>(dst + k * 64 + lane, v[k]);
    } else {
        const int64_t total = rows * W;
#pragma unroll
        for (int k = 0; k < W; k++) {
            int idx = k * 64 + lane;
            if (idx < total) st_stream<POLICY>(dst + idx, lds_wave[idx]);
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// flush_rows for a wave whose 64 rows all exist (every wave but the last of a launch): the W row reads are issued
// together and the W stores share one base address, no per-row bounds test.
template <int W>
__device__ __forceinline__ void flush_rows_full(double* __restrict__ out, int64_t wave_base, int lane,
                                                const double* __restrict__ lds_rows) {
    wave_lds_fence();
    double v[W];
#pragma unroll
    for (int k = 0; k < W; k++) v[k] = lds_rows[k * 64 + lane];
    double* dst = out + wave_base * W + lane;
#pragma unroll
    for (int k = 0; k < W; k++) st_stream(dst + k * 64, v[k]);
    __builtin_amdgcn_wave_barrier();
}

// Second half of store_rows for values the lanes have already put in LDS.
template <int W>
__device__ __forceinline__ void flush_rows(double* __restrict__ out, int64_t wave_base, int64_t n, int lane,
                                           const double* __restrict__ lds_rows) {
    wave_lds_fence();
    int64_t rows = n - wave_base;
    if (rows > 64) rows = 64;
    const int64_t total = rows * W;
    double* dst = out + wave_base * W;
#pragma unroll
    for (int k = 0; k < W; k++) {
        int idx = k * 64 + lane;
        if (idx < total) st_stream(dst + idx, lds_rows[idx]);
    }
    __builtin_amdgcn_wave_barrier();
}

// The first `nrows` rows of W doubles a wave has staged in LDS, written as one contiguous run (flush_rows for a wave that holds
// PW <= 64 poses: nrows <= PW).  (Not folded into flush_rows: solve_nearest_kernel is to compile as it did.)
template <int W, int PW>
__device__ __forceinline__ void flush_pose_rows(double* __restrict__ out, int64_t wave_base, int nrows, int lane,
                                                const double* __restrict__ lds_rows) {
    wave_lds_fence();
    const int total = nrows * W;
    double* dst = out + wave_base * W;
#pragma unroll
    for (int k = 0; k < W; k++) {
        if (k * 64 < PW * W) {
            const int idx = k * 64 + lane;
            if (idx < total) st_stream(dst + idx, lds_rows[idx]);
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// The counterpart of store_rows' second half, for inputs: a wave's rows of a row-major [n, W] array, one contiguous [64 * W] slab, go to
// LDS with W coalesced loads per wave and stay there; staged_row is the lane's row of that slab (a lane past the end: the last row).
// Between the two stands rows_staged: the LDS counter drained, the wave in lock-step.
template <int W>
__device__ __forceinline__ void stage_rows(const double* __restrict__ in, int64_t wave_base, int64_t n, int lane,
                                           double* __restrict__ lds_slab) {
    int64_t rows = n - wave_base;
    if (rows > 64) rows = 64;
    const int total = (int)rows * W;
    const double* src = in + wave_base * W;
#pragma unroll
    for (int k = 0; k < W; k++) {
        const int idx = k * 64 + lane;
        if (idx < total) lds_slab[idx] = ld_stream(src + idx);
    }
}
__device__ __forceinline__ void rows_staged() { wave_lds_fence(); }
template <int W>
__device__ __forceinline__ void staged_row(const double* lds_slab, int64_t wave_base, int64_t n, int lane, double (&vals)[W]) {
    int64_t rows = n - wave_base;
    if (rows > 64) rows = 64;
    const int mine = (lane < (int)rows ? lane : (int)rows - 1) * W;
#pragma unroll
    for (int k = 0; k < W; k++) vals[k] = lds_slab[mine + k];
}

// A compiler-only memory fence at the end of a branch that stages a lane's outputs in LDS.  Without it the compiler sinks the
// stores of the reachable and the unreachable branch into one sequence after the join and feeds it through ten register
// pairs that it first fills with the other branch's value: nine v_mov_b64 executed by every wave, reachable or not.
__device__ __forceinline__ void branch_stores_stay() { asm volatile("" ::: "memory"); }

}  // namespace rsik
