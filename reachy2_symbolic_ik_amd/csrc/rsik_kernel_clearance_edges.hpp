// rsik_kernel_clearance_edges.hpp — rsik_clearance_edges: the clearance of a path's joints ALONG the motion between its waypoints.  An
// edge runs from the waypoint before (or the start row) to a waypoint, joint by joint the short way round; it is sampled at S + 1
// sub-steps, each sample's clearance is rsik_clearance's of the sample's joints, and the least of them, where it lies, its pair and a
// lower bound on the clearance of the continuous motion are the edge's outputs (clearance_edges_kernel).  The per-path minima are a
// second, small launch over the edges' results (clearance_edges_fold_kernel).
#pragma once

#include "rsik_kernel_path.hpp"         // path_links, path_pairs
#include "rsik_kernel_track_avoid.hpp"  // kAvoidMaxSpheres, kAvoidMaxCapsules
#include "rsik_rows.hpp"
#include "rsik_tables.hpp"

namespace rsik {

struct ClearanceEdgesArgs {
    int64_t n;               // paths
    int64_t n_steps;         // waypoints per path; every per-edge array is [n_steps][n], waypoint-major
    const double* joints;    // [n_steps][n][7]
    const uint8_t* arm;      // [n] or NULL
    const double* start;     // [n][7] or NULL
    const double* spheres;   // [n_spheres][4]: x, y, z, r
    const double* capsules;  // [n_capsules][7]: a, b, r
    double* edge_clearance;  // [n_steps][n] or NULL
    int32_t* edge_sub;       // [n_steps][n] or NULL
    int32_t* edge_nearest;   // [n_steps][n][2] or NULL: (link, obstacle)
    double* edge_bound;      // [n_steps][n] or NULL
    double* ws_clearance;    // workspace, [n_steps][n] each, or NULL where no path output is asked for: what the fold reads
    double* ws_bound;
    int32_t* ws_sub;
    double* path_clearance;  // [n] or NULL
    int32_t* path_edge;      // [n][2] or NULL: (t, s)
    double* path_bound;      // [n] or NULL
    int32_t* n_below;        // [n] or NULL
    int32_t* first_below;    // [n] or NULL
    int n_sub;               // S
    int lanes;               // lanes per edge: a power of two, 1 ... 64 (the host's choice; no output depends on it)
    int fold_lanes;          // lanes per path in the fold: the same
    int n_spheres, n_capsules;
    double min_clearance;
    double link_radius[3];
    double sweep[2][3];      // per arm slot: R_0 = R_1, R_2 = R_3, R_4 = R_5 = R_6 of rsik.h (the host forms them)
    ArmC arms[2];            // as FkArgs.arms
};

// Workgroups the host launches per compute unit: what the kernel's registers leave resident (docs/experiments.md CE.1).
constexpr int kEdgeBlocksPerCu = 4;
constexpr int kEdgeNoSample = 0x7fffffff;  // the sub-step of a lane without a sample: every sample's is below it

// (d, s, code) of two samples: the smaller d, the lower s among equal d.  A total order (no two samples of an edge share s, d is never
// a NaN), so the minimum does not depend on how the samples are spread over lanes and trips.
__device__ __forceinline__ void edge_take(double& d, int& s, int& code, double od, int os, int oc) {
    const bool win = od < d || (od == d && os < s);
    d = win ? od : d;
    s = win ? os : s;
    code = win ? oc : code;
}

// `lanes` neighbouring lanes share an edge, 64 / lanes edges per wave, kBlock / lanes per workgroup; a workgroup strides over the
// edges in the order of the outputs (edge = t * n + path), so that neighbouring groups read and write neighbouring rows.
//   scene      staged ONCE per workgroup, as solve_path_kernel over PathClearArgs stages it (track_avoid_kernel's layout and validity
//              test), ahead of the tables' barrier; it stays for every edge the workgroup takes.
//   an edge    b = its row; a = the row of the waypoint before, where that row is numbers — else (rare) a walk back over the rows
//              that are not, down to the start row; delta = angle_diff(b, a), seven of them.  Every lane of the group does this for
//              itself: the loads are the same addresses.  Only the two rows' addresses are kept across the samples.
//   a sample   lane l of the group takes s = l, l + lanes, ...: q = a + delta * (s / S) (one division, a product, a sum; the build's
//              -ffp-contract=off keeps them apart), q(S) = b by a select; path_links and path_pairs on q: clearance_kernel's
//              expressions, hence rsik_clearance's bits for q.  A trip in which no lane of the wave holds a sample is skipped.
//   the fold   edge_take over the lane's own samples, then over the group by lane exchanges (a butterfly: every lane ends with the
//              group's minimum); nothing per sample reaches memory.  The group's first lane stores.
// No branch depends on data but the walk back, the far-angle branch of path_links and the skipped trips.
template <bool MIXED>
__global__ __launch_bounds__(kBlock, 4) void clearance_edges_kernel(const ClearanceEdgesArgs K) {
    __shared__ SharedTables lds_tab;
    __shared__ __attribute__((aligned(16))) double lds_sph[kAvoidMaxSpheres * 4];
    __shared__ __attribute__((aligned(16))) double lds_cap[kAvoidMaxCapsules * 8];
    static_assert(sizeof(SharedTables) + sizeof(g_sincos_tab) + sizeof(double) * (kAvoidMaxSpheres * 4 + kAvoidMaxCapsules * 8) <= 64 * 1024,
                  "the static LDS of a workgroup: tables and the staged scene");
    for (int o = threadIdx.x; o < K.n_spheres; o += kBlock) {  // n_spheres <= kAvoidMaxSpheres, n_capsules <= kAvoidMaxCapsules: the host refuses anything else
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
    stage_tables<MIXED>(lds_tab, K.arms);  // (ends with the barrier that also stands behind the scene)

    const int G = K.lanes;
    const int shift = __builtin_ctz((unsigned)G);
    const int lane = threadIdx.x & 63;
    const int gl = lane & (G - 1);  // this lane's place in its group
    const int S = K.n_sub;
    const int trips = (S + G) >> shift;  // ceil((S + 1) / G)
    const int64_t n = K.n;
    const int64_t edges = K.n_steps * n;
    const int64_t per_block = kBlock >> shift;
    const int64_t stride = (int64_t)gridDim.x * per_block;
    const int64_t wave_group = (int64_t)((threadIdx.x & ~63u) >> shift);  // the wave's first group among the workgroup's
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    const double sd = (double)S;
    const bool has_start = K.start != nullptr;

#pragma clang loop unroll(disable)
    for (int64_t e0 = (int64_t)blockIdx.x * per_block + wave_group; e0 < edges; e0 += stride) {  // (wave-uniform)
        const int64_t e_raw = e0 + (lane >> shift);
        const bool live = e_raw < edges;
        const int64_t e = live ? e_raw : edges - 1;  // a group past the end works on the last edge and stores nothing
        const int64_t t = e / n, i = e - t * n;
        const bool isl = MIXED ? (K.arm[i] != 0) : false;
        const Acc<MIXED> A = make_acc<MIXED>(K.arms, isl, lds_tab);

        // Where the rows lie, not the rows: pb = row (t, i), pa = the row the edge starts from (NULL: none).  A sample reads both
        // again (the same cache lines) and forms delta again, the same expression on the same operands each time, so that nothing of
        // the edge but two addresses stays in registers across the pair loop — which is what makes a fourth wave per SIMD fit.
        const double* pb = K.joints + e * 7;
        const double* pa = nullptr;
        bool wp, lost = false;
        {
            double r[7];
#pragma unroll
            for (int k = 0; k < 7; k++) r[k] = pb[k];
            wp = all_finite(r);
            if (t > 0) {
                const double* p = pb - n * 7;
#pragma unroll
                for (int k = 0; k < 7; k++) r[k] = p[k];
                bool found = all_finite(r);
                if (RSIK_RARE(!found)) {  // the row before is no waypoint: back to the last one that is
                    for (int64_t tb = t - 2; tb >= 0 && !found; tb--) {
                        p -= n * 7;
#pragma unroll
                        for (int k = 0; k < 7; k++) r[k] = p[k];
                        found = all_finite(r);
                    }
                }
                pa = found ? p : nullptr;
            }
            if (has_start) {  // rsik.h: a start row that holds something that is not a number loses its path
                const double* p = K.start + i * 7;
#pragma unroll
                for (int k = 0; k < 7; k++) r[k] = p[k];
                lost = !all_finite(r);
                pa = pa ? pa : p;
            }
        }
        wp = wp && !lost;  // row t is a waypoint of a path that has not lost itself
        const bool have_a = wp && pa != nullptr;
        pa = have_a ? pa : pb;  // (never read as a value where have_a is false; a valid address for the loads)
        const int first_s = have_a ? 0 : S;  // without a row before: the one-sample edge {b}, numbered S
        const auto row_b = [&](int k) { return wp ? pb[k] : 0.0; };  // (an edge that is none works on zeros)
        const auto row_a = [&](int k) { return have_a ? pa[k] : 0.0; };
        const auto delta_of = [&](double bk, double ak) { return have_a ? angle_diff(bk, ak) : 0.0; };

        double best_d = inf;
        int best_s = kEdgeNoSample, best_code = -1;
#pragma clang loop unroll(disable)
        for (int trip = 0; trip < trips; trip++) {
            const int s_raw = (trip << shift) + gl;
            const bool valid = wp && live && s_raw <= S && s_raw >= first_s;
            if (__builtin_amdgcn_ballot_w64(valid) == 0) continue;  // (scalar)
            const int s = s_raw < S ? s_raw : S;
            const double frac = (double)s / sd;
            double q[7];
#pragma unroll
            for (int k = 0; k < 7; k++) {
                const double bk = row_b(k), ak = row_a(k);
                const double step = delta_of(bk, ak) * frac;
                const double v = ak + step;
                q[k] = s == S ? bk : v;
            }
            V3 P[4], el[3];
            path_links(A, q, P, el);
            const ClrBest B = path_pairs(P, el, K.link_radius, K.n_spheres, K.n_capsules, lds_sph, lds_cap);
            edge_take(best_d, best_s, best_code, valid ? B.c : inf, valid ? s_raw : kEdgeNoSample, B.code);
        }
#pragma clang loop unroll(disable)
        for (int m = 1; m < G; m <<= 1) {  // (every lane of the wave: G is the launch's)
            const double od = __shfl_xor(best_d, m);
            const int os = __shfl_xor(best_s, m), oc = __shfl_xor(best_code, m);
            edge_take(best_d, best_s, best_code, od, os, oc);
        }

        if (live && gl == 0) {
            // acc = sum_k |delta_k| R_k, k = 0 ... 6 in order, unfused; 0 for the one-sample edge (its deltas are zeros)
            const double r0 = (MIXED && isl) ? K.sweep[1][0] : K.sweep[0][0];
            const double r2 = (MIXED && isl) ? K.sweep[1][1] : K.sweep[0][1];
            const double r4 = (MIXED && isl) ? K.sweep[1][2] : K.sweep[0][2];
            const double R[7] = {r0, r0, r2, r2, r4, r4, r4};
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 7; k++) acc = acc + fabs(delta_of(row_b(k), row_a(k))) * R[k];
            const double bound = best_d - 0.5 * (acc / sd);
            const bool none = best_code < 0;  // every obstacle was skipped
            const int link = none ? 0 : (best_code & 3), obs = none ? 0 : (best_code >> 2);
            const double out_d = wp ? best_d : nan, out_b = wp ? bound : nan;
            const int32_t out_s = wp ? best_s : -1;
            const unsigned long long word = (!wp || none) ? ~0ull : ((unsigned long long)(unsigned)obs << 32) | (unsigned)link;  // (link, obstacle)
            if (K.edge_clearance) st_stream(K.edge_clearance + e, out_d);
            if (K.edge_sub) st_stream(K.edge_sub + e, out_s);
            if (K.edge_nearest) st_stream((unsigned long long*)K.edge_nearest + e, word);
            if (K.edge_bound) st_stream(K.edge_bound + e, out_b);
            if (K.ws_clearance) {  // (plain stores: the fold reads them next)
                K.ws_clearance[e] = out_d;
                K.ws_bound[e] = out_b;
                K.ws_sub[e] = out_s;
            }
        }
    }
}

// The per-path outputs, over the edges' results in the workspace: `fold_lanes` neighbouring lanes share a path, lane l of them takes the
// waypoints t = l, l + fold_lanes, ..., then a butterfly over the group.  The least edge_clearance and its (t, s) — strictly less, then
// the lower t: a total order, so the answer does not depend on fold_lanes —, the least edge_bound, the edges below min_clearance and the
// first of them.  An edge whose sub-step is -1 is none.  A path without an edge: NaN, (-1, -1), NaN, 0, -1.
__global__ __launch_bounds__(kBlock) void clearance_edges_fold_kernel(const ClearanceEdgesArgs K) {
    const int P = K.fold_lanes;
    const int shift = __builtin_ctz((unsigned)P);
    const int pl = threadIdx.x & (P - 1);
    const int64_t i_raw = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> shift;
    const bool live = i_raw < K.n;
    const int64_t i = live ? i_raw : K.n - 1;  // a group past the end works on the last path and stores nothing
    const int T = (int)K.n_steps;
    double pc = __builtin_inf(), pb = __builtin_inf();
    int pt = kEdgeNoSample, ps = -1, below = 0, first = kEdgeNoSample;
    for (int t = pl; t < T; t += P) {
        const int64_t e = (int64_t)t * K.n + i;
        const int s = K.ws_sub[e];
        const double c = K.ws_clearance[e], bd = K.ws_bound[e];
        const bool edge = s >= 0;
        const bool win = edge && (c < pc || (c == pc && t < pt));
        pc = win ? c : pc;
        pt = win ? t : pt;
        ps = win ? s : ps;
        pb = (edge && bd < pb) ? bd : pb;
        const bool low = edge && c < K.min_clearance;
        below += low ? 1 : 0;
        first = (low && t < first) ? t : first;
    }
#pragma clang loop unroll(disable)
    for (int m = 1; m < P; m <<= 1) {  // (every lane of the wave: P is the launch's)
        const double oc = __shfl_xor(pc, m), ob = __shfl_xor(pb, m);
        const int ot = __shfl_xor(pt, m), os = __shfl_xor(ps, m), obelow = __shfl_xor(below, m), ofirst = __shfl_xor(first, m);
        const bool win = oc < pc || (oc == pc && ot < pt);
        pc = win ? oc : pc;
        pt = win ? ot : pt;
        ps = win ? os : ps;
        pb = ob < pb ? ob : pb;
        below += obelow;
        first = ofirst < first ? ofirst : first;
    }
    if (!live || pl != 0) return;
    const bool any = pt != kEdgeNoSample;
    const double nan = __builtin_nan("");
    if (K.path_clearance) st_stream(K.path_clearance + i, any ? pc : nan);
    if (K.path_edge) st_stream((unsigned long long*)K.path_edge + i, any ? ((unsigned long long)(unsigned)ps << 32) | (unsigned)pt : ~0ull);  // (t, s)
    if (K.path_bound) st_stream(K.path_bound + i, any ? pb : nan);
    if (K.n_below) st_stream(K.n_below + i, (int32_t)below);
    if (K.first_below) st_stream(K.first_below + i, (int32_t)(first == kEdgeNoSample ? -1 : first));
}

}  // namespace rsik
