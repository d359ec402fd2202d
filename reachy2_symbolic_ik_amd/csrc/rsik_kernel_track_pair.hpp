// rsik_kernel_track_pair.hpp — rsik_track_pair: rsik_track_avoid for robots of two arms that avoid each other (track_pair_kernel).  Row
// 2i is the right arm of robot i, row 2i + 1 its left arm; the two sit in neighbouring lanes of one wave.  A step is
// track_avoid_kernel's step (rsik_kernel_track_avoid.hpp) with three obstacles more in its pair loop: the partner's three links as
// capsules, formed from the partner's four link points of the same step, which the two lanes swap in registers.
//
// avoid_chain, avoid_levers, avoid_pick and the pair tests of clearance_kernel are called.  The step around them is
// track_avoid_kernel's restated, and not shared, for the reason written above jr_columns: as a function of both kernels it would have
// to compile in both exactly as it does now.
#pragma once

#include "rsik_kernel_track_avoid.hpp"  // TrackAvoidArgs, avoid_chain, avoid_levers, avoid_pick; through it clr_*, damping_usable, jr_tri

namespace rsik {

// The value the neighbouring lane (lane ^ 1) holds: two 32-bit DPP moves, quad_perm [1,0,3,2].  No LDS, no barrier; every lane of
// the wave must be active, so it stands in uniform control flow.
__device__ __forceinline__ double pair_swap(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0xB1, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), 0xB1, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ V3 pair_swap(V3 a) { return V3{pair_swap(a.x), pair_swap(a.y), pair_swap(a.z)}; }

// track_avoid_kernel (its comment describes the staging, the step, the stores and the variants; all of that is kept) for
// K.n = 2 n_pairs rows, K.arm not read: the arm of a row is its parity, which is the lane's (a wave starts at an even row).
//   partner    the four link points P[0 .. 3] that avoid_chain leaves go to lane ^ 1 and the partner's come back: 24 DPP moves per
//              step behind the capsule loop (the partner's P[0] ahead of the three trips, its P[l + 1] in trip l, so that two points
//              are live across a trip and not four), in every trip that gets as far as the pair loop, the one after the last step
//              included when min_clearance is asked for.  Both lanes hold the joints from BEFORE the step, so the two arms see each
//              other's state of the same instant and their order does not matter.  A partner that is NaN (start, rest, damping) has
//              NaN link points beyond its shoulder.
//   pair loop  after the staged capsules, the partner's link l as the capsule (Q0, Q1, link_radius[l]) = the partner's (P[l], P[l + 1]),
//              obstacle index n_spheres + n_capsules + l: its direction is Q1 - Q0, as clearance_kernel forms a capsule's from its
//              row (not the partner's own e[l]), so that a step's clearance is rsik_clearance's to the bit for that row.  A link with
//              a point that is not a number gets a NaN radius, which is what staging does to such a row: never the nearest.
//   winner     a third source beside the LDS sphere and the LDS capsule: the partner's link, its four points fetched again (24 moves:
//              the partner cannot know which link this lane wants), its two ends picked BY VALUE (avoid_pick), then the same point
//              at t.
//   past the end   a lane past the last row stays active, works on the last pair (row n - 2 + its parity) and stores nothing: its
//              partner is the lane past the end beside it.  n is even and a wave starts at a multiple of 64, so a pair never
//              straddles a wave and a live lane's partner is live.
//   variants   FF, LIM as track_avoid_kernel; the constants always come from LDS (Acc<true>): 4 instantiations.
// No branch depends on data but the far-angle one of the chain, and the order of every sum is fixed.
template <bool FF, bool LIM>
__global__ __launch_bounds__(kTrackBlock, 1) void track_pair_kernel(const TrackAvoidArgs K) {
    __shared__ SharedTables lds_tab;
    __shared__ double lds_rows[64 * 7];
    // What a lane carries through the whole loop and touches once a step, kept in LDS and not in registers (each lane reads what it
    // wrote itself, k * 64 + lane: no fence, no bank conflict): its rest row and its running minimum.  16 registers fewer across the
    // pair loop, which is what the partner's points and the third source of the winner take; with them in registers one value of
    // the loop spills in three of the four forms.
    __shared__ double lds_rest[7 * 64], lds_min[64];
    __shared__ __attribute__((aligned(16))) double lds_sph[kAvoidMaxSpheres * 4];
    __shared__ __attribute__((aligned(16))) double lds_cap[kAvoidMaxCapsules * 8];
    const int lane = threadIdx.x;
    const int64_t wave_row = (int64_t)blockIdx.x * kTrackBlock;  // < n: the grid has ceil(n / 64) workgroups
    // the obstacles, once: n_spheres <= kAvoidMaxSpheres and n_capsules <= kAvoidMaxCapsules (the host refuses anything else)
    for (int o = lane; o < K.n_spheres; o += kTrackBlock) {
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = K.spheres[(int64_t)o * 4 + k];
        if (!(all_finite(v) && v[3] >= 0.0)) v[3] = __builtin_nan("");
#pragma unroll
        for (int k = 0; k < 4; k++) lds_sph[o * 4 + k] = v[k];
    }
    for (int o = lane; o < K.n_capsules; o += kTrackBlock) {
        double v[7];
#pragma unroll
        for (int k = 0; k < 7; k++) v[k] = K.capsules[(int64_t)o * 7 + k];
        if (!(all_finite(v) && v[6] >= 0.0)) v[6] = __builtin_nan("");
#pragma unroll
        for (int k = 0; k < 7; k++) lds_cap[o * 8 + k] = v[k];
        lds_cap[o * 8 + 7] = 0.0;
    }
    stage_tables<true, 0, kTrackBlock>(lds_tab, K.arms);  // (ends with the barrier that also stands behind the obstacles)
    const int64_t row = wave_row + lane;
    const bool live = row < K.n;
    const int64_t r = live ? row : K.n - 2 + (lane & 1);  // a lane past the end works on the last pair and stores nothing
    const Acc<true> A = make_acc<true>(K.arms, (lane & 1) != 0, lds_tab);
    const int64_t w_end = K.n;
    int64_t rows_here = K.n - wave_row;
    if (rows_here > 64) rows_here = 64;
    const int ff_total = (int)rows_here * 6;
    const int ff_mine = (live ? lane : (int)rows_here - 2 + (lane & 1)) * 6;  // staged_row's index, with the last PAIR past the end
    const bool has_rest = K.rest_joints != nullptr;  // (uniform)

    double q[7], rest[7];
#pragma unroll
    for (int k = 0; k < 7; k++) q[k] = K.start_joints[r * 7 + k];
#pragma unroll
    for (int k = 0; k < 7; k++) rest[k] = has_rest ? K.rest_joints[r * 7 + k] : 0.0;
    const double lambda = K.damping ? ld_stream(K.damping + r) : K.damping_host;
    // the first step's goal and feed-forward; from here on step t + 1's are loaded while step t computes
    double g[12], ffs[6];
    const double* goal_col = K.m12_steps + r;
#pragma unroll
    for (int k = 0; k < 12; k++) g[k] = ld_stream(goal_col + k * K.n);
    if constexpr (FF) {
#pragma unroll
        for (int k = 0; k < 6; k++) ffs[k] = (k * 64 + lane < ff_total) ? ld_stream(K.feedforward + wave_row * 6 + k * 64 + lane) : 0.0;
    }

    const double nan = __builtin_nan("");
    const double l2 = lambda * lambda;
    const bool bad = !all_finite(q) || !damping_usable(lambda) || !all_finite(rest);
#pragma unroll
    for (int k = 0; k < 7; k++) lds_rest[k * 64 + lane] = rest[k];
    lds_min[lane] = __builtin_inf();
    if (bad) {  // (as track_kernel: NaN from the start, every step held; the partner sees NaN link points)
#pragma unroll
        for (int k = 0; k < 7; k++) q[k] = nan;
    }

    const bool want_final_err = K.final_err != nullptr, want_min = K.min_clearance != nullptr;
    const int n_static = K.n_spheres + K.n_capsules;  // the partner's links are the obstacles n_static, n_static + 1, n_static + 2
    double qd_out[7], err_out[2], clr_out = nan;  // what the step before leaves for the head of the next trip to store
    unsigned long long near_out = ~0ull;
#pragma clang loop unroll(disable)
    for (int64_t t = 0; t <= K.n_steps; t++) {
        const bool last_look = t == K.n_steps;  // (uniform) the trip after the last step: its stores and the final outputs
        double gc[12], ffc[6];
#pragma unroll
        for (int k = 0; k < 12; k++) gc[k] = g[k];
        if constexpr (FF) {
#pragma unroll
            for (int k = 0; k < 6; k++) ffc[k] = ffs[k];
        }
        // the wave waits HERE for this step's goal and feed-forward, issued a whole step ago: see track_kernel
        asm volatile("" ::"v"(gc[0]), "v"(gc[1]), "v"(gc[2]), "v"(gc[3]), "v"(gc[4]), "v"(gc[5]), "v"(gc[6]), "v"(gc[7]), "v"(gc[8]),
                     "v"(gc[9]), "v"(gc[10]), "v"(gc[11]) : "memory");
        if constexpr (FF) asm volatile("" ::"v"(ffc[0]), "v"(ffc[1]), "v"(ffc[2]), "v"(ffc[3]), "v"(ffc[4]), "v"(ffc[5]) : "memory");
        // 8. the stores of the step before, then the loads of the step after: both have this step's arithmetic to complete in
        if (t > 0) {
            if (K.clearance_steps != nullptr && live) st_stream(K.clearance_steps + (t - 1) * K.n + row, clr_out);
            if (K.nearest_steps != nullptr && live) st_stream((unsigned long long*)K.nearest_steps + (t - 1) * K.n + row, near_out);
            if (K.err_steps != nullptr) store_rows<2>(K.err_steps + (t - 1) * K.n * 2, wave_row, w_end, lane, lds_rows, err_out);
            if (K.rates_steps != nullptr) store_rows<7>(K.rates_steps + (t - 1) * K.n * 7, wave_row, w_end, lane, lds_rows, qd_out);
            if (K.joints_steps != nullptr || (last_look && K.final_joints != nullptr)) {
                double out[7];
#pragma unroll
                for (int k = 0; k < 7; k++) out[k] = bad ? nan : q[k];
                if (K.joints_steps != nullptr) store_rows<7>(K.joints_steps + (t - 1) * K.n * 7, wave_row, w_end, lane, lds_rows, out);
                if (last_look && K.final_joints != nullptr) store_rows<7>(K.final_joints, wave_row, w_end, lane, lds_rows, out);
            }
        }
        if (last_look && !want_final_err && !want_min) break;
        if (t + 1 < K.n_steps) {  // (uniform) the next step's inputs: issued here, used a step later
            const double* next = goal_col + (t + 1) * 12 * K.n;
#pragma unroll
            for (int k = 0; k < 12; k++) g[k] = ld_stream(next + k * K.n);
            if constexpr (FF) {
                const double* slab = K.feedforward + ((t + 1) * K.n + wave_row) * 6;
#pragma unroll
                for (int k = 0; k < 6; k++) ffs[k] = (k * 64 + lane < ff_total) ? ld_stream(slab + k * 64 + lane) : 0.0;
            }
        }
        bool skip = !all_finite(gc);
        double v[6];
        if constexpr (FF) {  // the wave's slab of this step -> LDS -> each lane's row
            if (!last_look) {
#pragma unroll
                for (int k = 0; k < 6; k++) lds_rows[k * 64 + lane] = ffc[k];
                rows_staged();
#pragma unroll
                for (int k = 0; k < 6; k++) v[k] = lds_rows[ff_mine + k];
                rows_staged();
                skip = skip || !all_finite(v);
            }
        }

        // 1. forward kinematics, the joint axes and the links
        double qa[7];
#pragma unroll
        for (int k = 0; k < 7; k++) qa[k] = q[k];
        V3 ang[7], fx, pos, P[4], e[3];
        double R[9];
        avoid_chain<true>(A, qa, ang, fx, pos, R, P, e);

        // 2. pose error: e_p = p_g - p, e_o the rotation vector of D = Rg R^T.  (2 and 3 stand AHEAD of the pair loop: the goal, the
        // position and the rotation end here, and the loop has their registers.)
        const V3 ep = {gc[9] - pos.x, gc[10] - pos.y, gc[11] - pos.z};
        const auto D = [&](int i, int j) { return fma(gc[3 * i], R[3 * j], fma(gc[3 * i + 1], R[3 * j + 1], gc[3 * i + 2] * R[3 * j + 2])); };
        const V3 w = {0.5 * (D(2, 1) - D(1, 2)), 0.5 * (D(0, 2) - D(2, 0)), 0.5 * (D(1, 0) - D(0, 1))};
        const double c = 0.5 * (((D(0, 0) + D(1, 1)) + D(2, 2)) - 1.0);
        const double s2 = dot(w, w), ep2 = dot(ep, ep);
        const double s = s2 > 0.0 ? sqrt_cr(s2) : 0.0;
        const double angle = fast_atan2(s, c);
        const double ep_norm = ep2 < __builtin_inf() ? sqrt_cr(ep2) : __builtin_inf();
        double err[2] = {ep2 > 0.0 ? ep_norm : 0.0, angle};
        if (last_look && want_final_err) {  // (uniform)
            double fe[2];
#pragma unroll
            for (int k = 0; k < 2; k++) fe[k] = (bad || skip) ? nan : err[k];
            store_rows<2>(K.final_err, wave_row, w_end, lane, lds_rows, fe);
        }
        const double scale = s2 >= 0x1p-52 ? angle * fast_rcp(s) : 1.0;
        const V3 eo = w * scale;

        // 3. twist
        if constexpr (FF) {
            v[0] = fma(K.kp, ep.x, v[0]); v[1] = fma(K.kp, ep.y, v[1]); v[2] = fma(K.kp, ep.z, v[2]);
            v[3] = fma(K.ko, eo.x, v[3]); v[4] = fma(K.ko, eo.y, v[4]); v[5] = fma(K.ko, eo.z, v[5]);
        } else {
            v[0] = K.kp * ep.x; v[1] = K.kp * ep.y; v[2] = K.kp * ep.z;
            v[3] = K.ko * eo.x; v[4] = K.ko * eo.y; v[5] = K.ko * eo.z;
        }
        // 4a. the clearance of q, its pair and its gradient: clearance_kernel's loop over the staged obstacles, then the partner's
        // three links, and its winner
        double grad[7] = {}, clr = nan;
        if (!last_look || want_min) {  // (uniform)
            double ee[3], inv_ee[3];
#pragma unroll
            for (int l = 0; l < 3; l++) { ee[l] = dot(e[l], e[l]); inv_ee[l] = clr_rcp(ee[l]); }
            ClrBest B = {__builtin_inf(), 0.0, 0.0, -1};
#pragma unroll 4  // (as track_avoid_kernel)
            for (int o = 0; o < K.n_spheres; o++) {
                const V3 C = {lds_sph[o * 4], lds_sph[o * 4 + 1], lds_sph[o * 4 + 2]};
                const double ro = lds_sph[o * 4 + 3];
#pragma unroll
                for (int l = 0; l < 3; l++) clr_point<true>(B, P[l], e[l], inv_ee[l], K.link_radius[l], C, ro, 4 * o + l);
            }
#pragma clang loop unroll(disable)
            for (int o = 0; o < K.n_capsules; o++) {
                const V3 Q0 = {lds_cap[o * 8], lds_cap[o * 8 + 1], lds_cap[o * 8 + 2]};
                const V3 Q1 = {lds_cap[o * 8 + 3], lds_cap[o * 8 + 4], lds_cap[o * 8 + 5]};
                const double ro = lds_cap[o * 8 + 6];
                const V3 fq = Q1 - Q0;
                const double ff = dot(fq, fq), inv_ff = clr_rcp(ff);
#pragma unroll
                for (int l = 0; l < 3; l++)
                    clr_segment<true>(B, P[l], e[l], ee[l], inv_ee[l], K.link_radius[l], Q0, fq, ff, inv_ff, ro, 4 * (K.n_spheres + o) + l);
            }
            // The partner's links as this lane's obstacles, each tested as staging tests a capsule's row.  One copy of the three tests,
            // like the capsule loop (unrolled, the nine tests spill), and the partner's points fetched as the loop needs them: its
            // P[0] ahead of it, its P[lp + 1] in trip lp, so that two points are live across a trip and not four.  (Uniform control
            // flow: the tests that lead here are of the argument block and of the trip, so every lane of the wave is here.)
            V3 Q1 = pair_swap(P[0]);
#pragma clang loop unroll(disable)
            for (int lp = 0; lp < 3; lp++) {
                const V3 Q0 = Q1;
                Q1 = pair_swap(avoid_pick(lp, P[1], P[2], P[3]));
                const double ends[6] = {Q0.x, Q0.y, Q0.z, Q1.x, Q1.y, Q1.z};
                const double ro = all_finite(ends) ? avoid_pick(lp, K.link_radius[0], K.link_radius[1], K.link_radius[2]) : nan;
                const V3 fq = Q1 - Q0;
                const double ff = dot(fq, fq), inv_ff = clr_rcp(ff);
#pragma unroll
                for (int l = 0; l < 3; l++)
                    clr_segment<true>(B, P[l], e[l], ee[l], inv_ee[l], K.link_radius[l], Q0, fq, ff, inv_ff, ro, 4 * (n_static + lp) + l);
            }
            const bool none = B.code < 0;  // every obstacle was skipped
            const int link = none ? 0 : (B.code & 3), obs = none ? 0 : (B.code >> 2);
            clr = bad ? nan : B.c;
            double min_clr = lds_min[lane];
            min_clr = B.c < min_clr ? B.c : min_clr;
            lds_min[lane] = min_clr;
            clr_out = clr;  // (both ahead of the branch, in the last look too, where nothing reads them: inside it they spill)
            near_out = (bad || none) ? ~0ull : ((unsigned long long)(unsigned)obs << 32) | (unsigned)link;  // (link, obstacle)
            if (last_look) {
                if (live) st_stream(K.min_clearance + row, bad ? nan : min_clr);  // (want_min holds here)
            } else {
                // the winner's obstacle again: a sphere's centre from LDS, or the point at t of a capsule from LDS or of the partner's
                // link from registers (a winner is never a skipped row, so what is held of it is what the caller holds)
                const bool is_sphere = obs < K.n_spheres, is_partner = obs >= n_static;
                const int so = is_sphere ? obs : 0, co = (is_sphere || is_partner) ? 0 : obs - K.n_spheres, lp = obs - n_static;
                const V3 C = {lds_sph[so * 4], lds_sph[so * 4 + 1], lds_sph[so * 4 + 2]};
                const V3 S0 = {lds_cap[co * 8], lds_cap[co * 8 + 1], lds_cap[co * 8 + 2]};
                const V3 S1 = {lds_cap[co * 8 + 3], lds_cap[co * 8 + 4], lds_cap[co * 8 + 5]};
                V3 PP[4];  // (the partner does not know which of its links this lane wants: all four points again, then the pick)
#pragma unroll
                for (int l = 0; l < 4; l++) PP[l] = pair_swap(P[l]);
                const V3 T0 = avoid_pick(lp, PP[0], PP[1], PP[2]), T1 = avoid_pick(lp, PP[1], PP[2], PP[3]);
                const V3 Q0 = {is_partner ? T0.x : S0.x, is_partner ? T0.y : S0.y, is_partner ? T0.z : S0.z};
                const V3 Q1 = {is_partner ? T1.x : S1.x, is_partner ? T1.y : S1.y, is_partner ? T1.z : S1.z};
                const V3 yc = madd(Q1 - Q0, B.t, Q0);
                const V3 y = {is_sphere ? C.x : yc.x, is_sphere ? C.y : yc.y, is_sphere ? C.z : yc.z};
                const V3 Pl = avoid_pick(link, P[0], P[1], P[2]), el = avoid_pick(link, e[0], e[1], e[2]);
                const V3 x = madd(el, B.s, Pl);
                const V3 d = x - y;
                const double d2 = dot(d, d);
                const double inv_d = (!none && d2 >= kClrTiny) ? fast_rcp(sqrt_cr(d2)) : 0.0;  // touching axes, or no pair: the zero vector
                const V3 un = {none ? 0.0 : d.x * inv_d, none ? 0.0 : d.y * inv_d, none ? 0.0 : d.z * inv_d};
#pragma unroll
                for (int k = 0; k < 7; k++) {
                    const bool moves = !none && k < (link == 0 ? 2 : link == 1 ? 4 : 7);
                    const V3 arm_k = (none ? Pl : x) - (k < 2 ? P[0] : k < 4 ? P[1] : P[2]);
                    const double gk = dot(un, cross(ang[k], arm_k));
                    grad[k] = moves ? gk : 0.0;
                }
            }
        }

        if (last_look) break;

        // 4b. bias: the rest term, and the push where the clearance is below the influence distance (a select: +infinity, "no
        // obstacle usable", and a NaN trajectory never push)
        const bool push = clr < K.influence;
        const double gain = K.avoid_gain * (K.influence - clr);
        const bool biased = has_rest || push;
        double q0[7];
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const double rest_k = has_rest ? K.rest_gain * (lds_rest[k * 64 + lane] - q[k]) : 0.0;
            const double pushed = rest_k + gain * grad[k];
            q0[k] = push ? pushed : rest_k;
        }

        // 5. rates: joint_rates_kernel's residual, normal matrix, factorisation, solves and last sum
        V3 lin[7], lever[3];
        avoid_levers<true>(A, ang[2], fx, e[2], lever);
#pragma unroll
        for (int k = 0; k < 7; k++) lin[k] = cross(ang[k], k < 2 ? lever[0] : k < 4 ? lever[1] : lever[2]);
        const auto J = [&](int i, int k) {
            return i == 0 ? lin[k].x : i == 1 ? lin[k].y : i == 2 ? lin[k].z : i == 3 ? ang[k].x : i == 4 ? ang[k].y : ang[k].z;
        };
        double y[6];  // the residual, then z, then y
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double res = v[i];
#pragma unroll
            for (int k = 0; k < 7; k++) res = fma(-J(i, k), q0[k], res);
            y[i] = biased ? res : v[i];
        }
        double a[21];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
                double sum = i == j ? l2 : 0.0;
#pragma unroll
                for (int k = 0; k < 7; k++) sum = fma(J(i, k), J(j, k), sum);
                a[jr_tri(i, j)] = sum;
            }
        double inv[6];
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double d = a[jr_tri(j, j)];
            double wk[5];  // wk[k] = L[j][k] d_k
#pragma unroll
            for (int k = 0; k < j; k++) {
                wk[k] = a[jr_tri(j, k)] * a[jr_tri(k, k)];
                d = fma(-a[jr_tri(j, k)], wk[k], d);
            }
            d = fmax(d, l2);
            a[jr_tri(j, j)] = d;
            inv[j] = fast_rcp(d);
#pragma unroll
            for (int i = j + 1; i < 6; i++) {
                double sum = a[jr_tri(i, j)];
#pragma unroll
                for (int k = 0; k < j; k++) sum = fma(-a[jr_tri(i, k)], wk[k], sum);
                a[jr_tri(i, j)] = sum * inv[j];
            }
        }
#pragma unroll
        for (int i = 1; i < 6; i++)
#pragma unroll
            for (int k = 0; k < i; k++) y[i] = fma(-a[jr_tri(i, k)], y[k], y[i]);
#pragma unroll
        for (int i = 0; i < 6; i++) y[i] *= inv[i];
#pragma unroll
        for (int i = 4; i >= 0; i--)
#pragma unroll
            for (int k = i + 1; k < 6; k++) y[i] = fma(-a[jr_tri(k, i)], y[k], y[i]);
        double qd[7];
#pragma unroll
        for (int k = 0; k < 7; k++) {
            double sum = q0[k];
#pragma unroll
            for (int i = 0; i < 6; i++) sum = fma(J(i, k), y[i], sum);
            qd[k] = sum;
        }

        // rates that are not numbers: the step is held like a skipped one (see track_kernel)
        skip = skip || !all_finite(qd);

        // 6. rate limit: one factor for the seven joints, so the direction is kept
        if constexpr (LIM) {
            double m = fabs(qd[0]) / K.rate_max[0];
#pragma unroll
            for (int k = 1; k < 7; k++) m = fmax(m, fabs(qd[k]) / K.rate_max[k]);
            if (m > 1.0) {
#pragma unroll
                for (int k = 0; k < 7; k++) qd[k] = qd[k] / m;
            }
        }
        // 7. integration; a skipped step holds the joints and reports no motion
#pragma unroll
        for (int k = 0; k < 7; k++) {
            double moved = fma(K.dt, qd[k], q[k]);
            if constexpr (LIM) moved = fmin(fmax(moved, K.q_min[k]), K.q_max[k]);
            q[k] = skip ? q[k] : moved;
            qd[k] = skip ? 0.0 : qd[k];
        }
        // (8. the stores: at the head of the next trip)
#pragma unroll
        for (int k = 0; k < 2; k++) err_out[k] = (bad || skip) ? nan : err[k];
#pragma unroll
        for (int k = 0; k < 7; k++) qd_out[k] = bad ? nan : qd[k];
    }
}

}  // namespace rsik
