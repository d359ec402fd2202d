// rsik_cont_run.hpp — the host-side scheduler of rsik_control_continuous_run: plan, workspace, dependency words, issue order
// (a fragment by design, not a header that stands alone: host code included by rsik_lib.hip inside its extern "C" block, after the
// context, the error and launch helpers and fill_continuous, whose statics it uses)
//
// The dependency graph.  Streams: the caller's (start-up and theta kernels), prepare, joints, chain (the context's own).  Kernels on
// one stream run in issue order; what else a kernel waits for, by form — captured (events, a run recorded into a hipGraph, or variant
// bit 1), launch by launch (words), overlapping (words, behind a run of the same shape with RSIK_OPT_CONT_GOALS_RESIDENT):
//   start-up   caller's stream.  All forms: nothing but the stream (the previous run's end is on it).                [issue_start]
//              Before it the prepare stream forks: it waits for kWordPrepareMayFork, signalled on the caller's stream — captured
//              and launch by launch; overlapping it does not fork, it carries on behind the previous run's prepare kernels.
//              Behind it kWordInitDone is signalled and the joints and chain streams wait for it — captured and launch by launch;
//              overlapping they do not (their first kernels wait for theta kernels, which are behind the start-up kernel).
//   prepare(b) prepare stream.  Captured: chain(b - slots), from the block that reuses a slot on.                    [issue_prepare]
//              Launch by launch: the chain kernel that used the slot last, whichever run it belonged to (Cont::slot_use).
//              Overlapping, besides: b = 0 the previous run's last chain kernel has started (kEdgeChainStarted, last_seq), b = 1 this
//              run's start-up kernel has started (kWordInitStarted), b >= 2 theta(b - 2) has started (kEdgeThetaStarted); where the
//              two runs write the same reachable / state rows the previous run's chain(b), or its last chain kernel (b = 0).
//   theta(b)   caller's stream.  Captured and launch by launch: prepare(b) (kEdgePrepared).                          [issue_theta]
//              Overlapping: no stream wait — the kernel itself waits for the kEdgePrepared word (kWordGaveUp if it gives up).
//   joints(b)  joints stream.  Captured: theta(b) (kEdgeTheta).                                                      [issue_back]
//              Launch by launch: theta(b), then theta(b + 1) has started (kEdgeThetaStarted; not with variant bit 2).
//              Overlapping: theta(b + 1) has started, which says theta(b) is done (same stream); the last block: theta(b).
//   chain(b)   chain stream.  All forms: joints(b) (kEdgeJoints).                                                    [issue_back]
//   the end    the caller's stream waits for the last chain kernel (kEdgeChain), all forms.                          [issue_all]
//              Launch by launch and overlapping, Cont::run_done is recorded on the chain stream behind it.           [cont_run_end]
#pragma once

// the run number at which the words that tie the streams of rsik_control_continuous_run start over (a test build sets it to a handful)
#ifndef RSIK_EDGE_SEQ_WRAP
#define RSIK_EDGE_SEQ_WRAP 0xfffffff0u
#endif

// RSIK_OPT_CONT_PHASED_VARIANT, the bits besides RSIK_PHASED_EDGES_BY_EVENT and RSIK_PHASED_NO_THETA_FIRST (include/rsik.h)
constexpr int kVariantPrepareNotHeld = 4;        // (runs that overlap) the next run's prepare kernels not held at all
constexpr int kVariantPrepareBehindChainEnd = 8; // ... held until the previous run's last chain kernel has FINISHED
constexpr int kVariantThetaStreamWaits = 16;     // ... its theta kernels behind stream waits instead of waiting for their prepare kernels themselves
constexpr int kVariantNoTurnHint = 64;           // the joints phase without its turn hints (joints then differ in their last bits)

// The dependency words (launch by launch) / events (captured): kRunWords for the run, then kEdgeKinds per block.  Words are per
// (kind, block) and only ever grow.
enum RunWord { kWordInitDone, kWordPrepareMayFork, kWordInitStarted, kWordGaveUp, kRunWords };  // the start-up kernel is done / the prepare
// stream may fork / the start-up kernel has started / not a sequence number: a theta kernel's "gave up waiting" mark (rsik_sync)
enum EdgeKind { kEdgePrepared, kEdgeTheta, kEdgeJoints, kEdgeChain, kEdgeThetaStarted, kEdgeChainStarted, kEdgeKinds };  // the last two: words only
static size_t edge_id(EdgeKind kind, int64_t b) { return kRunWords + kEdgeKinds * (size_t)b + kind; }

int rsik_ctx::Cont::synced(rsik_ctx* ctx) {
    // a theta kernel that gave up waiting for its prepare kernel (cannot happen; the wait is bounded so that it cannot hang either)
    if (edge_words) {
        unsigned gave_up = 0;
        RSIK_HIP(ctx, hipMemcpyAsync(&gave_up, edge_words + kWordGaveUp, sizeof gave_up, hipMemcpyDeviceToHost, ctx->stream));
        RSIK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (gave_up != 0) {
            (void)hipMemsetAsync(edge_words + kWordGaveUp, 0, sizeof gave_up, ctx->stream);
            (void)hipStreamSynchronize(ctx->stream);
            return fail(ctx, RSIK_E_HIP, "rsik_sync: a theta kernel of rsik_control_continuous_run waited a second for its prepare kernel and went on without it: the results of that run are invalid");
        }
    }
    // workspaces that continuous runs outgrew: whatever was issued into them has finished now
    if (!outgrown_ws.empty()) {
        if (have_run_done) RSIK_HIP(ctx, hipEventSynchronize(run_done));
        free_all(outgrown_ws);
    }
    return RSIK_OK;
}
void rsik_ctx::Cont::release() {
    free_all(retired_ws);
    free_all(outgrown_ws);
    if (ws) (void)hipFree(ws);
    ws = nullptr;
    ws_bytes = 0;
    ws_captured = false;
    last_run.valid = false;
    reset_slots();
}
void rsik_ctx::Cont::destroy() {
    if (ws) (void)hipFree(ws);
    if (edge_words) (void)hipFree(edge_words);
    if (have_run_done) (void)hipEventDestroy(run_done);
    free_all(retired_ws);
    free_all(outgrown_ws);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    if (have_side)
        for (hipStream_t st : side) (void)hipStreamDestroy(st);
}

// The theta phase's specialised step (continuous_next_theta_lean) replaces limit_theta_to_interval's choice of the nearer
// interval end — |angle_diff(theta, l1)| < |angle_diff(theta, l0)|, U:105-111 — by one comparison with a threshold.  Here
// that threshold is found with the reference's own arithmetic (Python's float `%`), by bisection over the doubles of the
// gap, and the equivalence is then checked on a sample of the gap and on the doubles around the threshold; an interval
// for which it does not hold (or a rate limit the step's range analysis does not cover) keeps the generic step.
static double host_angle_diff(double a, double b) { return host_pymod((a - b) + rsik::kPi, 2 * rsik::kPi) - rsik::kPi; }
static int theta_snap_plan(double l0, double l1, double d_theta_max, double* tdag) {
    const double pi = rsik::kPi;
    *tdag = 0.0;
    if (!(d_theta_max >= 0.0 && d_theta_max < 3.0)) return rsik::kSnapGeneric;
    if (!(std::fabs(l0) <= pi && std::fabs(l1) <= pi)) return rsik::kSnapGeneric;
    if (l0 == l1 || (std::fabs(l0) == pi && std::fabs(l1) == pi)) return rsik::kSnapGeneric;  // the whole circle (U:468-474)
    auto nearer_is_l1 = [&](double t) { return std::fabs(host_angle_diff(t, l1)) < std::fabs(host_angle_diff(t, l0)); };
    const bool wrap = !(l0 < l1);
    // the stretch of the gap that starts at l1: up to l0 (wrap) or up to pi (the rest, (-pi, l0), must answer l0)
    double lo = l1, hi = wrap ? l0 : pi;
    if (!(lo < hi)) return rsik::kSnapGeneric;
    if (!nearer_is_l1(std::nextafter(lo, hi)) || nearer_is_l1(hi)) return rsik::kSnapGeneric;
    lo = std::nextafter(lo, hi);
    while (std::nextafter(lo, hi) < hi) {
        const double mid = lo + (hi - lo) / 2;
        if (nearer_is_l1(mid)) lo = mid; else hi = mid;
    }
    const double t = hi;  // the smallest double of the stretch for which l1 is not the nearer end
    auto agrees = [&](double x) {
        const bool valid = wrap ? (l0 <= x || x <= l1) : (l0 <= x && x <= l1);
        if (valid || !(x > -pi && x <= pi)) return true;
        const bool want = nearer_is_l1(x);
        const bool got = wrap ? (x < t) : (x >= l0 && x < t);  // (below l0 the specialised step answers l0)
        return want == got;
    };
    double x = t;
    for (int k = 0; k < 64; k++) { x = std::nextafter(x, -4.0); if (!agrees(x)) return rsik::kSnapGeneric; }
    x = t;
    for (int k = 0; k < 64; k++) { if (!agrees(x)) return rsik::kSnapGeneric; x = std::nextafter(x, 4.0); }
    const int samples = 4096;
    for (int k = 0; k <= samples; k++) {
        if (!agrees(-pi + (2 * pi) * k / samples)) return rsik::kSnapGeneric;
        if (!agrees(std::nextafter(l1, 4.0) + (t - l1) * k / samples)) return rsik::kSnapGeneric;
    }
    *tdag = t;
    return wrap ? rsik::kSnapWrap : rsik::kSnapInner;
}

// How rsik_control_continuous_run cuts a run of n trajectories x n_steps steps into blocks, what it needs for that, and where in the
// workspace everything lies: `slots` slots of slot_bytes, then theta_carry, then the run's turn hints.
struct ContPlan {
    int64_t T;                           // steps per block (the last one may be shorter)
    std::vector<int64_t> block_t0, block_T;
    size_t per_step, chunks_per_block, slot_bytes, need;
    size_t slot_hint_off;                // a slot's turn hints, from the slot's start (they sit at its end, whatever the block's length)
    size_t theta_carry_off, run_hint_off;  // theta_carry and the run's turn hints, from the workspace's start
    int slots;
    size_t n_events;
};
static size_t align256(size_t bytes) { return (bytes + 255) / 256 * 256; }
constexpr int kContSlots = 8;
static_assert(kContSlots == sizeof(rsik_ctx::Cont::slot_use) / sizeof(rsik_ctx::Cont::slot_use[0]), "rsik_ctx::Cont::slot_use holds one entry per workspace slot");  // workspace slots in flight (block b + 8 reuses the slot of block b once its chain phase has finished)
// `capturing`: the call is being recorded into a hipGraph.  A replay executes the dependency DAG with 15-40 us per edge
// whatever the streams were, so fewer, longer blocks pay there (4096 x 1000 steps replayed: 0.379 ms with two blocks,
// 0.383 with three, 0.395 with four); launched eagerly four blocks are best (0.43 against 0.46 with two: more overlap for
// the same host-side issue cost).  Round 5, after the value-word edges and the theta-first hold: three blocks are level with or 1-2 %
// ahead of four in every sweep (blocks of 256 / 352 steps: 0.370 / 0.363, 0.378 / 0.374, 0.373 / 0.367 ms on three boxes).
// `all_slots`: the workspace holds kContSlots slots whatever the number of blocks (RSIK_OPT_CONT_GOALS_RESIDENT: the next run's
// blocks take the slots this run's do not).
static int cont_plan(rsik_ctx* ctx, const char* who, int64_t n, int64_t n_steps, bool capturing, ContPlan& P, bool all_slots = false) {
    // (the sequential phases address a block's arrays through 2 GB buffer windows: rows of n * 56 bytes, blocks of <= 384 MB
    // of workspace, i.e. <= 1.3 GB of joints; every block costs the host four launches, so blocks are as long as that allows)
    if (n > (int64_t)30 << 20) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": more than 30 Mi trajectories in one call");
    P.per_step = (size_t)n * (2 * sizeof(double) + 1);
    int64_t T_max = (int64_t)((size_t)384 << 20) / (int64_t)P.per_step;
    if (T_max < 1) T_max = 1;
    if (T_max > 65535) T_max = 65535;  // gridDim.y
    // block size: a third of the run (a quarter until round 5), half of it under capture (the phases of neighbouring blocks overlap: more blocks, shorter fill and drain;
    // fewer blocks, fewer of the ~12 us hand-overs between dependent launches: 4096 x 1000 steps take 0.49 / 0.48 / 0.46 /
    // 0.48 / 0.50 ms with blocks of 128 / 192 / 256 / 512 / 1000 steps), a multiple of the theta batch and of the joint
    // chunk; RSIK_OPT_CONT_BLOCK_STEPS overrides
    const int64_t parts = capturing ? 2 : 3;
    int64_t T = ctx->options[RSIK_OPT_CONT_BLOCK_STEPS] > 0 ? ctx->options[RSIK_OPT_CONT_BLOCK_STEPS] : (n_steps + parts - 1) / parts;
    if (T < 64 && ctx->options[RSIK_OPT_CONT_BLOCK_STEPS] == 0) T = 64;
    // (round 6, runs of 2 000 ... 16 000 steps launch by launch: blocks of 512 steps 0.340-0.377 ms per 1000 steps where a third of
    // the run took 0.362-0.450 and blocks of 256 / 352 0.36-0.41 — profiles/r06/config5_long_runs.txt)
    if (!capturing && ctx->options[RSIK_OPT_CONT_BLOCK_STEPS] == 0 && T > 512) T = 512;
    T = (T + rsik::kSeqBatch - 1) / rsik::kSeqBatch * rsik::kSeqBatch;
    if (T > T_max) T = T_max >= rsik::kSeqBatch ? T_max / rsik::kSeqBatch * rsik::kSeqBatch : T_max;
    if (T > n_steps) T = n_steps;
    P.T = T;
    P.block_t0.clear(); P.block_T.clear();
    for (int64_t t0 = 0; t0 < n_steps; t0 += T) {
        P.block_t0.push_back(t0);
        P.block_T.push_back(n_steps - t0 < T ? n_steps - t0 : T);
    }
    const int64_t n_blocks = (int64_t)P.block_t0.size();
    P.chunks_per_block = ((size_t)T + rsik::kJointChunk - 1) / rsik::kJointChunk;
    const size_t hint_bytes = align256((size_t)n * sizeof(unsigned));  // a turn-hint array: the run's, a slot's
    P.slot_hint_off = align256((size_t)T * P.per_step + P.chunks_per_block * (size_t)n);
    P.slot_bytes = P.slot_hint_off + hint_bytes;
    P.slots = (n_blocks < kContSlots && !all_slots) ? (int)n_blocks : kContSlots;
    P.theta_carry_off = P.slot_bytes * P.slots;
    P.run_hint_off = P.theta_carry_off + align256((size_t)n * 2 * sizeof(double));
    P.need = P.run_hint_off + hint_bytes;
    P.n_events = kRunWords + kEdgeKinds * (size_t)n_blocks;  // per run 4, per block: prepared, theta, joints, chain, "theta / chain has started" (words only)
    return RSIK_OK;
}
// Workspace, side streams and events for a plan.  Nothing here may happen while the caller's stream is capturing (device
// allocation, stream and event creation are not capturable): a capture needs rsik_control_continuous_reserve, or an
// earlier run of at least this size, first.  An outgrown workspace is retired, not freed: a hipGraph captured earlier
// still points into it.
static int cont_resources(rsik_ctx* ctx, const char* who, size_t need, bool want_streams, size_t n_events) {
    rsik_ctx::Cont& C = ctx->cont;
    const bool grow = C.ws_bytes < need, streams = want_streams && !C.have_side, events = C.events.size() < n_events;
    if (!grow && !streams && !events) return RSIK_OK;
    if (stream_is_capturing(ctx->stream))
        return fail(ctx, RSIK_E_INVALID, std::string(who) + ": the stream is capturing and this run needs a larger workspace / its streams / "
                    "more events than the context holds: call rsik_control_continuous_reserve(ctx, n, n_steps) before the capture");
    if (grow) {
        // geometric growth (a sweep over rising sizes reallocates a logarithmic number of times)
        size_t want = need;
        if (C.ws_bytes > 0 && want < C.ws_bytes + C.ws_bytes / 2) want = C.ws_bytes + C.ws_bytes / 2;
        void* fresh = nullptr;
        if (hipMalloc(&fresh, want) != hipSuccess) {
            (void)hipGetLastError();
            want = need;
            RSIK_HIP(ctx, hipMalloc(&fresh, want));
        }
        if (C.ws) {
            if (C.ws_captured) {
                // a hipGraph recorded from this context still points into the old workspace: kept until rsik_destroy or
                // rsik_control_continuous_release
                C.retired_ws.push_back(C.ws);
            } else {
                // nothing but runs already issued can use it: freed once they are known to have finished (rsik_sync, _release,
                // rsik_destroy) — not here: a device-wide wait and a free inside an asynchronous call would stall every stream of
                // the process and invalidate a capture some other thread has open
                C.outgrown_ws.push_back(C.ws);
            }
        }
        C.ws = fresh;
        C.ws_bytes = want;
        C.ws_captured = false;
    }
    if (streams) {
        for (auto& st : C.side) RSIK_HIP(ctx, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        C.have_side = true;
    }
    while (C.events.size() < n_events) {
        hipEvent_t e;
        // (hipEventReleaseToDevice / hipEventDisableSystemFence measured: 0.443 / 0.428 against 0.429-0.439 ms per pass — the
        // ~12 us between dependent launches on different streams are not the cache write-back of the event's release)
        RSIK_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        C.events.push_back(e);
    }
    return RSIK_OK;
}

#ifdef RSIK_PIPE_TIMING
// diagnostic builds: the phase kernels' first-start / last-end stamps of the PREVIOUS run are printed (RSIK_PIPE_TIMING_PRINT).  Two
// stamp areas take turns, and a run clears the area of the run AFTER it: with RSIK_OPT_CONT_GOALS_RESIDENT a run's prepare kernels
// can execute before the caller's stream has reached that run's start.
static unsigned long long* pipe_timing_begin(rsik_ctx* ctx, int64_t n_blocks) {
    static unsigned long long* pipe_t = nullptr;  // [2 areas][2][5 * 64]: min stamps, then max stamps
    static int64_t pipe_prev_blocks = 0, pipe_run = 0;
    auto clear = [&](unsigned long long* area, hipStream_t st) {
        (void)hipMemsetAsync(area, 0xff, 320 * sizeof(unsigned long long), st);
        (void)hipMemsetAsync(area + 320, 0, 320 * sizeof(unsigned long long), st);
    };
    if (!pipe_t) {
        if (hipMalloc(&pipe_t, 2 * 640 * sizeof(unsigned long long)) != hipSuccess) pipe_t = nullptr;
        if (pipe_t) { clear(pipe_t, ctx->stream); clear(pipe_t + 640, ctx->stream); (void)hipStreamSynchronize(ctx->stream); }
    }
    if (!pipe_t) return nullptr;
    unsigned long long* const mine = pipe_t + 640 * (pipe_run & 1), * const other = pipe_t + 640 * ((pipe_run + 1) & 1);
    if (getenv("RSIK_PIPE_TIMING_PRINT") && pipe_prev_blocks > 0) {  // (that run has been synchronised by now)
        unsigned long long h[640];
        (void)hipDeviceSynchronize();
        (void)hipMemcpy(h, other, sizeof h, hipMemcpyDeviceToHost);
        unsigned long long base = ~0ull;
        for (int k = 0; k < 320; k++) if (h[k] < base) base = h[k];
        static const char* names[5] = {"prepare", "theta", "joints", "chain", "turns"};
        for (int64_t b = 0; b < pipe_prev_blocks && b < 64; b++)
            for (int ph = 0; ph < 5; ph++)
                if (h[b * 5 + ph] != ~0ull)
                    fprintf(stderr, "[pipe] %-8s(%lld) %8.2f -> %8.2f us\n", names[ph], (long long)b, (h[b * 5 + ph] - base) / 100.0, (h[320 + b * 5 + ph] - base) / 100.0);
    }
    clear(other, ctx->stream);  // (for the run after this one)
    pipe_prev_blocks = n_blocks;
    pipe_run += 1;
    return mine;
}
#endif

// What an eager run and what a captured run of this size need (their block sizes differ): the larger of each.  A run asks for it
// too: the context holds what BOTH forms of a run of this size need, so that a run that was first issued eagerly can be
// captured afterwards (and the other way round) without creating anything
static int cont_reserve(rsik_ctx* ctx, const char* who, int64_t n, int64_t n_steps) {
    ContPlan P, Pc;
    int rc = cont_plan(ctx, who, n, n_steps, false, P, ctx->options[RSIK_OPT_CONT_GOALS_RESIDENT] != 0);
    if (rc != RSIK_OK) return rc;
    if ((rc = cont_plan(ctx, who, n, n_steps, true, Pc)) != RSIK_OK) return rc;
    if (Pc.need > P.need) P.need = Pc.need;
    if (Pc.n_events > P.n_events) P.n_events = Pc.n_events;
    return cont_resources(ctx, who, P.need, true, P.n_events);
}

int rsik_control_continuous_reserve(rsik_ctx* ctx, int64_t n, int64_t n_steps) {
    const char* who = "rsik_control_continuous_reserve";
    if (!ctx) return RSIK_E_INVALID;
    if (n < 0 || n_steps < 0) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": negative size");
    if (n == 0 || n_steps == 0) return RSIK_OK;
    RSIK_HIP(ctx, hipSetDevice(ctx->device));
    return cont_reserve(ctx, who, n, n_steps);
}

int rsik_control_continuous_release(rsik_ctx* ctx) {
    if (!ctx) return RSIK_E_INVALID;
    RSIK_HIP(ctx, hipSetDevice(ctx->device));
    RSIK_HIP(ctx, hipDeviceSynchronize());
    ctx->cont.release();
    return RSIK_OK;
}

// Two runs of one context share its workspace, words and side streams: a run issued on another stream than the one before it
// waits for that one's end (runs on one stream are ordered by the stream; hipGraphs recorded from one context must not be
// replayed concurrently: include/rsik.h).
static int cont_run_begin(rsik_ctx* ctx, bool capturing) {
    rsik_ctx::Cont& C = ctx->cont;
    // Workspaces and word arrays that earlier runs outgrew: a caller that synchronises through its own framework never calls
    // rsik_sync, so they are also let go here, without waiting — when the last run issued is known to have finished (every run
    // before it has, then: runs of one context are ordered).  Never inside a capture.
    if (!capturing && !C.outgrown_ws.empty() && C.have_run_done && hipEventQuery(C.run_done) == hipSuccess) free_all(C.outgrown_ws);
    (void)hipGetLastError();  // (hipErrorNotReady is not an error)
    if (capturing || !C.have_run_done || C.run_stream == ctx->stream) return RSIK_OK;
    RSIK_HIP(ctx, hipStreamWaitEvent(ctx->stream, C.run_done, 0));
    return RSIK_OK;
}
// `where`: the stream whose last operation marks the run's end — the chain stream behind the last chain kernel (every phase of every
// block is ahead of it), so that the record is not one more operation between this run's end and the next run's first kernel on the
// caller's stream (round 6: that stretch is on the critical path of runs that overlap); the caller's stream where a run failed part-way.
static int cont_run_end(rsik_ctx* ctx, bool capturing, hipStream_t where) {
    rsik_ctx::Cont& C = ctx->cont;
    if (capturing) return RSIK_OK;
    if (!C.have_run_done) {
        RSIK_HIP(ctx, hipEventCreateWithFlags(&C.run_done, hipEventDisableTiming));
        C.have_run_done = true;
    }
    RSIK_HIP(ctx, hipEventRecord(C.run_done, where));
    C.run_stream = ctx->stream;
    return RSIK_OK;
}

// One call of rsik_control_continuous_run: what it was asked, what it decided, and one member function per step, in the order
// rsik_control_continuous_run takes them.
struct ContRun {
    rsik_ctx* const ctx;
    rsik_ctx::Cont& C;  // ctx->cont
    const char* const who;
    const int64_t n, n_steps;
    const double* const m12_steps;
    rsik::ContinuousArgs K0;  // the step kernel's arguments for step 0 (fill_continuous), the start-up kernel's
    dim3 grid, block{rsik::kBlock};  // a thread per trajectory
    ContPlan P;
    int64_t n_blocks = 0, head = 0;
    rsik::ContRunArgs R;
    hipStream_t s_main = nullptr, s_theta = nullptr, s_prep = nullptr, s_joints = nullptr, s_chain = nullptr;
    bool capturing = false, resident = false, by_value = false, overlap = false, theta_waits = false, alias_same = false, alias_any = false;
    int variant = 0, slot_base = 0;
    unsigned seq = 0, last_seq = 0;
    int64_t last_blocks = 0;
    const uint8_t *st_lo = nullptr, *st_hi = nullptr, *rc_lo = nullptr, *rc_hi = nullptr;  // the reachable / state rows this run writes
    bool plane_binds = false;
    int snap_kind = rsik::kSnapGeneric;
    dim3 grid8;
#ifdef RSIK_PIPE_TIMING
    unsigned long long* pipe_t = nullptr;
#endif
    ContRun(rsik_ctx* c, const char* w, int64_t n_, int64_t n_steps_, const double* m12) : ctx(c), C(c->cont), who(w), n(n_), n_steps(n_steps_), m12_steps(m12) {}

    // RSIK_CONT_RUN_STEPS: one launch of the step kernel per control step
    int issue_steps() {
        // (what the run was issued as is the caller's to know: rsik_control_continuous_last_form — a solver whose projection margin
        // lets is_reachable_no_limits fail gets n_steps launches whatever RSIK_OPT_CONT_RUN_MODE says)
        C.last_run_form = ctx->options[RSIK_OPT_CONT_RUN_MODE] == RSIK_CONT_RUN_STEPS ? RSIK_CONT_FORM_STEPS : RSIK_CONT_FORM_STEPS_NO_LIMITS_CAN_FAIL;
        C.last_run.valid = false;  // (this run's outputs are written on the caller's stream: the next phased run forks behind them)
        for (int64_t k = 0; k < n_steps; k++) {
            rsik::ContinuousArgs K = K0;
            for (int c = 0; c < 12; c++) K.in[c] = m12_steps + ((size_t)k * 12 + c) * (size_t)n;
            if (k > 0) {
                K.first_timed_out = 0;
                K.current_joints = nullptr;
                for (int c = 0; c < 12; c++) K.cur_pose[c] = nullptr;
            }
            K.joints = K0.joints + (size_t)k * n * 7;
            K.reachable = K0.reachable ? K0.reachable + (size_t)k * n : nullptr;
            K.state = K0.state ? K0.state + (size_t)k * n : nullptr;
            launch_continuous_step(ctx, K0.arm, K, grid, block);
        }
        return launch_end(ctx);
    }

    // ---- phased pipeline.  The four phases of a block run on four streams (theta on the caller's, the others on the
    // context's own), ordered by events: prepare(b) -> theta(b) -> joints(b) -> chain(b), theta(b) after theta(b-1),
    // chain(b) after chain(b-1).  The two sequential phases (a lone wave per SIMD on a few CUs) then run beside each other
    // and beside the chip-filling ones of the neighbouring blocks.  Exactly four streams: the runtime multiplexes streams
    // onto four hardware queues, and a fifth stream shares a queue with another one — measured with theta on a stream of
    // its own: theta(b + 1) queued up behind chain(b)'s wait for joints(b), 0.85 -> 1.28 ms per 1000-step pass.  (Giving
    // the sequential phases compute units of their own with hipExtStreamCreateWithCUMask was measured too: every kernel
    // got slower, 2.4 ms per pass.)
    // A run is cut into blocks of steps; up to eight workspace slots are in flight (block b + 8 reuses the slot of block b
    // once its last phase has finished).
    int plan_and_resources() {
        // RSIK_OPT_CONT_GOALS_RESIDENT (rsik.h): the prepare phase of this run need not wait for the previous run's end
        resident = !capturing && ctx->options[RSIK_OPT_CONT_GOALS_RESIDENT] != 0;
        int rc = cont_plan(ctx, who, n, n_steps, capturing, P, resident);
        if (rc != RSIK_OK) return rc;
        if ((rc = cont_reserve(ctx, who, n, n_steps)) != RSIK_OK) return rc;
        if (capturing) C.ws_captured = true;
        n_blocks = (int64_t)P.block_t0.size();
        head = n_blocks < P.slots ? n_blocks : P.slots;  // blocks with a workspace slot of their own: issued phase by phase
#ifdef RSIK_PIPE_TIMING
        pipe_t = pipe_timing_begin(ctx, n_blocks);
#endif
        s_main = s_theta = ctx->stream; s_prep = C.side[0]; s_joints = C.side[1]; s_chain = C.side[2];
        return RSIK_OK;
    }

    // Dependencies between the streams.  Recorded into a hipGraph they are events (the only form a capture takes).  Issued
    // launch by launch they are words in device memory: the producer's stream writes this run's sequence number behind its
    // kernel (hipStreamWriteValue32), the consumer's stream waits for the word to reach it (hipStreamWaitValue32) — measured
    // on an otherwise idle chip (scripts/probes/edge_probe.hip): the dependent kernel starts 3.8 us after its parent's end,
    // against 10.6 us behind an event (15-55 us inside a pass).  Words are per (kind, block) and only ever grow.
    // (`run_seq`: this run's number, or — waits only — the previous run's; the event form has no use for it)
    hipError_t signal(hipStream_t st, size_t id, unsigned run_seq) const {
        if (by_value) return hipStreamWriteValue32(st, C.edge_words + id, run_seq, 0);
        return hipEventRecord(C.events[id], st);
    }
    hipError_t wait_for(hipStream_t st, size_t id, unsigned run_seq) const {
        if (by_value) return hipStreamWaitValue32(st, C.edge_words + id, run_seq, hipStreamWaitValueGte, 0xffffffffu);
        return hipStreamWaitEvent(st, C.events[id], 0);
    }
    // the words of a run issued launch by launch: enough of them, and this run's number
    int prepare_edge_words() {
        variant = ctx->options[RSIK_OPT_CONT_PHASED_VARIANT];
        by_value = !capturing && ctx->can_wait_value != 0 && !(variant & RSIK_PHASED_EDGES_BY_EVENT);
        if (by_value) {
            const size_t need_words = P.n_events;
            if (C.edge_count < need_words) {
                C.last_run.valid = false;  // (its words are not these: this run forks behind it)
                // (the old words: runs already issued still wait on them and write them — freed like an outgrown workspace)
                if (C.edge_words) { C.outgrown_ws.push_back(C.edge_words); C.edge_words = nullptr; C.edge_count = 0; }
                RSIK_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&C.edge_words), need_words * 2 * sizeof(unsigned)));
                RSIK_HIP(ctx, hipMemset(C.edge_words, 0, need_words * 2 * sizeof(unsigned)));
                C.edge_count = need_words * 2;
                C.edge_seq = 0;
            }
            if (C.edge_seq >= RSIK_EDGE_SEQ_WRAP) {
                // A word only ever grows and every wait is "word >= a run's number": before the 32-bit number wraps (4e9 runs: weeks of a
                // control loop that issues a run per tick) everything issued drains, the words start over from zero and this run forks
                // behind the caller's stream like a first one.
                RSIK_HIP(ctx, hipStreamSynchronize(ctx->stream));
                for (auto& st : C.side) RSIK_HIP(ctx, hipStreamSynchronize(st));
                // (kWordGaveUp is not a sequence number: a theta kernel's "gave up waiting" mark, rsik_sync's to read and clear)
                RSIK_HIP(ctx, hipMemset(C.edge_words, 0, kWordGaveUp * sizeof(unsigned)));
                RSIK_HIP(ctx, hipMemset(C.edge_words + kRunWords, 0, (C.edge_count - kRunWords) * sizeof(unsigned)));
                C.edge_seq = 0;
                C.last_run.valid = false;
            }
            C.edge_seq += 1;
        }
        // (a word's meaning does not depend on the run's number of blocks: a word is only ever written from one stream, in issue order,
        // so its value never goes back — runs that overlap, below, rely on it)
        seq = C.edge_seq;
        return RSIK_OK;
    }
    // Does this run's prepare phase start without waiting for the previous run's end?  Only behind a run of the same shape issued the
    // same way on the same stream into the same workspace and words (anything else: the streams meet first, as always).
    void decide_overlap() {
        const rsik_ctx::Cont::LastRun& L = C.last_run;
        overlap = resident && by_value && L.valid && L.stream == ctx->stream && L.ws == C.ws && L.words == C.edge_words &&
                  L.slot_bytes == P.slot_bytes && L.slots == P.slots && !C.ws_captured;
        st_lo = K0.state; st_hi = K0.state ? K0.state + (size_t)n_steps * (size_t)n : nullptr;
        rc_lo = K0.reachable; rc_hi = K0.reachable ? K0.reachable + (size_t)n_steps * (size_t)n : nullptr;
        if (overlap) {
            auto meet = [](const uint8_t* a0, const uint8_t* a1, const uint8_t* b0, const uint8_t* b1) { return a0 && b0 && a0 < b1 && b0 < a1; };
            alias_any = meet(st_lo, st_hi, L.state_lo, L.state_hi) || meet(st_lo, st_hi, L.reach_lo, L.reach_hi) ||
                        meet(rc_lo, rc_hi, L.state_lo, L.state_hi) || meet(rc_lo, rc_hi, L.reach_lo, L.reach_hi);
            alias_same = alias_any && st_lo == L.state_lo && rc_lo == L.reach_lo && n == L.n && n_steps == L.n_steps && P.T == L.T;
        } else {
            C.reset_slots();  // the streams meet at this run's start: every slot is free
        }
        slot_base = overlap ? C.slot_next : 0;
        // A run that overlaps the one before it: its theta kernels wait for their prepare kernels themselves (cont_theta_kernel), and the
        // joints kernel of a block takes "theta of the NEXT block has started" for "theta of this block is done" (same stream: it is) —
        // so that nothing stands between two theta kernels on the caller's stream.  Only there: K overlapping 1000-step passes 0.334-0.342
        // against 0.341-0.346 ms with stream waits, same box; a run on its own is level (0.357-0.371 / 0.363-0.378), a long one — 8 000 /
        // 16 000 steps in blocks of 512 — slower, 0.348 / 0.425 against 0.340 / 0.377 ms per 1000 steps (profiles/r06/config5_long_runs.txt).
        // (kVariantThetaStreamWaits, timing experiments and the A/B tests: stream waits and writes there too)
        theta_waits = by_value && overlap && !(variant & kVariantThetaStreamWaits);
        last_seq = L.seq;
        last_blocks = L.n_blocks;
    }
    // what every kernel of the run is given (set_block: what differs from block to block)
    void fill_args() {
        std::memset(&R, 0, sizeof R);
        R.n = n;
        R.m12_steps = m12_steps;
        R.arm = K0.arm;
        R.euler_roundtrip = K0.euler_roundtrip;
        for (int slot = 0; slot < 2; slot++) {
            R.pref_arg[slot] = K0.pref_arg[slot]; R.pref_self[slot] = K0.pref_self[slot];
            R.pref_self_cs[slot] = K0.pref_self_cs[slot]; R.pref_self_sn[slot] = K0.pref_self_sn[slot];
            R.lim[slot][0] = K0.lim[slot][0]; R.lim[slot][1] = K0.lim[slot][1];
            R.arms[slot] = K0.arms[slot];
        }
        R.d_theta_max = K0.d_theta_max;
        R.max_angle = K0.max_angle; R.cos_max = K0.cos_max; R.sin_max = K0.sin_max;
        R.st = K0.st; R.joints = K0.joints; R.reachable = K0.reachable; R.state = K0.state;
        R.theta_carry = reinterpret_cast<double*>(static_cast<char*>(C.ws) + P.theta_carry_off);
        R.no_turn_hint = (variant & kVariantNoTurnHint) ? 1 : 0;
        R.run_turn_hint = reinterpret_cast<unsigned*>(static_cast<char*>(C.ws) + P.run_hint_off);
        grid8 = dim3((unsigned)((n * 8 + rsik::kChainBlock - 1) / rsik::kChainBlock));  // (n <= 30 Mi: fits)
        plane_binds = singularity_plane_binds(R.arms);
        // the theta phase's step, specialised for the control interval where that is proven equivalent (single-arm launches)
        if (!K0.arm) snap_kind = theta_snap_plan(R.lim[0][0], R.lim[0][1], R.d_theta_max, &R.snap_tdag);
#ifdef RSIK_PIPE_TIMING
        R.tmin = pipe_t; R.tmax = pipe_t ? pipe_t + 320 : nullptr;
#endif
    }
    void set_block(int64_t b) {
#ifdef RSIK_PIPE_TIMING
        R.tslot = (int)(b < 64 ? b : 63);
#endif
        R.t0 = P.block_t0[b];
        R.T = P.block_T[b];
        R.first_block = b == 0;
        R.last_block = b == n_blocks - 1;
        R.ws = reinterpret_cast<double*>(static_cast<char*>(C.ws) + P.slot_bytes * (size_t)((slot_base + b) % P.slots));
        R.gw = R.ws + (size_t)R.T * (size_t)n;
        R.flags = reinterpret_cast<uint8_t*>(R.gw + (size_t)R.T * (size_t)n);
        R.chunk_event = R.flags + (size_t)R.T * (size_t)n;
        // (the slot's turn hints sit at its end, whatever the block's length; a block that is the first to use its slot in this run
        // reads the run's own)
        R.slot_turn_hint = reinterpret_cast<uint8_t*>(R.ws) + P.slot_hint_off;
        R.turn_hint = b < P.slots ? R.run_turn_hint : reinterpret_cast<unsigned*>(R.slot_turn_hint);
    }

    // What a pass really looks like was measured with in-kernel stamps (a -DRSIK_PIPE_TIMING build,
    // scripts/probes/c5_untraced_timeline.py; the profiler's kernel trace delays launches and shows another schedule): a
    // dependency between launches on DIFFERENT streams costs the dependent kernel 15-40 us after its last parent has
    // finished, launch by launch and in a graph replay alike (theta(b) -> joints(b): 31-41 us in a replay), a kernel
    // behind its predecessor on the SAME stream 4-7 us.  Keeping the whole critical chain on one in-order stream (init,
    // theta(b), joints(b) alternately, prepares beside it) removes those hand-overs but also the overlap of theta(b + 1)
    // with joints(b): 0.42 ms launch by launch (the best eager figure) but 0.40-0.43 replayed, against 0.39 for the
    // overlapped form below, which stays.  A block that reuses a workspace slot can only be issued once the block that
    // frees it has been (its event must have been recorded).
    int issue_prepare(int64_t b) {
        set_block(b);
        const dim3 grid2(grid.x, (unsigned)R.T);
        // the slot's previous block is done (launch by launch: whichever run it belonged to)
        if (by_value) {
            rsik_ctx::Cont::SlotUse& u = C.slot_use[(slot_base + b) % P.slots];
            if (u.seq != 0) RSIK_HIP(ctx, wait_for(s_prep, u.word, u.seq));
            u = {edge_id(kEdgeChain, b), seq};
            // a run that overlaps the one before it and writes the same reachable / state rows: behind that run's chain kernel of
            // the same rows (the same cut), or of its last block
            // (and not before that run's last joints kernel has finished: started earlier, this run's prepare kernels share the chip
            // with that run's joints kernels, which its end — and with it this run's start-up — waits for: K passes took 0.39-0.41 ms
            // each instead of 0.36-0.39; behind it they fill the chip while that run's last chain kernel and this run's start-up
            // search, lone waves both, have it to themselves)
            // (kVariantPrepareNotHeld / kVariantPrepareBehindChainEnd, timing experiments: no such wait / the last chain kernel's END)
            const bool held = overlap && !(variant & kVariantPrepareNotHeld);
            if (held && b == 0) RSIK_HIP(ctx, wait_for(s_prep, edge_id((variant & kVariantPrepareBehindChainEnd) ? kEdgeChain : kEdgeChainStarted, last_blocks - 1), last_seq));
            // ... and the later ones leave the chip to the lone waves ahead of them on the critical path — the start-up search, then
            // theta(0), theta(1) ...: prepare(1) is held until the start-up kernel has started, prepare(b) until theta(b - 2) has (each
            // issued before this wait, issue_all's order for a run that overlaps)
            if (held && b == 1) RSIK_HIP(ctx, wait_for(s_prep, kWordInitStarted, seq));
            if (held && b >= 2) RSIK_HIP(ctx, wait_for(s_prep, edge_id(kEdgeThetaStarted, b - 2), seq));
            if (alias_same) RSIK_HIP(ctx, wait_for(s_prep, edge_id(kEdgeChain, b), last_seq));
            else if (alias_any && b == 0) RSIK_HIP(ctx, wait_for(s_prep, edge_id(kEdgeChain, last_blocks - 1), last_seq));
        } else if (b >= P.slots) {
            RSIK_HIP(ctx, wait_for(s_prep, edge_id(kEdgeChain, b - P.slots), seq));
        }
        with_bool(K0.arm != nullptr, [&](auto MIXED) { with_bool(plane_binds, [&](auto PLANE) {
            hipLaunchKernelGGL((rsik::cont_prepare_kernel<MIXED(), PLANE()>), grid2, block, 0, s_prep, R); }); });
        RSIK_HIP(ctx, signal(s_prep, edge_id(kEdgePrepared, b), seq));
        return RSIK_OK;
    }
    int issue_theta(int64_t b) {
        set_block(b);
        // (launch by launch: the kernel says when it has started — the joints kernel of the block before is held until then)
        R.started_word = by_value ? C.edge_words + edge_id(kEdgeThetaStarted, b) : nullptr;
        R.started_seq = seq;
        if (theta_waits) {
            R.wait_word = C.edge_words + edge_id(kEdgePrepared, b);
            R.wait_seq = seq;
            R.timeout_word = C.edge_words + kWordGaveUp;
        } else {
            R.wait_word = nullptr;
            RSIK_HIP(ctx, wait_for(s_theta, edge_id(kEdgePrepared, b), seq));
        }
        const dim3 grid_t((unsigned)((n + rsik::kThetaBlock - 1) / rsik::kThetaBlock)), block_t(rsik::kThetaBlock);
        // (the specialised steps are single-arm only: theta_snap_plan is not asked for a mixed launch)
        if (K0.arm) hipLaunchKernelGGL((rsik::cont_theta_kernel<true, rsik::kSnapGeneric>), grid_t, block_t, 0, s_theta, R);
        else with_int3(snap_kind, [&](auto SNAP) { hipLaunchKernelGGL((rsik::cont_theta_kernel<false, SNAP()>), grid_t, block_t, 0, s_theta, R); });
        if (!theta_waits || b == n_blocks - 1) RSIK_HIP(ctx, signal(s_theta, edge_id(kEdgeTheta, b), seq));
        return RSIK_OK;
    }
    int issue_back(int64_t b) {  // joints(b), chain(b)
        set_block(b);
        // (a wave = 8 trajectories x 8 steps: n / 8 groups, 4 per workgroup)
        const dim3 grid2((unsigned)((n + 8 * (rsik::kBlock / 64) - 1) / (8 * (rsik::kBlock / 64))), (unsigned)((R.T + rsik::kJointChunk - 1) / rsik::kJointChunk));
        // joints(b) needs theta(b).  Launch by launch it is held a little longer: until theta(b + 1) has STARTED (which is after
        // theta(b)'s end: same stream).  The theta kernel's lone waves want 276 registers each — a SIMD that holds six waves of a
        // chip-filling kernel has none to give — so a theta kernel that becomes ready together with a joints kernel and loses the
        // race for the chip only gets in when that kernel drains: theta(b + 1) ran behind joints(b), not beside it (measured with
        // in-kernel stamps: a third of a pass).  Let in first, it has its SIMDs before the chip fills up.
        // (measured and not kept — with the theta phase as one persistent launch, docs/experiments.md A.4: the first joints kernel held until the last prepare kernel has
        // completed, so that the prepare kernels — which every later phase of a block waits for — have the chip to themselves:
        // 0.424 against 0.371 ms per pass, the joints kernels then run one behind the other with a stream operation's ~15 us
        // between them; higher stream priority for the prepare and chain streams: no difference)
        // (theta(b + 1) has been ISSUED before this wait — issue_all's order: streams can share a hardware queue, and a wait that
        // sat in one ahead of the launch it waits for would wait for ever)
        if (!theta_waits || b == n_blocks - 1) RSIK_HIP(ctx, wait_for(s_joints, edge_id(kEdgeTheta, b), seq));
        else RSIK_HIP(ctx, wait_for(s_joints, edge_id(kEdgeThetaStarted, b + 1), seq));
        if (by_value && !theta_waits && !(variant & RSIK_PHASED_NO_THETA_FIRST) && b + 1 < n_blocks)
            RSIK_HIP(ctx, wait_for(s_joints, edge_id(kEdgeThetaStarted, b + 1), seq));
        with_bool(K0.arm != nullptr, [&](auto MIXED) { hipLaunchKernelGGL(rsik::cont_joints_kernel<MIXED()>, grid2, block, 0, s_joints, R); });
        RSIK_HIP(ctx, signal(s_joints, edge_id(kEdgeJoints, b), seq));
        RSIK_HIP(ctx, wait_for(s_chain, edge_id(kEdgeJoints, b), seq));
        R.chain_started_word = by_value ? C.edge_words + edge_id(kEdgeChainStarted, b) : nullptr;
        R.started_seq = seq;
        with_bool(K0.arm != nullptr, [&](auto MIXED) { hipLaunchKernelGGL(rsik::cont_chain_kernel<MIXED()>, grid8, dim3(rsik::kChainBlock), 0, s_chain, R); });
        RSIK_HIP(ctx, signal(s_chain, edge_id(kEdgeChain, b), seq));
        return RSIK_OK;
    }
    // (Re)initialisation of the trajectories that start here (C:296-325: the start-up search for previous_theta, ~55 us
    // of lone waves), then the pipeline's streams join in.  The prepare phase depends on the goal matrices alone, not on
    // the trajectory state: its stream forks off BEFORE the initialisation (behind whatever the caller queued ahead of
    // this call), so prepare(0) runs beside it and theta(0) starts when both are done; the joints and chain streams fork
    // behind it.
    // RSIK_OPT_CONT_GOALS_RESIDENT, behind a run of the same shape: the prepare stream does not fork at all — it carries on behind
    // the previous run's prepare kernels, so this run's run beside that run's joints and chain kernels (its slots and output rows
    // are waited for one by one, issue_prepare); the start-up kernel and everything behind it wait for the previous run's end
    // as they must (the trajectory state).
    int issue_start() {
        if (!overlap) {
            RSIK_HIP(ctx, signal(s_main, kWordPrepareMayFork, seq));
            RSIK_HIP(ctx, wait_for(s_prep, kWordPrepareMayFork, seq));
        }
        // two lanes per trajectory where get_joints cannot move the solver's state (no elbow projection possible)
        const bool pair = !singularity_plane_binds(K0.arms);
        dim3 grid_init = grid;
        int rc = RSIK_OK;
        if (pair && (rc = launch_dims(ctx, n * 2, &grid_init, who)) != RSIK_OK) return rc;
        K0.started_word = by_value ? C.edge_words + kWordInitStarted : nullptr;
        K0.started_seq = seq;
        with_bool(K0.arm != nullptr, [&](auto MIXED) { with_bool(pair, [&](auto PAIR) {
            hipLaunchKernelGGL((rsik::cont_init_kernel<MIXED(), PAIR()>), grid_init, block, 0, s_main, K0); }); });
        // (the joints and chain streams' first kernels wait for theta(0), which is behind this kernel on its stream)
        if (!theta_waits) {
            RSIK_HIP(ctx, signal(s_main, kWordInitDone, seq));
            RSIK_HIP(ctx, wait_for(s_joints, kWordInitDone, seq));
            RSIK_HIP(ctx, wait_for(s_chain, kWordInitDone, seq));
        }
        return RSIK_OK;
    }
    // Issue order of the blocks that have a workspace slot of their own (it is also the order of the nodes in a captured
    // graph): prepare(0), theta(0), then the other prepares back to back, the other thetas, then joints + chain of
    // every block.  Measured on graph replays of 4096 x 1000 steps against three other orders (prepare / theta
    // alternating: 0.394-0.411 ms; all prepares, all thetas: 0.398-0.401; thetas and backs alternating: 0.414-0.416):
    // 0.387-0.392 ms.
    int issue_all() {
        int rc = issue_start();
        if (rc != RSIK_OK) return rc;
        if ((rc = issue_prepare(0)) != RSIK_OK) return rc;
        if ((rc = issue_theta(0)) != RSIK_OK) return rc;
        if (overlap) {
            // (a run that overlaps the one before it holds prepare(b) until theta(b - 2) has started: that one is issued first)
            for (int64_t b = 1; b < head; b++) {
                if ((rc = issue_prepare(b)) != RSIK_OK) return rc;
                if ((rc = issue_theta(b)) != RSIK_OK) return rc;
            }
        } else {
            for (int64_t b = 1; b < head; b++)
                if ((rc = issue_prepare(b)) != RSIK_OK) return rc;
            for (int64_t b = 1; b < head; b++)
                if ((rc = issue_theta(b)) != RSIK_OK) return rc;
        }
        // joints + chain of every block; a block beyond the head (it reuses a workspace slot: its prepare kernel waits for the
        // chain kernel of the block `slots` before it, issued by then) has its prepare and theta kernels issued just ahead of
        // the joints kernel of the block BEFORE it, so that that one can be held until the theta kernel has started, like the
        // head's (round 6: a 16 384-step run in blocks of 512 had its theta kernels start 60-100 us late, behind whichever
        // chip-filling kernel was draining, profiles/r06/config5_long_runs.txt)
        for (int64_t b = 0; b < n_blocks; b++) {
            if (b + 1 >= head && b + 1 < n_blocks) {
                if ((rc = issue_prepare(b + 1)) != RSIK_OK) return rc;
                if ((rc = issue_theta(b + 1)) != RSIK_OK) return rc;
            }
            if ((rc = issue_back(b)) != RSIK_OK) return rc;
        }
        // the caller's stream continues once the last chain (hence every phase of every block) is done
        RSIK_HIP(ctx, wait_for(s_main, edge_id(kEdgeChain, n_blocks - 1), seq));
        return launch_end(ctx);
    }
    // A failure part-way leaves value waits queued on the context's streams whose words nobody is going to write (an event
    // that was never recorded is no wait at all; a word is one).  Every word of the context is raised to this run's number
    // from a stream of its own, so that the streams drain and no later call (rsik_sync, _release, rsik_destroy) hangs on
    // them; the run's outputs are unspecified, the error is the caller's to see.
    void drain_after_failure() {
        const std::string first_error = ctx->err;
        if (by_value) {
            hipStream_t fresh = nullptr;
            if (hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking) == hipSuccess) {
                (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(C.edge_words), (int)seq, C.edge_count, fresh);
                (void)hipStreamSynchronize(fresh);
                (void)hipStreamDestroy(fresh);
            }
            (void)hipGetLastError();
        }
        C.last_run.valid = false;
        C.reset_slots();
        // (what was issued before the failure is still running: rsik_sync and the next run's housekeeping wait for THIS point)
        if (!capturing) {
            (void)cont_run_end(ctx, false, ctx->stream);
            (void)hipGetLastError();
        }
        ctx->err = first_error;
    }
    // what the next run needs to know of this one to overlap it (decide_overlap, issue_prepare)
    void remember() {
        if (capturing) {
            C.last_run_form = RSIK_CONT_FORM_PHASED_CAPTURED;
            return;
        }
        rsik_ctx::Cont::LastRun& L = C.last_run;
        C.last_run_form = overlap ? RSIK_CONT_FORM_PHASED_OVERLAPPED : RSIK_CONT_FORM_PHASED;
        L.valid = by_value;
        L.seq = seq; L.stream = ctx->stream; L.ws = C.ws; L.words = C.edge_words;
        L.n = n; L.n_steps = n_steps; L.T = P.T; L.n_blocks = n_blocks; L.slot_bytes = P.slot_bytes; L.slots = P.slots;
        L.state_lo = st_lo; L.state_hi = st_hi; L.reach_lo = rc_lo; L.reach_hi = rc_hi;
        C.slot_next = (int)((slot_base + n_blocks) % P.slots);
    }
};

// The whole trajectory batch: the phased pipeline (include/rsik.h), or — RSIK_CONT_RUN_STEPS — one launch of the step
// kernel per control step.
int rsik_control_continuous_run(rsik_ctx* ctx, int64_t n, int64_t n_steps, const double* m12_steps,
                                const double* const current_pose_m12_soa[12], const uint8_t* arm, int arm_uniform,
                                int first_step_timed_out, double preferred_theta, const double* preferred_theta_self_host,
                                int constrained_mode, double d_theta_max, const double* current_joints,
                                double orbita3d_max_angle, double* cont_state, double* joints_steps,
                                uint8_t* reachable_steps, uint8_t* state_steps) {
    const char* who = "rsik_control_continuous_run";
    if (!ctx) return RSIK_E_INVALID;
    if (n < 0 || n_steps < 0) return fail(ctx, RSIK_E_INVALID, "rsik_control_continuous_run: negative size");
    if (n == 0 || n_steps == 0) return check_arms(ctx, arm, arm_uniform, who);
    if (!m12_steps || !joints_steps) return fail(ctx, RSIK_E_INVALID, "rsik_control_continuous_run: NULL buffer");
    ContRun run(ctx, who, n, n_steps, m12_steps);
    const double* cols[12];
    for (int c = 0; c < 12; c++) cols[c] = m12_steps + (size_t)c * (size_t)n;  // step 0; step s is 12 n doubles further
    int rc = fill_continuous(ctx, who, run.K0, n, cols, current_pose_m12_soa, arm, arm_uniform, nullptr, first_step_timed_out ? 1 : 0,
                             preferred_theta, preferred_theta_self_host, constrained_mode, d_theta_max, current_joints,
                             orbita3d_max_angle, cont_state, joints_steps, reachable_steps, state_steps);
    if (rc != RSIK_OK) return rc;
    if ((rc = launch_begin(ctx, n, &run.grid, who)) != RSIK_OK) return rc;
    // is_reachable_no_limits can only fail (C:385-387) for a projection margin that lets the pulled-back wrist land beyond
    // u + f (S:343-345); the pipeline's phases do not carry that outcome, the step kernel does.
    bool no_limits_can_fail = false;
    for (int slot = 0; slot < 2; slot++) no_limits_can_fail = no_limits_can_fail || !(run.K0.arms[slot].v[RSIK_C_PROJ_MARGIN] > 1e-12);
    if (ctx->options[RSIK_OPT_CONT_RUN_MODE] == RSIK_CONT_RUN_STEPS || no_limits_can_fail) return run.issue_steps();
    run.capturing = stream_is_capturing(ctx->stream);
    if ((rc = cont_run_begin(ctx, run.capturing)) != RSIK_OK) return rc;
    if ((rc = run.plan_and_resources()) != RSIK_OK) return rc;
    if ((rc = run.prepare_edge_words()) != RSIK_OK) return rc;
    run.decide_overlap();
    run.fill_args();
    if ((rc = run.issue_all()) != RSIK_OK) {
        run.drain_after_failure();
        return rc;
    }
    run.remember();
    return cont_run_end(ctx, run.capturing, run.s_chain);
}

int rsik_control_continuous_last_form(const rsik_ctx* ctx) { return ctx ? ctx->cont.last_run_form : RSIK_CONT_FORM_NONE; }
