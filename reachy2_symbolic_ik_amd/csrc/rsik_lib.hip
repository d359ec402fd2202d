// rsik_lib.hip — the C ABI of include/rsik.h: context, argument checks and launches.  The kernels (gfx950) live in the
// rsik_kernel_*.hpp files next to it, one per entry point or family; what they share in rsik_tables.hpp (workgroup size, constant
// access, table staging), rsik_rows.hpp (streaming accesses, rows through LDS, the wave-level LDS fence) and rsik_goal.hpp (the pose
// kernels' head, the goal-matrix conversion); the per-pose mathematics in rsik_device.hpp / rsik_math.hpp.  Each of these headers
// includes what it uses.  Two files are fragments of this one, host code included inside its extern "C" block: the scheduler of
// rsik_control_continuous_run (rsik_cont_run.hpp) and the RCCL entry points (rsik_comm.hpp).
// Every launching entry point reads: its own checks, in its own order (the return code and the message that wins are part of the
// ABI), fill the kernel's argument block K, launch_begin, one launch line, launch_end.  What they share is below the memcpy entry
// points: check_arms, bind_arms, copy_cols, launch_form / tip_on_z, launch_dims / launch_begin / launch_end; and, for the sampling
// family (rsik_solve_sweep, rsik_solve_nearest, rsik_solve_path, rsik_solve_path_clear), check_samples, check_sample_inputs and fill_samples.
//
// Kernel shape: one pose per lane, 256-thread workgroups (4 wave64), SoA float64 inputs so that
// every global load is a fully coalesced 512-B wave access; the [n,7] / [n,3] row outputs are
// transposed through LDS so that each wave writes its 3584-B / 1536-B slab with unit-stride stores.
// Per-arm constants travel in the kernarg segment (scalar loads, wave-uniform).
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

// the kernels, by entry point (each header includes what it uses: any order)
#include "rsik_kernel_solve.hpp"
#include "rsik_kernel_discrete.hpp"
#include "rsik_kernel_continuous.hpp"
#include "rsik_kernel_pipeline.hpp"
#include "rsik_kernel_state.hpp"
#include "rsik_kernel_stages.hpp"
#include "rsik_kernel_theta_from_joints.hpp"
#include "rsik_kernel_sweep.hpp"
#include "rsik_kernel_nearest.hpp"
#include "rsik_kernel_path.hpp"
#include "rsik_kernel_reach_map.hpp"
#include "rsik_kernel_jacobian.hpp"
#include "rsik_kernel_joint_rates.hpp"
#include "rsik_kernel_track.hpp"
#include "rsik_kernel_clearance.hpp"
#include "rsik_kernel_track_avoid.hpp"
#include "rsik_kernel_track_pair.hpp"
#include "rsik_kernel_path_pair.hpp"
#include "rsik_kernel_clearance_edges.hpp"

// =====================================================================================
// C ABI
// =====================================================================================
struct rsik_ctx {
    int device = 0;
    int compute_units = 256;  // of the device (256 on MI355X): which launches are a single round
    hipStream_t stream = nullptr;
    bool have_arm[2] = {false, false};
    rsik::ArmC arms[2] = {};
    int options[RSIK_OPT_COUNT] = {};
    int can_wait_value = 0;          // hipDeviceAttributeCanUseStreamWaitValue
    // What rsik_control_continuous_run keeps from call to call (rsik_cont_run.hpp, where the member functions are too)
    struct Cont {
        void* ws = nullptr;          // workspace of rsik_control_continuous_run (device: the pipeline's block slots), grown on demand
        size_t ws_bytes = 0;
        bool ws_captured = false;        // a run recorded into a hipGraph points into the current workspace
        std::vector<void*> retired_ws;   // outgrown workspaces a captured hipGraph may still point into: kept until rsik_destroy / _release
        std::vector<void*> outgrown_ws;  // outgrown workspaces only runs already issued can use: freed by the next rsik_sync / _release / rsik_destroy
        hipEvent_t run_done = nullptr;   // recorded behind every continuous run issued launch by launch: the next run, if it comes on
        hipStream_t run_stream = nullptr;  // ANOTHER stream, waits for it (the workspace, the words and the side streams are the context's)
        bool have_run_done = false;
        unsigned* edge_words = nullptr;  // the phased pipeline's dependency words (device): see ContRun::signal / wait
        size_t edge_count = 0;
        unsigned edge_seq = 0;           // runs issued with them: the value a word must reach
        hipStream_t side[3] = {};        // the pipeline's own streams (prepare / joints / chain), created on first use
        bool have_side = false;
        // Bookkeeping across continuous runs issued launch by launch with value-word edges (RSIK_OPT_CONT_GOALS_RESIDENT, see
        // rsik_control_continuous_run): which chain kernel used each workspace slot last, and what the last run wrote besides.
        struct SlotUse { size_t word; unsigned seq; } slot_use[8] = {};  // seq 0: nobody since the streams last met
        int slot_next = 0;               // the slot the next overlapped run's first block takes
        struct LastRun {
            bool valid;                  // a phased run issued launch by launch with value words; nothing since has made it useless
            unsigned seq;
            hipStream_t stream;
            const void* ws;
            const unsigned* words;
            int64_t n, n_steps, T, n_blocks;
            size_t slot_bytes;
            int slots;
            const uint8_t *state_lo, *state_hi, *reach_lo, *reach_hi;  // the rows its prepare and chain kernels wrote
        } last_run = {};
        int last_run_form = RSIK_CONT_FORM_NONE;  // RSIK_CONT_FORM_* of the last rsik_control_continuous_run (rsik_control_continuous_last_form)
        std::vector<hipEvent_t> events;  // reusable, timing disabled
        void reset_slots() { for (auto& u : slot_use) u = {0, 0}; }
        int synced(rsik_ctx* ctx);       // rsik_sync's part
        void release();                  // rsik_control_continuous_release's
        void destroy();                  // rsik_destroy's
    } cont;
    std::string err;
};

static thread_local std::string g_create_err;

static int fail(rsik_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    else g_create_err = msg;
    return code;
}
static int hip_fail(rsik_ctx* ctx, hipError_t e, const char* what) {
    return fail(ctx, RSIK_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define RSIK_HIP(ctx, call)                                   \
    do {                                                      \
        hipError_t e_ = (call);                               \
        if (e_ != hipSuccess) return hip_fail(ctx, e_, #call); \
    } while (0)

// Runtime values as template arguments: with_bool(b, f) calls f(std::true_type()) or f(std::false_type()), with_int3(i, f) calls
// f(std::integral_constant<int, i>()) for i = 0, 1, 2.  The launches nest them, so that every kernel template has one launch line
// (the one exception: cont_theta_kernel in rsik_cont_run.hpp, whose specialised steps exist for single-arm launches only).
template <class F>
static void with_bool(bool b, F&& f) { if (b) f(std::true_type()); else f(std::false_type()); }
template <class F>
static void with_int3(int i, F&& f) {
    if (i == 0) f(std::integral_constant<int, 0>()); else if (i == 1) f(std::integral_constant<int, 1>()); else f(std::integral_constant<int, 2>());
}
template <class F>
static void with_lanes(int lanes, F&& f) {  // solve_nearest_kernel's lanes per pose
    if (lanes == 1) f(std::integral_constant<int, 1>()); else if (lanes == 8) f(std::integral_constant<int, 8>()); else f(std::integral_constant<int, 64>());
}

// A column table of the ABI (`count` device pointers): refuses a NULL table ("<table> is NULL") or a NULL column ("<a_column> is
// NULL"), copies the pointers otherwise.  (An entry point that refuses its NULL table earlier, together with other pointers,
// keeps that check and its message.)  A template: outside the extern "C" block.
template <class T>
static int copy_cols(rsik_ctx* ctx, const char* who, const char* table, const char* a_column, T* const* src, T** dst, int count) {
    if (!src) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": " + table + " is NULL");
    for (int k = 0; k < count; k++) {
        if (!src[k]) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": " + a_column + " is NULL");
        dst[k] = src[k];
    }
    return RSIK_OK;
}

static bool stream_is_capturing(hipStream_t stream) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}
static void free_all(std::vector<void*>& device_blocks) {
    for (void* w : device_blocks) (void)hipFree(w);
    device_blocks.clear();
}

// The accessor form of the solve, sweep and theta-from-joints kernels (AccK): 0 one arm for the launch, 1 mixed (an arm byte per
// row), 2 mixed and the two blocks agree in everything that has no handedness (arm_const_is_sided)
static int launch_form(const rsik_ctx* ctx, const rsik::ArmC (&arms)[2], const uint8_t* arm) {
    if (!arm) return 0;
    bool mirror = !ctx->options[RSIK_OPT_NO_MIRROR];
    for (int i = 0; mirror && i < RSIK_ARM_CONSTS_COUNT; i++)
        if (!rsik::arm_const_is_sided(i) && std::memcmp(&arms[0].v[i], &arms[1].v[i], sizeof(double)) != 0) mirror = false;
    return mirror ? 2 : 1;
}
// tip offset along the goal z axis only (the default arm / the URDF): the specialised goal stage of solve and sweep applies
static bool tip_on_z(const rsik_ctx* ctx, const rsik::ArmC (&arms)[2]) {
    return arms[0].v[RSIK_C_TIPL] == 0.0 && arms[0].v[RSIK_C_TIPL + 1] == 0.0 &&
           arms[1].v[RSIK_C_TIPL] == 0.0 && arms[1].v[RSIK_C_TIPL + 1] == 0.0 && !ctx->options[RSIK_OPT_NO_TIPZ];
}

// Can the singularity-plane half of is_elbow_ok (utils.py:459-464) fail at all?  The elbow lies on the sphere of
// radius u around the shoulder, so e_z - c e_x <= s_z - c s_x + u sqrt(1 + c^2); when that bound stays below the
// plane's right-hand side (the non-DVT offset -1.01: by a metre) the test is compiled out of the launch.
static bool singularity_plane_binds(const rsik::ArmC (&arms)[2]) {
    for (int slot = 0; slot < 2; slot++) {
        const double* c = arms[slot].v;
        const double sc = c[RSIK_C_SING_COEFF];
        const double rhs = c[RSIK_C_ES + 2] - c[RSIK_C_SING_OFFSET] - sc * c[RSIK_C_ES];
        const double reach_max = c[RSIK_C_SHOULDER + 2] - sc * c[RSIK_C_SHOULDER] + c[RSIK_C_UPPER_ARM] * std::sqrt(1.0 + sc * sc);
        if (!(rhs > reach_max + 1e-6)) return true;
    }
    return false;
}

// the step kernel: rsik_control_continuous_step, and rsik_control_continuous_run where it launches step by step
static void launch_continuous_step(rsik_ctx* ctx, const uint8_t* arm, const rsik::ContinuousArgs& K, dim3 grid, dim3 block) {
    with_bool(arm != nullptr, [&](auto MIXED) { with_bool(singularity_plane_binds(K.arms), [&](auto PLANE) {
        hipLaunchKernelGGL((rsik::control_continuous_kernel<MIXED(), PLANE()>), grid, block, 0, ctx->stream, K); }); });
}

extern "C" {

int rsik_abi_version(void) { return RSIK_ABI_VERSION; }
#ifndef RSIK_SOURCE_HASH
#define RSIK_SOURCE_HASH "00000000000000000000000000000000"
#endif
const char* rsik_build_id(void) { return "RSIK_SRC_HASH=" RSIK_SOURCE_HASH; }
int rsik_arm_consts_count(void) { return RSIK_ARM_CONSTS_COUNT; }

int rsik_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rsik_create(int device_id, rsik_ctx** out) {
    if (!out) return fail(nullptr, RSIK_E_INVALID, "rsik_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(nullptr, RSIK_E_NO_DEVICE, "rsik_create: no HIP device available");
    if (device_id < 0 || device_id >= n) return fail(nullptr, RSIK_E_NO_DEVICE, "rsik_create: device id out of range");
    rsik_ctx* c = new (std::nothrow) rsik_ctx();
    if (!c) return fail(nullptr, RSIK_E_INVALID, "rsik_create: out of host memory");
    c->device = device_id;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) c->compute_units = cus;
    (void)hipDeviceGetAttribute(&c->can_wait_value, hipDeviceAttributeCanUseStreamWaitValue, device_id);
    *out = c;
    return RSIK_OK;
}

int rsik_destroy(rsik_ctx* ctx) {
    if (ctx && hipSetDevice(ctx->device) == hipSuccess) ctx->cont.destroy();
    delete ctx;
    return RSIK_OK;
}

const char* rsik_last_error(const rsik_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int rsik_set_stream(rsik_ctx* ctx, void* hip_stream) {
    if (!ctx) return RSIK_E_INVALID;
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return RSIK_OK;
}

int rsik_sync(rsik_ctx* ctx) {
    if (!ctx) return RSIK_E_INVALID;
    RSIK_HIP(ctx, hipSetDevice(ctx->device));
    RSIK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ctx->cont.synced(ctx);
}

int rsik_set_arm(rsik_ctx* ctx, int arm, const double* consts_host, int count) {
    if (!ctx) return RSIK_E_INVALID;
    if (arm != RSIK_ARM_R && arm != RSIK_ARM_L) return fail(ctx, RSIK_E_INVALID, "rsik_set_arm: arm must be 0 (r) or 1 (l)");
    if (!consts_host || count != RSIK_ARM_CONSTS_COUNT)
        return fail(ctx, RSIK_E_INVALID, "rsik_set_arm: expected RSIK_ARM_CONSTS_COUNT doubles");
    std::memcpy(ctx->arms[arm].v, consts_host, sizeof(double) * RSIK_ARM_CONSTS_COUNT);
    ctx->have_arm[arm] = true;
    return RSIK_OK;
}

int rsik_set_option(rsik_ctx* ctx, int option, int value) {
    if (!ctx) return RSIK_E_INVALID;
    if (option < 0 || option >= RSIK_OPT_COUNT) return fail(ctx, RSIK_E_INVALID, "rsik_set_option: unknown option");
    int max_value = 0;  // by name: a new option cannot shift the others, and one without a case takes no value but 0
    switch (option) {
        case RSIK_OPT_EULER_ROUNDTRIP: max_value = RSIK_EULER_NEVER; break;
        case RSIK_OPT_SWEEP_MODE: max_value = 2; break;
        case RSIK_OPT_NO_TIPZ: max_value = 1; break;
        case RSIK_OPT_NO_MIRROR: max_value = 1; break;
        case RSIK_OPT_CONT_RUN_MODE: max_value = RSIK_CONT_RUN_STEPS; break;
        case RSIK_OPT_CONT_BLOCK_STEPS: max_value = 65535; break;
        case RSIK_OPT_CONT_PHASED_VARIANT: max_value = 127; break;
        case RSIK_OPT_CONT_GOALS_RESIDENT: max_value = 1; break;
        case RSIK_OPT_NEAREST_LANES: max_value = 64; break;  // (a set, not a range: below)
    }
    if (value < 0 || value > max_value) return fail(ctx, RSIK_E_INVALID, "rsik_set_option: value out of range");
    if (option == RSIK_OPT_NEAREST_LANES && value != 0 && value != 1 && value != 8 && value != 64)
        return fail(ctx, RSIK_E_INVALID, "rsik_set_option: RSIK_OPT_NEAREST_LANES takes 0, 1, 8 or 64");
    ctx->options[option] = value;
    return RSIK_OK;
}
int rsik_get_option(const rsik_ctx* ctx, int option, int* value) {
    if (!ctx || !value || option < 0 || option >= RSIK_OPT_COUNT) return RSIK_E_INVALID;
    *value = ctx->options[option];
    return RSIK_OK;
}

int rsik_malloc(rsik_ctx* ctx, size_t bytes, void** dev_ptr) {
    if (!ctx || !dev_ptr) return RSIK_E_INVALID;
    RSIK_HIP(ctx, hipSetDevice(ctx->device));
    RSIK_HIP(ctx, hipMalloc(dev_ptr, bytes));
    return RSIK_OK;
}
int rsik_free(rsik_ctx* ctx, void* dev_ptr) {
    if (!ctx) return RSIK_E_INVALID;
    RSIK_HIP(ctx, hipSetDevice(ctx->device));
    RSIK_HIP(ctx, hipFree(dev_ptr));
    return RSIK_OK;
}
int rsik_memcpy_h2d(rsik_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes) {
    if (!ctx) return RSIK_E_INVALID;
    RSIK_HIP(ctx, hipSetDevice(ctx->device));
    RSIK_HIP(ctx, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    RSIK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RSIK_OK;
}
int rsik_memcpy_d2h(rsik_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes) {
    if (!ctx) return RSIK_E_INVALID;
    RSIK_HIP(ctx, hipSetDevice(ctx->device));
    RSIK_HIP(ctx, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RSIK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RSIK_OK;
}

static int check_arms(rsik_ctx* ctx, const uint8_t* arm, int arm_uniform, const char* who) {
    if (arm) {
        if (!ctx->have_arm[0] || !ctx->have_arm[1])
            return fail(ctx, RSIK_E_NOT_SET, std::string(who) + ": per-pose arm ids need both arms' constants (rsik_set_arm)");
    } else {
        if (arm_uniform != RSIK_ARM_R && arm_uniform != RSIK_ARM_L)
            return fail(ctx, RSIK_E_INVALID, std::string(who) + ": arm_uniform must be 0 (r) or 1 (l)");
        if (!ctx->have_arm[arm_uniform])
            return fail(ctx, RSIK_E_NOT_SET, std::string(who) + ": constants of the requested arm were not uploaded");
    }
    return RSIK_OK;
}

static int launch_dims(rsik_ctx* ctx, int64_t n, dim3* grid, const char* who, int threads = rsik::kBlock) {
    const int64_t blocks = (n + threads - 1) / threads;
    if (blocks > 0x7fffffffLL) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": n too large for one launch");
    *grid = dim3((unsigned)blocks);
    return RSIK_OK;
}
// what brackets every launch: the context's device and the grid for n rows, then the launch's own error
static int launch_begin(rsik_ctx* ctx, int64_t n, dim3* grid, const char* who, int threads = rsik::kBlock) {
    RSIK_HIP(ctx, hipSetDevice(ctx->device));
    return launch_dims(ctx, n, grid, who, threads);
}
static int launch_end(rsik_ctx* ctx) {
    RSIK_HIP(ctx, hipGetLastError());
    return RSIK_OK;
}

// K.arms of a launch check_arms has passed: slot 0 = r, slot 1 = l with per-pose arm ids, the one arm in both slots without
static int slot_arm(const uint8_t* arm, int arm_uniform, int slot) { return arm ? slot : arm_uniform; }
static void bind_arms(const rsik_ctx* ctx, const uint8_t* arm, int arm_uniform, rsik::ArmC (&arms)[2]) {
    for (int slot = 0; slot < 2; slot++) arms[slot] = ctx->arms[slot_arm(arm, arm_uniform, slot)];
}
// seven joints' worth of host values into an argument block: the caller's, or `otherwise` for each where it passed NULL
static void fill7(double (&dst)[7], const double* src_host, double otherwise) {
    for (int k = 0; k < 7; k++) dst[k] = src_host ? src_host[k] : otherwise;
}

// The sampling family (rsik_solve_sweep, rsik_solve_nearest, rsik_solve_path): the same poses, the same theta grid and the same
// per-pose interval / reachable / state.  What their host side shares is here.  A check only one of them makes stays in that entry
// point, between the shared ones: the order of the checks, and with it the fault a call with two of them reports, is part of the ABI.
// The checks on the sample arguments, in that order: n_theta, theta_policy, flags, weights, arms.
static int check_samples(rsik_ctx* ctx, const char* who, int n_theta, int n_theta_max, int theta_policy, int flags, int flags_mask,
                         const double* weights_host, const uint8_t* arm, int arm_uniform) {
    const std::string w(who);
    if (n_theta < 1 || n_theta > n_theta_max) return fail(ctx, RSIK_E_INVALID, w + ": n_theta must be in [1, " + std::to_string(n_theta_max) + "]");
    if (theta_policy != RSIK_THETA_EXPLICIT && theta_policy != RSIK_THETA_FRACTION)
        return fail(ctx, RSIK_E_INVALID, w + ": theta_policy must be RSIK_THETA_EXPLICIT or RSIK_THETA_FRACTION");
    if (flags & ~flags_mask) return fail(ctx, RSIK_E_INVALID, w + ": unknown bits in flags");
    for (int q = 0; weights_host && q < 7; q++)
        if (!(weights_host[q] >= 0.0 && std::isfinite(weights_host[q]))) return fail(ctx, RSIK_E_INVALID, w + ": every weight must be finite and >= 0");
    return check_arms(ctx, arm, arm_uniform, who);
}
// the inputs no launch of n > 0 goes without
static int check_sample_inputs(rsik_ctx* ctx, const char* who, const double* const pose_soa[6], const double* theta_in) {
    if (!pose_soa) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": pose_soa is NULL");
    if (!theta_in) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": theta_in is NULL");
    return RSIK_OK;
}
extern "C++" {  // (templates)
// The fields SweepArgs, NearestArgs and PathArgs have in common, by name (the structs stay apart: each is its kernel's kernarg layout)
template <class ARGS>
static int fill_samples(rsik_ctx* ctx, const char* who, ARGS& K, int64_t n, const double* const pose_soa[6], const uint8_t* arm, int arm_uniform,
                        int n_theta, int theta_policy, const double* theta_in, int theta_per_pose, double* interval, uint8_t* reachable, uint8_t* state) {
    K.n = n;
    const int rc = copy_cols(ctx, who, "pose_soa", "a pose_soa column", pose_soa, K.in, 6);
    if (rc != RSIK_OK) return rc;
    K.arm = arm;
    K.theta_policy = theta_policy;
    K.n_theta = n_theta;
    K.theta_per_pose = theta_per_pose != 0;
    K.theta_in = theta_in;
    K.interval = interval; K.reachable = reachable; K.state = state;
    bind_arms(ctx, arm, arm_uniform, K.arms);
    return RSIK_OK;
}
// get_joints' previous_joints of an argument block that holds either form (rsik_solve and rsik_solve_rows too): one device row per
// pose, or one host row for every pose
template <class ARGS>
static void bind_prev(ARGS& K, const double* rows, const double* host) {
    if (rows) K.prev_rows = rows;  // (shares its kernarg bytes with K.prev)
    else fill7(K.prev, host, 0.0);
}
}

// rsik_solve (previous_rows == NULL: previous_joints_host for every pose) and rsik_solve_rows (previous_rows: one device row per pose)
static int solve_impl(rsik_ctx* ctx, const char* who, int64_t n, const double* const pose_soa[6], const uint8_t* arm, int arm_uniform,
                      int theta_policy, const double* theta_in, const double* previous_joints_host, const double* previous_rows,
                      double* joints, double* interval, double* elbow, uint8_t* reachable, uint8_t* state) {
    const std::string w(who);
    if (n < 0) return fail(ctx, RSIK_E_INVALID, w + ": n < 0");
    if (theta_policy < RSIK_THETA_INTERVAL0 || theta_policy > RSIK_THETA_NONE)
        return fail(ctx, RSIK_E_INVALID, w + ": unknown theta_policy");
    if ((theta_policy == RSIK_THETA_EXPLICIT || theta_policy == RSIK_THETA_FRACTION) && !theta_in && n > 0)
        return fail(ctx, RSIK_E_INVALID, w + ": theta_in is required for this theta_policy");
    int rc = check_arms(ctx, arm, arm_uniform, who);
    if (rc != RSIK_OK) return rc;
    if (n == 0) return RSIK_OK;
    rsik::SolveArgs K;
    K.n = n;
    if ((rc = copy_cols(ctx, who, "pose_soa", "a pose_soa column", pose_soa, K.in, 6)) != RSIK_OK) return rc;
    K.arm = arm;
    K.theta_policy = theta_policy;
    K.theta_in = theta_in;
    bind_prev(K, previous_rows, previous_joints_host);
    K.joints = joints; K.interval = interval; K.elbow = elbow; K.reachable = reachable; K.state = state;
    bind_arms(ctx, arm, arm_uniform, K.arms);
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, who)) != RSIK_OK) return rc;
    with_int3(launch_form(ctx, K.arms, arm), [&](auto FORM) { with_bool(tip_on_z(ctx, K.arms), [&](auto TIPZ) { with_bool(previous_rows != nullptr, [&](auto PREV_ROWS) {
        hipLaunchKernelGGL((rsik::solve_kernel<FORM(), TIPZ(), PREV_ROWS()>), grid, block, 0, ctx->stream, K); }); }); });
    return launch_end(ctx);
}

int rsik_solve(rsik_ctx* ctx, int64_t n, const double* const pose_soa[6], const uint8_t* arm, int arm_uniform,
               int theta_policy, const double* theta_in, const double* previous_joints_host, double* joints,
               double* interval, double* elbow, uint8_t* reachable, uint8_t* state) {
    if (!ctx) return RSIK_E_INVALID;
    return solve_impl(ctx, "rsik_solve", n, pose_soa, arm, arm_uniform, theta_policy, theta_in, previous_joints_host, nullptr,
                      joints, interval, elbow, reachable, state);
}

int rsik_solve_rows(rsik_ctx* ctx, int64_t n, const double* const pose_soa[6], const uint8_t* arm, int arm_uniform,
                    int theta_policy, const double* theta_in, const double* previous_joints, double* joints,
                    double* interval, double* elbow, uint8_t* reachable, uint8_t* state) {
    if (!ctx) return RSIK_E_INVALID;
    if (!previous_joints) return fail(ctx, RSIK_E_INVALID, "rsik_solve_rows: previous_joints is NULL");
    return solve_impl(ctx, "rsik_solve_rows", n, pose_soa, arm, arm_uniform, theta_policy, theta_in, nullptr, previous_joints,
                      joints, interval, elbow, reachable, state);
}

// rsik_solve_sweep: is_reachable once per pose, get_joints at n_theta elbow angles (rsik_kernel_sweep.hpp)
int rsik_solve_sweep(rsik_ctx* ctx, int64_t n, const double* const pose_soa[6], const uint8_t* arm, int arm_uniform,
                     int n_theta, int theta_policy, const double* theta_in, int theta_per_pose,
                     const double* previous_joints,
                     double* joints, double* elbow, uint8_t* projected, double* theta,
                     double* interval, uint8_t* reachable, uint8_t* state) {
    if (!ctx) return RSIK_E_INVALID;
    const char* who = "rsik_solve_sweep";
    const std::string w(who);
    if (n < 0) return fail(ctx, RSIK_E_INVALID, w + ": n < 0");
    int rc = check_samples(ctx, who, n_theta, 4096, theta_policy, 0, 0, nullptr, arm, arm_uniform);
    if (rc != RSIK_OK) return rc;
    if (n == 0) return RSIK_OK;
    if ((rc = check_sample_inputs(ctx, who, pose_soa, theta_in)) != RSIK_OK) return rc;
    if (!joints) return fail(ctx, RSIK_E_INVALID, w + ": joints is NULL");
    rsik::SweepArgs K;
    if ((rc = fill_samples(ctx, who, K, n, pose_soa, arm, arm_uniform, n_theta, theta_policy, theta_in, theta_per_pose, interval, reachable, state)) != RSIK_OK) return rc;
    bind_prev(K, previous_joints, nullptr);
    K.joints = joints; K.elbow = elbow; K.projected = projected; K.theta = theta;
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, who)) != RSIK_OK) return rc;
    with_int3(launch_form(ctx, K.arms, arm), [&](auto FORM) { with_bool(tip_on_z(ctx, K.arms), [&](auto TIPZ) { with_bool(previous_joints != nullptr, [&](auto PREV_ROWS) {
        hipLaunchKernelGGL((rsik::solve_sweep_kernel<FORM(), TIPZ(), PREV_ROWS()>), grid, block, 0, ctx->stream, K); }); }); });
    return launch_end(ctx);
}

// Lanes per pose of solve_nearest_kernel where RSIK_OPT_NEAREST_LANES leaves the choice to the library: a function of n and n_theta
// alone, the form scripts/nearest_cost.py measured fastest at each of its shapes (DESIGN section 3 "Nearest": with 64 samples 1 lane
// at 262 144 poses, 8 from 65 536 down to 4096, where 64 lanes draw level; 64 at 64 x 1024 and 2 x 1024).  The step from 8 lanes to 1
// sits halfway (in the logarithm) between the two shapes that bracket it, and a pose never gets more lanes than it has samples for
// more than one round of.
static int nearest_lanes(int64_t n, int n_theta) {
    if (n >= 131072 || n_theta == 1) return 1;
    if (n >= 4096 || n_theta <= 8) return 8;
    return 64;
}

// rsik_solve_nearest: rsik_solve_sweep's samples, and of them the one nearest to the pose's seed joints (rsik_kernel_nearest.hpp)
int rsik_solve_nearest(rsik_ctx* ctx, int64_t n, const double* const pose_soa[6], const uint8_t* arm, int arm_uniform,
                       int n_theta, int theta_policy, const double* theta_in, int theta_per_pose,
                       const double* previous_joints, const double* seed_joints, const double* weights_host, int flags,
                       int32_t* index, double* theta, double* joints, double* elbow, double* cost, uint8_t* projected,
                       double* interval, uint8_t* reachable, uint8_t* state) {
    if (!ctx) return RSIK_E_INVALID;
    const char* who = "rsik_solve_nearest";
    const std::string w(who);
    if (n < 0) return fail(ctx, RSIK_E_INVALID, w + ": n < 0");
    int rc = check_samples(ctx, who, n_theta, 4096, theta_policy, flags, RSIK_NEAREST_SKIP_PROJECTED, weights_host, arm, arm_uniform);
    if (rc != RSIK_OK) return rc;
    if (n == 0) return RSIK_OK;
    if ((rc = check_sample_inputs(ctx, who, pose_soa, theta_in)) != RSIK_OK) return rc;
    if (!seed_joints) return fail(ctx, RSIK_E_INVALID, w + ": seed_joints is NULL");
    if (!index && !theta && !joints) return fail(ctx, RSIK_E_INVALID, w + ": index, theta and joints are all NULL");
    rsik::NearestArgs K;
    if ((rc = fill_samples(ctx, who, K, n, pose_soa, arm, arm_uniform, n_theta, theta_policy, theta_in, theta_per_pose, interval, reachable, state)) != RSIK_OK) return rc;
    K.skip_projected = (flags & RSIK_NEAREST_SKIP_PROJECTED) != 0;
    bind_prev(K, previous_joints, nullptr);
    K.seed = seed_joints;
    fill7(K.weights, weights_host, 1.0);
    K.index = index; K.theta = theta; K.joints = joints; K.elbow = elbow; K.cost = cost; K.projected = projected;
    const int lanes = ctx->options[RSIK_OPT_NEAREST_LANES] ? ctx->options[RSIK_OPT_NEAREST_LANES] : nearest_lanes(n, n_theta);
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, who, rsik::kBlock / lanes)) != RSIK_OK) return rc;
    with_int3(launch_form(ctx, K.arms, arm), [&](auto FORM) { with_bool(tip_on_z(ctx, K.arms), [&](auto TIPZ) { with_bool(previous_joints != nullptr, [&](auto PREV_ROWS) { with_lanes(lanes, [&](auto LANES) {
        hipLaunchKernelGGL((rsik::solve_nearest_kernel<FORM(), TIPZ(), PREV_ROWS(), LANES()>), grid, block, 0, ctx->stream, K); }); }); }); });
    return launch_end(ctx);
}

// rsik_solve_path's workspace: the backpointer table, one byte per (path, waypoint, sample), and one winner byte per (path, waypoint)
static bool path_workspace_bytes(int64_t n, int64_t n_steps, int n_theta, size_t* bytes) {
    if (n < 0 || n_steps < 1 || n_steps > 65536 || n_theta < 1 || n_theta > 64) return false;
    const unsigned __int128 b = (unsigned __int128)n * (unsigned __int128)n_steps * (unsigned)(n_theta + 1);
    if (b > (unsigned __int128)SIZE_MAX) return false;
    *bytes = (size_t)b;
    return true;
}
int rsik_solve_path_workspace_bytes(int64_t n, int64_t n_steps, int n_theta, size_t* bytes) {
    if (!bytes || !path_workspace_bytes(n, n_steps, n_theta, bytes)) return RSIK_E_INVALID;
    return RSIK_OK;
}

// What rsik_solve_path and rsik_solve_path_clear share.  The checks come in two halves, in the order that is part of the ABI: those a call
// with n == 0 makes too, and those on the inputs no launch of n > 0 goes without; rsik_solve_path_clear's own stand behind each half.
static int check_path_shape(rsik_ctx* ctx, const char* who, int64_t n, int64_t n_steps, int n_theta, int theta_policy, int flags,
                            const double* weights_host, const uint8_t* arm, int arm_uniform) {
    const std::string w(who);
    if (n < 0) return fail(ctx, RSIK_E_INVALID, w + ": n < 0");
    if (n_steps < 1 || n_steps > 65536) return fail(ctx, RSIK_E_INVALID, w + ": n_steps must be in [1, 65536]");
    return check_samples(ctx, who, n_theta, 64, theta_policy, flags, RSIK_PATH_SKIP_PROJECTED | RSIK_PATH_UNWIND, weights_host, arm, arm_uniform);
}
static int check_path_inputs(rsik_ctx* ctx, const char* who, int64_t n, int64_t n_steps, int n_theta, const double* const pose_soa[6],
                             const double* theta_in, const void* workspace, size_t workspace_bytes, const int32_t* index,
                             const double* theta, const double* joints) {
    const std::string w(who);
    const int rc = check_sample_inputs(ctx, who, pose_soa, theta_in);
    if (rc != RSIK_OK) return rc;
    if (!index && !theta && !joints) return fail(ctx, RSIK_E_INVALID, w + ": index, theta and joints are all NULL");
    size_t need = 0;
    if (!path_workspace_bytes(n, n_steps, n_theta, &need)) return fail(ctx, RSIK_E_INVALID, w + ": n * n_steps too large");
    if (!workspace || workspace_bytes < need) return fail(ctx, RSIK_E_INVALID, w + ": workspace is NULL or smaller than rsik_solve_path_workspace_bytes");
    return RSIK_OK;
}
extern "C++" {  // (templates)
// PathArgs or PathClearArgs: the fields of the first, by name
template <class ARGS>
static int fill_path(rsik_ctx* ctx, const char* who, ARGS& K, int64_t n, int64_t n_steps, const double* const pose_soa[6], const uint8_t* arm,
                     int arm_uniform, int n_theta, int theta_policy, const double* theta_in, int theta_per_pose, const double* start_joints,
                     const double* weights_host, int flags, void* workspace, int32_t* index, double* theta, double* joints, double* elbow,
                     uint8_t* projected, double* step_cost, double* cost, int32_t* n_solved, double* interval, uint8_t* reachable, uint8_t* state) {
    const int rc = fill_samples(ctx, who, K, n, pose_soa, arm, arm_uniform, n_theta, theta_policy, theta_in, theta_per_pose, interval, reachable, state);
    if (rc != RSIK_OK) return rc;
    K.n_steps = n_steps;
    K.skip_projected = (flags & RSIK_PATH_SKIP_PROJECTED) != 0;
    K.unwind = (flags & RSIK_PATH_UNWIND) != 0;
    fill7(K.prev, nullptr, 0.0);
    K.start = start_joints;
    fill7(K.weights, weights_host, 1.0);
    K.back = static_cast<uint8_t*>(workspace);
    K.index = index; K.theta = theta; K.joints = joints; K.elbow = elbow; K.projected = projected;
    K.step_cost = step_cost; K.cost = cost; K.n_solved = n_solved;
    return RSIK_OK;
}
}

// rsik_solve_path: rsik_solve_sweep's samples at every waypoint of n paths, and the way through them that moves the joints least (rsik_kernel_path.hpp)
int rsik_solve_path(rsik_ctx* ctx, int64_t n, int64_t n_steps, const double* const pose_soa[6], const uint8_t* arm, int arm_uniform,
                    int n_theta, int theta_policy, const double* theta_in, int theta_per_pose,
                    const double* start_joints, const double* weights_host, int flags,
                    void* workspace, size_t workspace_bytes,
                    int32_t* index, double* theta, double* joints, double* elbow, uint8_t* projected,
                    double* step_cost, double* cost, int32_t* n_solved,
                    double* interval, uint8_t* reachable, uint8_t* state) {
    if (!ctx) return RSIK_E_INVALID;
    const char* who = "rsik_solve_path";
    int rc = check_path_shape(ctx, who, n, n_steps, n_theta, theta_policy, flags, weights_host, arm, arm_uniform);
    if (rc != RSIK_OK) return rc;
    if (n == 0) return RSIK_OK;
    if ((rc = check_path_inputs(ctx, who, n, n_steps, n_theta, pose_soa, theta_in, workspace, workspace_bytes, index, theta, joints)) != RSIK_OK) return rc;
    rsik::PathArgs K;
    if ((rc = fill_path(ctx, who, K, n, n_steps, pose_soa, arm, arm_uniform, n_theta, theta_policy, theta_in, theta_per_pose, start_joints,
                        weights_host, flags, workspace, index, theta, joints, elbow, projected, step_cost, cost, n_solved, interval, reachable, state)) != RSIK_OK) return rc;
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, who, rsik::kBlock / 64)) != RSIK_OK) return rc;
    with_int3(launch_form(ctx, K.arms, arm), [&](auto FORM) { with_bool(tip_on_z(ctx, K.arms), [&](auto TIPZ) {
        hipLaunchKernelGGL((rsik::solve_path_kernel<FORM(), TIPZ()>), grid, block, 0, ctx->stream, K); }); });
    return launch_end(ctx);
}

// rsik_solve_path_clear: rsik_solve_path where a sample nearer than min_clearance to a static scene is no candidate, and one nearer
// than `influence` pays for it (solve_path_kernel over PathClearArgs, rsik_kernel_path.hpp).  The scene's limits and checks are rsik_track_avoid's.
int rsik_solve_path_clear(rsik_ctx* ctx, int64_t n, int64_t n_steps, const double* const pose_soa[6], const uint8_t* arm, int arm_uniform,
                          int n_theta, int theta_policy, const double* theta_in, int theta_per_pose,
                          const double* start_joints, const double* weights_host, int flags,
                          const double* link_radius_host, int n_spheres, const double* spheres, int n_capsules, const double* capsules,
                          double min_clearance, double influence, double clearance_gain,
                          void* workspace, size_t workspace_bytes,
                          int32_t* index, double* theta, double* joints, double* elbow, uint8_t* projected,
                          double* step_cost, double* cost, int32_t* n_solved,
                          double* interval, uint8_t* reachable, uint8_t* state,
                          double* clearance, int32_t* nearest, uint8_t* blocked) {
    if (!ctx) return RSIK_E_INVALID;
    const char* who = "rsik_solve_path_clear";
    const std::string w(who);
    const auto gain_ok = [](double g) { return std::isfinite(g) && g >= 0.0; };
    int rc = check_path_shape(ctx, who, n, n_steps, n_theta, theta_policy, flags, weights_host, arm, arm_uniform);
    if (rc != RSIK_OK) return rc;
    if (n_spheres < 0 || n_spheres > rsik::kAvoidMaxSpheres) return fail(ctx, RSIK_E_INVALID, w + ": n_spheres must be 0 ... 256");
    if (n_capsules < 0 || n_capsules > rsik::kAvoidMaxCapsules) return fail(ctx, RSIK_E_INVALID, w + ": n_capsules must be 0 ... 64");
    if (n_spheres + n_capsules < 1) return fail(ctx, RSIK_E_INVALID, w + ": at least one obstacle (without obstacles: rsik_solve_path)");
    for (int l = 0; link_radius_host && l < 3; l++)
        if (!gain_ok(link_radius_host[l])) return fail(ctx, RSIK_E_INVALID, w + ": every link radius must be finite and >= 0");
    if (!gain_ok(influence) || !gain_ok(clearance_gain))
        return fail(ctx, RSIK_E_INVALID, w + ": influence and clearance_gain must be finite and >= 0");
    if (!(min_clearance < __builtin_inf()))  // (a NaN fails it too)
        return fail(ctx, RSIK_E_INVALID, w + ": min_clearance must be finite or -infinity");
    if (n == 0) return RSIK_OK;
    if ((rc = check_path_inputs(ctx, who, n, n_steps, n_theta, pose_soa, theta_in, workspace, workspace_bytes, index, theta, joints)) != RSIK_OK) return rc;
    if ((n_spheres > 0 && !spheres) || (n_capsules > 0 && !capsules))
        return fail(ctx, RSIK_E_INVALID, w + ": spheres or capsules is NULL with a count above 0");
    if (((uintptr_t)nearest & 7) != 0) return fail(ctx, RSIK_E_INVALID, w + ": nearest must be aligned to 8 bytes");
    rsik::PathClearArgs K;
    if ((rc = fill_path(ctx, who, K, n, n_steps, pose_soa, arm, arm_uniform, n_theta, theta_policy, theta_in, theta_per_pose, start_joints,
                        weights_host, flags, workspace, index, theta, joints, elbow, projected, step_cost, cost, n_solved, interval, reachable, state)) != RSIK_OK) return rc;
    K.spheres = spheres; K.capsules = capsules; K.n_spheres = n_spheres; K.n_capsules = n_capsules;
    K.clearance = clearance; K.nearest = nearest; K.blocked = blocked;
    K.min_clearance = min_clearance; K.influence = influence; K.clearance_gain = clearance_gain;
    for (int l = 0; l < 3; l++) K.link_radius[l] = link_radius_host ? link_radius_host[l] : 0.0;
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, who, rsik::kBlock / 64)) != RSIK_OK) return rc;
    with_int3(launch_form(ctx, K.arms, arm), [&](auto FORM) { with_bool(tip_on_z(ctx, K.arms), [&](auto TIPZ) {
        hipLaunchKernelGGL((rsik::solve_path_kernel<FORM(), TIPZ(), rsik::PathClearArgs>), grid, block, 0, ctx->stream, K); }); });
    return launch_end(ctx);
}

// rsik_solve_path_pair's workspace: a backpointer byte per (robot, waypoint, pair of samples), a flag byte per (robot, waypoint) and
// the two winners of each
static bool path_pair_workspace_bytes(int64_t n_pairs, int64_t n_steps, int n_theta, size_t* bytes) {
    if (n_pairs < 0 || n_pairs > 0x3fffffffffffffffLL || n_steps < 1 || n_steps > 65536 || n_theta < 1 || n_theta > rsik::kPairMaxTheta) return false;
    const unsigned __int128 b = (unsigned __int128)n_pairs * (unsigned __int128)n_steps * (unsigned)(n_theta * n_theta + 3);
    if (b > (unsigned __int128)SIZE_MAX) return false;
    *bytes = (size_t)b;
    return true;
}
int rsik_solve_path_pair_workspace_bytes(int64_t n_pairs, int64_t n_steps, int n_theta, size_t* bytes) {
    if (!bytes || !path_pair_workspace_bytes(n_pairs, n_steps, n_theta, bytes)) return RSIK_E_INVALID;
    return RSIK_OK;
}

// rsik_solve_path_pair: rsik_solve_path_clear for robots of two arms, each arm an obstacle to the other; a state is a pair of samples
// (solve_path_pair_kernel, rsik_kernel_path_pair.hpp).  The checks are rsik_solve_path_clear's in its order, without "no obstacle".
int rsik_solve_path_pair(rsik_ctx* ctx, int64_t n_pairs, int64_t n_steps, const double* const pose_soa[6],
                         int n_theta, int theta_policy, const double* theta_in, int theta_per_pose,
                         const double* start_joints, const double* weights_host, int flags,
                         const double* link_radius_host, int n_spheres, const double* spheres, int n_capsules, const double* capsules,
                         double min_clearance, double influence, double clearance_gain,
                         void* workspace, size_t workspace_bytes,
                         int32_t* index, double* theta, double* joints, double* elbow, uint8_t* projected,
                         double* step_cost, double* cost, int32_t* n_solved,
                         double* interval, uint8_t* reachable, uint8_t* state,
                         double* clearance, int32_t* nearest, uint16_t* blocked) {
    if (!ctx) return RSIK_E_INVALID;
    const char* who = "rsik_solve_path_pair";
    const std::string w(who);
    const auto gain_ok = [](double g) { return std::isfinite(g) && g >= 0.0; };
    if (n_pairs < 0) return fail(ctx, RSIK_E_INVALID, w + ": n_pairs < 0");
    if (n_pairs > 0x3fffffffffffffffLL) return fail(ctx, RSIK_E_INVALID, w + ": n too large for one launch");
    if (n_steps < 1 || n_steps > 65536) return fail(ctx, RSIK_E_INVALID, w + ": n_steps must be in [1, 65536]");
    if (n_theta < 1 || n_theta > rsik::kPairMaxTheta) return fail(ctx, RSIK_E_INVALID, w + ": n_theta must be in [1, 16]");
    if (theta_policy != RSIK_THETA_EXPLICIT && theta_policy != RSIK_THETA_FRACTION)
        return fail(ctx, RSIK_E_INVALID, w + ": theta_policy must be RSIK_THETA_EXPLICIT or RSIK_THETA_FRACTION");
    if (flags & ~(RSIK_PATH_SKIP_PROJECTED | RSIK_PATH_UNWIND)) return fail(ctx, RSIK_E_INVALID, w + ": unknown bits in flags");
    for (int q = 0; weights_host && q < 7; q++)
        if (!(weights_host[q] >= 0.0 && std::isfinite(weights_host[q]))) return fail(ctx, RSIK_E_INVALID, w + ": every weight must be finite and >= 0");
    if (!ctx->have_arm[RSIK_ARM_R] || !ctx->have_arm[RSIK_ARM_L])
        return fail(ctx, RSIK_E_NOT_SET, w + ": both arms' constants are needed (rsik_set_arm)");
    if (n_spheres < 0 || n_spheres > rsik::kAvoidMaxSpheres) return fail(ctx, RSIK_E_INVALID, w + ": n_spheres must be 0 ... 256");
    if (n_capsules < 0 || n_capsules > rsik::kAvoidMaxCapsules) return fail(ctx, RSIK_E_INVALID, w + ": n_capsules must be 0 ... 64");
    for (int l = 0; link_radius_host && l < 3; l++)
        if (!gain_ok(link_radius_host[l])) return fail(ctx, RSIK_E_INVALID, w + ": every link radius must be finite and >= 0");
    if (!gain_ok(influence) || !gain_ok(clearance_gain))
        return fail(ctx, RSIK_E_INVALID, w + ": influence and clearance_gain must be finite and >= 0");
    if (!(min_clearance < __builtin_inf()))  // (a NaN fails it too)
        return fail(ctx, RSIK_E_INVALID, w + ": min_clearance must be finite or -infinity");
    if (n_pairs == 0) return RSIK_OK;
    int rc = check_sample_inputs(ctx, who, pose_soa, theta_in);
    if (rc != RSIK_OK) return rc;
    if (!index && !theta && !joints) return fail(ctx, RSIK_E_INVALID, w + ": index, theta and joints are all NULL");
    size_t need = 0;
    if (!path_pair_workspace_bytes(n_pairs, n_steps, n_theta, &need)) return fail(ctx, RSIK_E_INVALID, w + ": n_pairs * n_steps too large");
    if (!workspace || workspace_bytes < need)
        return fail(ctx, RSIK_E_INVALID, w + ": workspace is NULL or smaller than rsik_solve_path_pair_workspace_bytes");
    if ((n_spheres > 0 && !spheres) || (n_capsules > 0 && !capsules))
        return fail(ctx, RSIK_E_INVALID, w + ": spheres or capsules is NULL with a count above 0");
    if (((uintptr_t)nearest & 7) != 0) return fail(ctx, RSIK_E_INVALID, w + ": nearest must be aligned to 8 bytes");
    const int64_t n = 2 * n_pairs;  // rows: 2i the right arm of robot i, 2i + 1 its left arm
    rsik::PathPairArgs K;  // (K.arm stays NULL: the arm of a row is its parity)
    K.n = n;
    if ((rc = copy_cols(ctx, who, "pose_soa", "a pose_soa column", pose_soa, K.in, 6)) != RSIK_OK) return rc;
    K.n_steps = n_steps; K.arm = nullptr;
    K.theta_policy = theta_policy; K.n_theta = n_theta; K.theta_per_pose = theta_per_pose != 0; K.theta_in = theta_in;
    K.skip_projected = (flags & RSIK_PATH_SKIP_PROJECTED) != 0;
    K.unwind = (flags & RSIK_PATH_UNWIND) != 0;
    fill7(K.prev, nullptr, 0.0);
    K.start = start_joints;
    fill7(K.weights, weights_host, 1.0);
    K.back = static_cast<uint8_t*>(workspace);
    K.index = index; K.theta = theta; K.joints = joints; K.elbow = elbow; K.projected = projected;
    K.step_cost = step_cost; K.cost = cost; K.n_solved = n_solved;
    K.interval = interval; K.reachable = reachable; K.state = state;
    K.spheres = spheres; K.capsules = capsules; K.n_spheres = n_spheres; K.n_capsules = n_capsules;
    K.clearance = clearance; K.nearest = nearest; K.blocked = blocked;
    K.min_clearance = min_clearance; K.influence = influence; K.clearance_gain = clearance_gain;
    for (int l = 0; l < 3; l++) K.link_radius[l] = link_radius_host ? link_radius_host[l] : 0.0;
    K.arms[0] = ctx->arms[RSIK_ARM_R]; K.arms[1] = ctx->arms[RSIK_ARM_L];
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n_pairs, &grid, who, rsik::kBlock / 64)) != RSIK_OK) return rc;
    with_bool(tip_on_z(ctx, K.arms), [&](auto TIPZ) {
        hipLaunchKernelGGL((rsik::solve_path_pair_kernel<TIPZ()>), grid, block, 0, ctx->stream, K); });
    return launch_end(ctx);
}

// Positions per wave of reach_map_kernel: as many (16, 8, 4, 2, 1) as still leave eight workgroups per compute unit, so that positions which
// end early ("Pose out of reach" is a scalar branch) do not leave compute units idle; above that, more positions per workgroup
// spread the orientation stage and the table staging over more poses.
static int reach_map_pos_per_wave(const rsik_ctx* ctx, int64_t n_pos) {
    for (int ppw = rsik::kReachMapMaxPosPerWave; ppw > 1; ppw >>= 1)
        if (n_pos >= (int64_t)ctx->compute_units * 8 * rsik::kReachMapWaves * ppw) return ppw;
    return 1;
}

// rsik_reach_map: is_reachable of n_pos positions x n_rot orientations, reduced per position on the device (rsik_kernel_reach_map.hpp)
int rsik_reach_map(rsik_ctx* ctx, int64_t n_pos, const double* const pos_soa[3], const uint8_t* arm, int arm_uniform,
                   int n_rot, const double* const euler_soa[3],
                   uint32_t* count, uint32_t* state_count, double* theta_measure, uint64_t* mask) {
    if (!ctx) return RSIK_E_INVALID;
    const char* who = "rsik_reach_map";
    const std::string w(who);
    if (n_pos < 0) return fail(ctx, RSIK_E_INVALID, w + ": n_pos < 0");
    if (n_rot < 1 || n_rot > 4096) return fail(ctx, RSIK_E_INVALID, w + ": n_rot must be in [1, 4096]");
    int rc = check_arms(ctx, arm, arm_uniform, who);
    if (rc != RSIK_OK) return rc;
    if (!count && !state_count && !theta_measure && !mask) return fail(ctx, RSIK_E_INVALID, w + ": count, state_count, theta_measure and mask are all NULL");
    if (n_pos == 0) return RSIK_OK;
    rsik::ReachMapArgs K;
    K.n_pos = n_pos;
    if ((rc = copy_cols(ctx, who, "pos_soa", "a pos_soa column", pos_soa, K.pos, 3)) != RSIK_OK) return rc;
    if ((rc = copy_cols(ctx, who, "euler_soa", "a euler_soa column", euler_soa, K.eul, 3)) != RSIK_OK) return rc;
    K.arm = arm;
    K.n_rot = n_rot;
    K.tile = std::min((n_rot + 63) & ~63, rsik::kReachMapTile);
    K.pos_per_wave = reach_map_pos_per_wave(ctx, n_pos);
    K.count = count; K.state_count = state_count; K.theta_measure = theta_measure; K.mask = mask;
    bind_arms(ctx, arm, arm_uniform, K.arms);
    const int form = launch_form(ctx, K.arms, arm);
    const size_t lds_bytes = rsik::reach_map_lds_bytes(form != 0 ? 2 : 1, K.tile);  // at most 49 KiB: no attribute to raise
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n_pos, &grid, who, rsik::kReachMapWaves * K.pos_per_wave)) != RSIK_OK) return rc;
    with_int3(form, [&](auto FORM) { with_bool(tip_on_z(ctx, K.arms), [&](auto TIPZ) {
        hipLaunchKernelGGL((rsik::reach_map_kernel<FORM(), TIPZ()>), grid, block, lds_bytes, ctx->stream, K); }); });
    return launch_end(ctx);
}

// Python float modulo (sign of the divisor), used for the l-arm limit wrap (C:243-250).
static double host_pymod(double a, double b) {
    double m = std::fmod(a, b);
    if (m != 0.0) {
        if ((b < 0) != (m < 0)) m += b;
    } else {
        m = std::copysign(0.0, b);
    }
    return m;
}

// C:225-252: interval_limit per constrained mode, mirrored and re-wrapped for the left arm.
static void control_limits(int arm, int constrained_mode, double preferred_theta, double lim[2], double* pref) {
    const double pi = rsik::kPi;
    if (constrained_mode == RSIK_MODE_UNCONSTRAINED) { lim[0] = 3 * pi / 4; lim[1] = -2 * pi / 6; }
    else { lim[0] = -4 * pi / 5; lim[1] = 0; }
    if (arm == RSIK_ARM_L) {
        double a = -pi - lim[1], b = -pi - lim[0];
        lim[0] = a; lim[1] = b;
        if (lim[0] < -pi) lim[0] = host_pymod(lim[0], 2 * pi);
        if (lim[1] < -pi) lim[1] = host_pymod(lim[1], 2 * pi);
        if (lim[0] > pi) lim[0] = host_pymod(lim[0], -2 * pi);
        if (lim[1] > pi) lim[1] = host_pymod(lim[1], -2 * pi);
        preferred_theta = -pi - preferred_theta;
    }
    *pref = preferred_theta;
}

// rsik_control_discrete (previous_rows == NULL: previous_sol_host, 2x7, per arm) and rsik_control_discrete_rows (previous_rows:
// one device row per goal, previous_sol_host NULL)
static int control_discrete_impl(rsik_ctx* ctx, const char* who, int64_t n, const double* const m12_soa[12], const uint8_t* arm,
                                 int arm_uniform, int nb_search_points, double preferred_theta, int constrained_mode,
                                 const double* previous_sol_host, const double* previous_rows, const double* current_joints,
                                 double orbita3d_max_angle, double* joints, uint8_t* reachable, uint8_t* state, uint8_t* emergency) {
    const std::string w(who);
    if (n < 0) return fail(ctx, RSIK_E_INVALID, w + ": n < 0");
    if (nb_search_points < 2) return fail(ctx, RSIK_E_INVALID, w + ": nb_search_points must be >= 2");
    if (constrained_mode != RSIK_MODE_UNCONSTRAINED && constrained_mode != RSIK_MODE_LOW_ELBOW)
        return fail(ctx, RSIK_E_INVALID, w + ": unknown constrained_mode");
    if (!previous_sol_host && !previous_rows) return fail(ctx, RSIK_E_INVALID, w + ": previous_sol_host is NULL");
    int rc = check_arms(ctx, arm, arm_uniform, who);
    if (rc != RSIK_OK) return rc;
    if (n == 0) return RSIK_OK;
    if (!m12_soa || !joints) return fail(ctx, RSIK_E_INVALID, w + ": m12_soa / joints is NULL");
    rsik::DiscreteArgs K;
    K.n = n;
    if ((rc = copy_cols(ctx, who, "m12_soa", "an m12_soa column", m12_soa, K.in, 12)) != RSIK_OK) return rc;
    K.arm = arm;
    K.nb = nb_search_points;
    int lg = 0;
    while ((1 << lg) < nb_search_points && lg < 6) lg++;
    K.log2p = lg;
    K.sweep_mode = ctx->options[RSIK_OPT_SWEEP_MODE];  // 0 unless a test / A-B run forces one of the two strategies
    K.euler_roundtrip = ctx->options[RSIK_OPT_EULER_ROUNDTRIP];
    // one round = every workgroup resident at once: 4 workgroups per compute unit (their LDS slabs)
    K.stagger = n <= (int64_t)ctx->compute_units * 4 * rsik::kDiscBlock ? 1 : 0;
    for (int slot = 0; slot < 2; slot++) {
        const int a = slot_arm(arm, arm_uniform, slot);
        control_limits(a, constrained_mode, preferred_theta, K.lim[slot], &K.pref[slot]);
        K.pref_cs[slot] = std::cos(K.pref[slot]);  // np.cos / np.sin of the reference (U:359-360), once per launch
        K.pref_sn[slot] = std::sin(K.pref[slot]);
        // The arc-end candidates of the per-lane search take |angle_diff(theta_k, preferred)| for a function of the wrapped
        // preferred angle.  For a huge preferred angle theta_k - preferred rounds to its ulp (0.125 at 1e15, everything from 2^53
        // on) and the reference's first strict minimum is decided by that staircase: such a launch evaluates every grid point,
        // in the reference's own arithmetic (the cooperative sweep).
        // (This overrides RSIK_OPT_SWEEP_MODE for such a launch, 2 included: the per-lane search is not the reference there.)
        if (!(std::fabs(K.pref[slot]) < rsik::kFarAngle)) K.sweep_mode = 1;
        if (previous_sol_host) {  // (the PREV_ROWS kernels read neither: prev_rows takes prev_sol's bytes, prev_cs / prev_sn stay unset)
            for (int k = 0; k < 7; k++) K.prev_sol[slot][k] = previous_sol_host[7 * a + k];
            for (int k = 0; k < 3; k++) {
                K.prev_cs[slot][k] = std::cos(K.prev_sol[slot][4 + k]);
                K.prev_sn[slot][k] = std::sin(K.prev_sol[slot][4 + k]);
            }
        }
    }
    bind_arms(ctx, arm, arm_uniform, K.arms);
    if (previous_rows) K.prev_rows = previous_rows;  // (shares its kernarg bytes with K.prev_sol)
    K.current_joints = current_joints;
    K.max_angle = orbita3d_max_angle;
    K.cos_max = std::cos(orbita3d_max_angle);
    K.sin_max = std::sin(orbita3d_max_angle);
    K.joints = joints; K.reachable = reachable; K.state = state; K.emergency = emergency;
    dim3 grid, block(rsik::kDiscBlock);
    if ((rc = launch_begin(ctx, n, &grid, who, rsik::kDiscBlock)) != RSIK_OK) return rc;
    with_bool(arm != nullptr, [&](auto MIXED) { with_bool(singularity_plane_binds(K.arms), [&](auto PLANE) { with_bool(previous_rows != nullptr, [&](auto PREV_ROWS) {
        hipLaunchKernelGGL((rsik::control_discrete_kernel<MIXED(), PLANE(), PREV_ROWS()>), grid, block, 0, ctx->stream, K); }); }); });
    return launch_end(ctx);
}

int rsik_control_discrete(rsik_ctx* ctx, int64_t n, const double* const m12_soa[12], const uint8_t* arm,
                          int arm_uniform, int nb_search_points, double preferred_theta, int constrained_mode,
                          const double* previous_sol_host, const double* current_joints, double orbita3d_max_angle,
                          double* joints, uint8_t* reachable, uint8_t* state, uint8_t* emergency) {
    if (!ctx) return RSIK_E_INVALID;
    return control_discrete_impl(ctx, "rsik_control_discrete", n, m12_soa, arm, arm_uniform, nb_search_points, preferred_theta,
                                 constrained_mode, previous_sol_host, nullptr, current_joints, orbita3d_max_angle, joints,
                                 reachable, state, emergency);
}

int rsik_control_discrete_rows(rsik_ctx* ctx, int64_t n, const double* const m12_soa[12], const uint8_t* arm,
                               int arm_uniform, int nb_search_points, double preferred_theta, int constrained_mode,
                               const double* previous_sol, const double* current_joints, double orbita3d_max_angle,
                               double* joints, uint8_t* reachable, uint8_t* state, uint8_t* emergency) {
    if (!ctx) return RSIK_E_INVALID;
    if (!previous_sol) return fail(ctx, RSIK_E_INVALID, "rsik_control_discrete_rows: previous_sol is NULL");
    return control_discrete_impl(ctx, "rsik_control_discrete_rows", n, m12_soa, arm, arm_uniform, nb_search_points,
                                 preferred_theta, constrained_mode, nullptr, previous_sol, current_joints, orbita3d_max_angle,
                                 joints, reachable, state, emergency);
}

// Arguments shared by the continuous-mode launches (validated once).
static int fill_continuous(rsik_ctx* ctx, const char* who, rsik::ContinuousArgs& K, int64_t n, const double* const m12_soa[12],
                           const double* const current_pose_m12_soa[12], const uint8_t* arm, int arm_uniform,
                           const uint8_t* timed_out, int first_timed_out, double preferred_theta,
                           const double* preferred_theta_self_host, int constrained_mode, double d_theta_max,
                           const double* current_joints, double orbita3d_max_angle, double* cont_state, double* joints,
                           uint8_t* reachable, uint8_t* state) {
    if (constrained_mode != RSIK_MODE_UNCONSTRAINED && constrained_mode != RSIK_MODE_LOW_ELBOW)
        return fail(ctx, RSIK_E_INVALID, std::string(who) + ": unknown constrained_mode");
    if (!preferred_theta_self_host) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": preferred_theta_self_host is NULL");
    int rc = check_arms(ctx, arm, arm_uniform, who);
    if (rc != RSIK_OK) return rc;
    if (!m12_soa || !cont_state || !joints) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": m12_soa / cont_state / joints is NULL");
    // include/rsik.h "Rows that are numbers, of any size": the continuous kernels take the sine and cosine of the preferred thetas
    // (the start theta of a timed-out row) and wrap them with the branch-free modulo of the serial phases, both written for
    // bounded angles, and the theta they would start is carried from step to step.  A finite preferred theta of magnitude >= 2^27
    // is refused here, before anything is launched or written (a NaN / an infinity propagates as IEEE arithmetic, as before).
    auto far_angle = [](double x) { return std::isfinite(x) && !(std::fabs(x) < rsik::kFarAngle); };
    bool far_pref = far_angle(preferred_theta);
    for (int slot = 0; slot < 2; slot++) far_pref = far_pref || far_angle(preferred_theta_self_host[slot_arm(arm, arm_uniform, slot)]);
    if (far_pref) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": |preferred_theta| / |preferred_theta_self| must be below 2^27 (134217728)");
    std::memset(&K, 0, sizeof K);
    K.n = n;
    K.first_timed_out = first_timed_out;
    for (int k = 0; k < 12; k++) {  // (the two tables column by column: which refusal wins is this loop's order, not copy_cols')
        if (!m12_soa[k]) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": an m12_soa column is NULL");
        K.in[k] = m12_soa[k];
        K.cur_pose[k] = current_pose_m12_soa ? current_pose_m12_soa[k] : nullptr;
        if (current_pose_m12_soa && !current_pose_m12_soa[k])
            return fail(ctx, RSIK_E_INVALID, std::string(who) + ": a current_pose column is NULL");
    }
    K.arm = arm;
    K.timed_out = timed_out;
    K.euler_roundtrip = ctx->options[RSIK_OPT_EULER_ROUNDTRIP];
    for (int slot = 0; slot < 2; slot++) {
        const int a = slot_arm(arm, arm_uniform, slot);
        control_limits(a, constrained_mode, preferred_theta, K.lim[slot], &K.pref_arg[slot]);
        K.pref_self[slot] = preferred_theta_self_host[a];
        K.pref_self_cs[slot] = std::cos(K.pref_self[slot]);  // np.cos / np.sin of the reference (U:359-360)
        K.pref_self_sn[slot] = std::sin(K.pref_self[slot]);
    }
    bind_arms(ctx, arm, arm_uniform, K.arms);
    K.d_theta_max = d_theta_max;
    K.current_joints = current_joints;
    K.max_angle = orbita3d_max_angle;
    K.cos_max = std::cos(orbita3d_max_angle);
    K.sin_max = std::sin(orbita3d_max_angle);
    K.st = cont_state; K.joints = joints; K.reachable = reachable; K.state = state;
    return RSIK_OK;
}

int rsik_control_continuous_step(rsik_ctx* ctx, int64_t n, const double* const m12_soa[12],
                                 const double* const current_pose_m12_soa[12], const uint8_t* arm, int arm_uniform,
                                 const uint8_t* timed_out, double preferred_theta, const double* preferred_theta_self_host,
                                 int constrained_mode, double d_theta_max, const double* current_joints,
                                 double orbita3d_max_angle, double* cont_state, double* joints, uint8_t* reachable,
                                 uint8_t* state) {
    if (!ctx) return RSIK_E_INVALID;
    if (n < 0) return fail(ctx, RSIK_E_INVALID, "rsik_control_continuous_step: n < 0");
    if (n == 0) return check_arms(ctx, arm, arm_uniform, "rsik_control_continuous_step");
    rsik::ContinuousArgs K;
    int rc = fill_continuous(ctx, "rsik_control_continuous_step", K, n, m12_soa, current_pose_m12_soa, arm, arm_uniform, timed_out,
                             0, preferred_theta, preferred_theta_self_host, constrained_mode, d_theta_max, current_joints,
                             orbita3d_max_angle, cont_state, joints, reachable, state);
    if (rc != RSIK_OK) return rc;
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, "rsik_control_continuous_step")) != RSIK_OK) return rc;
    launch_continuous_step(ctx, arm, K, grid, block);
    return launch_end(ctx);
}

#include "rsik_cont_run.hpp"

int rsik_matrix_to_pose(rsik_ctx* ctx, int64_t n, const double* const m12_soa[12], int identity_shortcut,
                        double* const pose_soa[6]) {
    if (!ctx) return RSIK_E_INVALID;
    if (n < 0) return fail(ctx, RSIK_E_INVALID, "rsik_matrix_to_pose: n < 0");
    if (n == 0) return RSIK_OK;
    if (!m12_soa || !pose_soa) return fail(ctx, RSIK_E_INVALID, "rsik_matrix_to_pose: NULL column table");
    rsik::MatrixToPoseArgs K;
    K.n = n;
    K.identity_shortcut = identity_shortcut;
    int rc = copy_cols(ctx, "rsik_matrix_to_pose", "m12_soa", "an m12_soa column", m12_soa, K.in, 12);
    if (rc != RSIK_OK) return rc;
    if ((rc = copy_cols(ctx, "rsik_matrix_to_pose", "pose_soa", "a pose_soa column", pose_soa, K.out, 6)) != RSIK_OK) return rc;
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, "rsik_matrix_to_pose")) != RSIK_OK) return rc;
    hipLaunchKernelGGL(rsik::matrix_to_pose_kernel, grid, block, 0, ctx->stream, K);
    return launch_end(ctx);
}

static int fill_state_args(rsik_ctx* ctx, rsik::StateArgs* K, int64_t n, const uint8_t* arm, int arm_uniform,
                           const char* who) {
    if (n < 0) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": n < 0");
    int rc = check_arms(ctx, arm, arm_uniform, who);
    if (rc != RSIK_OK) return rc;
    std::memset(K, 0, sizeof *K);
    K->n = n;
    K->arm = arm;
    bind_arms(ctx, arm, arm_uniform, K->arms);
    return RSIK_OK;
}

int rsik_reach_state(rsik_ctx* ctx, int64_t n, const double* const pose_soa[6], const uint8_t* arm, int arm_uniform,
                     int no_limits, double* solver_state, double* interval, uint8_t* reachable, uint8_t* state) {
    if (!ctx) return RSIK_E_INVALID;
    rsik::StateArgs K;
    int rc = fill_state_args(ctx, &K, n, arm, arm_uniform, "rsik_reach_state");
    if (rc != RSIK_OK) return rc;
    if (n == 0) return RSIK_OK;
    if (!pose_soa || !solver_state) return fail(ctx, RSIK_E_INVALID, "rsik_reach_state: pose_soa / solver_state is NULL");
    if ((rc = copy_cols(ctx, "rsik_reach_state", "pose_soa", "a pose_soa column", pose_soa, K.in, 6)) != RSIK_OK) return rc;
    K.no_limits = no_limits ? 1 : 0;
    K.solver_state = solver_state; K.interval = interval; K.reachable = reachable; K.state = state;
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, "rsik_reach_state")) != RSIK_OK) return rc;
    with_bool(arm != nullptr, [&](auto MIXED) { hipLaunchKernelGGL(rsik::reach_state_kernel<MIXED()>, grid, block, 0, ctx->stream, K); });
    return launch_end(ctx);
}

int rsik_joints_from_state(rsik_ctx* ctx, int64_t n, double* solver_state, const uint8_t* arm, int arm_uniform,
                           const double* theta, const double* previous_joints, double* joints, double* elbow) {
    if (!ctx) return RSIK_E_INVALID;
    rsik::StateArgs K;
    int rc = fill_state_args(ctx, &K, n, arm, arm_uniform, "rsik_joints_from_state");
    if (rc != RSIK_OK) return rc;
    if (n == 0) return RSIK_OK;
    if (!solver_state || !theta)  // joints may be NULL: the row's slots 24-30 carry them too
        return fail(ctx, RSIK_E_INVALID, "rsik_joints_from_state: solver_state / theta is NULL");
    K.solver_state = solver_state; K.theta = theta; K.prev = previous_joints; K.joints = joints; K.elbow = elbow;
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, "rsik_joints_from_state")) != RSIK_OK) return rc;
    with_bool(arm != nullptr, [&](auto MIXED) { hipLaunchKernelGGL(rsik::joints_state_kernel<MIXED()>, grid, block, 0, ctx->stream, K); });
    return launch_end(ctx);
}

int rsik_elbow_from_state(rsik_ctx* ctx, int64_t n, const double* solver_state, const double* theta, double* elbow) {
    if (!ctx) return RSIK_E_INVALID;
    if (n < 0) return fail(ctx, RSIK_E_INVALID, "rsik_elbow_from_state: n < 0");
    if (n == 0) return RSIK_OK;
    if (!solver_state || !theta || !elbow)
        return fail(ctx, RSIK_E_INVALID, "rsik_elbow_from_state: solver_state / theta / elbow is NULL");
    rsik::StateArgs K;
    std::memset(&K, 0, sizeof K);
    K.n = n;
    K.solver_state = const_cast<double*>(solver_state); K.theta = theta; K.elbow = elbow;
    dim3 grid, block(rsik::kBlock);
    int rc = launch_begin(ctx, n, &grid, "rsik_elbow_from_state");
    if (rc != RSIK_OK) return rc;
    hipLaunchKernelGGL(rsik::elbow_state_kernel, grid, block, 0, ctx->stream, K);
    return launch_end(ctx);
}

// utils.get_best_theta_to_current_joints for n rows (rsik_kernel_theta_from_joints.hpp)
static int fill_theta_from_joints(rsik_ctx* ctx, const char* who, rsik::ThetaFromJointsArgs& K, int64_t n, const uint8_t* arm,
                                  int arm_uniform, const double* preferred_theta_host) {
    int rc = check_arms(ctx, arm, arm_uniform, who);
    if (rc != RSIK_OK) return rc;
    std::memset(&K, 0, sizeof K);
    K.n = n;
    K.arm = arm;
    K.euler_roundtrip = ctx->options[RSIK_OPT_EULER_ROUNDTRIP];
    for (int slot = 0; slot < 2; slot++) K.pref[slot] = preferred_theta_host ? preferred_theta_host[slot_arm(arm, arm_uniform, slot)] : 0.0;
    bind_arms(ctx, arm, arm_uniform, K.arms);
    return RSIK_OK;
}

int rsik_theta_from_joints(rsik_ctx* ctx, int64_t n, int goal_kind, const double* const* goal_soa, const uint8_t* arm,
                           int arm_uniform, const double* current_joints, const double* preferred_theta_host, double* theta,
                           double* joints, double* bracket, double* distance, uint8_t* state) {
    const char* who = "rsik_theta_from_joints";
    if (!ctx) return RSIK_E_INVALID;
    if (n < 0) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": n < 0");
    if (goal_kind != RSIK_GOAL_POSE6 && goal_kind != RSIK_GOAL_M12)
        return fail(ctx, RSIK_E_INVALID, std::string(who) + ": goal_kind must be RSIK_GOAL_POSE6 or RSIK_GOAL_M12");
    rsik::ThetaFromJointsArgs K;
    int rc = fill_theta_from_joints(ctx, who, K, n, arm, arm_uniform, preferred_theta_host);
    if (rc != RSIK_OK) return rc;
    if (n == 0) return RSIK_OK;
    if (!goal_soa || !current_joints || !preferred_theta_host || !theta)
        return fail(ctx, RSIK_E_INVALID, std::string(who) + ": goal_soa / current_joints / preferred_theta_host / theta is NULL");
    const bool m12 = goal_kind == RSIK_GOAL_M12;
    if ((rc = copy_cols(ctx, who, "goal_soa", "a goal_soa column", goal_soa, K.goal, m12 ? 12 : 6)) != RSIK_OK) return rc;
    K.current_joints = current_joints; K.n_current = 7;
    K.theta = theta; K.joints = joints; K.bracket = bracket; K.distance = distance; K.state = state;
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, who)) != RSIK_OK) return rc;
    with_int3(launch_form(ctx, K.arms, arm), [&](auto FORM) { with_bool(m12, [&](auto M12) {
        hipLaunchKernelGGL((rsik::theta_from_joints_kernel<FORM(), M12()>), grid, block, 0, ctx->stream, K); }); });
    return launch_end(ctx);
}

int rsik_theta_from_joints_state(rsik_ctx* ctx, int64_t n, double* solver_state, const uint8_t* arm, int arm_uniform,
                                 const double* current_joints, int n_current, const double* preferred_theta_host,
                                 double* theta, double* bracket) {
    const char* who = "rsik_theta_from_joints_state";
    if (!ctx) return RSIK_E_INVALID;
    if (n < 0) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": n < 0");
    if (n_current != 7 && n_current != 14) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": n_current must be 7 or 14");
    rsik::ThetaFromJointsArgs K;
    int rc = fill_theta_from_joints(ctx, who, K, n, arm, arm_uniform, preferred_theta_host);
    if (rc != RSIK_OK) return rc;
    if (n == 0) return RSIK_OK;
    if (!solver_state || !current_joints || !preferred_theta_host || !theta)
        return fail(ctx, RSIK_E_INVALID, std::string(who) + ": solver_state / current_joints / preferred_theta_host / theta is NULL");
    K.solver_state = solver_state; K.current_joints = current_joints; K.n_current = n_current;
    K.theta = theta; K.bracket = bracket;
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, who)) != RSIK_OK) return rc;
    with_bool(arm != nullptr, [&](auto MIXED) { hipLaunchKernelGGL(rsik::theta_from_joints_state_kernel<MIXED()>, grid, block, 0, ctx->stream, K); });
    return launch_end(ctx);
}

int rsik_stage(rsik_ctx* ctx, int op, int64_t n, int arm, const double* in, int in_stride, double* out, int out_stride) {
    const char* who = "rsik_stage";
    if (!ctx) return RSIK_E_INVALID;
    // doubles a row takes and gives, by stage (include/rsik.h)
    static const int need_in[RSIK_STAGE_COUNT] = {6, 6, 6, 3, 17, 12, 10, 3, 2, 3, 4, 9, 14, 4, 10, 21, 18, 3, 19},
                     need_out[RSIK_STAGE_COUNT] = {5, 3, 7, 8, 3, 7, 7, 9, 1, 1, 2, 1, 7, 3, 8, 8, 3, 2, 4};
    // (stages 5 on read no arm constant: they do not need an arm to have been set)
    if (op < 0 || op >= RSIK_STAGE_COUNT) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": unknown stage");
    if (n < 0) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": n < 0");
    int rc = RSIK_OK;
    if (op <= RSIK_STAGE_CIRCLES_LINKED) {  // (the stages that read arm constants; the others run on a context no arm was uploaded to)
        if ((rc = check_arms(ctx, nullptr, arm, who)) != RSIK_OK) return rc;
    } else if (arm != RSIK_ARM_R && arm != RSIK_ARM_L) {
        return fail(ctx, RSIK_E_INVALID, std::string(who) + ": arm must be 0 (r) or 1 (l)");
    }
    if (n == 0) return RSIK_OK;
    if (!in || !out) return fail(ctx, RSIK_E_INVALID, std::string(who) + ": NULL buffer");
    if (in_stride < need_in[op] || out_stride < need_out[op])
        return fail(ctx, RSIK_E_INVALID, std::string(who) + ": stage " + std::to_string(op) + " reads " + std::to_string(need_in[op]) + " and writes " +
                    std::to_string(need_out[op]) + " doubles per row");
    rsik::StageArgs K;
    std::memset(&K, 0, sizeof K);
    K.n = n; K.op = op; K.in = in; K.out = out; K.in_stride = in_stride; K.out_stride = out_stride;
    if (ctx->have_arm[arm]) K.arms[0] = K.arms[1] = ctx->arms[arm];  // (else zeros: the utils helpers read none of it)
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, who)) != RSIK_OK) return rc;
    // (two kernels, not two forms of one: the limiter stages are compiled apart from is_reachable's)
    if (op >= RSIK_STAGE_TEND_TO_PREFERRED_THETA) hipLaunchKernelGGL(rsik::stage_limiter_kernel, grid, block, 0, ctx->stream, K);
    else hipLaunchKernelGGL(rsik::stage_kernel, grid, block, 0, ctx->stream, K);
    return launch_end(ctx);
}

static int launch_fk(rsik_ctx* ctx, rsik::FkArgs& K, int64_t n, const uint8_t* arm, int arm_uniform, const char* who) {
    int rc = check_arms(ctx, arm, arm_uniform, who);
    if (rc != RSIK_OK) return rc;
    K.n = n;
    K.arm = arm;
    bind_arms(ctx, arm, arm_uniform, K.arms);
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, who)) != RSIK_OK) return rc;
    with_bool(arm != nullptr, [&](auto MIXED) { hipLaunchKernelGGL(rsik::fk_kernel<MIXED()>, grid, block, 0, ctx->stream, K); });
    return launch_end(ctx);
}

int rsik_forward_kinematics(rsik_ctx* ctx, int64_t n, const double* joints, const uint8_t* arm, int arm_uniform,
                            double* position, double* rotation) {
    if (!ctx) return RSIK_E_INVALID;
    if (n < 0) return fail(ctx, RSIK_E_INVALID, "rsik_forward_kinematics: n < 0");
    if (n == 0) return RSIK_OK;
    if (!joints || (!position && !rotation))
        return fail(ctx, RSIK_E_INVALID, "rsik_forward_kinematics: joints or both outputs are NULL");
    rsik::FkArgs K;
    std::memset(&K, 0, sizeof K);
    K.joints = joints; K.pos = position; K.rot = rotation;
    return launch_fk(ctx, K, n, arm, arm_uniform, "rsik_forward_kinematics");
}

int rsik_fk_residual(rsik_ctx* ctx, int64_t n, int goal_kind, const double* const* goal_soa, const double* joints,
                     const uint8_t* arm, int arm_uniform, double* err) {
    if (!ctx) return RSIK_E_INVALID;
    if (n < 0) return fail(ctx, RSIK_E_INVALID, "rsik_fk_residual: n < 0");
    if (goal_kind != RSIK_GOAL_POSE6 && goal_kind != RSIK_GOAL_M12)
        return fail(ctx, RSIK_E_INVALID, "rsik_fk_residual: goal_kind must be RSIK_GOAL_POSE6 or RSIK_GOAL_M12");
    if (n == 0) return RSIK_OK;
    if (!goal_soa || !joints || !err) return fail(ctx, RSIK_E_INVALID, "rsik_fk_residual: goal_soa / joints / err is NULL");
    rsik::FkArgs K;
    std::memset(&K, 0, sizeof K);
    int rc = copy_cols(ctx, "rsik_fk_residual", "goal_soa", "a goal_soa column", goal_soa, K.goal, goal_kind == RSIK_GOAL_M12 ? 12 : 6);
    if (rc != RSIK_OK) return rc;
    K.goal_kind = goal_kind; K.joints = joints; K.err = err;
    return launch_fk(ctx, K, n, arm, arm_uniform, "rsik_fk_residual");
}

int rsik_jacobian(rsik_ctx* ctx, int64_t n, int64_t n_rep, const double* joints, const uint8_t* arm, int arm_uniform,
                  double* jacobian, double* null_vector, double* manipulability) {
    if (!ctx) return RSIK_E_INVALID;
    const char* who = "rsik_jacobian";
    if (n < 0) return fail(ctx, RSIK_E_INVALID, "rsik_jacobian: n < 0");
    if (n_rep < 1) return fail(ctx, RSIK_E_INVALID, "rsik_jacobian: n_rep < 1");
    if (n == 0) return RSIK_OK;
    if (!joints || (!jacobian && !null_vector && !manipulability))
        return fail(ctx, RSIK_E_INVALID, "rsik_jacobian: joints or all three outputs are NULL");
    int rc = check_arms(ctx, arm, arm_uniform, who);
    if (rc != RSIK_OK) return rc;
    rsik::JacobianArgs K;
    K.n = n;
    K.arm = arm;
    bind_arms(ctx, arm, arm_uniform, K.arms);
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, who)) != RSIK_OK) return rc;
    // the repetition is the grid's y, which holds 65535: more repetitions than that go in as many launches, each on its own slice
    for (int64_t rep0 = 0; rep0 < n_rep; rep0 += 65535) {
        const int64_t first = rep0 * n;
        grid.y = (unsigned)std::min<int64_t>(n_rep - rep0, 65535);
        K.joints = joints + first * 7;
        K.jacobian = jacobian ? jacobian + first * 42 : nullptr;
        K.null_vector = null_vector ? null_vector + first * 7 : nullptr;
        K.manipulability = manipulability ? manipulability + first : nullptr;
        with_bool(arm != nullptr, [&](auto MIXED) { with_bool(jacobian != nullptr, [&](auto WJ) { with_bool(null_vector != nullptr, [&](auto WN) {
            with_bool(manipulability != nullptr, [&](auto WM) {
                if constexpr (WJ() || WN() || WM())
                    hipLaunchKernelGGL((rsik::jacobian_kernel<MIXED(), WJ(), WN(), WM()>), grid, block, 0, ctx->stream, K); }); }); }); });
    }
    return launch_end(ctx);
}

int rsik_joint_rates(rsik_ctx* ctx, int64_t n, int64_t n_rep, const double* joints, const uint8_t* arm, int arm_uniform,
                     const double* twist, double damping_host, const double* damping, const double* bias_rates,
                     double* rates, double* achieved_twist) {
    if (!ctx) return RSIK_E_INVALID;
    const char* who = "rsik_joint_rates";
    if (n < 0) return fail(ctx, RSIK_E_INVALID, "rsik_joint_rates: n < 0");
    if (n_rep < 1) return fail(ctx, RSIK_E_INVALID, "rsik_joint_rates: n_rep < 1");
    if (n == 0) return RSIK_OK;
    if (!joints || !twist) return fail(ctx, RSIK_E_INVALID, "rsik_joint_rates: joints or twist is NULL");
    if (!rates && !achieved_twist) return fail(ctx, RSIK_E_INVALID, "rsik_joint_rates: both outputs are NULL");
    if (!damping && !rsik::damping_usable(damping_host))
        return fail(ctx, RSIK_E_INVALID, "rsik_joint_rates: damping_host must be finite and > 0 (its square a normal double)");
    int rc = check_arms(ctx, arm, arm_uniform, who);
    if (rc != RSIK_OK) return rc;
    rsik::JointRatesArgs K;
    K.n = n;
    K.arm = arm;
    K.damping_host = damping ? 0.0 : damping_host;
    bind_arms(ctx, arm, arm_uniform, K.arms);
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, who)) != RSIK_OK) return rc;
    // the repetition is the grid's y, as in rsik_jacobian: one launch per 65535 repetitions, each on its own slice
    for (int64_t rep0 = 0; rep0 < n_rep; rep0 += 65535) {
        const int64_t first = rep0 * n;
        grid.y = (unsigned)std::min<int64_t>(n_rep - rep0, 65535);
        K.joints = joints + first * 7;
        K.twist = twist + first * 6;
        K.damping = damping ? damping + first : nullptr;
        K.bias_rates = bias_rates ? bias_rates + first * 7 : nullptr;
        K.rates = rates ? rates + first * 7 : nullptr;
        K.achieved_twist = achieved_twist ? achieved_twist + first * 6 : nullptr;
        with_bool(arm != nullptr, [&](auto MIXED) { with_bool(bias_rates != nullptr, [&](auto BIAS) { with_bool(rates != nullptr, [&](auto WR) {
            with_bool(achieved_twist != nullptr, [&](auto WA) {
                if constexpr (WR() || WA())
                    hipLaunchKernelGGL((rsik::joint_rates_kernel<MIXED(), BIAS(), WR(), WA()>), grid, block, 0, ctx->stream, K); }); }); }); });
    }
    return launch_end(ctx);
}

int rsik_track(rsik_ctx* ctx, int64_t n, int64_t n_steps, const double* m12_steps, const uint8_t* arm, int arm_uniform,
               const double* start_joints, double dt, double kp, double ko, const double* feedforward_steps, double damping_host,
               const double* damping, const double* rest_joints, double rest_gain, const double* limits_host, double* joints_steps,
               double* rates_steps, double* err_steps, double* final_joints, double* final_err) {
    if (!ctx) return RSIK_E_INVALID;
    const char* who = "rsik_track";
    const auto gain_ok = [](double g) { return std::isfinite(g) && g >= 0.0; };
    if (n < 0) return fail(ctx, RSIK_E_INVALID, "rsik_track: n < 0");
    if (n_steps < 1 || n_steps > 65536) return fail(ctx, RSIK_E_INVALID, "rsik_track: n_steps must be 1 ... 65536");
    if (n == 0) return RSIK_OK;
    if (!m12_steps || !start_joints) return fail(ctx, RSIK_E_INVALID, "rsik_track: m12_steps or start_joints is NULL");
    if (!joints_steps && !rates_steps && !err_steps && !final_joints && !final_err)
        return fail(ctx, RSIK_E_INVALID, "rsik_track: all five outputs are NULL");
    if (!(std::isfinite(dt) && dt > 0.0)) return fail(ctx, RSIK_E_INVALID, "rsik_track: dt must be finite and > 0");
    if (!gain_ok(kp) || !gain_ok(ko)) return fail(ctx, RSIK_E_INVALID, "rsik_track: kp and ko must be finite and >= 0");
    if (rest_joints && !gain_ok(rest_gain)) return fail(ctx, RSIK_E_INVALID, "rsik_track: rest_gain must be finite and >= 0");
    if (!damping && !rsik::damping_usable(damping_host))
        return fail(ctx, RSIK_E_INVALID, "rsik_track: damping_host must be finite and > 0 (its square a normal double)");
    for (int k = 0; limits_host && k < 7; k++) {
        const double rate_max = limits_host[k], q_min = limits_host[7 + k], q_max = limits_host[14 + k];
        if (!(rate_max > 0.0) || !(q_min <= q_max))  // (a NaN fails both)
            return fail(ctx, RSIK_E_INVALID, "rsik_track: limits_host needs rate_max > 0 and q_min <= q_max, and no NaN");
    }
    int rc = check_arms(ctx, arm, arm_uniform, who);
    if (rc != RSIK_OK) return rc;
    rsik::TrackArgs K;
    std::memset(&K, 0, sizeof K);
    K.n = n; K.n_steps = n_steps; K.m12_steps = m12_steps; K.arm = arm; K.start_joints = start_joints;
    K.feedforward = feedforward_steps; K.damping = damping; K.rest_joints = rest_joints;
    K.joints_steps = joints_steps; K.rates_steps = rates_steps; K.err_steps = err_steps; K.final_joints = final_joints; K.final_err = final_err;
    K.damping_host = damping ? 0.0 : damping_host; K.dt = dt; K.kp = kp; K.ko = ko; K.rest_gain = rest_joints ? rest_gain : 0.0;
    if (limits_host) { fill7(K.rate_max, limits_host, 0.0); fill7(K.q_min, limits_host + 7, 0.0); fill7(K.q_max, limits_host + 14, 0.0); }
    bind_arms(ctx, arm, arm_uniform, K.arms);
    dim3 grid, block(rsik::kTrackBlock);
    if ((rc = launch_begin(ctx, n, &grid, who, rsik::kTrackBlock)) != RSIK_OK) return rc;
    with_bool(arm != nullptr, [&](auto MIXED) { with_bool(joints_steps != nullptr, [&](auto WJ) { with_bool(rates_steps != nullptr, [&](auto WR) {
        with_bool(err_steps != nullptr, [&](auto WE) { with_bool(feedforward_steps != nullptr, [&](auto FF) {
            with_bool(rest_joints != nullptr, [&](auto REST) { with_bool(limits_host != nullptr, [&](auto LIM) {
                constexpr int OUTS = (WJ() ? rsik::kTrackJoints : 0) | (WR() ? rsik::kTrackRates : 0) | (WE() ? rsik::kTrackErr : 0);
                hipLaunchKernelGGL((rsik::track_kernel<MIXED(), OUTS, FF(), REST(), LIM()>), grid, block, 0, ctx->stream, K); }); }); }); }); }); }); });
    return launch_end(ctx);
}

// What rsik_track_avoid and rsik_track_pair share: the checks on everything but the arms, in the order that is part of the ABI, and the
// argument block.  `rows` names the count in the messages ("n" or "n_pairs"; n is the number of rows either way); need_obstacle:
// rsik_track_avoid refuses a call without a static obstacle, rsik_track_pair always has the partner.  *launch is false where the call is
// valid and there is nothing to launch (n == 0).
static int check_track_avoid(rsik_ctx* ctx, const std::string& who, const char* rows, bool need_obstacle, int64_t n, int64_t n_steps,
                             const double* m12_steps, const double* start_joints, double dt, double kp, double ko, double damping_host,
                             const double* damping, const double* rest_joints, double rest_gain, const double* limits_host,
                             const double* link_radius_host, int n_spheres, const double* spheres, int n_capsules, const double* capsules,
                             double influence, double avoid_gain, bool any_output, const int32_t* nearest_steps, bool* launch) {
    const auto gain_ok = [](double g) { return std::isfinite(g) && g >= 0.0; };
    *launch = false;
    if (n < 0) return fail(ctx, RSIK_E_INVALID, who + ": " + rows + " < 0");
    if (n_steps < 1 || n_steps > 65536) return fail(ctx, RSIK_E_INVALID, who + ": n_steps must be 1 ... 65536");
    if (n_spheres < 0 || n_spheres > rsik::kAvoidMaxSpheres) return fail(ctx, RSIK_E_INVALID, who + ": n_spheres must be 0 ... 256");
    if (n_capsules < 0 || n_capsules > rsik::kAvoidMaxCapsules) return fail(ctx, RSIK_E_INVALID, who + ": n_capsules must be 0 ... 64");
    if (need_obstacle && n_spheres + n_capsules < 1) return fail(ctx, RSIK_E_INVALID, who + ": at least one obstacle (without obstacles: rsik_track)");
    for (int l = 0; link_radius_host && l < 3; l++)
        if (!gain_ok(link_radius_host[l])) return fail(ctx, RSIK_E_INVALID, who + ": every link radius must be finite and >= 0");
    if (!gain_ok(influence) || !gain_ok(avoid_gain))
        return fail(ctx, RSIK_E_INVALID, who + ": influence and avoid_gain must be finite and >= 0");
    if (n == 0) return RSIK_OK;
    if (!m12_steps || !start_joints) return fail(ctx, RSIK_E_INVALID, who + ": m12_steps or start_joints is NULL");
    if (!any_output) return fail(ctx, RSIK_E_INVALID, who + ": all eight outputs are NULL");
    if ((n_spheres > 0 && !spheres) || (n_capsules > 0 && !capsules))
        return fail(ctx, RSIK_E_INVALID, who + ": spheres or capsules is NULL with a count above 0");
    if (((uintptr_t)nearest_steps & 7) != 0) return fail(ctx, RSIK_E_INVALID, who + ": nearest_steps must be aligned to 8 bytes");
    if (!(std::isfinite(dt) && dt > 0.0)) return fail(ctx, RSIK_E_INVALID, who + ": dt must be finite and > 0");
    if (!gain_ok(kp) || !gain_ok(ko)) return fail(ctx, RSIK_E_INVALID, who + ": kp and ko must be finite and >= 0");
    if (rest_joints && !gain_ok(rest_gain)) return fail(ctx, RSIK_E_INVALID, who + ": rest_gain must be finite and >= 0");
    if (!damping && !rsik::damping_usable(damping_host))
        return fail(ctx, RSIK_E_INVALID, who + ": damping_host must be finite and > 0 (its square a normal double)");
    for (int k = 0; limits_host && k < 7; k++) {
        const double rate_max = limits_host[k], q_min = limits_host[7 + k], q_max = limits_host[14 + k];
        if (!(rate_max > 0.0) || !(q_min <= q_max))  // (a NaN fails both)
            return fail(ctx, RSIK_E_INVALID, who + ": limits_host needs rate_max > 0 and q_min <= q_max, and no NaN");
    }
    *launch = true;
    return RSIK_OK;
}
static void fill_track_avoid(rsik::TrackAvoidArgs& K, int64_t n, int64_t n_steps, const double* m12_steps, const uint8_t* arm,
                             const double* start_joints, double dt, double kp, double ko, const double* feedforward_steps,
                             double damping_host, const double* damping, const double* rest_joints, double rest_gain,
                             const double* limits_host, const double* link_radius_host, int n_spheres, const double* spheres,
                             int n_capsules, const double* capsules, double influence, double avoid_gain, double* joints_steps,
                             double* rates_steps, double* err_steps, double* clearance_steps, int32_t* nearest_steps,
                             double* final_joints, double* final_err, double* min_clearance) {
    std::memset(&K, 0, sizeof K);
    K.n = n; K.n_steps = n_steps; K.m12_steps = m12_steps; K.arm = arm; K.start_joints = start_joints;
    K.feedforward = feedforward_steps; K.damping = damping; K.rest_joints = rest_joints;
    K.spheres = spheres; K.capsules = capsules; K.n_spheres = n_spheres; K.n_capsules = n_capsules;
    K.joints_steps = joints_steps; K.rates_steps = rates_steps; K.err_steps = err_steps; K.clearance_steps = clearance_steps;
    K.nearest_steps = nearest_steps; K.final_joints = final_joints; K.final_err = final_err; K.min_clearance = min_clearance;
    K.damping_host = damping ? 0.0 : damping_host; K.dt = dt; K.kp = kp; K.ko = ko; K.rest_gain = rest_joints ? rest_gain : 0.0;
    K.influence = influence; K.avoid_gain = avoid_gain;
    for (int l = 0; l < 3; l++) K.link_radius[l] = link_radius_host ? link_radius_host[l] : 0.0;
    if (limits_host) { fill7(K.rate_max, limits_host, 0.0); fill7(K.q_min, limits_host + 7, 0.0); fill7(K.q_max, limits_host + 14, 0.0); }
}

int rsik_track_avoid(rsik_ctx* ctx, int64_t n, int64_t n_steps, const double* m12_steps, const uint8_t* arm, int arm_uniform,
                     const double* start_joints, double dt, double kp, double ko, const double* feedforward_steps, double damping_host,
                     const double* damping, const double* rest_joints, double rest_gain, const double* limits_host,
                     const double* link_radius_host, int n_spheres, const double* spheres, int n_capsules, const double* capsules,
                     double influence, double avoid_gain, double* joints_steps, double* rates_steps, double* err_steps,
                     double* clearance_steps, int32_t* nearest_steps, double* final_joints, double* final_err, double* min_clearance) {
    if (!ctx) return RSIK_E_INVALID;
    const char* who = "rsik_track_avoid";
    const bool any_output = joints_steps || rates_steps || err_steps || clearance_steps || nearest_steps || final_joints || final_err || min_clearance;
    bool launch;
    int rc = check_track_avoid(ctx, who, "n", true, n, n_steps, m12_steps, start_joints, dt, kp, ko, damping_host, damping, rest_joints,
                               rest_gain, limits_host, link_radius_host, n_spheres, spheres, n_capsules, capsules, influence,
                               avoid_gain, any_output, nearest_steps, &launch);
    if (rc != RSIK_OK || !launch) return rc;
    if ((rc = check_arms(ctx, arm, arm_uniform, who)) != RSIK_OK) return rc;
    rsik::TrackAvoidArgs K;
    fill_track_avoid(K, n, n_steps, m12_steps, arm, start_joints, dt, kp, ko, feedforward_steps, damping_host, damping, rest_joints,
                     rest_gain, limits_host, link_radius_host, n_spheres, spheres, n_capsules, capsules, influence, avoid_gain,
                     joints_steps, rates_steps, err_steps, clearance_steps, nearest_steps, final_joints, final_err, min_clearance);
    bind_arms(ctx, arm, arm_uniform, K.arms);
    dim3 grid, block(rsik::kTrackBlock);
    if ((rc = launch_begin(ctx, n, &grid, who, rsik::kTrackBlock)) != RSIK_OK) return rc;
    with_bool(arm != nullptr, [&](auto MIXED) { with_bool(feedforward_steps != nullptr, [&](auto FF) { with_bool(limits_host != nullptr, [&](auto LIM) {
        hipLaunchKernelGGL((rsik::track_avoid_kernel<MIXED(), FF(), LIM()>), grid, block, 0, ctx->stream, K); }); }); });
    return launch_end(ctx);
}

int rsik_track_pair(rsik_ctx* ctx, int64_t n_pairs, int64_t n_steps, const double* m12_steps, const double* start_joints, double dt,
                    double kp, double ko, const double* feedforward_steps, double damping_host, const double* damping,
                    const double* rest_joints, double rest_gain, const double* limits_host, const double* link_radius_host,
                    int n_spheres, const double* spheres, int n_capsules, const double* capsules, double influence, double avoid_gain,
                    double* joints_steps, double* rates_steps, double* err_steps, double* clearance_steps, int32_t* nearest_steps,
                    double* final_joints, double* final_err, double* min_clearance) {
    if (!ctx) return RSIK_E_INVALID;
    const char* who = "rsik_track_pair";
    if (n_pairs > 0x3fffffffffffffffLL) return fail(ctx, RSIK_E_INVALID, "rsik_track_pair: n too large for one launch");
    const int64_t n = n_pairs < 0 ? -1 : 2 * n_pairs;  // rows: 2i the right arm of robot i, 2i + 1 its left arm
    const bool any_output = joints_steps || rates_steps || err_steps || clearance_steps || nearest_steps || final_joints || final_err || min_clearance;
    bool launch;
    int rc = check_track_avoid(ctx, who, "n_pairs", false, n, n_steps, m12_steps, start_joints, dt, kp, ko, damping_host, damping,
                               rest_joints, rest_gain, limits_host, link_radius_host, n_spheres, spheres, n_capsules, capsules,
                               influence, avoid_gain, any_output, nearest_steps, &launch);
    if (rc != RSIK_OK || !launch) return rc;
    if (!ctx->have_arm[RSIK_ARM_R] || !ctx->have_arm[RSIK_ARM_L])
        return fail(ctx, RSIK_E_NOT_SET, "rsik_track_pair: both arms' constants are needed (rsik_set_arm)");
    rsik::TrackAvoidArgs K;  // (K.arm stays NULL: the arm of a row is its parity)
    fill_track_avoid(K, n, n_steps, m12_steps, nullptr, start_joints, dt, kp, ko, feedforward_steps, damping_host, damping, rest_joints,
                     rest_gain, limits_host, link_radius_host, n_spheres, spheres, n_capsules, capsules, influence, avoid_gain,
                     joints_steps, rates_steps, err_steps, clearance_steps, nearest_steps, final_joints, final_err, min_clearance);
    K.arms[0] = ctx->arms[RSIK_ARM_R]; K.arms[1] = ctx->arms[RSIK_ARM_L];
    dim3 grid, block(rsik::kTrackBlock);
    if ((rc = launch_begin(ctx, n, &grid, who, rsik::kTrackBlock)) != RSIK_OK) return rc;
    with_bool(feedforward_steps != nullptr, [&](auto FF) { with_bool(limits_host != nullptr, [&](auto LIM) {
        hipLaunchKernelGGL((rsik::track_pair_kernel<FF(), LIM()>), grid, block, 0, ctx->stream, K); }); });
    return launch_end(ctx);
}

int rsik_clearance(rsik_ctx* ctx, int64_t n, int64_t n_rep, const double* joints, const uint8_t* arm, int arm_uniform,
                   const double* link_radius_host, int n_spheres, const double* spheres, int n_capsules, const double* capsules,
                   double* clearance, int32_t* nearest, double* gradient, double* witness, double* link_points) {
    if (!ctx) return RSIK_E_INVALID;
    const char* who = "rsik_clearance";
    if (n < 0) return fail(ctx, RSIK_E_INVALID, "rsik_clearance: n < 0");
    if (n_rep < 1) return fail(ctx, RSIK_E_INVALID, "rsik_clearance: n_rep < 1");
    if (n_spheres < 0 || n_spheres > rsik::kClrMaxSpheres) return fail(ctx, RSIK_E_INVALID, "rsik_clearance: n_spheres must be 0 ... 4096");
    if (n_capsules < 0 || n_capsules > rsik::kClrMaxCapsules) return fail(ctx, RSIK_E_INVALID, "rsik_clearance: n_capsules must be 0 ... 256");
    if (n_spheres + n_capsules < 1) return fail(ctx, RSIK_E_INVALID, "rsik_clearance: at least one obstacle");
    for (int l = 0; link_radius_host && l < 3; l++)
        if (!(std::isfinite(link_radius_host[l]) && link_radius_host[l] >= 0.0))
            return fail(ctx, RSIK_E_INVALID, "rsik_clearance: every link radius must be finite and >= 0");
    if (n == 0) return RSIK_OK;
    if (!joints || (!clearance && !nearest && !gradient && !witness && !link_points))
        return fail(ctx, RSIK_E_INVALID, "rsik_clearance: joints or all five outputs are NULL");
    if ((n_spheres > 0 && !spheres) || (n_capsules > 0 && !capsules))
        return fail(ctx, RSIK_E_INVALID, "rsik_clearance: spheres or capsules is NULL with a count above 0");
    if (((uintptr_t)nearest & 7) != 0) return fail(ctx, RSIK_E_INVALID, "rsik_clearance: nearest must be aligned to 8 bytes");
    int rc = check_arms(ctx, arm, arm_uniform, who);
    if (rc != RSIK_OK) return rc;
    rsik::ClearanceArgs K;
    std::memset(&K, 0, sizeof K);
    K.n = n;
    K.arm = arm;
    K.spheres = spheres; K.capsules = capsules; K.n_spheres = n_spheres; K.n_capsules = n_capsules;
    for (int l = 0; l < 3; l++) K.link_radius[l] = link_radius_host ? link_radius_host[l] : 0.0;
    bind_arms(ctx, arm, arm_uniform, K.arms);
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, n, &grid, who)) != RSIK_OK) return rc;
    // the repetition is the grid's y, as in rsik_jacobian: one launch per 65535 repetitions, each on its own slice
    for (int64_t rep0 = 0; rep0 < n_rep; rep0 += 65535) {
        const int64_t first = rep0 * n;
        grid.y = (unsigned)std::min<int64_t>(n_rep - rep0, 65535);
        K.joints = joints + first * 7;
        K.clearance = clearance ? clearance + first : nullptr;
        K.nearest = nearest ? nearest + first * 2 : nullptr;
        K.gradient = gradient ? gradient + first * 7 : nullptr;
        K.witness = witness ? witness + first * 6 : nullptr;
        K.link_points = link_points ? link_points + first * 12 : nullptr;
        with_bool(arm != nullptr, [&](auto MIXED) { with_bool(gradient != nullptr || witness != nullptr, [&](auto WIT) {
            hipLaunchKernelGGL((rsik::clearance_kernel<MIXED(), WIT()>), grid, block, 0, ctx->stream, K); }); });
    }
    return launch_end(ctx);
}

// rsik_clearance_edges' workspace: what the per-path fold reads of every edge — its clearance, its bound (doubles) and its sub-step
// (int32), [n_steps][n] each, the total a multiple of 8 bytes
static bool clearance_edges_workspace_bytes(int64_t n, int64_t n_steps, size_t* bytes) {
    if (n < 0 || n_steps < 1 || n_steps > 65536) return false;
    const unsigned __int128 b = (unsigned __int128)n * (unsigned __int128)n_steps * 20u + 4u;
    if (b > (unsigned __int128)(SIZE_MAX / 2)) return false;
    *bytes = (size_t)b & ~(size_t)7;
    return true;
}
int rsik_clearance_edges_workspace_bytes(int64_t n, int64_t n_steps, size_t* bytes) {
    if (!bytes || !clearance_edges_workspace_bytes(n, n_steps, bytes)) return RSIK_E_INVALID;
    return RSIK_OK;
}

// rsik_clearance_edges: the clearance along the motion between a path's waypoints (rsik_kernel_clearance_edges.hpp).  The scene's
// limits and checks are rsik_solve_path_clear's, the arm checks rsik_jacobian's.
int rsik_clearance_edges(rsik_ctx* ctx, int64_t n, int64_t n_steps, const double* joints, const uint8_t* arm, int arm_uniform,
                         const double* start_joints, int n_sub,
                         const double* link_radius_host, int n_spheres, const double* spheres, int n_capsules, const double* capsules,
                         double min_clearance, void* workspace, size_t workspace_bytes,
                         double* edge_clearance, int32_t* edge_sub, int32_t* edge_nearest, double* edge_bound,
                         double* path_clearance, int32_t* path_edge, double* path_bound, int32_t* n_below, int32_t* first_below) {
    if (!ctx) return RSIK_E_INVALID;
    const char* who = "rsik_clearance_edges";
    const std::string w(who);
    if (n < 0) return fail(ctx, RSIK_E_INVALID, w + ": n < 0");
    if (n_steps < 1 || n_steps > 65536) return fail(ctx, RSIK_E_INVALID, w + ": n_steps must be 1 ... 65536");
    if (n_sub < 1 || n_sub > 256) return fail(ctx, RSIK_E_INVALID, w + ": n_sub must be 1 ... 256");
    if (n_spheres < 0 || n_spheres > rsik::kAvoidMaxSpheres) return fail(ctx, RSIK_E_INVALID, w + ": n_spheres must be 0 ... 256");
    if (n_capsules < 0 || n_capsules > rsik::kAvoidMaxCapsules) return fail(ctx, RSIK_E_INVALID, w + ": n_capsules must be 0 ... 64");
    if (n_spheres + n_capsules < 1) return fail(ctx, RSIK_E_INVALID, w + ": at least one obstacle");
    for (int l = 0; link_radius_host && l < 3; l++)
        if (!(std::isfinite(link_radius_host[l]) && link_radius_host[l] >= 0.0))
            return fail(ctx, RSIK_E_INVALID, w + ": every link radius must be finite and >= 0");
    if (!(min_clearance < __builtin_inf()))  // (a NaN fails it too)
        return fail(ctx, RSIK_E_INVALID, w + ": min_clearance must be finite or -infinity");
    if (n == 0) return RSIK_OK;
    const bool any_edge = edge_clearance || edge_sub || edge_nearest || edge_bound;
    const bool any_path = path_clearance || path_edge || path_bound || n_below || first_below;
    if (!joints || !(any_edge || any_path)) return fail(ctx, RSIK_E_INVALID, w + ": joints or all nine outputs are NULL");
    if ((n_spheres > 0 && !spheres) || (n_capsules > 0 && !capsules))
        return fail(ctx, RSIK_E_INVALID, w + ": spheres or capsules is NULL with a count above 0");
    if ((((uintptr_t)edge_nearest | (uintptr_t)path_edge) & 7) != 0)
        return fail(ctx, RSIK_E_INVALID, w + ": edge_nearest and path_edge must be aligned to 8 bytes");
    size_t need = 0;
    if (!clearance_edges_workspace_bytes(n, n_steps, &need)) return fail(ctx, RSIK_E_INVALID, w + ": n * n_steps too large");
    if (any_path && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7) != 0))
        return fail(ctx, RSIK_E_INVALID, w + ": a path output needs a workspace of rsik_clearance_edges_workspace_bytes, aligned to 8 bytes");
    int rc = check_arms(ctx, arm, arm_uniform, who);
    if (rc != RSIK_OK) return rc;
    rsik::ClearanceEdgesArgs K;
    std::memset(&K, 0, sizeof K);
    const int64_t edges = n * n_steps;
    K.n = n; K.n_steps = n_steps; K.joints = joints; K.arm = arm; K.start = start_joints;
    K.spheres = spheres; K.capsules = capsules; K.n_spheres = n_spheres; K.n_capsules = n_capsules;
    K.edge_clearance = edge_clearance; K.edge_sub = edge_sub; K.edge_nearest = edge_nearest; K.edge_bound = edge_bound;
    if (any_path) {
        K.ws_clearance = static_cast<double*>(workspace);
        K.ws_bound = K.ws_clearance + edges;
        K.ws_sub = reinterpret_cast<int32_t*>(K.ws_bound + edges);
    }
    K.path_clearance = path_clearance; K.path_edge = path_edge; K.path_bound = path_bound; K.n_below = n_below; K.first_below = first_below;
    K.n_sub = n_sub; K.min_clearance = min_clearance;
    for (int l = 0; l < 3; l++) K.link_radius[l] = link_radius_host ? link_radius_host[l] : 0.0;
    bind_arms(ctx, arm, arm_uniform, K.arms);
    for (int slot = 0; slot < 2; slot++) {  // how far one radian of a joint can move a point of the arm's axis (rsik.h)
        const double* c = K.arms[slot].v;
        const double tip = std::sqrt(c[RSIK_C_TIPL] * c[RSIK_C_TIPL] + c[RSIK_C_TIPL + 1] * c[RSIK_C_TIPL + 1] + c[RSIK_C_TIPL + 2] * c[RSIK_C_TIPL + 2]);
        K.sweep[slot][0] = c[RSIK_C_UPPER_ARM] + c[RSIK_C_FOREARM] + tip;
        K.sweep[slot][1] = c[RSIK_C_FOREARM] + tip;
        K.sweep[slot][2] = tip;
    }
    // Lanes per edge: as many as keep the launch within what is resident at once (one round of workgroups, no tail), and no more
    // than an edge has samples; one lane per edge beyond that, the workgroups striding over the edges.  The fold: as many lanes per
    // path as it has waypoints, while the paths alone do not fill the device.
    const int64_t resident = (int64_t)ctx->compute_units * rsik::kEdgeBlocksPerCu;
    int lanes = 1;
    while (lanes < 64 && lanes < n_sub + 1 && edges * lanes * 2 <= resident * rsik::kBlock) lanes *= 2;
    K.lanes = lanes;
    int fold_lanes = 1;
    while (fold_lanes < 64 && fold_lanes < n_steps && n * fold_lanes < resident * rsik::kBlock) fold_lanes *= 2;
    K.fold_lanes = fold_lanes;
    const int64_t groups = rsik::kBlock / lanes;
    const int64_t blocks = std::min<int64_t>((edges + groups - 1) / groups, resident);
    dim3 grid, block(rsik::kBlock);
    if ((rc = launch_begin(ctx, blocks * rsik::kBlock, &grid, who)) != RSIK_OK) return rc;
    with_bool(arm != nullptr, [&](auto MIXED) {
        hipLaunchKernelGGL((rsik::clearance_edges_kernel<MIXED()>), grid, block, 0, ctx->stream, K); });
    if (any_path) {
        if (n > INT64_MAX / 64) return fail(ctx, RSIK_E_INVALID, w + ": n too large for one launch");
        if ((rc = launch_dims(ctx, n * fold_lanes, &grid, who)) != RSIK_OK) return rc;
        hipLaunchKernelGGL(rsik::clearance_edges_fold_kernel, grid, block, 0, ctx->stream, K);
    }
    return launch_end(ctx);
}

int rsik_debug_math(rsik_ctx* ctx, int op, int64_t n, const double* a, const double* b, double* out0, double* out1) {
    if (!ctx) return RSIK_E_INVALID;
    if (n < 0 || op < 0 || op > 19) return fail(ctx, RSIK_E_INVALID, "rsik_debug_math: bad op or n");
    if (n == 0) return RSIK_OK;
    if (!a || !out0 || ((op == 3 || op == 5 || op == 6 || op == 7 || (op >= 9 && op <= 16)) && !b))
        return fail(ctx, RSIK_E_INVALID, "rsik_debug_math: NULL operand");
    RSIK_HIP(ctx, hipSetDevice(ctx->device));
    dim3 grid, block(rsik::kBlock);
    if (op == 8) {  // clock monitor: n waves, one per 64-thread workgroup so that they spread over the chip
        if (!out1 || n > 4096) return fail(ctx, RSIK_E_INVALID, "rsik_debug_math: op 8 needs out1 and n <= 4096 waves");
        hipLaunchKernelGGL(rsik::clock_monitor_kernel, dim3((unsigned)n), dim3(64), 0, ctx->stream, a, n, out0, out1);
        return launch_end(ctx);
    }
    if (op >= 9) {  // a lock-step width: one thread per group of N elements
        static const int kWidth[11] = {2, 3, 4, 7, 2, 3, 4, 7, 2, 3, 4};
        const int N = kWidth[op - 9];
        int rc = launch_dims(ctx, (n + N - 1) / N, &grid, "rsik_debug_math");
        if (rc != RSIK_OK) return rc;
        auto go = [&](auto FN, auto W) {
            hipLaunchKernelGGL((rsik::debug_math_width_kernel<FN(), W()>), grid, block, 0, ctx->stream, n, a, b, out0, out1);
        };
        auto width = [&](auto FN) {
            using std::integral_constant;
            if (N == 2) go(FN, integral_constant<int, 2>()); else if (N == 3) go(FN, integral_constant<int, 3>());
            else if (N == 4) go(FN, integral_constant<int, 4>());
            else if constexpr (FN() != 2) go(FN, integral_constant<int, 7>());
        };
        with_int3(op < 13 ? 0 : op < 17 ? 1 : 2, width);
        return launch_end(ctx);
    }
    int rc = launch_dims(ctx, n, &grid, "rsik_debug_math");  // (not launch_begin: the device is set above, ahead of op 8's own refusal)
    if (rc != RSIK_OK) return rc;
    hipLaunchKernelGGL(rsik::debug_math_kernel, grid, block, 0, ctx->stream, op, n, a, b, out0, out1);
    return launch_end(ctx);
}

#include "rsik_comm.hpp"

}  // extern "C"
