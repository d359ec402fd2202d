/*
 * rsik.h — C ABI of the MI355X-native batched analytic IK solver for the Reachy 2 arms.
 *
 * This is the drop-in boundary for ONE path of pollen-robotics/reachy2_symbolic_ik:
 *   SymbolicIK.is_reachable + theta_to_joints_func (= SymbolicIK.get_joints)
 *   ControlIK.symbolic_inverse_kinematics, control_type "discrete" (and "continuous" as state-carrying steps)
 *
 * The reference has no FFI: its boundary is the Python API of two classes
 * (src/reachy2_symbolic_ik/symbolic_ik.py:25-863, control_ik.py:27-497).  Each entry point below
 * cites the reference interface it replaces.  Plain C: pointers and sizes only, no C++/torch types.
 *
 * Conventions
 *   - Every function returns an int status: RSIK_OK (0) or a negative RSIK_E_* code;
 *     rsik_last_error(ctx) gives the message.  Unreachable poses are DATA (reachable/state
 *     arrays), never errors — the reference returns (False, [], None, state) rather than raising
 *     (symbolic_ik.py:130-132,161,263).
 *   - All `const double*` / `double*` / `uint8_t*` batch arguments are DEVICE pointers (HBM) owned
 *     by the caller unless the name ends in `_host`.  The library never frees or retains them.
 *   - Work is enqueued on the context's HIP stream (rsik_set_stream) and is asynchronous;
 *     rsik_sync waits for it.
 *   - Streams: calls of one context may be issued on different streams (rsik_set_stream between them).  The continuous run keeps
 *     a workspace, dependency words and side streams in the context: a run issued on another stream than the run before it
 *     waits for that run's end first.  hipGraphs recorded from ONE context's continuous runs share that workspace: replay
 *     them one at a time (or record them from different contexts).
 *   - Threads: a context is NOT thread-safe (it holds the stream, the arm constants, the options and the
 *     continuous pipeline's workspace that the next call uses; the reference's objects are not re-entrant either,
 *     symbolic_ik.py:143-144,185).  Use it from one thread at a time; several contexts — one per thread, per stream or
 *     per GPU — are independent and may be used concurrently.
 *   - Angles in radians, lengths in metres, everything IEEE float64.
 *   - Rows of unreachable poses in joints / interval / elbow are filled with NaN.
 */
#ifndef RSIK_H
#define RSIK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSIK_ABI_VERSION 8

/* ---- status codes ---- */
#define RSIK_OK 0
#define RSIK_E_INVALID (-1)   /* bad argument (null pointer, bad enum, n < 0 ...) */
#define RSIK_E_NO_DEVICE (-2) /* no usable HIP device / device id out of range */
#define RSIK_E_HIP (-3)       /* a HIP runtime call failed; see rsik_last_error */
#define RSIK_E_NOT_SET (-4)   /* arm constants were not uploaded for an arm the call needs */

/* ---- per-pose state codes (uint8); strings are the reference's own ---- */
#define RSIK_STATE_REACHABLE 0           /* "reachable"                         symbolic_ik.py:234 */
#define RSIK_STATE_POSE_OUT_OF_REACH 1   /* "Pose out of reach"                 symbolic_ik.py:300 */
#define RSIK_STATE_BACKWARD_POSE 2       /* "Backward pose"                     symbolic_ik.py:306 */
#define RSIK_STATE_WRIST_OUT_OF_RANGE 3  /* "wrist out of range"                symbolic_ik.py:159 */
#define RSIK_STATE_LIMITED_BY_WRIST 4    /* "limited by wrist"                  symbolic_ik.py:262 */
#define RSIK_STATE_SHOULD_NOT_HAPPEN 5   /* "out of reach - should not happen"  symbolic_ik.py:281 */
#define RSIK_STATE_LIMITED_BY_SHOULDER 6 /* "limited by shoulder"               control_ik.py:363,452 */
#define RSIK_STATE_EMPTY 7               /* ""  (continuous mode, reachable)    control_ik.py:297 */
#define RSIK_STATE_EMERGENCY 8           /* emergency stop latched              control_ik.py:205-210 */
#define RSIK_STATE_NOT_REACHABLE_NO_LIMITS 9 /* continuous mode: is_reachable_no_limits failed, where the reference raises
                                              * RuntimeError("Pose not reachable in symbolic IK. ...") control_ik.py:385-387.
                                              * Joints NaN, trajectory state untouched.  Needs projection_margin <= 0. */
#define RSIK_STATE_INVALID_INPUT 10       /* the row's goal (pose or matrix) holds a NaN or an infinity: see "Rows that are not
                                          * numbers" below.  Where the reference raises numpy.linalg.LinAlgError
                                          * (symbolic_ik.py:580, reached through the comparisons of :284-307, which are all
                                          * false for a NaN) or ValueError (scipy's Rotation.from_matrix, control_ik.py:215).
                                          * Also a goal matrix of finite entries whose rotation block has a determinant <= 0:
                                          * "Goal matrices that are not rotations" below. */

/* ---- Rows that are not numbers ----
 * A batch is data: a row with a NaN or an infinity in it is answered in that row, never with an error code, never by stalling,
 * and it changes nothing in any other row — every other row's outputs (and, in the continuous entry points, its trajectory
 * state) are bit for bit those of a run in which the bad row held an ordinary goal.
 *
 *  the goal — the six pose entries of rsik_solve / rsik_reach_state, the twelve matrix entries (rotation and translation) of
 *  rsik_control_discrete / rsik_control_continuous_step / rsik_control_continuous_run — holds a NaN or +-infinity:
 *      state RSIK_STATE_INVALID_INPUT, reachable 0, joints / elbow / interval NaN, emergency 0; rsik_reach_state leaves the
 *      solver-state row's geometry as it was.  (The reference raises for a NaN anywhere and for an infinite angle; for an
 *      infinite POSITION its is_reachable returns "Pose out of reach" / "Backward pose" with a projected pose that is itself
 *      NaN, symbolic_ik.py:292-307, and the control entry points raise on it a few lines later: one code for all of them.)
 *      Continuous mode, a step with such a goal: the latch comes first as always (a latched trajectory reports
 *      RSIK_STATE_EMERGENCY and previous_sol); otherwise the step reports the code and NaN joints, previous_sol / init / the
 *      latch stay as they were — the next good step is judged against the last good one — and previous_theta takes the step
 *      of a search that found nothing (utils.py:252-264 with goal = previous_theta, then limit_theta_to_interval: it stays
 *      where it is once inside the control interval).  The start-up branch of a timed-out step (control_ik.py:296-325) does
 *      not read the goal and runs before this.
 *  anything else that is not a number — theta_in, previous_joints, current_joints, current_pose, a row of cont_state or of a
 *  solver state: IEEE arithmetic as the reference would do it: the outputs of THAT row which depend on the value are NaN or
 *  what comparisons that are all false select (a NaN never trips an emergency stop, a NaN previous_theta stays NaN); the state
 *  code is one of the codes above.  A poisoned cont_state row stays poisoned until the caller re-initialises it (timed_out).
 *
 * Rows that ARE numbers, of any size.  Every finite double is a value, as in the reference (whose libm reduces any angle by pi
 * exactly): the Euler angles of a pose goal, theta_in and the theta grids (RSIK_THETA_EXPLICIT and a fraction that leaves
 * [0, 1]), the theta of rsik_joints_from_state / rsik_elbow_from_state, the preferred_theta of rsik_theta_from_joints and of
 * rsik_control_discrete(_rows), and previous joints read at an exact singularity may be wound up to DBL_MAX: an angle of
 * magnitude >= 2^27 is first reduced to the angle of [-pi, pi] it is congruent to (a rare, wave-skipped branch; a few 1e-16
 * rad), and the row is answered like its reduced twin — flags, states and the projected bit exactly, numbers to 1e-9.  Outputs
 * that echo an angle (theta of the sampling entry points, the shoulder pitch kept at a singularity, theta == preferred_theta)
 * return it as it came.  A position may be anything up to DBL_MAX and down to the smallest denormal: where the squared distance
 * from the shoulder overflows (beyond 1.34e154) the reference's norm is infinite, its direction zero and the projected goal the
 * shoulder itself, and so it is here ("Backward pose" on the default arms).  tests/test_gpu_far_inputs.py, G22.
 * The CONTINUOUS entry points refuse a finite preferred_theta / preferred_theta_self of magnitude >= 2^27 with RSIK_E_INVALID,
 * before anything is launched or written: their serial phases wrap angles with a modulo written for bounded values, and a
 * wrong start theta would be carried from step to step.  Below the bound they answer as the reference does.  Not covered:
 * a caller-written previous_theta in a cont_state row (the library itself keeps it inside the control interval; it is
 * assumed below 2^27 in magnitude).
 *
 * Goal matrices that are not rotations.  The reference converts the 3x3 block of a goal matrix with SciPy's
 * Rotation.from_matrix(...).as_euler("xyz") (utils.py:84-90; rule and SVD as in SciPy 1.15), and so does every entry point that
 * takes a matrix (rsik_matrix_to_pose, rsik_control_discrete(_rows), rsik_control_continuous_step / _run, rsik_theta_from_joints)
 * under RSIK_EULER_AUTO and RSIK_EULER_ALWAYS:
 *  - determinant <= 0 (a reflection such as a flipped axis, a singular block, the zero block): SciPy raises ValueError
 *    ("Non-positive determinant (left-handed or null coordinate frame)") before it looks at anything else.  rsik_matrix_to_pose
 *    gives NaN angles and passes the position through; the other entry points answer the row exactly as "Rows that are not
 *    numbers" says for a goal that holds a NaN — RSIK_STATE_INVALID_INPUT, reachable 0, NaN outputs, emergency 0, in continuous
 *    mode previous_sol / init / the latch untouched — and no other row changes.  The sign is that of row 2 . (row 0 x row 1) in
 *    binary64, tested also where the block's Gramian is the identity (a reflection's is).  The scalar Python drop-ins raise
 *    that ValueError.
 *  - determinant > 0: the block stands for the nearest rotation, the orthogonal polar factor U V^T of its SVD, whatever its scale
 *    or shear (SciPy takes a block whose Gramian is np.isclose to the identity as it is; so does the conversion here).  Range:
 *    no entry larger than 1e100 in magnitude and every singular value in [1e-100, 1e100], so that no product of three entries
 *    overflows and no determinant vanishes; within it the angles are SciPy's to max(1e-12, 8 x SciPy's own error against a
 *    50-digit polar factor) as rotations — 1e-12 down to a singular-value ratio of 1e-8, growing like 1 / c for two singular
 *    values c times the third (the polar factor's own condition) — and flags, states and joints follow as for any goal.
 *    tests/test_gpu_matrix_forms.py, tests/matrix_forms.py, G23.
 *  Not covered: blocks outside that range (entries beyond 1e100, singular values below 1e-100 or a determinant that underflows).
 *  RSIK_EULER_NEVER makes no conversion and no determinant test: the block is consumed as it came. */

/* ---- why an emergency stop tripped: one bit per message the reference appends to ControlIK.emergency_state
 * (utils.multiturn_safety_check utils.py:544-566, utils.continuity_check utils.py:584-586) ---- */
#define RSIK_EMERGENCY_SHOULDER_PITCH 1  /* "EMERGENCY STOP: shoulder pitch limit reached"  joint 0 beyond +-6 pi */
#define RSIK_EMERGENCY_ELBOW_YAW 2       /* "EMERGENCY STOP: elbow yaw limit reached"       joint 2 */
#define RSIK_EMERGENCY_WRIST_YAW 4       /* "EMERGENCY STOP: wrist yaw limit reached"       joint 6 */
#define RSIK_EMERGENCY_CONTINUITY 8      /* " EMERGENCY STOP: joints are not continuous ..." continuous mode only */

/* ---- arms ---- */
#define RSIK_ARM_R 0
#define RSIK_ARM_L 1

/* ---- theta policies for rsik_solve (which elbow angle get_joints is evaluated at) ---- */
#define RSIK_THETA_INTERVAL0 0 /* theta = interval[0]  (README.md:85, ik_benchmarks.py:27-31) */
#define RSIK_THETA_EXPLICIT 1  /* theta = theta_in[i] */
#define RSIK_THETA_FRACTION 2  /* theta = i0 + theta_in[i] * (i1' - i0), i1' = i1 (+2pi if wrapped) */
#define RSIK_THETA_NONE 3      /* is_reachable only: joints/elbow are not written */

/* ---- constrained modes (control_ik.py:225-232) ---- */
#define RSIK_MODE_UNCONSTRAINED 0
#define RSIK_MODE_LOW_ELBOW 1

/*
 * Per-arm constant block: a flat array of RSIK_ARM_CONSTS_COUNT doubles computed once on the host
 * from SymbolicIK.__init__'s arguments (symbolic_ik.py:26-83, utils.py:26-43) plus the
 * pose-independent parts of get_joints / make_elbow_projection (symbolic_ik.py:728-738, 653-672).
 * Offsets:
 */
enum {
    RSIK_C_SHOULDER = 0,      /* [3] shoulder_position                                   */
    RSIK_C_UPPER_ARM = 3,     /* upper_arm_size u                                         */
    RSIK_C_FOREARM = 4,       /* forearm_size f                                           */
    RSIK_C_TIPL = 5,          /* [3] wrist offset in the goal frame (-tip_x, tip_y, tip_z) symbolic_ik.py:422 */
    RSIK_C_MAX_LEN = 8,       /* max_arm_length                                           */
    RSIK_C_MIN_DIST = 9,      /* shoulder_wrist_min_distance                              */
    RSIK_C_BACKWARD = 10,     /* backward_limit                                           */
    RSIK_C_PROJ_MARGIN = 11,  /* projection_margin                                        */
    RSIK_C_NORMAL_MARGIN = 12,/* normal_vector_margin                                     */
    RSIK_C_UPF = 13,          /* u + f                                                    */
    RSIK_C_WRIST_R = 14,      /* sin(radians(wrist_limit)) * f          symbolic_ik.py:413 */
    RSIK_C_WRIST_AX = 15,     /* sqrt(f^2 - r^2)                        symbolic_ik.py:414 */
    RSIK_C_MST = 16,          /* [9] M_shoulder_torso row-major         symbolic_ik.py:728-736 */
    RSIK_C_TSH = 25,          /* [3] P_shoulder_torso = -M_shoulder_torso . s  symbolic_ik.py:737 */
    RSIK_C_ES = 28,           /* [3] elbow_singularity_position                           */
    RSIK_C_SING_OFFSET = 31,  /* singularity_offset                                       */
    RSIK_C_SING_COEFF = 32,   /* singularity_limit_coeff                                  */
    RSIK_C_ELBOW_LIMIT = 33,  /* radians(elbow_limit)                                     */
    RSIK_C_SIDE = 34,         /* +1 r_arm, -1 l_arm                                       */
    RSIK_C_PLANE_P = 35,      /* [3] P_limits                           symbolic_ik.py:657 */
    RSIK_C_PLANE_N = 38,      /* [3] v3 (unit plane normal)             symbolic_ik.py:668-669 */
    RSIK_C_PROJ_CENTER = 41,  /* [3] projected_center                   symbolic_ik.py:671 */
    RSIK_C_PROJ_RADIUS = 44,  /* radius (NaN if the plane misses the shoulder sphere)  symbolic_ik.py:672 */
    RSIK_C_TIP_Z = 45,        /* tip_position[2]                        symbolic_ik.py:837 */
    RSIK_C_INV_U = 46,        /* 1 / upper_arm_size        (lengths that hold by construction) */
    RSIK_C_INV_F = 47,        /* 1 / forearm_size                                          */
    RSIK_C_INV_TIPZ = 48,     /* 1 / |tip_position[2]|                                     */
    RSIK_C_INV_GRIP = 49,     /* 1 / gripper_size = 1 / |tip_position|                     */
    RSIK_C_MAX_LEN_SQ = 50,   /* largest double x with sqrt(x) <= max_arm_length: |v| > max_arm_length <=> v.v > x, bit for bit */
    RSIK_C_INV_MIN_DIST = 51, /* 1 / shoulder_wrist_min_distance                           */
    RSIK_C_PLANE_K = 52,      /* es_z - singularity_offset - singularity_limit_coeff * es_x: the elbow is above the singularity
                                 plane (symbolic_ik.py:708-713) iff e_z > coeff * e_x + this */
    RSIK_ARM_CONSTS_COUNT = 53
};

typedef struct rsik_ctx rsik_ctx;

/* ---- lifecycle ---- */
int rsik_abi_version(void);
/* "RSIK_SRC_HASH=<32 hex digits>": hash of the sources and flags the library was built from (csrc/build.py), so a host
 * can refuse a stale binary.  Not in the reference (pure Python, nothing to build). */
const char *rsik_build_id(void);
int rsik_arm_consts_count(void);
/* Number of HIP devices visible; 0 when there is none (never fails). */
int rsik_device_count(void);
/* Creates a context bound to one GPU.  Replaces constructing SymbolicIK / ControlIK objects
 * (symbolic_ik.py:26, control_ik.py:28): constants are uploaded separately with rsik_set_arm. */
int rsik_create(int device_id, rsik_ctx **out);
int rsik_destroy(rsik_ctx *ctx);
/* Message of the last failing call on this context ("" if none).  ctx == NULL: last rsik_create failure. */
const char *rsik_last_error(const rsik_ctx *ctx);
/* Use the caller's hipStream_t (e.g. torch's current stream) for all launches; NULL = default stream. */
int rsik_set_stream(rsik_ctx *ctx, void *hip_stream);
/* Waits for the context's stream; also frees the workspaces that continuous runs have outgrown since the last call, and reports
 * (RSIK_E_HIP) a theta kernel of an overlapping continuous run that gave up its bounded wait for its prepare kernel (cannot happen:
 * everything it waits for is issued before it; bounded so that it cannot hang the device either). */
int rsik_sync(rsik_ctx *ctx);
/* Uploads one arm's constant block (host pointer).  Replaces SymbolicIK.__init__ (symbolic_ik.py:26-83). */
int rsik_set_arm(rsik_ctx *ctx, int arm, const double *consts_host, int count);

/* ---- per-context options ---- */
/* RSIK_OPT_EULER_ROUNDTRIP.  ControlIK turns the goal matrix into extrinsic xyz Euler angles
 * (utils.get_euler_from_homogeneous_matrix, utils.py:84-90, called at control_ik.py:215) and SymbolicIK rebuilds the
 * rotation from them (symbolic_ik.py:420).  For a proper rotation matrix away from gimbal lock that round trip is the
 * identity to rounding.  RSIK_EULER_AUTO (default): the control kernels consume M[:3,:3] directly and make the round
 * trip (SciPy's nearest-rotation / matrix -> quaternion -> Euler algorithms) only where it changes the result — the
 * matrix is not orthonormal to 1e-12, or the pitch is within 1e-5 of +-pi/2 (at the lock: yaw := 0).
 * RSIK_EULER_ALWAYS / RSIK_EULER_NEVER force either behaviour. */
#define RSIK_EULER_AUTO 0
#define RSIK_EULER_ALWAYS 1
#define RSIK_EULER_NEVER 2
#define RSIK_OPT_EULER_ROUNDTRIP 0
/* Kernel-variant selectors.  Every value gives the same results (to rounding where a comment says so); the defaults
 * (0) let the library choose.  They exist so that tests can force each variant in turn and A/B timings can pin one.
 *   RSIK_OPT_SWEEP_MODE     rsik_control_discrete's grid search (utils.py:366-396): 0 = chosen per wave, 1 = always the
 *                           exhaustive wave-cooperative sweep, 2 = always the per-lane search (a launch whose preferred_theta is
 *                           2^27 or more in magnitude takes 1 whatever is set here: "Rows that are numbers, of any size")
 *   RSIK_OPT_NO_TIPZ        non-zero: never use the goal stage specialised for tip_x = tip_y = 0
 *   RSIK_OPT_NO_MIRROR      non-zero: mixed r/l launches read every constant per lane (no mirror-image shortcut)
 *   RSIK_OPT_CONT_RUN_MODE  rsik_control_continuous_run: 0 = chosen by the library, 1 = the phased trajectory pipeline
 *                           (kernels per block of steps on four streams), 2 = one launch of the step kernel per control
 *                           step, exactly what n_steps calls of rsik_control_continuous_step issue */
#define RSIK_OPT_SWEEP_MODE 1
#define RSIK_OPT_NO_TIPZ 2
#define RSIK_OPT_NO_MIRROR 3
#define RSIK_OPT_CONT_RUN_MODE 4
#define RSIK_CONT_RUN_AUTO 0
#define RSIK_CONT_RUN_PHASED 1
#define RSIK_CONT_RUN_STEPS 2
/* Tuning of rsik_control_continuous_run (results do not depend on it):
 *   RSIK_OPT_CONT_BLOCK_STEPS  control steps per block: 0 (default) = a third of the run, at least 64 and — launch by launch — at most
 *                              512 (half of the run under capture); n > 0 = n (rounded up to the sequential phases' batch of steps) */
#define RSIK_OPT_CONT_BLOCK_STEPS 5
/*   RSIK_OPT_CONT_PHASED_VARIANT  phased pipeline issued launch by launch, a bit mask (0 = the default form; results do not depend on it):
 *                              1  its streams tied by hipEvents (as a run recorded into a hipGraph always is) instead of by
 *                                 hipStreamWriteValue32 / hipStreamWaitValue32 on words in device memory
 *                              2  the joints kernel of a block NOT held until the theta kernel of the next block has started
 *                              4 / 8 / 16  (runs that overlap, RSIK_OPT_CONT_GOALS_RESIDENT) the next run's prepare kernels not held at all /
 *                                 held until the previous run's last chain kernel has FINISHED / its theta kernels behind stream waits
 *                                 instead of waiting for their prepare kernels themselves — the steps docs/experiments.md R6.2 measures
 *                              64 the joints phase without its turn hints (R6.3; joints then differ in their last bits) */
#define RSIK_OPT_CONT_PHASED_VARIANT 6
#define RSIK_PHASED_EDGES_BY_EVENT 1
#define RSIK_PHASED_NO_THETA_FIRST 2
/*   RSIK_OPT_CONT_GOALS_RESIDENT  rsik_control_continuous_run issued launch by launch, run after run on one stream (results do not
 *                              depend on it).  0 (default): every run's four streams meet at its start and at its end — a run begins
 *                              when everything queued ahead of it, the previous run included, has finished.  1: a PROMISE by the caller
 *                              that lets consecutive runs of one shape overlap: the goal matrices `m12_steps` (and `arm`) handed to a
 *                              run were complete before the PREVIOUS continuous run of this context was issued, and nothing the caller
 *                              queued on the stream since that call reads or writes this run's `reachable_steps` / `state_steps` (they
 *                              may be the previous run's own buffers: each block's rows are then written behind that run's chain kernel
 *                              of the same rows).  The prepare phase of run k + 1 — a function of the goals alone — then runs beside the
 *                              joints and chain kernels of run k, in the workspace slots run k does not use (all eight are kept); the
 *                              start-up kernel, the theta, joints and chain phases of run k + 1 wait for run k's end as before (the
 *                              trajectory state: control_ik.py:80-83, 276-407 carries it from call to call), and the caller's stream
 *                              continues behind each run's last kernel as before.  Takes effect behind a run of the same n, block
 *                              length and stream, issued with value-word edges into the same workspace, on a context no hipGraph
 *                              points into; otherwise the run is issued as with 0 (rsik_control_continuous_last_form tells). */
#define RSIK_OPT_CONT_GOALS_RESIDENT 7
/*   RSIK_OPT_NEAREST_LANES  rsik_solve_nearest, a kernel-variant selector as the ones above (every value gives the same bits in
 *                           every output): lanes that share a pose's samples, 0 (default) = chosen by the library from n and
 *                           n_theta, or 1, 8 or 64; any other value is RSIK_E_INVALID */
#define RSIK_OPT_NEAREST_LANES 8
#define RSIK_OPT_COUNT 9
int rsik_set_option(rsik_ctx *ctx, int option, int value);
int rsik_get_option(const rsik_ctx *ctx, int option, int *value);

/* ---- device memory helpers for hosts without their own allocator (torch users do not need them) ---- */
int rsik_malloc(rsik_ctx *ctx, size_t bytes, void **dev_ptr);
int rsik_free(rsik_ctx *ctx, void *dev_ptr);
int rsik_memcpy_h2d(rsik_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int rsik_memcpy_d2h(rsik_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/*
 * rsik_solve — fused SymbolicIK.is_reachable (symbolic_ik.py:121-282) + one call of the returned
 * theta_to_joints_func = SymbolicIK.get_joints (symbolic_ik.py:697-863) per pose, canonical
 * "fresh is_reachable, then exactly one get_joints" semantics.
 *
 *   n            number of poses
 *   pose_soa     6 device arrays of n doubles: px, py, pz, roll, pitch, yaw — the reference's
 *                goal_pose = [[x,y,z],[roll,pitch,yaw]], extrinsic xyz Euler (README.md:73-75)
 *   arm          device array of n uint8 (RSIK_ARM_R / RSIK_ARM_L) or NULL
 *   arm_uniform  arm used for every pose when arm == NULL
 *   theta_policy RSIK_THETA_*;  theta_in: device array of n doubles for EXPLICIT / FRACTION, else NULL
 *   previous_joints_host  7 doubles (host) or NULL for zeros — get_joints' previous_joints argument
 *   joints       [n,7] row-major or NULL      (shoulder_pitch, shoulder_roll, elbow_yaw, elbow_pitch,
 *                                               wrist_roll, wrist_pitch, wrist_yaw)
 *   interval     [n,2] or NULL                 theta interval, i0 > i1 means wrap-around (README.md:83-84)
 *   elbow        [n,3] or NULL                 elbow position returned by get_joints
 *   reachable    [n] uint8 or NULL
 *   state        [n] uint8 RSIK_STATE_* or NULL
 */
int rsik_solve(rsik_ctx *ctx, int64_t n, const double *const pose_soa[6], const uint8_t *arm, int arm_uniform,
               int theta_policy, const double *theta_in, const double *previous_joints_host, double *joints,
               double *interval, double *elbow, uint8_t *reachable, uint8_t *state);

/*
 * rsik_control_discrete — ControlIK.symbolic_inverse_kinematics(name, M, "discrete", ...)
 * (control_ik.py:162-274 -> symbolic_inverse_kinematics_discrete :409-462 -> safety_checks :464-497),
 * which is a pure function of its inputs and constructor-time constants.
 *
 *   m12_soa          12 device arrays of n doubles: R00,R01,R02,R10,...,R22 (row-major rotation of the
 *                    4x4 goal matrix M) then tx,ty,tz (M[:3,3])
 *   arm/arm_uniform  as above (name "r_arm"/"l_arm")
 *   nb_search_points ControlIK.nb_search_points (control_ik.py:64), >= 2
 *   preferred_theta  the preferred_theta argument (r-arm convention; mirrored for l inside, control_ik.py:252)
 *   constrained_mode RSIK_MODE_*
 *   previous_sol_host 14 doubles: ControlIK.previous_sol["r_arm"], ["l_arm"] (control_ik.py:136,140)
 *   current_joints   [n,7] device or NULL (=> previous_sol of the pose's arm, control_ik.py:237-238; rows that hold that
 *                    vector give the NULL form's outputs bit for bit)
 *   orbita3d_max_angle  wrist cone half-angle in radians (control_ik.py:84)
 *   joints [n,7], reachable [n], state [n] as above; emergency [n] uint8 or NULL: non-zero where
 *   multiturn_safety_check tripped (utils.py:535-568), as RSIK_EMERGENCY_* cause bits.
 */
int rsik_control_discrete(rsik_ctx *ctx, int64_t n, const double *const m12_soa[12], const uint8_t *arm,
                          int arm_uniform, int nb_search_points, double preferred_theta, int constrained_mode,
                          const double *previous_sol_host, const double *current_joints, double orbita3d_max_angle,
                          double *joints, uint8_t *reachable, uint8_t *state, uint8_t *emergency);

/*
 * Per-row previous joints: n independent callers (robots, planner seeds, arms of a fleet) in one launch, each with its own
 * last solution.  Same arguments, checks and outputs as the entry above it, except that the launch-uniform host array is
 * replaced by an [n,7] row-major DEVICE array, one row per pose / goal (not NULL: RSIK_E_INVALID).  With every row equal to
 * the uniform vector (per arm for discrete) the outputs are bit for bit those of the uniform entry, except that a discrete
 * row that falls back to previous_sol (no theta found, current_joints NULL) takes the sin / cos of its wrist joints on the
 * device instead of from the host's libm (a few ulp; for a previous_sol whose wrist pitch lies beyond +-pi/2 — not a
 * solution any call returns — those ulps can also decide which turn allow_multiturn picks).  "Rows that are not numbers" applies row by row: a NaN or an infinity
 * in one row's previous vector changes only that row's outputs.
 * There is no per-row previous_theta: discrete mode hands it to limit_theta_to_interval and get_best_discrete_theta, and
 * neither uses it (utils.py:93-112, 334-396; the Q12 note of rsik_device.hpp).
 *
 * rsik_solve_rows — rsik_solve with previous_joints [n,7]: row i is get_joints' previous_joints for pose i
 *   (symbolic_ik.py:697-699; read only at an exact shoulder / elbow singularity, :751-753, :782-784).
 */
int rsik_solve_rows(rsik_ctx *ctx, int64_t n, const double *const pose_soa[6], const uint8_t *arm, int arm_uniform,
                    int theta_policy, const double *theta_in, const double *previous_joints, double *joints,
                    double *interval, double *elbow, uint8_t *reachable, uint8_t *state);

/*
 * rsik_solve_sweep — SymbolicIK.is_reachable once per pose, then the closure it returns (theta_to_joints_func = get_joints,
 * symbolic_ik.py:235, 697-863) at n_theta elbow angles of that pose, all from one launch: the arm's redundant degree of freedom
 * sampled for a planner, a reachability map or a data generator.  Added within ABI version 8: a new symbol, nothing else changed.
 *
 * Sample (k, i) is, bit for bit, what rsik_solve returns for pose i under the same theta_policy with theta_in = that sample's
 * value (with previous_joints: what rsik_solve_rows returns for that row); interval / reachable / state are rsik_solve's for
 * the same poses.  The samples are independent of each other and of their order: every one starts from the wrist is_reachable
 * left, so a sample whose elbow projection fired (symbolic_ik.py:708-718: the goal is MOVED, the joints reach the moved goal)
 * leaves nothing behind for the next — unlike get_joints called repeatedly on one SymbolicIK object, or
 * rsik_joints_from_state on one solver-state row.  Every sample's cos / sin are those of its theta (fraction 0 included: as
 * RSIK_THETA_FRACTION with 0, not as RSIK_THETA_INTERVAL0).
 *
 *   n_theta          samples per pose, 1 ... 4096
 *   theta_policy     RSIK_THETA_FRACTION or RSIK_THETA_EXPLICIT (anything else: RSIK_E_INVALID)
 *   theta_in         device; theta_per_pose == 0: [n_theta] values shared by every pose (a grid of fractions, one set of angles);
 *                    otherwise [n_theta][n], sample-major
 *   previous_joints  [n,7] device or NULL for zeros: one row per pose, shared by its samples (read only at an exact singularity)
 * Outputs are sample-major — each sample is one contiguous [n, W] array of the shape rsik_solve writes:
 *   joints           [n_theta][n][7]
 *   elbow            [n_theta][n][3] or NULL
 *   projected        [n_theta][n] uint8 or NULL: 1 where the elbow projection fired for that sample; 0 for unreachable poses
 *   theta            [n_theta][n] or NULL: the angle evaluated — FRACTION: i0 + u * (i1' - i0), i1' = i1 + 2 pi when i0 > i1;
 *                    EXPLICIT: the input; NaN for unreachable poses
 *   interval [n,2], reachable [n], state [n]   as rsik_solve, any of them NULL
 * Unreachable and invalid poses give NaN joints and elbow in every sample.  "Rows that are not numbers" applies: a pose with a
 * NaN or an infinity reports RSIK_STATE_INVALID_INPUT and NaN in all its samples; a theta that is not a number poisons its own
 * (sample, pose) — that sample of every pose where it sits in a shared grid — and nothing else.
 * n == 0 launches nothing.  Enqueued on the context's stream; never waits for the device.
 */
int rsik_solve_sweep(rsik_ctx *ctx, int64_t n, const double *const pose_soa[6], const uint8_t *arm, int arm_uniform,
                     int n_theta, int theta_policy, const double *theta_in, int theta_per_pose,
                     const double *previous_joints,
                     double *joints, double *elbow, uint8_t *projected, double *theta,
                     double *interval, uint8_t *reachable, uint8_t *state);

/*
 * rsik_solve_nearest — rsik_solve_sweep's samples, and of them the one whose joints are nearest to the joints the caller has: what
 * a planner, an IK-seeded trajectory optimiser or a data generator asks after a sweep, answered on the device with one row per
 * pose instead of n_theta.  Added within ABI version 8: a new symbol and a new option (RSIK_OPT_NEAREST_LANES), nothing else changed.
 *
 * n ... previous_joints are rsik_solve_sweep's arguments, with its checks and its error codes (n_theta 1 ... 4096, RSIK_THETA_FRACTION or
 * RSIK_THETA_EXPLICIT, theta_in [n_theta] or [n_theta][n]).  Sample k of pose i is what rsik_solve_sweep computes for it.
 *
 *   seed_joints      [n,7] device, row-major: the joints row i wants to stay near (not NULL: RSIK_E_INVALID)
 *   weights_host     7 doubles (host) or NULL for ones; each finite and >= 0, otherwise RSIK_E_INVALID
 *   flags            bit mask: RSIK_NEAREST_SKIP_PROJECTED — a sample whose elbow projection fired is not a candidate (its joints
 *                    reach the MOVED goal, symbolic_ik.py:708-718); any other bit: RSIK_E_INVALID
 *
 * The cost of sample k of pose i is  c = sum_q w_q * d_q * d_q,  d_q = angle_diff(joints[k][i][q], seed[i][q])  (utils.py:486-490),
 * q = 0 ... 6 in that order, unfused.  With unit weights sqrt(c) is the number rsik_theta_from_joints returns as `distance`.
 * A sample is a candidate iff its pose is reachable, its c is a number (a theta or a seed entry that is NaN gives NaN) and `flags`
 * does not exclude it.  The winner is the candidate with the smallest c — compared on c, not on its square root —, the lowest k
 * among equal costs.
 *
 * Outputs, one row per pose, any of them NULL (index, theta and joints all NULL: RSIK_E_INVALID):
 *   index            [n] int32: the winning k, or -1 where the pose has no candidate
 *   theta [n], joints [n,7], elbow [n,3], projected [n] uint8
 *                    bit for bit what rsik_solve_sweep writes for sample index[i] of pose i; without a candidate NaN, projected 0
 *   cost             [n]: sqrt(c) of the winner, NaN without one
 *   interval [n,2], reachable [n], state [n]   as rsik_solve.  `reachable` stays is_reachable's answer: a pose can be reachable
 *                    and still have index -1 (every sample projected under RSIK_NEAREST_SKIP_PROJECTED, a NaN in its seed row,
 *                    no theta that is a number).
 * "Rows that are not numbers" applies row by row: a pose with a NaN or an infinity reports RSIK_STATE_INVALID_INPUT and index -1;
 * a seed row with a NaN loses its own row only (index -1, reachable unchanged); a theta that is not a number never wins.
 * The result does not depend on RSIK_OPT_NEAREST_LANES.  n == 0 launches nothing.  Enqueued on the context's stream; never waits
 * for the device.
 */
#define RSIK_NEAREST_SKIP_PROJECTED 1
int rsik_solve_nearest(rsik_ctx *ctx, int64_t n, const double *const pose_soa[6], const uint8_t *arm, int arm_uniform,
                       int n_theta, int theta_policy, const double *theta_in, int theta_per_pose,
                       const double *previous_joints, const double *seed_joints, const double *weights_host, int flags,
                       int32_t *index, double *theta, double *joints, double *elbow, double *cost, uint8_t *projected,
                       double *interval, uint8_t *reachable, uint8_t *state);

/*
 * rsik_solve_path — n paths of n_steps waypoints for one arm each: rsik_solve_sweep's n_theta samples at every waypoint, and of the
 * n_theta ^ n_steps ways through them the one along which the joints move least, found on the device by dynamic programming, from one
 * launch.  The offline, globally optimal counterpart of the continuous mode's greedy theta tracking (control_ik.py:276-407), and of a
 * chain of rsik_solve_nearest launches each seeded with the winner before it.  Added within ABI version 8: two new symbols and two
 * flags, nothing else changed.
 *
 * Every per-waypoint array is waypoint-major, [n_steps][n]: entry [t][i] is waypoint t of path i (the order of m12_steps and
 * joints_steps of rsik_control_continuous_run).
 *   n, n_steps       n >= 0 paths of 1 ... 65536 waypoints
 *   pose_soa         six device arrays of n_steps * n doubles
 *   arm              [n], one byte per path, or NULL with arm_uniform
 *   n_theta          samples per waypoint, 1 ... 64 (anything else: RSIK_E_INVALID)
 *   theta_policy     RSIK_THETA_FRACTION or RSIK_THETA_EXPLICIT
 *   theta_in         device; theta_per_pose == 0: [n_theta] values shared by every waypoint; otherwise [n_theta][n_steps * n]
 *   start_joints     [n,7] device or NULL: the joints each path starts from
 *   weights_host     7 doubles (host) or NULL for ones; each finite and >= 0, otherwise RSIK_E_INVALID
 *   flags            RSIK_PATH_SKIP_PROJECTED (as RSIK_NEAREST_SKIP_PROJECTED), RSIK_PATH_UNWIND (below); any other bit: RSIK_E_INVALID
 *   workspace        device memory of the caller's, at least rsik_solve_path_workspace_bytes(n, n_steps, n_theta) bytes (the
 *                    backpointer table, n * n_steps * n_theta bytes, and one byte per waypoint); NULL or too small: RSIK_E_INVALID.
 *                    Only read and written by the launch; free to reuse once the launch has finished.
 * There is no previous_joints: every sample is what rsik_solve_sweep computes with previous_joints == NULL.
 *
 * Definition (the result does not depend on how the kernel is laid out):
 *   Sample k of waypoint (t, i) is rsik_solve_sweep's sample k over the same n_steps * n poses; J[k] are its joints.
 *   A sample is a CANDIDATE iff its pose is reachable, none of its joints is a NaN, and `flags` does not exclude it.
 *   A waypoint with at least one candidate is SOLVED; one without is SKIPPED (index -1, NaN rows, projected 0) and the path goes on
 *   as if it were not there: the next solved waypoint is measured against the last solved one.
 *   The transition cost is  c(a, b) = sum_q w_q * d_q * d_q,  d_q = angle_diff(b_q, a_q)  (utils.py:486-490), q = 0 ... 6 in that
 *   order, unfused: rsik_solve_nearest's cost of joints b against seed a.
 *   At a path's first solved waypoint A(k) = c(start_joints[i], J[k]), or 0 when start_joints is NULL, for every candidate k.
 *   At every later solved waypoint A(j) = min over the candidates i of the previous solved waypoint of (A(i) + c(J_prev[i], J[j])) —
 *   one rounding for the sum —, the lowest i among equal values.
 *   The path ends in the candidate j with the smallest A at the last solved waypoint, the lowest j among equal values; the other
 *   winners follow by going back along the i that gave each A.
 *
 * Outputs, any of them NULL (index, theta and joints all NULL: RSIK_E_INVALID):
 *   index            [n_steps][n] int32: the winning k, -1 at a skipped waypoint
 *   theta [n_steps][n], joints [n_steps][n][7], elbow [n_steps][n][3], projected [n_steps][n] uint8
 *                    bit for bit what rsik_solve_sweep writes for sample index[t][i] of that waypoint; NaN / 0 at a skipped one
 *   step_cost        [n_steps][n]: sqrt of the transition cost into waypoint t (rsik_solve_nearest's `cost` unit): from the last
 *                    solved waypoint before it; at the first solved waypoint from start_joints, 0 without them; NaN at a skipped one
 *   cost             [n]: the minimal sum itself (the smallest A of the last solved waypoint), not its root; NaN when no waypoint is solved
 *   n_solved         [n] int32: the number of solved waypoints
 *   interval [n_steps][n][2], reachable [n_steps][n], state [n_steps][n]   as rsik_solve for the n_steps * n poses.  `reachable`
 *                    stays is_reachable's answer: a waypoint can be reachable and skipped.
 *
 * RSIK_PATH_UNWIND: row t of `joints` becomes allow_multiturn(row t as above, the previous solved waypoint's row AS WRITTEN)
 * (utils.py:493-505: prev + angle_diff(new, prev) per joint, what RSIK_STAGE_ALLOW_MULTITURN computes), in order along the path; the
 * first solved row is unwound against start_joints, or left as it is without them.  The rows are then continuous along the path and
 * may leave [-pi, pi].  index, the costs and every other output do not change: angle_diff does not see whole turns.
 *
 * "Rows that are not numbers": a waypoint whose pose holds a NaN or an infinity reports RSIK_STATE_INVALID_INPUT and is skipped; a
 * theta that is not a number never wins; a start_joints row that holds a NaN or an infinity loses its own path only — no sample of
 * that path is a candidate: n_solved 0, every index -1, cost NaN, reachable and state unchanged.  Every other path's outputs are the
 * bits of a run in which the bad value was an ordinary one.
 * n == 0 launches nothing.  Enqueued on the context's stream; allocates nothing and never waits for the device.
 *
 * rsik_solve_path_workspace_bytes — the workspace rsik_solve_path needs for (n, n_steps, n_theta), monotone in each of them;
 *   RSIK_E_INVALID for a NULL `bytes` or arguments rsik_solve_path refuses.
 */
#define RSIK_PATH_SKIP_PROJECTED 1
#define RSIK_PATH_UNWIND 2
int rsik_solve_path_workspace_bytes(int64_t n, int64_t n_steps, int n_theta, size_t *bytes);
int rsik_solve_path(rsik_ctx *ctx, int64_t n, int64_t n_steps, const double *const pose_soa[6],
                    const uint8_t *arm, int arm_uniform,
                    int n_theta, int theta_policy, const double *theta_in, int theta_per_pose,
                    const double *start_joints, const double *weights_host, int flags,
                    void *workspace, size_t workspace_bytes,
                    int32_t *index, double *theta, double *joints, double *elbow, uint8_t *projected,
                    double *step_cost, double *cost, int32_t *n_solved,
                    double *interval, uint8_t *reachable, uint8_t *state);

/*
 * rsik_solve_path_clear — rsik_solve_path among obstacles: the least-motion way through the samples that keep the arm at least
 * min_clearance away from a static scene, with a price on coming nearer than `influence`, from one launch.  What a planner otherwise
 * composes from rsik_solve_sweep, rsik_clearance over the n_theta * n_steps * n joints and a dynamic programme of its own.  Added within
 * ABI version 8: a new symbol, no new option, nothing else changed.
 *
 * Every argument rsik_solve_path has means exactly what it means there: the layouts, both flags, the skip rule, the refusals and "Rows
 * that are not numbers".  The workspace is rsik_solve_path's, and rsik_solve_path_workspace_bytes answers for both calls.
 *   link_radius_host, n_spheres, spheres, n_capsules, capsules
 *                    as rsik_track_avoid: 0 ... 256 spheres [n_spheres][4] and 0 ... 64 capsules [n_capsules][7] (device), at least one
 *                    obstacle in all, 3 link radii on the host or NULL for zeros.  The scene is static and shared by every path,
 *                    waypoint and sample.  An obstacle row with a NaN, an infinity or a negative radius is skipped, as there.
 *   min_clearance    m: the hard constraint; finite, or -infinity for none
 *   influence        m, finite and >= 0, and
 *   clearance_gain   rad^2 per m^2, finite and >= 0: the soft term; a gain of 0 turns it off
 *
 * Definition, on top of rsik_solve_path's and as independent of the kernel's layout:
 *   d(k) of sample k of waypoint (t, i) is, bit for bit, the `clearance` rsik_clearance returns for that sample's joints as
 *   rsik_solve_sweep writes them (before any unwinding), with the path's arm, the same radii and the same obstacles; +infinity if every
 *   obstacle is skipped.
 *   A sample is a CANDIDATE iff it is one for rsik_solve_path and d(k) >= min_clearance (false for a NaN).  A waypoint whose samples
 *   are all excluded is SKIPPED like any other, and stays `reachable`.
 *   The node penalty is p(k) = (clearance_gain * u) * u with u = influence - d(k) where d(k) < influence, 0 elsewhere: a select,
 *   unfused, in that order.
 *   At a path's first solved waypoint A(k) = c(start_joints[i], J[k]) + p(k); without start_joints A(k) = p(k).
 *   At every later solved waypoint A(j) = (min over i of (A(i) + c(J_prev[i], J[j]))) + p(j): the minimum first, then one more sum.
 *   Ties go to the lowest i among equal values, and at the end to the lowest j, as in rsik_solve_path.
 *   `cost` is the minimal A, penalties included; `step_cost` stays the root of the transition cost alone.
 *
 * Outputs beside rsik_solve_path's, any of them NULL (index, theta and joints all NULL remains RSIK_E_INVALID):
 *   clearance        [n_steps][n]: d of the winning sample, NaN at a skipped waypoint
 *   nearest          [n_steps][n][2] int32, aligned to 8 bytes: rsik_clearance's (link, obstacle index) for the winning sample; (-1, -1)
 *                    at a skipped waypoint and where every obstacle is skipped
 *   blocked          [n_steps][n] uint8: how many of the n_theta samples satisfy rsik_solve_path's candidate rule and fail
 *                    d >= min_clearance; 0 on a lost path and at an invalid pose.  It tells why a waypoint was skipped.
 *
 * Guarantees:
 *   Any subset of the outputs gives the same bits, and two launches give the same bits.
 *   A path's bits depend neither on n nor on the other paths.
 *   clearance and nearest are bit for bit what rsik_clearance returns for the `joints` this call returns without RSIK_PATH_UNWIND.
 *   With min_clearance = -infinity and clearance_gain = 0 every output shared with rsik_solve_path has rsik_solve_path's bits.
 *   index, cost and clearance do not depend on the order of the obstacles; nearest's obstacle index does.
 *
 * RSIK_E_INVALID, the first fault in this order, nothing written: what rsik_solve_path refuses of n, n_steps, n_theta, theta_policy,
 * flags, weights and arms; n_spheres or n_capsules outside its range; no obstacle; a link radius, influence or clearance_gain that is
 * negative or not finite; a min_clearance that is a NaN or +infinity; then, for n > 0, what rsik_solve_path refuses of its pointers and
 * workspace; a NULL obstacle array with a count above 0; a `nearest` that is not aligned to 8 bytes.
 * n == 0 launches nothing.  Enqueued on the context's stream; allocates nothing and never waits for the device.
 */
int rsik_solve_path_clear(rsik_ctx *ctx, int64_t n, int64_t n_steps, const double *const pose_soa[6],
                          const uint8_t *arm, int arm_uniform,
                          int n_theta, int theta_policy, const double *theta_in, int theta_per_pose,
                          const double *start_joints, const double *weights_host, int flags,
                          const double *link_radius_host, int n_spheres, const double *spheres, int n_capsules, const double *capsules,
                          double min_clearance, double influence, double clearance_gain,
                          void *workspace, size_t workspace_bytes,
                          int32_t *index, double *theta, double *joints, double *elbow, uint8_t *projected,
                          double *step_cost, double *cost, int32_t *n_solved,
                          double *interval, uint8_t *reachable, uint8_t *state,
                          double *clearance, int32_t *nearest, uint8_t *blocked);

/*
 * rsik_solve_path_pair — rsik_solve_path_clear for n_pairs robots of two arms that keep out of each other: the elbow angles along two
 * hand paths, chosen together, so that neither arm comes nearer than min_clearance to a static scene or to the other arm, from one
 * launch.  A state of the dynamic programme is a PAIR of samples, one per arm; the n_theta^2 arm-to-arm distances per waypoint stay
 * on the device.  Added within ABI version 8: two new symbols, no new option, nothing else changed.
 *
 * Rows are rsik_track_pair's: n = 2 * n_pairs, row 2i the right arm of robot i, row 2i + 1 its left arm; there is no arm argument and
 * both arms' constants must be set (RSIK_E_NOT_SET otherwise).  Every per-waypoint array has rsik_solve_path_clear's layout for n rows
 * ([n_steps][n]...), so one set of buffers serves rsik_solve_path_clear with arm bytes 0, 1, 0, 1, ... and then this call;
 * start_joints is [n][7]; weights_host, 7 doubles, is shared by both arms.  Per robot: cost [n_pairs], n_solved [n_pairs] and
 * blocked [n_steps][n_pairs], uint16 (the count can reach 256).
 * Every argument rsik_solve_path_clear has means what it means there — policies, both flags, "Rows that are not numbers" — but:
 *   n_theta          1 ... 16 (a robot has at most 256 states); anything else: RSIK_E_INVALID
 *   the scene        may be empty, as in rsik_track_pair: the partner is always an obstacle
 *   workspace        at least rsik_solve_path_pair_workspace_bytes(n_pairs, n_steps, n_theta) bytes (n_pairs * n_steps *
 *                    (n_theta^2 + 3): a backpointer byte per state, a flag and two winners per waypoint), monotone in each argument
 *
 * Definition (the result does not depend on how the kernel is laid out):
 *   Sample a of row 2i and sample b of row 2i + 1 at waypoint t are rsik_solve_sweep's samples over the n_steps * n poses with arm
 *   bytes 0, 1, 0, 1, ...; JR[a] and JL[b] are their joints.  Each is a ROW CANDIDATE by rsik_solve_path's rule (reachable, no NaN, flags).
 *   dR(a, b) is, bit for bit, rsik_clearance's `clearance` of JR[a] with the right arm, the given radii, the static spheres, and the
 *   static capsules followed by three more: (P_l, P_{l+1}, link_radius[l]), l = 0, 1, 2, with P the link_points rsik_clearance returns
 *   for JL[b] — rsik_track_pair's construction, with its obstacle indices n_spheres + n_capsules + l.  dL(a, b) is the same with the
 *   arms exchanged.  The two can differ in the last bit; both are kept.
 *   (a, b) is a CANDIDATE PAIR iff both are row candidates, dR(a, b) >= min_clearance and dL(a, b) >= min_clearance (false for a NaN).
 *   A waypoint with at least one candidate pair is SOLVED for both arms; any other is SKIPPED for both: index -1 and NaN in both
 *   rows, and the path goes on as if the waypoint were not there.  (A stretch one arm cannot reach is planned for the other arm
 *   alone with rsik_solve_path_clear.)
 *   The penalty is p(a, b) = pR + pL, each rsik_solve_path_clear's select on its own d; pR first, then one sum.
 *   At the first solved waypoint A(a, b) = (cR(startR, JR[a]) + cL(startL, JL[b])) + p(a, b); without start_joints A(a, b) = p(a, b).
 *   c is rsik_solve_path's transition cost on the arm's own joints.
 *   At every later solved waypoint, in two stages over the candidate pairs of the previous solved waypoint:
 *     1. B(a, b') = min over b with (a, b) a candidate pair of (A(a, b) + cL(JLprev[b], JL[b'])), the lowest b among equal values;
 *     2. A'(a', b') = (min over a for which B(a, b') exists of (B(a, b') + cR(JRprev[a], JR[a']))) + p(a', b'), the lowest a among
 *        equal values.  The backpointer of (a', b') is (a, the b stage 1 chose for (a, b')).
 *   The path ends in the candidate pair with the smallest A, the lowest a * n_theta + b among equal values; the other winners follow
 *   the backpointers.  `cost` is that A; `step_cost` is, per row, the root of that arm's own transition cost.
 *   RSIK_PATH_UNWIND acts per row, as in rsik_solve_path.
 *   A NaN or an infinity in either start row loses the whole robot: n_solved 0, index -1, cost NaN, blocked 0; no other robot changes.
 *
 * Outputs, any of them NULL (index, theta and joints all NULL: RSIK_E_INVALID):
 *   index, theta, joints, elbow, projected   of row r at (t, r): the bits of the sweep's winning sample of that row
 *   clearance        [n_steps][n]: clearance[t][2i] = dR of the winning pair, clearance[t][2i + 1] = dL; NaN at a skipped waypoint
 *   nearest          [n_steps][n][2] int32, aligned to 8 bytes: the (link, obstacle) of each view; (-1, -1) at a skipped waypoint
 *   blocked          [n_steps][n_pairs] uint16: the pairs (a, b) that are both row candidates and no candidate pair
 *   interval, reachable, state   as rsik_solve for the n_steps * n poses: a waypoint can be reachable for both arms and skipped
 *
 * Guarantees:
 *   Any subset of the outputs gives the same bits, and two launches give the same bits.
 *   A robot's bits depend neither on n_pairs, nor on its place in the launch, nor on the other robots.
 *   clearance and nearest of a row are bit for bit rsik_clearance's for the row's returned joints (without RSIK_PATH_UNWIND), with the
 *   static scene followed by the three capsules built from the partner's returned joints.
 *
 * RSIK_E_INVALID, the first fault in this order, nothing written: n_pairs < 0; then what rsik_solve_path_clear refuses, in its order,
 * with n_theta above 16 refused and "no obstacle" not.  n_pairs == 0 launches nothing.  Enqueued on the context's stream; allocates
 * nothing and never waits for the device.
 *
 * rsik_solve_path_pair_workspace_bytes — RSIK_E_INVALID for a NULL `bytes` or arguments rsik_solve_path_pair refuses.
 */
int rsik_solve_path_pair_workspace_bytes(int64_t n_pairs, int64_t n_steps, int n_theta, size_t *bytes);
int rsik_solve_path_pair(rsik_ctx *ctx, int64_t n_pairs, int64_t n_steps, const double *const pose_soa[6],
                         int n_theta, int theta_policy, const double *theta_in, int theta_per_pose,
                         const double *start_joints, const double *weights_host, int flags,
                         const double *link_radius_host, int n_spheres, const double *spheres, int n_capsules, const double *capsules,
                         double min_clearance, double influence, double clearance_gain,
                         void *workspace, size_t workspace_bytes,
                         int32_t *index, double *theta, double *joints, double *elbow, uint8_t *projected,
                         double *step_cost, double *cost, int32_t *n_solved,
                         double *interval, uint8_t *reachable, uint8_t *state,
                         double *clearance, int32_t *nearest, uint16_t *blocked);

/*
 * rsik_reach_map — a reachability map (capability map): for each of n_pos positions, over one set of n_rot hand orientations, how
 * many of the orientations are reachable, which ones, with which is_reachable outcome, and how much elbow freedom is left.  What the
 * reference's task_space_test builds pose by pose (src/benchmark/ik_comparison.py:137-181), from one launch and with a few bytes of
 * output per POSITION.  Added within ABI version 8: a new symbol, nothing else changed.
 *
 *   n_pos            positions, >= 0; n_pos == 0 launches nothing
 *   pos_soa          three device arrays of n_pos doubles: px, py, pz
 *   arm              [n_pos], one byte per POSITION (0 = r, 1 = l), or NULL with arm_uniform; rsik_solve's checks and error codes
 *                    (RSIK_E_NOT_SET where an arm's constants were not uploaded)
 *   n_rot            orientations, 1 ... 4096 (anything else: RSIK_E_INVALID)
 *   euler_soa        three device arrays of n_rot doubles: roll, pitch, yaw, the convention of rsik_solve
 *
 * Definition (the result does not depend on how the kernel is laid out): pose (i, j) is position i with orientation j.  Its
 * reachable, state and interval are, bit for bit, what rsik_solve returns under RSIK_THETA_NONE for that pose with arm byte arm[i].
 *
 * Outputs, one row per position, any of them NULL (all four NULL: RSIK_E_INVALID):
 *   count            [n_pos] uint32: the number of j with reachable == 1
 *   state_count      [n_pos][RSIK_REACH_MAP_STATES] uint32: entry c is the number of j whose state code is c (RSIK_STATE_*, indexed by
 *                    the code); every row sums to n_rot
 *   theta_measure    [n_pos]: the sum over the reachable j of the interval's width, i1 - i0, plus 2 pi where i0 > i1 (radians of
 *                    elbow angle left, summed over the orientations); 0.0, not NaN, where no orientation is reachable.  The order of
 *                    the sum is the kernel's own: the value is defined to rounding, n_rot^2 * 2 pi * 2^-53.  It is reproducible:
 *                    two launches on the same inputs give the same bits (no floating-point atomics, nothing accumulates into the
 *                    caller's memory).
 *   mask             [n_pos][ceil(n_rot / 64)] uint64: bit (j % 64) of word (j / 64) is pose (i, j)'s reachable flag; the padding
 *                    bits of the last word are 0
 *
 * "Rows that are not numbers" applies pose by pose, and follows from the definition:
 *   a position with a NaN or an infinity puts all n_rot of its poses in bin RSIK_STATE_INVALID_INPUT: count 0, theta_measure 0.0,
 *   mask 0; no other position changes;
 *   an orientation with a NaN or an infinity puts that one pose of every position in that bin, and nothing else changes.
 * Rows that are numbers, of any size, are answered as rsik_solve answers them: angles of magnitude 2^27 and above, positions up to
 * DBL_MAX.
 *
 * The parallelism comes from the POSITIONS: a position is owned by one wave, whose lanes are 64 orientations at a time.  A launch
 * with few positions and many orientations is correct but not fast (a few thousand positions fill an MI355X).
 * Enqueued on the context's stream; allocates nothing, needs no workspace and never waits for the device.
 */
#define RSIK_REACH_MAP_STATES 11 /* one bin per RSIK_STATE_* code, indexed by the code */
int rsik_reach_map(rsik_ctx *ctx, int64_t n_pos, const double *const pos_soa[3],
                   const uint8_t *arm, int arm_uniform,
                   int n_rot, const double *const euler_soa[3],
                   uint32_t *count, uint32_t *state_count, double *theta_measure, uint64_t *mask);

/*
 * rsik_control_discrete_rows — rsik_control_discrete with previous_sol [n,7]: row i is ControlIK.previous_sol[name] of the
 *   caller that owns goal i, for that row's own arm (no 2x7 split).  It is get_joints' previous_joints (control_ik.py:454-456),
 *   the fallback joints when no theta is found and current_joints is NULL (:237-238, :457-458), and safety_checks'
 *   reference (allow_multiturn and the +-6 pi limits, utils.py:493-505, 535-568).  Nothing is latched: a caller whose
 *   emergency stop is set filters its rows on the host (the reference returns previous_sol without solving).
 */
int rsik_control_discrete_rows(rsik_ctx *ctx, int64_t n, const double *const m12_soa[12], const uint8_t *arm,
                               int arm_uniform, int nb_search_points, double preferred_theta, int constrained_mode,
                               const double *previous_sol, const double *current_joints, double orbita3d_max_angle,
                               double *joints, uint8_t *reachable, uint8_t *state, uint8_t *emergency);

/*
 * rsik_control_continuous_step — ControlIK.symbolic_inverse_kinematics(name, M, "continuous", ...)
 * (control_ik.py:162-274 -> symbolic_inverse_kinematics_continuous :276-407) for n independent trajectories,
 * one control step per call.  The reference keeps previous_theta / previous_sol / init / emergency_stop on the
 * ControlIK object (control_ik.py:60-83); here they live in a caller-owned device array
 * cont_state[RSIK_CONT_STATE_ROWS][n] (SoA): row 0 previous_theta, rows 1-7 previous_sol, row 8 init (0/1),
 * row 9 emergency_stop (0/1), row 10 has_previous_sol (0/1); written only by the step that trips an emergency stop:
 * row 11 its RSIK_EMERGENCY_* cause bits and rows 12-18 the joints that failed the continuity check (the "joints" of
 * the reference's message, utils.py:584-586; its "previous_joints" are rows 1-7).
 *
 *   m12_soa               goal matrices of this step (layout as rsik_control_discrete)
 *   current_pose_m12_soa  current_pose of trajectories that (re)initialise this step, or NULL (=> the goal matrix)
 *   timed_out             [n] uint8 or NULL: 1 replaces the reference's wall-clock test
 *                         abs(t - last_call_t) > call_timeout (control_ik.py:296-304)
 *   preferred_theta       the preferred_theta argument (r convention; used by the init search and the unreachable branch)
 *   preferred_theta_self_host  2 doubles: ControlIK.preferred_theta["r_arm"], ["l_arm"] (control_ik.py:133-139),
 *                         used by the reachable branch (Q14)
 *   current_joints        [n,7] device or NULL (=> previous_sol)
 *   state codes           RSIK_STATE_EMPTY when reachable, RSIK_STATE_LIMITED_BY_SHOULDER, the is_reachable state when
 *                         unreachable, RSIK_STATE_EMERGENCY while the emergency stop is latched.
 */
#define RSIK_CONT_STATE_ROWS 19
int rsik_control_continuous_step(rsik_ctx *ctx, int64_t n, const double *const m12_soa[12],
                                 const double *const current_pose_m12_soa[12], const uint8_t *arm, int arm_uniform,
                                 const uint8_t *timed_out, double preferred_theta, const double *preferred_theta_self_host,
                                 int constrained_mode, double d_theta_max, const double *current_joints,
                                 double orbita3d_max_angle, double *cont_state, double *joints, uint8_t *reachable,
                                 uint8_t *state);

/*
 * rsik_control_continuous_run — n_steps consecutive control steps of n trajectories from one host call (the whole
 * trajectory batch resident in HBM).  The result equals n_steps calls of rsik_control_continuous_step (flags, state
 * codes and the carried theta bit for bit, joints to the last bits: see phase 3), but the work is not done step by
 * step: most of a control step does not depend on the previous one — the goal conversion, is_reachable /
 * is_reachable_no_limits and the 10-point search for the target theta (control_ik.py:327-388 up to the rate limiter)
 * are functions of the pose alone — so the batch is solved in four phases per block of steps:
 *   1. prepare   one thread per (step, trajectory), chip-filling: is_reachable + the search for the target theta; the
 *                step's goal for the rate limiter (the search's theta / the preferred theta / "stay") -> workspace
 *   2. theta     one thread per trajectory, sequential over steps: the d_theta_max rate limiter and
 *                limit_theta_to_interval (the only recurrence on previous_theta)
 *   3. joints    one thread per (step, trajectory), a wave = 8 consecutive steps of 8 trajectories: the circle of
 *                is_reachable / is_reachable_no_limits re-derived from the goal matrix, get_joints at the limited theta,
 *                the Orbita3D cone clamp, and allow_multiturn INSIDE the 8-step chunk (whole turns relative to the step
 *                before, a shuffle prefix sum); continuity / limit / singularity events are detected, not decided
 *   4. chain     eight lanes per trajectory (one per joint), sequential over CHUNKS: checks each chunk's first step
 *                against previous_sol (continuity_check, the +-6 pi clamp, the emergency latch) and finds the whole
 *                turns the chunk sits away from it, which it adds to the chunk's rows where they are not zero (fp64 atomic
 *                adds that nobody waits for); only a chunk with an event is walked step by step with the reference's own
 *                sequence of operations (also: steps whose get_joints hit an exact singularity)
 * A run is cut into blocks of steps: three — of at most 512 steps — when it is issued launch by launch, two when it is being captured
 * into a hipGraph (RSIK_OPT_CONT_BLOCK_STEPS overrides).  Flags, state codes, the carried theta and the latch do not depend on the cut,
 * nor do the joints of a run of up to eight blocks; beyond that the joints can differ in their last bits from cut to cut (each is
 * within 2 ulp of the step kernel's: from the ninth block on phase 3 writes a wound trajectory's rows where phase 4 left previous_sol
 * eight blocks earlier, one rounding instead of two).  Runs of one shape issued one after the other can overlap:
 * RSIK_OPT_CONT_GOALS_RESIDENT.
 * The phases of neighbouring blocks overlap on four streams (the caller's and three of the context's).  Issued launch by
 * launch the streams are tied by words in device memory (hipStreamWriteValue32 behind the producer, hipStreamWaitValue32
 * ahead of the consumer: a third of an event's latency) and a block's joints kernel is held until the NEXT block's theta
 * kernel has started (its lone 276-register waves cannot get onto a chip that a chip-filling kernel holds); while the
 * caller's stream is capturing, by events, which is all a capture takes.
 * A trajectory whose emergency stop is latched (control_ik.py:205-210: previous_sol, not reachable, the emergency state for every
 * goal until "unfreeze") is not walked by phase 4: its steps of a block are filled in at once — on entry where it was latched before
 * the block, behind the chunk in which it latches otherwise.
 * The workspace
 * (17 bytes per step and trajectory + 1 per 8-step chunk, of up to eight blocks in flight, + 16 per trajectory), the side streams and the
 * events belong to the context: they are created by the first call that needs them, or ahead of time by
 * rsik_control_continuous_reserve.  A call can be captured into a hipGraph (the side streams join the capture through
 * the events the call records) provided it has nothing to create: reserve first, or run a call of at least that size
 * first — otherwise the call fails with RSIK_E_INVALID instead of allocating inside the capture.  A captured graph
 * stays valid after later, larger calls (the workspace it points into is kept until rsik_destroy / _release; an
 * outgrown workspace that only runs already issued can use is freed by the next rsik_sync).  The call never waits for
 * the device — with one exception in 4e9 launch-by-launch runs of a context: the words carry a 32-bit run number, and before it
 * wraps the call drains what the context has issued and starts them over.  A solver whose
 * projection_margin is not positive (RSIK_STATE_NOT_REACHABLE_NO_LIMITS possible) is run step by step.  At most 30 Mi
 * trajectories per call.  4096 trajectories x 1000 steps: see DESIGN.md section 4.
 * A goal that is not numbers: see "Rows that are not numbers" above (the step is reported, the trajectory goes on).
 *   m12_steps        device [n_steps][12][n]: the goal matrices of every step
 *   current_pose_m12_soa / current_joints   used by the first step only (see rsik_control_continuous_step)
 *   first_step_timed_out  non-zero: every trajectory (re)initialises on the first step (the reference's behaviour for
 *                    the first call after construction, control_ik.py:160,298)
 *   joints_steps     device [n_steps][n][7]; reachable_steps / state_steps device [n_steps][n] or NULL
 */
int rsik_control_continuous_run(rsik_ctx *ctx, int64_t n, int64_t n_steps, const double *m12_steps,
                                const double *const current_pose_m12_soa[12], const uint8_t *arm, int arm_uniform,
                                int first_step_timed_out, double preferred_theta, const double *preferred_theta_self_host,
                                int constrained_mode, double d_theta_max, const double *current_joints,
                                double orbita3d_max_angle, double *cont_state, double *joints_steps,
                                uint8_t *reachable_steps, uint8_t *state_steps);

/*
 * rsik_control_continuous_last_form — how the last rsik_control_continuous_run of this context was issued (nothing is returned
 * through the run's own arguments: the results do not depend on the form, the cost does).  RSIK_CONT_FORM_STEPS_NO_LIMITS_CAN_FAIL:
 * the solver's projection_margin is not positive, so is_reachable_no_limits can fail (symbolic_ik.py:343-345; the reference then
 * raises on purpose, control_ik.py:385-387, here RSIK_STATE_NOT_REACHABLE_NO_LIMITS) — an outcome the pipeline's phases do not carry:
 * the run was n_steps launches of the step kernel whatever RSIK_OPT_CONT_RUN_MODE said, 10-30 x the pipeline's time.
 */
#define RSIK_CONT_FORM_NONE 0                      /* no run yet */
#define RSIK_CONT_FORM_PHASED 1                    /* the trajectory pipeline, launch by launch */
#define RSIK_CONT_FORM_PHASED_OVERLAPPED 2         /* ... its prepare phase started beside the previous run (RSIK_OPT_CONT_GOALS_RESIDENT) */
#define RSIK_CONT_FORM_PHASED_CAPTURED 3           /* ... recorded into a hipGraph */
#define RSIK_CONT_FORM_STEPS 4                     /* one launch of the step kernel per control step, as RSIK_OPT_CONT_RUN_MODE asked */
#define RSIK_CONT_FORM_STEPS_NO_LIMITS_CAN_FAIL 5  /* ... because the arm's projection margin is not positive */
int rsik_control_continuous_last_form(const rsik_ctx *ctx);

/*
 * rsik_control_continuous_reserve — creates what rsik_control_continuous_run(n, n_steps) would create on first use
 * (workspace, side streams, events), so that the run itself allocates nothing: call it before capturing such a run into
 * a hipGraph on a context that has not yet run one of that size.  Uses RSIK_OPT_CONT_BLOCK_STEPS as set at the time.
 */
int rsik_control_continuous_reserve(rsik_ctx *ctx, int64_t n, int64_t n_steps);

/*
 * rsik_control_continuous_release — waits for the device and frees everything rsik_control_continuous_run keeps in the
 * context between calls: the workspace and the workspaces it has outgrown.  After it, hipGraphs captured from this
 * context's continuous runs must not be replayed any more.  (The context otherwise holds one workspace, of the largest
 * run so far, grown geometrically.)
 */
int rsik_control_continuous_release(rsik_ctx *ctx);

/*
 * rsik_stage — the stages of SymbolicIK.is_reachable as the reference exposes them: public methods that take their operands
 * as arguments (and self.wrist_position, which a caller may assign), timed one by one by src/benchmark/ik_benchmarks.py:36-130.
 * The fused kernels never form these intermediates; this entry point does, with the reference's own sequence of operations, on
 * whatever operands it is given.  Row-major: row i reads in[i * in_stride ...], writes out[i * out_stride ...] (device pointers,
 * or pinned host memory the device can address); `arm`: whose constants (RSIK_ARM_R / RSIK_ARM_L).  Per row, in -> out:
 *   RSIK_STAGE_POSE_IN_REACH        is_pose_in_robot_reach symbolic_ik.py:284-307: position 3, euler 3 -> in reach 0/1, position 3 (pulled
 *                                   back / clamped), state code (RSIK_STATE_EMPTY = the reference's "")
 *   RSIK_STAGE_WRIST_POSITION       get_wrist_position :418-425: position 3, euler 3 -> wrist 3
 *   RSIK_STAGE_LIMITATION_CIRCLE    get_limitation_wrist_circle :401-416: wrist 3, goal position 3 -> centre 3, radius, normal 3 (not normalised)
 *   RSIK_STAGE_INTERSECTION_CIRCLE  get_intersection_circle :366-399: wrist 3 -> found 0/1 (0 = None), centre 3, radius, normal 3
 *   RSIK_STAGE_CIRCLES_LINKED       are_circles_linked :427-568: wrist 3, intersection circle (centre 3, radius, normal 3), limitation circle
 *                                   (the same seven) -> how many numbers the returned array holds (0 or 2), the interval 2
 *   RSIK_STAGE_NEAREST_APPROACH     points_of_nearest_approach :588-606: p1 3, normal1 3, p2 3, normal2 3 -> q found 0/1 (0 = []), q 3, v 3
 *   RSIK_STAGE_CIRCLE_LINE          intersection_circle_line_3d_vd :608-645: centre 3, radius, direction 3, point on line 3 -> points 0/1/2, point 3, point 3
 *   RSIK_STAGE_ROTATION_FROM_VECTOR utils.rotation_matrix_from_vector utils.py:59-81: vector 3 -> 3 x 3 row-major
 * and the policy layer's helpers as utils.py exposes them — scalar functions of explicit arguments that callers of the reference import
 * (src/example/test_ik.py:16-21, test_go_to.py:10-13); `arm` is not read by these (nor by the three stages before them: a context
 * no arm was uploaded to runs them):
 *   RSIK_STAGE_ANGLE_DIFF           angle_diff utils.py:486-490: a, b -> the difference in [-pi, pi)
 *   RSIK_STAGE_IS_VALID_ANGLE       is_valid_angle :468-474: angle, interval 2 -> 0/1
 *   RSIK_STAGE_LIMIT_THETA_TO_INTERVAL  limit_theta_to_interval :93-112: theta, previous_theta, interval 2 -> theta, "theta in interval" 0/1
 *   RSIK_STAGE_IS_ELBOW_OK          is_elbow_ok :443-465: elbow 3, side (+1 r / -1 l), singularity_offset, singularity_limit_coeff,
 *                                   elbow_singularity_position 3 -> 0/1
 *   RSIK_STAGE_ALLOW_MULTITURN      allow_multiturn :493-505: new joints 7, previous joints 7 -> joints 7
 *   RSIK_STAGE_LIMIT_ORBITA3D_JOINTS  limit_orbita3d_joints :508-519: roll, pitch, yaw (intrinsic XYZ), max angle -> the three angles in the cone
 *   RSIK_STAGE_MULTITURN_SAFETY_CHECK  multiturn_safety_check :535-568: joints 7, the three limits -> joints 7, RSIK_EMERGENCY_* bits
 *   RSIK_STAGE_CONTINUITY_CHECK     continuity_check :571-589: joints 7, previous joints 7, max angular change 7 -> joints 7, stop 0/1
 *   RSIK_STAGE_BEST_DISCRETE_THETA  get_best_discrete_theta :334-396: previous_theta, interval 2, nb_search_points, preferred_theta, side,
 *                                   singularity_offset, singularity_limit_coeff, elbow_singularity_position 3, the intersection circle its
 *                                   get_elbow_position argument reads (centre 3, radius, normal 3) -> found 0/1, theta, preferred worked 0/1
 *                                   (nb_search_points outside [0, 2^20] or not a number: an empty grid)
 * and the rate limiter of the continuous mode, which the fused kernels carry inside (`arm` is not read):
 *   RSIK_STAGE_TEND_TO_PREFERRED_THETA  tend_to_preferred_theta :115-127: previous_theta, d_theta_max, goal_theta -> reached 0/1, theta
 *   RSIK_STAGE_BEST_CONTINUOUS_THETA2   get_best_continuous_theta2 :220-264: the 18 operands of RSIK_STAGE_BEST_DISCRETE_THETA, d_theta_max
 *                                   -> reachable 0/1, theta, which text (0 = nothing found: the search's own text, 1 = "theta theta_goal
 *                                   ok et proche" appended, 2 = "theta theta_goal ok mais loin" alone), "preferred_theta worked" 0/1 of the
 *                                   search inside
 */
#define RSIK_STAGE_POSE_IN_REACH 0
#define RSIK_STAGE_WRIST_POSITION 1
#define RSIK_STAGE_LIMITATION_CIRCLE 2
#define RSIK_STAGE_INTERSECTION_CIRCLE 3
#define RSIK_STAGE_CIRCLES_LINKED 4
#define RSIK_STAGE_NEAREST_APPROACH 5
#define RSIK_STAGE_CIRCLE_LINE 6
#define RSIK_STAGE_ROTATION_FROM_VECTOR 7
#define RSIK_STAGE_ANGLE_DIFF 8
#define RSIK_STAGE_IS_VALID_ANGLE 9
#define RSIK_STAGE_LIMIT_THETA_TO_INTERVAL 10
#define RSIK_STAGE_IS_ELBOW_OK 11
#define RSIK_STAGE_ALLOW_MULTITURN 12
#define RSIK_STAGE_LIMIT_ORBITA3D_JOINTS 13
#define RSIK_STAGE_MULTITURN_SAFETY_CHECK 14
#define RSIK_STAGE_CONTINUITY_CHECK 15
#define RSIK_STAGE_BEST_DISCRETE_THETA 16
#define RSIK_STAGE_TEND_TO_PREFERRED_THETA 17
#define RSIK_STAGE_BEST_CONTINUOUS_THETA2 18
#define RSIK_STAGE_COUNT 19
int rsik_stage(rsik_ctx *ctx, int op, int64_t n, int arm, const double *in, int in_stride, double *out, int out_stride);

/*
 * Solver-state entry points: the scalar drop-in API.  A SymbolicIK object keeps self.goal_pose,
 * self.wrist_position and self.intersection_circle between is_reachable() and the closure it returns
 * (symbolic_ik.py:143-144,185,235), and get_joints() mutates them when the elbow projection fires
 * (symbolic_ik.py:714-718).  That state lives in a caller-owned device array, one row of
 * RSIK_SOLVER_STATE_STRIDE doubles per solver instance:
 *   0-2 goal position, 3-5 goal euler, 6-8 wrist position, 9-11 circle centre, 12 circle radius,
 *   13-15 circle normal, 16-18 elbow position of the last get_joints, 19 projection flag,
 *   20-21 interval, 22 reachable (0/1), 23 state code of the last is_reachable (so that a scalar caller can fetch a
 *   call's results and the updated state with one download), 24-30 joints of the last get_joints, 31 reserved.
 */
#define RSIK_SOLVER_STATE_STRIDE 32
/* how a goal is laid out where an entry point takes either form (rsik_theta_from_joints, rsik_fk_residual) */
#define RSIK_GOAL_POSE6 0
#define RSIK_GOAL_M12 1

/* SymbolicIK.is_reachable (no_limits == 0, symbolic_ik.py:121-282) or is_reachable_no_limits
 * (no_limits != 0, symbolic_ik.py:85-119).  Only the fields the reference would have assigned are
 * written into solver_state (an early "Pose out of reach" leaves the row untouched). */
int rsik_reach_state(rsik_ctx *ctx, int64_t n, const double *const pose_soa[6], const uint8_t *arm, int arm_uniform,
                     int no_limits, double *solver_state, double *interval, uint8_t *reachable, uint8_t *state);
/* SymbolicIK.get_joints(theta, previous_joints) on stored state (symbolic_ik.py:697-863); updates the
 * row like the reference updates self.  previous_joints: [n,7] device or NULL for zeros.  joints / elbow may be NULL
 * (the row's slots 24-30 / 16-18 carry them too). */
int rsik_joints_from_state(rsik_ctx *ctx, int64_t n, double *solver_state, const uint8_t *arm, int arm_uniform,
                           const double *theta, const double *previous_joints, double *joints, double *elbow);
/* SymbolicIK.get_elbow_position(theta) on stored state (symbolic_ik.py:684-695). */
int rsik_elbow_from_state(rsik_ctx *ctx, int64_t n, const double *solver_state, const double *theta, double *elbow);

/*
 * rsik_theta_from_joints — "which theta puts this arm nearest to these joints", for n independent rows (n robots, n planner seeds,
 * n restarted trajectories): what every caller of the reference does when it starts or restarts an arm (ControlIK.__init__
 * control_ik.py:142-158, the continuous start-up :306-325).  Per row: SymbolicIK.is_reachable_no_limits on the goal
 * (symbolic_ik.py:85-119), then utils.get_best_theta_to_current_joints (utils.py:267-331) with the reference's own sequence of
 * get_joints evaluations — the preferred theta first (within 0.01 of the joints: that theta is the answer), then the ternary
 * search over [-pi, pi] (r) / [0, 2 pi] (l), two evaluations per iteration, and one more at the mid point of the last bracket;
 * each evaluation moves the row's solver state where the elbow projection fires, as the reference's does.  The result is the
 * theta a timed-out rsik_control_continuous_step finds for the same current pose and joints, bit for bit.
 *
 *   goal_kind / goal_soa   RSIK_GOAL_POSE6: 6 device arrays of n doubles (the layout of rsik_solve); RSIK_GOAL_M12: 12 (the layout
 *                          of rsik_control_discrete; RSIK_OPT_EULER_ROUNDTRIP applies as there) — the pose the arm is in
 *   arm / arm_uniform      as rsik_solve
 *   current_joints         [n,7] device, row-major: the joints each arm measured
 *   preferred_theta_host   2 doubles (host): the preferred theta of r and of l (they differ: control_ik.py:136-140), used as given
 *   theta                  [n]: the theta found
 *   joints                 [n,7] or NULL: the joints of the last evaluation (utils.py:324; the preferred theta's for a shortcut row)
 *   bracket                [n,2] or NULL: the search's final low, high (the reference's returned text carries them); NaN for a
 *                          shortcut row
 *   distance               [n] or NULL: the search's objective at the returned theta — the norm of the seven angle_diffs between the
 *                          returned joints and current_joints — so that a caller can refuse a poor match
 *   state                  [n] uint8 or NULL: RSIK_STATE_REACHABLE; RSIK_STATE_NOT_REACHABLE_NO_LIMITS where is_reachable_no_limits
 *                          fails (outputs NaN); RSIK_STATE_INVALID_INPUT where the goal or the row's current joints hold a NaN or an
 *                          infinity (outputs NaN, no other row is touched: "Rows that are not numbers" above)
 * n == 0 launches nothing.  Enqueued on the context's stream; never waits for the device.
 */
int rsik_theta_from_joints(rsik_ctx *ctx, int64_t n, int goal_kind, const double *const *goal_soa, const uint8_t *arm,
                           int arm_uniform, const double *current_joints, const double *preferred_theta_host, double *theta,
                           double *joints, double *bracket, double *distance, uint8_t *state);
/* The drop-in call shape: utils.get_best_theta_to_current_joints(get_joints, ...) with the bound get_joints of a solver object.
 * Runs the same search on stored solver-state rows (as rsik_joints_from_state does, after rsik_reach_state) and leaves each row
 * as the reference leaves `self` after those get_joints calls: slots 0-2 and 6-8 moved by every projection that fired, slots
 * 16-19 and 24-30 of the last evaluation.  current_joints is [n, n_current], n_current = 7, or 14 for the list-of-both-arms form
 * ControlIK.__init__ hands over (control_ik.py:152-158: joints 0 and 1 are compared against all seven entries of the r list and
 * of the l list).  theta [n]; bracket [n,2] or NULL.  Works on pinned host rows like the other state entry points. */
int rsik_theta_from_joints_state(rsik_ctx *ctx, int64_t n, double *solver_state, const uint8_t *arm, int arm_uniform,
                                 const double *current_joints, int n_current, const double *preferred_theta_host,
                                 double *theta, double *bracket);

/* utils.get_euler_from_homogeneous_matrix for a batch (utils.py:84-90): goal matrices (m12_soa, layout as
 * rsik_control_discrete) -> pose_soa = 6 device arrays px,py,pz,roll,pitch,yaw (the input layout of rsik_solve),
 * Euler angles = Rotation.from_matrix(M[:3,:3]).as_euler("xyz").  identity_shortcut != 0 adds ControlIK's
 * np.allclose(M[:3,:3], I) => [0,0,0] (control_ik.py:212-214).  A block that is no rotation: its nearest rotation's angles for a
 * determinant > 0, NaN angles (the position passed through) for a determinant <= 0, where SciPy raises ValueError — "Goal
 * matrices that are not rotations" above. */
int rsik_matrix_to_pose(rsik_ctx *ctx, int64_t n, const double *const m12_soa[12], int identity_shortcut,
                        double *const pose_soa[6]);

/* Forward kinematics of the arm: the chain SymbolicIK.get_joints inverts (symbolic_ik.py:728-848):
 * joints [n,7] -> goal position [n,3] and goal rotation [n,9] (row-major), torso frame.  Either output may be NULL.
 * The reference has no FK (its examples use placo/reachy2_sdk for that, src/example/test_dk.py); this is the
 * self-contained monitor of SURVEY 8 f-4. */
int rsik_forward_kinematics(rsik_ctx *ctx, int64_t n, const double *joints, const uint8_t *arm, int arm_uniform,
                            double *position, double *rotation);
/* FK(joints) against the goal it was solved for: err[n,2] = (|position error| in m, rotation error in rad).
 * goal_soa: 6 columns (px,py,pz,roll,pitch,yaw) for RSIK_GOAL_POSE6, 12 columns (R row-major, t) for RSIK_GOAL_M12.
 * Rows whose joints are NaN (unreachable poses) give NaN. */
int rsik_fk_residual(rsik_ctx *ctx, int64_t n, int goal_kind, const double *const *goal_soa, const double *joints,
                     const uint8_t *arm, int arm_uniform, double *err);

/*
 * rsik_jacobian — how the goal frame moves when the joints move: the 6 x 7 geometric Jacobian of the chain rsik_forward_kinematics
 * evaluates, the arm's self-motion vector and Yoshikawa's manipulability, for n rows of joints (added within ABI version 8: one symbol,
 * no option, no workspace).  The reference has none of the three (like FK: its users take them from placo or the SDK).
 *
 *   joints           [n_rep][n][7] device, row-major: seven joints per row in the convention rsik_solve returns and
 *                    rsik_forward_kinematics reads.  n_rep >= 1; n_rep == 1 is the plain [n,7] form, n_rep > 1 takes the sample-major
 *                    joints of rsik_solve_sweep ([n_theta][n][7]) and the waypoint-major joints of rsik_solve_path in place.
 *   arm / arm_uniform  as rsik_forward_kinematics (arm: [n], one byte per row, shared by every repetition, or NULL)
 *   jacobian         [n_rep][n][6][7] or NULL.  Column k is the velocity of the goal frame per unit rate of joint k, in the torso
 *                    frame: rows 0-2 d position / d q_k for the position rsik_forward_kinematics returns (the goal-frame origin, tip
 *                    offset RSIK_C_TIPL included, not the wrist), rows 3-5 the angular velocity w_k, d R / d q_k = [w_k]x R for the
 *                    rotation it returns.  The signs are those of the caller's joints: joint 2 (elbow yaw) turns about -x of the upper
 *                    arm and joint 6 about the goal's own z, as the chain has them.
 *   null_vector      [n_rep][n][7] or NULL: the signed maximal minors of J, null[i] = (-1)^i det(J without column i) — the generalised
 *                    cross product of J's six rows, so J . null = 0, the sign is defined and the vector is continuous in the joints.
 *                    It is NOT normalised and goes to the zero vector at a singularity (a straight elbow, joints[3] == 0) instead of to
 *                    an arbitrary direction.  Away from singularities, where neither the elbow projection nor the elbow-limit clamp of
 *                    the solve is active, it is parallel to d joints / d theta of rsik_solve: with the sign the tests record for both
 *                    arms, null . d joints / d theta < 0 (the vector points the way a DEcreasing theta moves the arm).
 *   manipulability   [n_rep][n] or NULL: sqrt(sum null[i]^2) = sqrt(det(J J^T)) (Cauchy-Binet), without forming J J^T, which
 *                    would lose half the digits near a singularity; 0, not NaN, at a singular row.
 * Any output may be NULL, and the bits of an output do not depend on which others were requested.  A row with a NaN or an infinity
 * among its joints gives NaN in every output of that row and changes no other row ("Rows that are not numbers" above); a finite
 * angle of any size is answered like the angle of [-pi, pi] it is congruent to, to 1e-9.
 * n == 0 launches nothing; n < 0, n_rep < 1, joints == NULL or all three outputs NULL give RSIK_E_INVALID, the arm checks and their
 * codes are rsik_forward_kinematics' (RSIK_E_NOT_SET included).  Enqueued on the context's stream; allocates nothing and never waits
 * for the device.
 */
int rsik_jacobian(rsik_ctx *ctx, int64_t n, int64_t n_rep, const double *joints, const uint8_t *arm, int arm_uniform,
                  double *jacobian, double *null_vector, double *manipulability);

/*
 * rsik_joint_rates — the joint rates that give the goal frame a wanted twist: the damped least-squares solve on the Jacobian of
 * rsik_jacobian, for n rows, from one launch in which the Jacobian never leaves the registers (added within ABI version 8: one
 * symbol, no option, no workspace).  Resolved-rate teleoperation, velocity feed-forward beside the continuous mode, the Newton step
 * of a trajectory optimiser.  The reference has nothing of the kind.
 *
 *   joints, n_rep, arm / arm_uniform   exactly as rsik_jacobian: joints [n_rep][n][7], arm [n] shared by every repetition or NULL;
 *                    n_rep > 1 takes a sweep's or a path's joints in place
 *   twist            [n_rep][n][6] device, in the row order of the Jacobian: entries 0-2 the linear velocity of the goal-frame origin,
 *                    entries 3-5 the angular velocity, torso frame
 *   damping_host     lambda for every row when damping == NULL: finite and > 0 (and its square a normal double: 1.5e-154 < lambda <
 *                    1.3e154), otherwise RSIK_E_INVALID.  Not read when damping is given.
 *   damping          [n_rep][n] device or NULL: lambda per row, e.g. derived with torch from rsik_jacobian's manipulability
 *   bias_rates       [n_rep][n][7] device or NULL for zeros: the rates q0 the arm would like to have — joint centring, or a
 *                    self-motion command such as k * null_vector
 *   rates            [n_rep][n][7] or NULL
 *   achieved_twist   [n_rep][n][6] or NULL: J . rates, which differs from twist by the damping
 * Definition, per row, with J the Jacobian rsik_jacobian defines for that row:
 *     rates = argmin over q' of  |J q' - twist|^2 + lambda^2 |q' - q0|^2,
 * computed as rates = q0 + J^T y with (J J^T + lambda^2 I) y = twist - J q0.  The 6 x 6 system is solved by an L D L^T factorisation
 * (Cholesky without square roots) in natural order, every sum in a fixed order.  Every pivot is clamped from below at lambda^2: the
 * exact pivots are Schur complements of J J^T, which is positive semi-definite, plus lambda^2, so they are never smaller and the clamp
 * never changes an exact result; it is what makes a finite row give finite outputs at a straight elbow and with a tiny lambda, where
 * rounding alone could produce a pivot of zero or below.
 * lambda = 0 is not offered: lambda = 1e-6 is the pseudo-inverse solution to every digit that survives the solve (the two differ by
 * lambda^2 / sigma^2 relative, 1e-12 / sigma^2, below what the conditioning of J J^T leaves), and it stays defined at a singularity,
 * where the pseudo-inverse is not.
 * Either output may be NULL, both NULL is RSIK_E_INVALID; the bits of one do not depend on whether the other was requested.  A NaN or
 * an infinity among the row's joints, twist or bias, or a damping entry that is NaN, infinite or <= 0, makes every output of that
 * row NaN and changes no other row ("Rows that are not numbers" above); a finite angle of any size is answered like the angle of
 * [-pi, pi] it is congruent to.
 * n == 0 launches nothing; n < 0, n_rep < 1, joints == NULL or twist == NULL give RSIK_E_INVALID, the arm checks and their codes are
 * rsik_jacobian's (RSIK_E_NOT_SET included).  Enqueued on the context's stream; allocates nothing and never waits for the device.
 */
int rsik_joint_rates(rsik_ctx *ctx, int64_t n, int64_t n_rep, const double *joints, const uint8_t *arm, int arm_uniform,
                     const double *twist, double damping_host, const double *damping, const double *bias_rates,
                     double *rates, double *achieved_twist);

/*
 * rsik_track — closed-loop tracking of goal trajectories at the velocity level: the loop a caller of rsik_joint_rates runs (forward
 * kinematics, pose error, twist, joint rates, one integration step), for n trajectories of n_steps goals each, from ONE launch in which
 * the joints never leave the registers (added within ABI version 8: one symbol, no option, no workspace).  It starts from any joints,
 * degrades gracefully where the analytic solve answers NaN (a goal out of reach, the wrist limit), obeys rate and joint limits, and is
 * continuous where the elbow projection makes the analytic answer jump.  The reference has nothing of the kind.
 *
 *   m12_steps        [n_steps][12][n] device, the layout of rsik_control_continuous_run (R row-major, then t): one buffer can feed
 *                    both.  The 3 x 3 block is consumed as it comes, without an Euler round trip and without a determinant test (as
 *                    RSIK_EULER_NEVER): it MUST be a rotation.
 *   arm / arm_uniform  as rsik_jacobian (arm: [n], one byte per trajectory, or NULL)
 *   start_joints     [n][7] device: where every trajectory starts.  NULL is RSIK_E_INVALID.
 *   dt, kp, ko       the integration step (finite, > 0) and the gains on the position and the orientation error (finite, >= 0)
 *   feedforward_steps  [n_steps][n][6] device, or NULL for zeros: a twist in the row order of the Jacobian, added to the feedback
 *   damping_host / damping   lambda of rsik_joint_rates, for every trajectory or [n] device, one per trajectory and constant over the
 *                    steps; the rules are rsik_joint_rates' (damping_host is not read when damping is given)
 *   rest_joints      [n][7] device or NULL: a posture the arm is drawn to in the null space; rest_gain (finite, >= 0) is not read when
 *                    rest_joints is NULL
 *   limits_host      21 doubles on the HOST, [3][7], or NULL for none: the rows are rate_max, q_min, q_max.  rate_max > 0 and
 *                    q_min <= q_max; +-infinity is allowed; a NaN is RSIK_E_INVALID.
 *   joints_steps     [n_steps][n][7] or NULL: the joints after every step
 *   rates_steps      [n_steps][n][7] or NULL: the rates of every step, after the rate limit
 *   err_steps        [n_steps][n][2] or NULL: (|position error| in m, rotation error in rad) every step saw, before it moved
 *   final_joints     [n][7] or NULL: the joints after the last step
 *   final_err        [n][2] or NULL: the error of the last goal at the joints after the last step
 * Definition, per trajectory: q := start_joints, then for t = 0 ... n_steps - 1
 *   1. (p, R) = rsik_forward_kinematics(q)
 *   2. e_p = p_g - p;  D = R_g R^T,  w = 1/2 (D21 - D12, D02 - D20, D10 - D01),  s = |w|,  c = 1/2 (tr D - 1),  angle = atan2(s, c),
 *      e_o = w (angle / s) where s^2 >= 2^-52, else e_o = w: the rotation vector of D.  At a rotation by pi the direction is undefined
 *      and e_o is close to 0 (s is): the loop does not turn towards such a goal until something else moves it off pi.
 *      err_steps[t] = (|e_p|, angle).
 *   3. v = feedforward[t] + (kp e_p, ko e_o)
 *   4. q0 = rest_gain (rest_joints - q), a plain difference (q is continuous along the run); 0 without rest_joints
 *   5. q' = exactly what rsik_joint_rates defines for (q, v, lambda, q0): L D L^T, pivot clamp, fixed order
 *   6. with limits: m = max_k |q'_k| / rate_max_k; if m > 1, q' := q' / m (one factor for all joints: the direction is kept)
 *   7. q := q + dt q'; with limits, clamped to [q_min, q_max] per joint
 *   8. rates_steps[t] = q' (after the limit), joints_steps[t] = q
 * final_joints is the last q; final_err is step 2 once more, for the last goal at the last q.
 * Any output may be NULL, all five NULL is RSIK_E_INVALID; the bits of an output do not depend on which others were requested, two
 * launches on the same inputs give the same bits, and a trajectory's bits depend neither on n nor on its neighbours.
 * A NaN or an infinity in a trajectory's start_joints or rest_joints row, or a damping that is not usable, makes every output of that
 * trajectory NaN and changes nothing else.  A step whose goal or feed-forward holds a NaN or an infinity is skipped: q is held,
 * joints_steps[t] = q, rates_steps[t] = 0, err_steps[t] = NaN, and the trajectory goes on from there with the bits of the same run
 * without that step; final_err is NaN if the last goal is such a goal.  A finite angle of any size is answered as rsik_jacobian
 * answers it.  A goal or a feed-forward that is finite but so large that the arithmetic overflows is not an error: a step whose
 * rates q' (step 5) do not come out finite is held like a skipped step (q held, rates_steps[t] = 0, err_steps[t] = NaN), with
 * and without limits, and err_steps[t][0] and final_err[0] are +infinity where |e_p|^2 overflows (|e_p| >= 1.34e154) on a step
 * that is taken.
 * n == 0 launches nothing; n < 0, n_steps outside 1 ... 65536, m12_steps == NULL, start_joints == NULL, all outputs NULL, a dt, gain,
 * damping_host or limit outside the above give RSIK_E_INVALID, the arm checks and their codes are rsik_jacobian's (RSIK_E_NOT_SET
 * included).  Enqueued on the context's stream; allocates nothing and never waits for the device.
 */
int rsik_track(rsik_ctx *ctx, int64_t n, int64_t n_steps, const double *m12_steps,
               const uint8_t *arm, int arm_uniform, const double *start_joints,
               double dt, double kp, double ko, const double *feedforward_steps,
               double damping_host, const double *damping,
               const double *rest_joints, double rest_gain, const double *limits_host,
               double *joints_steps, double *rates_steps, double *err_steps, double *final_joints, double *final_err);

/*
 * rsik_clearance — how far the arm is from a set of obstacles, which link and which obstacle are nearest, where, and how the distance
 * changes with the joints, for n rows of joints from one launch (added within ABI version 8: one symbol, no option, no workspace).
 * What a planner asks of the K elbow angles of a sweep ("which keep the arm off the table, the torso, the other arm?"), and what a
 * caller of rsik_joint_rates or rsik_track puts into bias_rates for obstacle avoidance in the null space.  The reference has nothing
 * of the kind.
 *
 * The arm is three capsules: link 0 shoulder -> elbow, link 1 elbow -> wrist, link 2 wrist -> goal origin (the position
 * rsik_forward_kinematics returns, RSIK_C_TIPL included), with the radii link_radius_host[0..2].  The end points are the origins of
 * the joints: joints 0, 1 at the shoulder, 2, 3 at the elbow, 4, 5, 6 at the wrist.
 *
 *   joints, n_rep, arm / arm_uniform   exactly as rsik_jacobian: joints [n_rep][n][7], arm [n] shared by every repetition or NULL;
 *                    n_rep > 1 takes a sweep's or a path's joints in place
 *   link_radius_host 3 doubles on the HOST, or NULL for zeros; each finite and >= 0, otherwise RSIK_E_INVALID
 *   n_spheres, spheres   0 ... 4096 rows [n_spheres][4] device, row-major: (x, y, z, r) in the torso frame
 *   n_capsules, capsules 0 ... 256 rows [n_capsules][7] device: (ax, ay, az, bx, by, bz, r); a == b is allowed (a sphere)
 *                    At least one obstacle in all; a count outside its range is RSIK_E_INVALID.  The obstacles are shared by every
 *                    row and every repetition.  Obstacle index o: spheres are 0 ... n_spheres - 1, capsule j is n_spheres + j.
 *   clearance        [n_rep][n] or NULL: the minimum, over the 3 links and all usable obstacles, of (distance between the link's axis
 *                    segment and the obstacle's axis segment or centre) - link radius - obstacle radius.  The distance is the true
 *                    minimum of |x - y| over the two segments.  Negative: the radii penetrate; touching AXES give -(r_link + r_obs).
 *                    An axis distance below 1.1e-136 m counts as touching.
 *   nearest          [n_rep][n][2] int32 or NULL, aligned to 8 bytes: (link, obstacle index) of the pair that gives the minimum.
 *                    Pairs are compared on the clearance as computed; the first minimum wins in the order (obstacle 0, link 0),
 *                    (obstacle 0, link 1), (obstacle 0, link 2), (obstacle 1, link 0) ...
 *   witness          [n_rep][n][2][3] or NULL: x on the link's axis and y on the obstacle's axis for the winning pair, a pair that
 *                    attains the distance (not unique for parallel segments)
 *   gradient         [n_rep][n][7] or NULL: d clearance / d joints of the winning pair, g_k = u . (a_k x (x - o_k)) for the joints that
 *                    move the link (0-1 for link 0, 0-3 for link 1, 0-6 for link 2) and 0 for the others, with a_k, o_k the axis and
 *                    origin of joint k as in rsik_jacobian and u = (x - y) / |x - y|.  Where the axes touch it is the zero vector.
 *                    k * gradient as bias_rates of rsik_joint_rates or rsik_track moves the arm away in the null space.
 *   link_points      [n_rep][n][4][3] or NULL: shoulder, elbow, wrist, goal origin — for drawing, and what a caller turns into the
 *                    three capsules of this arm as obstacles for the other one
 * Any output may be NULL, all five NULL is RSIK_E_INVALID.  The bits of an output depend neither on which others were requested, nor
 * on n, n_rep or the arm form; clearance does not depend on the order of the obstacles; two launches give the same bits.
 * A row with a NaN or an infinity among its joints gives NaN outputs and nearest (-1, -1) and changes no other row.  An obstacle whose
 * row holds a NaN or an infinity, or a negative radius, is skipped: it is never the nearest and changes nothing else.  If every
 * obstacle is skipped: clearance +infinity, nearest (-1, -1), gradient 0, witness NaN.  A finite angle of any size is answered as
 * rsik_jacobian answers it.
 * n == 0 launches nothing; n < 0, n_rep < 1, joints == NULL, a NULL obstacle array with a count above 0 give RSIK_E_INVALID, the arm
 * checks and their codes are rsik_jacobian's (RSIK_E_NOT_SET included).  Enqueued on the context's stream; allocates nothing, needs no
 * workspace and never waits for the device.
 */
int rsik_clearance(rsik_ctx *ctx, int64_t n, int64_t n_rep, const double *joints, const uint8_t *arm, int arm_uniform,
                   const double *link_radius_host,
                   int n_spheres, const double *spheres, int n_capsules, const double *capsules,
                   double *clearance, int32_t *nearest, double *gradient, double *witness, double *link_points);

/*
 * rsik_track_avoid — rsik_track with obstacle avoidance inside the loop: at every step the clearance of the joints the loop has
 * reached against a static set of obstacles (what rsik_clearance computes), and, where it is below an influence distance, its joint
 * gradient as a push in the bias of the damped least-squares rates — the null-space avoidance that rsik_clearance's gradient is for,
 * at the joints that exist only inside the launch (added within ABI version 8: one symbol, no option, no workspace).  The reference
 * has nothing of the kind.
 *
 * Every argument rsik_track has means what it means there: the layouts, the rules for damping, rest_joints and limits_host, what is
 * not a number, skipped and held steps, the refusals.  The new ones:
 *   link_radius_host, n_spheres, spheres, n_capsules, capsules   exactly as rsik_clearance, with smaller counts: 0 ... 256 spheres and
 *                    0 ... 64 capsules, at least one obstacle in all (without obstacles the call to make is rsik_track); anything
 *                    else is RSIK_E_INVALID.  The obstacles are static: shared by every trajectory and every step.  A row with a
 *                    NaN, an infinity or a negative radius is skipped, as there.
 *   influence        finite, >= 0, in m: the push acts where the clearance is below it
 *   avoid_gain       finite, >= 0: rad/s of bias per metre of (influence - clearance) and unit of gradient
 *   clearance_steps  [n_steps][n] or NULL: the clearance every step saw, before it moved
 *   nearest_steps    [n_steps][n][2] int32 or NULL, aligned to 8 bytes: (link, obstacle index) of that clearance
 *   min_clearance    [n] or NULL: the minimum of clearance_steps[0 ... n_steps - 1] and of the clearance at the final joints; +infinity
 *                    if every obstacle is skipped
 * Definition, per trajectory and step: steps 1-3 and 5-8 are rsik_track's, word for word; step 4 is
 *   4a. (d, link, obstacle, g) = clearance, nearest and gradient as rsik_clearance defines them for the current q (pair order, first
 *       minimum, skipped obstacles: the same).  clearance_steps[t] = d, nearest_steps[t] = (link, obstacle).  They depend on q alone
 *       and are written on a skipped or held step too, with the held q.
 *   4b. q0 = rest_gain (rest_joints - q), or 0 without rest_joints.  Where d < influence: a = avoid_gain (influence - d) and
 *       q0_k := q0_k + a g_k (a product, then a sum).  Where d >= influence, or no obstacle is usable (d = +infinity), q0 is left
 *       alone: a select, not a multiplication by zero.
 * Step 5 is rsik_joint_rates' rates for (q, v, lambda, q0), as before.  The push is a bias, not a constraint: the damped solve weighs
 * it against the twist with lambda^2, so it moves the arm in the null space of the task first and gives way to the task elsewhere.
 * min_clearance costs one more pass over the obstacles, after the last step, and only when it is asked for.
 * Any output may be NULL, all eight NULL is RSIK_E_INVALID.  Beyond what rsik_track states of its outputs (any subset, n, the
 * neighbours, two launches: the same bits): clearance_steps[t] and nearest_steps[t] are bit for bit what rsik_clearance returns for
 * the joints before step t (start_joints, then joints_steps[t - 1]) with the same obstacles and radii, and a trajectory on which the
 * push never acts has rsik_track's bits in the five outputs the two share (where neither a rest posture nor a push is there the
 * bias is left out of the solve, as rsik_track leaves it out; the sign of a zero is the one place where the two could ever differ).
 * A trajectory that is NaN (start_joints, rest_joints, damping) is NaN in every double output and (-1, -1) in nearest_steps.
 * n == 0 launches nothing; the refusals of rsik_track, a count outside its range, no obstacle, a NULL obstacle array with a count
 * above 0, an influence, avoid_gain or link radius that is negative or not finite, a nearest_steps that is not aligned give
 * RSIK_E_INVALID; the arm checks and their codes are rsik_jacobian's (RSIK_E_NOT_SET included).  Enqueued on the context's stream;
 * allocates nothing and never waits for the device.
 */
int rsik_track_avoid(rsik_ctx *ctx, int64_t n, int64_t n_steps, const double *m12_steps,
                     const uint8_t *arm, int arm_uniform, const double *start_joints,
                     double dt, double kp, double ko, const double *feedforward_steps,
                     double damping_host, const double *damping,
                     const double *rest_joints, double rest_gain, const double *limits_host,
                     const double *link_radius_host,
                     int n_spheres, const double *spheres, int n_capsules, const double *capsules,
                     double influence, double avoid_gain,
                     double *joints_steps, double *rates_steps, double *err_steps,
                     double *clearance_steps, int32_t *nearest_steps,
                     double *final_joints, double *final_err, double *min_clearance);

/*
 * rsik_track_pair — rsik_track_avoid for n_pairs robots of two arms that avoid each other: both arms of a robot are tracked in the
 * same launch, and at every step each arm has, beside the static obstacles, the other arm's three links as capsules, at the joints
 * the other arm has reached at that step — joints that exist only inside the launch (added within ABI version 8: one symbol, no
 * option, no workspace).  The reference has nothing of the kind.
 *
 * Rows: there are n = 2 n_pairs rows; row 2i is the right arm of robot i (RSIK_ARM_R), row 2i + 1 its left arm (RSIK_ARM_L).  Every
 * array has exactly rsik_track_avoid's layout for n rows (m12_steps [n_steps][12][n], start_joints [n][7], feedforward_steps
 * [n_steps][n][6], damping [n], rest_joints [n][7], the eight outputs), so one set of buffers can feed rsik_track_avoid with the arm
 * bytes 0, 1, 0, 1, ... and then this call.  There is no arm argument; both arms' constants must be set (rsik_set_arm), otherwise
 * RSIK_E_NOT_SET.  Both arms live in the torso frame, as their RSIK_C_SHOULDER constants say.  Every other argument means what it
 * means in rsik_track_avoid, with one difference:
 *   n_spheres, spheres, n_capsules, capsules   0 ... 256 spheres and 0 ... 64 capsules; NO static obstacle is allowed here, because the
 *                    partner is always an obstacle
 * Definition, per row and step: steps 1-3 and 5-8 are rsik_track's, word for word; step 4b is rsik_track_avoid's, word for word;
 * step 4a is rsik_clearance's minimum, nearest pair and gradient over a longer list of obstacles:
 *     the spheres, indices 0 ... n_spheres - 1; the capsules, indices n_spheres ... n_spheres + n_capsules - 1; then the partner's
 *     three links as capsules, indices n_spheres + n_capsules + l for l = 0, 1, 2.
 *   The partner's link l is the capsule (P_l, P_{l+1}, link_radius_host[l]), P the partner's link_points as rsik_clearance returns
 *   them for the partner's joints BEFORE step t: both arms look at each other's state before the step, so the order of the arms does
 *   not matter.  Its direction is P_{l+1} - P_l, formed from those two points as a capsule's is from its row.  Pair order and "first
 *   minimum wins" are unchanged, the partner's links come last.  The gradient is with respect to the row's own joints only: the
 *   partner counts as standing still during the step.
 * clearance_steps[t] and nearest_steps[t] are therefore bit for bit what rsik_clearance returns for the row's joints before step t
 * with the static spheres, and the static capsules followed by those three, as its obstacles; on a held step of the partner they
 * see the held partner.  min_clearance includes the partner at the final joints.
 * A partner that is not numbers (a NaN or an infinity in its start_joints or rest_joints row, an unusable damping) is NaN in its own
 * outputs, as in rsik_track_avoid, and its three capsules are skipped exactly like an obstacle row that holds a NaN: never the
 * nearest, and they change nothing else.  The live arm then has rsik_track_avoid's bits for the same static scene; without a static
 * scene its clearance is +infinity, its nearest (-1, -1), and the five outputs it shares with rsik_track have rsik_track's bits.
 * Any output may be NULL, all eight NULL is RSIK_E_INVALID.  Any subset of the outputs gives the same bits, two launches give the
 * same bits, and a pair's bits depend neither on n_pairs, nor on its place in the launch, nor on the other pairs.
 * n_pairs == 0 launches nothing; n_pairs < 0 is RSIK_E_INVALID, and so is everything rsik_track_avoid refuses apart from "no
 * obstacle": n_steps outside 1 ... 65536, a count outside its range, m12_steps == NULL, start_joints == NULL, a NULL obstacle array
 * with a count above 0, a dt, gain, damping_host, limit, influence, avoid_gain or link radius outside its range, a nearest_steps that
 * is not aligned to 8 bytes.  Enqueued on the context's stream; allocates nothing and never waits for the device.
 */
int rsik_track_pair(rsik_ctx *ctx, int64_t n_pairs, int64_t n_steps, const double *m12_steps,
                    const double *start_joints,
                    double dt, double kp, double ko, const double *feedforward_steps,
                    double damping_host, const double *damping,
                    const double *rest_joints, double rest_gain, const double *limits_host,
                    const double *link_radius_host,
                    int n_spheres, const double *spheres, int n_capsules, const double *capsules,
                    double influence, double avoid_gain,
                    double *joints_steps, double *rates_steps, double *err_steps,
                    double *clearance_steps, int32_t *nearest_steps,
                    double *final_joints, double *final_err, double *min_clearance);

/*
 * rsik_clearance_edges — the clearance of a path ALONG the motion between its waypoints: rsik_solve_path_clear and rsik_solve_path_pair
 * keep min_clearance at the waypoints only, and say nothing of the way from one winner to the next.  That motion is the one their
 * transition cost assumes: joint by joint, the short way round (angle_diff).  One call takes a path's joints in place, samples every
 * edge at n_sub + 1 sub-steps and returns, per edge, the least clearance, where it lies, the pair that gives it and a certified lower
 * bound on the clearance of the whole continuous motion; per path, the minima of these.  What a caller otherwise composes from an
 * interpolation of its own, rsik_clearance with n_rep = n_sub + 1 over (n_sub + 1) * n_steps * n rows, and two reductions.  Added
 * within ABI version 8: two new symbols, no new option, nothing else changed.  The reference has nothing of the kind.
 *
 *   joints           [n_steps][n][7] device, waypoint-major: the `joints` output of rsik_solve_path, rsik_solve_path_clear or
 *                    rsik_solve_path_pair (rows 2 i, 2 i + 1 are paths of their own here), with or without RSIK_PATH_UNWIND, or
 *                    joints_steps of the track calls.  n >= 0, n_steps 1 ... 65536.
 *   arm / arm_uniform   [n], one byte per path, or NULL and the one arm: as rsik_solve_path
 *   start_joints     [n][7] device or NULL: the joints each path starts from
 *   n_sub            S, 1 ... 256: the sub-steps of an edge
 *   link_radius_host, n_spheres, spheres, n_capsules, capsules
 *                    as rsik_solve_path_clear: 0 ... 256 spheres and 0 ... 64 capsules, at least one obstacle, 3 radii on the host or
 *                    NULL for zeros.  An obstacle row with a NaN, an infinity or a negative radius is skipped.
 *   min_clearance    m, finite, or -infinity for none: it feeds n_below and first_below, nothing else
 *   workspace        device, aligned to 8 bytes, at least rsik_clearance_edges_workspace_bytes(n, n_steps) bytes: needed only when one
 *                    of the five per-path outputs is asked for; otherwise it may be NULL
 *
 * Definition, independent of the kernel's layout:
 *   Waypoints and edges.  A row of `joints` with a NaN or an infinity is NOT A WAYPOINT: this is how the path calls mark a skipped
 *   one.  The edge INTO waypoint (t, i) starts at a, the last waypoint of path i before t, or start_joints[i] for the path's first
 *   waypoint, and ends at b = row (t, i): step_cost's rule.  The first waypoint of a path without start_joints has the one-sample edge
 *   {b}, numbered s = S.
 *   Samples.  delta_k = angle_diff(b_k, a_k), the value RSIK_STAGE_ANGLE_DIFF returns.  Sample s has q_k(s) = a_k + delta_k * (s / S)
 *   for s = 0 ... S - 1: s / S is one division, then a product, then a sum, unfused.  q(S) = b itself (a select: both ends of an edge
 *   are the rows as given).  d(s) and its (link, obstacle) are, bit for bit, what rsik_clearance returns for q(s): the same arm, radii
 *   and obstacles, the same order of the pairs, the first minimum, finite angles of any size.
 * Per edge, [n_steps][n], any of them NULL:
 *   edge_clearance   the minimum over s of d(s)
 *   edge_sub         int32: the lowest s that attains it
 *   edge_nearest     [n_steps][n][2] int32, aligned to 8 bytes: (link, obstacle index) of that sample
 *   edge_bound       edge_clearance - 0.5 * (acc / S), with acc = sum over k of |delta_k| * R_k, k = 0 ... 6 in this order, unfused,
 *                    R_0 = R_1 = u + f + |tip|, R_2 = R_3 = f + |tip|, R_4 = R_5 = R_6 = |tip|; u = RSIK_C_UPPER_ARM, f =
 *                    RSIK_C_FOREARM, |tip| the length of RSIK_C_TIPL, of the path's arm.  acc = 0 for a one-sample edge.
 *   Where row t is not a waypoint: NaN, -1, (-1, -1), NaN.  Where every obstacle is skipped: +infinity, the edge's first s, (-1, -1),
 *   +infinity.
 * Why edge_bound is a lower bound.  Joint k turns every point beyond it about an axis through its origin — joints 0, 1 at the
 * shoulder, 2, 3 at the elbow, 4 - 6 at the wrist — and no point of the arm's axis (shoulder - elbow - wrist - goal origin) is
 * further from that origin than R_k.  Between two neighbouring samples joint k turns by |delta_k| / S, so no point of the axis moves
 * more than acc / S, and every configuration between them is within acc / (2 S) of the nearer sample.  The distance between a point
 * set and the obstacles is 1-Lipschitz in that displacement.  Hence the clearance of the continuous motion is never below edge_bound,
 * up to the rounding of d and of the bound's own few operations.  An edge_bound above 0 proves the edge free; one below 0 with an
 * edge_clearance above 0 asks for a finer n_sub.
 * Per path, [n], any of them NULL:
 *   path_clearance   the minimum of edge_clearance over the path's edges
 *   path_edge        [n][2] int32, aligned to 8 bytes: (t, s) of that minimum, the lowest t among equal values
 *   path_bound       the minimum of edge_bound
 *   n_below          int32: the edges with edge_clearance < min_clearance
 *   first_below      int32: the lowest such t, or -1
 *   A path without a waypoint: NaN, (-1, -1), NaN, 0, -1.
 * A start_joints row that holds a NaN or an infinity loses its own path, as in rsik_solve_path: every edge output of the path is as
 * for "not a waypoint", its path outputs as for a path without one.  It changes no other path.
 *
 * Guarantees: any output may be NULL, all nine NULL is RSIK_E_INVALID.  Any subset of the outputs gives the same bits, and two
 * launches give the same bits.  A path's bits depend neither on n, nor on its place in the launch, nor on the other paths.
 * edge_clearance and the bounds do not depend on the order of the obstacles; edge_nearest's obstacle index does.
 *
 * RSIK_E_INVALID, nothing written: n < 0; n_steps or n_sub outside its range; a count outside its range, or no obstacle; a link
 * radius that is negative or not finite; a min_clearance that is a NaN or +infinity; then, for n > 0: joints == NULL or all nine
 * outputs NULL; a NULL obstacle array with a count above 0; an edge_nearest or path_edge that is not aligned to 8 bytes; with a
 * per-path output, a workspace that is NULL, too small or not aligned to 8 bytes.  The arm checks and their codes are rsik_jacobian's
 * (RSIK_E_NOT_SET included).  rsik_clearance_edges_workspace_bytes refuses n < 0, n_steps outside its range, bytes == NULL and a
 * product that does not fit; it grows with n and with n_steps.
 * n == 0 launches nothing.  Enqueued on the context's stream — the per-edge kernel, then, where a per-path output is asked for, a
 * second small one behind it —; allocates nothing and never waits for the device.
 */
int rsik_clearance_edges_workspace_bytes(int64_t n, int64_t n_steps, size_t *bytes);
int rsik_clearance_edges(rsik_ctx *ctx, int64_t n, int64_t n_steps, const double *joints,
                         const uint8_t *arm, int arm_uniform, const double *start_joints, int n_sub,
                         const double *link_radius_host,
                         int n_spheres, const double *spheres, int n_capsules, const double *capsules,
                         double min_clearance, void *workspace, size_t workspace_bytes,
                         double *edge_clearance, int32_t *edge_sub, int32_t *edge_nearest, double *edge_bound,
                         double *path_clearance, int32_t *path_edge, double *path_bound, int32_t *n_below, int32_t *first_below);

/*
 * Multi-GPU.  Poses are independent, so a job is sharded across the GPUs of a node — one process and one
 * rsik context per GPU — with no data-path collective; the only exchange is the all-gather of the final arrays
 * (joints [n,7], state [n]) over RCCL / xGMI.  The reference has nothing distributed (single-threaded Python).  Python
 * hosts use torch.distributed (backend "nccl" = RCCL, reachy2_symbolic_ik_amd/distributed.py); these four entry points
 * give a C host the same step without linking RCCL itself (librccl.so is opened with dlopen on first use).
 *   rsik_comm_unique_id   fills 128 bytes (ncclUniqueId) on ONE rank; the host carries them to the others
 *   rsik_comm_init_rank   collective over all ranks: creates this rank's communicator on the context's GPU
 *   rsik_allgather        every rank contributes bytes_per_rank bytes at `send`; rank r's block lands at
 *                         recv + r * bytes_per_rank on every rank (send may be recv + rank * bytes_per_rank: in place).
 *                         Enqueued on the context's stream like the kernels; device pointers.
 */
int rsik_comm_unique_id(void *id128);
int rsik_comm_init_rank(rsik_ctx *ctx, int nranks, int rank, const void *id128, void **comm);
int rsik_comm_destroy(rsik_ctx *ctx, void *comm);
int rsik_allgather(rsik_ctx *ctx, void *comm, const void *send, void *recv, size_t bytes_per_rank);

/* Test hook: evaluates the kernels' own elementary functions (csrc/rsik_math.hpp) on device arrays so their
 * accuracy can be measured against the host libm.  op: 0 reciprocal, 1 sqrt (out0, out1 two variants),
 * 2 reciprocal sqrt, 3 atan2(a, b), 4 sincos(a) -> out0 = sin, out1 = cos, 5 out0 = a mod 2pi (Python
 * semantics), out1 = angle_diff(a, b) (utils.py:486-490), 6 fp64 FMA issue-rate calibration (8 x 2048 dependent fma per element, scripts/valu_peak.py),
 * 7 the solve path's table atan2 of a UNIT vector: out0 = atan2(a, b) for a^2 + b^2 = 1,
 * 8 clock monitor: n waves each wait a[0] ticks of the 100 MHz counter (clamped to 5 s); out0[w] = shader-clock ticks,
 *   out1[w] = 100 MHz ticks that passed (core clock = out0 / out1 x 100 MHz); run it on a side stream beside a load.
 * 9-19 the widths at which the kernels evaluate N of these in lock step (ops 3, 4 and 7 are width 1): 9, 10, 11, 12 the
 *   unit-vector atan2 of op 7 at N = 2, 3, 4, 7; 13, 14, 15, 16 the atan2 of op 3 at N = 2, 3, 4, 7; 17, 18, 19 the sincos
 *   of op 4 at N = 2, 3, 4.  Element i is slot i mod N of group i / N; a ragged last group is padded with (0, 1) / 0.
 * Not part of the reference surface. */
int rsik_debug_math(rsik_ctx *ctx, int op, int64_t n, const double *a, const double *b, double *out0, double *out1);

#ifdef __cplusplus
}
#endif
#endif /* RSIK_H */
