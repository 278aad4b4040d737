/*
 * lpvmpc.h -- C ABI of liblpvmpc.so: batched LPV-MPC / LPV-MPP solve path on MI355X (gfx950).
 *
 * The reference (euge2838/Autonomous-Racing-LPV-MPP-MPC) has no FFI for this path: its boundary is
 * two Python classes that call numpy/scipy and the third-party OSQP wheel.  Each entry point below
 * names the reference interface it replaces (paths relative to workspace/src/barc/src):
 *   CTRL = ControllerObject/PathFollowingLPVMPC.py     PLAN = PlannerObject/LPV_MPC_Planner.py
 *   UTIL = Utilities/utilities.py                      TRACK = Utilities/trackInitialization.py
 *
 * Conventions
 *   - plain C, no exceptions across the boundary; every int-returning call gives 0 on success or a
 *     negative LPVMPC_E_* code, and lpvmpc_last_error() returns a message for the last failure;
 *   - all arrays are float64, row-major ("C order"), instance-major: [B][...]; a batch call with B = 0 is a no-op
 *     that returns LPVMPC_OK (fleet engines need B >= 1);
 *   - the caller owns every buffer; nothing passed in is retained after the call returns;
 *   - one handle per (device, stream); a handle is not thread-safe, different handles are;
 *   - a process that drives SEVERAL streams should export GPU_MAX_HW_QUEUES (the HIP runtime's number of hardware queues, default 4, read
 *     once when the runtime initialises) before anything touches HIP: streams that share a hardware queue run in order, so a launch
 *     holding a slow instance blocks its queue's other streams (configs[1]: 1.3 M solves/s with 8 queues, 2.4 M with 16; with straggler
 *     deferral four streams on four queues reach 4.1 M; beyond ~20 queues the hardware time-slices).  The library does not set it: it is
 *     the process's to choose (bench.py sets 2);
 *   - there is NO CPU fallback: without a usable HIP device every compute call fails with
 *     LPVMPC_E_NODEVICE.
 *
 * Decision vector per instance: z = [x_0 .. x_N, u_0 .. u_{N-1}]  (CTRL:479-492, PLAN:434-445)
 *   controller nx = 6  [vx vy wz epsi s ey]   (CTRL:712-718)
 *   planner    nx = 5  [vx vy wz ey epsi]     (PLAN:288-292)
 *   inputs     nu = 2  [delta a]
 */
#ifndef LPVMPC_H
#define LPVMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LPVMPC_VERSION 200            /* 0.2.0: round 5 removed the lpvmpc_lane_* exports (an ABI break), round 6 adds lpvmpc_defer_stats and kernel_variant 9;
                                         the lpvmpc_observer_* additions are backward compatible and keep the value, which tests/test_cabi.py pins */

#define LPVMPC_KIND_CONTROLLER 0      /* PathFollowingLPV_MPC  (CTRL:30-258) */
#define LPVMPC_KIND_PLANNER    1      /* LPV_MPC_Planner       (PLAN:29-320) */

#define LPVMPC_MAX_TRACK_ROWS 16
#define LPVMPC_MAX_N          52      /* (N+1) stages x 3008 B of LDS per instance must fit 160 KiB (run-time-horizon kernel) */

/* error codes */
#define LPVMPC_OK            0
#define LPVMPC_E_ARG        -1
#define LPVMPC_E_NODEVICE   -2
#define LPVMPC_E_HIP        -3
#define LPVMPC_E_NOMEM      -4

/* per-instance solver status, numerically equal to OSQP's status_val (CTRL:320-324, PLAN:214-216) */
#define LPVMPC_SOLVED                        1
#define LPVMPC_SOLVED_INACCURATE             2
#define LPVMPC_PRIMAL_INFEASIBLE_INACCURATE  3
#define LPVMPC_DUAL_INFEASIBLE_INACCURATE    4
#define LPVMPC_MAX_ITER_REACHED             -2
#define LPVMPC_PRIMAL_INFEASIBLE            -3
#define LPVMPC_DUAL_INFEASIBLE              -4
#define LPVMPC_NON_CVX                      -7
#define LPVMPC_UNSOLVED                    -10      /* also: non-finite input data (NaN / Inf in x0, A, B, vel_ref, uOld,
                                                      max_ey) -- no iteration is run, xPred / uPred are NaN, iters = 0 */
#define LPVMPC_PENDING                     -11      /* straggler deferral only (option "defer_after"): the instance is parked; the launch
                                                      * that finishes it has not written the final status yet */

typedef struct lpvmpc_config {
    int32_t kind;            /* LPVMPC_KIND_* */
    int32_t N;               /* horizon (ctor arg N, CTRL:35 / PLAN:34) */
    int32_t device;          /* HIP device ordinal */
    int32_t steering_delay;  /* controller: ctor arg steeringDelay (CTRL:35,68-71): the first steering_delay stages get an equality
                              * row delta_i = OldSteering[i+1] (CTRL:518-527); 0 (the reference's mains, CMAIN:49) .. 8.  Planner: 0 */
    double  dt;              /* sample time (ctor arg dt) */
    /* vehicle parameters the reference reads from ROS (CTRL:38-48, PLAN:70-82) */
    double  lf, lr, m, Iz, Cf, Cr, mu;
    double  max_vel, min_vel;
    /* weights (ctor args Q, R, dR, L_cf); Q is nx*nx row-major in the first nx*nx slots */
    double  Q[36];
    double  R[4];
    double  dR[2];
    double  L_cf[6];         /* planner only (PLAN:163) */
    /* hard-coded limits of the reference, exposed: controller CTRL:334-348, planner PLAN:173-177 */
    double  ctrl_vx_min;     /* 0.01  */
    double  ctrl_delta_max;  /* 0.249 */
    double  ctrl_a_max;      /* 4.0   */
    double  ctrl_a_min_abs;  /* 1.0   (a >= -1.0) */
    double  plan_xmin[5];    /* [min_vel -1 -2 -max_ey -0.8]; slots 0 and 3 are overwritten from min_vel / max_ey */
    double  plan_xmax[5];
    double  plan_umin[2];    /* [-0.249 -0.7] */
    double  plan_umax[2];    /* [ 0.249  2.0] */
    /* OSQP settings (defaults of the 0.6.x series; the reference passes only polish=True).  The loop schedule is OSQP's: an iteration
     * that is a multiple of check_termination is checked (0: never inside the loop), one that is a multiple of adaptive_rho_interval
     * may change rho, and a run that reaches max_iter on an unchecked iteration gets OSQP's closing update and check (here: the last
     * iteration is always a checked one).  adaptive_rho_interval = 0 means NO ADAPTATION here, the same as adaptive_rho = 0: in OSQP 0
     * asks for an interval chosen from the measured set-up time, the one default that cannot be reproduced (the default here is 25).
     * polish = 0: the ADMM iterate is returned, polish flags 0. */
    double  rho, sigma, alpha, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf;
    double  polish_delta, adaptive_rho_tolerance;
    int32_t max_iter, check_termination, scaling, adaptive_rho, adaptive_rho_interval;
    int32_t polish, polish_refine_iter, reserved1;
    /* track table = Map.PointAndTangent (TRACK:88-202): rows [x y psi cum_s seg_len curvature] */
    int32_t track_rows;
    int32_t reserved2;
    double  track[LPVMPC_MAX_TRACK_ROWS * 6];
} lpvmpc_config;

typedef struct lpvmpc_handle lpvmpc_handle;

/* library / ABI version (LPVMPC_VERSION). */
int lpvmpc_version(void);

/* Fill *cfg with the reference's launch-file and hard-coded defaults for `kind`
 * (MAIN_LAUNCH.launch:5-11,40-44; controllerMain.py:139-150; plannerMain.py:96-99). */
void lpvmpc_default_config(int32_t kind, lpvmpc_config *cfg);

/* Replaces the constructors PathFollowingLPV_MPC.__init__ (CTRL:35-84) and
 * LPV_MPC_Planner.__init__ (PLAN:34-82).  Returns NULL on failure (see lpvmpc_last_error(NULL)). */
lpvmpc_handle *lpvmpc_create(const lpvmpc_config *cfg);
void lpvmpc_destroy(lpvmpc_handle *h);
const char *lpvmpc_last_error(const lpvmpc_handle *h);
/* LPVMPC_E_* code of the last failure on this thread (0 when none); tells why lpvmpc_create returned NULL. */
int lpvmpc_last_error_code(void);

/* Runtime options.  "kernel_variant": 0 = fastest instantiation for (kind, N) (default), 1 = run-time-horizon
 * kernel (factor tiles in LDS, any N), 2 = compile-time horizon with ONE wavefront per instance (where it
 * exists; the default for N = 20 / 30 / 40 uses two wavefronts and a two-sided elimination).
 * "force_generic_kernel" (0/1) is shorthand for variants 0 / 1.  Used by the tests to cross-check the kernels.
 * "warm_start": 0 = every solve starts from x = z = y = 0 like the reference (fresh OSQP object per call,
 * CTRL:302,316 / PLAN:204-208; default); 1 = start from the previous solve's (x, y) of the same handle and
 * batch size; 2 = the same shifted by one stage (receding horizon).  Opt-in, changes iteration counts, not optima.
 * Applied as osqp_warm_start does (x, y as given, z = A x).  The shift of mode 2: stage k takes the previous solve's stage k + 1 and
 * the last stage that exists for a variable or row is kept -- states, dynamics rows and the planner's state-box rows run to stage N,
 * inputs, the planner's input-box rows and the controller's box rows to stage N - 1; of the steeringDelay pinned-steering rows, the row
 * of stage k takes the row of stage k + 1 and the last one (stage steeringDelay - 1) starts at 0, stage steeringDelay having none.
 * What is kept of a solve: the returned point with its duals -- the polished ones after an accepted polish, the ADMM iterate's otherwise
 * (rejected polish, SOLVED_INACCURATE, MAX_ITER_REACHED); zeros, a cold start, for an instance without a solution (PRIMAL / DUAL
 * INFEASIBLE, exact or inaccurate, UNSOLVED).  Whose state is valid: an instance warm-starts from ITS OWN most recent solve since the
 * option was last set (setting it again, to the same value too, is a fresh start), the workspace was (re)allocated or a fleet, cascade or
 * race was initialised on the handle; otherwise it starts cold.  A call of another batch size than the previous one starts cold, and an
 * instance that lpvmpc_solve_batch_masked leaves inactive keeps the state (or the cold start) it had.  Against the oracle's warm-started
 * run (tests/test_gpu_warm_start.py, every solve route, both modes, two warm ticks): status, iteration count and polish flag equal on
 * every instance the oracle itself decides robustly (all controller instances, 88 % .. 98 % of the planners':
 * tests/golden/warm_start/make_robust.py).
 * "cascade_prefetch" (0/1, default 1): read by lpvmpc_cascade_init on the controller handle, see there.
 * "kernel_variant" 3 = the DPP two-wavefront kernels of round 1 for the controller at N = 20 and the planner at N = 20 / 30 / 40 (their
 * defaults run the KKT sweeps and the factorisation on the matrix cores; the planner at N = 30 / 40 with FOUR wavefronts per instance, the
 * two elimination chains relayed over two wavefronts each -- at N = 30 for launches that leave compute units free and for handles with
 * straggler deferral, while plain launches of 512 instances or more take the two-wavefront form of the same arithmetic: every output word
 * is the same either way); 4 = the planner N = 30 kernel with two wavefronts and MFMA sweeps whatever the batch; 5 = the planner N = 30 DPP kernel
 * with every vector in LDS (two instances per CU); 6 = the planner N = 40 kernel with two wavefronts and MFMA sweeps whatever the batch;
 * 7 = round 3's default at N = 30: the DPP kernel with its three equilibration vectors in global memory (three instances per CU) for
 * batches beyond 512 instances without deferral, variant 5 otherwise; 8 = the four-wavefront planner kernels whatever the batch.  One
 * arithmetic per (kind, N) by default: an instance's result does not depend on the batch it is solved in.
 * 9 = the LATENCY form of the N = 20 kernels, controller (steeringDelay 0) and planner, on handles without straggler deferral (every
 * other handle and shape: as 0):
 * the two elimination chains relayed over FOUR wavefronts, the arithmetic of the default kernel step for step.  An instance that has its
 * compute unit to itself (batches up to 256) finishes 6 % sooner, a full chip gains nothing.  Opt-in: the block-wide sums of the N = 20
 * kernels (the cost normalisation's mean, the infeasibility certificates' sums, the objective) associate by the number of wavefronts,
 * so between variants 0 and 9 a word may differ in its last bits where such a sum decides (statuses and iteration counts are equal,
 * solutions to 5e-6: tests/test_gpu_parity.py; every word equal on the batches tried, where the cost normalisation is decided by the
 * linear term's maximum; planner N = 20: -7 % for a lone instance, -8 % at 64 ... 256).  The drop-in classes (one vehicle per handle)
 * select it.
 * "defer_after" (iterations, 0 = off, default): STRAGGLER DEFERRAL for lpvmpc_solve_batch_dev.  One OSQP solve in a thousand
 * needs thousands of ADMM iterations where the typical one needs 50; a launch lasts as long as its slowest instance, so those
 * few hold the caller's stream for milliseconds.  With defer_after = K an instance that is still unsolved at a termination
 * check with iter >= K is parked (status LPVMPC_PENDING, whole solver state saved) and its workgroup ends.
 * "defer_budget" (iterations, default 200) says how the parked instances go on.  > 0: they RIDE IN THE HANDLE'S NEXT DEFERRED CALL.
 * That call's main launch carries, in front of its own instances, one workgroup per pool entry (grid pool + B); these riders continue
 * everything parked on the handle -- by the previous call and by earlier ones -- for defer_budget more iterations beside the new
 * instances, in the residency slots those free as they finish, and park again what is still unsolved.  No launch follows a call on
 * its stream (before, a bounded resume pass of a quarter of a millisecond did, and the stream's next call waited for it).  A parked
 * instance therefore advances with the handle's next deferred call, or at lpvmpc_join -- a call that nothing follows leaves its
 * stragglers as they are until the join -- and its results arrive one call of the handle later than with a pass behind every call.
 * 0: every deferred call is followed, on the same stream, by a resume pass of the same kernel that runs everything parked to completion.
 * -1: no pass behind a deferred call and no riders; the parked instances wait for lpvmpc_join (what a caller that joins after every
 * call wants: one batch, then the tail kernel; lpvmpc_solve_batch does this by itself).
 * With "defer_tail" 0 the results are bit-identical to the plain call (a restored instance re-factors K from its saved state); with
 * the default "defer_tail" 1 the passes to completion use the tail kernel: equal to round-off, see there.
 * Completion contract (unchanged): an instance's outputs are final when its status is no longer LPVMPC_PENDING; lpvmpc_join(h, stream)
 * enqueues the pass that finishes whatever is still parked, so work behind it in `stream` sees complete outputs.  Until then
 * the buffers of the deferred calls -- outputs, and the inputs while the call itself runs -- must stay valid and must not be reused
 * for other data while one of the call's instances is LPVMPC_PENDING.  A caller that cycles through a ring of output sets without
 * joining needs one more set per handle than with a pass behind every call: a straggler of call j is written by the launches of
 * calls j + 1, j + 2, ... of its handle (forty of them for a 4000-iteration instance at a budget of 100, as before).  The
 * synchronous host-array calls (lpvmpc_solve_batch, lpvmpc_solve_batch_masked) join by themselves before they copy the outputs back:
 * they never return LPVMPC_PENDING and carry no riders -- what earlier deferred calls left parked is finished by their join.
 * "defer_pool" (entries, 0 = max(64, B / 8), default): capacity of each of the two pools.  ADMISSION IS ORDERED BY AGE (K = defer_after):
 * instances with fewer than 2 K iterations may take three quarters of a pool, those between 2 K and 4 K an eighth of their own, and an
 * instance beyond 4 K takes any free entry (at least the last eighth).  An instance that finds its class's share full is not parked at
 * that check; it goes on iterating inside the launch that holds it and asks again at its next check (25 iterations older), so the few
 * many-thousand-iteration instances of a batch always get parked, however many nearly-done ones a small K sends to the pool first
 * (before round 6 admission was first come, first served: with K = 50 two fifths of a controller batch filled the pool at iteration 50,
 * the 4000-iteration instance stayed in the main launch to its end and a burst ran at half the rate of K = 75 .. 125; now K = 50 .. 125
 * are within 3 % of each other).  K is still a cost parameter: every parked instance is restored and re-factored by the pass that
 * continues it, so park what is rare -- choose K near the point where ~99 % of the instances are done (100 for the controller workloads
 * here; K = 25 parks most of a batch once and runs a burst at three quarters of the rate).  lpvmpc_defer_stats tells how many requests
 * were refused, i.e. whether "defer_pool" should grow.  With "defer_budget" > 0 the riders of a launch park into the same pool as its new
 * instances (which may take up to seven eighths of it), so the pool must hold the stragglers of ALL calls in flight on the handle, not of one:
 * a rider that finds no free entry is refused like any other instance and goes on iterating in place -- a many-thousand-iteration rider then
 * holds its main launch, and the stream, to its end.
 * "defer_tail" (0 | 1, default 1): the passes that run parked instances to completion (lpvmpc_join, the synchronous entry
 * points, "defer_budget" 0) use the whole-CU tail kernel where one exists for the handle (controller or planner, N = 20): a 512-thread
 * workgroup per instance that applies K^-1 as a dense matrix held in registers, runs two phases per ADMM iteration and evaluates the
 * termination checks beside the iterations (round 5: 1.0 us per iteration against 1.9 us for an instance that has the GPU to
 * itself).  Handles with steering_delay > 0 keep the two-wavefront kernel for these passes.  Statuses, iteration counts and polish
 * flags have been OBSERVED equal to the other kernel's on every instance compared so far (196 608 over four tracks,
 * profiles/r05_tail_parity_sweep.txt; the seeds of tests/test_gpu_deferral.py are regression fixtures for this build) -- an
 * observation, not a guarantee: the two kernels round differently, and a termination test that is decided by round-off can move by
 * one check (25 iterations) on another toolchain or device.  Solutions agree to round-off (1e-7 polished, 1e-6 for an un-polished
 * iterate; observed 3.1e-9 / 1.1e-7), so bit-identity with the plain call holds with 0 only.
 *
 * FLOAT TOLERANCE of the QP stage against the reference algorithm (the CPU oracle on identical data; tests/_tolerance.py,
 * DESIGN.md section 2): status and iteration count equal -- except a run that ends at max_iter, where OSQP's 10 eps "solved
 * inaccurate" test is decided by round-off (MAX_ITER_REACHED <-> SOLVED_INACCURATE, same iteration count) -- and xPred / uPred in one of
 * three classes: (A) polished: 1e-6; (B) un-polished, converged: 2e-4 (observed <= 1e-6); (C) ran to the max_iter cap (an unconverged
 * ADMM iterate, which OSQP guarantees nothing for and the reference uses as it comes): same iteration count, |du| <= 2e-2 (observed
 * <= 1.01e-2 on 42 of 110 202 instances, all of them planner QPs at 4000 iterations).  Class C carries NO objective bound: two of the 42
 * sit 1.8e-2 / 2.8e-4 (relative) from the oracle's objective -- MAX_ITER_REACHED points, for which OSQP promises nothing.
 * (D) no solution on either side (PRIMAL / DUAL INFEASIBLE: NaN outputs, equal statuses): the certificate of a diverging iterate may fire
 * one termination check (25 iterations) apart -- the oracle itself does under its two KKT elimination orders (1 of 110 202: Euge_Track,
 * planner N = 40: device 50, batch oracle 75, oracle with the other order 50).  The reference discards such a tick either way. */
int lpvmpc_set_option(lpvmpc_handle *h, const char *name, int32_t value);
/* Straggler deferral (see "defer_after"): enqueues on `stream` (a hipStream_t; ordered behind the stream of the handle's last
 * deferred call if it is another one) the resume pass that runs every parked instance to completion.  With "defer_budget" > 0 this
 * is also what continues the stragglers of a handle's LAST call: riders need a next call to travel in.  No-op without deferral. */
int lpvmpc_join(lpvmpc_handle *h, void *stream);
/* Straggler deferral counters of the handle since its first deferred call: *parked = instances parked (every parking counts, also a
 * re-parking by a rider), *refused = parking requests turned down because the pool share of the instance's age class was
 * full (see "defer_pool": the instance went on in its launch and asked again later).  Waits for the stream of the handle's last
 * deferred call, so every launch enqueued so far is counted.  Either pointer may be NULL. */
int lpvmpc_defer_stats(lpvmpc_handle *h, int64_t *parked, int64_t *refused);
/* Like lpvmpc_kernel_time_stats (below) for the resume launches of the straggler deferral: the passes to completion of lpvmpc_join
 * and of "defer_budget" 0.  (The bounded continuation of "defer_budget" > 0 has no launch of its own: its riders are part of the main
 * launches that lpvmpc_kernel_time_stats times.) */
int lpvmpc_resume_time_stats(lpvmpc_handle *h, double *total_ms, int32_t *count);

/* (Round 4 shipped an experimental "long-runner lane" here -- lpvmpc_lane_*: reserved compute units for the whole-CU tail kernel.
 * It lost on every configuration measured (profiles/r04_lane_ab.txt: the driver's burst 13.3 -> 14.1-16.6 ms, the default run
 * 3.17 -> 2.5-2.7 M solves/s) and was removed from the library in round 5; docs/HISTORY.md keeps the design notes.) */

/* Pre-size the device workspace for batches up to B (otherwise grown on demand). */
int lpvmpc_reserve(lpvmpc_handle *h, int32_t B);

/*
 * LPV evaluation + horizon roll-out.  Replaces LPVPrediction (CTRL:166-258 / PLAN:242-320).
 *   x0       [B][nx]
 *   u_prev   [B][N][2]       previous input prediction (uPred)
 *   vel_ref  [B][N+1]        controller: vx scheduling (CTRL:200); entry N unused here.  NULL for planner
 *   curv_s   controller: curv_ref [B][N] used when lap != 0 (CTRL:196-198), may be NULL when lap == 0;
 *            planner:    SS [B][N+1]  (PLAN:270-271)
 *   cf_new   controller: Cf = Cr = cf_new (CTRL:172-173); ignored for the planner
 *   lap      controller: LapNumber (0 -> curvature from the map at the rolled-out s)
 * outputs (any may be NULL):
 *   states   [B][N][nx]      STATES_vec
 *   A        [B][N][nx][nx]  Atv      Bm [B][N][nx][2]  Btv       (Ctv is identically zero, CTRL:236-241)
 */
int lpvmpc_lpv_batch(lpvmpc_handle *h, int32_t B, const double *x0, const double *u_prev,
                     const double *vel_ref, const double *curv_s, double cf_new, int32_t lap,
                     double *states, double *A, double *Bm);

/* Seed-mode linearisation along a given trajectory.  Replaces _EstimateABC (CTRL:732-809 / PLAN:519-591).
 *   xlast [B][N][6]  controller columns [vx vy wz epsi s ey]; planner columns [vx vy wz ey epsi s]
 *   delta [B][N]     steering angle per stage */
int lpvmpc_estimate_abc_batch(lpvmpc_handle *h, int32_t B, const double *xlast, const double *delta,
                              double *A, double *Bm);

/*
 * QP build + OSQP-ADMM solve with caller-supplied LPV matrices.  Replaces
 * PathFollowingLPV_MPC.solve(x0, ., uPred, ., vel_ref, A_L, B_L, C_L, .) (CTRL:89-162 incl. _buildMatEqConst,
 * _buildMatCost, _buildMatIneqConst, osqp_solve_qp) and LPV_MPC_Planner.solve (PLAN:86-236).
 *   x0      [B][nx]
 *   A       [B][N][nx][nx]   Bm [B][N][nx][2]
 *   vel_ref [B][N+1]   controller tracking reference: entries 0..N-1 = vel_ref[i], entry N = vel_ref[-1]
 *                      (CTRL:434-438); NULL for the planner
 *   u_old   [B][2 + steering_delay]  [OldSteering[0], OldAccelera[0], OldSteering[1 .. steering_delay]] (CTRL:395, 523;
 *                      PLAN:114); NULL = zeros
 *   max_ey  [B]        planner lateral bound (solve arg max_ey, PLAN:176-177); NULL for the controller
 * outputs:
 *   xPred [B][N+1][nx], uPred [B][N][2]  (NaN for instances without a solution, as OSQP returns)
 *   status [B], iters [B]  (may be NULL)
 *   resid  [B][4] = {pri_res, dua_res, obj_val, rho_final}  (may be NULL): OSQP's info words, in the unscaled problem.
 *                   pri_res = |Ax - z|_inf and dua_res = |Px + q + A'y|_inf of the point the status refers to; obj_val = 1/2 x'Px + q'x
 *                   of the returned point; rho_final = the rho of the last ADMM iteration (the configured rho when adaptive_rho = 0,
 *                   adaptive_rho_interval = 0 or max_iter < adaptive_rho_interval).  By status:
 *                     SOLVED, polish accepted (polish = 1)   the polished point's residuals and objective; rho_final stays the ADMM's
 *                     SOLVED, polish rejected (-1) or off (0), SOLVED_INACCURATE, MAX_ITER_REACHED
 *                                                            the last ADMM iterate's residuals and objective (the point returned)
 *                     PRIMAL_INFEASIBLE (exact / inaccurate) obj_val = +1e30; pri_res / dua_res of the last iterate; xPred / uPred NaN
 *                     DUAL_INFEASIBLE (exact / inaccurate)   obj_val = -1e30; likewise
 *                     UNSOLVED (non-finite inputs: no iteration is run)   four NaN
 *                     LPVMPC_PENDING (parked by the straggler deferral)   not written yet: the caller's words stay until the
 *                                                            instance's results arrive with its final status
 *                   One difference from OSQP, in rho_final alone: when max_iter is off the check_termination grid and on the
 *                   adaptive_rho_interval grid, a run that the closing check of iteration max_iter ends as SOLVED or (PRIMAL / DUAL)
 *                   INFEASIBLE reports the rho of iteration max_iter - 1 -- OSQP updates rho once more in front of that check
 *                   (tests/_tolerance.py late_rho; the iterate, the status and the other words are OSQP's).
 *   polish [B]    = OSQP status_polish (1 accepted, -1 rejected, 0 not run)  (may be NULL)
 */
int lpvmpc_solve_batch_AB(lpvmpc_handle *h, int32_t B, const double *x0, const double *A, const double *Bm,
                          const double *vel_ref, const double *u_old, const double *max_ey,
                          double *xPred, double *uPred, int32_t *status, int32_t *iters, double *resid,
                          int32_t *polish);

/* Fused tick: lpvmpc_lpv_batch followed by lpvmpc_solve_batch_AB with x0 as the initial state
 * (the call pair controllerMain.py:361-363 / plannerMain.py:175-176), without the host round trip. */
int lpvmpc_solve_batch(lpvmpc_handle *h, int32_t B, const double *x0, const double *u_prev,
                       const double *vel_ref, const double *curv_s, const double *u_old, const double *max_ey,
                       double cf_new, int32_t lap,
                       double *xPred, double *uPred, int32_t *status, int32_t *iters, double *resid,
                       int32_t *polish);

/* lpvmpc_solve_batch for the instances with active[i] != 0 (active [B], host memory) only.  The other instances are not
 * solved -- their workgroups return before reading or writing anything -- and their rows of xPred / uPred / status /
 * iters / resid / polish are left exactly as the caller had them.  All-zero mask: no work, nothing written. */
int lpvmpc_solve_batch_masked(lpvmpc_handle *h, int32_t B, const double *x0, const double *u_prev,
                              const double *vel_ref, const double *curv_s, const double *u_old,
                              const double *max_ey, double cf_new, int32_t lap, double *xPred, double *uPred,
                              int32_t *status, int32_t *iters, double *resid, int32_t *polish, const int32_t *active);

/* Same as lpvmpc_solve_batch but every pointer is a DEVICE pointer and the work is enqueued on `stream`
 * (a hipStream_t; NULL = default stream) without synchronising.  Used by the closed-loop / bench paths. */
int lpvmpc_solve_batch_dev(lpvmpc_handle *h, int32_t B, const double *x0, const double *u_prev,
                           const double *vel_ref, const double *curv_s, const double *u_old, const double *max_ey,
                           double cf_new, int32_t lap,
                           double *xPred, double *uPred, int32_t *status, int32_t *iters, double *resid,
                           int32_t *polish, void *stream);

/* Enable (1) / disable (0) HIP-event timing of the solve kernel: while enabled every launch of the
 * ADMM solve kernel is bracketed by an event pair recorded on the launch stream (no host sync).
 * Enabling resets the statistics.  (bench.py roofline leg.) */
int lpvmpc_set_timing(lpvmpc_handle *h, int32_t on);

/* Sum of the solve-kernel durations (ms) and the number of launches recorded since timing was enabled
 * (at most the last 1024).  Synchronises with the recorded events. */
int lpvmpc_kernel_time_stats(lpvmpc_handle *h, double *total_ms, int32_t *count);

/* Duration (ms) of the most recent timed solve-kernel launch, negative if none. */
double lpvmpc_last_kernel_ms(lpvmpc_handle *h);

/* ---------------------------------------------------------------------------------------------------
 * "Next row" f1 of the hot-path scope table: the caller-side pieces a closed-loop run needs, batched.
 * ------------------------------------------------------------------------------------------------- */

/* Map.getLocalPosition (TRACK:283-383): xy_psi [B][3] -> out [B][4] = {s, ey, epsi, inside}; off the track the
 * reference's sentinels {10000, 10000, 10000, 0}.  half_width / slack = Map.halfWidth / Map.slack. */
int lpvmpc_local_position_batch(lpvmpc_handle *h, int32_t B, const double *xy_psi, double half_width, double slack,
                                double *out);

/* Map.getGlobalPosition (TRACK:205-262): s_ey [B][2] -> out [B][3] = {x, y, theta}. */
int lpvmpc_global_position_batch(lpvmpc_handle *h, int32_t B, const double *s_ey, double *out);

/* n_sub steps of Simulator.f (vehicleSimulator.py:164-199; linear tyres Fy = 60 alpha) on
 * state [B][8] = {x, y, vx, vy, ax, ay, yaw, psiDot} (in/out) under the constant input u [B][2] = {a, delta}.
 * lf, lr, m, Iz come from the handle's configuration; mu_sim = simulator/mu, dt_sim = simulator/dt. */
int lpvmpc_plant_step_batch(lpvmpc_handle *h, int32_t B, double *state, const double *u, int32_t n_sub, double dt_sim,
                            double mu_sim);

/* Closed-loop fleet of B vehicles under the LPV-MPC controller in the lap-0 path-tracking branch of
 * controllerMain.py (:179-190 measurement incl. quirk Q9 when q9_swap != 0, :289-298 last command as uOld,
 * :310-315 nine seed ticks, :325-331 LPV prediction with x0 = first rolled-out state, :381-386 command), with the
 * plant advanced n_sub simulator steps per control tick.  Everything stays on the device; lpvmpc_cl_tick enqueues
 * n_ticks control ticks without synchronising, lpvmpc_cl_read synchronises and copies the current fleet state
 * (any pointer may be NULL): plant [B][8], local_state [B][6], cmd [B][2] = {servo, motor}, iters / status [B]. */
int lpvmpc_cl_init(lpvmpc_handle *h, int32_t B, const double *plant0, double half_width, double slack, int32_t q9_swap,
                   int32_t n_sub, double dt_sim, double mu_sim);
int lpvmpc_cl_tick(lpvmpc_handle *h, int32_t n_ticks);
int lpvmpc_cl_read(lpvmpc_handle *h, double *plant, double *local_state, double *cmd, int32_t *iters, int32_t *status);
/* A handle that runs a fleet (lpvmpc_cl_init) or a cascade (lpvmpc_cascade_init, the controller handle and its planner
 * handle) keeps the fleet's receding-horizon state in its workspace between ticks: the stand-alone batch calls
 * (lpvmpc_solve_batch*, lpvmpc_lpv_batch, lpvmpc_estimate_abc_batch, lpvmpc_*_position_batch, lpvmpc_plant_step_batch,
 * lpvmpc_handoff_batch) on such a handle fail with LPVMPC_E_ARG instead of overwriting it -- use a second handle.
 * lpvmpc_cl_release ends the fleet / cascade of the handle (waits for its queued ticks, frees the fleet buffers); the handle
 * then accepts batch calls again. */
int lpvmpc_cl_release(lpvmpc_handle *h);

/* ---------------------------------------------------------------------------------------------------------------
 * Planner -> controller reference hand-off.  Replaces the post-processing in the planner node
 *   plannerMain.py:201-224   s integration along the planned states, centre-line pose (Map.getGlobalPosition),
 *                            xp / yp / yaw reconstruction, vel = vx, curv = wz / vx
 *   plannerMain.py:257-280   scipy interp1d(kind='cubic') from N samples at dt to round(N dt / interp_dt) samples,
 *                            scipy.signal.filtfilt(b, a, curvature, padlen)
 *   plannerMain.py:303-308   the five My_Planning arrays x_d, y_d, psi_d, vx_d, curv_d (barc/msg/My_Planning.msg:1-6)
 * Resampling and filtering are linear in the N samples, so they are applied as two dense operators built on the host:
 * W (cubic not-a-knot spline evaluation) and FW = filtfilt o W. */
#define LPVMPC_MAX_FILTER_ORDER 8
typedef struct lpvmpc_handoff_config {
    double  interp_dt;                          /* 0.033                                   PMAIN:257 */
    int32_t padlen;                             /* 50                                      PMAIN:280 */
    int32_t order;                              /* 4: signal.ellip(4, 0.01, 120, 0.125)    PMAIN:112 */
    double  b[LPVMPC_MAX_FILTER_ORDER + 1];     /* numerator, order + 1 entries used */
    double  a[LPVMPC_MAX_FILTER_ORDER + 1];     /* denominator */
} lpvmpc_handoff_config;

/* the reference's values, including the coefficients of its elliptic filter */
void lpvmpc_handoff_default_config(lpvmpc_handoff_config *cfg);

/* Number of resampled points M = round(N dt / interp_dt) (PMAIN:259), or LPVMPC_E_ARG when the configuration cannot
 * work: like scipy's filtfilt (and so the reference's node) this refuses M <= padlen, i.e. N < 34 at the reference's rates. */
int lpvmpc_handoff_length(int32_t N, double dt, const lpvmpc_handoff_config *cfg);

/* Host-only (no device needed): the operators W and FW, each [M][N] row-major; returns M. */
int lpvmpc_handoff_operators(int32_t N, double dt, const lpvmpc_handoff_config *cfg, double *W, double *FW);

/* Build the operators for a PLANNER handle's (N, dt) and keep them on its device; returns M. */
int lpvmpc_handoff_setup(lpvmpc_handle *planner, const lpvmpc_handoff_config *cfg);

/* One hand-off for B planner solutions: xPred [B][N+1][5]; SS [B][N+1] and pose [B][3] = {Xlast, Ylast, Thetalast}
 * are the node's carried state (in/out: SS is re-integrated and SS[0] = SS[1], pose = centre-line pose of stage 1);
 * sig [B][5][N] (may be NULL) = xp, yp, yaw, vel, curv at the planner's rate; refs [B][5][M] = the My_Planning arrays. */
int lpvmpc_handoff_batch(lpvmpc_handle *planner, int32_t B, const double *xPred, double *SS, double *pose, double *sig,
                         double *refs);

/* Planner + controller + plant cascade for a fleet of B vehicles in the racing phase (LapNumber >= 1), resident on the
 * device.  `ctrl` is a controller handle with the trajectory-tracking tuning (Controller_TT, CMAIN:142-150), `planner` a
 * planner handle on which lpvmpc_handoff_setup has been called.  Per controller tick (30 Hz):
 *   - planner ticks 0 .. floor(2k/3) have run before controller tick k (20 Hz node; PMAIN:126-224,257-308: first tick
 *     from the measured state with the seed trajectory of PMAIN:465-505, later ticks open loop from xPred[1]);
 *   - measurement of the LapNumber >= 1 branch (CMAIN:176-182,198-248): yaw - 2 pi LapNumber wrapped, reference windows
 *     [0:N] re-read from the latest message on every second tick only (`index` toggle), Body_Frame_Errors (CMAIN:495-506)
 *     with dead-reckoned s, racing lap counter (CMAIN:268-272); uOld = last command (CMAIN:289-298);
 *   - Controller_TT.LPVPrediction + solve from the measured state (CMAIN:361-363); command = uPred[0] (CMAIN:381-386);
 *   - the plant advances n_sub[k % 3] steps of Simulator.f (7, 7, 6 steps of 5 ms = 100 ms per 3 ticks).
 * plant0 [B][8], cmd0 [B][2] = {servo, motor} and uPred0 [B][N][2] (Controller_TT.uPred = Controller.uPred, CMAIN:336)
 * describe the fleet at the lap event; lap0 >= 1.  half_width / slack: the map's, used by Map.getLocalPosition;
 * plan_max_ey: the max_ey argument of the planner's solve (the ROS parameter /TrajectoryPlanner/halfWidth).  q9_swap: the planner's first x0 takes the map's (ey, epsi) in the
 * (epsi, ey) slots as PMAIN:141 assigns them.  The two nodes run on their own HIP streams; with option
 * "cascade_prefetch" = 1 (default; set on `ctrl` before init) a planner tick is enqueued as soon as its message buffer is
 * free, so that it overlaps the controller ticks that still use the previous message -- results do not change.
 * lpvmpc_cascade_tick enqueues n_ticks controller ticks without synchronising; lpvmpc_cascade_read synchronises and copies
 * (any pointer may be NULL): plant [B][8], local_state [B][6], cmd [B][2], ctrl_iters / ctrl_status [B], lap / lap_tick [B]
 * (lap counter and the controller tick of the last lap event), refs [B][5][M] and plan_xPred [B][Np+1][5] / plan_iters /
 * plan_status [B] of the most recent planner tick, ticks [2] = {controller ticks, planner ticks} enqueued so far.
 * The planner handle must outlive the cascade (it ends with the controller handle, or with the next lpvmpc_cascade_init). */
int lpvmpc_cascade_init(lpvmpc_handle *ctrl, lpvmpc_handle *planner, int32_t B, const double *plant0, const double *cmd0,
                        const double *uPred0, int32_t lap0, double half_width, double slack, double plan_max_ey,
                        int32_t q9_swap, const int32_t *n_sub, double dt_sim, double mu_sim);
int lpvmpc_cascade_tick(lpvmpc_handle *ctrl, int32_t n_ticks);
int lpvmpc_cascade_read(lpvmpc_handle *ctrl, double *plant, double *local_state, double *cmd, int32_t *ctrl_iters,
                        int32_t *ctrl_status, int32_t *lap, int32_t *lap_tick, double *refs, double *plan_xPred,
                        int32_t *plan_iters, int32_t *plan_status, int32_t *ticks);
/* alive_ticks [B]: controller ticks each vehicle has entered with a finite plant state since lpvmpc_cascade_init (a vehicle whose
 * planner QP went primal infeasible carries NaN from then on and costs no iterations: the sum over the fleet is the number of
 * vehicle-ticks that did work).  Synchronises like lpvmpc_cascade_read. */
int lpvmpc_cascade_alive_ticks(lpvmpc_handle *ctrl, int32_t *alive_ticks);

/* ---------------------------------------------------------------------------------------------------------------
 * Race engine: the reference's whole experiment (controllerMain.py + plannerMain.py from the grid to NumberOfLaps) for a
 * fleet of B vehicles, each in its own phase, resident on the device; one lpvmpc_race_tick call enqueues n_ticks
 * controller ticks (30 Hz) and nothing goes to the host between them.  Three handles: `path` (controller, path-following
 * tuning: Controller), `tt` (controller, racing tuning: Controller_TT) and `planner` (lpvmpc_handoff_setup done).
 * Per vehicle and tick, in this order on the path handle's stream:
 *   phase 0 (lap 0): measurement of the lap-0 branch (Map.getLocalPosition, vx >= 0.01, quirk Q9 with q9_swap);
 *     HalfTrack = 1 once s >= 3L/4; the race's first 9 ticks solve `path` on the seed trajectories (first_it < 10,
 *     CMAIN:310-320), later ticks LPVPrediction(lap 0) + solve on `path` from the first rolled-out state (CMAIN:325-331);
 *   lap event (HalfTrack && s <= L/4, CMAIN:254-262): lap = 1, SS = 0, HalfTrack = 0, phase 1.  On this tick `tt` solves
 *     from the lap-0 measurement with vel_ref = ones(N+1), curv_ref = zeros(N), LapNumber = 1, uPred = the path handle's
 *     uPred (CMAIN:336) and u_old = the last command (within the seed ticks `path` solves instead, as ControllerNode.step);
 *   phase 1, racing tick k (k = 0 on the tick after the event): the vehicle's planner ticks 0 .. floor(2k/3) have run
 *     before it (the first from the measured plant state with the seed of PMAIN:465-505, later ones open loop from
 *     xPred[1]; each followed by the hand-off into the vehicle's message); measurement of the LapNumber >= 1 branch with
 *     the vehicle's own `index` latch (windows re-read on even k); LPVPrediction + solve on `tt`; racing lap event
 *     (|x| < 0.1 && s >= L - L/10, CMAIN:268-272);
 *   command = uPred[0] of the controller of the vehicle's lap; the plant advances n_sub_lap0 simulator steps on lap-0
 *     ticks (the event tick included) and n_sub[k % 3] on racing tick k.
 * Definitions of this engine where the ROS run has none:
 *   finish: when the lap counter exceeds `laps` (RunController = 0 in the reference) the vehicle is phase 2 and FROZEN from
 *     that tick on -- plant and command are not advanced, it costs no iterations, its outputs stay readable;
 *   lost: a vehicle entering a tick with a non-finite plant state (with an estimator: or a non-finite estimate) is phase 3
 *     and frozen the same way;
 *   lap time: lap_step [B][laps + 2] holds the plant-step index at which lap 0, 1, ... started (-1: not reached), so
 *     lap times are step differences x dt_sim (simulated time; the reference's TLAPTIME is wall-clock time).
 * Kernel launches that only write per-tick scratch run unmasked (the seed-tick ABC linearisation of `path`); every launch
 * that writes carried state -- LPV roll-outs, solves, hand-off -- is masked to this tick's vehicles (SolveArgs::active).
 * Refused with LPVMPC_E_ARG: handles on different devices or of the wrong kinds, path / tt with different N, dt or track,
 * N > 20 (the seed rows), steering_delay != 0 (lpvmpc_race_init_actuated runs delayed controllers), a planner without lpvmpc_handoff_setup or with a message shorter than N,
 * warm_start != 0 on any of the three, an estimator on `path`, a handle already running a fleet, cascade or race.
 * The race belongs to `path`: lpvmpc_cl_release(path) (or destroying any of the three) ends it; while it runs, batch calls
 * on all three handles fail.  plant0 [B][8] = {x y vx vy ax ay yaw psiDot}; half_track0 [B] or NULL (= 0).
 *
 * lpvmpc_race_init_observed runs the race with the gain-scheduled LPV estimator and the simulated sensors in the loop
 * (below: "Gain-scheduled LPV state estimator"); with obs == NULL it is exactly lpvmpc_race_init.  obs is checked like
 * lpvmpc_observer_setup's config, and a path handle with lpvmpc_observer_setup attached is refused by both calls: the race's
 * estimator is configured through obs only.  With an estimator:
 *   start: each vehicle's estimator starts as the lap-0 fleet's: estimate [init_vx, 0, 0, x0, y0, yaw0] of plant0, GPS hold at
 *     the start position, step counter 0.  ONE estimator runs for the whole race: it carries on through the lap event (the
 *     reference's estimator node keeps running) and is not restarted from the plant as lpvmpc_cascade_init starts one;
 *   plant steps: each of a vehicle's n_sub_lap0 / n_sub[k % 3] plant steps of a tick is followed by its sensors and one observer
 *     step, as in a fleet with an estimator.  Finished and lost vehicles advance neither plant nor observer and their step
 *     counter stays put, so a vehicle's noise depends on (seed, vehicle_offset + b, its own step) only -- not on the batch, the
 *     other vehicles' phases or the sharding;
 *   measurement: every measurement reads the ESTIMATE in the plant's layout [x y vx vy 0 0 yaw psiDot] in place of the plant:
 *     the lap-0 branch with HalfTrack and the lap-0 event rule, the racing branch with the racing event rule (|x| < 0.1 with x
 *     the estimate's), and the planner's first state (PMAIN:141);
 *   outputs: lpvmpc_race_read's plant stays the ground truth, local_state is the measurement made from the estimate;
 *     lap_step and alive_ticks keep their meaning; lpvmpc_observer_read(path, ...) returns the estimate [B][6] and the latest
 *     sensor reading [B][5] (on a race without an estimator it fails with LPVMPC_E_ARG).
 * The estimator state belongs to the race: lpvmpc_cl_release(path) (or destroying any of the three handles) frees it, and a
 * later lpvmpc_cl_init on `path` runs on ground truth. */
typedef struct lpvmpc_race_config {
    int32_t laps;             /* NumberOfLaps: a vehicle finishes when its lap counter exceeds it (>= 1) */
    int32_t n_sub_lap0;       /* plant steps per lap-0 tick (7) */
    int32_t n_sub[3];         /* plant steps per racing tick k % 3 (7, 7, 6) */
    int32_t q9_swap;          /* 1: SURVEY quirk Q9 in both measurements (CMAIN:188, PMAIN:141) */
    double  half_width, slack, plan_max_ey, dt_sim, mu_sim;   /* the map's, the planner's max_ey, the simulator's (0.3, 0.15, 0.2, 0.005, 0.05) */
} lpvmpc_race_config;
void lpvmpc_race_default_config(lpvmpc_race_config *cfg);
int  lpvmpc_race_init(lpvmpc_handle *path, lpvmpc_handle *tt, lpvmpc_handle *planner, int32_t B,
                      const double *plant0, const int32_t *half_track0, const lpvmpc_race_config *cfg);
struct lpvmpc_observer_config;
int  lpvmpc_race_init_observed(lpvmpc_handle *path, lpvmpc_handle *tt, lpvmpc_handle *planner, int32_t B,
                               const double *plant0, const int32_t *half_track0, const lpvmpc_race_config *cfg,
                               const struct lpvmpc_observer_config *obs);
/* enqueue n_ticks ticks; no synchronisation */
int  lpvmpc_race_tick(lpvmpc_handle *path, int32_t n_ticks);
/* synchronises and copies (any pointer may be NULL): plant [B][8], local_state [B][6] (the last measurement), cmd [B][2],
 * phase / lap [B]; iters / status [B]: the controller solve of the vehicle's phase on the last tick (iters 0 and status
 * unchanged when it did not solve: frozen, lost); plan_iters / plan_status [B] of the vehicle's last planner tick (0 before
 * its first: the race's start zeroes the three handles' iteration, status and polish rows); ticks [1] = ticks run. */
int  lpvmpc_race_read(lpvmpc_handle *path, double *plant, double *local_state, double *cmd, int32_t *phase,
                      int32_t *lap, int32_t *iters, int32_t *status, int32_t *plan_iters, int32_t *plan_status,
                      int32_t *ticks);
/* lap_step [B][laps + 2] (see above), alive_ticks [B]: ticks entered with a finite plant state and not frozen (either may be NULL) */
int  lpvmpc_race_laps(lpvmpc_handle *path, int32_t *lap_step, int32_t *alive_ticks);
/* the two controllers' predicted inputs uPred [B][N][2] as they are now (the path handle's, the tt handle's; either may be NULL):
 * the u_prev of their next LPV roll-out.  Synchronises like lpvmpc_race_read. */
int  lpvmpc_race_predictions(lpvmpc_handle *path, double *path_uPred, double *tt_uPred);

/* ---------------------------------------------------------------------------------------------------------------
 * Gain-scheduled LPV state estimator and simulated sensors (stateEstimator.py = EST, vehicleSimulator.py = SIM).
 *
 * Observer step (Estimator.GS_LPV_Est, EST:349-398, with Continuous_AB_Comp EST:402-436 and L_Gain_Comp EST:439-492):
 *   x = [vx vy psiDot x y yaw], y = [vx psiDot x y yaw] (C selects states 0, 2, 3, 4, 5: EST:248-252), u = [servo, motor];
 *   t = k dt with dt = 1 / loop_rate and k the number of observer steps including this one (k = 1 on the first step);
 *   scheduling variables (vx, vy, theta) = (x[0], x[1], x[5]) when t > 0.02, else (y[0], 0, y[4]) (EST:368-376);
 *   A_obs(vx, vy, theta, steer), B_obs(steer) with the observer's own constants lf = lr = 0.125, m = 1.98, I = 0.03,
 *   Cf = Cr = 60, mu = 0.05 (independent of lpvmpc_config; a row per vehicle: "Per-vehicle state estimator" below);
 *   polytope HS when vx > lim_ls[0][1], else LS; 16 vertex weights from the limit rows 0, 1, 3, 5 (vx, vy, steer, theta) in
 *   EST:475-491's order (vertex i: bit 3 = vx, bit 2 = vy, bit 1 = steer, bit 0 = theta; a set bit takes 1 - M).  Like the
 *   reference the weights are NOT clamped: outside the polytope some are negative and the gain is extrapolated;
 *   L = sum_i mu_i Llmi[:, :, i];  x+ = x + (dt (A + L C) x + dt B u - dt L y).
 *
 * Sensors (SIM:222-329 and the estimator's callbacks EST:600-760), drawn from the plant state after each plant step:
 *   IMU yaw = yaw + n_psi, IMU psiDot = psiDot + n_psiDot; GPS x, y = x + n_x, y + n_y, published when the publish counter
 *   exceeds thUpdate = (1 / gps_freq) / dt_sim (then the counter resets to 0, else it increments; the estimator keeps the
 *   last PUBLISHED value, initially the plant's start position); encoder v = sqrt(vx^2 + vy^2) + n_v, and the estimator's
 *   encoder reading becomes 0 after more than 40 consecutive unchanged readings (EST:733-741).  While t <= 0.02 the
 *   estimator measures y = [x_est[0], IMU psiDot, GPS x, GPS y, plant yaw] (EST:330-333).
 *   Each noise n = clip(std * g, -std * n_bound, std * n_bound) with g standard normal.
 *
 * Noise generator (counter based; a numpy restatement reproduces it):
 *   mix(z)   = splitmix64 finaliser: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *              (all arithmetic modulo 2^64);
 *   key      = mix(mix(seed + 0x9E3779B97F4A7C15 * (vid + 1)) ^ (8 * step + channel)), where vid = vehicle_offset + b is the
 *              global vehicle id, step = k (the observer step, from 1) and channel 0..4 = psi, psiDot, x, y, v;
 *   u1       = ((mix(key + 0x9E3779B97F4A7C15) >> 11) + 1) * 2^-53  in (0, 1],
 *   u2       = (mix(key + 2 * 0x9E3779B97F4A7C15) >> 11) * 2^-53    in [0, 1),
 *   g        = sqrt(-2 log u1) * cos(2 pi u2).
 *   A vehicle's noise therefore depends on (seed, vid, step, channel) only: not on B, the batch or the GPU.
 *
 * Schedule inside a control tick of a fleet with an observer, for each of the n_sub plant steps: plant step under the
 * current command, sensors from the new plant state, one observer step with u = [servo, motor] (delays 0).  The controller's
 * measurement is then built from the ESTIMATE instead of the plant: [max(vx, 0.01), vy, psiDot] and the map's local frame of
 * (x, y, yaw), with quirk Q9 as without an observer.  The estimate starts at [init_vx, 0, 0, x0, y0, yaw0] of plant0.
 * Pinned by tests/golden/estimator/estimator.npz (generated from the reference's own Estimator and Simulator) and the
 * numpy restatement in tests/_observer_ref.py. */
typedef struct lpvmpc_observer_config {
    double  L_ls[6 * 5 * 16];       /* Llmi of the low-speed polytope, [6][5][16] row-major (Estimator_Gains_LS.mat, EST:230) */
    double  lim_ls[6 * 2];          /* SchedVars_Limits of the low-speed polytope, [6][2] = {min, max} per scheduling row */
    double  L_hs[6 * 5 * 16];       /* the same for the high-speed polytope (Estimator_Gains_HS.mat, EST:233-234) */
    double  lim_hs[6 * 2];
    double  loop_rate;              /* 200 Hz: dt = 1 / loop_rate                               EST:47 */
    double  init_vx;                /* initial vx estimate (simulator/init_vx)                  EST:262 */
    double  psi_std, psiDot_std;    /* IMU noise (simulator/psi_std, psiDot_std)                MAIN_LAUNCH:60-87: 0 */
    double  x_std, y_std;           /* GPS noise                                                0 */
    double  v_std;                  /* encoder noise                                            0 */
    double  n_bound;                /* clipping bound in standard deviations                    0.5 */
    double  gps_freq;               /* GPS publish rate (Hz)                                    1000 */
    uint64_t seed;                  /* noise key */
    int64_t vehicle_offset;         /* global id of vehicle 0 of this fleet (sharded fleets draw like one big fleet) */
} lpvmpc_observer_config;

/* The launch file's sensor values (every std 0, n_bound 0.5, gps_freq 1000), loop_rate 200, init_vx 0.2, seed 0, offset 0;
 * the gain and limit tables are zeroed: the caller supplies them (the reference loads them from its .mat files). */
void lpvmpc_observer_default_config(lpvmpc_observer_config *cfg);

/* Attach (cfg != NULL) or remove (cfg == NULL) the estimator of a controller handle.  It takes effect at the next
 * lpvmpc_cl_init or lpvmpc_cascade_init on that handle (the controller handle of a cascade); a handle that never calls this
 * behaves exactly as without an estimator.  In a cascade both nodes measure the estimate: the controller's racing-phase
 * measurement (CMAIN:179-180,198-283) and the planner's first state (PMAIN:141) read it in place of the plant, with the same
 * per-plant-step schedule; the cascade starts at the lap event of a running vehicle, so its estimate starts at the plant state
 * [vx, vy, psiDot, x, y, yaw] of plant0 (GPS hold at the start position, step counter 0). */
int lpvmpc_observer_setup(lpvmpc_handle *h, const lpvmpc_observer_config *cfg);

/* The fleet's, cascade's or race's estimator state (synchronises like lpvmpc_cl_read; either pointer may be NULL): est [B][6] the current estimate,
 * meas [B][5] the measurement y of the latest observer step. */
int lpvmpc_observer_read(lpvmpc_handle *h, double *est, double *meas);

/* One observer step for each of B independent instances (tests, the drop-in GainScheduledLPVObserver): est [B][6] in/out,
 * y [B][5], u [B][2] = {servo, motor}, k [B] the step index (t = k dt).  aux [B][78] (may be NULL) receives L_gain [6][5],
 * A_obs [6][6] and B_obs [6][2] of the step.  Refused while the handle runs a fleet, like the other batch calls. */
int lpvmpc_observer_step_batch(lpvmpc_handle *h, int32_t B, const lpvmpc_observer_config *cfg, double *est, const double *y,
                               const double *u, const int32_t *k, double *aux);

/* ---------------------------------------------------------------------------------------------------------------
 * Actuator delay and servo lag (vehicleSimulator.py = SIM, main loop SIM:53-78) in the device plant, and fleets whose
 * controllers carry a steering delay.  All entry points here are new; the calls above keep their behaviour and refusals.
 *
 * Per vehicle and simulator step k (the vehicle's own plant-step counter; dt = dt_sim) the plant receives
 *   a     = motor command of step k - La   (0 while k < La)                  La = delay_a  (a_his, SIM:53)
 *   delta = servo command of step k - Ld   (0 while k < Ld)                  Ld = delay_df (df_his, SIM:54)
 * with La / Ld in simulator steps, 0 .. LPVMPC_ACT_MAX_DELAY; the reference's configuration is in seconds and its FIFO
 * length is int(delay / dt), truncation included (int(0.145 / 0.005) = 28): the Python helper actuator_config converts.
 * With low_level_dyn the servo filter runs on the DELAYED steering and is what the plant receives (SIM:70-72):
 *   servo_inp = (1 - dt / servo_tf) * servo_inp + (dt / servo_tf) * delta,   servo_inp = 0 at the start, servo_tf = 0.07.
 * The estimator, where it runs, is fed the COMMANDED input (it subscribes to `ecu`, stateEstimator.py:785); its own delays
 * stay 0 (stateEstimator.py:42-43).  Frozen (finished, lost) race vehicles advance neither plant nor actuator.
 *
 * Actuator state of one vehicle, host layout of lpvmpc_plant_step_actuated_batch / lpvmpc_actuator_read:
 *   act_state [B][LPVMPC_ACT_WORDS] = [motor ring (64), servo ring (64), servo_inp, k]: ring slot k % 64 holds the command of
 *   plant step k (the last 64 commands), k is the number of plant steps taken (an exact integer).  A fresh state is all zeros.
 *
 * Controllers with steeringDelay d = 1 .. 8 (lpvmpc_config.steering_delay) in a fleet: each controller keeps its history
 * u_old [B][2 + d] = [OldSteering[0], OldAccelera[0], OldSteering[1 .. d]] (CTRL:71-73, 395, 523), zeros at the start.  On each
 * tick, before its solve, the controller of the vehicle's lap appends the last command and drops the oldest entry
 * (CMAIN:289-298: `path` on lap 0, `tt` from the lap-event tick on).  Quirk kept: on the event tick `tt`'s history has only
 * been updated once, so it is [0, .., 0, last servo] -- its dR term and its first d - 1 pinned steerings read zeros.  With d = 0
 * the history is the last command, as in the calls above.  The reference pairs the two delays as
 * Steering_Delay = int(delay_df / dt) (CMAIN:52; dt = 1/30): the Python helper controller_delay.
 *
 * Per-vehicle delays: delay_a / delay_df are arrays of B entries or NULL (NULL: cfg's value for every vehicle).
 * Refused with LPVMPC_E_ARG: a delay < 0 or > LPVMPC_ACT_MAX_DELAY, servo_tf <= 0 with low_level_dyn, a race whose path and
 * tt handles have different steering delays.  lpvmpc_cascade_init keeps refusing delayed controllers (not extended here).
 * With cfg all off (no delays, no servo lag) and steering_delay 0 the new calls compute what the calls above compute, word
 * for word (they run the delayed kernels, whose actuator stage then passes the command through). */
#define LPVMPC_ACT_MAX_DELAY 64
#define LPVMPC_ACT_WORDS (2 * LPVMPC_ACT_MAX_DELAY + 2)
typedef struct lpvmpc_actuator_config {
    int32_t delay_a, delay_df;   /* simulator steps (0) */
    int32_t low_level_dyn;       /* 1: servo filter on the delayed steering (0) */
    int32_t reserved;            /* 0 */
    double  servo_tf;            /* filter time constant Tf, seconds (0.07, SIM:62) */
} lpvmpc_actuator_config;
void lpvmpc_actuator_default_config(lpvmpc_actuator_config *cfg);
/* n_sub simulator steps of B vehicles through the actuator stage under the held command u [B][2] = (motor, servo):
 * state [B][8] and act_state [B][LPVMPC_ACT_WORDS] are in / out, so a trace split over several calls equals one call.
 * A batch call like lpvmpc_plant_step_batch (refused while the handle runs a fleet). */
int  lpvmpc_plant_step_actuated_batch(lpvmpc_handle *h, int32_t B, double *state, double *act_state, const double *u,
                                      int32_t n_sub, double dt_sim, double mu_sim, const lpvmpc_actuator_config *cfg,
                                      const int32_t *delay_a, const int32_t *delay_df);
/* lpvmpc_cl_init with the actuator in the plant (dt = dt_sim) and a controller of any steering_delay (0 .. 8); an estimator
 * attached with lpvmpc_observer_setup runs as in lpvmpc_cl_init, fed the commanded input. */
int  lpvmpc_cl_init_actuated(lpvmpc_handle *h, int32_t B, const double *plant0, double half_width, double slack, int32_t q9_swap,
                             int32_t n_sub, double dt_sim, double mu_sim, const lpvmpc_actuator_config *act,
                             const int32_t *delay_a, const int32_t *delay_df);
/* lpvmpc_race_init / lpvmpc_race_init_observed (obs NULL: ground truth) with the actuator in the plant and path / tt handles
 * of the same steering_delay (0 .. 8). */
int  lpvmpc_race_init_actuated(lpvmpc_handle *path, lpvmpc_handle *tt, lpvmpc_handle *planner, int32_t B,
                               const double *plant0, const int32_t *half_track0, const lpvmpc_race_config *cfg,
                               const struct lpvmpc_observer_config *obs, const lpvmpc_actuator_config *act,
                               const int32_t *delay_a, const int32_t *delay_df);
/* of a fleet or race started by the two calls above (synchronises; any pointer may be NULL): act_state [B][LPVMPC_ACT_WORDS];
 * path_hist [B][2 + d]: the u_old history of the fleet's controller -- the lap-0 fleet makes the history step in the launch that
 * advances the plant, so this is what its NEXT solve reads -- or of the race's `path`, whose history steps in the next tick's
 * measurement, so this is what its LAST solve read; tt_hist [B][2 + d]: the race's `tt`, likewise (NULL for a fleet). */
int  lpvmpc_actuator_read(lpvmpc_handle *h, double *act_state, double *path_hist, double *tt_hist);

/* ---------------------------------------------------------------------------------------------------------------
 * Race recorder: telemetry and per-lap tracking statistics of a race, kept on the device (the controller node's ALL_LOCAL_DATA,
 * GLOBAL_DATA, References and the RMSE_ve / RMSE_ye / RMSE_thetae it declares, CMAIN:101-106,115,194-195,217-218,411-419).
 * While recording is on, lpvmpc_race_tick launches one more kernel per tick, after the command / plant kernel; with it off a
 * tick issues the launches it always did.  Recording changes no output of the race.
 *
 * Ring of records: recording keeps the last `capacity` records.  Tick t (the race's tick number as lpvmpc_race_read reports it,
 * counted before the tick) is recorded when (t - t_start) % stride == 0, t_start = the first tick after lpvmpc_race_record; record
 * k (0-based since the start) is tick t_start + k * stride.  Each record holds, per vehicle, the vehicle's state after the tick --
 * what lpvmpc_race_read would return after it -- in two planes, channel-major and vehicle-minor: f64 [LPVMPC_REC_F64][B] and
 * i32 [LPVMPC_REC_I32][B]:
 *   plant [x y vx vy ax ay yaw psiDot]; local: the tick's measurement [vx vy w epsi s ey] in lpvmpc_race_read's slots (quirk Q9
 *   swaps slots 3 / 5 in lap 0 with q9_swap); cmd [servo motor] applied on this tick; ref [x_ref y_ref yaw_ref vel_ref];
 *   track [s ey epsi]: Map.getLocalPosition of the ground-truth plant (lpvmpc_local_position_batch's function and sentinels);
 *   est [vx vy psiDot x y yaw]: the estimator's state (NaN on a race without one);
 *   phase, lap, src (controller that solved: -1 none, 0 path, 1 tt), iters, status (as lpvmpc_race_read), plan_iters /
 *   plan_status of a planner solve on this tick (-1 when the vehicle ran none), inside (the track frame's flag).
 * ref follows the node's References: [0 0 0 1] on every tick measured by the lap-0 branch, the event tick included
 * (CMAIN:194-195); on a racing tick the point the measurement's Body_Frame_Errors used and vel_ref[0] of the tt controller.  On
 * odd racing ticks this differs from the node's References row, which logs planning_data.*[0] of the newest message while the
 * `index` latch measures against the window read one tick earlier.
 *
 * Per-lap statistics, updated on every tick while recording is on (whatever the stride), per vehicle and lap l = 0 .. laps:
 * f64 [B][laps + 1][LPVMPC_LAPSTAT_F64], i32 [B][laps + 1][LPVMPC_LAPSTAT_I32].  A tick counts when the vehicle's controller
 * solved on it (src >= 0: not frozen, lost or finishing -- nothing of a finishing tick is applied) and goes to l = the lap counter
 * after its measurement, with the planner solve of the same tick, if any.  With e_v = local vx - vel_ref, ey / epsi the lateral /
 * heading error of the measurement -- local[5] / local[3], except on ticks measured by the lap-0 branch (phase 0 after the tick,
 * or the event tick) of a race with q9_swap, whose measurement stores them in local[3] / local[5] -- and ey_track = track ey,
 * in tick order:
 *   sse_v += e_v * e_v; sse_ey += ey * ey; sse_epsi += epsi * epsi; sum_vx += local vx (each s = s + x * x, rounded twice,
 *   no fused multiply-add); max_ey = |ey| if |ey| > max_ey; max_ey_track likewise (all start at 0; a NaN never replaces them);
 *   ticks, ctrl_iters (sum), ctrl_iters_max, ctrl_not_solved (status != LPVMPC_SOLVED), plan_ticks, plan_iters (sum),
 *   plan_iters_max, plan_not_solved, off_track (inside == 0).
 * RMSE_ve = sqrt(sse_v / ticks), likewise ey and epsi.  end_tick [B]: the tick on which the vehicle became finished or lost,
 * -1 while it runs or when it ended before recording started.
 *
 * lpvmpc_race_record starts recording from the next tick: it frees a previous recorder, allocates the ring and the statistics and
 * zeroes them.  capacity == 0 stops recording and frees them.  Refused with LPVMPC_E_ARG: no race on the handle, capacity < 0,
 * stride < 1, a size that overflows; with LPVMPC_E_NOMEM: a failed allocation, after which the race runs on unrecorded.  The
 * recorder belongs to the race: lpvmpc_cl_release(path) or destroying a handle frees it, and a new race starts unrecorded. */
#define LPVMPC_REC_F64            29
#define LPVMPC_REC_PLANT           0  /* 8 channels */
#define LPVMPC_REC_LOCAL           8  /* 6 */
#define LPVMPC_REC_CMD            14  /* 2 */
#define LPVMPC_REC_REF            16  /* 4 */
#define LPVMPC_REC_TRACK          20  /* 3 */
#define LPVMPC_REC_EST            23  /* 6 */
#define LPVMPC_REC_I32             8
#define LPVMPC_REC_PHASE           0
#define LPVMPC_REC_LAP             1
#define LPVMPC_REC_SRC             2
#define LPVMPC_REC_ITERS           3
#define LPVMPC_REC_STATUS          4
#define LPVMPC_REC_PLAN_ITERS      5
#define LPVMPC_REC_PLAN_STATUS     6
#define LPVMPC_REC_INSIDE          7
#define LPVMPC_LAPSTAT_F64              6
#define LPVMPC_LAPSTAT_SSE_V            0
#define LPVMPC_LAPSTAT_SSE_EY           1
#define LPVMPC_LAPSTAT_SSE_EPSI         2
#define LPVMPC_LAPSTAT_MAX_EY           3
#define LPVMPC_LAPSTAT_SUM_VX           4
#define LPVMPC_LAPSTAT_MAX_EY_TRACK     5
#define LPVMPC_LAPSTAT_I32              9
#define LPVMPC_LAPSTAT_TICKS            0
#define LPVMPC_LAPSTAT_CTRL_ITERS       1
#define LPVMPC_LAPSTAT_CTRL_ITERS_MAX   2
#define LPVMPC_LAPSTAT_CTRL_NOT_SOLVED  3
#define LPVMPC_LAPSTAT_PLAN_TICKS       4
#define LPVMPC_LAPSTAT_PLAN_ITERS       5
#define LPVMPC_LAPSTAT_PLAN_ITERS_MAX   6
#define LPVMPC_LAPSTAT_PLAN_NOT_SOLVED  7
#define LPVMPC_LAPSTAT_OFF_TRACK        8
typedef struct lpvmpc_race_record_config {
    int32_t capacity;         /* records kept (0: stop recording) */
    int32_t stride;           /* record every stride-th tick (>= 1) */
} lpvmpc_race_record_config;
int  lpvmpc_race_record(lpvmpc_handle *path, const lpvmpc_race_record_config *cfg);
/* synchronises and copies the last min(n, kept) records, oldest first (kept = min(total, capacity)): tick [m], f64 [m][LPVMPC_REC_F64][B],
 * i32 [m][LPVMPC_REC_I32][B] (any of the three may be NULL); total [1] = records written since recording started (0, and nothing
 * copied, while recording is off). */
int  lpvmpc_race_record_read(lpvmpc_handle *path, int32_t n, int32_t *total, int32_t *tick, double *f64, int32_t *i32);
/* synchronises and copies the per-lap statistics (any pointer may be NULL); refused with LPVMPC_E_ARG while recording is off */
int  lpvmpc_race_lap_stats(lpvmpc_handle *path, double *f64, int32_t *i32, int32_t *end_tick);

/* ---------------------------------------------------------------------------------------------------------------
 * Per-vehicle plant parameters: every vehicle of a lap-0 fleet or a race steps the simulated plant (Simulator.f, SIM:164-199)
 * with its own row of parameters, held on the device.  The controllers, the planner and the estimator keep the nominal model of
 * their handles unless rows are bound to them ("Per-vehicle model parameters", "Per-vehicle state estimator" below; the mismatch is the point: a Monte-Carlo sweep of how the controller holds up when the car is not the model it
 * was tuned on).  All entry points here are new; the calls above keep their behaviour and refusals.
 *
 * Host layout: plant_params [B][LPVMPC_PLANT_WORDS] = {lf, lr, m, Iz, Cf, Cr, mu} per vehicle.  Cf and Cr are the linear tyre
 * stiffnesses of the plant, FyF = Cf * aF, FyR = Cr * aR, where Simulator.f has the constant 60; mu is the simulator's drag
 * coefficient (simulator/mu).  n_sub and dt_sim stay fleet-wide.
 *   plant_params == NULL: every vehicle has the nominal row -- the handle's lf, lr, m, Iz (the path handle's, for a race),
 *     Cf = Cr = 60 (the simulator's constant, not the controller's Cf) and mu = mu_sim (cfg->mu_sim for a race).  With the nominal
 *     row each call computes what its _actuated counterpart computes, word for word.
 *   plant_params given: mu_sim (cfg->mu_sim for a race) is ignored.
 *   act == NULL: the actuator is all off (lpvmpc_actuator_default_config; delay_a / delay_df are ignored).  The calls run the
 *     delayed fleets' kernels in any case, so a fleet or race started here is read with lpvmpc_actuator_read as well, and its
 *     controllers may carry a steering delay as in the _actuated calls.
 * Refused with LPVMPC_E_ARG, nothing started or allocated: a non-finite word, lf, lr, m or Iz <= 0, Cf, Cr or mu < 0, and
 * everything the _actuated calls refuse.  The rows belong to the fleet or race: lpvmpc_cl_release frees them, and a later
 * lpvmpc_cl_init* on the handle runs nominal.  lpvmpc_cascade_init stays nominal (not extended here). */
#define LPVMPC_PLANT_WORDS 7
/* lpvmpc_plant_step_actuated_batch with a row per vehicle; act_state may be NULL when act is NULL (a fresh all-off actuator,
 * not returned). */
int  lpvmpc_plant_step_vehicles_batch(lpvmpc_handle *h, int32_t B, double *state, double *act_state, const double *u,
                                      int32_t n_sub, double dt_sim, double mu_sim, const lpvmpc_actuator_config *act,
                                      const int32_t *delay_a, const int32_t *delay_df, const double *plant_params);
/* lpvmpc_cl_init_actuated with a row per vehicle; an estimator attached with lpvmpc_observer_setup runs as in
 * lpvmpc_cl_init_actuated. */
int  lpvmpc_cl_init_vehicles(lpvmpc_handle *h, int32_t B, const double *plant0, double half_width, double slack, int32_t q9_swap,
                             int32_t n_sub, double dt_sim, double mu_sim, const lpvmpc_actuator_config *act,
                             const int32_t *delay_a, const int32_t *delay_df, const double *plant_params);
/* lpvmpc_race_init_actuated with a row per vehicle (obs NULL: ground truth). */
int  lpvmpc_race_init_vehicles(lpvmpc_handle *path, lpvmpc_handle *tt, lpvmpc_handle *planner, int32_t B,
                               const double *plant0, const int32_t *half_track0, const lpvmpc_race_config *cfg,
                               const struct lpvmpc_observer_config *obs, const lpvmpc_actuator_config *act,
                               const int32_t *delay_a, const int32_t *delay_df, const double *plant_params);
/* the rows [B][LPVMPC_PLANT_WORDS] of the fleet or race that h runs (the path handle, for a race), started by the two calls
 * above (synchronises). */
int  lpvmpc_plant_params_read(lpvmpc_handle *h, double *plant_params);

/* ---------------------------------------------------------------------------------------------------------------
 * Per-vehicle model parameters: every instance of a batch -- every vehicle of a fleet, cascade or race -- is linearised with a
 * model row of its own instead of the vehicle words lf, lr, m, Iz, Cf, Cr, mu of the handle's configuration: a heterogeneous batch
 * on one handle, or the model side of a mismatch study (matched to each vehicle's plant row, or off by a chosen error).  dt, the
 * track table, limits, weights and the OSQP settings stay the handle's.  Both entry points are new; every call above keeps its
 * behaviour and refusals, and a handle without a binding (the default) launches what it launched before.
 *
 * Host layout: model_params [B][LPVMPC_MODEL_WORDS] = {lf, lr, m, Iz, Cf, Cr, mu} per vehicle, the word order of the plant rows.
 *
 * The binding belongs to the handle and acts wherever the handle linearises: lpvmpc_lpv_batch, lpvmpc_estimate_abc_batch,
 * lpvmpc_solve_batch, _masked and _dev, seed mode, the lap-0 fleet (lpvmpc_cl_init*), the cascade (lpvmpc_cascade_init; bind the
 * controller and the planner handle separately) and the race (lpvmpc_race_init*; path, tt and planner handle separately: the same
 * rows, or not).  Vehicle b takes row b: the row is indexed by vehicle, not by launch slot, so masked launches work unchanged.
 *   - Bound, every such call must have the binding's batch size: another B is refused with LPVMPC_E_ARG before anything is
 *     launched (the engines check it at init).
 *   - The controller roll-out (lpvmpc_lpv_batch and the solves of a controller handle) takes the row's Cf for BOTH axles -- the
 *     reference passes Cf_new for both (CTRL:203-218) -- and the call's cf_new (the literal 60.0 of the fleet, cascade and race
 *     engines) is ignored, as mu_sim is ignored when plant rows are given.  The controller's seed-mode linearisation and the
 *     planner take the row's Cf and Cr, as they take the handle's without a binding.
 *   - Every value is formed by the same operations in the same order as without a binding: a row equal to the handle's words (and
 *     Cf equal to the call's cf_new, for the controller roll-out) gives the same words as the unbound handle.
 *   - lpvmpc_solve_batch_AB takes the caller's blocks and is unaffected (any B).  The estimator does not read these rows: it has a
 *     binding of its own, with gain tables designed for each row ("Per-vehicle state estimator" below).
 * lpvmpc_set_model_params copies the rows to the device (synchronises); B = 0 unbinds (model_params is then ignored).  Refused with
 * LPVMPC_E_ARG, the binding unchanged: a non-finite word, lf, lr, m or Iz <= 0, Cf, Cr or mu < 0 (the plant rows' rules), B < 0,
 * B > 0 with model_params NULL, and any call while the handle runs a fleet, cascade or race (as stand-alone batch calls are
 * refused then; lpvmpc_cl_release ends it).  lpvmpc_destroy frees the table.
 * lpvmpc_model_params_read: *B = the binding's batch size (0: unbound) and, if model_params is not NULL, the bound rows
 * [*B][LPVMPC_MODEL_WORDS] as they were set (synchronises). */
#define LPVMPC_MODEL_WORDS 7
int  lpvmpc_set_model_params(lpvmpc_handle *h, int32_t B, const double *model_params);
int  lpvmpc_model_params_read(lpvmpc_handle *h, int32_t *B, double *model_params);

/* ---------------------------------------------------------------------------------------------------------------
 * Per-vehicle tunings: every instance of a batch -- every vehicle of a fleet, cascade or race -- builds its QP with weights and box
 * limits of its own instead of Q, R, dR, L_cf and the ctrl_* / plan_* limits of the handle's configuration: one batch, fleet or race
 * evaluates as many controller or planner tunings as it has instances.  The OSQP settings, the horizon, steering_delay, dt, the
 * track table and the vehicle words stay the handle's.  All four entry points are new; every call above keeps its behaviour and
 * refusals, and a handle without a binding (the default) computes what it computed before.
 *
 * Public row, LPVMPC_TUNING_WORDS doubles in the units of lpvmpc_config:
 *   [0..35]  Q, nx*nx row-major in the first nx*nx slots        [36..39] R        [40..41] dR
 *   [42..47] L_cf (planner; ignored by a controller)
 *   [48..63] limits.  Controller: [48] vx_min, [49] max_vel, [50] delta_max, [51] a_max, [52] a_min_abs; the rest is ignored.
 *            Planner: [48..52] xmin, [53..57] xmax, [58..59] umin, [60..61] umax; xmin[0] and xmax[0] are min_vel and max_vel;
 *            slot 3 (ey) of xmin / xmax is ignored: max_ey stays the per-instance argument it is.
 * Ignored words are stored and read back as set.
 *
 * Table layout: rows [B][LPVMPC_TUNING_WORDS], instance-major, on the host and on the device.  The consumer is the solve kernel's
 * set-up block, one workgroup per instance, which reads its 512-byte row at wave-uniform addresses.  (The plant and model tables
 * are parameter-major on the device because their consumers are one lane per vehicle.)
 *
 * lpvmpc_tuning_from_config (host only): the public row a handle created from cfg solves with.
 * lpvmpc_tuning_device_row (host only): the 64 words the kernel reads for a public row -- the block Q R dR Lcf box_lo[8] box_hi[8]
 * of the device configuration (controller box rows: -vx <= -vx_min, vx <= max_vel, +-delta <= delta_max, a <= a_max,
 * -a <= a_min_abs, lower bounds -inf; planner: the state and input boxes).  lpvmpc_create fills its configuration block through
 * these two: the device row of a handle's own configuration is that handle's block, bit for bit.
 *
 * The binding belongs to the handle and acts wherever the handle solves: lpvmpc_solve_batch, _AB (unlike the model binding), _dev
 * and _masked, seed mode, warm starts, straggler deferral, the lap-0 fleet (lpvmpc_cl_init*), the cascade and the race started
 * afterwards (bind each handle they are made of separately: the same rows, or not).  Instance b takes row b: the row is indexed by
 * vehicle, not by launch slot, so masked launches work unchanged.  A parked instance carries its words in its image: resume
 * passes, riders and the tail kernel read nothing from the table.
 *   - Bound, every such call must have the binding's batch size: another B is refused with LPVMPC_E_ARG before anything is
 *     launched (the engines check it at init).
 *   - Every value is formed by the same operations in the same order as without a binding: the handle's own row bound to every
 *     instance gives the same words as the unbound handle.
 * lpvmpc_set_tunings joins the handle's parked work, copies the rows to the device and synchronises; B = 0 unbinds (rows is then
 * ignored).  Refused with LPVMPC_E_ARG, the binding unchanged: a non-finite weight word (of those the handle's kind reads), a NaN
 * limit (infinite limits stay legal: the kernel clips to +-1e30), a lower limit above its upper one (vx_min > max_vel,
 * delta_max < 0, a_max < -a_min_abs, xmin > xmax, umin > umax), B < 0, B > 0 with rows NULL, and any call while the handle runs a
 * fleet, cascade or race.  lpvmpc_destroy frees the table.
 * lpvmpc_tunings_read: *B = the binding's batch size (0: unbound) and, if rows is not NULL, the bound public rows as they were set. */
#define LPVMPC_TUNING_WORDS 64
int  lpvmpc_set_tunings(lpvmpc_handle *h, int32_t B, const double *rows);
int  lpvmpc_tunings_read(lpvmpc_handle *h, int32_t *B, double *rows);
int  lpvmpc_tuning_from_config(const lpvmpc_config *cfg, double *row);
int  lpvmpc_tuning_device_row(int32_t kind, const double *row, double *dev);

/* ---------------------------------------------------------------------------------------------------------------
 * Tyre model: every vehicle of a lap-0 fleet or a race steps the simulated plant with a tyre row of its own next to its plant row.
 * The reference's simulator ships two tyres: the linear one that Simulator.f uses (FyF = 60 * a_F, SIM:174-175) and
 * Simulator.pacejka (SIM:202-205), whose two calls in f are commented out (SIM:172-173) and whose parameters the launch file sets
 * (simulator/B = 6.0, simulator/C = 1.6, simulator/c_f = 0.8).  The controllers, the planner and the estimator keep their linear
 * model.  All entry points here are new; the calls above keep their behaviour and refusals.
 *
 * Host layout: tyre_params [B][LPVMPC_TYRE_WORDS] = {kind, B, C, c_f} per vehicle.
 *   kind 0: the linear tyre of the vehicle's plant row, FyF = Cf * aF, FyR = Cr * aR; B, C, c_f are ignored (stored and read back).
 *     A kind 0 vehicle computes what it computes in the _vehicles call, word for word.
 *   kind 1: Pacejka on both axles, Fy = D * sin(C * atan(B * a)) with D = ((c_f * m) * 9.81) / 2 and m the mass of the vehicle's plant
 *     row.  Slip angles and the |vx| > 0.2 gate are Simulator.f's.
 *   tyre_params == NULL: kind 0 for every vehicle.
 * kind is per vehicle: one fleet may mix both.  plant_params, act, delay_a, delay_df: as in the _vehicles calls.
 * Refused with LPVMPC_E_ARG, nothing started or allocated and a running fleet or race left as it is: kind other than exactly 0 or 1,
 * a non-finite or negative B, C or c_f, and everything the _vehicles calls refuse.  The rows belong to the fleet or race:
 * lpvmpc_cl_release frees them.  lpvmpc_cascade_init keeps the linear tyre (not extended here). */
#define LPVMPC_TYRE_WORDS 4
/* lpvmpc_plant_step_vehicles_batch with a tyre row per vehicle */
int  lpvmpc_plant_step_tyres_batch(lpvmpc_handle *h, int32_t B, double *state, double *act_state, const double *u,
                                   int32_t n_sub, double dt_sim, double mu_sim, const lpvmpc_actuator_config *act,
                                   const int32_t *delay_a, const int32_t *delay_df, const double *plant_params,
                                   const double *tyre_params);
/* lpvmpc_cl_init_vehicles with a tyre row per vehicle */
int  lpvmpc_cl_init_tyres(lpvmpc_handle *h, int32_t B, const double *plant0, double half_width, double slack, int32_t q9_swap,
                          int32_t n_sub, double dt_sim, double mu_sim, const lpvmpc_actuator_config *act,
                          const int32_t *delay_a, const int32_t *delay_df, const double *plant_params, const double *tyre_params);
/* lpvmpc_race_init_vehicles with a tyre row per vehicle */
int  lpvmpc_race_init_tyres(lpvmpc_handle *path, lpvmpc_handle *tt, lpvmpc_handle *planner, int32_t B,
                            const double *plant0, const int32_t *half_track0, const lpvmpc_race_config *cfg,
                            const struct lpvmpc_observer_config *obs, const lpvmpc_actuator_config *act,
                            const int32_t *delay_a, const int32_t *delay_df, const double *plant_params, const double *tyre_params);
/* the rows [B][LPVMPC_TYRE_WORDS] of the fleet or race that h runs (the path handle, for a race), started by the two calls above
 * (synchronises); lpvmpc_plant_params_read returns its plant rows. */
int  lpvmpc_tyre_params_read(lpvmpc_handle *h, double *tyre_params);
/* the curve alone, on the device: force [B] = the lateral force of tyre row b at slip angle alpha [B] for a vehicle of mass m [B]
 * (finite, > 0).  A kind 0 row has no stiffness of its own here and gives Simulator.f's 60 * alpha.  Refused while the handle runs a
 * fleet, cascade or race, like the other batch calls. */
int  lpvmpc_tyre_force_batch(lpvmpc_handle *h, int32_t B, const double *tyre_params, const double *m, const double *alpha,
                             double *force);

/* ---------------------------------------------------------------------------------------------------------------
 * Per-vehicle state estimator: gain tables designed on the device for each vehicle's own model row.  The gain-scheduled estimator
 * above blends the gains of the 16 vertices of a polytope; those gains belong to the model they were designed on.  Here the
 * design runs on the device, one problem per (vehicle b, polytope p in {LS, HS}, vertex i in 0..15, in the order of the
 * estimator's vertex weights: bit 3 = vx, bit 2 = vy, bit 1 = steer, bit 0 = theta of i takes the maximum):
 *   A = A_obs(vx, vy, theta, steer) at the vertex, formed as the observer step forms it, with the seven constants taken from the
 *   vehicle's row {lf, lr, m, Iz, Cf, Cr, mu} (the plant rows' order);
 *   P solves the filter equation A P + P A^T - P C^T Ro^-1 C P + Qo = 0;  L = -P C^T Ro^-1 [6][5], so that A + L C is Hurwitz.
 * Method: matrix-sign Newton iteration on the Hamiltonian [[A^T, -C^T Ro^-1 C], [-Qo, -A]] with Frobenius-norm scaling, stopped
 * when the step is <= 1e-13 of the iterate (cap: 40 iterations), P from the normal equations of the sign's stable subspace,
 * symmetrised.  A vehicle's tables do not depend on the batch around it (no atomics, fixed summation order).
 * A problem that does not meet the stop rule within the cap gets NaN gains and the iteration count -1.
 *
 * lpvmpc_observer_design_batch: rows [B][LPVMPC_PLANT_WORDS]; L_ls, L_hs [B][6][5][16] (the layout of lpvmpc_observer_config's tables
 * per vehicle); iters [B][2][16] (may be NULL) the Newton iterations of each problem.  Refused with LPVMPC_E_ARG, the outputs
 * untouched: a row the plant rows' rules refuse (non-finite word, lf, lr, m, Iz <= 0, Cf, Cr, mu < 0), Ro not symmetric positive
 * definite, Qo not symmetric positive semidefinite or with a non-finite word, a limit row 0, 1, 3 or 5 with max <= min, a lower vx
 * limit <= 0, B > LPVMPC_OBSERVER_DESIGN_MAX_B, and any call while the handle runs a fleet, cascade or race. */
#define LPVMPC_OBSERVER_DESIGN_MAX_B (1 << 22)
typedef struct lpvmpc_observer_design {
    double lim_ls[6 * 2], lim_hs[6 * 2];    /* SchedVars_Limits of the two polytopes, as in lpvmpc_observer_config */
    double Qo[6 * 6], Ro[5 * 5];            /* process and measurement weights of the filter equation */
} lpvmpc_observer_design;
/* Qo = I, Ro = diag(0.1, 0.1, 0.01, 0.01, 0.01); the limit tables are zeroed: the caller's */
void lpvmpc_observer_default_design(lpvmpc_observer_design *d);
int  lpvmpc_observer_design_batch(lpvmpc_handle *h, int32_t B, const double *rows, const lpvmpc_observer_design *d,
                                  double *L_ls, double *L_hs, int32_t *iters);

/* The binding: a model row and the two gain tables per vehicle on a controller handle (for a race: the path handle).  An estimator
 * of a fleet or race started on the handle by lpvmpc_cl_init_vehicles, lpvmpc_cl_init_tyres, lpvmpc_race_init_vehicles or
 * lpvmpc_race_init_tyres then runs vehicle b's observer step with row b's seven words in A_obs and B_obs and with vehicle b's
 * tables; the tables of the estimator configuration are ignored, its limit tables, polytope switch, sensors and noise stay.  Every
 * value is formed by the same operations in the same order as without a binding: the nominal row {0.125, 0.125, 1.98, 0.03, 60,
 * 60, 0.05} with tables equal to the configuration's gives the unbound estimator's words.  A handle without a binding (the default)
 * launches what it launched before.
 *   lpvmpc_set_observer_vehicles: rows [B][LPVMPC_PLANT_WORDS], and exactly one of (L_ls and L_hs, [B][6][5][16] each: the caller's
 *     tables, finite) or design (the tables are designed on the device straight into the binding, no host copy; a problem that does
 *     not converge fails the call with LPVMPC_E_ARG and a message naming vehicle and vertex).  B = 0 unbinds.  Synchronises.
 *     Refused with LPVMPC_E_ARG, the previous binding kept: what lpvmpc_observer_design_batch refuses, neither or both of tables
 *     and design, a planner handle, and any call while the handle runs a fleet, cascade or race.  lpvmpc_cl_release keeps the
 *     binding, lpvmpc_destroy frees it.
 *   Starts: with an estimator configured, the four calls above refuse another B than the binding's and a designed binding whose limit
 *     tables differ from the estimator configuration's; every other start of a fleet or race with an estimator and
 *     lpvmpc_cascade_init with one refuse a bound handle.  Starts without an estimator ignore the binding.
 *   lpvmpc_observer_vehicles_read: *B = the binding's batch size (0: unbound) and, where not NULL, the rows and tables as bound.
 *   lpvmpc_observer_step_vehicles_batch: lpvmpc_observer_step_batch with a row and tables per instance (cfg's own tables are ignored). */
int  lpvmpc_set_observer_vehicles(lpvmpc_handle *h, int32_t B, const double *rows, const double *L_ls, const double *L_hs,
                                  const lpvmpc_observer_design *design);
int  lpvmpc_observer_vehicles_read(lpvmpc_handle *h, int32_t *B, double *rows, double *L_ls, double *L_hs);
int  lpvmpc_observer_step_vehicles_batch(lpvmpc_handle *h, int32_t B, const lpvmpc_observer_config *cfg, double *est, const double *y,
                                         const double *u, const int32_t *k, double *aux, const double *rows, const double *L_ls,
                                         const double *L_hs);

/* ---------------------------------------------------------------------------------------------------------------
 * Per-vehicle tracks: every instance of a batch is transformed and linearised on a track of its own instead of the one table of
 * the handle's configuration: one batch on several circuits, mirrored or scaled variants of one, a tuning sweep crossed with a track
 * sweep.  The binding is a palette of T tracks plus one palette index per vehicle, not B tables: a batch uses a handful of
 * circuits, and a palette of at most LPVMPC_MAX_TRACKS * 768 bytes stays in the cache.  dt, N, the vehicle words, limits, weights
 * and the OSQP settings stay the handle's.  Both entry points are new; a handle without a binding (the default) launches what it
 * launched before.
 *
 * Host layout: track_rows [T] the rows of each track in use (2 .. LPVMPC_MAX_TRACK_ROWS); tables [T][LPVMPC_MAX_TRACK_ROWS * 6],
 * the PointAndTangent rows [x, y, psi, cum_s, seg_len, curvature] of lpvmpc_config::track per track (rows beyond track_rows are
 * ignored and read back as zero); half_width [T], slack [T]; track_of [B] the palette entry of each vehicle, 0 .. T-1.
 *
 * The binding belongs to the handle and acts on: lpvmpc_local_position_batch and lpvmpc_global_position_batch; wherever the
 * handle linearises in a batch call: lpvmpc_lpv_batch, lpvmpc_estimate_abc_batch, lpvmpc_solve_batch, _masked and _dev (the
 * curvature look-ups of the controller at lap 0, of its seed mode and of the planner); lpvmpc_handoff_batch on a bound planner
 * handle (curvature and centre-line pose from each vehicle's track); the lap-0 fleet started through lpvmpc_cl_init_tyres and the
 * race started through lpvmpc_race_init_tyres, the most general entry points (measurement from the plant or from the estimate, seed
 * mode, the LPV roll-outs and the planner of every tick; with or without an estimator, per-vehicle estimator included).  Vehicle b
 * takes track track_of[b]: indexed by vehicle, not by launch slot, so masked launches work unchanged.
 *   - In a race path, tt and planner are bound separately and must carry equal bindings (T, B, track_rows, tables, half_width,
 *     slack, track_of): all three, or none; anything else is refused.  Equal bindings replace the comparison of the handles' own
 *     tables.  The lap-event rules take the vehicle's own lap length L: HalfTrack at s >= 3L/4, the event at s <= L/4, the racing
 *     rule s >= L - L/10.  The recorder's track frame is the vehicle's own track, width and slack.  plan_max_ey stays one value per
 *     race, max_ey the per-instance argument it is.
 *   - Bound, every such call must have the binding's B: another B is refused with LPVMPC_E_ARG before anything is launched.
 *   - lpvmpc_local_position_batch, lpvmpc_cl_init_tyres and lpvmpc_race_init_tyres (lpvmpc_race_config) take each track's half_width
 *     and slack; the call's own are ignored, as mu_sim is ignored when plant rows are given.
 *   - Every value is formed by the same operations in the same order as without a binding: an instance computes, word for word,
 *     what a handle created with its track computes (called with that track's half width and slack), with or without model rows
 *     bound beside the tracks.  A handle without model rows linearises on a table of its own vehicle words and takes the call's
 *     cf_new as without a binding.
 *   - lpvmpc_solve_batch_AB reads no track and is unaffected (any B).  A bound handle needs no track table of its own.
 *   - The controller roll-out without its [A | B] blocks (states only) has no bound form: no entry point asks for it, and the
 *     library refuses it by name (LPVMPC_E_ARG) rather than run another kernel.
 *   - lpvmpc_cl_init, _actuated and _vehicles refuse a bound handle with LPVMPC_E_ARG and a message that names lpvmpc_cl_init_tyres
 *     (with NULL rows it computes what they compute, word for word).  A vehicle of a bound fleet computes, bit for bit, what it
 *     computes in a fleet on a handle created with its track.  lpvmpc_race_init, _observed, _actuated and _vehicles refuse bound
 *     handles likewise and name lpvmpc_race_init_tyres.
 *   - lpvmpc_cascade_init refuses a bound handle (controller or planner) with LPVMPC_E_ARG: the cascade runs on the handle's own
 *     track.
 * lpvmpc_set_tracks copies the binding to the device (synchronises); T = 0 or B = 0 unbinds (the arrays are then ignored).  Refused
 * with LPVMPC_E_ARG, the binding unchanged: T outside 1 .. LPVMPC_MAX_TRACKS, a track_rows outside 2 .. LPVMPC_MAX_TRACK_ROWS, a
 * non-finite table word in the rows in use, a segment length <= 0, a non-finite or negative half_width or slack, a track_of[b]
 * outside 0 .. T-1, B < 0, a NULL array, and any call while the handle runs a fleet, cascade or race.  lpvmpc_destroy frees it.
 * lpvmpc_tracks_read: *T and *B of the binding (0, 0: unbound) and, where not NULL, the arrays as they were set. */
#define LPVMPC_MAX_TRACKS 64
int  lpvmpc_set_tracks(lpvmpc_handle *h, int32_t T, const int32_t *track_rows, const double *tables, const double *half_width,
                       const double *slack, int32_t B, const int32_t *track_of);
int  lpvmpc_tracks_read(lpvmpc_handle *h, int32_t *T, int32_t *B, int32_t *track_rows, double *tables, double *half_width,
                        double *slack, int32_t *track_of);

/* ---------------------------------------------------------------------------------------------------------------
 * Plant disturbances: gusts, a kick and low-grip patches for the vehicles of a lap-0 fleet or a race.  The reference's simulator has
 * sensor noise only; its dynamics are deterministic and uniform along the lap.  The model here acts at the control tick, on every
 * tick on which a vehicle's plant advances n > 0 simulator steps, after that tick's solve and immediately before its command / plant
 * kernel (one more launch per tick; with nothing attached a tick issues the launches it always did).  k0 is the vehicle's own
 * plant-step counter, j its own count of disturbed ticks since the binding was attached, vid = vehicle_offset + b.  In order:
 *   1. grip: (s, ey, epsi, inside) = Map.getLocalPosition of the ground-truth plant pose on the vehicle's own track (the handle's
 *      table, or the vehicle's palette entry where tracks are bound; with an estimator in the loop it still reads the plant).
 *      gamma = the product of gamma_p over the patches p in {0, 1} that contain s, 1 when inside == 0 or no patch does.  A patch
 *      contains s when d < len, d = s - s0 and d += L when d < 0 (L: the lap length of the vehicle's track, so a patch may span the
 *      start line).  The live tables' words become Cf = gamma * Cf_base, Cr = gamma * Cr_base (plant row) and c_f = gamma * c_f_base
 *      (tyre row): the linear tyre's stiffnesses and the Pacejka peak D.  gamma == 1 leaves the base words bit for bit.
 *   2. gusts: for each channel c in {0: ax, 1: ay, 2: yaw acceleration} with sigma_c != 0,
 *      g = clip(gauss(seed ^ LPVMPC_DIST_STREAM, vid, j, c), +-n_bound) on the estimator's counter-based generator;
 *      d_c = sigma_c * g on j == 0, else d_c = rho * d_c + sigma_c * q * g with q = sqrt(1 - rho^2) formed once on the host: a
 *      stationary first-order Gauss-Markov process of variance sigma_c^2 on every tick.  With T = n * dt_sim it is applied as an
 *      impulse: vx = |vx + d_0 T|, vy += d_1 T, psiDot += d_2 T.  A channel with sigma_c == 0 draws nothing and adds nothing.
 *   3. kick: if k0 <= kick_step < k0 + n: vy += kick_vy, psiDot += kick_w.  Once; kick_step < 0: never.
 *   4. j += 1.
 * Frozen vehicles (finished, lost) are not touched and their j stays put, so a vehicle's draws depend on (seed, vid, j) only: not on
 * B, the other vehicles or how a fleet is sharded.  An all-off row (sigma = 0, kick_step = -1, len = 0 or gamma = 1) changes no word
 * of plant or tables.
 *
 * Host layouts: rows [B][LPVMPC_DIST_WORDS] = {sigma_ax, sigma_ay, sigma_aw, rho, kick_step, kick_vy, kick_w, p0_s0, p0_len,
 * p0_gamma, p1_s0, p1_len, p1_gamma}; state [B][LPVMPC_DIST_STATE] = {d_ax, d_ay, d_aw, ticks (= j), gamma (of the last disturbed
 * tick; 1 before the first)}.
 *
 * lpvmpc_set_disturbances attaches rows to the lap-0 fleet or race that h runs (the path handle, for a race), from the next tick on;
 * cfg NULL: the defaults.  The fleet or race must have plant and tyre tables (lpvmpc_cl_init_tyres / lpvmpc_race_init_tyres): there is
 * nothing to scale otherwise.  Attaching again replaces the binding (state and j start over, the base rows stay).  rows == NULL
 * detaches: the live words are restored from the base copy and the state is freed.  lpvmpc_cl_release frees the binding; a new fleet
 * starts undisturbed.  While a binding is attached lpvmpc_plant_params_read and lpvmpc_tyre_params_read return the base rows.
 * Refused with LPVMPC_E_ARG, a running fleet left exactly as it is: no fleet or race on the handle or one without the tables, another
 * B than the fleet's, a non-finite word, sigma < 0, rho outside [0, 1), kick_step not integer-valued or >= 2^31, s0 < 0 or >= the
 * vehicle's lap length, len < 0 or > the lap length, gamma < 0, n_bound <= 0.  lpvmpc_disturbances_read: the rows as they were set
 * and the state (synchronises); either pointer may be NULL.  lpvmpc_cascade_init is not extended.
 *
 * lpvmpc_plant_step_disturbed_batch: lpvmpc_plant_step_tyres_batch as one tick of n_sub steps with the model in front of it, on the
 * handle's track or its track binding (an unbound handle takes lpvmpc_race_default_config's half_width and slack for the
 * transform); dist_state [B][LPVMPC_DIST_STATE] is read and written (NULL: fresh, nothing returned; refused: a non-finite d word, a
 * tick count that is not an integer >= 0). */
#define LPVMPC_DIST_WORDS 13
#define LPVMPC_DIST_STATE 5
#define LPVMPC_DIST_STREAM 0xD157A2B3C4D5E6F7ull   /* keeps the gusts' draws apart from the sensors' under one seed */
typedef struct lpvmpc_disturbance_config {
    uint64_t seed;             /* 0 */
    int64_t  vehicle_offset;   /* 0: global index of vehicle 0 of this fleet (shards of one fleet draw the same numbers) */
    double   n_bound;          /* 3.0: the gusts' clip, in standard deviations */
} lpvmpc_disturbance_config;
void lpvmpc_disturbance_default_config(lpvmpc_disturbance_config *cfg);
int  lpvmpc_set_disturbances(lpvmpc_handle *h, int32_t B, const lpvmpc_disturbance_config *cfg, const double *rows);
int  lpvmpc_disturbances_read(lpvmpc_handle *h, double *rows, double *state);
int  lpvmpc_plant_step_disturbed_batch(lpvmpc_handle *h, int32_t B, double *state, double *act_state, const double *u,
                                       int32_t n_sub, double dt_sim, double mu_sim, const lpvmpc_actuator_config *act,
                                       const int32_t *delay_a, const int32_t *delay_df, const double *plant_params,
                                       const double *tyre_params, const lpvmpc_disturbance_config *cfg, const double *rows,
                                       double *dist_state);

/* ---------------------------------------------------------------------------------------------------------------
 * Tyre wear and temperature: a tyre-set state per vehicle of a lap-0 fleet or a race -- wear W, temperature T and the sliding energy E
 * that drives both -- and the grip factor g it gives.  The reference's simulator has none: this is the engine's own definition.  The
 * model acts at the control tick, on every tick on which a vehicle's plant advances n > 0 simulator steps, behind the disturbances'
 * kernel (where one is attached; the interactions', the contact model's and the walls' too) and immediately before that tick's
 * command / plant kernel (one more launch per tick; with nothing attached a tick issues the launches it always did).  Inputs per
 * vehicle: the ground-truth plant state st = [x y vx vy ax ay yaw psiDot] as the tick's plant steps will start from it; lr and m of
 * the vehicle's BASE plant row; D = n * dt_sim; the vehicle's row and state.  In this order and with exactly this association, every
 * product and sum rounded on its own, min(a, b) = a < b ? a : b and max(a, b) = a > b ? a : b:
 *      v_s = |vx| > 0.2 ? fabs(-vy + lr * psiDot) : 0       the numerator of the plant's rear slip angle, behind the plant's own gate
 *      F   = m * fabs(ay)                                   st[5]: the last simulator step's total lateral tyre force
 *      P   = F * v_s
 *      E   = E + P * D
 *      h   = max(0, T - T_opt)
 *      W   = min(1, W + ((k_wear * P) * D) * (1 + k_hot * h))      on the old T
 *      T   = T + D * (k_heat * P - k_cool * (T - T_amb))
 *      d   = T - T_opt                                             the new T
 *      gT  = 1 - (k_temp * d) * d
 *      gW  = (1 - wear_slope * W) - cliff_slope * max(0, W - cliff_at)
 *      g   = min(1, max(g_min, gW * gT))
 *      live Cf, Cr (plant words 4, 5), c_f (tyre word 3) = g * (gamma * base)
 *      j  += 1
 * gamma is the disturbances' value of this tick where they are attached; otherwise the factor is absent and live = g * base.  g == 1
 * leaves gamma * base bit for bit.  Frozen vehicles (finished, lost, n == 0) are not touched and their j stays put, so a vehicle's
 * state depends on its own history only: not on B, the other vehicles or how a fleet is sharded.  The model uses + - * fabs and
 * selects alone and the kernel is compiled without contraction: the device words equal a float64 restatement bit for bit.
 *
 * Host layouts: rows [B][LPVMPC_WEAR_WORDS] = {k_wear, k_hot, k_heat, k_cool, T_amb, T_opt, k_temp, wear_slope, cliff_at, cliff_slope,
 * g_min, T_start}; state [B][LPVMPC_WEAR_STATE] = {W, T, P of the last worn tick, g (1 before the first), ticks (= j), E}.  An
 * all-off row (every k_ and slope 0) gives g == 1 and T == T_start for ever and changes no word of plant or tables.
 *
 * lpvmpc_set_tyre_wear attaches rows to the lap-0 fleet or race that h runs (the path handle, for a race), from the next tick on; the
 * state starts at {0, T_start, 0, 1, 0, 0}.  The fleet or race must have plant and tyre tables (lpvmpc_cl_init_tyres /
 * lpvmpc_race_init_tyres).  Attaching again replaces the binding and the state starts over.  rows == NULL detaches: the live words go
 * back to gamma * base where disturbances are attached (their gamma of the last disturbed tick), else to base, and the state is
 * freed.  lpvmpc_cl_release frees the binding; a new fleet starts unworn.  While a binding is attached lpvmpc_plant_params_read and
 * lpvmpc_tyre_params_read return the base rows.  Disturbances and wear may be attached and detached in any order: both rewrite the
 * live words from the base copy on every tick that steps the vehicle, and no product is stored.  Refused with LPVMPC_E_ARG, a running
 * fleet left exactly as it is: no fleet or race on the handle or one without the tables, another B than the fleet's, a non-finite
 * word, any of k_wear, k_hot, k_heat, k_cool, k_temp, wear_slope, cliff_slope negative, cliff_at outside [0, 1], g_min outside
 * (0, 1], k_cool * n_max * dt_sim >= 1 (the Euler step's bound; n_max: the engine's largest steps per tick, of a race the largest of
 * n_sub_lap0 and n_sub[]).  lpvmpc_cascade_init is not extended.
 *
 * lpvmpc_tyre_wear_read: the rows and the state (synchronises); either pointer may be NULL.  The rows are those set, or after a
 * race's restore or clone those that travelled with the vehicle.
 *
 * lpvmpc_tyre_wear_fit: a tyre change between ticks.  The vehicles with mask[b] != 0 (mask [B]) get {0, T_start, 0, 1, j kept, E
 * kept}; the others are untouched.  Refused without a binding.  Synchronises.
 *
 * lpvmpc_plant_step_worn_batch: lpvmpc_plant_step_disturbed_batch with the wear model behind the disturbances' (rows NULL: no
 * disturbance model, dist_state is not touched) and in front of the n_sub steps; wear_state [B][LPVMPC_WEAR_STATE] is read and
 * written (NULL: fresh, nothing returned; refused: a non-finite word, a tick count that is not an integer >= 0), n_max = n_sub. */
#define LPVMPC_WEAR_WORDS 12
#define LPVMPC_WEAR_STATE 6
int  lpvmpc_set_tyre_wear(lpvmpc_handle *h, int32_t B, const double *rows);
int  lpvmpc_tyre_wear_read(lpvmpc_handle *h, double *rows, double *state);
int  lpvmpc_tyre_wear_fit(lpvmpc_handle *h, const int32_t *mask /* [B] */);
int  lpvmpc_plant_step_worn_batch(lpvmpc_handle *h, int32_t B, double *state, double *act_state, const double *u, int32_t n_sub,
                                  double dt_sim, double mu_sim, const lpvmpc_actuator_config *act, const int32_t *delay_a,
                                  const int32_t *delay_df, const double *plant_params, const double *tyre_params,
                                  const lpvmpc_disturbance_config *cfg, const double *rows, double *dist_state,
                                  const double *wear_rows, double *wear_state);

/* ---------------------------------------------------------------------------------------------------------------
 * Race snapshot, restore and clone: checkpoint a running race, continue it later (in the same race, or in a freshly initialised
 * one of the same shape, even in another process), and branch it: vehicles take the whole dynamic state of other vehicles.  All
 * calls take the race's path handle and fail with LPVMPC_E_ARG ("call lpvmpc_race_init first") on a handle without a race.  None of
 * them is on the path of a tick: a race that calls none of them issues the launches it always did.
 *
 * State and bindings.  The three calls act on the race's per-vehicle STATE: every device array of which a tick can read a word that an
 * earlier tick, or the init, wrote -- plant, command, measurement, phase and lap bookkeeping, this tick's masks, the planner message
 * and recursion, the carried rows of the three handles' workspaces (u_old, uPred, vel, curv, xPred, iters, status, polish), and
 * where present the estimate view and estimator state, the actuator's ring / servo / step counter, the disturbances' process
 * state and the tyre sets -- plus the host's tick counter.  A tyre set ("Tyre wear and temperature") travels whole: the wear's
 * state AND its rows are state here, the one binding that moves with the vehicle, because a worn set means nothing on another
 * set's coefficients.  Restored or cloned wear rows are copied as they are: they were checked when they were set, and the Euler
 * bound k_cool * n_max * dt_sim < 1 is NOT checked again against the receiving race, so restore a worn blob into a race of the
 * same dt_sim and step counts only.  All other BINDINGS are the caller's business and are never touched: plant, tyre, model,
 * tuning, track, estimator-gain and disturbance rows, actuator delays, the planner's max_ey, the hand-off operators, the live
 * Cf / Cr / c_f words (the disturbance kernel and the tyre wear kernel rewrite them from the base rows on every tick that steps
 * the vehicle), the seeds.  Apart from the tyre sets a blob carries state only: to continue a race elsewhere, initialise one with
 * the same bindings first (wear attached, with any rows, if the blob has it), then restore.  The recorder's ring and statistics
 * are neither.
 *
 * Blob format, version 1.  Little-endian, no pointers, self-describing:
 *   header     LPVMPC_SNAP_HEADER_BYTES = 64 B: char magic[8] = "LPVRACE\0"; then int32 words: version; B, N, Np, M (samples of the
 *              planner message), sd (steeringDelay), lap_cols (= laps + 2), laps, ticks; features (LPVMPC_SNAP_HAS_*: one bit each for
 *              the estimator in the loop, actuator state present, disturbances attached, tracks bound, tyre wear attached); count
 *              (arrays); 3 words zero
 *   directory  count entries of LPVMPC_SNAP_ENTRY_BYTES = 40 B: char name[16] (NUL-padded, at most 15 characters); int32 type
 *              (LPVMPC_SNAP_F64 / _I32), W (words per vehicle), layout (LPVMPC_SNAP_VEHICLE_MAJOR [B][W] / _WORD_MAJOR [W][B]), zero;
 *              int64 offset of the array from the start of the blob
 *   arrays     each exactly as it lies on the device, B * W elements, each starting on a multiple of 8 B (zero padding)
 * lpvmpc_race_snapshot_size returns the blob's size for the race as it is now (attaching or detaching disturbances or tyre wear
 * changes it; a blob of a race without tyre wear is byte for byte what it was before the wear existed).
 *
 * lpvmpc_race_snapshot synchronises the path handle's stream and copies the state into buf (bytes >= the size).  It changes no
 * state and is allowed while a recorder is attached.
 *
 * lpvmpc_race_restore accepts a blob only if the live race matches it: magic and version; the shape words B, N, Np, M, sd, lap_cols,
 * laps; the feature word; the directory equal to the live table in count, names, types, W, layouts and offsets; bytes covering all of
 * it.  Otherwise LPVMPC_E_ARG, lpvmpc_last_error names the first mismatch, and the race is untouched.  On success the arrays are copied
 * to the device on the handle's stream, ticks is set to the blob's, and the call synchronises: the next lpvmpc_race_tick continues the
 * snapshotted race word for word, noise and gust draws included (their counters are state).
 *
 * lpvmpc_race_clone: vehicle b takes the whole state of vehicle src[b] (src [B]; src[b] == b: untouched) and keeps its own bindings.
 * src may hold duplicates, cycles and swaps: every read sees the state before the call (the words are staged in a buffer that lives
 * for the call, which synchronises before it returns).  moved (may be NULL) returns the number of b with src[b] != b.  The sensors'
 * and gusts' generators are keyed by (seed, vehicle slot, the vehicle's own counter), so a clone in another slot draws another stream
 * from the next tick on: importance splitting needs nothing more.  Refused with nothing changed: an index outside [0, B); on a
 * track-bound race, track_of[src[b]] != track_of[b] (a pose and a lap table mean nothing on another track).
 *
 * Recorder: restore and clone are refused while a recorder is attached (stop it with lpvmpc_race_record, capacity 0, and start it
 * again afterwards); its ring and per-lap statistics are not carried.  The same holds while heats ("Heats") or an event log ("Race
 * event log") are attached.  The lap-0 fleet (lpvmpc_cl_*) and the cascade have no snapshot. */
#define LPVMPC_SNAP_VERSION 1
#define LPVMPC_SNAP_HEADER_BYTES 64
#define LPVMPC_SNAP_ENTRY_BYTES 40
#define LPVMPC_SNAP_F64 0
#define LPVMPC_SNAP_I32 1
#define LPVMPC_SNAP_VEHICLE_MAJOR 0
#define LPVMPC_SNAP_WORD_MAJOR 1
#define LPVMPC_SNAP_HAS_ESTIMATOR 1u
#define LPVMPC_SNAP_HAS_ACTUATOR 2u
#define LPVMPC_SNAP_HAS_DISTURBANCES 4u
#define LPVMPC_SNAP_HAS_TRACKS 8u
#define LPVMPC_SNAP_HAS_TYRE_WEAR 16u
int  lpvmpc_race_snapshot_size(lpvmpc_handle *path, int64_t *bytes);
int  lpvmpc_race_snapshot(lpvmpc_handle *path, void *buf, int64_t bytes);
int  lpvmpc_race_restore(lpvmpc_handle *path, const void *buf, int64_t bytes);
int  lpvmpc_race_clone(lpvmpc_handle *path, const int32_t *src /* [B] */, int32_t *moved /* out, may be NULL */);

/* ---------------------------------------------------------------------------------------------------------------
 * Heats: standings, gaps, passes and contacts of the vehicles of a race that share a track, kept on the device.  A heat is a set of
 * vehicles of one race that are taken to be on one track together; each vehicle belongs to one heat or to none, a heat has at most
 * LPVMPC_HEAT_MAX members.  While heats are attached, lpvmpc_race_tick launches one more kernel per tick, after the command / plant
 * kernel (one workgroup per heat, the members staged in LDS); with none attached a tick issues the launches it always did.  Heats
 * only observe: no output of the race changes.  Everything below is per vehicle b of heat g, on tick t (the race's tick number
 * counted before the tick, as the recorder's).
 *
 * Track frame.  (s, ey, epsi, inside) = Map.getLocalPosition of the ground-truth plant (x, y, yaw) with the race's half_width /
 * slack (each track's own, with tracks bound): the recorder's LPVMPC_REC_TRACK function, sentinels included.
 * Located: inside == 1 and s finite.  A vehicle that is not located keeps the s and turns of the last tick on which it was; one
 * never located since the attach has progress NaN.
 * Turns and progress.  turns starts at turns0[b] (NULL: 0; -1 for a car gridded behind the line).  Between two located ticks
 * turns += 1 when s_now - s_last < -L / 2 and turns -= 1 when s_now - s_last > L / 2, L the length of the vehicle's track.
 * progress = (double)turns * L + s, product and sum each rounded (no fused multiply-add).  turns has nothing to do with the race's
 * lap counter: the lap events fire ahead of the line (CMAIN:254-272), turns counts crossings of s = 0 itself.
 * Class, from the race's phase: 0 finished (phase 2), 1 running and located at least once, 2 running and never located, 3 lost
 * (phase 3).
 * Order within a heat -- a total order, so positions are a permutation of 0 .. n-1: by class ascending; within class 0 by finish
 * tick ascending (the tick on which phase became 2 while heats were attached; -1, sorting first, for a vehicle that had finished
 * before the attach), then progress descending, then vehicle index ascending; within classes 1 and 3 by progress descending (a
 * lost vehicle keeps its last progress; NaN sorts last), then index; within class 2 by index.
 * position = the number of members ordered before b; ahead = the member one place in front (-1 for the leader);
 * gap_ahead = progress[ahead] - progress[b], gap_leader = progress[leader] - progress[b], one subtraction each, NaN when either
 * vehicle is outside class 1 or b leads.
 * Passes.  For an unordered pair (i, j) of members that are both class 1 on the previous tick and on this one: when i was ordered
 * behind j on the previous tick and is in front of j on this one, passes[i] += 1 and passed[j] += 1.  The first tick after the
 * attach counts nothing.
 * Line crossings, K = laps + 2.  When turns reaches turns0 + k + 1 for the first time, 0 <= k < K, line_tick[b][k] = t and
 * line_pos[b][k] = position of that tick; untouched entries are -1.
 * Footprint and clearance.  A footprint is the rectangle centred at (x, y) with heading yaw and half extents half_length /
 * half_width_car (defaults 0.4 / 0.2, the reference's drawn car, plotCarTrajectory.py:115,161-166).  For a pair, sep is the largest
 * of the four separating-axis gaps |d . a| - (r_own(a) + r_other(a)) over the two axes a of each rectangle: d the difference of the
 * centres, r_own the rectangle's own half extent along its axis, r_other the other rectangle's projected half extent,
 * half_length |u . a| + half_width_car |v . a| with u / v its axes.  The rectangles overlap exactly when sep < 0.  Both vehicles
 * evaluate sep with the lower index as the first rectangle, so it is the same word on both sides.  Only pairs of vehicles that are
 * both class 1 or 2 with a finite pose take part (finished and lost cars have left the track).  Per tick: clearance = the smallest
 * sep over the vehicle's partners (+inf without one), nearest = that partner (lowest index on a tie, -1 without one), contact =
 * clearance < 0.  Since the attach: min_clearance, contact_ticks, first_contact_tick (-1: none).
 *
 * lpvmpc_race_heats attaches heats from the next tick: heat [B], the heat of each vehicle, -1 for none (indices need not be dense,
 * empty heats are allowed); turns0 [B] or NULL.  It frees a previous attachment first; heat == NULL detaches.  The member lists are
 * built on the host and the attachment is installed only when it is whole.  Refused with LPVMPC_E_ARG: no race on the handle, a heat
 * index below -1, a heat of more than LPVMPC_HEAT_MAX members, extents that are not finite and positive, and, with tracks bound, a
 * heat whose members are on different palette entries; a refused argument leaves a previous attachment as it was.  A failed
 * allocation or copy (LPVMPC_E_NOMEM, LPVMPC_E_HIP) comes after the previous attachment was freed and leaves the race without heats.
 * The attachment belongs to the race, as the recorder does:
 * lpvmpc_cl_release(path) or destroying a handle frees it, a new race starts without heats.  lpvmpc_race_snapshot works with heats
 * attached and does not contain them; lpvmpc_race_restore and lpvmpc_race_clone are refused while heats are attached (detach with
 * lpvmpc_race_heats(path, cfg, NULL, NULL)): a position history means nothing after a restore.
 *
 * lpvmpc_race_standings synchronises and copies (any pointer may be NULL) two planes, channel-major and vehicle-minor as the
 * recorder's, f64 [LPVMPC_HEAT_F64][B] and i32 [LPVMPC_HEAT_I32][B], and line_tick / line_pos [B][laps + 2].  A vehicle in no heat
 * reads NaN in every f64 channel, -1 in position, ahead, nearest, first_contact_tick and class, 0 in contact, contact_ticks, passes,
 * passed and turns, -1 in its line tables; so does every vehicle before the first tick after the attach (a member's turns reads turns0).
 * Refused with LPVMPC_E_ARG while no heats are attached.
 *
 * lpvmpc_heat_step_batch is one tick of the same device function on caller-supplied data (as lpvmpc_plant_step_*_batch): heat [B]
 * with indices in [-1, n_heats), L [B] each vehicle's track length, pose [B][3] = x y yaw, s [B] / inside [B] the track frame,
 * phase [B].  The caller owns the state carried from tick to tick and passes it in and gets it back: carry_f64
 * [LPVMPC_HEAT_CARRY_F64][B] and carry_i32 [LPVMPC_HEAT_CARRY_I32][B], channel-major.  A carry with flag word 0 is the state "just
 * attached": its TURNS word is turns0, its PHASE word the phase before the attach (0: running), every other word is ignored and
 * written; so an all-zero carry is a fresh attachment with turns0 = 0.  CROSSINGS counts the lines crossed since the attach: on the
 * tick it becomes k + 1 the race writes line_tick[b][k] / line_pos[b][k].  Outputs f64 / i32 as lpvmpc_race_standings.  It needs a
 * handle (device and stream) that runs no fleet, cascade or race. */
#define LPVMPC_HEAT_MAX                 256
#define LPVMPC_HEAT_F64                   5
#define LPVMPC_HEAT_PROGRESS              0
#define LPVMPC_HEAT_GAP_AHEAD             1
#define LPVMPC_HEAT_GAP_LEADER            2
#define LPVMPC_HEAT_CLEARANCE             3
#define LPVMPC_HEAT_MIN_CLEARANCE         4
#define LPVMPC_HEAT_I32                  10
#define LPVMPC_HEAT_POSITION              0
#define LPVMPC_HEAT_AHEAD                 1
#define LPVMPC_HEAT_NEAREST               2
#define LPVMPC_HEAT_CONTACT               3
#define LPVMPC_HEAT_CONTACT_TICKS         4
#define LPVMPC_HEAT_FIRST_CONTACT_TICK    5
#define LPVMPC_HEAT_PASSES                6
#define LPVMPC_HEAT_PASSED                7
#define LPVMPC_HEAT_TURNS                 8
#define LPVMPC_HEAT_CLASS                 9
#define LPVMPC_HEAT_CARRY_F64             3
#define LPVMPC_HEAT_CARRY_S               0  /* s of the last located tick */
#define LPVMPC_HEAT_CARRY_PROGRESS        1  /* progress of the previous tick */
#define LPVMPC_HEAT_CARRY_MIN_CLEARANCE   2
#define LPVMPC_HEAT_CARRY_I32            10
#define LPVMPC_HEAT_CARRY_FLAGS           0  /* bit 0: a tick has run since the attach; bit 1: located at least once */
#define LPVMPC_HEAT_CARRY_TURNS           1
#define LPVMPC_HEAT_CARRY_TURNS0          2
#define LPVMPC_HEAT_CARRY_CROSSINGS       3
#define LPVMPC_HEAT_CARRY_PHASE           4  /* phase of the previous tick */
#define LPVMPC_HEAT_CARRY_FINISH_TICK     5
#define LPVMPC_HEAT_CARRY_CONTACT_TICKS   6
#define LPVMPC_HEAT_CARRY_FIRST_CONTACT   7
#define LPVMPC_HEAT_CARRY_PASSES          8
#define LPVMPC_HEAT_CARRY_PASSED          9
typedef struct lpvmpc_heats_config {
    double half_length;       /* half extents of a vehicle's footprint, along and across its heading */
    double half_width_car;
} lpvmpc_heats_config;
void lpvmpc_heats_default_config(lpvmpc_heats_config *cfg);
int  lpvmpc_race_heats(lpvmpc_handle *path, const lpvmpc_heats_config *cfg, const int32_t *heat /* [B], -1: none */,
                       const int32_t *turns0 /* [B] or NULL */);
int  lpvmpc_race_standings(lpvmpc_handle *path, double *f64, int32_t *i32, int32_t *line_tick, int32_t *line_pos);
int  lpvmpc_heat_step_batch(lpvmpc_handle *h, int32_t B, int32_t n_heats, const int32_t *heat, const double *L,
                            const lpvmpc_heats_config *cfg, int32_t t, const double *pose, const double *s, const int32_t *inside,
                            const int32_t *phase, double *carry_f64, int32_t *carry_i32, double *f64, int32_t *i32);

/* ---------------------------------------------------------------------------------------------------------------
 * Sensor faults: GPS loss and jumps, IMU bias and drift, a slipping or stuck encoder for the vehicles of a lap-0 fleet or a race with
 * the estimator in the loop.  The simulated sensors above are healthy: white noise, a GPS that publishes on its cadence, an encoder
 * that always delivers.  The model here is stateless and keyed on the vehicle's own observer step k (the step counter after its
 * increment: the first step is k = 1) and its global index vid = vehicle_offset + b.  One row per vehicle:
 *   rows [B][LPVMPC_FAULT_WORDS] = {gps_out_k0, gps_out_len, gps_loss_z, gps_jump_k0, gps_jump_len, gps_jump_dx, gps_jump_dy,
 *                                   imu_w_bias, imu_yaw_drift, enc_scale, enc_out_k0, enc_out_len}
 * A window (k0, len) contains k when k0 <= k < k0 + len; len = 0: never.  With noise_c the sensors' draw of channel c on step k
 * (channel = std order: psi, psiDot, x, y, v), st the plant state just advanced and dt = 1 / loop_rate, the sensor stage of one
 * observer sub-step becomes, in this order (everything not named is the healthy stage, word for word):
 *   1. IMU:      imu_yaw = st[6] + noise_0 + imu_yaw_drift * (k * dt);  imu_w = st[7] + noise_1 + imu_w_bias.
 *   2. GPS:      gx = st[0] + noise_2, inside the jump window gx = (st[0] + noise_2) + gps_jump_dx; gy likewise with noise_3 and
 *                gps_jump_dy.  pub and the publish counter follow the healthy cadence rule unchanged (the beacon keeps its rhythm).  A
 *                publication is LOST when k is inside the outage window, or when gps_loss_z < 9 and
 *                gauss(seed ^ LPVMPC_FAULT_STREAM, vid, k, 5) > gps_loss_z on the estimator's counter-based generator (channel 5;
 *                drawn only on steps with pub).  The held reading is updated only when pub && !lost.  z >= 9 draws nothing: the
 *                generator cannot exceed sqrt(-2 ln 2^-53) = 8.57.  (A loss probability p is z = the standard normal's inverse CDF
 *                at 1 - p; the Python helper converts.)
 *   3. Encoder:  v = enc_scale * (|v_xy| + noise_4); inside the encoder window the delivered value is the previous one (the
 *                stored previous reading), a stuck reading: it counts as unchanged, so the healthy rule "more than 40 unchanged readings
 *                in a row read 0" fires by itself on the 41st stuck step, and the first step after the window reads v again.
 *   4. The start-up branch (k dt <= 0.02) and the observer step are untouched.
 * An all-off row (every len = 0, gps_loss_z >= 9, dx = dy = 0, bias = drift = 0, enc_scale = 1) changes no word of any output.
 *
 * lpvmpc_set_sensor_faults attaches rows to the lap-0 fleet or race that h runs (the path handle, for a race), from the next tick
 * on; cfg NULL: the defaults.  Attaching again replaces the binding; rows == NULL detaches; lpvmpc_cl_release (and the end of the
 * race) frees it.  With nothing attached a tick issues exactly the launches it always did; with a binding attached the tick launches
 * the faulted kernel IN PLACE of its fused command / plant / observe kernel: no extra launch.  Refused with LPVMPC_E_ARG, the running
 * fleet left exactly as it was: a non-finite word; k0 or len not integer-valued, negative or >= 2^31; enc_scale <= 0; another B than
 * the fleet's; no fleet or race on the handle; one without an estimator; one without plant and tyre tables (only the
 * lpvmpc_cl_init_tyres / lpvmpc_race_init_tyres starts are served: one general kernel form); a lap-0 fleet with a track binding (a
 * race with tracks is served: its fused kernel reads no track).  lpvmpc_cascade_init is not extended.
 * The rows are a binding, not state: the race's snapshot blob and its version do not change, and snapshot, restore and clone work
 * while faults are attached.  A clone keeps its slot's own row and, keyed on vid, draws its own losses.
 * lpvmpc_sensor_faults_read: the rows as they were set ([B][LPVMPC_FAULT_WORDS]); *B returns the binding's size, 0 with none
 * attached (rows is then untouched); either pointer may be NULL.
 *
 * lpvmpc_sensor_step_batch: ONE sensors + observer sub-step for B vehicles on caller arrays, as the fused kernels run it once per
 * plant step: obs_state [B][LPVMPC_OBS_STATE_WORDS] is read and written -- the estimator's whole per-vehicle state {estimate [6],
 * last measurement y [5], held GPS x, y, previous encoder reading, encoder measurement, GPS publish counter, unchanged-encoder
 * counter, step counter k} -- plant [B][8] is the plant state just advanced, servo [B] / motor [B] the commanded input.  rows ==
 * NULL: the healthy stage.  obs is the estimator configuration (gains, limits, noise, seed, vehicle_offset), dt_sim the simulator
 * step that sets the GPS cadence (thUpdate = (1 / gps_freq) / dt_sim).  A handle with per-vehicle estimator rows bound
 * (lpvmpc_set_observer_vehicles) runs the bound form (B must be the binding's).  Refused: the row rules above, a counter word that is
 * not an integer >= 0, and a handle that runs a fleet, cascade or race. */
#define LPVMPC_FAULT_WORDS 12
#define LPVMPC_OBS_STATE_WORDS 18
#define LPVMPC_FAULT_STREAM 0x5E4507FA17C0FFEEull   /* keeps the loss draws apart from the sensors' and the gusts' under one seed */
typedef struct lpvmpc_sensor_fault_config {
    uint64_t seed;             /* 0 */
    int64_t  vehicle_offset;   /* 0: global index of vehicle 0 of this fleet (shards of one fleet draw the same losses) */
} lpvmpc_sensor_fault_config;
void lpvmpc_sensor_fault_default_config(lpvmpc_sensor_fault_config *cfg);
int  lpvmpc_set_sensor_faults(lpvmpc_handle *h, int32_t B, const lpvmpc_sensor_fault_config *cfg, const double *rows);
int  lpvmpc_sensor_faults_read(lpvmpc_handle *h, int32_t *B, double *rows);
int  lpvmpc_sensor_step_batch(lpvmpc_handle *h, int32_t B, const lpvmpc_observer_config *obs, double dt_sim,
                              const lpvmpc_sensor_fault_config *cfg, const double *rows, double *obs_state, const double *plant,
                              const double *servo, const double *motor);

/* ---------------------------------------------------------------------------------------------------------------
 * Interactions: slipstream and contact response between the vehicles of a heat.  Heats observe; interactions let the members of a heat
 * act on each other's PLANTS: a car in another's wake has less drag, and overlapping footprints exchange an impulse and are pushed
 * apart.  Plant side only: one more kernel in front of the tick's command / plant kernel, behind the disturbances' (a kick comes
 * before a contact of the same tick); no controller, planner or estimator knows about an opponent.  The reference's simulator drives
 * one car, so nothing here has a counterpart in it: this text is the definition, and the defaults are invented values of the right
 * order for a 1:10 car.  The contact is frictionless and acts through the centres: it changes the velocity along the contact normal
 * and the position, never yaw, psiDot, ax or ay.
 *
 * Participants.  A vehicle takes part on a tick when it is a member of an attached heat, its plant advances this tick (nstep[b] > 0,
 * the disturbances' rule: a frozen vehicle is neither touched nor seen) and its x, y, yaw, vx, vy are finite.  Everything below is
 * per heat, over its participants, in member (= ascending vehicle index) order.
 * Staged per participant, before anything is written: x, y; c = cos(yaw), s = sin(yaw); the world velocity ux = c*vx - s*vy,
 * uy = s*vx + c*vy; m (plant row word 2) and the base mu (plant row word 6).  Every product and sum here and below is rounded on its
 * own (no fused multiply-add), in the order written, a unary minus applying to the factor it stands in front of.
 *
 * Slipstream of vehicle i, over every other participant j:
 *   dx = x_i - x_j, dy = y_i - y_j;  lon = -(dx*c_j + dy*s_j), the distance behind j's centre along j's heading;
 *   lat = -dx*s_j + dy*c_j;  align = c_i*c_j + s_i*s_j.
 *   i is in j's wake when 0 < lon < wake_length, |lat| < wake_half_width and align > 0; then
 *   w_ij = (1 - lon/wake_length) * (1 - |lat|/wake_half_width), else w_ij = 0.
 *   w_i = max_j w_ij (the shelter); leader_i = the lowest j attaining the max, -1 when w_i == 0.
 * The live plant table's drag word of vehicle i becomes mu_i * (1 - draft_gain * w_i), mu_i the base word; it is rewritten on every
 * tick on which the vehicle takes part, as the grip patches rewrite Cf, Cr, c_f.  A max does not depend on the order of evaluation:
 * no atomics, and reruns are bit-identical.
 *
 * Contact (contact != 0), for every unordered pair a < b of participants whose footprints overlap: sep < 0 by the heats' own
 * definition ("Heats", footprint and clearance), with the heats' configured half extents and a, the lower index, as the first
 * rectangle, so both sides hold the same word.  With d = centre_b - centre_a, the projections p0 = d . u_a, p1 = d . v_a,
 * p2 = d . u_b, p3 = d . v_b on the axes u = (c, s), v = (-s, c) of each rectangle (p1 = dy*c_a - dx*s_a, p3 likewise) and the four gaps
 * g_k = |p_k| - r_k of that definition:
 *   the contact axis is the first of (u_a, v_a, u_b, v_b) whose gap attains the max, sep = that gap;
 *   n = axis * sign(p_k), sign(0) = +1: the normal, from a to b;
 *   vn = (u_b - u_a) . n;   J = vn < 0 ? -(1 + restitution) * vn / (1/m_a + 1/m_b) : 0   (a separating pair gets no impulse);
 *   du_a = -(J/m_a) n,  du_b = +(J/m_b) n;
 *   depth = -sep;  dc_a = -push * depth * (m_b/(m_a + m_b)) n,  dc_b = +push * depth * (m_a/(m_a + m_b)) n.
 * Each vehicle sums the du and dc of its own contacts over its partners in ascending order, starting from 0; all of them come from
 * the staged (pre-tick) words, a Jacobi step: the result does not depend on which pair is handled first.
 * A vehicle WITHOUT an overlapping partner keeps every state word as it is (no round trip through the world frame).  One with an
 * overlapping partner or more writes u' = u + sum du, vx = max(c*u'_x + s*u'_y, 0), vy = -s*u'_x + c*u'_y, x += sum dc_x,
 * y += sum dc_y.
 *
 * Outputs per vehicle, channel-major and vehicle-minor as the standings: f64 [LPVMPC_INTER_F64][B] = SHELTER (w_i), MU (the live word
 * written), IMPULSE (the sum of |J| over its contacts of this tick), IMPULSE_TOTAL (since the attach); i32 [LPVMPC_INTER_I32][B] =
 * LEADER (vehicle index), HIT (0 / 1 this tick), HIT_TICKS, FIRST_HIT_TICK (-1: none), DRAFT_TICKS (ticks with w_i > 0).  The three
 * counters and the total are carried.  A member that does not take part on a tick reads SHELTER 0, IMPULSE 0, LEADER -1, HIT 0; its
 * carried words and its MU word stay put (before its first tick MU reads the base word).  A vehicle in no heat reads NaN in every f64
 * channel, -1 in LEADER and FIRST_HIT_TICK, 0 in HIT, HIT_TICKS and DRAFT_TICKS, as in lpvmpc_race_standings.
 *
 * Configuration (lpvmpc_interaction_default_config: draft_gain 0.3, wake_length 3.0 m, wake_half_width 0.3 m, contact 1,
 * restitution 0.2, push 0.5): draft_gain in [0, 1] (0: no slipstream), wake_length > 0, wake_half_width > 0, contact 0 / 1,
 * restitution in [0, 1], push in [0, 1].  With draft_gain = 0 and contact = 0 no word of any plant changes and the live mu word is the
 * base word.
 *
 * lpvmpc_race_interactions attaches the interactions to the race of the path handle from the next tick on; attaching again replaces
 * the binding (counters start anew), cfg == NULL detaches.  It needs a race with heats attached (it reads their member lists and
 * extents) and a plant table (the lpvmpc_race_init_vehicles / _tyres starts).  Refused with LPVMPC_E_ARG, the race left as it was: no
 * race on the handle, no heats, no plant table, a config word that is not finite or outside its range.  The binding is built whole
 * and then installed; the race owns it next to the heats and frees it with them.  lpvmpc_race_heats, whether it re-attaches or
 * detaches, detaches the interactions first.  A detach writes the base mu words back to the live plant table.  While attached
 * lpvmpc_race_tick issues one more launch, behind the disturbances' and in front of the command / plant kernel; with nothing attached
 * a tick issues exactly the launches it always did.  lpvmpc_plant_params_read returns the caller's rows (the base mu) while attached,
 * as it does for the disturbances' words; disturbances and interactions may be attached and detached in either order: each keeps the
 * caller's words as its base, and with both detached the live tables are word for word what the race started with.
 * lpvmpc_race_snapshot works while attached and does not contain the binding (the live mu word is a table word, the counters belong
 * to the binding); restore and clone are refused while heats are attached.
 * lpvmpc_race_interactions_read synchronises and copies the two output planes (either pointer may be NULL); refused with LPVMPC_E_ARG
 * while nothing is attached.
 *
 * lpvmpc_interaction_step_batch is one tick of the same kernel on caller-supplied data: heat [B] with indices in [-1, n_heats) and the
 * heats' extents heats_cfg, plant [B][8] in / out, plant_params [B][LPVMPC_PLANT_WORDS] (words 2 and 6 are read), nstep [B] or NULL
 * (every vehicle steps), the carried state carry_f64 [LPVMPC_INTER_CARRY_F64][B] / carry_i32 [LPVMPC_INTER_CARRY_I32][B] in / out (just
 * attached: zeros, FIRST_HIT_TICK -1), mu_live [B] out (the base word for a vehicle that does not take part) and the output planes.  It
 * needs a handle (device and stream) that runs no fleet, cascade or race. */
#define LPVMPC_INTER_F64                  4
#define LPVMPC_INTER_SHELTER              0
#define LPVMPC_INTER_MU                   1
#define LPVMPC_INTER_IMPULSE              2
#define LPVMPC_INTER_IMPULSE_TOTAL        3
#define LPVMPC_INTER_I32                  5
#define LPVMPC_INTER_LEADER               0
#define LPVMPC_INTER_HIT                  1
#define LPVMPC_INTER_HIT_TICKS            2
#define LPVMPC_INTER_FIRST_HIT_TICK       3
#define LPVMPC_INTER_DRAFT_TICKS          4
#define LPVMPC_INTER_CARRY_F64            1
#define LPVMPC_INTER_CARRY_IMPULSE_TOTAL  0
#define LPVMPC_INTER_CARRY_I32            3
#define LPVMPC_INTER_CARRY_HIT_TICKS      0
#define LPVMPC_INTER_CARRY_FIRST_HIT_TICK 1
#define LPVMPC_INTER_CARRY_DRAFT_TICKS    2
typedef struct lpvmpc_interaction_config {
    double  draft_gain;        /* [0, 1]: the share of the drag word a full shelter takes away; 0: no slipstream */
    double  wake_length;       /* > 0, metres behind the leader's centre */
    double  wake_half_width;   /* > 0, metres to either side of the leader's axis */
    int32_t contact;           /* 0 / 1 */
    int32_t reserved;          /* 0 */
    double  restitution;       /* [0, 1] */
    double  push;              /* [0, 1]: the share of the overlap depth removed per tick */
} lpvmpc_interaction_config;
void lpvmpc_interaction_default_config(lpvmpc_interaction_config *cfg);
int  lpvmpc_race_interactions(lpvmpc_handle *path, const lpvmpc_interaction_config *cfg /* NULL: detach */);
int  lpvmpc_race_interactions_read(lpvmpc_handle *path, double *f64, int32_t *i32);
int  lpvmpc_interaction_step_batch(lpvmpc_handle *h, int32_t B, int32_t n_heats, const int32_t *heat,
                                   const lpvmpc_heats_config *heats_cfg, const lpvmpc_interaction_config *cfg, int32_t t,
                                   double *plant /* [B][8] in/out */, const double *plant_params /* [B][7] */,
                                   const int32_t *nstep /* [B] or NULL: all step */, double *carry_f64, int32_t *carry_i32,
                                   double *mu_live /* [B] out */, double *f64, int32_t *i32);

/* ---------------------------------------------------------------------------------------------------------------
 * Walls: barrier contact at the track's edges.  The interactions let cars act on each other; the walls let the TRACK act on a car:
 * a corner of a footprint that passes the wall gets an impulse there and the car is pushed back, so a shoved or kicked car is turned
 * and stopped instead of leaving a world without edges.  Plant side only: one more kernel in front of the tick's command / plant
 * kernel, behind the disturbances' and the interactions' (a shove into a wall is answered on the same tick); no controller, planner or
 * estimator knows about a wall.  The reference simulates one car on an open plane, so nothing here has a counterpart in it: this text
 * is the definition, and the defaults are invented values of the right order for a 1:10 car.  Every product and sum below is rounded
 * on its own (no fused multiply-add), in the order written, a unary minus applying to the factor it stands in front of.
 *
 * Participants.  A vehicle takes part on a tick when its plant advances this tick (nstep[b] > 0: a frozen vehicle is neither touched
 * nor counted) and its x, y, yaw, vx, vy, psiDot are finite.  Heats play no part: a race without heats can have walls.
 *
 * Geometry.  The wall stands at |ey| = wall_ey = half_width + margin, half_width the race's, or the vehicle's track's when tracks are
 * bound (lpvmpc_set_tracks).  The footprint is the rectangle half_length x half_width_car of this configuration around (x, y), turned
 * by yaw; with c = cos(yaw), s = sin(yaw) its corners k = 0 .. 3 are taken in the order
 *   (a, b) = (+half_length, +half_width_car), (+half_length, -half_width_car), (-half_length, +half_width_car),
 *            (-half_length, -half_width_car):   r_k = (c*a - s*b, s*a + c*b),   corner_k = (x + r_kx, y + r_ky).
 * A point p is located by a search over ALL rows i of the track table (PointAndTangent; ip the row before, the last for i = 0;
 * S = (x, y) of row ip, F = (x, y) of row i, cv = word 5 of row i).  A row is Map.getLocalPosition's arithmetic for that row
 * (lpvmpc_local_position_batch; computeAngle(a, o, b) = atan2 of the cross and dot products of a - o and b - o, |.| the norm
 * sqrt(dx*dx + dy*dy)), giving (ey, th) where that function gives (s, ey, epsi); s and epsi are not computed:
 *   cv == 0 (straight): |S - p| == 0 or |F - p| == 0: ey = 0.  Else, when |computeAngle(p, S, F)| <= pi/2 and
 *     |computeAngle(p, F, S)| <= pi/2: ey = |p - S| * sin(computeAngle(F, S, p)); else the row does not see p.  th = word 2 of row ip.
 *   cv != 0 (arc): r = 1/cv, d = r >= 0 ? 1 : -1, ang = word 2 of row ip, C = S + |r| * (cos(ang + d*pi/2), sin(ang + d*pi/2)).
 *     |S - p| == 0: ey = 0, th = ang.  |F - p| == 0: ey = 0, th = word 2 of row i.  Else arc1 = word 4 * word 5 of row i,
 *     arc2 = computeAngle(S, C, p): when sign(arc1) == sign(arc2) and |arc1| >= |arc2|: ey = -d * (|p - C| - |r|), th = ang + arc2;
 *     else the row does not see p.
 *   A row that sees p accepts it when |ey| <= wall_ey + reach (the function's own bound is half_width + slack).
 * Among the rows that accept p the one with the smallest |ey| wins, the first of them on a tie: the wall is the nearest stretch of
 * track, not whichever row comes first where two stretches run close.  A point that no row accepts is not located.
 * A corner that is not located is not in contact on that tick.  A located corner penetrates when |ey_k| > wall_ey, with
 * depth_k = |ey_k| - wall_ey.  The contact corner is the first corner that attains the largest depth: at most one contact per vehicle
 * and tick.  With side = ey_k > 0 ? +1 : -1 and th of the winning row, the inward normal is n = (side * sin(th), -(side * cos(th)))
 * (= -side * (-sin th, cos th)) and the tangent t = (-n_y, n_x).
 *
 * Response at the contact corner.  Staged before anything is written: c, s; the world velocity u_x = c*vx - s*vy, u_y = s*vx + c*vy;
 * w = psiDot; m and Iz (plant row words 2 and 3); r = r_k.  With yaw_response == 0, r is taken as (0, 0) in everything below and psiDot
 * is never written: the interactions' "through the centres" form.
 *   Normal impulse:  v_c = (u_x + w * -r_y, u_y + w * r_x);  vn = v_cx*n_x + v_cy*n_y;  rn = r_x*n_y - r_y*n_x;
 *     kn = 1/m + (rn*rn)/Iz;  Jn = vn < 0 ? (-(1 + restitution) * vn) / kn : 0.
 *     u' = (u_x + (Jn/m)*n_x, u_y + (Jn/m)*n_y);  w' = w + (rn*Jn)/Iz.
 *   Friction impulse, from the velocity after the normal impulse:  v_c' = (u'_x + w' * -r_y, u'_y + w' * r_x);
 *     vt = v_c'x*t_x + v_c'y*t_y;  rt = r_x*t_y - r_y*t_x;  kt = 1/m + (rt*rt)/Iz;  lim = friction * Jn;
 *     Jt = -vt / kt, then lim where Jt > lim, then -lim where Jt < -lim.
 *     u'' = (u'_x + (Jt/m)*t_x, u'_y + (Jt/m)*t_y);  w'' = w' + (rt*Jt)/Iz.
 * One pass, normal then friction.  Each step moves along its own impulse towards that direction's energy minimum and never beyond
 * it, so the pair cannot add kinetic energy; a decoupled one-shot friction formula could.
 * Written for a vehicle with a penetrating corner:  vx = max(c*u''_x + s*u''_y, 0) (the plant's vx is never negative),
 * vy = -s*u''_x + c*u''_y,  psiDot = w'' when yaw_response != 0,  x += (push*depth)*n_x,  y += (push*depth)*n_y.  A penetrating but
 * separating corner (vn >= 0) gets the push and no impulse (Jn = Jt = 0).  yaw, ax, ay are never written.  A vehicle without a
 * penetrating corner keeps every state word bit for bit.
 *
 * Outputs per vehicle, channel-major and vehicle-minor as the standings: f64 [LPVMPC_WALL_F64][B] = DEPTH (of the contact corner, 0
 * without one), IMPULSE (|Jn| of this tick), IMPULSE_TOTAL, MAX_IMPULSE (since the attach); i32 [LPVMPC_WALL_I32][B] = HIT (0 / 1: a
 * penetrating corner this tick), SIDE (+1 / -1, 0 without a hit), CORNER (0 .. 3, -1: none), HIT_TICKS, FIRST_HIT_TICK (-1: none),
 * OUTSIDE (1: the vehicle takes part and no row accepts its centre (x, y) within wall_ey + reach).  IMPULSE_TOTAL, MAX_IMPULSE,
 * HIT_TICKS and FIRST_HIT_TICK are carried.  A vehicle that does not take part on a tick reads 0 in DEPTH, IMPULSE, HIT, SIDE and
 * OUTSIDE and -1 in CORNER, and keeps its carried words.
 *
 * Configuration (lpvmpc_wall_default_config: margin 0.25, reach 0.5, half_length 0.4, half_width_car 0.2 (the heats' footprint),
 * restitution 0.2, friction 0.3, push 0.5, yaw_response 1; invented values of the right order): margin >= 0, reach > 0,
 * half_length > 0, half_width_car > 0, restitution in [0, 1], friction >= 0, push in [0, 1], yaw_response 0 / 1, reserved 0.  The
 * margin is the caller's trade: with the race's half_width 0.3 / slack 0.15 the default leaves the centre of a car that runs along
 * the wall at |ey| <= 0.35, inside what the controller's measurement locates; a larger margin lets a car slide to where
 * Map.getLocalPosition loses it before the wall stops it, a smaller one makes the walls touch cars that merely run wide.
 *
 * lpvmpc_race_walls attaches the walls to the race of the path handle from the next tick on; attaching again replaces the binding
 * (counters start anew), cfg == NULL detaches.  It needs a race with a plant table (the lpvmpc_race_init_vehicles / _tyres starts: m
 * and Iz).  Refused with LPVMPC_E_ARG, the race left as it was: no race on the handle, no plant table, a config word that is not finite
 * or outside its range, reserved != 0.  The binding is built whole and then installed; the race owns it and frees it.  Attach and
 * detach are independent of heats, interactions and disturbances, in any order.  While attached lpvmpc_race_tick issues one more
 * launch, behind the disturbances' and the interactions' and in front of the command / plant kernel; with nothing attached a tick
 * issues exactly the launches it always did.  lpvmpc_race_snapshot, _restore and _clone work while attached: the blob and its version
 * do not change, and the counters and outputs belong to the binding's slots (a restore or a clone leaves them as they are).
 * lpvmpc_race_walls_read synchronises and copies the two output planes (either pointer may be NULL); refused with LPVMPC_E_ARG while
 * nothing is attached.
 *
 * lpvmpc_wall_step_batch is one tick of the same kernel on caller-supplied data: plant [B][8] in / out, plant_params
 * [B][LPVMPC_PLANT_WORDS] (words 2 and 3 are read), nstep [B] or NULL (every vehicle steps), the carried state carry_f64
 * [LPVMPC_WALL_CARRY_F64][B] / carry_i32 [LPVMPC_WALL_CARRY_I32][B] in / out (just attached: zeros, FIRST_HIT_TICK -1) and the output
 * planes.  The track is the handle's own with half_width, or, when tracks are bound to the handle (B vehicles), each vehicle's palette
 * entry and its half width (half_width is then ignored).  It needs a handle that runs no fleet, cascade or race. */
#define LPVMPC_WALL_F64                  4
#define LPVMPC_WALL_DEPTH                0
#define LPVMPC_WALL_IMPULSE              1
#define LPVMPC_WALL_IMPULSE_TOTAL        2
#define LPVMPC_WALL_MAX_IMPULSE          3
#define LPVMPC_WALL_I32                  6
#define LPVMPC_WALL_HIT                  0
#define LPVMPC_WALL_SIDE                 1
#define LPVMPC_WALL_CORNER               2
#define LPVMPC_WALL_HIT_TICKS            3
#define LPVMPC_WALL_FIRST_HIT_TICK       4
#define LPVMPC_WALL_OUTSIDE              5
#define LPVMPC_WALL_CARRY_F64            2
#define LPVMPC_WALL_CARRY_IMPULSE_TOTAL  0
#define LPVMPC_WALL_CARRY_MAX_IMPULSE    1
#define LPVMPC_WALL_CARRY_I32            2
#define LPVMPC_WALL_CARRY_HIT_TICKS      0
#define LPVMPC_WALL_CARRY_FIRST_HIT_TICK 1
typedef struct lpvmpc_wall_config {
    double  margin;            /* >= 0, metres: the wall's offset beyond half_width */
    double  reach;             /* > 0, metres: how far beyond the wall a corner is still located */
    double  half_length;       /* > 0: footprint half length */
    double  half_width_car;    /* > 0: footprint half width */
    double  restitution;       /* [0, 1] */
    double  friction;          /* >= 0 */
    double  push;              /* [0, 1]: the share of the depth removed per tick */
    int32_t yaw_response;      /* 0 / 1: 0 applies the impulses through the centre and leaves psiDot alone */
    int32_t reserved;          /* 0 */
} lpvmpc_wall_config;
void lpvmpc_wall_default_config(lpvmpc_wall_config *cfg);
int  lpvmpc_race_walls(lpvmpc_handle *path, const lpvmpc_wall_config *cfg /* NULL: detach */);
int  lpvmpc_race_walls_read(lpvmpc_handle *path, double *f64, int32_t *i32);
int  lpvmpc_wall_step_batch(lpvmpc_handle *h, int32_t B, const lpvmpc_wall_config *cfg, double half_width, int32_t t,
                            double *plant /* [B][8] in/out */, const double *plant_params /* [B][7] */,
                            const int32_t *nstep /* [B] or NULL: all step */, double *carry_f64, int32_t *carry_i32, double *f64,
                            int32_t *i32);

/* ---------------------------------------------------------------------------------------------------------------
 * Contact model: the corner form of the car-to-car contact.  The interactions' contact is frictionless and acts through both centres;
 * the walls' acts at a corner, with friction, and turns the car.  The contact model gives a pair of cars the walls' response: one
 * contact point per overlapping pair, a normal and a clamped friction impulse there, and the yaw rates that follow from the lever
 * arms.  It is attached ON TOP of the interactions (contact = 1) and replaces their kernel's launch on the ticks on which it is
 * attached; slipstream, push, the interactions' configuration, planes and counters keep their meaning and are written by the same
 * launch.  Nothing here has a counterpart in the reference; this text is the definition.  Every product and sum below is rounded on
 * its own (no fused multiply-add), in the order written, a unary minus applying to the factor it stands in front of; a / 2 is exact.
 *
 * Participants.  The interactions' rule, and psiDot finite as well (the walls' rule).  Staged per participant before anything is
 * written, in addition to the interactions' words: w = psiDot and Iz (plant row word 3).
 * Decision.  For every unordered pair a < b of participants the overlap decision is the interactions' own, word for word: the four
 * projections p_k and gaps g_k, k the first axis of (u_a, v_a, u_b, v_b) attaining the max, sep = g_k, n = axis * sign(p_k) from a to b.
 * A pair with sep >= 0 is untouched.  The half extents hl (along u) and hw (along v) are the heats' footprint.
 *
 * Reference and incident body.  R owns the contact axis: a for k in {0, 1}, b for k in {2, 3}; I is the other one.  n_R = n when R = a,
 * else (-n_x, -n_y); t_R = (-n_Ry, n_Rx).  r_n = hl and r_t = hw for k in {0, 2} (a u axis), r_n = hw and r_t = hl for k in {1, 3}.
 * Incident face.  With (c, s) of I: d_0 = c*n_Rx + s*n_Ry (face +u_I), d_1 = -d_0 (-u_I), d_2 = -s*n_Rx + c*n_Ry (+v_I), d_3 = -d_2
 * (-v_I); the face is the first that attains the min.  Its end points are I's corners on it in the walls' corner order,
 *   (a_0, b_0), (a_1, b_1) = face 0: (+hl, +hw), (+hl, -hw);  1: (-hl, +hw), (-hl, -hw);  2: (+hl, +hw), (-hl, +hw);
 *   3: (+hl, -hw), (-hl, -hw);      E_j = (x_I + (c*a_j - s*b_j), y_I + (s*a_j + c*b_j)),
 *   q_j = (E_jx - x_R, E_jy - y_R);  tau_j = q_jx*t_Rx + q_jy*t_Ry;  delta_j = r_n - (q_jx*n_Rx + q_jy*n_Ry)   (depth below R's face).
 * Contact point.  The face is E_0 + s (E_1 - E_0), s in [0, 1]; tau and delta are linear in s.  dt = tau_1 - tau_0 (never 0 for the
 * chosen face);  s1 = (r_t - tau_0)/dt,  s2 = (-r_t - tau_0)/dt;  s_lo = max(0, min(s1, s2)),  s_hi = min(1, max(s1, s2)).
 * When delta_0 < 0 and delta_1 < 0 the interval is empty.  Else, when delta_0 < 0: s_lo = max(s_lo, -delta_0/(delta_1 - delta_0)); else,
 * when delta_1 < 0: s_hi = min(s_hi, -delta_0/(delta_1 - delta_0)).  The interval is empty as well when s_lo > s_hi.
 *   s* = (s_lo + s_hi)/2, or, of an empty interval, 0 when delta_0 >= delta_1 and 1 otherwise (no overlapping pair is known to
 *   reach this; the rule makes the text total);   P = (E_0x + s* * (E_1x - E_0x), E_0y + s* * (E_1y - E_0y)).
 * A flat nose-to-tail hit gets the middle of the shared width; a corner driven into a side gets a point next to the corner.
 * Between parallel cars two axes tie and the lower index owns the axis: with the labels swapped P moves by the depth along n, which
 * changes the friction's lever arms and nothing else.
 *
 * Response at P.  r_a = (P_x - x_a, P_y - y_a), r_b likewise; with yaw_response == 0 both are (0, 0) in everything below and psiDot is
 * never written: the interactions' through-the-centres form, with friction.  For a direction d (n, then t = (-n_y, n_x)) and the
 * velocities (u_a, w_a, u_b, w_b) of the pair:
 *   v_b = (u_bx + w_b * -r_by, u_by + w_b * r_bx),  v_a likewise;   vd = (v_bx - v_ax)*d_x + (v_by - v_ay)*d_y;
 *   ka = r_ax*d_y - r_ay*d_x,  kb = r_bx*d_y - r_by*d_x;   kd = ((1/m_a + 1/m_b) + (ka*ka)/Iz_a) + (kb*kb)/Iz_b.
 *   Normal impulse (d = n, the staged velocities):  Jn = vn < 0 ? (-(1 + restitution) * vn) / kn : 0, restitution the interactions'.
 *     u_a' = u_a - (Jn/m_a) n,  w_a' = w_a - (ka*Jn)/Iz_a;   u_b' = u_b + (Jn/m_b) n,  w_b' = w_b + (kb*Jn)/Iz_b.
 *   Friction impulse (d = t, the primed velocities):  lim = friction * Jn;  Jt = -vt / kt, then lim where Jt > lim, then -lim where
 *     Jt < -lim.  With ka, kb of d = t named la, lb:
 *   du_a = (-((Jn/m_a)*n_x) + -((Jt/m_a)*t_x), same in y),   dw_a = -((ka*Jn)/Iz_a) + -((la*Jt)/Iz_a);
 *   du_b = ((Jn/m_b)*n_x + (Jt/m_b)*t_x, same in y),         dw_b = (kb*Jn)/Iz_b + (lb*Jt)/Iz_b.
 * One pass, normal then friction, as the walls': neither step passes its direction's energy minimum, so an isolated pair on which
 * no vx clamp acts keeps its linear momentum and its angular momentum about the origin (sum m (c x u) + Iz w, at the positions before
 * the push) to rounding and never gains kinetic energy, rotation included.  NOTHING of that kind is claimed for a vehicle with
 * several partners on one tick: their contributions are summed from the same staged words (below), and the sum of two admissible
 * impulses can add energy.
 * Push.  The interactions' own: dc_a, dc_b of that section, unchanged.
 * Several partners.  du, dw, dc of every partner come from the staged (pre-tick) words and are summed in ascending partner order,
 * starting from 0: the interactions' Jacobi step.
 * Written for a vehicle with at least one overlapping partner: u' = u + sum du;  vx = max(c*u'_x + s*u'_y, 0),  vy = -s*u'_x + c*u'_y,
 * psiDot = w + sum dw when yaw_response != 0,  x += sum dc_x,  y += sum dc_y.  yaw, ax, ay are never written; a vehicle without an
 * overlapping partner keeps every state word bit for bit.  Slipstream: unchanged, computed by the same launch in the same words.
 * With friction = 0 and yaw_response = 0 every plant word and every plane of the interactions is the word the interactions alone
 * give (when every psiDot is finite).
 *
 * Outputs.  The interactions' planes as they are (IMPULSE sums |Jn|).  f64 [LPVMPC_CONTACT_F64][B] = FRICTION_IMPULSE (the sum of |Jt|
 * over its partners of this tick), YAW_KICK (sum dw of this tick), YAW_KICK_TOTAL (the sum of |dw| over every partner and tick since
 * the attach, carried); i32 [LPVMPC_CONTACT_I32][B] = PARTNERS (overlapping partners this tick), MAX_PARTNERS (carried).  A member that
 * does not take part on a tick reads 0 in FRICTION_IMPULSE, YAW_KICK and PARTNERS and keeps its carried words; a vehicle in no heat reads
 * NaN in every f64 channel and 0 in both i32 channels.
 *
 * Configuration (lpvmpc_contact_default_config: friction 0.3, yaw_response 1, the walls' values): friction >= 0 and finite,
 * yaw_response 0 / 1, reserved 0.  Restitution and push are read from the attached interactions.
 *
 * lpvmpc_race_contact attaches the contact model to the race of the path handle from the next tick on; attaching again replaces the
 * binding (its counters start anew; the interactions' go on), cfg == NULL goes back to the centres form.  It needs interactions attached
 * with contact = 1.  Refused with LPVMPC_E_ARG, the race left as it was: no race on the handle, no interactions attached, contact == 0,
 * a word that is not finite or out of range, reserved != 0.  The binding is built whole and then installed; the race owns it.
 * lpvmpc_race_interactions, whether it re-attaches or detaches, detaches the contact model first, and so does lpvmpc_race_heats.  While
 * attached lpvmpc_race_tick launches the contact model's kernel IN PLACE OF the interactions': one launch in the same position, behind
 * the disturbances' and in front of the walls'.  lpvmpc_race_contact_read synchronises and copies the two planes (either pointer may be
 * NULL); refused while nothing is attached.
 *
 * lpvmpc_contact_step_batch is one tick of the same kernel on caller-supplied data: lpvmpc_interaction_step_batch's arguments (of
 * plant_params word 3 is read as well) plus the contact configuration, the carried state ccarry_f64 [LPVMPC_CONTACT_CARRY_F64][B] /
 * ccarry_i32 [LPVMPC_CONTACT_CARRY_I32][B] in / out (just attached: zeros) and the two planes. */
#define LPVMPC_CONTACT_F64                  3
#define LPVMPC_CONTACT_FRICTION_IMPULSE     0
#define LPVMPC_CONTACT_YAW_KICK             1
#define LPVMPC_CONTACT_YAW_KICK_TOTAL       2
#define LPVMPC_CONTACT_I32                  2
#define LPVMPC_CONTACT_PARTNERS             0
#define LPVMPC_CONTACT_MAX_PARTNERS         1
#define LPVMPC_CONTACT_CARRY_F64            1
#define LPVMPC_CONTACT_CARRY_YAW_KICK_TOTAL 0
#define LPVMPC_CONTACT_CARRY_I32            1
#define LPVMPC_CONTACT_CARRY_MAX_PARTNERS   0
typedef struct lpvmpc_contact_config {
    double  friction;          /* >= 0 */
    int32_t yaw_response;      /* 0 / 1: 0 applies the impulses through the centres and leaves psiDot alone */
    int32_t reserved;          /* 0 */
} lpvmpc_contact_config;
void lpvmpc_contact_default_config(lpvmpc_contact_config *cfg);
int  lpvmpc_race_contact(lpvmpc_handle *path, const lpvmpc_contact_config *cfg /* NULL: back to the centres form */);
int  lpvmpc_race_contact_read(lpvmpc_handle *path, double *f64, int32_t *i32);
int  lpvmpc_contact_step_batch(lpvmpc_handle *h, int32_t B, int32_t n_heats, const int32_t *heat,
                               const lpvmpc_heats_config *heats_cfg, const lpvmpc_interaction_config *cfg,
                               const lpvmpc_contact_config *contact_cfg, int32_t t, double *plant /* [B][8] in/out */,
                               const double *plant_params /* [B][7] */, const int32_t *nstep /* [B] or NULL: all step */,
                               double *carry_f64, int32_t *carry_i32, double *ccarry_f64, int32_t *ccarry_i32,
                               double *mu_live /* [B] out */, double *f64, int32_t *i32, double *cf64, int32_t *ci32);

/* ---------------------------------------------------------------------------------------------------------------
 * Race event log: an ordered record, kept on the device, of what happened on each tick of a race.  The reads above answer "what is
 * the state after tick t" and the heats and the walls count since their attach; the log says who passed whom on which tick, when a
 * contact began and how long it lasted, and in what order cars hit the wall, for a race that ran hundreds of ticks in one
 * lpvmpc_race_tick call.  It is the race's fifth attachment and it only observes: no output of the race or of another attachment
 * changes by a bit while it is attached, and with nothing attached a tick issues exactly the launches it always did.  While it is
 * attached a tick issues one more launch, the last of the tick, behind the heats': phase, lap rows, the standings and the walls'
 * planes of this tick are final by then.  (On the first tick on which the log sees an attachment of the heats one small launch in
 * front of it fills the log's own table of each vehicle's heat from the heats' member lists.)
 *
 * An event is six int32 words and two doubles: i32 [LPVMPC_EVENT_I32] = TICK, KIND, VEHICLE, OTHER, A, B and f64 [LPVMPC_EVENT_F64] =
 * V0, V1.  TICK is the race's tick number counted before the tick, as the recorder's and the heats'.  An unused integer word is -1,
 * an unused double NaN.  "Before" and "after" below are the words the log stored at the end of the previous tick and the words that
 * stand at the end of this one.
 *
 * From the race itself:
 *   1 LAP            the vehicle's lap counter is larger than before.  A = the new lap counter, B = phase after,
 *                    V0 = (double)lap_step[b][A] as lpvmpc_race_laps returns it after this tick.
 *   2 FINISH         phase became 2.  A = lap counter.
 *   3 LOST           phase became 3.  A = lap counter.
 * From the heats, for a vehicle in a heat, while heats are attached:
 *   4 PASS           VEHICLE = i, OTHER = j, members of one heat: both are class 1 before and after, i was ordered behind j before
 *                    (POSITION larger) and is in front after.  A / B = POSITION of i / of j after, V0 = PROGRESS[i] - PROGRESS[j]
 *                    after (one subtraction).  This is the heats' own rule evaluated on the words the heats wrote, so per vehicle and
 *                    tick the number of PASS events with VEHICLE = b is the increment of PASSES[b], the number with OTHER = b that of
 *                    PASSED[b].
 *   5 CONTACT_BEGIN  the heats' CONTACT word went 0 -> 1.  OTHER = NEAREST, V0 = CLEARANCE.
 *   6 CONTACT_END    CONTACT went 1 -> 0.  OTHER = the NEAREST of the spell's last contact tick, A = the spell's length in ticks,
 *                    V0 = the smallest CLEARANCE over the spell's ticks.
 * From the walls, while walls are attached:
 *   7 WALL_HIT       HIT went 0 -> 1.  A = SIDE, B = CORNER, V0 = DEPTH, V1 = IMPULSE.
 *   8 WALL_CLEAR     HIT went 1 -> 0.  A = the spell's length in ticks, V0 = the largest IMPULSE of the spell.
 *
 * First sight.  On the first tick after its own attach the log stores the race's rows and emits nothing from them.  The same holds
 * per source on the first tick on which the log sees a given attachment of the heats or of the walls: one attached or replaced since
 * the last tick, or one present when the log was attached.  A spell open at first sight is taken as beginning then, without a BEGIN
 * event; when a source is detached its open spells are dropped without an END event.  The log holds no pointer of another layer:
 * lpvmpc_race_tick passes the current attachments' output planes and the heats' member lists at each launch, and a serial per slot,
 * bumped wherever an attachment is installed or detached, tells it which it has seen.  So the log stands alone in the detach chain,
 * as the walls do: attach and detach are independent of the other four layers, in any order.
 *
 * Order.  The events of a race are totally ordered by (TICK, VEHICLE, KIND, OTHER), all ascending; for PASS the VEHICLE is the passer.
 * This order is the log's contract, the same for every launch shape, batch size and run: a tick's slots come from an exclusive prefix
 * sum of the vehicles' event counts over the vehicle index, not from an atomic counter.
 * Ring.  The log keeps the last `capacity` events: the event with global index g (0-based since the attach) lives in slot
 * g % capacity; total is a 64-bit count of every event since the attach, kept and advanced on the device (a multi-tick lpvmpc_race_tick
 * does not synchronise).  A tick that produces more events than capacity keeps exactly its last capacity events: an event is written
 * only when g >= total_after_tick - capacity, so no two writes of one tick meet in a slot.
 * Kinds mask.  Bit k of kinds selects kind k.  An unselected kind is neither written nor counted; its state is still carried.
 * Per-vehicle outputs i32 [LPVMPC_EVENT_OUT_I32][B] = COUNT (events with this VEHICLE on the last tick), COUNT_TOTAL (since the
 * attach); 0 before the first tick.
 *
 * lpvmpc_race_events attaches the log from the next tick on; attaching again replaces the binding and its count starts at 0;
 * cfg == NULL detaches.  Refused with LPVMPC_E_ARG, the race left as it was: no race on the handle, capacity < 1 or a size that
 * overflows, a kinds bit outside 1 .. 8, reserved != 0.  The binding is built whole and then installed; the race owns it
 * (lpvmpc_cl_release(path) or destroying a handle frees it, a new race starts without one).  lpvmpc_race_snapshot works while it is
 * attached and does not contain it; lpvmpc_race_restore and lpvmpc_race_clone are refused while it is attached, as with the heats:
 * before and after mean nothing across a restore.  lpvmpc_event_default_config: capacity 65536, every kind.
 *
 * lpvmpc_race_events_read synchronises and copies the last m = min(n, kept) events, oldest first, with kept = min(total, capacity):
 * i32 [m][LPVMPC_EVENT_I32], f64 [m][LPVMPC_EVENT_F64], and the output plane out_i32 [LPVMPC_EVENT_OUT_I32][B].  Any pointer may be
 * NULL.  Refused with LPVMPC_E_ARG for n < 0 and while nothing is attached.
 *
 * lpvmpc_event_step_batch is one tick of the same device function on caller-supplied data, on a handle that runs no fleet, cascade or
 * race: t, phase [B], lap [B], lap_value [B] (the V0 of a LAP event); the heats' side n_heats, heat [B] with indices in [-1, n_heats)
 * and the heats' two output planes heat_f64 [LPVMPC_HEAT_F64][B] / heat_i32 [LPVMPC_HEAT_I32][B] (all three NULL: no heats); the
 * walls' two output planes wall_f64 / wall_i32 (both NULL: no walls); kinds; the carry planes carry_f64 [LPVMPC_EVENT_CARRY_F64][B] /
 * carry_i32 [LPVMPC_EVENT_CARRY_I32][B] in / out; total [1] in / out; max_events and the two event arrays i32 [max_events][6] /
 * f64 [max_events][2], filled from index 0 with this tick's events in order (only the first max_events are written); n_events [1] =
 * how many the tick produced; out_i32 the per-vehicle output plane.  An all-zero carry is "just attached".  FLAGS bit 0: the race's
 * rows are stored; bit 1 / bit 2: the heats' / the walls' words are stored (cleared on a tick without that source, and for a vehicle
 * in no heat).  COUNT_TOTAL is carried; every other word is the "before" word of its name, the spells' first ticks and extrema. */
#define LPVMPC_EVENT_I32                 6
#define LPVMPC_EVENT_TICK                0
#define LPVMPC_EVENT_KIND                1
#define LPVMPC_EVENT_VEHICLE             2
#define LPVMPC_EVENT_OTHER               3
#define LPVMPC_EVENT_A                   4
#define LPVMPC_EVENT_B                   5
#define LPVMPC_EVENT_F64                 2
#define LPVMPC_EVENT_V0                  0
#define LPVMPC_EVENT_V1                  1
#define LPVMPC_EVENT_LAP                 1
#define LPVMPC_EVENT_FINISH              2
#define LPVMPC_EVENT_LOST                3
#define LPVMPC_EVENT_PASS                4
#define LPVMPC_EVENT_CONTACT_BEGIN       5
#define LPVMPC_EVENT_CONTACT_END         6
#define LPVMPC_EVENT_WALL_HIT            7
#define LPVMPC_EVENT_WALL_CLEAR          8
#define LPVMPC_EVENT_ALL_KINDS           0x1FEu
#define LPVMPC_EVENT_OUT_I32             2
#define LPVMPC_EVENT_COUNT               0
#define LPVMPC_EVENT_COUNT_TOTAL         1
#define LPVMPC_EVENT_CARRY_F64           2
#define LPVMPC_EVENT_CARRY_MIN_CLEARANCE 0  /* smallest CLEARANCE of the open contact spell */
#define LPVMPC_EVENT_CARRY_MAX_IMPULSE   1  /* largest IMPULSE of the open wall spell */
#define LPVMPC_EVENT_CARRY_I32          11
#define LPVMPC_EVENT_CARRY_FLAGS         0
#define LPVMPC_EVENT_CARRY_PHASE         1
#define LPVMPC_EVENT_CARRY_LAP           2
#define LPVMPC_EVENT_CARRY_POSITION      3
#define LPVMPC_EVENT_CARRY_CLASS         4
#define LPVMPC_EVENT_CARRY_CONTACT       5
#define LPVMPC_EVENT_CARRY_NEAREST       6  /* NEAREST of the spell's last contact tick */
#define LPVMPC_EVENT_CARRY_CONTACT_START 7  /* first tick of the open contact spell, -1: none */
#define LPVMPC_EVENT_CARRY_HIT           8
#define LPVMPC_EVENT_CARRY_HIT_START     9  /* first tick of the open wall spell, -1: none */
#define LPVMPC_EVENT_CARRY_COUNT_TOTAL  10
typedef struct lpvmpc_event_config {
    int32_t  capacity;         /* >= 1: events kept */
    uint32_t kinds;            /* bit k selects kind k, 1 .. 8 */
    int32_t  reserved[2];      /* 0 */
} lpvmpc_event_config;
void lpvmpc_event_default_config(lpvmpc_event_config *cfg);
int  lpvmpc_race_events(lpvmpc_handle *path, const lpvmpc_event_config *cfg /* NULL: detach */);
int  lpvmpc_race_events_read(lpvmpc_handle *path, int32_t n, int64_t *total, int32_t *kept, int32_t *i32 /* [m][6] */,
                             double *f64 /* [m][2] */, int32_t *out_i32 /* [2][B] */);
int  lpvmpc_event_step_batch(lpvmpc_handle *h, int32_t B, int32_t t, const int32_t *phase, const int32_t *lap, const double *lap_value,
                             int32_t n_heats, const int32_t *heat, const double *heat_f64, const int32_t *heat_i32,
                             const double *wall_f64, const int32_t *wall_i32, uint32_t kinds, double *carry_f64, int32_t *carry_i32,
                             int64_t *total, int32_t max_events, int32_t *i32, double *f64, int32_t *n_events, int32_t *out_i32);

#ifdef __cplusplus
}
#endif
#endif /* LPVMPC_H */
