// lpvmpc_device.hpp -- device-side configuration shared by the kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace lpvmpc {

constexpr int kMaxSeg = 16;   // rows of the track table kept in the kernel argument block
constexpr int kTS = 72;       // LDS stride (doubles) of one 8x8 tile: 64 + 8 pad => stage tiles start 16 banks apart

// OSQP constants (0.6.x), see oracle/osqp_ref.c header
constexpr double kInfty = 1e30;
constexpr double kRhoMin = 1e-6, kRhoMax = 1e6, kRhoEqOverIneq = 1e3, kRhoTol = 1e-4;
constexpr double kMinScaling = 1e-4, kMaxScaling = 1e4;

struct DevCfg {
    int32_t kind, N, track_rows, max_iter;
    int32_t check_termination, scaling, adaptive_rho, adaptive_rho_interval;
    int32_t polish, polish_refine_iter, steering_delay, pad1;
    double dt, lf, lr, m, Iz, Cf, Cr, mu, max_vel, min_vel;
    // the tuning words: kTuneWords contiguous doubles, the device row of lpvmpc_set_tunings (a row of the handle's table replaces them
    // per instance in the solve kernel's set-up block; nothing else on the device reads them)
    double Q[36], R[4], dR[2], Lcf[6];
    double box_lo[8], box_hi[8];   // per-stage box rows, unscaled (planner row 3 = ey is per instance)
    double rho, sigma, alpha, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf, delta, rho_tol;
    double track[kMaxSeg * 6];
};

// Piecewise-constant curvature lookup, reference UTIL:31-50 (Curvature).  Same wrap (repeated subtraction of the track
// length, UTIL:36-40) and the same comparisons (s >= start && s < start + len) in float64.  Where the reference raises
// (UTIL:44-48 finds no segment: s < 0, s exactly on the end of the closing segment) or would spin (s not finite, or more than
// kMaxWrapLaps track lengths ahead: a diverged roll-out) the lookup returns NaN: the NaN travels through the LPV blocks into
// the solve kernel, which runs no iteration on non-finite data and reports LPVMPC_UNSOLVED with NaN outputs -- the caller
// sees the failure instead of a silently substituted segment.
constexpr int kMaxWrapLaps = 4096;
__device__ inline double wrap_track_s(double s, double L) {
    if (!(s <= L * (double)kMaxWrapLaps)) return __builtin_nan("");     // also catches NaN and +Inf
    for (int it = 0; it < kMaxWrapLaps && s > L; ++it) s -= L;
    return s;
}
// The track functions are written once, on a table T [rows][6] of PointAndTangent rows; the configuration's own table (here) and a
// palette entry (track_view.hpp) forward to them.
__device__ inline double track_curvature(const double *T, int rows, double s) {
    const double L = T[(rows - 1) * 6 + 3] + T[(rows - 1) * 6 + 4];
    s = wrap_track_s(s, L);
    for (int i = 0; i < rows; ++i) {
        const double st = T[i * 6 + 3], ln = T[i * 6 + 4];
        if (s >= st && s < st + ln) return T[i * 6 + 5];
    }
    return __builtin_nan("");
}
__device__ __forceinline__ double track_curvature(const DevCfg &c, double s) { return track_curvature(c.track, c.track_rows, s); }

// offsets of the tuning words within their block (DevCfg::Q onward) and within a device row of the tuning table
constexpr int kTuneWords = 64;               // = LPVMPC_TUNING_WORDS
constexpr int kTuneR = 36, kTunedR = 40, kTuneLcf = 42, kTuneLo = 48, kTuneHi = 56;
static_assert(offsetof(DevCfg, R) - offsetof(DevCfg, Q) == kTuneR * sizeof(double) && offsetof(DevCfg, dR) - offsetof(DevCfg, Q) == kTunedR * sizeof(double) &&
              offsetof(DevCfg, Lcf) - offsetof(DevCfg, Q) == kTuneLcf * sizeof(double) && offsetof(DevCfg, box_lo) - offsetof(DevCfg, Q) == kTuneLo * sizeof(double) &&
              offsetof(DevCfg, box_hi) - offsetof(DevCfg, Q) == kTuneHi * sizeof(double) && offsetof(DevCfg, rho) - offsetof(DevCfg, Q) == kTuneWords * sizeof(double),
              "the tuning words are one contiguous block of DevCfg");

// arguments of the solve kernel (device pointers)
struct SolveArgs {
    int B;
    const double *x0;       // [B][x0_stride], first NX used
    const double *AB;       // [B][N][NX][NX+2]
    const double *vel_ref;  // [B][N+1]   controller
    const double *u_old;    // [B][2 + steering_delay] or null
    const double *max_ey;   // [B]        planner
    double *xPred;          // [B][N+1][NX]
    double *uPred;          // [B][N][2]
    int32_t *status, *iters, *polish;
    double *resid;          // [B][4]
    double *state;          // [B][3][8(N+1)] unscaled x, y(dynamics rows), y(box rows) of the previous solve, or null
    int warm;               // 0 cold start (reference behaviour), 1 warm start from state, 2 same shifted by one stage
    int x0_stride;          // doubles between consecutive instances' x0 (NX, or N*NX when x0 = first rolled-out state)
    // straggler deferral (lpvmpc_set_option "defer_after"): an instance that is still unsolved at a termination check after its
    // iteration budget is PARKED -- its whole LDS image, loop state and output pointers go to a pool entry -- and the workgroup
    // ends; a later launch of the same kernel with resume = 1 (one workgroup per entry of pool_in) restores it, re-factors K
    // with the saved rho (a pure function of the saved image, so the iterates continue bit for bit) and runs it for another
    // budget (parking it again in pool) or to completion (defer_after = 0).
    int defer_after;        // main launch: park at the first check with iter >= defer_after; resume launch: after that many more
                            // iterations; 0: run to completion
    int resume;             // 1: continue the parked instances of pool_in (blockIdx.x = entry)
                            // 2: a main launch that carries riders (grid pool_cap + B): workgroups 0 .. pool_cap-1 continue the entries of
                            // pool_in for defer_budget more iterations as a resume launch would -- the low block indices are dispatched first,
                            // so the long runners start first -- and workgroups pool_cap .. pool_cap+B-1 are instances blockIdx.x - pool_cap
                            // of the call (B, active and defer_after apply to them only); both park into pool
    double *pool;           // [pool_cap][pool_stride] entries written by this launch
    int32_t *pool_count;    // [4]: slots requested so far in pool (may exceed pool_cap: the surplus instances were not parked), [1] see pool_in_count,
                            // [2] / [3] requests of the young / middle age class (admission by age: Solver::park_slot)
    unsigned long long *defer_stats;   // [2]: instances parked / parking attempts refused (pool share of the instance's age class full) by launches of this handle
    const double *pool_in;  // resume: entries to continue
    int32_t *pool_in_count; // [4]: entries, the number of resume workgroups that have read it, the class counters (the last reader clears all:
                            // the pool is empty again when the pass ends, without a separate memset launch)
    int pool_cap, pool_stride;
    // planner N = 30, no deferral: the three equilibration vectors (D, E of the dynamics rows, E of the box rows) of instance i
    // live at scal + i * 3 * 8 (N + 1) in global memory instead of LDS (they are read at set-up, at the termination checks and by
    // the factorisations, never inside an ADMM iteration), which brings the instance under a third of a CU's LDS; null: in LDS
    double *scal;
    // resume launches that run to completion (defer_after == 0): 1 = take the whole-CU tail kernel where one exists for the
    // handle's (kind, N) (lpvmpc_set_option "defer_tail", default on); it continues the same pool entries
    int tail;
    // [B] active-instance mask of a main launch (null: every instance).  A workgroup whose flag is 0 returns at its entry, before it
    // reads or writes anything (its output rows and carried state stay as they are; it never parks).  Resume launches ignore it.
    const int32_t *active;
    int defer_budget;       // resume = 2: iterations the riders continue for before they park again (defer_after is the new instances' word there;
                            // a resume launch carries its budget in defer_after, as before)
    // [B][kTuneWords] per-instance tuning words (lpvmpc_set_tunings), instance-major: one workgroup reads one 512-byte row at
    // wave-uniform addresses.  Indexed by instance of the call (a masked launch reads the rows of the vehicles it runs).  null: the
    // configuration block's own words.  Resume, riders and tail launches read nothing from it: the parked image carries the words
    const double *tune;
};
constexpr int kParkScalars = 16;     // behind the LDS image of a pool entry: c, cinv, rho, iter, to_chk, to_adp, instance index and the
                                     // instance's output pointers (xPred, uPred, status, iters, polish, resid, state) as 64-bit words
constexpr int LPVMPC_PENDING_ = -11; // status of a parked instance until its resume launch has finished it (lpvmpc.h: LPVMPC_PENDING)

// host-side launchers (defined next to their kernels)
int solve_has_fast_path(int kind, int N);
size_t solve_lds_bytes(int kind, int N);
hipError_t launch_solve(const DevCfg &cfg, const DevCfg *dcfg, const SolveArgs &a, hipStream_t stream, int force_generic);
// active: optional [B] instance mask (null: every instance); a masked instance's rows of states / AB are not written.
// model: the handle's per-vehicle model table (below), or null: the handle's own vehicle words
// trk: the handle's track binding (below), or null: the configuration's own table; own_model: with trk, the binding's table of the
// handle's own vehicle words, which the bound forms read where model is null
struct TrackDev;
hipError_t launch_lpv(const DevCfg &cfg, const DevCfg *dcfg, const double *model, int B, const double *x0, const double *u_prev,
                      const double *vel_ref, const double *curv_s, double cf_new, int lap, double *states, double *AB, hipStream_t stream,
                      const int32_t *active = nullptr, const TrackDev *trk = nullptr, const double *own_model = nullptr);
hipError_t launch_abc(const DevCfg &cfg, const DevCfg *dcfg, const double *model, int B, const double *xlast, const double *delta, double *AB,
                      hipStream_t stream, const int32_t *active = nullptr, const TrackDev *trk = nullptr, const double *own_model = nullptr);
// per-vehicle model parameters (veh_lpv_eval.hip; lpvmpc_set_model_params, include/lpvmpc.h "Per-vehicle model parameters"): the
// handle's table [kModelWords][B], parameter-major and vehicle-minor like the plant table below, indexed by vehicle (not by launch
// slot: masked launches read the rows of the vehicles they run).  The launchers of the per-vehicle forms, called by the two above
constexpr int kModelWords = 7;               // = LPVMPC_MODEL_WORDS: lf, lr, m, Iz, Cf, Cr, mu
void launch_ctrl_lpv_pre_veh(const DevCfg *dcfg, const double *model, int B, int N, const double *u_prev, const double *vel_ref, double *AB,
                             hipStream_t stream, const int32_t *active);
void launch_lpv_veh(int kind, const DevCfg *dcfg, const double *model, int B, const double *x0, const double *u_prev, const double *vel_ref,
                    const double *curv_s, int lap, double *states, double *AB, hipStream_t stream, const int32_t *active);
void launch_abc_veh(int kind, const DevCfg *dcfg, const double *model, int B, int N, const double *xlast, const double *delta, double *AB,
                    hipStream_t stream, const int32_t *active);

// per-vehicle tracks (track_view.hpp; lpvmpc_set_tracks, include/lpvmpc.h "Per-vehicle tracks"): the launchers of the bound forms
// (track_vehicles.hip: the stand-alone transforms; track_lpv_eval.hip: the LPV / ABC kernels that read the track, called by the two
// launchers above).  model: a table [kModelWords][B], never null: the handle's bound model rows, or the binding's table of the handle's
// own words
hipError_t launch_local_position_trk(const TrackDev &trk, int B, const double *xypsi, double *out, hipStream_t s);
hipError_t launch_global_position_trk(const TrackDev &trk, int B, const double *sey, double *out, hipStream_t s);
void launch_ctrl_lpv_roll_trk(const DevCfg *dcfg, const TrackDev &trk, int B, const double *x0, const double *u_prev, const double *curv_ref,
                              int lap, double *states, double *AB, hipStream_t stream, const int32_t *active);
void launch_plan_lpv_trk(const DevCfg *dcfg, const TrackDev &trk, const double *model, int B, const double *x0, const double *u_prev,
                         const double *SS, double *states, double *AB, hipStream_t stream, const int32_t *active);
void launch_abc_trk(int kind, const DevCfg *dcfg, const TrackDev &trk, const double *model, int B, int N, const double *xlast,
                    const double *delta, double *AB, hipStream_t stream, const int32_t *active);

// closed-loop helpers (closed_loop.hip)
struct PlantCfg { double lf, lr, m, Iz, mu, dt; int n_sub; };
hipError_t launch_local_position(const DevCfg *dcfg, int B, const double *xypsi, double half_width, double slack, double *out, hipStream_t s);
hipError_t launch_global_position(const DevCfg *dcfg, int B, const double *sey, double *out, hipStream_t s);
hipError_t launch_cl_seed(int B, int N, const double *local_state, double *xlast, double *delta, hipStream_t s);

// actuator stage of the simulator (fleet_kernels.hpp, actuator.hip; vehicleSimulator.py:53-78; lpvmpc_*_actuated, include/lpvmpc.h "Actuator delay and servo lag"):
// per vehicle a ring of its last kActRing commands in global memory (a runtime-indexed per-lane array would live in scratch), the
// servo state and the vehicle's own plant-step counter, which keys the ring
constexpr int kActRing = 64;                 // = LPVMPC_ACT_MAX_DELAY: step k reads slot (k - L) % kActRing before overwriting slot k % kActRing
struct ActDev {
    double *ring;                            // [2][kActRing][B]: channel 0 motor, 1 servo; slot k % kActRing holds the command of plant step k
    double *servo;                           // [B] servo_inp of the low-level servo model
    int32_t *k;                              // [B] plant steps the vehicle has taken
    const int32_t *La, *Ld;                  // [B] motor / steering delay in plant steps, 0 .. kActRing
    int B, lld;                              // lld: lowLevelDyn
    double c, c1;                            // T / Tf and 1 - T / Tf
};

// per-vehicle plant parameters (plant_params.hip; lpvmpc_*_vehicles, include/lpvmpc.h "Per-vehicle plant parameters"): the fleet's
// table [kPlantWords][B], parameter-major and vehicle-minor like the actuator ring, so that a wavefront's loads of one word coalesce.
// It is the per-vehicle forms' own kernel argument: PlantCfg, which every other fleet kernel takes by value, keeps its layout
constexpr int kPlantWords = 7;               // = LPVMPC_PLANT_WORDS: lf, lr, m, Iz, Cf, Cr, mu
struct VehPlantCfg {
    const double *p;                         // [kPlantWords][B]
    int B;                                   // the table's row stride (vehicles)
    double dt; int n_sub;                    // fleet-wide, as in PlantCfg
};
// tyre model (tyre.hip; lpvmpc_*_tyres, include/lpvmpc.h "Tyre model"): the per-vehicle forms' argument plus the fleet's tyre table
// [kTyreWords][B], laid out and read like the plant table
constexpr int kTyreWords = 4;                // = LPVMPC_TYRE_WORDS: kind (0 linear, 1 Pacejka), B, C, c_f
struct TyrePlantCfg : VehPlantCfg {
    const double *t;                         // [kTyreWords][B], the stride is VehPlantCfg::B
};
// the plant argument of a fleet kernel (fleet_kernels.hpp): one PlantCfg for the fleet, the table (kVeh), or the table and the tyre
// table (kTyre)
template <bool kVeh, bool kTyre = false> struct PlantArgT { using type = PlantCfg; };
template <> struct PlantArgT<true, false> { using type = VehPlantCfg; };
template <> struct PlantArgT<true, true> { using type = TyrePlantCfg; };
template <bool kVeh, bool kTyre = false> using PlantArg = typename PlantArgT<kVeh, kTyre>::type;
// force [B] = the tyre curve of row b of tyre [kTyreWords][B] at slip angle alpha [B] for a vehicle of mass m [B]
hipError_t launch_tyre_force(int B, const double *tyre, const double *m, const double *alpha, double *force, hipStream_t s);


// gain-scheduled LPV estimator and simulated sensors (observer.hip)
constexpr int kObsTable = 6 * 5 * 16;   // one Llmi table [6][5][16]
constexpr int kObsAux = 30 + 36 + 12;   // L_gain [6][5], A_obs [6][6], B_obs [6][2] of lpvmpc_observer_step_batch
// per-vehicle estimator state of a fleet, [B][kObsStride] doubles (counters are stored as exact integers)
enum ObsSlot { OBS_EST = 0, OBS_Y = 6, OBS_GPS_X = 11, OBS_GPS_Y = 12, OBS_ENC_PREV = 13, OBS_ENC_MEAS = 14, OBS_GPS_CNT = 15,
               OBS_ENC_CNT = 16, OBS_K = 17 };
constexpr int kObsStride = 18;
// sensor std order = noise channel: psi, psiDot, x, y, v
struct ObsParams { double dt, th_update, n_bound, std[5]; unsigned long long seed; long long voff; };
// per-vehicle estimator (lpvmpc_set_observer_vehicles): the binding's model rows [kPlantWords][B] and gain planes [2][kObsTable][B]
// (polytope, gain word, vehicle: the 64 lanes of a workgroup read consecutive words); with the gain words' pointer g, the `gains`
// argument of the bound estimator kernels (observer_vehicles.hip)
struct ObsVehDev { const double *rows = nullptr, *L = nullptr; int B = 0; };
struct ObsVehGains : ObsVehDev { const double *g = nullptr; };
hipError_t launch_observer_step(const double *gains, int B, double *est, const double *y, const double *u, const int32_t *k, double dt,
                                double *aux, hipStream_t s);


// planner -> controller hand-off and trajectory-tracking measurement (handoff.hip)
#define LPVMPC_HANDOFF_MAX_N 64
int handoff_length(int N, double dt, double interp_dt);
hipError_t launch_plan_pose(const DevCfg *dcfg, int B, const double *xPred, double *SS, double *pose, double *sig, hipStream_t s,
                            const int32_t *active = nullptr);
hipError_t launch_resample(int B, int N, int M, const double *WT, const double *FWT, const double *sig, double *refs, hipStream_t s,
                           const int32_t *active = nullptr);
hipError_t launch_plan_first(const DevCfg *dcfg, int B, const double *plant, double hw, double slack, int q9_swap, double accel_rate,
                             double *x0, double *xlast, double *delta, hipStream_t s);
hipError_t launch_tt_measure(const DevCfg *dcfg, int B, int M, int tick, const double *plant, const double *cmd, const double *refs, int latch,
                             double *vel, double *curv, double *ref0, int32_t *lap, int32_t *lap_tick, double *SS, double *local_state,
                             double *u_old, int32_t *alive_ticks, hipStream_t s);

// race engine: lap 0, lap events and racing with a phase per vehicle (race.hip)
struct RaceDev {              // device pointers and constants of one race (lpvmpc_race_*), passed by value
    int B, N, Np, M, laps, q9, n_sub_lap0, n_sub[3], lap_cols;
    double hw, slack;
    double *plant, *cmd, *local;                // [B][8], [B][2], [B][6]
    const double *meas;                         // [B][8] what the measurements read: the plant, or with an estimator estv
    double *estv;                               // [B][8] with an estimator: the estimate in the plant's layout [x y vx vy 0 0 yaw psiDot]
    int32_t *phase, *lap, *half, *rk, *plan_done, *idx;   // [B]: phase, lap counter, HalfTrack, racing ticks done, planner ticks done, `index`
    int32_t *nstep, *src;                       // [B] this tick: plant steps; controller that solved (0 path, 1 TT, -1 none)
    int32_t *step, *lap_step, *alive;           // [B] plant steps so far; [B][lap_cols] step at which each lap starts (-1: not yet); alive ticks
    int32_t *iters, *status;                    // [B] the vehicle's controller solve of the last tick
    int32_t *m_path, *m_tt, *m_plan, *m_pfirst, *m_pcont;   // [B] masks of this tick
    double *SSc, *ref0, *refs;                  // [B], [B][3], [B][5][M] (the vehicle's latest planner message)
    double *SSp, *pose, *sig;                   // planner carried state [B][Np+1], [B][3]; scratch [B][5][Np]
    // the three handles' workspaces
    double *p_uold, *p_uPred, *p_vel, *p_curv;  // path
    int32_t *p_iters, *p_status;
    double *t_uold, *t_uPred, *t_vel, *t_curv;  // trajectory tracking
    int32_t *t_iters, *t_status;
    double *q_x0, *q_xPred, *q_xlast, *q_delta; // planner
};
hipError_t launch_race_plan_start(const DevCfg *pcfg, const RaceDev &r, hipStream_t s);
// observer_vehicles.hip: the per-vehicle-estimator forms
hipError_t launch_observer_step_vehicles(const ObsVehGains &v, int B, double *est, const double *y, const double *u, const int32_t *k, double dt,
                                         double *aux, hipStream_t s);

// track_race.hip: the bound forms of the race's, the hand-off's and the recorder's kernels that read the track (RecDev: record.hpp)
struct RecDev;
hipError_t launch_race_plan_start_trk(const DevCfg *pcfg, const TrackDev &trk, const RaceDev &r, hipStream_t s);
hipError_t launch_plan_pose_trk(const DevCfg *dcfg, const TrackDev &trk, int B, const double *xPred, double *SS, double *pose, double *sig,
                                hipStream_t s, const int32_t *active = nullptr);
hipError_t launch_race_record_trk(const TrackDev &trk, const RecDev &r, int t, int slot, hipStream_t s);

// plant disturbances (disturbance.hip; lpvmpc_set_disturbances, include/lpvmpc.h "Plant disturbances"): the binding on the device,
// passed by value to the one kernel that runs in front of a tick's command / plant kernel.  Every table is word-major [word][B]
constexpr int kDistWords = 13;               // = LPVMPC_DIST_WORDS
constexpr int kDistState = 5;                // = LPVMPC_DIST_STATE: d_ax, d_ay, d_aw, ticks, gamma
struct DistDev {
    const double *rows;                      // [kDistWords + 1][B]: the public words, then q = sqrt(1 - rho^2)
    double *state;                           // [kDistState][B]
    const double *base;                      // [3][B]: Cf, Cr of the base plant rows, c_f of the base tyre rows
    double *live_p, *live_t;                 // the fleet's plant table [kPlantWords][B] and tyre table [kTyreWords][B]
    double *plant;                           // [B][8]
    const int32_t *k;                        // [B] ActDev::k, the vehicle's plant-step counter
    const int32_t *nstep;                    // [B] plant steps of this tick (a race's), or null: n_fixed for every vehicle
    int B, n_fixed;
    double dt, n_bound, hw, slack;           // dt_sim; the clip in standard deviations; the unbound form's map width
    unsigned long long seed;                 // the configuration's seed ^ LPVMPC_DIST_STREAM
    long long voff;
};
// trk null: the handle's own track (dcfg, d.hw, d.slack); else every vehicle on its palette entry
hipError_t launch_disturbance(const DevCfg *dcfg, const TrackDev *trk, const DistDev &d, hipStream_t s);

// tyre wear and temperature (tyre_wear.hip; lpvmpc_set_tyre_wear, include/lpvmpc.h "Tyre wear and temperature"): the binding on the
// device, passed by value to the one kernel that runs behind the disturbances' and immediately in front of a tick's command / plant
// kernel.  Every table is word-major [word][B]
constexpr int kWearWords = 12;               // = LPVMPC_WEAR_WORDS
constexpr int kWearState = 6;                // = LPVMPC_WEAR_STATE: W, T, P, g, ticks, E
struct WearDev {
    const double *rows;                      // [kWearWords][B]: the public words
    double *state;                           // [kWearState][B]
    const double *base;                      // [5][B]: Cf, Cr of the base plant rows, c_f of the base tyre rows, lr and m of the base plant rows
    const double *gamma;                     // [B] the disturbances' gamma of this tick (word 4 of DistDev::state), null: none attached
    double *live_p, *live_t;                 // the fleet's plant table [kPlantWords][B] and tyre table [kTyreWords][B]
    const double *plant;                     // [B][8]
    const int32_t *nstep;                    // [B] plant steps of this tick (a race's), or null: n_fixed for every vehicle
    int B, n_fixed;
    double dt;                               // dt_sim
};
hipError_t launch_tyre_wear(const WearDev &d, hipStream_t s);

// sensor faults (sensor_faults.hip; lpvmpc_set_sensor_faults, include/lpvmpc.h "Sensor faults"): the binding on the device, passed
// by value to the faulted fused kernels, which a tick launches in place of its command / plant / observe kernel
constexpr int kFaultWords = 12;              // = LPVMPC_FAULT_WORDS
struct FaultDev {
    const double *rows;                      // [kFaultWords][B], word-major
    int B;                                   // the table's row stride (vehicles)
    unsigned long long seed;                 // the configuration's seed ^ LPVMPC_FAULT_STREAM
    long long voff;
};
// lpvmpc_sensor_step_batch: one sensors + observer sub-step on caller arrays; f.rows null: the healthy stage; v.L null: the
// configuration's tables and the observer's own constants
hipError_t launch_sensor_step(const ObsVehGains &v, int B, double *obs, const double *plant, const double *servo, const double *motor,
                              const ObsParams &op, const FaultDev &f, hipStream_t s);

// The kernels that advance a plant come in forms (fleet_kernels.hpp: delayed, per-vehicle plant, tyre, estimator, per-vehicle gains;
// track_vehicles.hip / track_race.hip: bound tracks; sensor_faults.hip: faults), one form per translation unit.  Each family has one
// argument struct, the union of what its kernels take, and every launcher of the family has the one signature below; it stands next
// to its kernel and reads what that kernel takes.  Which launcher serves an engine is decided in one place: step_form.hpp maps the
// engine's form to a kernel enumerator, fleet_launch.hip binds the enumerators to the launchers (null: the form has no kernel).
// tpc slices to the per-vehicle forms' VehPlantCfg; gains.g is the plain forms' `gains`.
#define LPVMPC_GRID(n) dim3(((n) + 63) / 64), dim3(64)
struct FleetStepArgs {        // lpvmpc_cl_tick: command, plant and the coming tick's measurement (hw, slack: the unbound forms' map)
    const DevCfg *dcfg; const TrackDev *trk;
    int B, N;
    const double *uPred; double *cmd, *plant;
    PlantCfg pc; TyrePlantCfg tpc;
    double hw, slack; int q9;
    double *local_next, *u_old; int sd;
    ObsVehGains gains; double *obs; ObsParams op;
    ActDev act; FaultDev fault;
};
struct FleetMeasureArgs {     // the first tick's measurement: of the plant, or with an estimator of obs
    const DevCfg *dcfg; const TrackDev *trk;
    int B;
    const double *plant, *obs, *cmd;
    double hw, slack; int q9;
    double *local_state, *u_old; int sd;
};
struct RaceStepArgs { RaceDev r; PlantCfg pc; TyrePlantCfg tpc; ObsVehGains gains; double *obs; ObsParams op; ActDev act; FaultDev fault; };
struct RaceMeasureArgs { const DevCfg *ccfg; const TrackDev *trk; RaceDev r; int seed_tick, sd; };
struct PlantStepArgs { int B; double *plant; const double *u; PlantCfg pc; TyrePlantCfg tpc; ActDev act; };
using FleetStepFn = hipError_t(const FleetStepArgs &, hipStream_t);
using FleetMeasureFn = hipError_t(const FleetMeasureArgs &, hipStream_t);
using RaceStepFn = hipError_t(const RaceStepArgs &, hipStream_t);
using RaceMeasureFn = hipError_t(const RaceMeasureArgs &, hipStream_t);
using PlantStepFn = hipError_t(const PlantStepArgs &, hipStream_t);
// closed_loop.hip, observer.hip, race.hip: the plain forms; actuator.hip: the delayed forms; plant_params.hip: the per-vehicle forms;
// tyre.hip: the tyre forms; observer_vehicles.hip: the per-vehicle-estimator forms; track_vehicles.hip, track_race.hip: the bound forms;
// sensor_faults.hip: the faulted forms
FleetStepFn launch_cl_command_plant_measure, launch_cl_command_plant_observe, launch_cl_command_plant_measure_act, launch_cl_command_plant_observe_act,
    launch_cl_command_plant_measure_veh, launch_cl_command_plant_observe_veh, launch_cl_command_plant_measure_tyre, launch_cl_command_plant_observe_tyre,
    launch_cl_command_plant_observe_veh_obsveh, launch_cl_command_plant_observe_tyre_obsveh, launch_cl_command_plant_measure_trk,
    launch_cl_command_plant_observe_trk, launch_cl_command_plant_observe_trk_obsveh, launch_cl_command_plant_observe_faulted,
    launch_cl_command_plant_observe_faulted_obsveh;
// the cascade's step (no table: it has the plain forms only): command and plant, and with its estimator the estimate's view in local_next
FleetStepFn launch_cl_command_plant, launch_cascade_plant_observe;
FleetMeasureFn launch_cl_measure, launch_cl_observe_measure, launch_cl_measure_act, launch_cl_observe_measure_act, launch_cl_measure_trk,
    launch_cl_observe_measure_trk;
RaceStepFn launch_race_command_plant, launch_race_command_plant_observe, launch_race_command_plant_act, launch_race_command_plant_observe_act,
    launch_race_command_plant_veh, launch_race_command_plant_observe_veh, launch_race_command_plant_tyre, launch_race_command_plant_observe_tyre,
    launch_race_command_plant_observe_veh_obsveh, launch_race_command_plant_observe_tyre_obsveh, launch_race_command_plant_observe_faulted,
    launch_race_command_plant_observe_faulted_obsveh;
RaceMeasureFn launch_race_measure, launch_race_measure_act, launch_race_measure_trk;
PlantStepFn launch_plant, launch_plant_actuated, launch_plant_veh, launch_plant_tyre;
// fleet_launch.hip: the launcher of a form (step_form.hpp: step_form), null: the family has no kernel for it
FleetStepFn *fleet_step_launcher(unsigned form);
FleetMeasureFn *fleet_measure_launcher(unsigned form);
RaceStepFn *race_step_launcher(unsigned form);
RaceMeasureFn *race_measure_launcher(unsigned form);
PlantStepFn *plant_step_launcher(unsigned form);

}  // namespace lpvmpc
