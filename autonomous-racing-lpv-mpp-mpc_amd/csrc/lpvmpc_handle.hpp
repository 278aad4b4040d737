// lpvmpc_handle.hpp -- private host-side definitions shared by every translation unit that implements the C ABI, the *_api.hip files:
// lpvmpc_api.hip (solver entry points and the lap-0 fleet), cascade_api.hip (hand-off and planner + controller cascade), race_api.hip
// (the race engine) and race_state_api.hip (its snapshot, restore and clone); the bindings of a handle or of its engine's plant side
// (actuator_, plant_params_, tyre_, model_params_, tunings_, observer_design_, tracks_, disturbance_, tyre_wear_, sensor_faults_api.hip); and,
// through race_attach.hpp, what attaches to a running race (heats_, interactions_, contact_, walls_api.hip).  No kernel translation
// unit includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "lpvmpc.h"
#include "lpvmpc_device.hpp"
#include "step_form.hpp"
#include "track_view.hpp"

#define LPVMPC_HIDDEN __attribute__((visibility("hidden")))

struct lpvmpc_cascade;       // cascade_api.hip
struct lpvmpc_race;          // race_api.hip
struct DistStep;             // below: the stand-alone step's disturbance arguments
struct WearStep;             // below: the stand-alone step's tyre-wear arguments

using lpvmpc::DevCfg;
using lpvmpc::SolveArgs;

// Owner of device memory: a list of hipMalloc blocks, freed together when the arena is released, assigned over or destroyed.
// The pointers it hands out live in the struct next to it (kernel arguments keep their raw pointers); releasing an owner is
// `x = {}`.  Only init / reserve / setup paths allocate.
struct DevArena {
    std::vector<void *> blocks;
    DevArena() = default;
    DevArena(DevArena &&o) noexcept { blocks.swap(o.blocks); }
    DevArena &operator=(DevArena &&o) noexcept { blocks.swap(o.blocks); o.release(); return *this; }
    ~DevArena() { release(); }
    void release() { for (void *b : blocks) (void)hipFree(b); blocks.clear(); }
    // a failed allocation leaves the arena and p as they were and clears the error HIP keeps pending in the thread (a later
    // launcher would report it through hipGetLastError for a launch that succeeded)
    template <class T> hipError_t alloc(T *&p, size_t bytes) {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); return e; }
        blocks.push_back(q); p = (T *)q;
        return hipSuccess;
    }
};
template <class T> void release(T &x) { x = T{}; }          // release<Workspace>(*h): one owner of a handle

struct ActState { lpvmpc::ActDev d{}; DevArena mem; };          // actuator state of a delayed fleet or race (lpvmpc_act_alloc; d.ring == null: none)
struct PlantTable { lpvmpc::VehPlantCfg d{}; DevArena mem; };   // plant table of a per-vehicle fleet or race (lpvmpc_plant_upload; d.p == null: one PlantCfg)
struct TyreTable { const double *t = nullptr; DevArena mem; };   // tyre table [4][B] next to the plant table (lpvmpc_tyre_upload; t == null: the linear tyre's kernels)
// the tyre forms' kernel argument: the plant table with its tyre table
inline lpvmpc::TyrePlantCfg tyre_plant(const PlantTable &v, const TyreTable &y) { lpvmpc::TyrePlantCfg c; static_cast<lpvmpc::VehPlantCfg &>(c) = v.d; c.t = y.t; return c; }

// plant disturbances of a fleet or race (lpvmpc_set_disturbances, disturbance_api.hip; d.rows null: none attached): the kernel
// argument with its device memory, and on the host the rows as they were set and the base plant / tyre tables [word][B] that the
// read-backs return and a detach restores
struct DistBinding {
    lpvmpc::DistDev d{};
    DevArena mem;
    lpvmpc_disturbance_config cfg{};
    std::vector<double> rows, base_p, base_t;
};

// tyre wear and temperature of a fleet or race (lpvmpc_set_tyre_wear, tyre_wear_api.hip; d.rows null: none attached): the kernel
// argument with its device memory (rows and state live on the device alone: a race's restore and clone move them), and on the host
// the base plant / tyre tables [word][B] as the disturbances' binding keeps them
struct WearBinding {
    lpvmpc::WearDev d{};
    DevArena mem;
    std::vector<double> base_p, base_t;
};

// sensor faults of a fleet or race (lpvmpc_set_sensor_faults, sensor_faults_api.hip; d.rows null: none attached): the faulted kernels'
// argument with its device memory, and on the host the configuration and the rows as they were set, for the read-back
struct FaultBinding {
    lpvmpc::FaultDev d{};
    DevArena mem;
    lpvmpc_sensor_fault_config cfg{};
    std::vector<double> rows;
};

// The plant an engine drives, stored once: a lap-0 fleet (Fleet::cl_side) and a race (lpvmpc_race::side) each hold one, and the
// bindings and read-backs reach the running engine's through lpvmpc_plant_side.  Built in a local with the engine that owns it and
// moved in after the last step that can fail
struct PlantSide {
    int B = 0;                          // fleet size
    lpvmpc::PlantCfg pc{};              // the fleet-wide plant (a race's: n_sub = 1, each vehicle's steps of a tick are RaceDev::nstep)
    int actuated = 0;                   // started by an _actuated call (or _vehicles / _tyres, which take the delayed kernels): actuator state act
    ActState act;
    PlantTable veh;                     // started by a _vehicles call: the plant table
    TyreTable tyre;                     // started by a _tyres call: the tyre table as well
    DistBinding dist;                   // lpvmpc_set_disturbances on that engine (freed with it)
    WearBinding wear;                   // lpvmpc_set_tyre_wear on that engine (freed with it)
    FaultBinding fault;                 // lpvmpc_set_sensor_faults on that engine (freed with it)
    lpvmpc::TyrePlantCfg tpc() const { return tyre_plant(veh, tyre); }
    // the base plant / tyre tables while a binding rewrites the live Cf / Cr / c_f words (null: none does, the live tables are the base)
    const std::vector<double> *base_p() const { return dist.d.rows ? &dist.base_p : wear.d.rows ? &wear.base_p : nullptr; }
    const std::vector<double> *base_t() const { return dist.d.rows ? &dist.base_t : wear.d.rows ? &wear.base_t : nullptr; }
    // the wear kernel's argument of this tick: the binding with the gamma words of the disturbances as they are attached now
    lpvmpc::WearDev wear_arg() const { lpvmpc::WearDev w = wear.d; w.gamma = dist.d.rows ? dist.d.state + 4 * (size_t)B : nullptr; return w; }
};

struct EventRing {                      // ring of event pairs around launches (lpvmpc_set_timing)
    std::vector<hipEvent_t> e0, e1;
    int count = 0;                      // pairs recorded since timing was (re)enabled
    EventRing() = default;
    EventRing(const EventRing &) = delete;
    ~EventRing() { for (hipEvent_t e : e0) if (e) (void)hipEventDestroy(e); for (hipEvent_t e : e1) if (e) (void)hipEventDestroy(e); }
};

// The handle's owners: each is released as a whole and rebuilt in a local before it is installed, so no entry point ever sees half of one.
struct Workspace {                      // device workspace (ensure_ws)
    DevArena ws_mem;
    int cap = 0;                        // capacity (instances)
    double *d_x0 = nullptr, *d_uprev = nullptr, *d_vel = nullptr, *d_curv = nullptr, *d_uold = nullptr, *d_maxey = nullptr, *d_AB = nullptr,
           *d_states = nullptr, *d_xPred = nullptr, *d_uPred = nullptr, *d_resid = nullptr, *d_xlast = nullptr, *d_delta = nullptr;
    double *d_scal = nullptr;           // planner N = 30: the kernel's equilibration vectors [cap][3][8(N+1)] (SolveArgs::scal), else null
    double *d_state = nullptr;          // warm-start state [cap][3][8(N+1)] (opt-in)
    int32_t *d_status = nullptr, *d_iters = nullptr, *d_polish = nullptr;
    int32_t *d_active = nullptr;        // [cap] instance mask of lpvmpc_solve_batch_masked
};
struct Fleet {                          // closed-loop fleet (lpvmpc_cl_*): plant [B][8], local state [B][6], command [B][2] and scratch
    DevArena cl_mem;
    double *cl_plant = nullptr, *cl_local = nullptr, *cl_cmd = nullptr;
    double *cl_local_next = nullptr;    // measurement of the coming tick, made by the launch that advanced the plant (valid: cl_next_valid)
    int cl_next_valid = 0;
    int cl_first_it = 1, cl_q9 = 1, cl_ticks = 0;
    double cl_hw = 0, cl_slack = 0;
    PlantSide cl_side;                  // the plant it drives
};
struct ObsState {                       // the fleet's / cascade's / race's estimator state [obs_B][kObsStride] (null: it runs on ground truth;
    DevArena obs_mem;                   // a race's is set by lpvmpc_race_init_observed without obs_cfg and freed with the race)
    double *obs_state = nullptr;
    int obs_B = 0;
    lpvmpc::ObsParams obs_p{};
};
struct ObsGains { DevArena gains_mem; double *obs_gains = nullptr; };   // device copy of the gain words (head of lpvmpc_observer_config): the fleet's or the batch call's
struct ObsStage { DevArena stage_mem; char *obs_ws = nullptr; int obs_ws_cap = 0; };   // lpvmpc_observer_step_batch staging, obs_ws_cap instances
struct DeferPools {                     // the two pools of parked instances (ensure_defer)
    DevArena defer_mem;
    double *dpool[2] = {nullptr, nullptr};
    int32_t *dcount[2] = {nullptr, nullptr};
    int defer_cur_cap = 0, defer_stride = 0;
};
struct Handoff {                        // planner -> controller hand-off operators (lpvmpc_handoff_setup, planner handles): [M][N] row-major each
    DevArena ho_mem;
    double *d_Wop = nullptr, *d_FWop = nullptr;
    int ho_M = 0;
};
struct ModelTable {                     // per-vehicle model parameters (lpvmpc_set_model_params, model_params_api.hip): the table [kModelWords][model_B] that
    DevArena model_mem;                 // every LPV / ABC launch of this handle takes (lpvmpc::launch_lpv / launch_abc), null: the handle's own vehicle words
    double *d_model = nullptr;
    int model_B = 0;
};
struct TuneTable {                      // per-vehicle tunings (lpvmpc_set_tunings, tunings_api.hip): the device rows [tune_B][kTuneWords], instance-major, that
    DevArena tune_mem;                  // every main solve launch of this handle takes (SolveArgs::tune, lpvmpc_solve_tune), null: the configuration's own
    double *d_tune = nullptr;           // words; the public rows as they were set stay on the host for the read-back
    int tune_B = 0;
    std::vector<double> tune_rows;
};
struct ObsVehTable {                    // per-vehicle estimator (lpvmpc_set_observer_vehicles, observer_design_api.hip): the model rows [kPlantWords][ov_B] and
    DevArena ov_mem;                    // the gain planes [2][kObsTable][ov_B] that the estimator kernels of a fleet or race started by the _vehicles / _tyres
    lpvmpc::ObsVehDev ov{};             // calls take (ov.L null: the configuration's tables and the observer's own constants)
    int ov_B = 0;
    bool ov_designed = false;           // the tables were designed on the device, on the limit tables ov_lim (LS, HS)
    double ov_lim[24] = {};
};
struct TrackTable {                     // per-vehicle tracks (lpvmpc_set_tracks, tracks_api.hip): the palette and the index per vehicle on the device (trk,
    DevArena trk_mem;                   // the bound kernels' argument; trk.tab null: the configuration's own table), the table [kModelWords][trk.B] of the handle's
    lpvmpc::TrackDev trk{};             // own vehicle words that the bound LPV / ABC kernels read on a handle without model rows, and the binding as it was
    double *d_trk_model = nullptr;      // set, on the host, for the read-back and the comparison of a race's three bindings
    std::vector<int32_t> trk_rows, trk_of;
    std::vector<double> trk_tables, trk_hw, trk_slack;
};

struct lpvmpc_handle : Workspace, Fleet, ObsState, ObsGains, ObsStage, DeferPools, Handoff, ModelTable, TuneTable, ObsVehTable, TrackTable {
    lpvmpc_config cfg{};
    DevCfg dev{};
    DevArena mem;                       // what lives as long as the handle: d_cfg, dstats, the device staging buffers
    DevCfg *d_cfg = nullptr;            // device copy of dev (kernels read the configuration through this pointer)
    int nx = 0, nb = 0;
    int warm_mode = 0, state_valid_B = 0;   // 0 off (default); instances whose state is valid from the previous solve
    hipStream_t stream = nullptr;
    EventRing ev;                       // around the solve-kernel launches
    bool timing = false;
    int force_generic = 0;              // 1: always use the run-time-horizon kernel (validation)
    double last_ms = -1.0;
    std::string err;
    // small-batch I/O staging (lpvmpc_api.hip, IoPack): one pinned host buffer and one device buffer per direction
    char *h_pack_in = nullptr, *h_pack_out = nullptr, *d_pack_in = nullptr, *d_pack_out = nullptr;
    // straggler deferral (options "defer_after" / "defer_budget" / "defer_pool", lpvmpc_solve_batch_dev only): two pools of
    // parked instances used alternately -- with defer_budget > 0 a call's main launch continues the entries of pool[dcur] in its
    // rider workgroups and parks, riders and new instances alike, into the other pool, which becomes dcur; otherwise launches park
    // into pool[dcur] and a resume pass (lpvmpc_join; budget 0: behind every call) runs its entries to completion
    int defer_after = 0, defer_budget = 200, defer_cap = 0;   // iterations before parking (0 = off); iterations a rider continues for (0 / -1: see lpvmpc.h); pool entries (0 = default)
    int defer_tail = 1;                 // option "defer_tail" (default 1): passes that run to completion take the whole-CU tail kernel
    bool defer_skip_pass = false;       // transient: the synchronous entry point joins at once, no riders and no pass in between
    unsigned long long *dstats = nullptr;   // [2] device counters: instances parked / parking requests refused (lpvmpc_defer_stats), kept when the pools are rebuilt
    int dcur = 0;
    hipStream_t defer_stream = nullptr; // stream of the last deferred call (lpvmpc_join orders against it); valid iff defer_stream_set
    bool defer_stream_set = false;      // (the null stream is a stream like any other: nullptr cannot mean "none yet")
    hipEvent_t defer_event = nullptr;
    EventRing rv;                       // around the resume launches
    int cascade_prefetch = 1;           // option "cascade_prefetch" (default 1)
    lpvmpc_cascade *cascade = nullptr;  // owned by the controller handle of a cascade (lpvmpc_cascade_init)
    lpvmpc_handle *cascade_owner = nullptr;   // planner handle: the controller handle whose cascade drives it (its workspace carries the planner recursion)
    lpvmpc_race *race = nullptr;        // owned by the path controller handle of a race (lpvmpc_race_init)
    lpvmpc_handle *race_owner = nullptr;      // trajectory-tracking / planner handle of a race: the path handle that owns it
    const int32_t *solve_mask = nullptr;      // transient: the mask lpvmpc_launch_solve_timed puts on the launches of a masked call
    // gain-scheduled LPV estimator (lpvmpc_observer_*, observer.hip)
    std::unique_ptr<lpvmpc_observer_config> obs_cfg;   // set by lpvmpc_observer_setup, taken by the next lpvmpc_cl_init (null: no estimator)
    // lpvmpc_destroy synchronises the device and ends the engines that link handles before it deletes the handle
    ~lpvmpc_handle() {
        if (h_pack_in) (void)hipHostFree(h_pack_in);
        if (h_pack_out) (void)hipHostFree(h_pack_out);
        if (defer_event) (void)hipEventDestroy(defer_event);
    }
};

// the handle runs a fleet, cascade or race whose state lives in its workspace: no batch call, no second engine
inline bool busy(const lpvmpc_handle *x) { return x->cl_plant || x->cascade || x->cascade_owner || x->race || x->race_owner; }

LPVMPC_HIDDEN int lpvmpc_fail(lpvmpc_handle *h, int code, const char *fmt, ...);
#define fail lpvmpc_fail
#define HIP_TRY(h, expr)                                                                            \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return fail(h, LPVMPC_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)


#define H2D(dst, src, n) HIP_TRY(h, hipMemcpyAsync(dst, src, (n), hipMemcpyHostToDevice, st))
#define D2H(dst, src, n) HIP_TRY(h, hipMemcpyAsync(dst, src, (n), hipMemcpyDeviceToHost, st))

// helpers defined in lpvmpc_api.hip
LPVMPC_HIDDEN int lpvmpc_need_track(lpvmpc_handle *h, const char *who);
LPVMPC_HIDDEN int lpvmpc_check_common(lpvmpc_handle *h, int B, const char *who);       // validates, selects the device, sizes the workspace
LPVMPC_HIDDEN int lpvmpc_check_batch(lpvmpc_handle *h, int B, const char *who);        // the same for the stand-alone batch calls: refused while the handle runs a fleet
LPVMPC_HIDDEN int lpvmpc_launch_solve_timed(lpvmpc_handle *h, const lpvmpc::SolveArgs &a, hipStream_t st);
// the same with the handle's warm start (option "warm_start"): fills a.state / a.warm and, once launched, marks the state of a.B instances valid
LPVMPC_HIDDEN int lpvmpc_launch_solve_warm(lpvmpc_handle *h, lpvmpc::SolveArgs a, hipStream_t st);
LPVMPC_HIDDEN lpvmpc::PlantCfg lpvmpc_plant_cfg(const lpvmpc_handle *h, int n_sub, double dt_sim, double mu_sim);
LPVMPC_HIDDEN void lpvmpc_cascade_free(lpvmpc_handle *h);
LPVMPC_HIDDEN void lpvmpc_race_free(lpvmpc_handle *h);                                  // race_api.hip
// race_api.hip: the inventory of the running race's per-vehicle state (include/lpvmpc.h, "Race snapshot, restore and clone"), the one
// table that lpvmpc_race_snapshot / _restore / _clone (race_state_api.hip) walk.  An array is in it if a tick can read a word of it
// that an earlier tick, or the init, wrote; bindings and tables, scratch that a tick writes before it reads, and the recorder are not.
// type / layout: lpvmpc::StateType / StateLayout (race_state.hpp).  false: the handle owns no race
struct RaceStateDesc { char name[16]; void *ptr; int32_t type, W, layout; };
struct RaceState {
    int32_t shape[8] = {};                      // B, N, Np, M, sd, lap_cols, laps, ticks
    uint32_t features = 0;                      // LPVMPC_SNAP_HAS_*
    bool recording = false;                     // a recorder is attached (lpvmpc_race_record)
    bool heats = false;                         // heats are attached (lpvmpc_race_heats)
    bool events = false;                        // an event log is attached (lpvmpc_race_events)
    const std::vector<int32_t> *track_of = nullptr;   // [B] with tracks bound, else null
    std::vector<RaceStateDesc> tab;
};
LPVMPC_HIDDEN bool lpvmpc_race_state(lpvmpc_handle *h, RaceState &s);
LPVMPC_HIDDEN void lpvmpc_race_set_ticks(lpvmpc_handle *h, int ticks);
// race_api.hip: the caller's mu words [B] (plant row word 6) while interactions are attached to the race that h owns
// (lpvmpc_race_interactions rewrites the live words), else null: what a base copy of the live plant table takes in their place
LPVMPC_HIDDEN const std::vector<double> *lpvmpc_race_mu_base(lpvmpc_handle *h);
LPVMPC_HIDDEN int lpvmpc_observer_start(lpvmpc_handle *h, const lpvmpc_observer_config &o, int B, const double *plant0, double dt_sim,
                                        int from_plant);                                // lpvmpc_api.hip
// actuator_api.hip: checks cfg / per-vehicle delays and allocates a zeroed actuator state for B vehicles in a (released first)
LPVMPC_HIDDEN int lpvmpc_act_alloc(lpvmpc_handle *h, int B, const lpvmpc_actuator_config *cfg, const int32_t *delay_a, const int32_t *delay_df,
                                   double dt_sim, const char *who, ActState &a);
LPVMPC_HIDDEN int lpvmpc_act_download(lpvmpc_handle *h, const lpvmpc::ActDev &a, double *act_state, hipStream_t st);   // device -> host layout
LPVMPC_HIDDEN int lpvmpc_observer_check(lpvmpc_handle *h, const lpvmpc_observer_config *c, const char *who);   // lpvmpc_api.hip
// plant_params_api.hip: per-vehicle plant parameters (lpvmpc_*_vehicles).  lpvmpc_plant_rows checks the host rows [B][7] (null: the
// nominal row lf, lr, m, Iz, 60, 60, mu for every vehicle) and returns the device layout [7][B] in t; nothing is allocated.
// lpvmpc_plant_upload allocates and fills the fleet's table in v, released first (synchronises)
LPVMPC_HIDDEN int lpvmpc_plant_rows(lpvmpc_handle *h, int B, const double *rows, const lpvmpc_config &nominal, double mu, const char *who,
                                    std::vector<double> &t);
LPVMPC_HIDDEN int lpvmpc_plant_upload(lpvmpc_handle *h, int B, const std::vector<double> &t, double dt_sim, int n_sub, PlantTable &v);
// race_api.hip: the plant side of the engine that h runs -- the race's (*race: its RaceDev), else the lap-0 fleet's (*race null), else
// null -- and the engine's step form (step_form.hpp); lpvmpc_race_dist: what a race's disturbances act on
LPVMPC_HIDDEN PlantSide *lpvmpc_plant_side(lpvmpc_handle *h, const lpvmpc::RaceDev **race = nullptr);
LPVMPC_HIDDEN lpvmpc::DistDev lpvmpc_race_dist(const PlantSide &p, const lpvmpc::RaceDev &d);
inline lpvmpc::StepForm lpvmpc_step_form(const lpvmpc_handle *h, const PlantSide &p, const lpvmpc::RaceDev *race) {
    return lpvmpc::step_form(p.actuated, p.veh.d.p, p.tyre.t, race ? race->estv != nullptr : h->obs_state != nullptr, h->ov.L, h->trk.tab, p.fault.d.rows);
}
// lpvmpc_plant_step_vehicles_batch with the checked tyre table [4][B] of tyre_api.hip (null: the per-vehicle forms' kernel)
LPVMPC_HIDDEN int lpvmpc_plant_step_rows(lpvmpc_handle *h, int32_t B, double *state, double *act_state, const double *u, int32_t n_sub, double dt_sim,
                                         double mu_sim, const lpvmpc_actuator_config *act, const int32_t *delay_a, const int32_t *delay_df,
                                         const double *plant_params, const std::vector<double> *tyre, const char *who,
                                         const DistStep *dist = nullptr, const WearStep *wear = nullptr);
// tyre_api.hip: tyre rows (lpvmpc_*_tyres).  lpvmpc_tyre_rows checks the host rows [B][4] (null: kind 0 for every vehicle) and returns
// the device layout [4][B] in t; nothing is allocated.  lpvmpc_tyre_upload allocates and fills the table in y, released first (synchronises)
LPVMPC_HIDDEN int lpvmpc_tyre_rows(lpvmpc_handle *h, int B, const double *rows, const char *who, std::vector<double> &t);
LPVMPC_HIDDEN int lpvmpc_tyre_upload(lpvmpc_handle *h, const std::vector<double> &t, TyreTable &y);
// the fleet / race starts shared by the _vehicles and _tyres entry points (lpvmpc_api.hip, race_api.hip); tyre_params: see lpvmpc_tyre_rows,
// tyres false: the _vehicles call
LPVMPC_HIDDEN int lpvmpc_cl_init_rows(lpvmpc_handle *h, int32_t B, const double *plant0, double half_width, double slack, int32_t q9_swap,
                                      int32_t n_sub, double dt_sim, double mu_sim, const lpvmpc_actuator_config *act, const int32_t *delay_a,
                                      const int32_t *delay_df, const double *plant_params, bool tyres, const double *tyre_params);
LPVMPC_HIDDEN int lpvmpc_race_init_rows(lpvmpc_handle *h, lpvmpc_handle *tt, lpvmpc_handle *plan, int32_t B, const double *plant0,
                                        const int32_t *half_track0, const lpvmpc_race_config *cfg, const lpvmpc_observer_config *obs,
                                        const lpvmpc_actuator_config *act, const int32_t *delay_a, const int32_t *delay_df,
                                        const double *plant_params, bool tyres, const double *tyre_params);
// disturbance_api.hip: plant disturbances.  lpvmpc_dist_rows checks cfg and the host rows [B][LPVMPC_DIST_WORDS] against each vehicle's lap length and returns the device
// layout [LPVMPC_DIST_WORDS + 1][B] in t.  lpvmpc_dist_step: the stand-alone step's launch in front of its plant kernel, on tables
// that live in mem; dist_state [B][LPVMPC_DIST_STATE] in (null: fresh), lpvmpc_dist_step_read copies it out after the step
struct DistStep { const lpvmpc_disturbance_config *cfg; const double *rows; double *dist_state; };
LPVMPC_HIDDEN int lpvmpc_dist_rows(lpvmpc_handle *h, int B, const lpvmpc_disturbance_config *cfg, const double *rows, const char *who,
                                   std::vector<double> &t);
LPVMPC_HIDDEN int lpvmpc_dist_step(lpvmpc_handle *h, int B, const DistStep &ds, const std::vector<double> &rows_dev, const std::vector<double> &plant_tab,
                                   const std::vector<double> &tyre_tab, double *d_plant, const int32_t *d_k, int n_sub, double dt_sim,
                                   double *live_p, double *live_t, DistBinding &tmp, hipStream_t st);
LPVMPC_HIDDEN int lpvmpc_dist_step_read(lpvmpc_handle *h, int B, const DistStep &ds, const DistBinding &tmp, hipStream_t st);
// the base tables [word][B] of the engine that h runs, for a binding that is about to rewrite live words: the copy another binding
// keeps (PlantSide::base_p), else the live tables themselves with the caller's mu words (synchronises)
LPVMPC_HIDDEN int lpvmpc_plant_base(lpvmpc_handle *h, const PlantSide &side, std::vector<double> &base_p, std::vector<double> &base_t, hipStream_t st);
// tyre_wear_api.hip: tyre wear and temperature.  lpvmpc_wear_rows checks the host rows [B][LPVMPC_WEAR_WORDS] against the Euler step's
// bound k_cool * n_max * dt_sim < 1 and returns the device layout [LPVMPC_WEAR_WORDS][B] in t.  lpvmpc_wear_step: the stand-alone step's
// launch behind the disturbances' (gamma: their word of this tick, or null) and in front of its plant kernel, on tables that live in
// tmp; wear_state [B][LPVMPC_WEAR_STATE] in (null: fresh), lpvmpc_wear_step_read copies it out after the step
struct WearStep { const double *rows; double *wear_state; };
LPVMPC_HIDDEN int lpvmpc_wear_rows(lpvmpc_handle *h, int B, const double *rows, int n_max, double dt_sim, const char *who, std::vector<double> &t);
LPVMPC_HIDDEN int lpvmpc_wear_step(lpvmpc_handle *h, int B, const WearStep &ws, const std::vector<double> &rows_dev, const std::vector<double> &plant_tab,
                                   const std::vector<double> &tyre_tab, const double *d_plant, const double *gamma, int n_sub, double dt_sim,
                                   double *live_p, double *live_t, WearBinding &tmp, hipStream_t st);
LPVMPC_HIDDEN int lpvmpc_wear_step_read(lpvmpc_handle *h, int B, const WearStep &ws, const WearBinding &tmp, hipStream_t st);
// model_params_api.hip: lpvmpc_model_check refuses a batch size other than that of the handle's bound model rows (unbound: any);
// called by every entry point that linearises, before anything is launched
LPVMPC_HIDDEN int lpvmpc_model_check(lpvmpc_handle *h, int B, const char *who);
// tracks_api.hip: lpvmpc_tracks_check refuses a batch size other than that of the handle's track binding (unbound: any); called by every
// entry point the binding acts on, before anything is launched.  lpvmpc_tracks_unbound refuses a bound handle on an entry point the
// binding does not act on; general: the entry point that starts the same engine on a bound handle (null: none does).  lpvmpc_trk:
// the `trk` argument of lpvmpc::launch_lpv / launch_abc (null: unbound)
LPVMPC_HIDDEN int lpvmpc_tracks_check(lpvmpc_handle *h, int B, const char *who);
LPVMPC_HIDDEN int lpvmpc_tracks_unbound(lpvmpc_handle *h, const lpvmpc_handle *bound, const char *who, const char *general = nullptr);
// the two handles carry the same binding (a race's three handles must)
inline bool lpvmpc_tracks_equal(const lpvmpc_handle *a, const lpvmpc_handle *b) {
    return a->trk.T == b->trk.T && a->trk.B == b->trk.B && a->trk_rows == b->trk_rows && a->trk_of == b->trk_of && a->trk_tables == b->trk_tables &&
           a->trk_hw == b->trk_hw && a->trk_slack == b->trk_slack;
}
inline const lpvmpc::TrackDev *lpvmpc_trk(const lpvmpc_handle *h) { return h->trk.tab ? &h->trk : nullptr; }
// tunings_api.hip: lpvmpc_tuning_check refuses a batch size other than that of the handle's bound tuning rows (unbound: any);
// called by every entry point that solves, before anything is launched.  lpvmpc_solve_tune fills SolveArgs::tune of a launch that
// sets instances up (main launches, with or without riders; a resume pass reads no row) and refuses one the table does not cover
LPVMPC_HIDDEN int lpvmpc_tuning_check(lpvmpc_handle *h, int B, const char *who);
LPVMPC_HIDDEN int lpvmpc_solve_tune(lpvmpc_handle *h, lpvmpc::SolveArgs &a);
// observer_design_api.hip: lpvmpc_observer_vehicles_check is called by every engine start with an estimator (obs non-null).  honoured: the
// start runs the per-vehicle forms' kernels (the _vehicles / _tyres calls).  It refuses a bound handle on a start that does not honour
// the binding, another B than the binding's, and a designed binding whose limit tables differ from the estimator configuration's.
// lpvmpc_observer_vehicles_gains: the `gains` argument of the bound estimator kernels
LPVMPC_HIDDEN int lpvmpc_observer_vehicles_check(lpvmpc_handle *h, int B, const lpvmpc_observer_config *obs, bool honoured, const char *who);
inline lpvmpc::ObsVehGains lpvmpc_observer_vehicles_gains(const lpvmpc_handle *h) { lpvmpc::ObsVehGains g; static_cast<lpvmpc::ObsVehDev &>(g) = h->ov; g.g = h->obs_gains; return g; }
namespace lpvmpc {
// handoff.hip (host): interpolation operator W and interpolation + filtfilt operator FW, both [M][N] row-major
bool handoff_operators(int N, double dt, double interp_dt, int padlen, int ord, const double *b, const double *a,
                       std::vector<double> &W, std::vector<double> &FW);
}
