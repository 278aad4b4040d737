// race_api.hip -- C ABI of the race engine (include/lpvmpc.h, lpvmpc_race_*): lap 0, per-vehicle lap events and racing
// for one fleet on the device, owned by the path controller handle.  Kernels: race.hip (per-tick glue), lpv_eval.hip,
// admm_solve.hip and handoff.hip (masked launches).  A race with the estimator in the loop (lpvmpc_race_init_observed) keeps
// the estimator state, gains and parameters in the path handle's obs_state / obs_gains / obs_p (obs_cfg stays null, so the
// handle's next lpvmpc_cl_init runs on ground truth); lpvmpc_race_free releases them.  The recorder (lpvmpc_race_record,
// record.hip), the heats (lpvmpc_race_heats, heats_api.hip / heats.hip), the interactions (lpvmpc_race_interactions,
// interactions_api.hip / interactions.hip), the contact model (lpvmpc_race_contact, contact_api.hip / contact.hip), the walls
// (lpvmpc_race_walls, walls_api.hip / walls.hip) and the event log (lpvmpc_race_events, events_api.hip / events.hip) belong to the
// race as well.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "contact_host.hpp"
#include "events_host.hpp"
#include "race_state.hpp"
#include "record.hpp"
#include "walls_host.hpp"

struct lpvmpc_race_recorder {
    lpvmpc::RecDev d{};           // kernel argument: race state pointers and the recorder's buffers
    DevArena mem;                 // the recorder's buffers
    int capacity = 0, stride = 0, t_start = 0, total = 0;
};

struct lpvmpc_race {
    lpvmpc_handle *tt = nullptr, *plan = nullptr;
    lpvmpc::RaceDev d{};          // device pointers and constants (kernel argument)
    DevArena mem;                 // the race's own buffers of d (the p_ / t_ / q_ pointers are the three handles' workspaces)
    int ticks = 0;
    PlantSide side;               // the plant it drives (side.actuated: the controllers keep histories of steering delay sd)
    int sd = 0;
    std::unique_ptr<lpvmpc_race_recorder> rec;   // lpvmpc_race_record (null: not recording)
    std::unique_ptr<HeatsBinding> heats;         // lpvmpc_race_heats (heats_api.hip; null: none attached)
    std::unique_ptr<InterBinding> inter;         // lpvmpc_race_interactions (interactions_api.hip; null: none attached; reads the heats' lists)
    std::unique_ptr<ContactBinding> contact;     // lpvmpc_race_contact (contact_api.hip; null: the centres form; reads the interactions' binding)
    std::unique_ptr<WallBinding> walls;          // lpvmpc_race_walls (walls_api.hip; null: none attached)
    std::unique_ptr<EventBinding> events;        // lpvmpc_race_events (events_api.hip; null: none attached; reads no binding)
    uint32_t heats_serial = 0, walls_serial = 0; // bumped wherever that slot's binding is installed or detached: the log's first sight
};

void lpvmpc_race_free(lpvmpc_handle *h) {
    lpvmpc_race *r = h->race;
    if (!r) return;
    (void)hipSetDevice(h->cfg.device);
    (void)hipStreamSynchronize(h->stream);
    if (r->d.estv) { release<ObsState>(*h); release<ObsGains>(*h); }   // the race's estimator
    if (r->tt->race_owner == h) r->tt->race_owner = nullptr;
    if (r->plan->race_owner == h) r->plan->race_owner = nullptr;
    delete r;
    h->race = nullptr;
}

extern "C" void lpvmpc_race_default_config(lpvmpc_race_config *c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->laps = 1;
    c->n_sub_lap0 = 7;                                          // 7 x 5 ms per 33 ms tick (tests/golden/make_golden.py section 2)
    c->n_sub[0] = 7; c->n_sub[1] = 7; c->n_sub[2] = 6;          // 100 ms per three racing ticks
    c->q9_swap = 1;
    c->half_width = 0.3; c->slack = 0.15; c->plan_max_ey = 0.2; c->dt_sim = 0.005; c->mu_sim = 0.05;
}

static int race_init(lpvmpc_handle *h, lpvmpc_handle *tt, lpvmpc_handle *plan, int32_t B, const double *plant0, const int32_t *half_track0,
                     const lpvmpc_race_config *cfg, const lpvmpc_observer_config *obs, bool observed_call,
                     const lpvmpc_actuator_config *act = nullptr, const int32_t *delay_a = nullptr, const int32_t *delay_df = nullptr,
                     const std::vector<double> *veh = nullptr, const std::vector<double> *tyre = nullptr) {
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "lpvmpc_race_init: path handle is NULL");
    if (!tt || !plan || !plant0 || !cfg || B <= 0) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init: NULL argument or B <= 0");
    if (h->cfg.kind != LPVMPC_KIND_CONTROLLER || tt->cfg.kind != LPVMPC_KIND_CONTROLLER || plan->cfg.kind != LPVMPC_KIND_PLANNER || h == tt)
        return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init: needs two controller handles (path, tt) and a planner handle");
    if (h->cfg.device != tt->cfg.device || h->cfg.device != plan->cfg.device)
        return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init: the three handles live on different devices");
    // per-vehicle tracks (lpvmpc_set_tracks): all three handles carry equal bindings, or none does; equal bindings replace the
    // comparison of the handles' own tables
    const int n_bound = (h->trk.tab != nullptr) + (tt->trk.tab != nullptr) + (plan->trk.tab != nullptr);
    if (n_bound != 0 && n_bound != 3)
        return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init: %d of the three handles have per-vehicle tracks bound (lpvmpc_set_tracks); bind path, tt and "
                    "planner with equal bindings, or none", n_bound);
    if (n_bound == 3 && !tyre)
        return lpvmpc_tracks_unbound(h, h, veh ? "lpvmpc_race_init_vehicles" : act ? "lpvmpc_race_init_actuated" : observed_call ? "lpvmpc_race_init_observed" : "lpvmpc_race_init",
                                     "lpvmpc_race_init_tyres");
    if (n_bound == 3 && (!lpvmpc_tracks_equal(h, tt) || !lpvmpc_tracks_equal(h, plan)))
        return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init_tyres: the track bindings (lpvmpc_set_tracks) of path, tt and planner differ in T, B, tables, "
                    "widths, slacks or track_of");
    if (h->cfg.N != tt->cfg.N || h->cfg.dt != tt->cfg.dt ||
        (n_bound == 0 && (h->cfg.track_rows != tt->cfg.track_rows || std::memcmp(h->cfg.track, tt->cfg.track, sizeof(double) * 6 * h->cfg.track_rows) != 0)))
        return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init: path and tt handles differ in N, dt or track");
    if (h->cfg.N > 20) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init: the reference's seed trajectories have 20 rows (N <= 20)");
    if ((h->cfg.steering_delay != 0 || tt->cfg.steering_delay != 0) && !act)
        return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init: the fleet engines run the reference's steeringDelay = 0 (CMAIN:49); lpvmpc_race_init_actuated runs delayed controllers");
    if (act && h->cfg.steering_delay != tt->cfg.steering_delay)
        return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init_actuated: path and tt handles differ in steeringDelay (%d, %d)", h->cfg.steering_delay, tt->cfg.steering_delay);
    if (!plan->d_Wop) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init: call lpvmpc_handoff_setup on the planner handle first");
    if (plan->ho_M < h->cfg.N) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init: the planner message (%d samples) is shorter than the controller horizon", plan->ho_M);
    if (h->warm_mode || tt->warm_mode || plan->warm_mode) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init: warm_start must be 0 on all three handles");
    if (h->obs_cfg && !observed_call) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init: the race does not run the state estimator (remove it from the path handle)");
    if (h->obs_cfg) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init_observed: the race's estimator is configured through the obs argument; "
                                                 "remove the one lpvmpc_observer_setup attached to the path handle");
    if (busy(h) || busy(tt) || busy(plan)) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init: a handle already runs a fleet, cascade or race (lpvmpc_cl_release ends it)");
    if (cfg->laps < 1 || cfg->n_sub_lap0 < 1 || cfg->n_sub[0] < 1 || cfg->n_sub[1] < 1 || cfg->n_sub[2] < 1 || !(cfg->dt_sim > 0))
        return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init: bad configuration (laps >= 1, step counts >= 1, dt_sim > 0)");
    int rc;
    if (obs) { rc = lpvmpc_observer_check(h, obs, "lpvmpc_race_init_observed"); if (rc) return rc; }
    if (obs) { rc = lpvmpc_observer_vehicles_check(h, B, obs, veh != nullptr, "lpvmpc_race_init"); if (rc) return rc; }
    rc = lpvmpc_need_track(h, "lpvmpc_race_init"); if (rc) return rc;
    rc = lpvmpc_need_track(plan, "lpvmpc_race_init(planner)"); if (rc) return fail(h, rc, "%s", lpvmpc_last_error(plan));
    rc = lpvmpc_check_common(h, B, "lpvmpc_race_init"); if (rc) return rc;
    rc = lpvmpc_check_common(tt, B, "lpvmpc_race_init(tt)"); if (rc) return fail(h, rc, "%s", lpvmpc_last_error(tt));
    rc = lpvmpc_check_common(plan, B, "lpvmpc_race_init(planner)"); if (rc) return fail(h, rc, "%s", lpvmpc_last_error(plan));
    rc = lpvmpc_tracks_check(h, B, "lpvmpc_race_init_tyres"); if (rc) return rc;      // (equal bindings: one check covers the three)
    rc = lpvmpc_model_check(h, B, "lpvmpc_race_init"); if (rc) return rc;
    rc = lpvmpc_model_check(tt, B, "lpvmpc_race_init(tt)"); if (rc) return fail(h, rc, "%s", lpvmpc_last_error(tt));
    rc = lpvmpc_model_check(plan, B, "lpvmpc_race_init(planner)"); if (rc) return fail(h, rc, "%s", lpvmpc_last_error(plan));
    rc = lpvmpc_tuning_check(h, B, "lpvmpc_race_init"); if (rc) return rc;
    rc = lpvmpc_tuning_check(tt, B, "lpvmpc_race_init(tt)"); if (rc) return fail(h, rc, "%s", lpvmpc_last_error(tt));
    rc = lpvmpc_tuning_check(plan, B, "lpvmpc_race_init(planner)"); if (rc) return fail(h, rc, "%s", lpvmpc_last_error(plan));
    // the race is built in r and installed in the three handles after the last step that can fail: a failed call leaves them idle
    std::unique_ptr<lpvmpc_race> r(new (std::nothrow) lpvmpc_race());
    if (!r) return fail(h, LPVMPC_E_NOMEM, "out of host memory");
    if (act) { rc = lpvmpc_act_alloc(h, B, act, delay_a, delay_df, cfg->dt_sim, veh ? "lpvmpc_race_init_vehicles" : "lpvmpc_race_init_actuated", r->side.act); if (rc) return rc; }
    if (veh) { rc = lpvmpc_plant_upload(h, B, *veh, cfg->dt_sim, 1, r->side.veh); if (rc) return rc; }
    if (tyre) { rc = lpvmpc_tyre_upload(h, *tyre, r->side.tyre); if (rc) return rc; }
    r->tt = tt; r->plan = plan;
    r->side.B = B; r->side.actuated = act != nullptr; r->sd = h->cfg.steering_delay;
    r->side.pc = lpvmpc_plant_cfg(h, 1, cfg->dt_sim, cfg->mu_sim);
    lpvmpc::RaceDev &d = r->d;
    const size_t b = B, N = h->cfg.N, Np = plan->cfg.N, M = plan->ho_M;
    d.B = B; d.N = (int)N; d.Np = (int)Np; d.M = (int)M; d.laps = cfg->laps; d.q9 = cfg->q9_swap != 0; d.n_sub_lap0 = cfg->n_sub_lap0;
    for (int i = 0; i < 3; ++i) d.n_sub[i] = cfg->n_sub[i];
    d.lap_cols = cfg->laps + 2; d.hw = cfg->half_width; d.slack = cfg->slack;
#define ALLOC(p, n) HIP_TRY(h, r->mem.alloc(p, (n)))
    ALLOC(d.plant, b * 8 * 8); ALLOC(d.cmd, b * 2 * 8); ALLOC(d.local, b * 6 * 8);
    ALLOC(d.phase, b * 4); ALLOC(d.lap, b * 4); ALLOC(d.half, b * 4); ALLOC(d.rk, b * 4); ALLOC(d.plan_done, b * 4); ALLOC(d.idx, b * 4);
    ALLOC(d.nstep, b * 4); ALLOC(d.src, b * 4); ALLOC(d.step, b * 4); ALLOC(d.lap_step, b * d.lap_cols * 4); ALLOC(d.alive, b * 4);
    ALLOC(d.iters, b * 4); ALLOC(d.status, b * 4);
    ALLOC(d.m_path, b * 4); ALLOC(d.m_tt, b * 4); ALLOC(d.m_plan, b * 4); ALLOC(d.m_pfirst, b * 4); ALLOC(d.m_pcont, b * 4);
    ALLOC(d.SSc, b * 8); ALLOC(d.ref0, b * 3 * 8); ALLOC(d.refs, b * 5 * M * 8);
    ALLOC(d.SSp, b * (Np + 1) * 8); ALLOC(d.pose, b * 3 * 8); ALLOC(d.sig, b * 5 * Np * 8);
#undef ALLOC
    d.meas = d.plant;
    d.p_uold = h->d_uold; d.p_uPred = h->d_uPred; d.p_vel = h->d_vel; d.p_curv = h->d_curv; d.p_iters = h->d_iters; d.p_status = h->d_status;
    d.t_uold = tt->d_uold; d.t_uPred = tt->d_uPred; d.t_vel = tt->d_vel; d.t_curv = tt->d_curv; d.t_iters = tt->d_iters; d.t_status = tt->d_status;
    d.q_x0 = plan->d_x0; d.q_xPred = plan->d_xPred; d.q_xlast = plan->d_xlast; d.q_delta = plan->d_delta;
    hipStream_t st = h->stream;
    H2D(d.plant, plant0, b * 8 * 8);
    std::vector<int32_t> half(b, 0), lap_step(b * d.lap_cols, -1);
    if (half_track0) for (size_t i = 0; i < b; ++i) half[i] = half_track0[i] != 0;
    for (size_t i = 0; i < b; ++i) lap_step[i * d.lap_cols] = 0;                       // lap 0 starts at step 0
    H2D(d.half, half.data(), b * 4);
    H2D(d.lap_step, lap_step.data(), lap_step.size() * 4);
    int32_t *zero_i[] = {d.phase, d.lap, d.rk, d.plan_done, d.idx, d.nstep, d.step, d.alive, d.iters, d.status, d.m_path, d.m_tt, d.m_plan, d.m_pfirst, d.m_pcont};
    for (int32_t *p : zero_i) HIP_TRY(h, hipMemsetAsync(p, 0, b * 4, st));
    HIP_TRY(h, hipMemsetAsync(d.src, 0xff, b * 4, st));
    HIP_TRY(h, hipMemsetAsync(d.cmd, 0, b * 2 * 8, st));                                 // servo = motor = 0 before the first tick
    HIP_TRY(h, hipMemsetAsync(d.local, 0, b * 6 * 8, st));
    HIP_TRY(h, hipMemsetAsync(d.SSc, 0, b * 8, st));
    HIP_TRY(h, hipMemsetAsync(d.ref0, 0, b * 3 * 8, st));
    HIP_TRY(h, hipMemsetAsync(d.SSp, 0, b * (Np + 1) * 8, st));
    HIP_TRY(h, hipMemsetAsync(d.pose, 0, b * 3 * 8, st));
    // the handles' carried rows: commands and predictions start at zero, lap-0 references vel_ref = ones (CMAIN:311,326)
    const size_t nu = 2 + r->sd;                                                           // u_old [B][2 + steering_delay]
    HIP_TRY(h, hipMemsetAsync(h->d_uold, 0, b * nu * 8, st)); HIP_TRY(h, hipMemsetAsync(tt->d_uold, 0, b * nu * 8, st));
    HIP_TRY(h, hipMemsetAsync(h->d_uPred, 0, b * N * 2 * 8, st)); HIP_TRY(h, hipMemsetAsync(tt->d_uPred, 0, b * N * 2 * 8, st));
    HIP_TRY(h, hipMemsetAsync(plan->d_uPred, 0, b * Np * 2 * 8, st));
    HIP_TRY(h, hipMemsetAsync(tt->d_curv, 0, b * (N + 1) * 8, st));
    // the solves' iteration counts, statuses and polish flags are carried rows too (a masked launch leaves the rows of the vehicles it
    // does not run): 0 until a vehicle's controller or planner has solved, whatever the workspace held when it was allocated
    for (lpvmpc_handle *e : {h, tt, plan})
        for (int32_t *p : {e->d_iters, e->d_status, e->d_polish}) HIP_TRY(h, hipMemsetAsync(p, 0, b * 4, st));
    std::vector<double> ones(b * (N + 1), 1.0), mey(b, cfg->plan_max_ey);
    H2D(h->d_vel, ones.data(), ones.size() * 8); H2D(tt->d_vel, ones.data(), ones.size() * 8);
    H2D(plan->d_maxey, mey.data(), b * 8);                                                 // Planner.solve(..., HW)  (PMAIN:162,176)
    HIP_TRY(h, hipStreamSynchronize(st));
    h->state_valid_B = tt->state_valid_B = plan->state_valid_B = 0;
    if (obs) {    // the estimator in the loop: it starts as the lap-0 fleet's (from_plant = 0) and runs through the lap event
        std::vector<double> v(b * 8, 0.0);                                              // the estimate in the plant's layout
        for (size_t i = 0; i < b; ++i) {
            const double *p = plant0 + i * 8;
            v[i * 8 + 0] = p[0]; v[i * 8 + 1] = p[1]; v[i * 8 + 2] = obs->init_vx; v[i * 8 + 6] = p[6];
        }
        HIP_TRY(h, r->mem.alloc(d.estv, b * 8 * 8));
        H2D(d.estv, v.data(), b * 8 * 8);
        d.meas = d.estv;
        rc = lpvmpc_observer_start(h, *obs, B, plant0, cfg->dt_sim, 0); if (rc) return rc;     // (synchronises)
    }
    h->race = r.release(); tt->race_owner = h; plan->race_owner = h;
    return LPVMPC_OK;
}

extern "C" int lpvmpc_race_init(lpvmpc_handle *h, lpvmpc_handle *tt, lpvmpc_handle *plan, int32_t B, const double *plant0,
                                const int32_t *half_track0, const lpvmpc_race_config *cfg) {
    return race_init(h, tt, plan, B, plant0, half_track0, cfg, nullptr, false);
}

extern "C" int lpvmpc_race_init_actuated(lpvmpc_handle *h, lpvmpc_handle *tt, lpvmpc_handle *plan, int32_t B, const double *plant0,
                                         const int32_t *half_track0, const lpvmpc_race_config *cfg, const lpvmpc_observer_config *obs,
                                         const lpvmpc_actuator_config *act, const int32_t *delay_a, const int32_t *delay_df) {
    if (!act) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_init_actuated: actuator config is NULL");
    return race_init(h, tt, plan, B, plant0, half_track0, cfg, obs, true, act, delay_a, delay_df);
}

int lpvmpc_race_init_rows(lpvmpc_handle *h, lpvmpc_handle *tt, lpvmpc_handle *plan, int32_t B, const double *plant0, const int32_t *half_track0,
                          const lpvmpc_race_config *cfg, const lpvmpc_observer_config *obs, const lpvmpc_actuator_config *act,
                          const int32_t *delay_a, const int32_t *delay_df, const double *plant_params, bool tyres, const double *tyre_params) {
    const char *who = tyres ? "lpvmpc_race_init_tyres" : "lpvmpc_race_init_vehicles";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: path handle is NULL", who);
    if (!cfg || B <= 0) return fail(h, LPVMPC_E_ARG, "%s: NULL configuration or B <= 0", who);
    std::vector<double> tab, tyr;
    int rc = lpvmpc_plant_rows(h, B, plant_params, h->cfg, cfg->mu_sim, who, tab); if (rc) return rc;
    if (tyres) { rc = lpvmpc_tyre_rows(h, B, tyre_params, who, tyr); if (rc) return rc; }
    lpvmpc_actuator_config off;
    lpvmpc_actuator_default_config(&off);
    if (!act) { act = &off; delay_a = delay_df = nullptr; }               // all off: the delayed kernels pass the command through
    return race_init(h, tt, plan, B, plant0, half_track0, cfg, obs, true, act, delay_a, delay_df, &tab, tyres ? &tyr : nullptr);
}

extern "C" int lpvmpc_race_init_vehicles(lpvmpc_handle *h, lpvmpc_handle *tt, lpvmpc_handle *plan, int32_t B, const double *plant0,
                                         const int32_t *half_track0, const lpvmpc_race_config *cfg, const lpvmpc_observer_config *obs,
                                         const lpvmpc_actuator_config *act, const int32_t *delay_a, const int32_t *delay_df,
                                         const double *plant_params) {
    return lpvmpc_race_init_rows(h, tt, plan, B, plant0, half_track0, cfg, obs, act, delay_a, delay_df, plant_params, false, nullptr);
}

PlantSide *lpvmpc_plant_side(lpvmpc_handle *h, const lpvmpc::RaceDev **race) {
    if (race) *race = h && h->race ? &h->race->d : nullptr;
    return !h ? nullptr : h->race ? &h->race->side : h->cl_plant ? &h->cl_side : nullptr;
}

// what a race's disturbances act on (lpvmpc_set_disturbances): each vehicle steps RaceDev::nstep times in a tick
lpvmpc::DistDev lpvmpc_race_dist(const PlantSide &p, const lpvmpc::RaceDev &d) {
    lpvmpc::DistDev t{};
    t.B = d.B; t.plant = d.plant; t.k = p.act.d.k; t.nstep = d.nstep; t.n_fixed = 0; t.dt = p.pc.dt;
    t.hw = d.hw; t.slack = d.slack;
    t.live_p = const_cast<double *>(p.veh.d.p); t.live_t = const_cast<double *>(p.tyre.t);
    return t;
}

// The inventory of the race's per-vehicle state (lpvmpc_handle.hpp: RaceState; include/lpvmpc.h, "Race snapshot, restore and clone").
// Worked out from the kernels of a tick (race.hip, fleet_kernels.hpp, track_race.hip, handoff.hip, disturbance.hip and the masked LPV /
// solve launches): an array is listed if a tick can read a word of it that an earlier tick, or the init, wrote.  A masked launch
// leaves the rows of the vehicles it does not run as they are, so every per-vehicle output that a later tick or a read-back can see
// is state (the handles' uPred, iters, status, polish, the planner's xPred ...).  Not listed, because every word a tick reads of them
// is written earlier in the same tick under the same mask: sig, the handles' d_AB / d_states / d_resid, the controllers' d_xPred /
// d_xlast / d_delta, and the path handle's d_curv, which no kernel of a race dereferences.  The planner's x0 / xlast / delta are
// written by race_plan_start_kernel before their readers too; they are carried so that a blob holds the planner's whole recursion.
// Bindings and tables (plant, tyre, model, tuning, track, gain and disturbance rows, La / Ld, d_maxey, the hand-off operators, the
// live Cf / Cr / c_f words that the disturbances' kernel rewrites on every tick that steps the vehicle) are the caller's business
bool lpvmpc_race_state(lpvmpc_handle *h, RaceState &s) {
    lpvmpc_race *r = h->race;
    if (!r) return false;
    using namespace lpvmpc;
    const RaceDev &d = r->d;
    const lpvmpc_handle *tt = r->tt, *p = r->plan;
    const int N = d.N, Np = d.Np;
    s = RaceState{};
    const int32_t shape[8] = {d.B, N, Np, d.M, r->sd, d.lap_cols, d.laps, r->ticks};
    std::memcpy(s.shape, shape, sizeof(shape));
    s.recording = r->rec != nullptr;
    s.heats = r->heats != nullptr;
    s.events = r->events != nullptr;
    if (h->trk.tab) s.track_of = &h->trk_of;
    s.features = (d.estv ? LPVMPC_SNAP_HAS_ESTIMATOR : 0u) | (r->side.act.d.ring ? LPVMPC_SNAP_HAS_ACTUATOR : 0u) |
                 (r->side.dist.d.rows ? LPVMPC_SNAP_HAS_DISTURBANCES : 0u) | (h->trk.tab ? LPVMPC_SNAP_HAS_TRACKS : 0u) |
                 (r->side.wear.d.rows ? LPVMPC_SNAP_HAS_TYRE_WEAR : 0u);
    auto add = [&s](const char *name, void *ptr, int type, int W, int layout = STATE_VEHICLE_MAJOR) {
        RaceStateDesc e{};
        std::strncpy(e.name, name, 15);
        e.ptr = ptr; e.type = type; e.W = W; e.layout = layout;
        s.tab.push_back(e);
    };
    // RaceDev
    add("plant", d.plant, STATE_F64, 8); add("cmd", d.cmd, STATE_F64, 2); add("local", d.local, STATE_F64, 6);
    if (d.estv) add("estv", d.estv, STATE_F64, 8);
    add("phase", d.phase, STATE_I32, 1); add("lap", d.lap, STATE_I32, 1); add("half", d.half, STATE_I32, 1); add("rk", d.rk, STATE_I32, 1);
    add("plan_done", d.plan_done, STATE_I32, 1); add("idx", d.idx, STATE_I32, 1); add("nstep", d.nstep, STATE_I32, 1);
    add("src", d.src, STATE_I32, 1); add("step", d.step, STATE_I32, 1); add("alive", d.alive, STATE_I32, 1);
    add("iters", d.iters, STATE_I32, 1); add("status", d.status, STATE_I32, 1);
    add("lap_step", d.lap_step, STATE_I32, d.lap_cols);
    add("m_path", d.m_path, STATE_I32, 1); add("m_tt", d.m_tt, STATE_I32, 1); add("m_plan", d.m_plan, STATE_I32, 1);
    add("m_pfirst", d.m_pfirst, STATE_I32, 1); add("m_pcont", d.m_pcont, STATE_I32, 1);
    add("SSc", d.SSc, STATE_F64, 1); add("ref0", d.ref0, STATE_F64, 3); add("refs", d.refs, STATE_F64, 5 * d.M);
    add("SSp", d.SSp, STATE_F64, Np + 1); add("pose", d.pose, STATE_F64, 3);
    // path and trajectory-tracking handles: the carried rows of their workspaces (d_curv [B][N]: race_measure_kernel's stride)
    add("path.uold", h->d_uold, STATE_F64, 2 + r->sd); add("path.uPred", h->d_uPred, STATE_F64, N * 2); add("path.vel", h->d_vel, STATE_F64, N + 1);
    add("path.iters", h->d_iters, STATE_I32, 1); add("path.status", h->d_status, STATE_I32, 1); add("path.polish", h->d_polish, STATE_I32, 1);
    add("tt.uold", tt->d_uold, STATE_F64, 2 + r->sd); add("tt.uPred", tt->d_uPred, STATE_F64, N * 2); add("tt.vel", tt->d_vel, STATE_F64, N + 1);
    add("tt.curv", tt->d_curv, STATE_F64, N);
    add("tt.iters", tt->d_iters, STATE_I32, 1); add("tt.status", tt->d_status, STATE_I32, 1); add("tt.polish", tt->d_polish, STATE_I32, 1);
    // planner handle
    add("plan.x0", p->d_x0, STATE_F64, 5); add("plan.xPred", p->d_xPred, STATE_F64, (Np + 1) * 5); add("plan.uPred", p->d_uPred, STATE_F64, Np * 2);
    add("plan.xlast", p->d_xlast, STATE_F64, Np * 6); add("plan.delta", p->d_delta, STATE_F64, Np);
    add("plan.iters", p->d_iters, STATE_I32, 1); add("plan.status", p->d_status, STATE_I32, 1); add("plan.polish", p->d_polish, STATE_I32, 1);
    // actuator, estimator, disturbances, tyre wear
    if (r->side.act.d.ring) {
        add("act.ring", r->side.act.d.ring, STATE_F64, 2 * kActRing, STATE_WORD_MAJOR);
        add("act.servo", r->side.act.d.servo, STATE_F64, 1); add("act.k", r->side.act.d.k, STATE_I32, 1);
    }
    if (d.estv) add("obs.state", h->obs_state, STATE_F64, kObsStride);
    if (r->side.dist.d.rows) add("dist.state", r->side.dist.d.state, STATE_F64, kDistState, STATE_WORD_MAJOR);
    if (r->side.wear.d.rows) {                                                  // the tyre set travels whole: its state and its rows
        add("wear.state", r->side.wear.d.state, STATE_F64, kWearState, STATE_WORD_MAJOR);
        add("wear.rows", const_cast<double *>(r->side.wear.d.rows), STATE_F64, kWearWords, STATE_WORD_MAJOR);
    }
    return true;
}
void lpvmpc_race_set_ticks(lpvmpc_handle *h, int ticks) { if (h->race) h->race->ticks = ticks; }

bool lpvmpc_race_attach_view(lpvmpc_handle *h, RaceAttachView &v) {
    lpvmpc_race *r = h->race;
    if (!r) return false;
    v.B = r->d.B; v.laps = r->d.laps; v.hw = r->d.hw; v.slack = r->d.slack; v.plant = r->d.plant; v.nstep = r->d.nstep; v.phase = r->d.phase;
    v.side = &r->side;
    v.heats = &r->heats; v.inter = &r->inter; v.contact = &r->contact; v.walls = &r->walls; v.events = &r->events;
    v.heats_serial = &r->heats_serial; v.walls_serial = &r->walls_serial;
    return true;
}

// the detach chain (race_attach.hpp): heats -> interactions -> contact model, readers first; the walls and the event log stand alone
int lpvmpc_race_detach_readers(lpvmpc_handle *h, RaceLayer layer) {
    if (layer == RACE_HEATS) return lpvmpc_race_detach(h, RACE_INTERACTIONS);   // the interactions read the heats' lists and extents
    if (layer == RACE_INTERACTIONS) return lpvmpc_race_detach(h, RACE_CONTACT); // the contact model reads the interactions' binding
    return LPVMPC_OK;
}
int lpvmpc_race_detach(lpvmpc_handle *h, RaceLayer layer) {
    lpvmpc_race *r = h ? h->race : nullptr;
    if (!r) return LPVMPC_OK;
    RC_TRY(lpvmpc_race_detach_readers(h, layer));
    const bool attached = layer == RACE_HEATS ? r->heats != nullptr : layer == RACE_INTERACTIONS ? r->inter != nullptr :
                          layer == RACE_CONTACT ? r->contact != nullptr : layer == RACE_WALLS ? r->walls != nullptr : r->events != nullptr;
    if (!attached) return LPVMPC_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    HIP_TRY(h, hipStreamSynchronize(st));                                       // no tick in flight reads the binding
    switch (layer) {
    case RACE_HEATS: r->heats.reset(); r->heats_serial++; break;
    case RACE_INTERACTIONS: {
        const InterBinding &q = *r->inter;
        H2D(q.d.mu_live, q.mu_base.data(), q.mu_base.size() * 8);               // the base words back to the live table
        HIP_TRY(h, hipStreamSynchronize(st));
        r->inter.reset();
        break;
    }
    case RACE_CONTACT: r->contact.reset(); break;                               // back to the centres form
    case RACE_WALLS: r->walls.reset(); r->walls_serial++; break;
    case RACE_EVENTS: r->events.reset(); break;
    }
    return LPVMPC_OK;
}
const std::vector<double> *lpvmpc_race_mu_base(lpvmpc_handle *h) {
    return h && h->race && h->race->inter ? &h->race->inter->mu_base : nullptr;
}

extern "C" int lpvmpc_race_init_observed(lpvmpc_handle *h, lpvmpc_handle *tt, lpvmpc_handle *plan, int32_t B, const double *plant0,
                                         const int32_t *half_track0, const lpvmpc_race_config *cfg, const lpvmpc_observer_config *obs) {
    return race_init(h, tt, plan, B, plant0, half_track0, cfg, obs, true);
}

// one tick, in order on the path handle's stream: masked planner work, measurement, path LPV + solve, TT LPV + solve,
// command + plant
extern "C" int lpvmpc_race_tick(lpvmpc_handle *h, int32_t n_ticks) {
    if (!h || !h->race || n_ticks < 1) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_tick: call lpvmpc_race_init first");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    lpvmpc_race *r = h->race;
    lpvmpc_handle *tt = r->tt, *p = r->plan;
    const lpvmpc::RaceDev &d = r->d;
    const int B = d.B, N = d.N;
    hipStream_t st = h->stream;
    // the kernels of the race's form (step_form.hpp)
    const PlantSide &side = r->side;
    const lpvmpc::StepForm form = lpvmpc_step_form(h, side, &d);
    lpvmpc::RaceMeasureFn *measure = lpvmpc::race_measure_launcher(form);
    lpvmpc::RaceStepFn *step = lpvmpc::race_step_launcher(form);
    if (!measure || !step) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_tick: internal error: no kernel for step form 0x%x", form);
    for (int t = 0; t < n_ticks; ++t) {
        // planner ticks of the racing vehicles whose controller tick reads a new message (PMAIN:126-224, 257-308)
        // bound (lpvmpc_set_tracks on all three handles, equal): every kernel that reads the track takes its bound form
        const lpvmpc::TrackDev *trk = lpvmpc_trk(h), *ttrk = lpvmpc_trk(tt), *ptrk = lpvmpc_trk(p);
        if (ptrk) HIP_TRY(h, lpvmpc::launch_race_plan_start_trk(p->d_cfg, *ptrk, d, st));
        else HIP_TRY(h, lpvmpc::launch_race_plan_start(p->d_cfg, d, st));
        HIP_TRY(h, lpvmpc::launch_lpv(p->dev, p->d_cfg, p->d_model, B, p->d_x0, p->d_uPred, nullptr, d.SSp, 60.0, 0, p->d_states, p->d_AB, st, d.m_pcont,
                                      ptrk, p->d_trk_model));
        HIP_TRY(h, lpvmpc::launch_abc(p->dev, p->d_cfg, p->d_model, B, p->d_xlast, p->d_delta, p->d_AB, st, d.m_pfirst, ptrk, p->d_trk_model));
        SolveArgs pa{B, p->d_x0, p->d_AB, nullptr, nullptr, p->d_maxey, p->d_xPred, p->d_uPred, p->d_status, p->d_iters, p->d_polish, p->d_resid,
                     nullptr, 0, 5};
        pa.active = d.m_plan;
        int rc = lpvmpc_launch_solve_timed(p, pa, st); if (rc) return fail(h, rc, "%s", lpvmpc_last_error(p));
        if (ptrk) HIP_TRY(h, lpvmpc::launch_plan_pose_trk(p->d_cfg, *ptrk, B, p->d_xPred, d.SSp, d.pose, d.sig, st, d.m_plan));
        else HIP_TRY(h, lpvmpc::launch_plan_pose(p->d_cfg, B, p->d_xPred, d.SSp, d.pose, d.sig, st, d.m_plan));
        HIP_TRY(h, lpvmpc::launch_resample(B, d.Np, d.M, p->d_Wop, p->d_FWop, d.sig, d.refs, st, d.m_plan));
        // measurement, lap logic, masks of the two controllers
        const int seed = r->ticks < 9;
        HIP_TRY(h, measure(lpvmpc::RaceMeasureArgs{h->d_cfg, trk, d, seed, r->sd}, st));
        // path controller (CMAIN:310-336)
        const double *x0 = d.local; int x0_stride = 6;
        if (seed) {                                                          // scratch only: unmasked
            HIP_TRY(h, lpvmpc::launch_cl_seed(B, N, d.local, h->d_xlast, h->d_delta, st));
            HIP_TRY(h, lpvmpc::launch_abc(h->dev, h->d_cfg, h->d_model, B, h->d_xlast, h->d_delta, h->d_AB, st, nullptr, trk, h->d_trk_model));
        } else {
            HIP_TRY(h, lpvmpc::launch_lpv(h->dev, h->d_cfg, h->d_model, B, d.local, h->d_uPred, h->d_vel, nullptr, 60.0, 0, h->d_states, h->d_AB, st, d.m_path,
                                          trk, h->d_trk_model));
            x0 = h->d_states; x0_stride = N * 6;
        }
        SolveArgs ca{B, x0, h->d_AB, h->d_vel, h->d_uold, nullptr, h->d_xPred, h->d_uPred, h->d_status, h->d_iters, h->d_polish, h->d_resid,
                     nullptr, 0, x0_stride};
        ca.active = d.m_path;
        rc = lpvmpc_launch_solve_timed(h, ca, st); if (rc) return rc;
        // trajectory-tracking controller (CMAIN:361-363)
        HIP_TRY(h, lpvmpc::launch_lpv(tt->dev, tt->d_cfg, tt->d_model, B, d.local, tt->d_uPred, tt->d_vel, tt->d_curv, 60.0, 1, tt->d_states, tt->d_AB, st, d.m_tt,
                                      ttrk, tt->d_trk_model));
        SolveArgs ta{B, d.local, tt->d_AB, tt->d_vel, tt->d_uold, nullptr, tt->d_xPred, tt->d_uPred, tt->d_status, tt->d_iters, tt->d_polish,
                     tt->d_resid, nullptr, 0, 6};
        ta.active = d.m_tt;
        rc = lpvmpc_launch_solve_timed(tt, ta, st); if (rc) return fail(h, rc, "%s", lpvmpc_last_error(tt));
        if (side.dist.d.rows) HIP_TRY(h, lpvmpc::launch_disturbance(h->d_cfg, trk, side.dist.d, st));   // lpvmpc_set_disturbances
        if (const ContactBinding *q = r->contact.get())                             // lpvmpc_race_contact: in place of the interactions' launch
            HIP_TRY(h, lpvmpc::launch_contact_tick(q->d, q->block, r->ticks, st));
        else if (const InterBinding *q = r->inter.get())                            // lpvmpc_race_interactions: a kick comes before a contact
            HIP_TRY(h, lpvmpc::launch_interaction_tick(q->d, q->block, r->ticks, st));
        if (const WallBinding *q = r->walls.get())                                  // lpvmpc_race_walls: a shove into a wall is answered on this tick
            HIP_TRY(h, lpvmpc::launch_wall_tick(q->d, r->ticks, st));
        if (side.wear.d.rows) HIP_TRY(h, lpvmpc::launch_tyre_wear(side.wear_arg(), st));                // lpvmpc_set_tyre_wear: on the state the step starts from
        HIP_TRY(h, step(lpvmpc::RaceStepArgs{d, side.pc, side.tpc(), lpvmpc_observer_vehicles_gains(h), h->obs_state, h->obs_p, side.act.d, side.fault.d}, st));
        if (lpvmpc_race_recorder *q = r->rec.get()) {                               // the recorder (record.hip)
            int slot = -1;
            if ((r->ticks - q->t_start) % q->stride == 0) { slot = q->total % q->capacity; q->total++; }
            if (trk) HIP_TRY(h, lpvmpc::launch_race_record_trk(*trk, q->d, r->ticks, slot, st));
            else HIP_TRY(h, lpvmpc::launch_race_record(h->d_cfg, q->d, r->ticks, slot, st));
        }
        if (const HeatsBinding *q = r->heats.get())                                 // the heats (heats.hip)
            HIP_TRY(h, lpvmpc::launch_heat_tick(h->d_cfg, trk, q->d, q->block, r->ticks, st));
        if (EventBinding *q = r->events.get()) {                                    // the event log (events.hip): last, every plane is final
            lpvmpc::EventSrc s{};                                                   // the bindings of THIS tick: the log keeps no pointer of theirs
            s.phase = d.phase; s.lap = d.lap; s.lap_step = d.lap_step; s.lap_cols = d.lap_cols;
            if (const HeatsBinding *hb = r->heats.get()) {
                s.heat_f = hb->d.out_f; s.heat_i = hb->d.out_i; s.off = hb->d.off; s.members = hb->d.members; s.n_heats = hb->d.n_heats;
                s.heat_of = q->heat_of;
                s.heats_fresh = !q->heats_known || q->heats_serial != r->heats_serial;
                if (s.heats_fresh) HIP_TRY(h, lpvmpc::launch_event_heat_of(B, s.n_heats, s.off, s.members, q->heat_of, st));
            }
            if (const WallBinding *wb = r->walls.get()) {
                s.wall_f = wb->d.out_f; s.wall_i = wb->d.out_i;
                s.walls_fresh = !q->walls_known || q->walls_serial != r->walls_serial;
            }
            HIP_TRY(h, lpvmpc::launch_event_tick(q->d, s, r->ticks, st));
            // seen only once the tick that stores its words is launched: a failed launch leaves the source at first sight
            if (s.heat_f) { q->heats_known = true; q->heats_serial = r->heats_serial; }
            if (s.wall_f) { q->walls_known = true; q->walls_serial = r->walls_serial; }
        }
        r->ticks++;
    }
    return LPVMPC_OK;
}

extern "C" int lpvmpc_race_read(lpvmpc_handle *h, double *plant, double *local_state, double *cmd, int32_t *phase, int32_t *lap,
                                int32_t *iters, int32_t *status, int32_t *plan_iters, int32_t *plan_status, int32_t *ticks) {
    if (!h || !h->race) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_read: call lpvmpc_race_init first");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    lpvmpc_race *r = h->race;
    const lpvmpc::RaceDev &d = r->d;
    const size_t B = d.B;
    hipStream_t st = h->stream;
    if (plant) D2H(plant, d.plant, B * 8 * 8);
    if (local_state) D2H(local_state, d.local, B * 6 * 8);
    if (cmd) D2H(cmd, d.cmd, B * 2 * 8);
    if (phase) D2H(phase, d.phase, B * 4);
    if (lap) D2H(lap, d.lap, B * 4);
    if (iters) D2H(iters, d.iters, B * 4);
    if (status) D2H(status, d.status, B * 4);
    if (plan_iters) D2H(plan_iters, r->plan->d_iters, B * 4);
    if (plan_status) D2H(plan_status, r->plan->d_status, B * 4);
    HIP_TRY(h, hipStreamSynchronize(st));
    if (ticks) ticks[0] = r->ticks;
    return LPVMPC_OK;
}

extern "C" int lpvmpc_race_laps(lpvmpc_handle *h, int32_t *lap_step, int32_t *alive_ticks) {
    if (!h || !h->race) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_laps: call lpvmpc_race_init first");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const lpvmpc::RaceDev &d = h->race->d;
    hipStream_t st = h->stream;
    if (lap_step) D2H(lap_step, d.lap_step, (size_t)d.B * d.lap_cols * 4);
    if (alive_ticks) D2H(alive_ticks, d.alive, (size_t)d.B * 4);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

extern "C" int lpvmpc_race_predictions(lpvmpc_handle *h, double *path_uPred, double *tt_uPred) {
    if (!h || !h->race) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_predictions: call lpvmpc_race_init first");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const lpvmpc::RaceDev &d = h->race->d;
    hipStream_t st = h->stream;
    const size_t n = (size_t)d.B * d.N * 2 * 8;
    if (path_uPred) D2H(path_uPred, d.p_uPred, n);
    if (tt_uPred) D2H(tt_uPred, d.t_uPred, n);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

// the race recorder (include/lpvmpc.h, "Race recorder"; kernel: record.hip)
static bool mul_size(size_t &acc, size_t x) { return !__builtin_mul_overflow(acc, x, &acc); }

extern "C" int lpvmpc_race_record(lpvmpc_handle *h, const lpvmpc_race_record_config *cfg) {
    if (!h || !h->race) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_record: call lpvmpc_race_init first");
    if (!cfg || cfg->capacity < 0 || cfg->stride < 1)
        return fail(h, LPVMPC_E_ARG, "lpvmpc_race_record: NULL configuration, capacity < 0 or stride < 1");
    lpvmpc_race *r = h->race;
    const lpvmpc::RaceDev &d = r->d;
    const size_t B = d.B, cap = cfg->capacity, laps1 = (size_t)d.laps + 1;
    size_t nf = cap, ni = cap, sf = B, si = B;
    if (!mul_size(nf, LPVMPC_REC_F64) || !mul_size(nf, B) || !mul_size(nf, sizeof(double)) || !mul_size(ni, LPVMPC_REC_I32) ||
        !mul_size(ni, B) || !mul_size(ni, sizeof(int32_t)) || !mul_size(sf, laps1) || !mul_size(sf, LPVMPC_LAPSTAT_F64 * sizeof(double)) ||
        !mul_size(si, laps1) || !mul_size(si, LPVMPC_LAPSTAT_I32 * sizeof(int32_t)))
        return fail(h, LPVMPC_E_ARG, "lpvmpc_race_record: capacity %d x %d vehicles overflows the buffer size", cfg->capacity, d.B);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    HIP_TRY(h, hipStreamSynchronize(st));                                       // no tick in flight reads the old recorder
    r->rec.reset();                                                             // the old recorder first: a ring may fill the card
    if (cap == 0) return LPVMPC_OK;
    std::unique_ptr<lpvmpc_race_recorder> q(new (std::nothrow) lpvmpc_race_recorder());   // installed once it is complete
    if (!q) return fail(h, LPVMPC_E_NOMEM, "out of host memory");
    lpvmpc::RecDev &e = q->d;
    hipError_t err = hipSuccess;
    size_t want = 0;
    auto take = [&](auto *&p, size_t n) { if (err == hipSuccess) { want = n; err = q->mem.alloc(p, n); } };
    take(e.rec_f, nf); take(e.rec_i, ni); take(e.stat_f, sf); take(e.stat_i, si); take(e.prev_phase, B * 4); take(e.end_tick, B * 4);
    if (err != hipSuccess) return fail(h, LPVMPC_E_NOMEM, "lpvmpc_race_record: hipMalloc of %zu B failed: %s", want, hipGetErrorString(err));
    e.B = d.B; e.N = d.N; e.laps = d.laps; e.q9 = d.q9; e.hw = d.hw; e.slack = d.slack;
    e.plant = d.plant; e.local = d.local; e.cmd = d.cmd; e.ref0 = d.ref0; e.t_vel = d.t_vel;
    e.obs = d.estv ? h->obs_state : nullptr;
    e.phase = d.phase; e.lap = d.lap; e.rk = d.rk; e.src = d.src; e.iters = d.iters; e.status = d.status; e.m_plan = d.m_plan;
    e.q_iters = r->plan->d_iters; e.q_status = r->plan->d_status;
    q->capacity = cfg->capacity; q->stride = cfg->stride; q->t_start = r->ticks; q->total = 0;
    err = hipMemsetAsync(e.stat_f, 0, sf, st);
    if (err == hipSuccess) err = hipMemsetAsync(e.stat_i, 0, si, st);
    if (err == hipSuccess) err = hipMemsetAsync(e.end_tick, 0xff, B * 4, st);
    if (err == hipSuccess) err = hipMemcpyAsync(e.prev_phase, d.phase, B * 4, hipMemcpyDeviceToDevice, st);
    if (err != hipSuccess) {                                                    // no recorder with statistics that were never zeroed
        (void)hipStreamSynchronize(st);
        return fail(h, LPVMPC_E_HIP, "lpvmpc_race_record: resetting the recorder failed: %s", hipGetErrorString(err));
    }
    r->rec = std::move(q);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_race_record_read(lpvmpc_handle *h, int32_t n, int32_t *total, int32_t *tick, double *f64, int32_t *i32) {
    if (!h || !h->race) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_record_read: call lpvmpc_race_init first");
    if (n < 0) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_record_read: n < 0");
    const lpvmpc_race_recorder *q = h->race->rec.get();
    if (!q) { if (total) total[0] = 0; return LPVMPC_OK; }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t B = q->d.B, wf = (size_t)LPVMPC_REC_F64 * B, wi = (size_t)LPVMPC_REC_I32 * B;
    const int kept = q->total < q->capacity ? q->total : q->capacity, m = n < kept ? n : kept;
    const int k0 = q->total - m;                                                // the first record copied (0-based since the start)
    for (int j = 0; j < m;) {                                                   // at most two runs of the ring
        const int slot = (k0 + j) % q->capacity, run = std::min(m - j, q->capacity - slot);
        if (f64) D2H(f64 + (size_t)j * wf, q->d.rec_f + (size_t)slot * wf, (size_t)run * wf * 8);
        if (i32) D2H(i32 + (size_t)j * wi, q->d.rec_i + (size_t)slot * wi, (size_t)run * wi * 4);
        j += run;
    }
    HIP_TRY(h, hipStreamSynchronize(st));
    if (tick) for (int j = 0; j < m; ++j) tick[j] = q->t_start + (k0 + j) * q->stride;
    if (total) total[0] = q->total;
    return LPVMPC_OK;
}

extern "C" int lpvmpc_race_lap_stats(lpvmpc_handle *h, double *f64, int32_t *i32, int32_t *end_tick) {
    if (!h || !h->race) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_lap_stats: call lpvmpc_race_init first");
    const lpvmpc_race_recorder *q = h->race->rec.get();
    if (!q) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_lap_stats: recording is off (lpvmpc_race_record)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t n = (size_t)q->d.B * (q->d.laps + 1);
    if (f64) D2H(f64, q->d.stat_f, n * LPVMPC_LAPSTAT_F64 * 8);
    if (i32) D2H(i32, q->d.stat_i, n * LPVMPC_LAPSTAT_I32 * 4);
    if (end_tick) D2H(end_tick, q->d.end_tick, (size_t)q->d.B * 4);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}
