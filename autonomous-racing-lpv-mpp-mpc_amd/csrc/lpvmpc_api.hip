// lpvmpc_api.hip -- the C ABI of liblpvmpc.so (declared in include/lpvmpc.h): handle management,
// workspace, host<->device staging and kernel launches.  No CPU compute path exists here: every
// compute entry point fails with LPVMPC_E_NODEVICE when no HIP device is usable.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "lpvmpc_handle.hpp"

static thread_local std::string g_last_error;
static thread_local int g_last_code = 0;

int lpvmpc_fail(lpvmpc_handle *h, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    g_last_error = buf;
    g_last_code = code;
    return code;
}

extern "C" int lpvmpc_version(void) { return LPVMPC_VERSION; }

extern "C" void lpvmpc_default_config(int32_t kind, lpvmpc_config *c) {
    std::memset(c, 0, sizeof(*c));
    c->kind = kind; c->device = 0;
    c->lf = 0.125; c->lr = 0.125; c->m = 1.98; c->Iz = 0.03; c->Cf = 60.0; c->Cr = 60.0; c->mu = 0.05;
    c->max_vel = 5.0; c->min_vel = 0.9;
    if (kind == LPVMPC_KIND_CONTROLLER) {
        c->N = 20; c->dt = 1.0 / 30.0;
        const double q[6] = {400.0, 1.0, 1.0, 20.0, 0.0, 1100.0};    // racing tuning, controllerMain.py:146-148
        for (int i = 0; i < 6; ++i) c->Q[i * 6 + i] = q[i];
        c->dR[0] = 100.0; c->dR[1] = 45.0;
    } else {
        c->N = 30; c->dt = 0.05;
        const double q[5] = {0.000000000000088, 9.703658572659423, 0.5, -0.000000000213635, 0.153591566469547};
        for (int i = 0; i < 5; ++i) c->Q[i * 5 + i] = q[i];           // plannerMain.py:96
        const double l[5] = {-1.00702414775175, -0.187661946033823, 0.0, -0.0, 0.0329493219494661};
        for (int i = 0; i < 5; ++i) c->L_cf[i] = l[i];                // plannerMain.py:97
        c->R[0] = 0.8; c->dR[0] = 6.0; c->dR[1] = 6.0;               // plannerMain.py:98-99
    }
    c->ctrl_vx_min = 0.01; c->ctrl_delta_max = 0.249; c->ctrl_a_max = 4.0; c->ctrl_a_min_abs = 1.0;
    const double xmin[5] = {0.9, -1, -2, -0.2, -0.8}, xmax[5] = {5.0, 1, 2, 0.2, 0.8};
    for (int i = 0; i < 5; ++i) { c->plan_xmin[i] = xmin[i]; c->plan_xmax[i] = xmax[i]; }
    c->plan_umin[0] = -0.249; c->plan_umin[1] = -0.7; c->plan_umax[0] = 0.249; c->plan_umax[1] = 2.0;
    c->rho = 0.1; c->sigma = 1e-6; c->alpha = 1.6; c->eps_abs = 1e-3; c->eps_rel = 1e-3;
    c->eps_prim_inf = 1e-4; c->eps_dual_inf = 1e-4; c->polish_delta = 1e-6; c->adaptive_rho_tolerance = 5.0;
    c->max_iter = 4000; c->check_termination = 25; c->scaling = 10; c->adaptive_rho = 1;
    c->adaptive_rho_interval = 25; c->polish = 1; c->polish_refine_iter = 3;
    c->track_rows = 0;
}

static const int kEventRing = 1024;      // event pairs kept by lpvmpc_set_timing (main launches, and separately resume passes)
extern "C" int lpvmpc_join(lpvmpc_handle *h, void *stream);
// ---- straggler deferral: the two pools ---------------------------------------------------------------------------------
// an entry holds the LDS image of whichever kernel variant runs (the run-time-horizon kernel keeps its factor tiles in LDS:
// the largest image) plus the loop scalars and output pointers
static int entry_stride_for(int N) { return (N + 1) * (3 * lpvmpc::kTS + 19 * 8 + 8) + 16 + 64 + 8 + 80 + 64 + lpvmpc::kParkScalars; }
static int defer_entry_stride(const lpvmpc_handle *h) { return entry_stride_for(h->cfg.N); }
static int ensure_defer(lpvmpc_handle *h, int B, hipStream_t st) {
    const int cap = h->defer_cap > 0 ? h->defer_cap : (B / 8 > 64 ? B / 8 : 64);
    const int stride = defer_entry_stride(h);
    if (h->dpool[0] && h->defer_cur_cap >= cap && h->defer_stride == stride) return LPVMPC_OK;
    if (h->dpool[0]) {      // growing: finish what is parked in the old pools first
        int rc = lpvmpc_join(h, (void *)(h->defer_stream_set ? h->defer_stream : st)); if (rc) return rc;
        HIP_TRY(h, hipStreamSynchronize(h->defer_stream_set ? h->defer_stream : st));
    }
    release<DeferPools>(*h);
    DeferPools p;
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(h, p.defer_mem.alloc(p.dpool[i], (size_t)cap * stride * 8));
        HIP_TRY(h, p.defer_mem.alloc(p.dcount[i], 16));
        HIP_TRY(h, hipMemsetAsync(p.dcount[i], 0, 16, st));
    }
    if (!h->defer_event) HIP_TRY(h, hipEventCreateWithFlags(&h->defer_event, hipEventDisableTiming));
    if (!h->dstats) { HIP_TRY(h, h->mem.alloc(h->dstats, 16)); HIP_TRY(h, hipMemsetAsync(h->dstats, 0, 16, st)); }
    p.defer_cur_cap = cap; p.defer_stride = stride;
    static_cast<DeferPools &>(*h) = std::move(p); h->dcur = 0;
    return LPVMPC_OK;
}
// one resume pass on `st`: continues the entries of pool[dcur] for `budget` more iterations (0 = to completion), parks the
// unfinished ones in the other pool, which becomes the current one.  (Only the passes to completion are left: lpvmpc_join and
// defer_budget 0.  The bounded continuation rides in the next deferred call's main launch, lpvmpc_solve_batch_dev.)
static int resume_pass(lpvmpc_handle *h, int budget, hipStream_t st) {
    const int A = h->dcur, Bp = 1 - A;
    SolveArgs a{};
    a.B = h->defer_cur_cap; a.resume = 1; a.defer_after = budget; a.tail = h->defer_tail;
    a.pool_in = h->dpool[A]; a.pool_in_count = h->dcount[A];
    a.pool = h->dpool[Bp]; a.pool_count = h->dcount[Bp];
    a.pool_cap = h->defer_cur_cap; a.pool_stride = h->defer_stride; a.x0_stride = h->nx; a.defer_stats = h->dstats;
    const int slot = h->rv.count % kEventRing;
    if (h->timing) HIP_TRY(h, hipEventRecord(h->rv.e0[slot], st));
    HIP_TRY(h, lpvmpc::launch_solve(h->dev, h->d_cfg, a, st, h->force_generic));
    if (h->timing) { HIP_TRY(h, hipEventRecord(h->rv.e1[slot], st)); h->rv.count++; }
    h->dcur = Bp;
    return LPVMPC_OK;
}

// the pools are ordered by stream: hands them over from the stream of the last deferred call to st
static int defer_take_stream(lpvmpc_handle *h, hipStream_t st) {
    if (h->defer_stream_set && h->defer_stream != st) {
        HIP_TRY(h, hipEventRecord(h->defer_event, h->defer_stream));
        HIP_TRY(h, hipStreamWaitEvent(st, h->defer_event, 0));
    }
    h->defer_stream = st; h->defer_stream_set = true;
    return LPVMPC_OK;
}

static int ensure_ws(lpvmpc_handle *h, int B) {
    if (B <= h->cap) return LPVMPC_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    release<Workspace>(*h); h->state_valid_B = 0;     // engines cache workspace pointers: batch calls are refused on busy handles
    Workspace w;
    const size_t N = h->cfg.N, nx = h->nx, nb = h->nb, b = B;
#define ALLOC(p, n) HIP_TRY(h, w.ws_mem.alloc(w.p, (n)))
    ALLOC(d_x0, b * nx * 8); ALLOC(d_uprev, b * N * 2 * 8); ALLOC(d_vel, b * (N + 1) * 8);
    ALLOC(d_curv, b * (N + 1) * 8); ALLOC(d_uold, b * (2 + h->cfg.steering_delay) * 8); ALLOC(d_maxey, b * 8);
    ALLOC(d_AB, b * N * nx * nb * 8); ALLOC(d_states, b * N * nx * 8);
    ALLOC(d_xPred, b * (N + 1) * nx * 8); ALLOC(d_uPred, b * N * 2 * 8); ALLOC(d_resid, b * 4 * 8);
    ALLOC(d_xlast, b * N * 6 * 8); ALLOC(d_delta, b * N * 8);
    ALLOC(d_state, b * 3 * (N + 1) * 8 * 8);
    if (h->cfg.kind == LPVMPC_KIND_PLANNER && N == 30) ALLOC(d_scal, b * 3 * (N + 1) * 8 * 8);      // see SolveArgs::scal
    ALLOC(d_status, b * 4); ALLOC(d_iters, b * 4); ALLOC(d_polish, b * 4); ALLOC(d_active, b * 4);
#undef ALLOC
    w.cap = B;
    static_cast<Workspace &>(*h) = std::move(w);
    return LPVMPC_OK;
}

extern "C" lpvmpc_handle *lpvmpc_create(const lpvmpc_config *cfg) {
    if (!cfg) { fail(nullptr, LPVMPC_E_ARG, "lpvmpc_create: cfg is NULL"); return nullptr; }
    if (cfg->kind != LPVMPC_KIND_CONTROLLER && cfg->kind != LPVMPC_KIND_PLANNER) { fail(nullptr, LPVMPC_E_ARG, "lpvmpc_create: bad kind %d", cfg->kind); return nullptr; }
    if (cfg->N < 8 || cfg->N > LPVMPC_MAX_N) { fail(nullptr, LPVMPC_E_ARG, "lpvmpc_create: N=%d outside [8,%d]", cfg->N, LPVMPC_MAX_N); return nullptr; }
    if (cfg->steering_delay < 0 || cfg->steering_delay > 8 || cfg->steering_delay >= cfg->N || (cfg->kind == LPVMPC_KIND_PLANNER && cfg->steering_delay != 0)) {
        fail(nullptr, LPVMPC_E_ARG, "lpvmpc_create: steering_delay=%d (controller: 0..8 and < N; planner: 0)", cfg->steering_delay); return nullptr; }
    if (cfg->track_rows < 0 || cfg->track_rows > LPVMPC_MAX_TRACK_ROWS) { fail(nullptr, LPVMPC_E_ARG, "lpvmpc_create: track_rows=%d outside [0,%d]", cfg->track_rows, LPVMPC_MAX_TRACK_ROWS); return nullptr; }
    if (!(cfg->dt > 0) || !(cfg->rho > 0) || !(cfg->sigma > 0) || !(cfg->alpha > 0 && cfg->alpha < 2) || !(cfg->polish_delta > 0)) {
        fail(nullptr, LPVMPC_E_ARG, "lpvmpc_create: dt, rho, sigma, polish_delta must be > 0 and 0 < alpha < 2"); return nullptr; }
    // the remaining settings OSQP 0.6 (validate_settings) refuses
    if (!(cfg->eps_abs >= 0) || !(cfg->eps_rel >= 0) || (cfg->eps_abs == 0 && cfg->eps_rel == 0) || !(cfg->eps_prim_inf > 0) || !(cfg->eps_dual_inf > 0)) {
        fail(nullptr, LPVMPC_E_ARG, "lpvmpc_create: eps_abs, eps_rel must be >= 0 and not both 0; eps_prim_inf, eps_dual_inf must be > 0"); return nullptr; }
    if (cfg->max_iter <= 0 || cfg->scaling < 0 || cfg->polish_refine_iter < 0 || cfg->check_termination < 0 || cfg->adaptive_rho_interval < 0) {
        fail(nullptr, LPVMPC_E_ARG, "lpvmpc_create: max_iter must be > 0; scaling, polish_refine_iter, check_termination, adaptive_rho_interval >= 0"); return nullptr; }
    if (!(cfg->adaptive_rho_tolerance >= 1)) { fail(nullptr, LPVMPC_E_ARG, "lpvmpc_create: adaptive_rho_tolerance must be >= 1"); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { fail(nullptr, LPVMPC_E_NODEVICE, "lpvmpc_create: no HIP device available (there is no CPU fallback)"); return nullptr; }
    if (cfg->device < 0 || cfg->device >= ndev) { fail(nullptr, LPVMPC_E_ARG, "lpvmpc_create: device %d of %d", cfg->device, ndev); return nullptr; }
    lpvmpc_handle *h = new (std::nothrow) lpvmpc_handle();
    if (!h) { fail(nullptr, LPVMPC_E_NOMEM, "out of host memory"); return nullptr; }
    h->cfg = *cfg;
    h->nx = cfg->kind == LPVMPC_KIND_CONTROLLER ? 6 : 5; h->nb = h->nx + 2;
    DevCfg &d = h->dev;
    std::memset(&d, 0, sizeof(d));
    d.kind = cfg->kind; d.N = cfg->N; d.track_rows = cfg->track_rows; d.max_iter = cfg->max_iter;
    d.check_termination = cfg->check_termination; d.scaling = cfg->scaling; d.adaptive_rho = cfg->adaptive_rho;
    d.adaptive_rho_interval = cfg->adaptive_rho_interval; d.polish = cfg->polish; d.polish_refine_iter = cfg->polish_refine_iter;
    d.steering_delay = cfg->steering_delay;
    d.dt = cfg->dt; d.lf = cfg->lf; d.lr = cfg->lr; d.m = cfg->m; d.Iz = cfg->Iz; d.Cf = cfg->Cf; d.Cr = cfg->Cr; d.mu = cfg->mu;
    d.max_vel = cfg->max_vel; d.min_vel = cfg->min_vel;
    {   // the tuning words Q R dR Lcf box_lo box_hi: the device row of the configuration's own tuning (tunings_api.hip)
        double row[LPVMPC_TUNING_WORDS];
        lpvmpc_tuning_from_config(cfg, row);
        lpvmpc_tuning_device_row(cfg->kind, row, d.Q);
    }
    d.rho = cfg->rho; d.sigma = cfg->sigma; d.alpha = cfg->alpha; d.eps_abs = cfg->eps_abs; d.eps_rel = cfg->eps_rel;
    d.eps_prim_inf = cfg->eps_prim_inf; d.eps_dual_inf = cfg->eps_dual_inf; d.delta = cfg->polish_delta;
    d.rho_tol = cfg->adaptive_rho_tolerance;
    std::memcpy(d.track, cfg->track, sizeof(double) * 6 * cfg->track_rows);
    if (hipSetDevice(cfg->device) != hipSuccess) { fail(nullptr, LPVMPC_E_HIP, "hipSetDevice(%d) failed", cfg->device); delete h; return nullptr; }
    if (h->mem.alloc(h->d_cfg, sizeof(DevCfg)) != hipSuccess ||
        hipMemcpy(h->d_cfg, &h->dev, sizeof(DevCfg), hipMemcpyHostToDevice) != hipSuccess) {
        fail(nullptr, LPVMPC_E_HIP, "uploading the configuration failed"); lpvmpc_destroy(h); return nullptr; }
    const size_t lds = lpvmpc::solve_lds_bytes(cfg->kind, cfg->N);
    if (lds > 160 * 1024) { fail(nullptr, LPVMPC_E_ARG, "lpvmpc_create: N=%d needs %zu B of LDS per instance (> 160 KiB)", cfg->N, lds); lpvmpc_destroy(h); return nullptr; }
    return h;
}

extern "C" void lpvmpc_destroy(lpvmpc_handle *h) {
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    (void)hipDeviceSynchronize();          // launches of this handle may still be running on the caller's streams (deferred calls: their resume passes)
    if (h->cascade) lpvmpc_cascade_free(h);                                  // (frees the cascade's estimator state)
    if (h->race) lpvmpc_race_free(h);
    if (h->race_owner && h->race_owner->race) lpvmpc_race_free(h->race_owner);   // a handle the race of another one drives: end that race
    // a planner handle that a controller's cascade still drives: end that cascade first (it holds a pointer to this handle)
    if (h->cascade_owner && h->cascade_owner->cascade) lpvmpc_cascade_free(h->cascade_owner);
    delete h;
}

extern "C" int lpvmpc_last_error_code(void) { return g_last_code; }
extern "C" const char *lpvmpc_last_error(const lpvmpc_handle *h) { return h ? h->err.c_str() : g_last_error.c_str(); }

extern "C" int lpvmpc_set_option(lpvmpc_handle *h, const char *name, int32_t value) {
    if (!h || !name) return fail(h, LPVMPC_E_ARG, "lpvmpc_set_option: bad arguments");
    if ((std::strcmp(name, "force_generic_kernel") == 0 || std::strcmp(name, "kernel_variant") == 0) && h->dpool[0]) {
        // parked instances hold the LDS image of the kernel variant that parked them: finish them before the variant changes
        int rc = lpvmpc_join(h, (void *)h->defer_stream); if (rc) return rc;
        HIP_TRY(h, hipStreamSynchronize(h->defer_stream));
    }
    if (std::strcmp(name, "force_generic_kernel") == 0) { h->force_generic = value != 0 ? 1 : 0; return LPVMPC_OK; }
    if (std::strcmp(name, "warm_start") == 0) {
        if (value < 0 || value > 2) return fail(h, LPVMPC_E_ARG, "warm_start must be 0 (off), 1 (previous solution) or 2 (shifted by one stage)");
        h->warm_mode = value; h->state_valid_B = 0; return LPVMPC_OK;
    }
    if (std::strcmp(name, "kernel_variant") == 0) { if (value < 0 || value > 9) return fail(h, LPVMPC_E_ARG, "kernel_variant must be 0 .. 9"); h->force_generic = value; return LPVMPC_OK; }
    if (std::strcmp(name, "defer_after") == 0) {
        if (value < 0) return fail(h, LPVMPC_E_ARG, "defer_after must be >= 0 (iterations; 0 = off)");
        if (value == 0 && h->defer_after > 0 && h->dpool[0]) { int rc = lpvmpc_join(h, (void *)h->defer_stream); if (rc) return rc; }   // nothing stays parked
        h->defer_after = value; return LPVMPC_OK;
    }
    if (std::strcmp(name, "defer_budget") == 0) {
        if (value < -1) return fail(h, LPVMPC_E_ARG, "defer_budget must be >= -1 (iterations per resume pass; 0 = every pass runs to completion; -1 = no pass behind a call: parked instances wait for lpvmpc_join)");
        h->defer_budget = value; return LPVMPC_OK;
    }
    if (std::strcmp(name, "defer_pool") == 0) {
        if (value < 0) return fail(h, LPVMPC_E_ARG, "defer_pool must be >= 0 (pool entries; 0 = max(64, B / 8))");
        HIP_TRY(h, hipSetDevice(h->cfg.device));
        if (h->dpool[0]) { int rc = lpvmpc_join(h, (void *)h->defer_stream); if (rc) return rc; HIP_TRY(h, hipStreamSynchronize(h->defer_stream)); }
        release<DeferPools>(*h); h->defer_cap = value; return LPVMPC_OK;
    }
    if (std::strcmp(name, "defer_tail") == 0) { h->defer_tail = value != 0 ? 1 : 0; return LPVMPC_OK; }      // both kernels continue the same pool entries
    if (std::strcmp(name, "cascade_prefetch") == 0) { h->cascade_prefetch = value != 0 ? 1 : 0; return LPVMPC_OK; }   // read by lpvmpc_cascade_init
    return fail(h, LPVMPC_E_ARG, "lpvmpc_set_option: unknown option '%s'", name);
}

extern "C" int lpvmpc_reserve(lpvmpc_handle *h, int32_t B) {
    if (!h || B <= 0) return fail(h, LPVMPC_E_ARG, "lpvmpc_reserve: bad arguments");
    return ensure_ws(h, B);
}


extern "C" int lpvmpc_set_timing(lpvmpc_handle *h, int32_t on) {
    if (!h) return LPVMPC_E_ARG;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (EventRing *r : {&h->ev, &h->rv})
        if (on && r->e0.empty()) {
            r->e0.resize(kEventRing); r->e1.resize(kEventRing);
            for (int i = 0; i < kEventRing; ++i) { HIP_TRY(h, hipEventCreate(&r->e0[i])); HIP_TRY(h, hipEventCreate(&r->e1[i])); }
        }
    h->timing = on != 0; h->ev.count = 0; h->rv.count = 0; h->last_ms = -1.0;
    return LPVMPC_OK;
}

// total time between the pairs of a ring (waits for them); last: the time of the newest pair, if wanted
static int ring_time_stats(lpvmpc_handle *h, const EventRing &r, double *total_ms, int32_t *count, double *last) {
    if (!total_ms || !count) return LPVMPC_E_ARG;
    const int n = r.count < kEventRing ? r.count : kEventRing;
    double tot = 0.0;
    for (int i = 0; i < n; ++i) {
        float ms = 0.f;
        HIP_TRY(h, hipEventSynchronize(r.e1[i]));
        HIP_TRY(h, hipEventElapsedTime(&ms, r.e0[i], r.e1[i]));
        tot += ms;
        if (last) *last = ms;
    }
    *total_ms = tot; *count = n;
    return LPVMPC_OK;
}

extern "C" int lpvmpc_kernel_time_stats(lpvmpc_handle *h, double *total_ms, int32_t *count) {
    return h ? ring_time_stats(h, h->ev, total_ms, count, &h->last_ms) : LPVMPC_E_ARG;
}

extern "C" double lpvmpc_last_kernel_ms(lpvmpc_handle *h) {
    if (!h) return -1.0;
    double tot; int32_t n;
    if (lpvmpc_kernel_time_stats(h, &tot, &n) != LPVMPC_OK || n == 0) return -1.0;
    return h->last_ms;
}

// ------------------------------------------------------------------------------------------------
int lpvmpc_need_track(lpvmpc_handle *h, const char *who) {
    if (h->cfg.track_rows < 1 && !h->trk.tab) return fail(h, LPVMPC_E_ARG, "%s: the handle was created without a track table", who);
    return LPVMPC_OK;
}

static int launch_lpv(lpvmpc_handle *h, int B, const double *x0, const double *u_prev, const double *vel_ref,
                      const double *curv_s, double cf_new, int lap, double *states, double *AB, hipStream_t st) {
    // (lpvmpc::launch_lpv has no bound form of the controller roll-out without [A | B]; every entry point passes the workspace's)
    if (h->trk.tab && h->cfg.kind == LPVMPC_KIND_CONTROLLER && !AB)
        return fail(h, LPVMPC_E_ARG, "lpvmpc_lpv_batch: the states-only controller roll-out is not available on a handle with per-vehicle tracks "
                    "bound (lpvmpc_set_tracks)");
    HIP_TRY(h, lpvmpc::launch_lpv(h->dev, h->d_cfg, h->d_model, B, x0, u_prev, vel_ref, curv_s, cf_new, lap, states, AB, st, nullptr,
                                  lpvmpc_trk(h), h->d_trk_model));
    return LPVMPC_OK;
}

int lpvmpc_launch_solve_timed(lpvmpc_handle *h, const SolveArgs &a, hipStream_t st) {
    const int slot = h->ev.count % kEventRing;
    if (h->timing) HIP_TRY(h, hipEventRecord(h->ev.e0[slot], st));
    SolveArgs b = a;
    if (h->d_scal && a.B <= h->cap) b.scal = h->d_scal;          // (the launcher ignores it for deferred / resumed launches)
    if (h->solve_mask && !a.resume) b.active = h->solve_mask;      // lpvmpc_solve_batch_masked (synchronous: its launch carries no riders)
    { int rc = lpvmpc_solve_tune(h, b); if (rc) return rc; }       // the handle's tuning rows (every main launch of every route comes through here)
    HIP_TRY(h, lpvmpc::launch_solve(h->dev, h->d_cfg, b, st, h->force_generic));
    if (h->timing) { HIP_TRY(h, hipEventRecord(h->ev.e1[slot], st)); h->ev.count++; }
    return LPVMPC_OK;
}

int lpvmpc_launch_solve_warm(lpvmpc_handle *h, SolveArgs a, hipStream_t st) {
    a.state = h->warm_mode ? h->d_state : nullptr;
    a.warm = (h->warm_mode && h->state_valid_B == a.B) ? h->warm_mode : 0;
    // a cold launch with the option on: what the state holds (uninitialised memory, solves from before the option was set again or of
    // another batch size) must not reach the next call through an instance this launch does not write (lpvmpc_solve_batch_masked).
    // Zeros are a cold start: the kernel stores them itself for an instance without a solution.
    if (h->warm_mode && !a.warm) HIP_TRY(h, hipMemsetAsync(h->d_state, 0, (size_t)a.B * 3 * (h->cfg.N + 1) * 8 * 8, st));
    int rc = lpvmpc_launch_solve_timed(h, a, st); if (rc) return rc;
    if (h->warm_mode) h->state_valid_B = a.B;
    return LPVMPC_OK;
}

// The closed-loop fleet (lpvmpc_cl_*) and the cascade keep their state between ticks in the handle's workspace (reference
// windows, receding-horizon inputs, last commands, statuses): a stand-alone batch call on the same handle would overwrite it
// -- or, with a larger B, reallocate it -- without any error.  Such calls are refused; use a second handle.
int lpvmpc_check_batch(lpvmpc_handle *h, int B, const char *who) {
    if (h && busy(h))
        return fail(h, LPVMPC_E_ARG, "%s: this handle runs a %s whose state lives in its workspace; use another handle for batch calls "
                    "(lpvmpc_cl_release ends the fleet)", who, h->cl_plant ? "closed-loop fleet" : (h->race || h->race_owner) ? "race" : "planner + controller cascade");
    return lpvmpc_check_common(h, B, who);
}

int lpvmpc_check_common(lpvmpc_handle *h, int B, const char *who) {
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (B <= 0) return fail(h, LPVMPC_E_ARG, "%s: B=%d", who, B);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return ensure_ws(h, B);
}



// ------------------------------------------------------------------------------------------------
// Small batches (the 30 Hz control loop calls with B = 1): every host array of a call travels through ONE pinned
// staging buffer and ONE copy per direction instead of one pageable copy per array (11 copies per fused tick).
// Large batches keep the direct copies.  in() / out() return the device pointer the kernels must use.
// ------------------------------------------------------------------------------------------------
static const size_t kPackBytes = 512 * 1024;
struct IoPack {
    lpvmpc_handle *h; hipStream_t st; bool on; size_t in_off, out_off;
    struct Out { void *user, *dev; size_t off, bytes; } outs[8];
    int n_out;
    static size_t al(size_t n) { return (n + 255) & ~(size_t)255; }
    int begin(lpvmpc_handle *h_, hipStream_t st_, size_t in_bytes, size_t out_bytes, int n_arrays) {
        h = h_; st = st_; in_off = out_off = 0; n_out = 0;
        on = in_bytes + 256 * (size_t)n_arrays <= kPackBytes && out_bytes + 256 * (size_t)n_arrays <= kPackBytes;
        if (on && !h->d_pack_out) {                       // (the last of the four: set once all are there)
            if (!h->h_pack_in) HIP_TRY(h, hipHostMalloc((void **)&h->h_pack_in, kPackBytes));
            if (!h->h_pack_out) HIP_TRY(h, hipHostMalloc((void **)&h->h_pack_out, kPackBytes));
            if (!h->d_pack_in) HIP_TRY(h, h->mem.alloc(h->d_pack_in, kPackBytes));
            HIP_TRY(h, h->mem.alloc(h->d_pack_out, kPackBytes));
        }
        return LPVMPC_OK;
    }
    // host staging area of an input (packed mode) -- lets a caller write a re-laid-out array directly
    void *in_slot(size_t bytes, void **dev) { void *p = h->h_pack_in + in_off; *dev = h->d_pack_in + in_off; in_off += al(bytes); return p; }
    int in(const void *src, void *dev_default, size_t bytes, void **dev) {
        if (!on) { *dev = dev_default; HIP_TRY(h, hipMemcpyAsync(dev_default, src, bytes, hipMemcpyHostToDevice, st)); return LPVMPC_OK; }
        std::memcpy(in_slot(bytes, dev), src, bytes);
        return LPVMPC_OK;
    }
    int flush_in() {
        if (on && in_off) HIP_TRY(h, hipMemcpyAsync(h->d_pack_in, h->h_pack_in, in_off, hipMemcpyHostToDevice, st));
        return LPVMPC_OK;
    }
    void *out(void *user, void *dev_default, size_t bytes) {          // user may be NULL (result not wanted)
        void *dev = on ? (void *)(h->d_pack_out + out_off) : dev_default;
        outs[n_out++] = Out{user, dev, out_off, bytes};
        if (on) out_off += al(bytes);
        return dev;
    }
    const void *host_of(int i) const { return h->h_pack_out + outs[i].off; }           // valid after flush_out in packed mode
    int flush_out() {
        if (on) {
            if (out_off) HIP_TRY(h, hipMemcpyAsync(h->h_pack_out, h->d_pack_out, out_off, hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipStreamSynchronize(st));
            for (int i = 0; i < n_out; ++i) if (outs[i].user) std::memcpy(outs[i].user, h->h_pack_out + outs[i].off, outs[i].bytes);
        } else {
            for (int i = 0; i < n_out; ++i) if (outs[i].user) HIP_TRY(h, hipMemcpyAsync(outs[i].user, outs[i].dev, outs[i].bytes, hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipStreamSynchronize(st));
        }
        return LPVMPC_OK;
    }
};
#define IO_TRY(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)

// rows [A|B] of the device layout [rows][nx][nx + 2] -> the caller's A [rows][nx][nx] and B [rows][nx][2] (either may be NULL)
static void split_ab(const double *src, size_t rows, size_t nx, double *A, double *Bm) {
    const size_t nb = nx + 2;
    for (size_t t = 0; t < rows; ++t)
        for (size_t r = 0; r < nx; ++r) {
            const double *row = src + (t * nx + r) * nb;
            if (A) for (size_t a = 0; a < nx; ++a) A[(t * nx + r) * nx + a] = row[a];
            if (Bm) { Bm[(t * nx + r) * 2 + 0] = row[nx]; Bm[(t * nx + r) * 2 + 1] = row[nx + 1]; }
        }
}

extern "C" int lpvmpc_lpv_batch(lpvmpc_handle *h, int32_t B, const double *x0, const double *u_prev,
                                const double *vel_ref, const double *curv_s, double cf_new, int32_t lap,
                                double *states, double *A, double *Bm) {
    if (h && B == 0) return LPVMPC_OK;                                   // an empty batch is a no-op
    int rc = lpvmpc_check_batch(h, B, "lpvmpc_lpv_batch"); if (rc) return rc;
    rc = lpvmpc_model_check(h, B, "lpvmpc_lpv_batch"); if (rc) return rc;
    rc = lpvmpc_tracks_check(h, B, "lpvmpc_lpv_batch"); if (rc) return rc;
    const bool ctrl = h->cfg.kind == LPVMPC_KIND_CONTROLLER;
    if (!x0 || !u_prev) return fail(h, LPVMPC_E_ARG, "lpvmpc_lpv_batch: x0 / u_prev is NULL");
    if (ctrl && !vel_ref) return fail(h, LPVMPC_E_ARG, "lpvmpc_lpv_batch: controller needs vel_ref");
    if (ctrl && lap != 0 && !curv_s) return fail(h, LPVMPC_E_ARG, "lpvmpc_lpv_batch: controller with lap != 0 needs curv_ref");
    if (!ctrl && !curv_s) return fail(h, LPVMPC_E_ARG, "lpvmpc_lpv_batch: planner needs SS");
    if ((ctrl && lap == 0) || !ctrl) { rc = lpvmpc_need_track(h, "lpvmpc_lpv_batch"); if (rc) return rc; }
    const size_t N = h->cfg.N, nx = h->nx, nb = h->nb, b = B;
    hipStream_t st = h->stream;
    const size_t n_ab = b * N * nx * nb, n_st = b * N * nx;
    IoPack io;
    IO_TRY(io.begin(h, st, (b * nx + b * N * 2 + b * (N + 1) * 2) * 8, (n_ab + n_st) * 8, 6));
    void *p_x0, *p_up, *p_vel = nullptr, *p_curv = nullptr;
    IO_TRY(io.in(x0, h->d_x0, b * nx * 8, &p_x0)); IO_TRY(io.in(u_prev, h->d_uprev, b * N * 2 * 8, &p_up));
    if (ctrl) IO_TRY(io.in(vel_ref, h->d_vel, b * (N + 1) * 8, &p_vel));
    if (curv_s) IO_TRY(io.in(curv_s, h->d_curv, b * (ctrl ? N : N + 1) * 8, &p_curv));
    IO_TRY(io.flush_in());
    std::vector<double> ab;
    if (!io.on && (A || Bm)) ab.resize(n_ab);
    // packed mode: [A|B] is de-interleaved straight from the staging buffer (no user copy of the raw block)
    double *p_ab = (double *)io.out(io.on ? nullptr : (void *)ab.data(), h->d_AB, n_ab * 8);
    double *p_states = (double *)io.out(states, h->d_states, n_st * 8);
    rc = launch_lpv(h, B, (const double *)p_x0, (const double *)p_up, (const double *)p_vel, (const double *)p_curv, cf_new, lap, p_states, p_ab, st);
    if (rc) return rc;
    IO_TRY(io.flush_out());
    if (A || Bm) split_ab(io.on ? (const double *)io.host_of(0) : ab.data(), b * N, nx, A, Bm);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_estimate_abc_batch(lpvmpc_handle *h, int32_t B, const double *xlast, const double *delta,
                                         double *A, double *Bm) {
    if (h && B == 0) return LPVMPC_OK;                                   // an empty batch is a no-op
    int rc = lpvmpc_check_batch(h, B, "lpvmpc_estimate_abc_batch"); if (rc) return rc;
    rc = lpvmpc_model_check(h, B, "lpvmpc_estimate_abc_batch"); if (rc) return rc;
    rc = lpvmpc_tracks_check(h, B, "lpvmpc_estimate_abc_batch"); if (rc) return rc;
    if (!xlast || !delta) return fail(h, LPVMPC_E_ARG, "lpvmpc_estimate_abc_batch: NULL input");
    rc = lpvmpc_need_track(h, "lpvmpc_estimate_abc_batch"); if (rc) return rc;
    const size_t N = h->cfg.N, nx = h->nx, nb = h->nb, b = B;
    hipStream_t st = h->stream;
    H2D(h->d_xlast, xlast, b * N * 6 * 8); H2D(h->d_delta, delta, b * N * 8);
    HIP_TRY(h, lpvmpc::launch_abc(h->dev, h->d_cfg, h->d_model, B, h->d_xlast, h->d_delta, h->d_AB, st, nullptr, lpvmpc_trk(h), h->d_trk_model));
    std::vector<double> ab(b * N * nx * nb);
    D2H(ab.data(), h->d_AB, ab.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    split_ab(ab.data(), b * N, nx, A, Bm);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_solve_batch_AB(lpvmpc_handle *h, int32_t B, const double *x0, const double *A, const double *Bm,
                                     const double *vel_ref, const double *u_old, const double *max_ey,
                                     double *xPred, double *uPred, int32_t *status, int32_t *iters, double *resid,
                                     int32_t *polish) {
    if (h && B == 0) return LPVMPC_OK;                                   // an empty batch is a no-op
    int rc = lpvmpc_check_batch(h, B, "lpvmpc_solve_batch_AB"); if (rc) return rc;
    rc = lpvmpc_tuning_check(h, B, "lpvmpc_solve_batch_AB"); if (rc) return rc;
    const bool ctrl = h->cfg.kind == LPVMPC_KIND_CONTROLLER;
    if (!x0 || !A || !Bm) return fail(h, LPVMPC_E_ARG, "lpvmpc_solve_batch_AB: x0 / A / B is NULL");
    if (ctrl && !vel_ref) return fail(h, LPVMPC_E_ARG, "lpvmpc_solve_batch_AB: controller needs vel_ref");
    if (!ctrl && !max_ey) return fail(h, LPVMPC_E_ARG, "lpvmpc_solve_batch_AB: planner needs max_ey");
    const size_t N = h->cfg.N, nx = h->nx, nb = h->nb, b = B;
    hipStream_t st = h->stream;
    const size_t n_ab = b * N * nx * nb, n_x = b * (N + 1) * nx, n_u = b * N * 2;
    IoPack io;
    IO_TRY(io.begin(h, st, (b * nx + n_ab + b * (N + 1) + b * (3 + h->cfg.steering_delay)) * 8, (n_x + n_u + b * 4) * 8 + b * 12, 12));
    void *p_x0, *p_ab, *p_vel = nullptr, *p_uold = nullptr, *p_mey = nullptr;
    IO_TRY(io.in(x0, h->d_x0, b * nx * 8, &p_x0));
    std::vector<double> ab;
    double *abh;
    if (io.on) abh = (double *)io.in_slot(n_ab * 8, &p_ab);                 // interleave [A|B] straight into the staging buffer
    else { ab.resize(n_ab); abh = ab.data(); }
    for (size_t t = 0; t < b * N; ++t)
        for (size_t r = 0; r < nx; ++r) {
            double *row = abh + (t * nx + r) * nb;
            for (size_t a = 0; a < nx; ++a) row[a] = A[(t * nx + r) * nx + a];
            row[nx] = Bm[(t * nx + r) * 2 + 0]; row[nx + 1] = Bm[(t * nx + r) * 2 + 1];
        }
    if (!io.on) { p_ab = h->d_AB; H2D(h->d_AB, ab.data(), n_ab * 8); }
    if (ctrl) IO_TRY(io.in(vel_ref, h->d_vel, b * (N + 1) * 8, &p_vel));
    if (u_old) IO_TRY(io.in(u_old, h->d_uold, b * (2 + h->cfg.steering_delay) * 8, &p_uold));
    if (!ctrl) IO_TRY(io.in(max_ey, h->d_maxey, b * 8, &p_mey));
    IO_TRY(io.flush_in());
    double *o_x = (double *)io.out(xPred, h->d_xPred, n_x * 8), *o_u = (double *)io.out(uPred, h->d_uPred, n_u * 8);
    int32_t *o_st = (int32_t *)io.out(status, h->d_status, b * 4), *o_it = (int32_t *)io.out(iters, h->d_iters, b * 4);
    double *o_res = (double *)io.out(resid, h->d_resid, b * 4 * 8);
    int32_t *o_pol = (int32_t *)io.out(polish, h->d_polish, b * 4);
    SolveArgs a{B, (const double *)p_x0, (const double *)p_ab, (const double *)p_vel, (const double *)p_uold, (const double *)p_mey,
                o_x, o_u, o_st, o_it, o_pol, o_res, nullptr, 0, h->nx};
    rc = lpvmpc_launch_solve_warm(h, a, st); if (rc) return rc;
    return io.flush_out();
}

extern "C" int lpvmpc_solve_batch_dev(lpvmpc_handle *h, int32_t B, const double *x0, const double *u_prev,
                                      const double *vel_ref, const double *curv_s, const double *u_old,
                                      const double *max_ey, double cf_new, int32_t lap, double *xPred, double *uPred,
                                      int32_t *status, int32_t *iters, double *resid, int32_t *polish, void *stream) {
    if (h && B == 0) return LPVMPC_OK;                                   // an empty batch is a no-op
    int rc = lpvmpc_check_batch(h, B, "lpvmpc_solve_batch_dev"); if (rc) return rc;
    rc = lpvmpc_model_check(h, B, "lpvmpc_solve_batch_dev"); if (rc) return rc;
    rc = lpvmpc_tracks_check(h, B, "lpvmpc_solve_batch_dev"); if (rc) return rc;
    rc = lpvmpc_tuning_check(h, B, "lpvmpc_solve_batch_dev"); if (rc) return rc;
    const bool ctrl = h->cfg.kind == LPVMPC_KIND_CONTROLLER;
    if (!x0 || !u_prev || !xPred || !uPred) return fail(h, LPVMPC_E_ARG, "lpvmpc_solve_batch_dev: NULL x0 / u_prev / xPred / uPred");
    if (ctrl && !vel_ref) return fail(h, LPVMPC_E_ARG, "lpvmpc_solve_batch_dev: controller needs vel_ref");
    if (ctrl && lap != 0 && !curv_s) return fail(h, LPVMPC_E_ARG, "lpvmpc_solve_batch_dev: controller with lap != 0 needs curv_ref");
    if (!ctrl && (!curv_s || !max_ey)) return fail(h, LPVMPC_E_ARG, "lpvmpc_solve_batch_dev: planner needs SS and max_ey");
    if ((ctrl && lap == 0) || !ctrl) { rc = lpvmpc_need_track(h, "lpvmpc_solve_batch_dev"); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;
    // a warm start reads the previous call's final (x, y): with straggler deferral, finish what that call left parked first
    if (h->warm_mode && h->defer_after > 0 && h->dpool[0]) { rc = lpvmpc_join(h, stream); if (rc) return rc; }
    rc = launch_lpv(h, B, x0, u_prev, vel_ref, curv_s, cf_new, lap, nullptr, h->d_AB, st); if (rc) return rc;
    SolveArgs a{B, x0, h->d_AB, ctrl ? vel_ref : nullptr, u_old, ctrl ? nullptr : max_ey, xPred, uPred, status, iters, polish, resid,
                nullptr, 0, h->nx};
    if (h->defer_after > 0) {
        // Straggler deferral: this launch parks what is still unsolved after defer_after iterations.  With defer_budget > 0 it also
        // carries the RIDERS: everything that earlier calls of this handle left parked continues, for defer_budget more iterations,
        // in workgroups of this same launch (SolveArgs::resume 2) -- they run beside the new instances, in the residency slots that
        // free up as those finish, instead of holding the stream with a launch of their own.  The launch reads pool[dcur] and parks
        // -- riders and new instances alike -- into the other pool, which becomes the current one.  No workgroup lasts much longer than
        // its budget, so the stream is never held by one slow instance; lpvmpc_join runs the pass that finishes whatever is still parked.
        rc = ensure_defer(h, B, st); if (rc) return rc;
        rc = defer_take_stream(h, st); if (rc) return rc;
        a.defer_after = h->defer_after; a.pool_cap = h->defer_cur_cap; a.pool_stride = h->defer_stride; a.defer_stats = h->dstats;
        if (h->defer_budget > 0 && !h->defer_skip_pass) {
            const int A = h->dcur, Bp = 1 - A;
            a.resume = 2; a.defer_budget = h->defer_budget;
            a.pool_in = h->dpool[A]; a.pool_in_count = h->dcount[A];
            a.pool = h->dpool[Bp]; a.pool_count = h->dcount[Bp];
            rc = lpvmpc_launch_solve_warm(h, a, st); if (rc) return rc;
            h->dcur = Bp;
        } else {
            // budget 0: the pass behind the call runs everything that is parked to completion.  Budget -1, and the synchronous
            // host-array entry point, which joins right away: no pass -- the closing pass (the tail kernel) takes the parked
            // instances straight from this launch.  Either way this launch parks behind what pool[dcur] already holds.
            a.resume = 0; a.pool = h->dpool[h->dcur]; a.pool_count = h->dcount[h->dcur];
            rc = lpvmpc_launch_solve_warm(h, a, st); if (rc) return rc;
            if (h->defer_budget == 0 && !h->defer_skip_pass) { rc = resume_pass(h, 0, st); if (rc) return rc; }
        }
    } else {
        rc = lpvmpc_launch_solve_warm(h, a, st); if (rc) return rc;
    }
    return LPVMPC_OK;
}

extern "C" int lpvmpc_join(lpvmpc_handle *h, void *stream) {
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "lpvmpc_join: handle is NULL");
    if (!h->dpool[0]) return LPVMPC_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    int rc = defer_take_stream(h, st); if (rc) return rc;
    return resume_pass(h, 0, st);                                  // to completion: nothing stays parked
}

extern "C" int lpvmpc_resume_time_stats(lpvmpc_handle *h, double *total_ms, int32_t *count) {
    return h ? ring_time_stats(h, h->rv, total_ms, count, nullptr) : LPVMPC_E_ARG;
}

// instances parked / parking requests refused by the launches of this handle that have COMPLETED on the stream of its last deferred
// call (waits for that stream); counted since the handle's first deferred call
extern "C" int lpvmpc_defer_stats(lpvmpc_handle *h, int64_t *parked, int64_t *refused) {
    if (!h) return LPVMPC_E_ARG;
    unsigned long long v[2] = {0, 0};
    if (h->dstats) {
        HIP_TRY(h, hipSetDevice(h->cfg.device));
        if (h->defer_stream_set) HIP_TRY(h, hipStreamSynchronize(h->defer_stream));
        HIP_TRY(h, hipMemcpy(v, h->dstats, 16, hipMemcpyDeviceToHost));
    }
    if (parked) *parked = (int64_t)v[0];
    if (refused) *refused = (int64_t)v[1];
    return LPVMPC_OK;
}

extern "C" int lpvmpc_solve_batch(lpvmpc_handle *h, int32_t B, const double *x0, const double *u_prev,
                                  const double *vel_ref, const double *curv_s, const double *u_old,
                                  const double *max_ey, double cf_new, int32_t lap, double *xPred, double *uPred,
                                  int32_t *status, int32_t *iters, double *resid, int32_t *polish) {
    if (h && B == 0) return LPVMPC_OK;                                   // an empty batch is a no-op
    int rc = lpvmpc_check_batch(h, B, "lpvmpc_solve_batch"); if (rc) return rc;
    rc = lpvmpc_model_check(h, B, "lpvmpc_solve_batch"); if (rc) return rc;
    rc = lpvmpc_tracks_check(h, B, "lpvmpc_solve_batch"); if (rc) return rc;
    rc = lpvmpc_tuning_check(h, B, "lpvmpc_solve_batch"); if (rc) return rc;
    const bool ctrl = h->cfg.kind == LPVMPC_KIND_CONTROLLER;
    if (!x0 || !u_prev) return fail(h, LPVMPC_E_ARG, "lpvmpc_solve_batch: x0 / u_prev is NULL");
    if (ctrl && !vel_ref) return fail(h, LPVMPC_E_ARG, "lpvmpc_solve_batch: controller needs vel_ref");
    if (ctrl && lap != 0 && !curv_s) return fail(h, LPVMPC_E_ARG, "lpvmpc_solve_batch: controller with lap != 0 needs curv_ref");
    if (!ctrl && (!curv_s || !max_ey)) return fail(h, LPVMPC_E_ARG, "lpvmpc_solve_batch: planner needs SS and max_ey");
    const size_t N = h->cfg.N, nx = h->nx, b = B;
    hipStream_t st = h->stream;
    const size_t n_x = b * (N + 1) * nx, n_u = b * N * 2;
    IoPack io;
    IO_TRY(io.begin(h, st, (b * nx + n_u + b * (N + 1) * 2 + b * (3 + h->cfg.steering_delay)) * 8, (n_x + n_u + b * 4) * 8 + b * 12, 12));
    void *p_x0, *p_up, *p_vel = nullptr, *p_curv = nullptr, *p_uold = nullptr, *p_mey = nullptr;
    IO_TRY(io.in(x0, h->d_x0, b * nx * 8, &p_x0)); IO_TRY(io.in(u_prev, h->d_uprev, n_u * 8, &p_up));
    if (ctrl) IO_TRY(io.in(vel_ref, h->d_vel, b * (N + 1) * 8, &p_vel));
    if (curv_s) IO_TRY(io.in(curv_s, h->d_curv, b * (ctrl ? N : N + 1) * 8, &p_curv));
    if (u_old) IO_TRY(io.in(u_old, h->d_uold, b * (2 + h->cfg.steering_delay) * 8, &p_uold));
    if (!ctrl) IO_TRY(io.in(max_ey, h->d_maxey, b * 8, &p_mey));
    IO_TRY(io.flush_in());
    double *o_x = (double *)io.out(xPred, h->d_xPred, n_x * 8), *o_u = (double *)io.out(uPred, h->d_uPred, n_u * 8);
    int32_t *o_st = (int32_t *)io.out(status, h->d_status, b * 4), *o_it = (int32_t *)io.out(iters, h->d_iters, b * 4);
    double *o_res = (double *)io.out(resid, h->d_resid, b * 4 * 8);
    int32_t *o_pol = (int32_t *)io.out(polish, h->d_polish, b * 4);
    h->defer_skip_pass = true;
    rc = lpvmpc_solve_batch_dev(h, B, (const double *)p_x0, (const double *)p_up, (const double *)p_vel, (const double *)p_curv,
                                (const double *)p_uold, (const double *)p_mey, cf_new, lap, o_x, o_u, o_st, o_it, o_res, o_pol, (void *)st);
    h->defer_skip_pass = false;
    if (rc) return rc;
    if (h->defer_after > 0) { rc = lpvmpc_join(h, (void *)st); if (rc) return rc; }      // a synchronous call returns finished instances only
    return io.flush_out();
}

// the same for the flagged instances only: the others are not solved and the caller's rows of them are not written
extern "C" int lpvmpc_solve_batch_masked(lpvmpc_handle *h, int32_t B, const double *x0, const double *u_prev,
                                         const double *vel_ref, const double *curv_s, const double *u_old,
                                         const double *max_ey, double cf_new, int32_t lap, double *xPred, double *uPred,
                                         int32_t *status, int32_t *iters, double *resid, int32_t *polish, const int32_t *active) {
    if (h && B == 0) return LPVMPC_OK;                                   // an empty batch is a no-op
    int rc = lpvmpc_check_batch(h, B, "lpvmpc_solve_batch_masked"); if (rc) return rc;
    rc = lpvmpc_model_check(h, B, "lpvmpc_solve_batch_masked"); if (rc) return rc;
    rc = lpvmpc_tracks_check(h, B, "lpvmpc_solve_batch_masked"); if (rc) return rc;
    rc = lpvmpc_tuning_check(h, B, "lpvmpc_solve_batch_masked"); if (rc) return rc;
    if (!active) return fail(h, LPVMPC_E_ARG, "lpvmpc_solve_batch_masked: active is NULL");
    std::vector<int32_t> rows;
    for (int i = 0; i < B; ++i) if (active[i]) rows.push_back(i);
    if (rows.empty()) return LPVMPC_OK;                                  // nothing flagged: no launch at all
    const size_t N = h->cfg.N, nx = h->nx, b = B;
    std::vector<int32_t> flags(b);
    for (size_t i = 0; i < b; ++i) flags[i] = active[i] != 0;
    std::vector<double> tx(b * (N + 1) * nx), tu(b * N * 2), tr(b * 4);
    std::vector<int32_t> ts(b), ti(b), tp(b);
    HIP_TRY(h, hipMemcpy(h->d_active, flags.data(), b * 4, hipMemcpyHostToDevice));
    h->solve_mask = h->d_active;
    rc = lpvmpc_solve_batch(h, B, x0, u_prev, vel_ref, curv_s, u_old, max_ey, cf_new, lap, tx.data(), tu.data(), ts.data(), ti.data(),
                            tr.data(), tp.data());
    h->solve_mask = nullptr;
    if (rc) return rc;
    for (int32_t i : rows) {
        if (xPred) std::memcpy(xPred + (size_t)i * (N + 1) * nx, tx.data() + (size_t)i * (N + 1) * nx, (N + 1) * nx * 8);
        if (uPred) std::memcpy(uPred + (size_t)i * N * 2, tu.data() + (size_t)i * N * 2, N * 2 * 8);
        if (resid) std::memcpy(resid + (size_t)i * 4, tr.data() + (size_t)i * 4, 4 * 8);
        if (status) status[i] = ts[i];
        if (iters) iters[i] = ti[i];
        if (polish) polish[i] = tp[i];
    }
    return LPVMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// caller-side helpers of the reference, batched on the device
// ------------------------------------------------------------------------------------------------
extern "C" int lpvmpc_local_position_batch(lpvmpc_handle *h, int32_t B, const double *xy_psi, double half_width, double slack, double *out) {
    if (h && B == 0) return LPVMPC_OK;                                   // an empty batch is a no-op
    int rc = lpvmpc_check_batch(h, B, "lpvmpc_local_position_batch"); if (rc) return rc;
    if (!xy_psi || !out) return fail(h, LPVMPC_E_ARG, "lpvmpc_local_position_batch: NULL argument");
    rc = lpvmpc_need_track(h, "lpvmpc_local_position_batch"); if (rc) return rc;
    rc = lpvmpc_tracks_check(h, B, "lpvmpc_local_position_batch"); if (rc) return rc;
    hipStream_t st = h->stream;
    // workspace reuse: inputs in d_xlast ([cap][N][6] >= [B][3]), outputs in d_states ([cap][N][nx] >= [B][4])
    H2D(h->d_xlast, xy_psi, (size_t)B * 3 * 8);
    // bound: every instance on its own track, with that track's half width and slack (the call's are ignored)
    if (h->trk.tab) HIP_TRY(h, lpvmpc::launch_local_position_trk(h->trk, B, h->d_xlast, h->d_states, st));
    else HIP_TRY(h, lpvmpc::launch_local_position(h->d_cfg, B, h->d_xlast, half_width, slack, h->d_states, st));
    D2H(out, h->d_states, (size_t)B * 4 * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

extern "C" int lpvmpc_global_position_batch(lpvmpc_handle *h, int32_t B, const double *s_ey, double *out) {
    if (h && B == 0) return LPVMPC_OK;                                   // an empty batch is a no-op
    int rc = lpvmpc_check_batch(h, B, "lpvmpc_global_position_batch"); if (rc) return rc;
    if (!s_ey || !out) return fail(h, LPVMPC_E_ARG, "lpvmpc_global_position_batch: NULL argument");
    rc = lpvmpc_need_track(h, "lpvmpc_global_position_batch"); if (rc) return rc;
    rc = lpvmpc_tracks_check(h, B, "lpvmpc_global_position_batch"); if (rc) return rc;
    hipStream_t st = h->stream;
    H2D(h->d_xlast, s_ey, (size_t)B * 2 * 8);
    if (h->trk.tab) HIP_TRY(h, lpvmpc::launch_global_position_trk(h->trk, B, h->d_xlast, h->d_states, st));
    else HIP_TRY(h, lpvmpc::launch_global_position(h->d_cfg, B, h->d_xlast, h->d_states, st));
    D2H(out, h->d_states, (size_t)B * 3 * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

lpvmpc::PlantCfg lpvmpc_plant_cfg(const lpvmpc_handle *h, int n_sub, double dt_sim, double mu_sim) {
    lpvmpc::PlantCfg pc; pc.lf = h->cfg.lf; pc.lr = h->cfg.lr; pc.m = h->cfg.m; pc.Iz = h->cfg.Iz; pc.mu = mu_sim; pc.dt = dt_sim; pc.n_sub = n_sub;
    return pc;
}

extern "C" int lpvmpc_plant_step_batch(lpvmpc_handle *h, int32_t B, double *state, const double *u, int32_t n_sub, double dt_sim, double mu_sim) {
    if (h && B == 0) return LPVMPC_OK;                                   // an empty batch is a no-op
    int rc = lpvmpc_check_batch(h, B, "lpvmpc_plant_step_batch"); if (rc) return rc;
    if (!state || !u || n_sub < 1 || !(dt_sim > 0)) return fail(h, LPVMPC_E_ARG, "lpvmpc_plant_step_batch: bad argument");
    hipStream_t st = h->stream;
    H2D(h->d_xlast, state, (size_t)B * 8 * 8); H2D(h->d_states, u, (size_t)B * 2 * 8);
    lpvmpc::PlantStepArgs a{};
    a.B = B; a.plant = h->d_xlast; a.u = h->d_states; a.pc = lpvmpc_plant_cfg(h, n_sub, dt_sim, mu_sim);
    HIP_TRY(h, lpvmpc::plant_step_launcher(0)(a, st));
    D2H(state, h->d_xlast, (size_t)B * 8 * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

// ---- closed-loop fleet: controller in the lap-0 path-tracking branch of controllerMain.py ----------------
extern "C" int lpvmpc_cl_release(lpvmpc_handle *h) {
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "lpvmpc_cl_release: handle is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->cascade) { HIP_TRY(h, hipDeviceSynchronize()); lpvmpc_cascade_free(h); }
    if (h->race) lpvmpc_race_free(h);
    release<Fleet>(*h);
    release<ObsState>(*h);
    return LPVMPC_OK;
}

// act == nullptr: lpvmpc_cl_init (refuses delayed controllers); else lpvmpc_cl_init_actuated (any steering_delay, actuator in the plant).
// veh: the plant table [7][B] of lpvmpc_cl_init_vehicles (checked; act is then set), else null; tyre: with veh, the tyre table [4][B]
// of lpvmpc_cl_init_tyres (checked), else null
static int cl_init(lpvmpc_handle *h, int32_t B, const double *plant0, double half_width, double slack, int32_t q9_swap,
                   int32_t n_sub, double dt_sim, double mu_sim, const lpvmpc_actuator_config *act, const int32_t *delay_a, const int32_t *delay_df,
                   const std::vector<double> *veh = nullptr, const std::vector<double> *tyre = nullptr) {
    int rc = lpvmpc_check_common(h, B, "lpvmpc_cl_init"); if (rc) return rc;
    rc = lpvmpc_model_check(h, B, "lpvmpc_cl_init"); if (rc) return rc;
    // a track binding acts on the start that takes every per-vehicle table (the tyre forms' kernels have the bound forms)
    const char *entry = tyre ? "lpvmpc_cl_init_tyres" : veh ? "lpvmpc_cl_init_vehicles" : act ? "lpvmpc_cl_init_actuated" : "lpvmpc_cl_init";
    if (!tyre) { rc = lpvmpc_tracks_unbound(h, h, entry, "lpvmpc_cl_init_tyres"); if (rc) return rc; }
    rc = lpvmpc_tracks_check(h, B, "lpvmpc_cl_init"); if (rc) return rc;
    rc = lpvmpc_tuning_check(h, B, "lpvmpc_cl_init"); if (rc) return rc;
    if (h->cfg.kind != LPVMPC_KIND_CONTROLLER) return fail(h, LPVMPC_E_ARG, "lpvmpc_cl_init: controller handles only");
    if (h->race || h->race_owner) return fail(h, LPVMPC_E_ARG, "lpvmpc_cl_init: this handle takes part in a race (lpvmpc_cl_release on its path handle ends it)");
    if (h->cfg.N > 20) return fail(h, LPVMPC_E_ARG, "lpvmpc_cl_init: the reference's seed trajectories have 20 rows (N <= 20)");
    if (h->cfg.steering_delay != 0 && !act)
        return fail(h, LPVMPC_E_ARG, "lpvmpc_cl_init: the fleet engines run the reference's steeringDelay = 0 (CMAIN:49); lpvmpc_cl_init_actuated runs delayed controllers");
    if (!plant0 || n_sub < 1 || !(dt_sim > 0)) return fail(h, LPVMPC_E_ARG, "lpvmpc_cl_init: bad argument");
    rc = lpvmpc_need_track(h, "lpvmpc_cl_init"); if (rc) return rc;
    if (h->obs_cfg) { rc = lpvmpc_observer_vehicles_check(h, B, h->obs_cfg.get(), veh != nullptr, "lpvmpc_cl_init"); if (rc) return rc; }
    // the new fleet is built in f and installed after the last step that can fail: a failed call leaves no fleet (a refused
    // actuator configuration leaves the old one), never half of one
    Fleet f;
    if (act) { rc = lpvmpc_act_alloc(h, B, act, delay_a, delay_df, dt_sim, veh ? "lpvmpc_cl_init_vehicles" : "lpvmpc_cl_init_actuated", f.cl_side.act); if (rc) return rc; }
    release<Fleet>(*h);                                          // the old fleet first: never two at once
    release<ObsState>(*h);
    if (veh) { rc = lpvmpc_plant_upload(h, B, *veh, dt_sim, n_sub, f.cl_side.veh); if (rc) return rc; }
    if (tyre) { rc = lpvmpc_tyre_upload(h, *tyre, f.cl_side.tyre); if (rc) return rc; }
    f.cl_side.actuated = act != nullptr;
    HIP_TRY(h, f.cl_mem.alloc(f.cl_local_next, (size_t)B * 6 * 8));
    HIP_TRY(h, f.cl_mem.alloc(f.cl_plant, (size_t)B * 8 * 8));
    HIP_TRY(h, f.cl_mem.alloc(f.cl_local, (size_t)B * 6 * 8));
    HIP_TRY(h, f.cl_mem.alloc(f.cl_cmd, (size_t)B * 2 * 8));
    hipStream_t st = h->stream;
    H2D(f.cl_plant, plant0, (size_t)B * 8 * 8);
    HIP_TRY(h, hipMemsetAsync(f.cl_cmd, 0, (size_t)B * 2 * 8, st));
    std::vector<double> ones((size_t)B * (h->cfg.N + 1), 1.0);                  // vel_ref = 1 m/s on lap 0 (CMAIN:311,326)
    H2D(h->d_vel, ones.data(), ones.size() * 8);
    // the controller's OldSteering / OldAccelera start at zero (CTRL:71-73)
    if (act) HIP_TRY(h, hipMemsetAsync(h->d_uold, 0, (size_t)B * (2 + h->cfg.steering_delay) * 8, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    f.cl_side.B = B; f.cl_q9 = q9_swap != 0; f.cl_hw = half_width; f.cl_slack = slack;
    f.cl_side.pc = lpvmpc_plant_cfg(h, n_sub, dt_sim, mu_sim);
    h->state_valid_B = 0;
    if (h->obs_cfg) { rc = lpvmpc_observer_start(h, *h->obs_cfg, B, plant0, dt_sim, 0); if (rc) return rc; }   // the estimator in the loop
    static_cast<Fleet &>(*h) = std::move(f);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_cl_init(lpvmpc_handle *h, int32_t B, const double *plant0, double half_width, double slack, int32_t q9_swap,
                              int32_t n_sub, double dt_sim, double mu_sim) {
    return cl_init(h, B, plant0, half_width, slack, q9_swap, n_sub, dt_sim, mu_sim, nullptr, nullptr, nullptr);
}

extern "C" int lpvmpc_cl_init_actuated(lpvmpc_handle *h, int32_t B, const double *plant0, double half_width, double slack, int32_t q9_swap,
                                       int32_t n_sub, double dt_sim, double mu_sim, const lpvmpc_actuator_config *act,
                                       const int32_t *delay_a, const int32_t *delay_df) {
    if (!act) return fail(h, LPVMPC_E_ARG, "lpvmpc_cl_init_actuated: actuator config is NULL");
    return cl_init(h, B, plant0, half_width, slack, q9_swap, n_sub, dt_sim, mu_sim, act, delay_a, delay_df);
}

int lpvmpc_cl_init_rows(lpvmpc_handle *h, int32_t B, const double *plant0, double half_width, double slack, int32_t q9_swap, int32_t n_sub,
                        double dt_sim, double mu_sim, const lpvmpc_actuator_config *act, const int32_t *delay_a, const int32_t *delay_df,
                        const double *plant_params, bool tyres, const double *tyre_params) {
    const char *who = tyres ? "lpvmpc_cl_init_tyres" : "lpvmpc_cl_init_vehicles";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (B <= 0) return fail(h, LPVMPC_E_ARG, "%s: B <= 0", who);
    std::vector<double> tab, tyr;
    int rc = lpvmpc_plant_rows(h, B, plant_params, h->cfg, mu_sim, who, tab); if (rc) return rc;
    if (tyres) { rc = lpvmpc_tyre_rows(h, B, tyre_params, who, tyr); if (rc) return rc; }
    lpvmpc_actuator_config off;
    lpvmpc_actuator_default_config(&off);
    if (!act) { act = &off; delay_a = delay_df = nullptr; }               // all off: the delayed kernels pass the command through
    return cl_init(h, B, plant0, half_width, slack, q9_swap, n_sub, dt_sim, mu_sim, act, delay_a, delay_df, &tab, tyres ? &tyr : nullptr);
}

extern "C" int lpvmpc_cl_init_vehicles(lpvmpc_handle *h, int32_t B, const double *plant0, double half_width, double slack, int32_t q9_swap,
                                       int32_t n_sub, double dt_sim, double mu_sim, const lpvmpc_actuator_config *act,
                                       const int32_t *delay_a, const int32_t *delay_df, const double *plant_params) {
    return lpvmpc_cl_init_rows(h, B, plant0, half_width, slack, q9_swap, n_sub, dt_sim, mu_sim, act, delay_a, delay_df, plant_params, false, nullptr);
}

extern "C" int lpvmpc_cl_tick(lpvmpc_handle *h, int32_t n_ticks) {
    if (!h || !h->cl_plant || n_ticks < 1) return fail(h, LPVMPC_E_ARG, "lpvmpc_cl_tick: call lpvmpc_cl_init first");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int B = h->cl_side.B, N = h->cfg.N;
    hipStream_t st = h->stream;
    // the kernels of the fleet's form (step_form.hpp)
    const PlantSide &side = h->cl_side;
    const lpvmpc::TrackDev *trk = lpvmpc_trk(h);           // bound: the fleet was started by lpvmpc_cl_init_tyres, every vehicle on its own track
    const lpvmpc::StepForm form = lpvmpc_step_form(h, side, nullptr);
    lpvmpc::FleetMeasureFn *measure = lpvmpc::fleet_measure_launcher(form);
    lpvmpc::FleetStepFn *step = lpvmpc::fleet_step_launcher(form);
    if (!measure || !step) return fail(h, LPVMPC_E_ARG, "lpvmpc_cl_tick: internal error: no kernel for step form 0x%x", form);
    for (int t = 0; t < n_ticks; ++t) {
        // the measurement of this tick: made by the launch that advanced the plant at the end of the previous tick, or here
        if (h->cl_next_valid) { double *t_ = h->cl_local; h->cl_local = h->cl_local_next; h->cl_local_next = t_; }
        else HIP_TRY(h, measure(lpvmpc::FleetMeasureArgs{h->d_cfg, trk, B, h->cl_plant, h->obs_state, h->cl_cmd, h->cl_hw, h->cl_slack, h->cl_q9, h->cl_local,
                                                         h->d_uold, h->cfg.steering_delay}, st));
        const double *x0 = h->cl_local; int x0_stride = 6;
        if (h->cl_first_it < 10) {                                           // CMAIN:310-315: seed mode
            HIP_TRY(h, lpvmpc::launch_cl_seed(B, N, h->cl_local, h->d_xlast, h->d_delta, st));
            HIP_TRY(h, lpvmpc::launch_abc(h->dev, h->d_cfg, h->d_model, B, h->d_xlast, h->d_delta, h->d_AB, st, nullptr, trk, h->d_trk_model));
            h->cl_first_it++;
        } else {                                                             // CMAIN:325-331: LPV prediction, x0 = first rolled-out state
            HIP_TRY(h, lpvmpc::launch_lpv(h->dev, h->d_cfg, h->d_model, B, h->cl_local, h->d_uPred, h->d_vel, nullptr, 60.0, 0, h->d_states, h->d_AB, st,
                                          nullptr, trk, h->d_trk_model));
            x0 = h->d_states; x0_stride = N * 6;
        }
        SolveArgs a{B, x0, h->d_AB, h->d_vel, h->d_uold, nullptr, h->d_xPred, h->d_uPred, h->d_status, h->d_iters, h->d_polish, h->d_resid,
                    nullptr, 0, x0_stride};
        int rc = lpvmpc_launch_solve_warm(h, a, st); if (rc) return rc;
        if (side.dist.d.rows) HIP_TRY(h, lpvmpc::launch_disturbance(h->d_cfg, trk, side.dist.d, st));   // lpvmpc_set_disturbances
        if (side.wear.d.rows) HIP_TRY(h, lpvmpc::launch_tyre_wear(side.wear_arg(), st));                // lpvmpc_set_tyre_wear
        HIP_TRY(h, step(lpvmpc::FleetStepArgs{h->d_cfg, trk, B, N, h->d_uPred, h->cl_cmd, h->cl_plant, side.pc, side.tpc(), h->cl_hw, h->cl_slack, h->cl_q9,
                                              h->cl_local_next, h->d_uold, h->cfg.steering_delay, lpvmpc_observer_vehicles_gains(h), h->obs_state, h->obs_p,
                                              side.act.d, side.fault.d}, st));
        h->cl_next_valid = 1;
        h->cl_ticks++;
    }
    return LPVMPC_OK;
}

extern "C" int lpvmpc_cl_read(lpvmpc_handle *h, double *plant, double *local_state, double *cmd, int32_t *iters, int32_t *status) {
    if (!h || !h->cl_plant) return fail(h, LPVMPC_E_ARG, "lpvmpc_cl_read: call lpvmpc_cl_init first");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t B = h->cl_side.B;
    hipStream_t st = h->stream;
    if (plant) D2H(plant, h->cl_plant, B * 8 * 8);
    if (local_state) D2H(local_state, h->cl_local, B * 6 * 8);
    if (cmd) D2H(cmd, h->cl_cmd, B * 2 * 8);
    if (iters) D2H(iters, h->d_iters, B * 4);
    if (status) D2H(status, h->d_status, B * 4);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

// ---- gain-scheduled LPV estimator and simulated sensors (observer.hip) --------------------------------------------------------
// the kernels read the two tables with their limits as one block of words from the head of the struct
static_assert(offsetof(lpvmpc_observer_config, L_ls) == 0 &&
              offsetof(lpvmpc_observer_config, loop_rate) == sizeof(double) * 2 * (lpvmpc::kObsTable + 12), "observer config layout");
extern "C" void lpvmpc_observer_default_config(lpvmpc_observer_config *c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->loop_rate = 200.0; c->init_vx = 0.2;                                 // EST:47, MAIN_LAUNCH simulator/init_vx
    c->n_bound = 0.5; c->gps_freq = 1000.0;                                  // MAIN_LAUNCH:60-87 (every std 0)
}

int lpvmpc_observer_check(lpvmpc_handle *h, const lpvmpc_observer_config *c, const char *who) {
    if (!(c->loop_rate > 0) || !(c->gps_freq > 0) || !(c->n_bound >= 0))
        return fail(h, LPVMPC_E_ARG, "%s: loop_rate and gps_freq must be > 0, n_bound >= 0", who);
    const double sd[5] = {c->psi_std, c->psiDot_std, c->x_std, c->y_std, c->v_std};
    for (double v : sd) if (!(v >= 0)) return fail(h, LPVMPC_E_ARG, "%s: sensor standard deviations must be >= 0", who);
    return LPVMPC_OK;
}

// the estimator state of a fleet (from_plant = 0: estimate [init_vx, 0, 0, x0, y0, yaw0]) or of a cascade (from_plant = 1: the cascade
// starts at the lap event of a running vehicle, whose estimator has been running since its start -- the estimate starts at the plant
// state [vx, vy, psiDot, x, y, yaw]); GPS hold = start position, encoder reading 0, step counter 0.  Synchronises.
int lpvmpc_observer_start(lpvmpc_handle *h, const lpvmpc_observer_config &o, int B, const double *plant0, double dt_sim, int from_plant) {
    std::vector<double> os((size_t)B * lpvmpc::kObsStride, 0.0);
    for (int b = 0; b < B; ++b) {
        double *e = os.data() + (size_t)b * lpvmpc::kObsStride; const double *p = plant0 + (size_t)b * 8;
        e[0] = from_plant ? p[2] : o.init_vx; e[1] = from_plant ? p[3] : 0.0; e[2] = from_plant ? p[7] : 0.0;
        e[3] = p[0]; e[4] = p[1]; e[5] = p[6];
        e[lpvmpc::OBS_GPS_X] = p[0]; e[lpvmpc::OBS_GPS_Y] = p[1];
    }
    hipStream_t st = h->stream;
    if (h->obs_state) { HIP_TRY(h, hipStreamSynchronize(st)); release<ObsState>(*h); }
    ObsState s;
    if (!h->obs_gains) HIP_TRY(h, h->gains_mem.alloc(h->obs_gains, sizeof(double) * 2 * (lpvmpc::kObsTable + 12)));
    HIP_TRY(h, s.obs_mem.alloc(s.obs_state, os.size() * 8));
    H2D(h->obs_gains, o.L_ls, sizeof(double) * 2 * (lpvmpc::kObsTable + 12));
    H2D(s.obs_state, os.data(), os.size() * 8);
    lpvmpc::ObsParams &op = s.obs_p;
    op.dt = 1.0 / o.loop_rate; op.th_update = (1.0 / o.gps_freq) / dt_sim; op.n_bound = o.n_bound;
    op.std[0] = o.psi_std; op.std[1] = o.psiDot_std; op.std[2] = o.x_std; op.std[3] = o.y_std; op.std[4] = o.v_std;
    op.seed = o.seed; op.voff = o.vehicle_offset;
    s.obs_B = B;
    HIP_TRY(h, hipStreamSynchronize(st));
    static_cast<ObsState &>(*h) = std::move(s);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_observer_setup(lpvmpc_handle *h, const lpvmpc_observer_config *cfg) {
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "lpvmpc_observer_setup: handle is NULL");
    if (h->cfg.kind != LPVMPC_KIND_CONTROLLER) return fail(h, LPVMPC_E_ARG, "lpvmpc_observer_setup: controller handles only");
    if (!cfg) { h->obs_cfg.reset(); return LPVMPC_OK; }
    int rc = lpvmpc_observer_check(h, cfg, "lpvmpc_observer_setup"); if (rc) return rc;
    if (!h->obs_cfg) h->obs_cfg.reset(new (std::nothrow) lpvmpc_observer_config());
    if (!h->obs_cfg) return fail(h, LPVMPC_E_NOMEM, "out of host memory");
    *h->obs_cfg = *cfg;
    return LPVMPC_OK;
}

extern "C" int lpvmpc_observer_read(lpvmpc_handle *h, double *est, double *meas) {
    if (!h || !(h->cl_plant || h->cascade || h->race) || !h->obs_state)
        return fail(h, LPVMPC_E_ARG, "lpvmpc_observer_read: no fleet, cascade or race with an estimator (lpvmpc_observer_setup, then lpvmpc_cl_init / "
                                     "lpvmpc_cascade_init; or lpvmpc_race_init_observed)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipDeviceSynchronize());      // a cascade runs on its own streams
    const size_t B = h->obs_B;
    std::vector<double> os(B * lpvmpc::kObsStride);
    HIP_TRY(h, hipMemcpyAsync(os.data(), h->obs_state, os.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t b = 0; b < B; ++b) {
        const double *e = os.data() + b * lpvmpc::kObsStride;
        if (est) for (int i = 0; i < 6; ++i) est[b * 6 + i] = e[lpvmpc::OBS_EST + i];
        if (meas) for (int i = 0; i < 5; ++i) meas[b * 5 + i] = e[lpvmpc::OBS_Y + i];
    }
    return LPVMPC_OK;
}

extern "C" int lpvmpc_observer_step_batch(lpvmpc_handle *h, int32_t B, const lpvmpc_observer_config *cfg, double *est, const double *y,
                                          const double *u, const int32_t *k, double *aux) {
    if (h && B == 0) return LPVMPC_OK;                                   // an empty batch is a no-op
    // the fleet / cascade rule of the batch calls; the solver workspace is not needed (this call stages its own buffers)
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "lpvmpc_observer_step_batch: handle is NULL");
    if (busy(h))
        return fail(h, LPVMPC_E_ARG, "lpvmpc_observer_step_batch: this handle runs a fleet whose state lives in its workspace; use another handle "
                    "for batch calls (lpvmpc_cl_release ends the fleet)");
    if (B < 0) return fail(h, LPVMPC_E_ARG, "lpvmpc_observer_step_batch: B=%d", B);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    int rc;
    if (!cfg || !est || !y || !u || !k) return fail(h, LPVMPC_E_ARG, "lpvmpc_observer_step_batch: bad argument");
    rc = lpvmpc_observer_check(h, cfg, "lpvmpc_observer_step_batch"); if (rc) return rc;
    const size_t per = (size_t)(6 + 5 + 2 + lpvmpc::kObsAux) * 8 + 8;
    if (B > h->obs_ws_cap) {
        release<ObsStage>(*h);
        HIP_TRY(h, h->stage_mem.alloc(h->obs_ws, per * B));
        h->obs_ws_cap = B;
    }
    if (!h->obs_gains) HIP_TRY(h, h->gains_mem.alloc(h->obs_gains, sizeof(double) * 2 * (lpvmpc::kObsTable + 12)));
    const size_t b = B;
    double *d_est = (double *)h->obs_ws, *d_y = d_est + b * 6, *d_u = d_y + b * 5, *d_aux = d_u + b * 2;
    int32_t *d_k = (int32_t *)(d_aux + b * lpvmpc::kObsAux);
    hipStream_t st = h->stream;
    H2D(h->obs_gains, cfg->L_ls, sizeof(double) * 2 * (lpvmpc::kObsTable + 12));
    H2D(d_est, est, b * 6 * 8); H2D(d_y, y, b * 5 * 8); H2D(d_u, u, b * 2 * 8); H2D(d_k, k, b * 4);
    HIP_TRY(h, lpvmpc::launch_observer_step(h->obs_gains, B, d_est, d_y, d_u, d_k, 1.0 / cfg->loop_rate, aux ? d_aux : nullptr, st));
    D2H(est, d_est, b * 6 * 8);
    if (aux) D2H(aux, d_aux, b * lpvmpc::kObsAux * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}
