// disturbance_api.hip -- C ABI of the plant disturbances (include/lpvmpc.h, "Plant disturbances"): the checks, the binding of a lap-0
// fleet or a race (PlantSide::dist of the running engine, lpvmpc_plant_side), the read-back and the stand-alone step's launch.  Kernel:
// disturbance.hip, launched in front of the command / plant launch of lpvmpc_cl_tick, lpvmpc_race_tick and lpvmpc_plant_step_rows.
#include <cmath>
#include <vector>

#include "lpvmpc_handle.hpp"

static_assert(lpvmpc::kDistWords == LPVMPC_DIST_WORDS && lpvmpc::kDistState == LPVMPC_DIST_STATE, "host rows and device tables hold the same words");

extern "C" void lpvmpc_disturbance_default_config(lpvmpc_disturbance_config *c) {
    if (!c) return;
    c->seed = 0; c->vehicle_offset = 0; c->n_bound = 3.0;
}

// lap length of vehicle b's track: its palette entry, or the handle's own table
static double lap_length(const lpvmpc_handle *h, int b) {
    const double *T = h->cfg.track;
    int rows = h->cfg.track_rows;
    if (h->trk.tab) { const int t = h->trk_of[b]; T = h->trk_tables.data() + (size_t)t * lpvmpc::kTrackStride; rows = h->trk_rows[t]; }
    return T[(rows - 1) * 6 + 3] + T[(rows - 1) * 6 + 4];
}

int lpvmpc_dist_rows(lpvmpc_handle *h, int B, const lpvmpc_disturbance_config *cfg, const double *rows, const char *who, std::vector<double> &t) {
    static const char *names[LPVMPC_DIST_WORDS] = {"sigma_ax", "sigma_ay", "sigma_aw", "rho", "kick_step", "kick_vy", "kick_w",
                                                   "p0_s0", "p0_len", "p0_gamma", "p1_s0", "p1_len", "p1_gamma"};
    if (!(std::isfinite(cfg->n_bound) && cfg->n_bound > 0)) return fail(h, LPVMPC_E_ARG, "%s: n_bound = %g must be finite and > 0", who, cfg->n_bound);
    const size_t n = B;
    t.assign(n * (LPVMPC_DIST_WORDS + 1), 0.0);
    for (size_t b = 0; b < n; ++b) {
        const double *r = rows + b * LPVMPC_DIST_WORDS;
        const double L = lap_length(h, (int)b);
        for (int i = 0; i < LPVMPC_DIST_WORDS; ++i) {
            const double v = r[i];
            bool ok = std::isfinite(v);
            if (ok && i < 3) ok = v >= 0;
            else if (ok && i == 3) ok = v >= 0 && v < 1;
            else if (ok && i == 4) ok = v == std::floor(v) && v < 2147483648.0;
            else if (ok && (i == 7 || i == 10)) ok = v >= 0 && v < L;
            else if (ok && (i == 8 || i == 11)) ok = v >= 0 && v <= L;
            else if (ok && (i == 9 || i == 12)) ok = v >= 0;
            if (!ok)
                return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: %s = %g (every word finite; sigma >= 0; rho in [0, 1); kick_step integer-valued and "
                            "< 2^31; 0 <= s0 < L and 0 <= len <= L with the lap length L = %g; gamma >= 0)", who, b, names[i], v, L);
            t[(size_t)i * n + b] = v;
        }
        t[(size_t)LPVMPC_DIST_WORDS * n + b] = std::sqrt(1.0 - r[3] * r[3]);
    }
    return LPVMPC_OK;
}

// device tables of a binding in x.mem: rows, state (fresh: zeros, gamma 1; else the host layout [B][kDistState]) and the base words
static int dist_upload(lpvmpc_handle *h, int B, const std::vector<double> &rows_dev, const double *state, const std::vector<double> &base_p,
                       const std::vector<double> &base_t, DistBinding &x, hipStream_t st) {
    const size_t n = B;
    double *d_rows = nullptr, *d_state = nullptr, *d_base = nullptr;
    HIP_TRY(h, x.mem.alloc(d_rows, rows_dev.size() * 8));
    HIP_TRY(h, x.mem.alloc(d_state, n * LPVMPC_DIST_STATE * 8));
    HIP_TRY(h, x.mem.alloc(d_base, n * 3 * 8));
    std::vector<double> s(n * LPVMPC_DIST_STATE, 0.0), base(n * 3);
    for (size_t b = 0; b < n; ++b) {
        s[4 * n + b] = 1.0;
        if (state) for (size_t i = 0; i < LPVMPC_DIST_STATE; ++i) s[i * n + b] = state[b * LPVMPC_DIST_STATE + i];
        base[b] = base_p[4 * n + b]; base[n + b] = base_p[5 * n + b]; base[2 * n + b] = base_t[3 * n + b];
    }
    H2D(d_rows, rows_dev.data(), rows_dev.size() * 8);
    H2D(d_state, s.data(), s.size() * 8);
    H2D(d_base, base.data(), base.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));                                  // the staging vectors end with this call
    x.d.rows = d_rows; x.d.state = d_state; x.d.base = d_base; x.d.B = B;
    return LPVMPC_OK;
}

static void dist_cfg(const lpvmpc_disturbance_config &c, lpvmpc::DistDev &d) {
    d.seed = c.seed ^ LPVMPC_DIST_STREAM; d.voff = c.vehicle_offset; d.n_bound = c.n_bound;
}

// the binding of the fleet or race that h runs and, in t, what it acts on (null: none with plant and tyre tables)
static DistBinding *dist_target(lpvmpc_handle *h, lpvmpc::DistDev &t) {
    const lpvmpc::RaceDev *race = nullptr;
    PlantSide *p = lpvmpc_plant_side(h, &race);
    if (!p || !p->veh.d.p || !p->tyre.t) return nullptr;
    if (race) { t = lpvmpc_race_dist(*p, *race); return &p->dist; }
    t = lpvmpc::DistDev{};
    t.B = p->B; t.plant = h->cl_plant; t.k = p->act.d.k; t.nstep = nullptr; t.n_fixed = p->pc.n_sub; t.dt = p->pc.dt;
    t.hw = h->cl_hw; t.slack = h->cl_slack;
    t.live_p = const_cast<double *>(p->veh.d.p); t.live_t = const_cast<double *>(p->tyre.t);
    return &p->dist;
}

int lpvmpc_plant_base(lpvmpc_handle *h, const PlantSide &side, std::vector<double> &base_p, std::vector<double> &base_t, hipStream_t st) {
    if (side.base_p()) { base_p = *side.base_p(); base_t = *side.base_t(); return LPVMPC_OK; }   // a binding is attached: the live words may be scaled
    const size_t n = side.B;
    base_p.resize(n * LPVMPC_PLANT_WORDS); base_t.resize(n * LPVMPC_TYRE_WORDS);
    D2H(base_p.data(), side.veh.d.p, base_p.size() * 8);
    D2H(base_t.data(), side.tyre.t, base_t.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    if (const std::vector<double> *mu = lpvmpc_race_mu_base(h))            // interactions attached: the live mu words are theirs
        for (size_t b = 0; b < n; ++b) base_p[6 * n + b] = (*mu)[b];
    return LPVMPC_OK;
}

// the live tables' scaled words back from the base copy (the other words never change; an attached wear binding scales them again on
// the next tick that steps the vehicle)
static int dist_restore(lpvmpc_handle *h, const DistBinding &x, hipStream_t st) {
    const size_t n = x.d.B;
    H2D(x.d.live_p + 4 * n, x.base_p.data() + 4 * n, 2 * n * 8);
    H2D(x.d.live_t + 3 * n, x.base_t.data() + 3 * n, n * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

extern "C" int lpvmpc_set_disturbances(lpvmpc_handle *h, int32_t B, const lpvmpc_disturbance_config *cfg, const double *rows) {
    const char *who = "lpvmpc_set_disturbances";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    lpvmpc::DistDev t{};
    DistBinding *cur = dist_target(h, t);
    if (!cur)
        return fail(h, LPVMPC_E_ARG, "%s: the handle runs no lap-0 fleet or race with plant and tyre tables (start it through lpvmpc_cl_init_tyres / "
                    "lpvmpc_race_init_tyres; for a race pass the path handle): there is nothing to scale", who);
    if (B != t.B) return fail(h, LPVMPC_E_ARG, "%s: B=%d, but the handle's fleet has %d vehicles", who, B, t.B);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    if (!rows) {                                                           // detach
        HIP_TRY(h, hipStreamSynchronize(st));
        if (cur->d.rows) { int rc = dist_restore(h, *cur, st); if (rc) return rc; }
        *cur = DistBinding{};
        return LPVMPC_OK;
    }
    lpvmpc_disturbance_config c;
    lpvmpc_disturbance_default_config(&c);
    if (cfg) c = *cfg;
    std::vector<double> rows_dev;
    int rc = lpvmpc_dist_rows(h, B, &c, rows, who, rows_dev); if (rc) return rc;
    // built in x and installed after the last step that can fail
    const size_t n = B;
    DistBinding x;
    x.cfg = c;
    x.rows.assign(rows, rows + n * LPVMPC_DIST_WORDS);
    HIP_TRY(h, hipStreamSynchronize(st));                                  // no tick in flight writes the tables read below
    rc = lpvmpc_plant_base(h, *lpvmpc_plant_side(h), x.base_p, x.base_t, st); if (rc) return rc;
    x.d = t;
    dist_cfg(c, x.d);
    rc = dist_upload(h, B, rows_dev, nullptr, x.base_p, x.base_t, x, st); if (rc) return rc;
    if (cur->d.rows) { rc = dist_restore(h, x, st); if (rc) return rc; }
    *cur = std::move(x);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_disturbances_read(lpvmpc_handle *h, double *rows, double *state) {
    const char *who = "lpvmpc_disturbances_read";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    lpvmpc::DistDev t{};
    const DistBinding *cur = dist_target(h, t);
    if (!cur || !cur->d.rows) return fail(h, LPVMPC_E_ARG, "%s: no disturbances attached (lpvmpc_set_disturbances)", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t n = cur->d.B;
    std::vector<double> s(n * LPVMPC_DIST_STATE);
    D2H(s.data(), cur->d.state, s.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    if (rows) for (size_t i = 0; i < cur->rows.size(); ++i) rows[i] = cur->rows[i];
    if (state)
        for (size_t b = 0; b < n; ++b)
            for (size_t i = 0; i < LPVMPC_DIST_STATE; ++i) state[b * LPVMPC_DIST_STATE + i] = s[i * n + b];
    return LPVMPC_OK;
}

int lpvmpc_dist_step(lpvmpc_handle *h, int B, const DistStep &ds, const std::vector<double> &rows_dev, const std::vector<double> &plant_tab,
                     const std::vector<double> &tyre_tab, double *d_plant, const int32_t *d_k, int n_sub, double dt_sim, double *live_p,
                     double *live_t, DistBinding &tmp, hipStream_t st) {
    lpvmpc_race_config rc0;
    lpvmpc_race_default_config(&rc0);                                      // an unbound handle's map width for the transform
    int rc = dist_upload(h, B, rows_dev, ds.dist_state, plant_tab, tyre_tab, tmp, st); if (rc) return rc;
    lpvmpc::DistDev &d = tmp.d;
    d.plant = d_plant; d.k = d_k; d.nstep = nullptr; d.n_fixed = n_sub; d.dt = dt_sim; d.hw = rc0.half_width; d.slack = rc0.slack;
    d.live_p = live_p; d.live_t = live_t;
    dist_cfg(*ds.cfg, d);
    HIP_TRY(h, lpvmpc::launch_disturbance(h->d_cfg, lpvmpc_trk(h), d, st));
    return LPVMPC_OK;
}

int lpvmpc_dist_step_read(lpvmpc_handle *h, int B, const DistStep &ds, const DistBinding &tmp, hipStream_t st) {
    if (!ds.dist_state) return LPVMPC_OK;
    const size_t n = B;
    std::vector<double> s(n * LPVMPC_DIST_STATE);
    D2H(s.data(), tmp.d.state, s.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    for (size_t b = 0; b < n; ++b)
        for (size_t i = 0; i < LPVMPC_DIST_STATE; ++i) ds.dist_state[b * LPVMPC_DIST_STATE + i] = s[i * n + b];
    return LPVMPC_OK;
}

extern "C" int lpvmpc_plant_step_disturbed_batch(lpvmpc_handle *h, int32_t B, double *state, double *act_state, const double *u, int32_t n_sub,
                                                 double dt_sim, double mu_sim, const lpvmpc_actuator_config *act, const int32_t *delay_a,
                                                 const int32_t *delay_df, const double *plant_params, const double *tyre_params,
                                                 const lpvmpc_disturbance_config *cfg, const double *rows, double *dist_state) {
    const char *who = "lpvmpc_plant_step_disturbed_batch";
    if (h && B == 0) return LPVMPC_OK;
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (B < 0 || !rows) return fail(h, LPVMPC_E_ARG, "%s: B < 0 or rows is NULL", who);
    int rc = lpvmpc_need_track(h, who); if (rc) return rc;
    rc = lpvmpc_tracks_check(h, B, who); if (rc) return rc;
    if (dist_state)
        for (size_t b = 0; b < (size_t)B; ++b) {
            const double *s = dist_state + b * LPVMPC_DIST_STATE;
            if (!(s[3] >= 0 && s[3] < 9007199254740992.0) || s[3] != std::floor(s[3]))
                return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: tick count %g is not an integer >= 0", who, b, s[3]);
            for (int i = 0; i < 3; ++i)
                if (!std::isfinite(s[i])) return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: process word %d of dist_state = %g is not finite", who, b, i, s[i]);
        }
    lpvmpc_disturbance_config c;
    lpvmpc_disturbance_default_config(&c);
    if (cfg) c = *cfg;
    std::vector<double> tyr;
    rc = lpvmpc_tyre_rows(h, B, tyre_params, who, tyr); if (rc) return rc;
    const DistStep ds{&c, rows, dist_state};
    return lpvmpc_plant_step_rows(h, B, state, act_state, u, n_sub, dt_sim, mu_sim, act, delay_a, delay_df, plant_params, &tyr, who, &ds);
}
