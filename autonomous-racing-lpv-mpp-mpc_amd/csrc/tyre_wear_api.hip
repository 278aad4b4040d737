// tyre_wear_api.hip -- C ABI of the tyre wear and temperature (include/lpvmpc.h, "Tyre wear and temperature"): the checks, the binding
// of a lap-0 fleet or a race (PlantSide::wear of the running engine, lpvmpc_plant_side), the read-back, the tyre change and the
// stand-alone step's launch.  Kernel: tyre_wear.hip, launched behind the disturbances' and in front of the command / plant launch of
// lpvmpc_cl_tick, lpvmpc_race_tick and lpvmpc_plant_step_rows.
#include <algorithm>
#include <cmath>
#include <vector>

#include "lpvmpc_handle.hpp"

static_assert(lpvmpc::kWearWords == LPVMPC_WEAR_WORDS && lpvmpc::kWearState == LPVMPC_WEAR_STATE, "host rows and device tables hold the same words");

int lpvmpc_wear_rows(lpvmpc_handle *h, int B, const double *rows, int n_max, double dt_sim, const char *who, std::vector<double> &t) {
    static const char *names[LPVMPC_WEAR_WORDS] = {"k_wear", "k_hot", "k_heat", "k_cool", "T_amb", "T_opt", "k_temp", "wear_slope", "cliff_at",
                                                   "cliff_slope", "g_min", "T_start"};
    const size_t n = B;
    t.assign(n * LPVMPC_WEAR_WORDS, 0.0);
    for (size_t b = 0; b < n; ++b) {
        const double *r = rows + b * LPVMPC_WEAR_WORDS;
        for (int i = 0; i < LPVMPC_WEAR_WORDS; ++i) {
            const double v = r[i];
            bool ok = std::isfinite(v);
            if (ok && (i <= 3 || i == 6 || i == 7 || i == 9)) ok = v >= 0;
            else if (ok && i == 8) ok = v >= 0 && v <= 1;
            else if (ok && i == 10) ok = v > 0 && v <= 1;
            if (!ok)
                return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: %s = %g (every word finite; k_wear, k_hot, k_heat, k_cool, k_temp, wear_slope, "
                            "cliff_slope >= 0; cliff_at in [0, 1]; g_min in (0, 1])", who, b, names[i], v);
            t[(size_t)i * n + b] = v;
        }
        if (!(r[3] * (double)n_max * dt_sim < 1.0))
            return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: k_cool * n_max * dt_sim = %g * %d * %g >= 1: the temperature's Euler step would overshoot "
                        "the ambient", who, b, r[3], n_max, dt_sim);
    }
    return LPVMPC_OK;
}

// device tables of a binding in x.mem: rows, state (fresh: {0, T_start, 0, 1, 0, 0}; else the host layout [B][kWearState]) and the
// base words
static int wear_upload(lpvmpc_handle *h, int B, const std::vector<double> &rows_dev, const double *state, const std::vector<double> &base_p,
                       const std::vector<double> &base_t, WearBinding &x, hipStream_t st) {
    const size_t n = B;
    double *d_rows = nullptr, *d_state = nullptr, *d_base = nullptr;
    HIP_TRY(h, x.mem.alloc(d_rows, rows_dev.size() * 8));
    HIP_TRY(h, x.mem.alloc(d_state, n * LPVMPC_WEAR_STATE * 8));
    HIP_TRY(h, x.mem.alloc(d_base, n * 5 * 8));
    std::vector<double> s(n * LPVMPC_WEAR_STATE, 0.0), base(n * 5);
    for (size_t b = 0; b < n; ++b) {
        s[n + b] = rows_dev[11 * n + b]; s[3 * n + b] = 1.0;
        if (state) for (size_t i = 0; i < LPVMPC_WEAR_STATE; ++i) s[i * n + b] = state[b * LPVMPC_WEAR_STATE + i];
        base[b] = base_p[4 * n + b]; base[n + b] = base_p[5 * n + b]; base[2 * n + b] = base_t[3 * n + b];
        base[3 * n + b] = base_p[n + b]; base[4 * n + b] = base_p[2 * n + b];
    }
    H2D(d_rows, rows_dev.data(), rows_dev.size() * 8);
    H2D(d_state, s.data(), s.size() * 8);
    H2D(d_base, base.data(), base.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));                                  // the staging vectors end with this call
    x.d.rows = d_rows; x.d.state = d_state; x.d.base = d_base; x.d.B = B;
    return LPVMPC_OK;
}

// the plant side of the fleet or race that h runs and, in t, what its wear acts on with the engine's largest steps per tick in n_max
// (null: none with plant and tyre tables)
static PlantSide *wear_target(lpvmpc_handle *h, lpvmpc::WearDev &t, int &n_max) {
    const lpvmpc::RaceDev *race = nullptr;
    PlantSide *p = lpvmpc_plant_side(h, &race);
    if (!p || !p->veh.d.p || !p->tyre.t) return nullptr;
    t = lpvmpc::WearDev{};
    t.B = p->B; t.dt = p->pc.dt;
    t.live_p = const_cast<double *>(p->veh.d.p); t.live_t = const_cast<double *>(p->tyre.t);
    if (race) {                                                            // each vehicle steps RaceDev::nstep times in a tick
        t.plant = race->plant; t.nstep = race->nstep; t.n_fixed = 0;
        n_max = std::max(std::max(race->n_sub_lap0, race->n_sub[0]), std::max(race->n_sub[1], race->n_sub[2]));
    } else {
        t.plant = h->cl_plant; t.nstep = nullptr; t.n_fixed = p->pc.n_sub;
        n_max = p->pc.n_sub;
    }
    return p;
}

// the live tables' scaled words without the wear's factor: gamma * base where disturbances are attached (their gamma of the last
// disturbed tick), else base
static int wear_restore(lpvmpc_handle *h, const PlantSide &side, const WearBinding &x, hipStream_t st) {
    const size_t n = x.d.B;
    std::vector<double> gamma(n, 1.0), w(3 * n);
    if (side.dist.d.rows) {
        D2H(gamma.data(), side.dist.d.state + 4 * n, n * 8);
        HIP_TRY(h, hipStreamSynchronize(st));
    }
    for (size_t b = 0; b < n; ++b) {
        const double base[3] = {x.base_p[4 * n + b], x.base_p[5 * n + b], x.base_t[3 * n + b]};
        for (int i = 0; i < 3; ++i) w[i * n + b] = side.dist.d.rows ? gamma[b] * base[i] : base[i];
    }
    H2D(x.d.live_p + 4 * n, w.data(), 2 * n * 8);
    H2D(x.d.live_t + 3 * n, w.data() + 2 * n, n * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

extern "C" int lpvmpc_set_tyre_wear(lpvmpc_handle *h, int32_t B, const double *rows) {
    const char *who = "lpvmpc_set_tyre_wear";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    lpvmpc::WearDev t{};
    int n_max = 0;
    PlantSide *side = wear_target(h, t, n_max);
    if (!side)
        return fail(h, LPVMPC_E_ARG, "%s: the handle runs no lap-0 fleet or race with plant and tyre tables (start it through lpvmpc_cl_init_tyres / "
                    "lpvmpc_race_init_tyres; for a race pass the path handle): there is nothing to scale", who);
    if (B != t.B) return fail(h, LPVMPC_E_ARG, "%s: B=%d, but the handle's fleet has %d vehicles", who, B, t.B);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    WearBinding *cur = &side->wear;
    if (!rows) {                                                           // detach
        HIP_TRY(h, hipStreamSynchronize(st));
        if (cur->d.rows) { int rc = wear_restore(h, *side, *cur, st); if (rc) return rc; }
        *cur = WearBinding{};
        return LPVMPC_OK;
    }
    std::vector<double> rows_dev;
    int rc = lpvmpc_wear_rows(h, B, rows, n_max, t.dt, who, rows_dev); if (rc) return rc;
    // built in x and installed after the last step that can fail
    WearBinding x;
    HIP_TRY(h, hipStreamSynchronize(st));                                  // no tick in flight writes the tables read below
    rc = lpvmpc_plant_base(h, *side, x.base_p, x.base_t, st); if (rc) return rc;
    x.d = t;
    rc = wear_upload(h, B, rows_dev, nullptr, x.base_p, x.base_t, x, st); if (rc) return rc;
    if (cur->d.rows) { rc = wear_restore(h, *side, x, st); if (rc) return rc; }   // the state starts over: g = 1 until the next tick
    *cur = std::move(x);
    return LPVMPC_OK;
}

// the binding of the engine that h runs, or the refusal
static int wear_attached(lpvmpc_handle *h, const char *who, WearBinding *&cur) {
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    PlantSide *side = lpvmpc_plant_side(h);
    if (!side || !side->wear.d.rows) return fail(h, LPVMPC_E_ARG, "%s: no tyre wear attached (lpvmpc_set_tyre_wear)", who);
    cur = &side->wear;
    return LPVMPC_OK;
}

// word-major device table [W][n] <-> host layout [n][W]
static void to_host(const std::vector<double> &dev, size_t n, size_t W, double *out) {
    for (size_t b = 0; b < n; ++b)
        for (size_t i = 0; i < W; ++i) out[b * W + i] = dev[i * n + b];
}

extern "C" int lpvmpc_tyre_wear_read(lpvmpc_handle *h, double *rows, double *state) {
    const char *who = "lpvmpc_tyre_wear_read";
    WearBinding *cur = nullptr;
    int rc = wear_attached(h, who, cur); if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t n = cur->d.B;
    std::vector<double> r(n * LPVMPC_WEAR_WORDS), s(n * LPVMPC_WEAR_STATE);
    D2H(r.data(), cur->d.rows, r.size() * 8);
    D2H(s.data(), cur->d.state, s.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    if (rows) to_host(r, n, LPVMPC_WEAR_WORDS, rows);
    if (state) to_host(s, n, LPVMPC_WEAR_STATE, state);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_tyre_wear_fit(lpvmpc_handle *h, const int32_t *mask) {
    const char *who = "lpvmpc_tyre_wear_fit";
    WearBinding *cur = nullptr;
    int rc = wear_attached(h, who, cur); if (rc) return rc;
    if (!mask) return fail(h, LPVMPC_E_ARG, "%s: mask is NULL", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t n = cur->d.B;
    std::vector<double> T_start(n), s(n * 4);                              // W, T, P, g: the first four state words
    D2H(T_start.data(), cur->d.rows + 11 * n, n * 8);
    D2H(s.data(), cur->d.state, s.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));                                  // between ticks: none in flight writes the state
    for (size_t b = 0; b < n; ++b)
        if (mask[b]) { s[b] = 0.0; s[n + b] = T_start[b]; s[2 * n + b] = 0.0; s[3 * n + b] = 1.0; }
    H2D(cur->d.state, s.data(), s.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

int lpvmpc_wear_step(lpvmpc_handle *h, int B, const WearStep &ws, const std::vector<double> &rows_dev, const std::vector<double> &plant_tab,
                     const std::vector<double> &tyre_tab, const double *d_plant, const double *gamma, int n_sub, double dt_sim, double *live_p,
                     double *live_t, WearBinding &tmp, hipStream_t st) {
    int rc = wear_upload(h, B, rows_dev, ws.wear_state, plant_tab, tyre_tab, tmp, st); if (rc) return rc;
    lpvmpc::WearDev &d = tmp.d;
    d.plant = d_plant; d.gamma = gamma; d.nstep = nullptr; d.n_fixed = n_sub; d.dt = dt_sim; d.live_p = live_p; d.live_t = live_t;
    HIP_TRY(h, lpvmpc::launch_tyre_wear(d, st));
    return LPVMPC_OK;
}

int lpvmpc_wear_step_read(lpvmpc_handle *h, int B, const WearStep &ws, const WearBinding &tmp, hipStream_t st) {
    if (!ws.wear_state) return LPVMPC_OK;
    const size_t n = B;
    std::vector<double> s(n * LPVMPC_WEAR_STATE);
    D2H(s.data(), tmp.d.state, s.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    to_host(s, n, LPVMPC_WEAR_STATE, ws.wear_state);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_plant_step_worn_batch(lpvmpc_handle *h, int32_t B, double *state, double *act_state, const double *u, int32_t n_sub,
                                            double dt_sim, double mu_sim, const lpvmpc_actuator_config *act, const int32_t *delay_a,
                                            const int32_t *delay_df, const double *plant_params, const double *tyre_params,
                                            const lpvmpc_disturbance_config *cfg, const double *rows, double *dist_state,
                                            const double *wear_rows, double *wear_state) {
    const char *who = "lpvmpc_plant_step_worn_batch";
    if (h && B == 0) return LPVMPC_OK;
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (B < 0 || !wear_rows) return fail(h, LPVMPC_E_ARG, "%s: B < 0 or wear_rows is NULL", who);
    if (rows) {                                                            // the disturbances' transform reads the track
        int rc = lpvmpc_need_track(h, who); if (rc) return rc;
        rc = lpvmpc_tracks_check(h, B, who); if (rc) return rc;
    }
    if (wear_state)
        for (size_t b = 0; b < (size_t)B; ++b) {
            const double *s = wear_state + b * LPVMPC_WEAR_STATE;
            for (int i = 0; i < LPVMPC_WEAR_STATE; ++i)
                if (!std::isfinite(s[i])) return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: word %d of wear_state = %g is not finite", who, b, i, s[i]);
            if (!(s[4] >= 0 && s[4] < 9007199254740992.0) || s[4] != std::floor(s[4]))
                return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: tick count %g is not an integer >= 0", who, b, s[4]);
        }
    lpvmpc_disturbance_config c;
    lpvmpc_disturbance_default_config(&c);
    if (cfg) c = *cfg;
    std::vector<double> tyr;
    int rc = lpvmpc_tyre_rows(h, B, tyre_params, who, tyr); if (rc) return rc;
    const DistStep ds{&c, rows, dist_state};
    const WearStep ws{wear_rows, wear_state};
    return lpvmpc_plant_step_rows(h, B, state, act_state, u, n_sub, dt_sim, mu_sim, act, delay_a, delay_df, plant_params, &tyr, who,
                                  rows ? &ds : nullptr, &ws);
}
