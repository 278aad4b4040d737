// tunings_api.hip -- C ABI of the per-vehicle tunings (include/lpvmpc.h, "Per-vehicle tunings"): the public row and the device row
// of a tuning, the handle's table of device rows, its checks and the read-back.  The binding acts through SolveArgs::tune, which
// lpvmpc_launch_solve_timed -- the one place every main solve launch of every route comes through -- fills with lpvmpc_solve_tune;
// the kernel reads the row in the set-up block of Solver::run (admm_solve.hip) and nowhere else.
#include <cmath>
#include <cstring>
#include <vector>

#include "lpvmpc_handle.hpp"

static_assert(lpvmpc::kTuneWords == LPVMPC_TUNING_WORDS, "public rows, device rows and the configuration's block hold the same number of words");

enum { kW_Q = 0, kW_R = 36, kW_dR = 40, kW_Lcf = 42, kW_lim = 48 };

extern "C" int lpvmpc_tuning_from_config(const lpvmpc_config *cfg, double *row) {
    if (!cfg || !row) return fail(nullptr, LPVMPC_E_ARG, "lpvmpc_tuning_from_config: NULL argument");
    if (cfg->kind != LPVMPC_KIND_CONTROLLER && cfg->kind != LPVMPC_KIND_PLANNER) return fail(nullptr, LPVMPC_E_ARG, "lpvmpc_tuning_from_config: bad kind %d", cfg->kind);
    std::memset(row, 0, sizeof(double) * LPVMPC_TUNING_WORDS);
    std::memcpy(row + kW_Q, cfg->Q, sizeof(cfg->Q)); std::memcpy(row + kW_R, cfg->R, sizeof(cfg->R));
    std::memcpy(row + kW_dR, cfg->dR, sizeof(cfg->dR)); std::memcpy(row + kW_Lcf, cfg->L_cf, sizeof(cfg->L_cf));
    double *lim = row + kW_lim;
    if (cfg->kind == LPVMPC_KIND_CONTROLLER) {
        lim[0] = cfg->ctrl_vx_min; lim[1] = cfg->max_vel; lim[2] = cfg->ctrl_delta_max; lim[3] = cfg->ctrl_a_max; lim[4] = cfg->ctrl_a_min_abs;
    } else {
        for (int r = 0; r < 5; ++r) { lim[r] = cfg->plan_xmin[r]; lim[5 + r] = cfg->plan_xmax[r]; }
        lim[0] = cfg->min_vel; lim[5] = cfg->max_vel;                           // PLAN:176-177
        for (int r = 0; r < 2; ++r) { lim[10 + r] = cfg->plan_umin[r]; lim[12 + r] = cfg->plan_umax[r]; }
    }
    return LPVMPC_OK;
}

extern "C" int lpvmpc_tuning_device_row(int32_t kind, const double *row, double *dev) {
    if (!row || !dev) return fail(nullptr, LPVMPC_E_ARG, "lpvmpc_tuning_device_row: NULL argument");
    if (kind != LPVMPC_KIND_CONTROLLER && kind != LPVMPC_KIND_PLANNER) return fail(nullptr, LPVMPC_E_ARG, "lpvmpc_tuning_device_row: bad kind %d", kind);
    std::memcpy(dev, row, sizeof(double) * kW_lim);                             // Q R dR Lcf: the configuration's words as they are
    const double *lim = row + kW_lim;
    double *lo = dev + lpvmpc::kTuneLo, *hi = dev + lpvmpc::kTuneHi;
    for (int r = 0; r < 8; ++r) lo[r] = hi[r] = 0.0;
    const double inf = INFINITY;
    if (kind == LPVMPC_KIND_CONTROLLER) {
        // rows: -vx <= -vx_min, vx <= max_vel, d <= dmax, -d <= dmax, a <= amax, -a <= amin   (CTRL:334-348)
        const double h6[6] = {-lim[0], lim[1], lim[2], lim[2], lim[3], lim[4]};
        for (int r = 0; r < 6; ++r) { lo[r] = -inf; hi[r] = h6[r]; }
    } else {
        for (int r = 0; r < 5; ++r) { lo[r] = lim[r]; hi[r] = lim[5 + r]; }
        for (int r = 0; r < 2; ++r) { lo[5 + r] = lim[10 + r]; hi[5 + r] = lim[12 + r]; }
    }
    return LPVMPC_OK;
}

// the rules of lpvmpc_set_tunings for one public row; returns null or what is wrong with it
static const char *row_fault(int kind, const double *w) {
    const bool ctrl = kind == LPVMPC_KIND_CONTROLLER;
    const int nx = ctrl ? 6 : 5;
    for (int i = 0; i < nx * nx; ++i) if (!std::isfinite(w[kW_Q + i])) return "a non-finite word of Q";
    for (int i = 0; i < 4; ++i) if (!std::isfinite(w[kW_R + i])) return "a non-finite word of R";
    for (int i = 0; i < 2; ++i) if (!std::isfinite(w[kW_dR + i])) return "a non-finite word of dR";
    const double *lim = w + kW_lim;
    if (ctrl) {
        for (int i = 0; i < 5; ++i) if (std::isnan(lim[i])) return "a NaN limit";
        if (lim[0] > lim[1]) return "vx_min > max_vel";
        if (lim[2] < 0) return "delta_max < 0";
        if (lim[3] < -lim[4]) return "a_max < -a_min_abs";
    } else {
        for (int i = 0; i < nx; ++i) if (!std::isfinite(w[kW_Lcf + i])) return "a non-finite word of L_cf";
        for (int r = 0; r < 5; ++r) {
            if (r == 3) continue;                                               // ey: the per-instance max_ey
            if (std::isnan(lim[r]) || std::isnan(lim[5 + r])) return "a NaN limit";
            if (lim[r] > lim[5 + r]) return "xmin > xmax";
        }
        for (int r = 0; r < 2; ++r) {
            if (std::isnan(lim[10 + r]) || std::isnan(lim[12 + r])) return "a NaN limit";
            if (lim[10 + r] > lim[12 + r]) return "umin > umax";
        }
    }
    return nullptr;
}

int lpvmpc_tuning_check(lpvmpc_handle *h, int B, const char *who) {
    if (h->d_tune && h->tune_B != B)
        return fail(h, LPVMPC_E_ARG, "%s: B=%d, but the handle has tuning rows for %d instances bound (lpvmpc_set_tunings)", who, B, h->tune_B);
    return LPVMPC_OK;
}

int lpvmpc_solve_tune(lpvmpc_handle *h, SolveArgs &a) {
    a.tune = nullptr;
    if (!h->d_tune || a.resume == 1) return LPVMPC_OK;                          // (a resume pass sets nothing up: the parked image carries the words)
    if (a.B != h->tune_B)                                                       // the entry points have refused it already: never launch past the table
        return fail(h, LPVMPC_E_ARG, "solve launch of %d instances, but the handle has tuning rows for %d bound (lpvmpc_set_tunings)", a.B, h->tune_B);
    a.tune = h->d_tune;
    return LPVMPC_OK;
}

extern "C" int lpvmpc_join(lpvmpc_handle *h, void *stream);

extern "C" int lpvmpc_set_tunings(lpvmpc_handle *h, int32_t B, const double *rows) {
    const char *who = "lpvmpc_set_tunings";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (busy(h))
        return fail(h, LPVMPC_E_ARG, "%s: this handle runs a %s; bind the tuning rows before it starts (lpvmpc_cl_release ends it)", who,
                    h->cl_plant ? "closed-loop fleet" : (h->race || h->race_owner) ? "race" : "planner + controller cascade");
    if (B < 0) return fail(h, LPVMPC_E_ARG, "%s: B=%d", who, B);
    if (B > 0 && !rows) return fail(h, LPVMPC_E_ARG, "%s: rows is NULL (B = 0 unbinds)", who);
    const size_t W = LPVMPC_TUNING_WORDS;
    std::vector<double> dev((size_t)B * W);
    for (int b = 0; b < B; ++b) {
        const char *what = row_fault(h->cfg.kind, rows + (size_t)b * W);
        if (what) return fail(h, LPVMPC_E_ARG, "%s: row %d: %s", who, b, what);
        lpvmpc_tuning_device_row(h->cfg.kind, rows + (size_t)b * W, dev.data() + (size_t)b * W);
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // what is parked finishes first (its launches are ordered on the stream of the last deferred call), then the device is idle:
    // no launch reads the old table when it is freed
    if (h->dpool[0]) {
        int rc = lpvmpc_join(h, (void *)(h->defer_stream_set ? h->defer_stream : h->stream)); if (rc) return rc;
    }
    HIP_TRY(h, hipDeviceSynchronize());
    TuneTable t;                                                         // B = 0: none
    if (B > 0) {
        HIP_TRY(h, t.tune_mem.alloc(t.d_tune, dev.size() * 8));
        if (hipMemcpy(t.d_tune, dev.data(), dev.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
            return fail(h, LPVMPC_E_HIP, "%s: uploading the rows failed", who);
        t.tune_B = B;
        t.tune_rows.assign(rows, rows + (size_t)B * W);
    }
    static_cast<TuneTable &>(*h) = std::move(t);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_tunings_read(lpvmpc_handle *h, int32_t *B, double *rows) {
    const char *who = "lpvmpc_tunings_read";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (!B) return fail(h, LPVMPC_E_ARG, "%s: B is NULL", who);
    *B = h->d_tune ? h->tune_B : 0;
    if (h->d_tune && rows) std::memcpy(rows, h->tune_rows.data(), h->tune_rows.size() * 8);
    return LPVMPC_OK;
}
