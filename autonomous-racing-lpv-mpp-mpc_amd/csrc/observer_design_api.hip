// observer_design_api.hip -- C ABI of the per-vehicle state estimator (include/lpvmpc.h, "Per-vehicle state estimator"): the checks of
// a gain design (weights, limit tables, vehicle rows), its constant block and the stand-alone design call; the handle's binding of
// model rows and gain tables per vehicle, its read-back and the stand-alone observer step.  The binding acts where a fleet or race
// started by the _vehicles / _tyres calls launches its estimator kernel (lpvmpc_cl_tick, lpvmpc_race_tick).
// Kernels: observer_design.hip, observer_vehicles.hip.
#include <cmath>
#include <cstring>
#include <vector>

#include "lpvmpc_handle.hpp"
#include "observer_design.hpp"

using lpvmpc::ObsDesignConst;

static int lpvmpc_observer_design_const(lpvmpc_handle *h, const lpvmpc_observer_design *d, const char *who, double *cst);

extern "C" void lpvmpc_observer_default_design(lpvmpc_observer_design *d) {
    if (!d) return;
    std::memset(d, 0, sizeof(*d));
    for (int i = 0; i < 6; ++i) d->Qo[i * 6 + i] = 1.0;
    const double r[5] = {0.1, 0.1, 0.01, 0.01, 0.01};
    for (int i = 0; i < 5; ++i) d->Ro[i * 5 + i] = r[i];
}

namespace {

// a [n][n] finite and symmetric to rounding
bool symmetric(const double *a, int n) {
    double big = 0.0;
    for (int i = 0; i < n * n; ++i) { if (!std::isfinite(a[i])) return false; big = std::fmax(big, std::fabs(a[i])); }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) if (std::fabs(a[i * n + j] - a[j * n + i]) > 1e-12 * big) return false;
    return true;
}
// lower Cholesky factor of the symmetric part of a [n][n] in c; false: not positive definite
bool cholesky(const double *a, int n, double *c) {
    for (int j = 0; j < n; ++j) {
        double d = a[j * n + j];
        for (int k = 0; k < j; ++k) d -= c[j * n + k] * c[j * n + k];
        if (!(d > 0.0)) return false;
        c[j * n + j] = d = std::sqrt(d);
        for (int i = j + 1; i < n; ++i) {
            double s = 0.5 * (a[i * n + j] + a[j * n + i]);
            for (int k = 0; k < j; ++k) s -= c[i * n + k] * c[j * n + k];
            c[i * n + j] = s / d;
        }
    }
    return true;
}

}  // namespace

// checks a design and fills the constant block of its kernel
static int lpvmpc_observer_design_const(lpvmpc_handle *h, const lpvmpc_observer_design *d, const char *who, double *cst) {
    if (!symmetric(d->Ro, 5)) return fail(h, LPVMPC_E_ARG, "%s: Ro is not a finite symmetric table", who);
    if (!symmetric(d->Qo, 6)) return fail(h, LPVMPC_E_ARG, "%s: Qo is not a finite symmetric table", who);
    double c[36];
    if (!cholesky(d->Ro, 5, c)) return fail(h, LPVMPC_E_ARG, "%s: Ro is not positive definite", who);
    // Qo positive SEMI-definite: Qo + eps |Qo| I must factor (a zero table passes)
    double big = 0.0, q[36];
    for (int i = 0; i < 36; ++i) big = std::fmax(big, std::fabs(d->Qo[i]));
    std::memcpy(q, d->Qo, sizeof(q));
    for (int i = 0; i < 6; ++i) q[i * 6 + i] += 1e-10 * big + 1e-300;
    double cq[36];
    if (!cholesky(q, 6, cq)) return fail(h, LPVMPC_E_ARG, "%s: Qo is not positive semidefinite", who);
    // Ro^-1 from the factor: column j solves C C^T x = e_j
    double Ri[25];
    for (int j = 0; j < 5; ++j) {
        double x[5];
        for (int i = 0; i < 5; ++i) {
            double s = i == j ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) s -= c[i * 5 + k] * x[k];
            x[i] = s / c[i * 5 + i];
        }
        for (int i = 4; i >= 0; --i) {
            double s = x[i];
            for (int k = i + 1; k < 5; ++k) s -= c[k * 5 + i] * x[k];
            x[i] = s / c[i * 5 + i];
        }
        for (int i = 0; i < 5; ++i) Ri[i * 5 + j] = x[i];
    }
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < i; ++j) Ri[i * 5 + j] = Ri[j * 5 + i] = 0.5 * (Ri[i * 5 + j] + Ri[j * 5 + i]);
    for (int p = 0; p < 2; ++p) {
        const double *lim = p ? d->lim_hs : d->lim_ls;
        const char *name = p ? "lim_hs" : "lim_ls";
        for (int i = 0; i < 12; ++i) if (!std::isfinite(lim[i])) return fail(h, LPVMPC_E_ARG, "%s: %s holds a non-finite word", who, name);
        for (int row : {0, 1, 3, 5})
            if (!(lim[row * 2 + 1] > lim[row * 2])) return fail(h, LPVMPC_E_ARG, "%s: %s row %d: max %g <= min %g", who, name, row, lim[row * 2 + 1], lim[row * 2]);
        if (!(lim[0] > 0.0)) return fail(h, LPVMPC_E_ARG, "%s: %s: the lower vx limit %g must be > 0", who, name, lim[0]);
    }
    static const int meas[6] = {0, -1, 1, 2, 3, 4};                        // state -> measurement (C selects states 0, 2, 3, 4, 5)
    std::memset(cst, 0, sizeof(double) * ObsDesignConst::kWords);
    for (int i = 0; i < 36; ++i) cst[ObsDesignConst::kQo + i] = 0.5 * (d->Qo[i] + d->Qo[(i % 6) * 6 + i / 6]);
    for (int a = 0; a < 6; ++a) {
        if (meas[a] < 0) continue;
        for (int b = 0; b < 6; ++b) if (meas[b] >= 0) cst[ObsDesignConst::kG + a * 6 + b] = Ri[meas[a] * 5 + meas[b]];
        for (int k = 0; k < 5; ++k) cst[ObsDesignConst::kCtRi + a * 5 + k] = Ri[meas[a] * 5 + k];
    }
    std::memcpy(cst + ObsDesignConst::kLim, d->lim_ls, sizeof(double) * 12);
    std::memcpy(cst + ObsDesignConst::kLim + 12, d->lim_hs, sizeof(double) * 12);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_observer_design_batch(lpvmpc_handle *h, int32_t B, const double *rows, const lpvmpc_observer_design *d, double *L_ls,
                                            double *L_hs, int32_t *iters) {
    const char *who = "lpvmpc_observer_design_batch";
    if (h && B == 0) return LPVMPC_OK;                                   // an empty batch is a no-op
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (busy(h))
        return fail(h, LPVMPC_E_ARG, "%s: this handle runs a fleet, cascade or race; use another handle for batch calls (lpvmpc_cl_release ends it)", who);
    if (B < 0 || B > LPVMPC_OBSERVER_DESIGN_MAX_B) return fail(h, LPVMPC_E_ARG, "%s: B=%d (1..%d)", who, B, LPVMPC_OBSERVER_DESIGN_MAX_B);
    if (!rows || !d || !L_ls || !L_hs) return fail(h, LPVMPC_E_ARG, "%s: bad argument", who);
    std::vector<double> tab;                                             // (the checks of the plant rows; the kernel reads the host layout)
    int rc = lpvmpc_plant_rows(h, B, rows, h->cfg, 0.0, who, tab); if (rc) return rc;
    double cst[ObsDesignConst::kWords];
    rc = lpvmpc_observer_design_const(h, d, who, cst); if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    DevArena mem;                                                        // (freed when the call returns)
    const size_t b = B;
    double *d_rows = nullptr, *d_cst = nullptr, *d_L = nullptr;
    int32_t *d_it = nullptr;
    HIP_TRY(h, mem.alloc(d_rows, b * LPVMPC_PLANT_WORDS * 8));
    HIP_TRY(h, mem.alloc(d_cst, sizeof(cst)));
    HIP_TRY(h, mem.alloc(d_L, b * 960 * 8));
    HIP_TRY(h, mem.alloc(d_it, b * 32 * 4));
    hipStream_t st = h->stream;
    auto run = [&]() -> int {
        H2D(d_rows, rows, b * LPVMPC_PLANT_WORDS * 8);
        H2D(d_cst, cst, sizeof(cst));
        HIP_TRY(h, lpvmpc::launch_observer_design(B, d_rows, d_cst, d_L, d_L + b * 480, 480, 16, 1, d_it, st));
        D2H(L_ls, d_L, b * 480 * 8);
        D2H(L_hs, d_L + b * 480, b * 480 * 8);
        if (iters) D2H(iters, d_it, b * 32 * 4);
        HIP_TRY(h, hipStreamSynchronize(st));
        return LPVMPC_OK;
    };
    rc = run();
    (void)hipStreamSynchronize(st);                                      // nothing of this call is in flight when its memory goes
    return rc;
}

// ---- the binding: model rows and gain tables per vehicle, on the handle ---------------------------------------------------
int lpvmpc_observer_vehicles_check(lpvmpc_handle *h, int B, const lpvmpc_observer_config *obs, bool honoured, const char *who) {
    if (!h->ov.L) return LPVMPC_OK;
    if (!honoured)
        return fail(h, LPVMPC_E_ARG, "%s: the handle has a per-vehicle estimator bound (lpvmpc_set_observer_vehicles), which only the _vehicles and _tyres "
                                     "starts of a fleet or race run; unbind it (B = 0) or start with one of those", who);
    if (h->ov_B != B)
        return fail(h, LPVMPC_E_ARG, "%s: B=%d, but the handle has a per-vehicle estimator for %d vehicles bound (lpvmpc_set_observer_vehicles)", who, B, h->ov_B);
    if (h->ov_designed && (std::memcmp(h->ov_lim, obs->lim_ls, sizeof(double) * 12) != 0 || std::memcmp(h->ov_lim + 12, obs->lim_hs, sizeof(double) * 12) != 0))
        return fail(h, LPVMPC_E_ARG, "%s: the bound gain tables were designed on other limit tables than the estimator configuration's", who);
    return LPVMPC_OK;
}

namespace {

// host [B][480] -> device plane [480][B] of one polytope (refuses a non-finite word), and back
int planes_from_host(lpvmpc_handle *h, const char *who, const char *name, size_t B, const double *L, double *plane) {
    for (size_t b = 0; b < B; ++b)
        for (size_t e = 0; e < 480; ++e) {
            const double v = L[b * 480 + e];
            if (!std::isfinite(v)) return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: %s[%zu] = %g is not finite", who, b, name, e, v);
            plane[e * B + b] = v;
        }
    return LPVMPC_OK;
}

// the device tables of a binding in t, from explicit tables or designed in place; iters (device, [B][2][16]) only with a design
int build_tables(lpvmpc_handle *h, const char *who, int32_t B, const double *rows, const double *L_ls, const double *L_hs,
                 const lpvmpc_observer_design *design, ObsVehTable &t) {
    std::vector<double> tab;                                             // [7][B], checked by the plant rows' rules
    int rc = lpvmpc_plant_rows(h, B, rows, h->cfg, 0.0, who, tab); if (rc) return rc;
    double cst[ObsDesignConst::kWords];
    if (design) { rc = lpvmpc_observer_design_const(h, design, who, cst); if (rc) return rc; }
    const size_t b = B;
    std::vector<double> planes;
    if (!design) {
        planes.resize(2 * 480 * b);
        rc = planes_from_host(h, who, "L_ls", b, L_ls, planes.data()); if (rc) return rc;
        rc = planes_from_host(h, who, "L_hs", b, L_hs, planes.data() + 480 * b); if (rc) return rc;
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    double *d_rows = nullptr, *d_L = nullptr;
    HIP_TRY(h, t.ov_mem.alloc(d_rows, tab.size() * 8));
    HIP_TRY(h, t.ov_mem.alloc(d_L, 2 * 480 * b * 8));
    hipStream_t st = h->stream;
    H2D(d_rows, tab.data(), tab.size() * 8);
    if (!design) {
        H2D(d_L, planes.data(), planes.size() * 8);
        HIP_TRY(h, hipStreamSynchronize(st));
    } else {
        DevArena tmp;                                                    // the kernel's inputs in the host layout and its iteration counts
        double *d_in = nullptr, *d_cst = nullptr;
        int32_t *d_it = nullptr;
        HIP_TRY(h, tmp.alloc(d_in, b * LPVMPC_PLANT_WORDS * 8));
        HIP_TRY(h, tmp.alloc(d_cst, sizeof(cst)));
        HIP_TRY(h, tmp.alloc(d_it, b * 32 * 4));
        std::vector<int32_t> it(b * 32);
        auto run = [&]() -> int {
            H2D(d_in, rows, b * LPVMPC_PLANT_WORDS * 8);
            H2D(d_cst, cst, sizeof(cst));
            HIP_TRY(h, lpvmpc::launch_observer_design(B, d_in, d_cst, d_L, d_L + 480 * b, 1, 16 * (long long)b, (long long)b, d_it, st));
            D2H(it.data(), d_it, it.size() * 4);
            HIP_TRY(h, hipStreamSynchronize(st));
            return LPVMPC_OK;
        };
        rc = run();
        (void)hipStreamSynchronize(st);
        if (rc) return rc;
        for (size_t q = 0; q < it.size(); ++q)
            if (it[q] < 1)
                return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: the gain design did not converge at vertex %zu of the %s polytope", who, q / 32, q % 16,
                            (q / 16) % 2 ? "high-speed" : "low-speed");
        t.ov_designed = true;
        std::memcpy(t.ov_lim, design->lim_ls, sizeof(double) * 12);
        std::memcpy(t.ov_lim + 12, design->lim_hs, sizeof(double) * 12);
    }
    t.ov.rows = d_rows; t.ov.L = d_L; t.ov.B = B; t.ov_B = B;
    return LPVMPC_OK;
}

}  // namespace

extern "C" int lpvmpc_set_observer_vehicles(lpvmpc_handle *h, int32_t B, const double *rows, const double *L_ls, const double *L_hs,
                                            const lpvmpc_observer_design *design) {
    const char *who = "lpvmpc_set_observer_vehicles";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (h->cfg.kind != LPVMPC_KIND_CONTROLLER) return fail(h, LPVMPC_E_ARG, "%s: controller handles only (for a race: the path handle)", who);
    if (busy(h))
        return fail(h, LPVMPC_E_ARG, "%s: this handle runs a %s; bind the estimator rows before it starts (lpvmpc_cl_release ends it)", who,
                    h->cl_plant ? "closed-loop fleet" : (h->race || h->race_owner) ? "race" : "planner + controller cascade");
    if (B < 0 || B > LPVMPC_OBSERVER_DESIGN_MAX_B) return fail(h, LPVMPC_E_ARG, "%s: B=%d (0..%d)", who, B, LPVMPC_OBSERVER_DESIGN_MAX_B);
    ObsVehTable t;                                                       // B = 0: none
    if (B > 0) {
        if (!rows) return fail(h, LPVMPC_E_ARG, "%s: rows is NULL (B = 0 unbinds)", who);
        if ((L_ls != nullptr) != (L_hs != nullptr) || (L_ls != nullptr) == (design != nullptr))
            return fail(h, LPVMPC_E_ARG, "%s: give either both gain tables or a design, not both and not neither", who);
        int rc = build_tables(h, who, B, rows, L_ls, L_hs, design, t); if (rc) return rc;
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    static_cast<ObsVehTable &>(*h) = std::move(t);                       // (freeing the old tables waits for the launches that read them)
    return LPVMPC_OK;
}

// device [7][B], [2][480][B] -> host [B][7], [B][480] twice
extern "C" int lpvmpc_observer_vehicles_read(lpvmpc_handle *h, int32_t *B, double *rows, double *L_ls, double *L_hs) {
    const char *who = "lpvmpc_observer_vehicles_read";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (!B) return fail(h, LPVMPC_E_ARG, "%s: B is NULL", who);
    *B = h->ov.L ? h->ov_B : 0;
    if (!h->ov.L || (!rows && !L_ls && !L_hs)) return LPVMPC_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t n = h->ov_B;
    std::vector<double> t(n * (rows ? LPVMPC_PLANT_WORDS : 0)), g(n * 960);
    if (rows) HIP_TRY(h, hipMemcpy(t.data(), h->ov.rows, t.size() * 8, hipMemcpyDeviceToHost));
    if (L_ls || L_hs) HIP_TRY(h, hipMemcpy(g.data(), h->ov.L, g.size() * 8, hipMemcpyDeviceToHost));
    for (size_t b = 0; b < n; ++b) {
        if (rows) for (size_t i = 0; i < LPVMPC_PLANT_WORDS; ++i) rows[b * LPVMPC_PLANT_WORDS + i] = t[i * n + b];
        if (L_ls) for (size_t e = 0; e < 480; ++e) L_ls[b * 480 + e] = g[e * n + b];
        if (L_hs) for (size_t e = 0; e < 480; ++e) L_hs[b * 480 + e] = g[(480 + e) * n + b];
    }
    return LPVMPC_OK;
}

// lpvmpc_observer_step_batch with a model row and gain tables per instance
extern "C" int lpvmpc_observer_step_vehicles_batch(lpvmpc_handle *h, int32_t B, const lpvmpc_observer_config *cfg, double *est, const double *y,
                                                   const double *u, const int32_t *k, double *aux, const double *rows, const double *L_ls,
                                                   const double *L_hs) {
    const char *who = "lpvmpc_observer_step_vehicles_batch";
    if (h && B == 0) return LPVMPC_OK;                                   // an empty batch is a no-op
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (busy(h))
        return fail(h, LPVMPC_E_ARG, "%s: this handle runs a fleet, cascade or race; use another handle for batch calls (lpvmpc_cl_release ends it)", who);
    if (B < 0 || B > LPVMPC_OBSERVER_DESIGN_MAX_B) return fail(h, LPVMPC_E_ARG, "%s: B=%d", who, B);
    if (!cfg || !est || !y || !u || !k || !rows || !L_ls || !L_hs) return fail(h, LPVMPC_E_ARG, "%s: bad argument", who);
    int rc = lpvmpc_observer_check(h, cfg, who); if (rc) return rc;
    ObsVehTable t;                                                       // (all freed when the call returns)
    rc = build_tables(h, who, B, rows, L_ls, L_hs, nullptr, t); if (rc) return rc;
    const size_t b = B;
    DevArena mem;
    double *d_g = nullptr, *d_est = nullptr, *d_y = nullptr, *d_u = nullptr, *d_aux = nullptr;
    int32_t *d_k = nullptr;
    HIP_TRY(h, mem.alloc(d_g, sizeof(double) * 2 * (lpvmpc::kObsTable + 12)));
    HIP_TRY(h, mem.alloc(d_est, b * 6 * 8)); HIP_TRY(h, mem.alloc(d_y, b * 5 * 8)); HIP_TRY(h, mem.alloc(d_u, b * 2 * 8));
    HIP_TRY(h, mem.alloc(d_k, b * 4));
    if (aux) HIP_TRY(h, mem.alloc(d_aux, b * lpvmpc::kObsAux * 8));
    hipStream_t st = h->stream;
    auto run = [&]() -> int {
        H2D(d_g, cfg->L_ls, sizeof(double) * 2 * (lpvmpc::kObsTable + 12));
        H2D(d_est, est, b * 6 * 8); H2D(d_y, y, b * 5 * 8); H2D(d_u, u, b * 2 * 8); H2D(d_k, k, b * 4);
        lpvmpc::ObsVehGains v; static_cast<lpvmpc::ObsVehDev &>(v) = t.ov; v.g = d_g;
        HIP_TRY(h, lpvmpc::launch_observer_step_vehicles(v, B, d_est, d_y, d_u, d_k, 1.0 / cfg->loop_rate, d_aux, st));
        D2H(est, d_est, b * 6 * 8);
        if (aux) D2H(aux, d_aux, b * lpvmpc::kObsAux * 8);
        HIP_TRY(h, hipStreamSynchronize(st));
        return LPVMPC_OK;
    };
    rc = run();
    (void)hipStreamSynchronize(st);
    return rc;
}
