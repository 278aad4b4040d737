// tyre_api.hip -- C ABI of the tyre model (include/lpvmpc.h, "Tyre model"): the checks and device table shared by the fleet entry
// points, the stand-alone batch calls and the read-back.  The fleet and race starts are lpvmpc_cl_init_rows (lpvmpc_api.hip) and
// lpvmpc_race_init_rows (race_api.hip), the stand-alone step lpvmpc_plant_step_rows (plant_params_api.hip), each shared with its
// _vehicles call.  Kernels: the <true, true, true> forms of fleet_kernels.hpp, launched from tyre.hip.
#include <cmath>
#include <vector>

#include "lpvmpc_handle.hpp"

static_assert(lpvmpc::kTyreWords == LPVMPC_TYRE_WORDS, "host rows and device table hold the same words");

int lpvmpc_tyre_rows(lpvmpc_handle *h, int B, const double *rows, const char *who, std::vector<double> &t) {
    static const char *names[LPVMPC_TYRE_WORDS] = {"kind", "B", "C", "c_f"};
    const size_t n = B;
    t.assign(n * LPVMPC_TYRE_WORDS, 0.0);                              // rows == null: kind 0 everywhere
    if (!rows) return LPVMPC_OK;
    for (size_t b = 0; b < n; ++b)
        for (int i = 0; i < LPVMPC_TYRE_WORDS; ++i) {
            const double v = rows[b * LPVMPC_TYRE_WORDS + i];
            if (i == 0 ? !(v == 0.0 || v == 1.0) : !(std::isfinite(v) && v >= 0))
                return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: tyre %s = %g (kind must be 0 or 1; B, C, c_f finite and >= 0)", who, b, names[i], v);
            t[(size_t)i * n + b] = v;
        }
    return LPVMPC_OK;
}

int lpvmpc_tyre_upload(lpvmpc_handle *h, const std::vector<double> &t, TyreTable &y) {
    y = {};
    double *d = nullptr;
    HIP_TRY(h, y.mem.alloc(d, t.size() * 8));
    y.t = d;
    hipStream_t st = h->stream;
    H2D(d, t.data(), t.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

extern "C" int lpvmpc_plant_step_tyres_batch(lpvmpc_handle *h, int32_t B, double *state, double *act_state, const double *u, int32_t n_sub,
                                             double dt_sim, double mu_sim, const lpvmpc_actuator_config *act, const int32_t *delay_a,
                                             const int32_t *delay_df, const double *plant_params, const double *tyre_params) {
    const char *who = "lpvmpc_plant_step_tyres_batch";
    if (h && B == 0) return LPVMPC_OK;
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (B < 0) return fail(h, LPVMPC_E_ARG, "%s: B=%d", who, B);
    std::vector<double> tyr;
    int rc = lpvmpc_tyre_rows(h, B, tyre_params, who, tyr); if (rc) return rc;
    return lpvmpc_plant_step_rows(h, B, state, act_state, u, n_sub, dt_sim, mu_sim, act, delay_a, delay_df, plant_params, &tyr, who);
}

extern "C" int lpvmpc_cl_init_tyres(lpvmpc_handle *h, int32_t B, const double *plant0, double half_width, double slack, int32_t q9_swap,
                                    int32_t n_sub, double dt_sim, double mu_sim, const lpvmpc_actuator_config *act, const int32_t *delay_a,
                                    const int32_t *delay_df, const double *plant_params, const double *tyre_params) {
    return lpvmpc_cl_init_rows(h, B, plant0, half_width, slack, q9_swap, n_sub, dt_sim, mu_sim, act, delay_a, delay_df, plant_params, true, tyre_params);
}

extern "C" int lpvmpc_race_init_tyres(lpvmpc_handle *h, lpvmpc_handle *tt, lpvmpc_handle *plan, int32_t B, const double *plant0,
                                      const int32_t *half_track0, const lpvmpc_race_config *cfg, const lpvmpc_observer_config *obs,
                                      const lpvmpc_actuator_config *act, const int32_t *delay_a, const int32_t *delay_df,
                                      const double *plant_params, const double *tyre_params) {
    return lpvmpc_race_init_rows(h, tt, plan, B, plant0, half_track0, cfg, obs, act, delay_a, delay_df, plant_params, true, tyre_params);
}

// device [4][B] -> host [B][4]
extern "C" int lpvmpc_tyre_params_read(lpvmpc_handle *h, double *tyre_params) {
    const char *who = "lpvmpc_tyre_params_read";
    const PlantSide *side = lpvmpc_plant_side(h);
    const double *t = side ? side->tyre.t : nullptr;
    if (!t) return fail(h, LPVMPC_E_ARG, "%s: no fleet or race started by lpvmpc_cl_init_tyres / lpvmpc_race_init_tyres", who);
    if (!tyre_params) return fail(h, LPVMPC_E_ARG, "%s: tyre_params is NULL", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t B = side->B;
    std::vector<double> v(B * LPVMPC_TYRE_WORDS);
    if (side->base_t()) v = *side->base_t();                             // disturbances or wear attached: the base rows, not the scaled live words
    else D2H(v.data(), t, v.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < LPVMPC_TYRE_WORDS; ++i) tyre_params[b * LPVMPC_TYRE_WORDS + i] = v[i * B + b];
    return LPVMPC_OK;
}

// the curve alone: force [B] at slip angle alpha [B] for vehicles of mass m [B]; a one-off table, freed when the call returns
extern "C" int lpvmpc_tyre_force_batch(lpvmpc_handle *h, int32_t B, const double *tyre_params, const double *m, const double *alpha, double *force) {
    const char *who = "lpvmpc_tyre_force_batch";
    if (h && B == 0) return LPVMPC_OK;
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (busy(h)) return fail(h, LPVMPC_E_ARG, "%s: this handle runs a fleet, cascade or race; use another handle for batch calls", who);
    if (B < 0 || !m || !alpha || !force) return fail(h, LPVMPC_E_ARG, "%s: B < 0 or NULL argument", who);
    const size_t n = B;
    for (size_t b = 0; b < n; ++b)
        if (!(std::isfinite(m[b]) && m[b] > 0)) return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: m = %g must be finite and > 0", who, b, m[b]);
    std::vector<double> tyr;
    int rc = lpvmpc_tyre_rows(h, B, tyre_params, who, tyr); if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    DevArena mem;                                                   // table [4][B], m, alpha, force
    double *d = nullptr;
    HIP_TRY(h, mem.alloc(d, n * (LPVMPC_TYRE_WORDS + 3) * 8));
    double *dm = d + n * LPVMPC_TYRE_WORDS, *da = dm + n, *df = da + n;
    hipStream_t st = h->stream;
    auto run = [&]() -> int {
        H2D(d, tyr.data(), n * LPVMPC_TYRE_WORDS * 8); H2D(dm, m, n * 8); H2D(da, alpha, n * 8);
        HIP_TRY(h, lpvmpc::launch_tyre_force(B, d, dm, da, df, st));
        D2H(force, df, n * 8);
        HIP_TRY(h, hipStreamSynchronize(st));
        return LPVMPC_OK;
    };
    rc = run();
    (void)hipStreamSynchronize(st);                                 // nothing in flight reads the table when it is freed
    return rc;
}
