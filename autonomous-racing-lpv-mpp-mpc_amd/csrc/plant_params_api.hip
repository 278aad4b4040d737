// plant_params_api.hip -- C ABI of the per-vehicle plant parameters (include/lpvmpc.h, "Per-vehicle plant parameters"): the
// stand-alone batch call, the checks and device table shared by the fleet entry points and the read-back.  The fleet entry points
// themselves are lpvmpc_cl_init_vehicles (lpvmpc_api.hip) and lpvmpc_race_init_vehicles (race_api.hip).  Kernels: the <true, true>
// forms of fleet_kernels.hpp, launched from plant_params.hip.
#include <cmath>
#include <cstring>
#include <vector>

#include "lpvmpc_handle.hpp"

static_assert(lpvmpc::kPlantWords == LPVMPC_PLANT_WORDS, "host rows and device table hold the same words");

int lpvmpc_plant_rows(lpvmpc_handle *h, int B, const double *rows, const lpvmpc_config &nominal, double mu, const char *who,
                      std::vector<double> &t) {
    static const char *names[LPVMPC_PLANT_WORDS] = {"lf", "lr", "m", "Iz", "Cf", "Cr", "mu"};
    const double nom[LPVMPC_PLANT_WORDS] = {nominal.lf, nominal.lr, nominal.m, nominal.Iz, 60.0, 60.0, mu};   // Simulator.f's tyre: 60
    const size_t n = B;
    t.assign(n * LPVMPC_PLANT_WORDS, 0.0);
    for (size_t b = 0; b < n; ++b)
        for (int i = 0; i < LPVMPC_PLANT_WORDS; ++i) {
            const double v = rows ? rows[b * LPVMPC_PLANT_WORDS + i] : nom[i];
            if (!std::isfinite(v)) return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: %s = %g is not finite", who, b, names[i], v);
            if (i < 4 ? !(v > 0) : !(v >= 0))
                return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: %s = %g (lf, lr, m, Iz must be > 0; Cf, Cr, mu >= 0)", who, b, names[i], v);
            t[(size_t)i * n + b] = v;
        }
    return LPVMPC_OK;
}

int lpvmpc_plant_upload(lpvmpc_handle *h, int B, const std::vector<double> &t, double dt_sim, int n_sub, PlantTable &v) {
    v = {};
    double *d = nullptr;
    HIP_TRY(h, v.mem.alloc(d, t.size() * 8));
    v.d.p = d; v.d.B = B; v.d.dt = dt_sim; v.d.n_sub = n_sub;
    hipStream_t st = h->stream;
    H2D(d, t.data(), t.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

int lpvmpc_plant_step_rows(lpvmpc_handle *h, int32_t B, double *state, double *act_state, const double *u, int32_t n_sub, double dt_sim,
                           double mu_sim, const lpvmpc_actuator_config *act, const int32_t *delay_a, const int32_t *delay_df,
                           const double *plant_params, const std::vector<double> *tyre, const char *who, const DistStep *dist,
                           const WearStep *wear) {
    if (h && B == 0) return LPVMPC_OK;
    int rc = lpvmpc_check_batch(h, B, who); if (rc) return rc;
    if (!state || !u || n_sub < 1 || !(dt_sim > 0) || (act && !act_state)) return fail(h, LPVMPC_E_ARG, "%s: bad argument", who);
    std::vector<double> tab;
    rc = lpvmpc_plant_rows(h, B, plant_params, h->cfg, mu_sim, who, tab); if (rc) return rc;
    std::vector<double> dist_rows;                                  // lpvmpc_plant_step_disturbed_batch: the model in front of the step
    if (dist) { rc = lpvmpc_dist_rows(h, B, dist->cfg, dist->rows, who, dist_rows); if (rc) return rc; }
    std::vector<double> wear_rows;                                  // lpvmpc_plant_step_worn_batch: the wear model behind it
    if (wear) { rc = lpvmpc_wear_rows(h, B, wear->rows, n_sub, dt_sim, who, wear_rows); if (rc) return rc; }
    lpvmpc_actuator_config off;
    lpvmpc_actuator_default_config(&off);
    if (!act) { act = &off; delay_a = delay_df = nullptr; }
    const size_t b = B, R = lpvmpc::kActRing;
    std::vector<double> ring(b * 2 * R, 0.0), sv(b, 0.0);
    std::vector<int32_t> k(b, 0);
    if (act_state)
        for (size_t i = 0; i < b; ++i) {
            const double *o = act_state + i * LPVMPC_ACT_WORDS;
            const double kk = o[2 * R + 1];
            if (!(kk >= 0 && kk < 2147483647.0) || kk != (double)(int32_t)kk) return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: step counter %g is not an integer >= 0", who, i, kk);
            for (size_t c = 0; c < 2; ++c)
                for (size_t j = 0; j < R; ++j) ring[(c * R + j) * b + i] = o[c * R + j];
            sv[i] = o[2 * R]; k[i] = (int32_t)kk;
        }
    ActState as;                                                    // (all freed when the call returns)
    PlantTable v;
    TyreTable y;
    DistBinding dtmp;
    WearBinding wtmp;
    rc = lpvmpc_act_alloc(h, B, act, delay_a, delay_df, dt_sim, who, as); if (rc) return rc;
    const lpvmpc::ActDev &a = as.d;
    rc = lpvmpc_plant_upload(h, B, tab, dt_sim, n_sub, v);
    if (rc == LPVMPC_OK && tyre) rc = lpvmpc_tyre_upload(h, *tyre, y);
    hipStream_t st = h->stream;
    auto run = [&]() -> int {
        H2D(a.ring, ring.data(), ring.size() * 8); H2D(a.servo, sv.data(), b * 8); H2D(a.k, k.data(), b * 4);
        H2D(h->d_xlast, state, b * 8 * 8); H2D(h->d_states, u, b * 2 * 8);
        if (dist) {
            int rd = lpvmpc_dist_step(h, B, *dist, dist_rows, tab, *tyre, h->d_xlast, a.k, n_sub, dt_sim, const_cast<double *>(v.d.p),
                                      const_cast<double *>(y.t), dtmp, st);
            if (rd) return rd;
        }
        if (wear) {
            int rw = lpvmpc_wear_step(h, B, *wear, wear_rows, tab, *tyre, h->d_xlast, dist ? dtmp.d.state + 4 * b : nullptr, n_sub, dt_sim,
                                      const_cast<double *>(v.d.p), const_cast<double *>(y.t), wtmp, st);
            if (rw) return rw;
        }
        const lpvmpc::PlantStepArgs pa{B, h->d_xlast, h->d_states, lpvmpc::PlantCfg{}, tyre_plant(v, y), a};
        HIP_TRY(h, lpvmpc::plant_step_launcher(lpvmpc::step_form(true, true, y.t, false, false, false, false))(pa, st));
        D2H(state, h->d_xlast, b * 8 * 8);
        if (dist) { int rd = lpvmpc_dist_step_read(h, B, *dist, dtmp, st); if (rd) return rd; }
        if (wear) { int rw = lpvmpc_wear_step_read(h, B, *wear, wtmp, st); if (rw) return rw; }
        if (act_state) return lpvmpc_act_download(h, a, act_state, st);   // (synchronises)
        HIP_TRY(h, hipStreamSynchronize(st));
        return LPVMPC_OK;
    };
    if (rc == LPVMPC_OK) rc = run();
    (void)hipStreamSynchronize(st);
    return rc;
}

extern "C" int lpvmpc_plant_step_vehicles_batch(lpvmpc_handle *h, int32_t B, double *state, double *act_state, const double *u, int32_t n_sub,
                                                double dt_sim, double mu_sim, const lpvmpc_actuator_config *act, const int32_t *delay_a,
                                                const int32_t *delay_df, const double *plant_params) {
    return lpvmpc_plant_step_rows(h, B, state, act_state, u, n_sub, dt_sim, mu_sim, act, delay_a, delay_df, plant_params, nullptr,
                                  "lpvmpc_plant_step_vehicles_batch");
}

// device [7][B] -> host [B][7]
extern "C" int lpvmpc_plant_params_read(lpvmpc_handle *h, double *plant_params) {
    const char *who = "lpvmpc_plant_params_read";
    const PlantSide *side = lpvmpc_plant_side(h);
    const lpvmpc::VehPlantCfg *v = side ? &side->veh.d : nullptr;
    if (!v || !v->p) return fail(h, LPVMPC_E_ARG, "%s: no fleet or race started by lpvmpc_cl_init_vehicles / lpvmpc_race_init_vehicles", who);
    if (!plant_params) return fail(h, LPVMPC_E_ARG, "%s: plant_params is NULL", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t B = v->B;
    std::vector<double> t(B * LPVMPC_PLANT_WORDS);
    if (side->base_p()) t = *side->base_p();                             // disturbances or wear attached: the base rows, not the scaled live words
    else D2H(t.data(), v->p, t.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));
    if (const std::vector<double> *mu = lpvmpc_race_mu_base(h))          // interactions attached: the base mu, not the sheltered live word
        for (size_t b = 0; b < B; ++b) t[6 * B + b] = (*mu)[b];
    for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < LPVMPC_PLANT_WORDS; ++i) plant_params[b * LPVMPC_PLANT_WORDS + i] = t[i * B + b];
    return LPVMPC_OK;
}
