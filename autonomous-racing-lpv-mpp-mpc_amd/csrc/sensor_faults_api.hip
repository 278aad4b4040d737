// sensor_faults_api.hip -- C ABI of the sensor faults (include/lpvmpc.h, "Sensor faults"): the checks, the binding of a lap-0 fleet
// or a race (PlantSide::fault of the running engine, lpvmpc_plant_side), the read-back and the stand-alone sensor step.  Kernels:
// sensor_faults.hip; lpvmpc_cl_tick and lpvmpc_race_tick launch the faulted kernel in place of their fused observe kernel.
#include <cmath>
#include <vector>

#include "lpvmpc_handle.hpp"

static_assert(lpvmpc::kFaultWords == LPVMPC_FAULT_WORDS && lpvmpc::kObsStride == LPVMPC_OBS_STATE_WORDS, "host rows and device tables hold the same words");

extern "C" void lpvmpc_sensor_fault_default_config(lpvmpc_sensor_fault_config *c) {
    if (!c) return;
    c->seed = 0; c->vehicle_offset = 0;
}

// checks the host rows [B][LPVMPC_FAULT_WORDS] and returns the device layout [LPVMPC_FAULT_WORDS][B] in t
static int fault_rows(lpvmpc_handle *h, int B, const double *rows, const char *who, std::vector<double> &t) {
    static const char *names[LPVMPC_FAULT_WORDS] = {"gps_out_k0", "gps_out_len", "gps_loss_z", "gps_jump_k0", "gps_jump_len", "gps_jump_dx",
                                                    "gps_jump_dy", "imu_w_bias", "imu_yaw_drift", "enc_scale", "enc_out_k0", "enc_out_len"};
    const size_t n = B;
    t.assign(n * LPVMPC_FAULT_WORDS, 0.0);
    for (size_t b = 0; b < n; ++b)
        for (int i = 0; i < LPVMPC_FAULT_WORDS; ++i) {
            const double v = rows[b * LPVMPC_FAULT_WORDS + i];
            bool ok = std::isfinite(v);
            if (ok && (i == 0 || i == 1 || i == 3 || i == 4 || i == 10 || i == 11)) ok = v >= 0 && v == std::floor(v) && v < 2147483648.0;
            else if (ok && i == 9) ok = v > 0;
            if (!ok)
                return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: %s = %g (every word finite; k0 and len integer-valued, >= 0 and < 2^31; enc_scale > 0)",
                            who, b, names[i], v);
            t[(size_t)i * n + b] = v;
        }
    return LPVMPC_OK;
}

static void fault_cfg(const lpvmpc_sensor_fault_config &c, lpvmpc::FaultDev &d) { d.seed = c.seed ^ LPVMPC_FAULT_STREAM; d.voff = c.vehicle_offset; }

// the binding of the fleet or race that h runs; B its size; why: what keeps it from being served (null: served)
static FaultBinding *fault_target(lpvmpc_handle *h, int &B, const char *&why) {
    using namespace lpvmpc;
    why = nullptr;
    const RaceDev *race = nullptr;
    PlantSide *p = lpvmpc_plant_side(h, &race);
    if (!p) return nullptr;
    B = p->B;
    // the faulted kernels have the general form only: the _tyres starts with an estimator (step_form.hpp: their rows)
    const StepForm form = lpvmpc_step_form(h, *p, race);
    const bool tables = (form & SF_TYRES) == SF_TYRES;
    if (race) {
        if (!(form & SF_OBS) || !tables) why = "the race has no estimator in the loop or no plant and tyre tables (start it through lpvmpc_race_init_tyres with an estimator configuration)";
    }
    else if (!(form & SF_OBS)) why = "the fleet runs on ground truth: there are no sensors (lpvmpc_observer_setup before lpvmpc_cl_init_tyres)";
    else if (!tables) why = "the fleet has no plant and tyre tables (start it through lpvmpc_cl_init_tyres: the faulted kernel has the general form only)";
    else if (form & SF_TRK) why = "the fleet has per-vehicle tracks bound (lpvmpc_set_tracks): the faulted kernel has no track form (a race with tracks is served)";
    return &p->fault;
}

extern "C" int lpvmpc_set_sensor_faults(lpvmpc_handle *h, int32_t B, const lpvmpc_sensor_fault_config *cfg, const double *rows) {
    const char *who = "lpvmpc_set_sensor_faults";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    int fleet_B = 0;
    const char *why = nullptr;
    FaultBinding *cur = fault_target(h, fleet_B, why);
    if (!cur) return fail(h, LPVMPC_E_ARG, "%s: the handle runs no lap-0 fleet or race (for a race pass the path handle)", who);
    if (why) return fail(h, LPVMPC_E_ARG, "%s: %s", who, why);
    if (B != fleet_B) return fail(h, LPVMPC_E_ARG, "%s: B=%d, but the handle's fleet has %d vehicles", who, B, fleet_B);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    if (!rows) {                                                           // detach
        HIP_TRY(h, hipStreamSynchronize(st));                              // no tick in flight reads the table freed here
        *cur = FaultBinding{};
        return LPVMPC_OK;
    }
    lpvmpc_sensor_fault_config c;
    lpvmpc_sensor_fault_default_config(&c);
    if (cfg) c = *cfg;
    std::vector<double> rows_dev;
    int rc = fault_rows(h, B, rows, who, rows_dev); if (rc) return rc;
    // built in x and installed after the last step that can fail
    FaultBinding x;
    x.cfg = c;
    x.rows.assign(rows, rows + (size_t)B * LPVMPC_FAULT_WORDS);
    double *d_rows = nullptr;
    HIP_TRY(h, x.mem.alloc(d_rows, rows_dev.size() * 8));
    H2D(d_rows, rows_dev.data(), rows_dev.size() * 8);
    HIP_TRY(h, hipStreamSynchronize(st));                                  // the staging vector ends with this call; no tick reads the old table
    x.d.rows = d_rows; x.d.B = B;
    fault_cfg(c, x.d);
    *cur = std::move(x);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_sensor_faults_read(lpvmpc_handle *h, int32_t *B, double *rows) {
    const char *who = "lpvmpc_sensor_faults_read";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    int fleet_B = 0;
    const char *why = nullptr;
    const FaultBinding *cur = fault_target(h, fleet_B, why);
    const bool on = cur && cur->d.rows;
    if (B) *B = on ? cur->d.B : 0;
    if (on && rows) for (size_t i = 0; i < cur->rows.size(); ++i) rows[i] = cur->rows[i];
    return LPVMPC_OK;
}

extern "C" int lpvmpc_sensor_step_batch(lpvmpc_handle *h, int32_t B, const lpvmpc_observer_config *obs, double dt_sim,
                                        const lpvmpc_sensor_fault_config *cfg, const double *rows, double *obs_state, const double *plant,
                                        const double *servo, const double *motor) {
    const char *who = "lpvmpc_sensor_step_batch";
    if (h && B == 0) return LPVMPC_OK;                                   // an empty batch is a no-op
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (busy(h))
        return fail(h, LPVMPC_E_ARG, "%s: this handle runs a fleet, cascade or race; use another handle for batch calls (lpvmpc_cl_release ends it)", who);
    if (B < 0 || !obs || !obs_state || !plant || !servo || !motor) return fail(h, LPVMPC_E_ARG, "%s: B < 0 or a NULL argument", who);
    if (!(dt_sim > 0) || !std::isfinite(dt_sim)) return fail(h, LPVMPC_E_ARG, "%s: dt_sim = %g must be finite and > 0", who, dt_sim);
    int rc = lpvmpc_observer_check(h, obs, who); if (rc) return rc;
    if (h->ov.L && h->ov_B != B)
        return fail(h, LPVMPC_E_ARG, "%s: B=%d, but the handle's per-vehicle estimator rows cover %d vehicles (lpvmpc_set_observer_vehicles)", who, B, h->ov_B);
    const size_t n = B;
    for (size_t b = 0; b < n; ++b)
        for (int i : {(int)lpvmpc::OBS_GPS_CNT, (int)lpvmpc::OBS_ENC_CNT, (int)lpvmpc::OBS_K}) {
            const double v = obs_state[b * LPVMPC_OBS_STATE_WORDS + i];
            if (!(v >= 0 && v < 9007199254740992.0) || v != std::floor(v))
                return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: counter word %d of obs_state = %g is not an integer >= 0", who, b, i, v);
        }
    std::vector<double> rows_dev;
    if (rows) { rc = fault_rows(h, B, rows, who, rows_dev); if (rc) return rc; }
    lpvmpc_sensor_fault_config c;
    lpvmpc_sensor_fault_default_config(&c);
    if (cfg) c = *cfg;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    DevArena mem;                                                        // (all freed when the call returns)
    double *d_g = nullptr, *d_obs = nullptr, *d_plant = nullptr, *d_u = nullptr, *d_rows = nullptr;
    const size_t gw = sizeof(double) * 2 * (lpvmpc::kObsTable + 12);
    HIP_TRY(h, mem.alloc(d_g, gw));
    HIP_TRY(h, mem.alloc(d_obs, n * LPVMPC_OBS_STATE_WORDS * 8)); HIP_TRY(h, mem.alloc(d_plant, n * 8 * 8)); HIP_TRY(h, mem.alloc(d_u, n * 2 * 8));
    if (rows) HIP_TRY(h, mem.alloc(d_rows, rows_dev.size() * 8));
    auto run = [&]() -> int {
        H2D(d_g, obs->L_ls, gw);
        H2D(d_obs, obs_state, n * LPVMPC_OBS_STATE_WORDS * 8); H2D(d_plant, plant, n * 8 * 8);
        H2D(d_u, servo, n * 8); H2D(d_u + n, motor, n * 8);
        if (rows) H2D(d_rows, rows_dev.data(), rows_dev.size() * 8);
        lpvmpc::ObsParams op{};
        op.dt = 1.0 / obs->loop_rate; op.th_update = (1.0 / obs->gps_freq) / dt_sim; op.n_bound = obs->n_bound;
        op.std[0] = obs->psi_std; op.std[1] = obs->psiDot_std; op.std[2] = obs->x_std; op.std[3] = obs->y_std; op.std[4] = obs->v_std;
        op.seed = obs->seed; op.voff = obs->vehicle_offset;
        lpvmpc::FaultDev f{};
        f.rows = d_rows; f.B = B;
        fault_cfg(c, f);
        lpvmpc::ObsVehGains v; static_cast<lpvmpc::ObsVehDev &>(v) = h->ov; v.g = d_g;
        HIP_TRY(h, lpvmpc::launch_sensor_step(v, B, d_obs, d_plant, d_u, d_u + n, op, f, st));
        D2H(obs_state, d_obs, n * LPVMPC_OBS_STATE_WORDS * 8);
        HIP_TRY(h, hipStreamSynchronize(st));
        return LPVMPC_OK;
    };
    rc = run();
    (void)hipStreamSynchronize(st);
    return rc;
}
