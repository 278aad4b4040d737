// actuator_api.hip -- C ABI of the actuator model (include/lpvmpc.h, "Actuator delay and servo lag"): the stand-alone batch call,
// the configuration and the read-back of a delayed fleet's or race's actuator state and controller histories.  The fleet entry
// points themselves are lpvmpc_cl_init_actuated (lpvmpc_api.hip) and lpvmpc_race_init_actuated (race_api.hip).  Kernels: the <true>
// forms of fleet_kernels.hpp, launched from actuator.hip.
#include <cstring>
#include <vector>

#include "lpvmpc_handle.hpp"

static_assert(lpvmpc::kActRing == LPVMPC_ACT_MAX_DELAY, "the device ring holds LPVMPC_ACT_MAX_DELAY commands per channel");
static_assert(LPVMPC_ACT_WORDS == 2 * lpvmpc::kActRing + 2, "host layout: two rings, servo_inp, k");

extern "C" void lpvmpc_actuator_default_config(lpvmpc_actuator_config *c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->servo_tf = 0.07;                                          // Tf (vehicleSimulator.py:62)
}

int lpvmpc_act_alloc(lpvmpc_handle *h, int B, const lpvmpc_actuator_config *cfg, const int32_t *delay_a, const int32_t *delay_df,
                     double dt_sim, const char *who, ActState &as) {
    as = {};
    lpvmpc::ActDev &a = as.d;
    if (!cfg) return fail(h, LPVMPC_E_ARG, "%s: actuator config is NULL", who);
    if (cfg->low_level_dyn && !(cfg->servo_tf > 0)) return fail(h, LPVMPC_E_ARG, "%s: servo_tf must be > 0 with low_level_dyn", who);
    std::vector<int32_t> La(B, cfg->delay_a), Ld(B, cfg->delay_df);
    if (delay_a) std::memcpy(La.data(), delay_a, (size_t)B * 4);
    if (delay_df) std::memcpy(Ld.data(), delay_df, (size_t)B * 4);
    for (int b = 0; b < B; ++b)
        if (La[b] < 0 || La[b] > LPVMPC_ACT_MAX_DELAY || Ld[b] < 0 || Ld[b] > LPVMPC_ACT_MAX_DELAY)
            return fail(h, LPVMPC_E_ARG, "%s: vehicle %d: delays (%d, %d) steps outside 0 .. %d (LPVMPC_ACT_MAX_DELAY)", who, b, La[b], Ld[b],
                        LPVMPC_ACT_MAX_DELAY);
    const size_t n = B;
    hipStream_t st = h->stream;
    int32_t *dLa = nullptr, *dLd = nullptr;
    HIP_TRY(h, as.mem.alloc(a.ring, n * 2 * lpvmpc::kActRing * 8));
    HIP_TRY(h, as.mem.alloc(a.servo, n * 8));
    HIP_TRY(h, as.mem.alloc(a.k, n * 4));
    HIP_TRY(h, as.mem.alloc(dLa, n * 4)); a.La = dLa;
    HIP_TRY(h, as.mem.alloc(dLd, n * 4)); a.Ld = dLd;
    HIP_TRY(h, hipMemsetAsync(a.ring, 0, n * 2 * lpvmpc::kActRing * 8, st));
    HIP_TRY(h, hipMemsetAsync(a.servo, 0, n * 8, st));
    HIP_TRY(h, hipMemsetAsync(a.k, 0, n * 4, st));
    H2D(dLa, La.data(), n * 4);
    H2D(dLd, Ld.data(), n * 4);
    HIP_TRY(h, hipStreamSynchronize(st));
    a.B = B; a.lld = cfg->low_level_dyn != 0;
    a.c = cfg->low_level_dyn ? dt_sim / cfg->servo_tf : 0.0;     // T / Tf and 1 - T / Tf as the reference evaluates them
    a.c1 = 1 - a.c;
    return LPVMPC_OK;
}

// device [2][R][B] + servo [B] + k [B] -> host [B][2R + 2]
int lpvmpc_act_download(lpvmpc_handle *h, const lpvmpc::ActDev &a, double *act_state, hipStream_t st) {
    const size_t B = a.B, R = lpvmpc::kActRing;
    std::vector<double> ring(B * 2 * R), sv(B);
    std::vector<int32_t> k(B);
    D2H(ring.data(), a.ring, ring.size() * 8);
    D2H(sv.data(), a.servo, B * 8);
    D2H(k.data(), a.k, B * 4);
    HIP_TRY(h, hipStreamSynchronize(st));
    for (size_t b = 0; b < B; ++b) {
        double *o = act_state + b * LPVMPC_ACT_WORDS;
        for (size_t c = 0; c < 2; ++c)
            for (size_t j = 0; j < R; ++j) o[c * R + j] = ring[(c * R + j) * B + b];
        o[2 * R] = sv[b]; o[2 * R + 1] = (double)k[b];
    }
    return LPVMPC_OK;
}

extern "C" int lpvmpc_plant_step_actuated_batch(lpvmpc_handle *h, int32_t B, double *state, double *act_state, const double *u, int32_t n_sub,
                                                double dt_sim, double mu_sim, const lpvmpc_actuator_config *cfg, const int32_t *delay_a,
                                                const int32_t *delay_df) {
    const char *who = "lpvmpc_plant_step_actuated_batch";
    if (h && B == 0) return LPVMPC_OK;
    int rc = lpvmpc_check_batch(h, B, who); if (rc) return rc;
    if (!state || !act_state || !u || n_sub < 1 || !(dt_sim > 0)) return fail(h, LPVMPC_E_ARG, "%s: bad argument", who);
    const size_t b = B, R = lpvmpc::kActRing;
    std::vector<double> ring(b * 2 * R), sv(b);
    std::vector<int32_t> k(b);
    for (size_t i = 0; i < b; ++i) {
        const double *o = act_state + i * LPVMPC_ACT_WORDS;
        const double kk = o[2 * R + 1];
        if (!(kk >= 0 && kk < 2147483647.0) || kk != (double)(int32_t)kk) return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: step counter %g is not an integer >= 0", who, i, kk);
        for (size_t c = 0; c < 2; ++c)
            for (size_t j = 0; j < R; ++j) ring[(c * R + j) * b + i] = o[c * R + j];
        sv[i] = o[2 * R]; k[i] = (int32_t)kk;
    }
    ActState as;                                                    // (freed when the call returns)
    rc = lpvmpc_act_alloc(h, B, cfg, delay_a, delay_df, dt_sim, who, as); if (rc) return rc;
    const lpvmpc::ActDev &a = as.d;
    hipStream_t st = h->stream;
    H2D(a.ring, ring.data(), ring.size() * 8); H2D(a.servo, sv.data(), b * 8); H2D(a.k, k.data(), b * 4);
    H2D(h->d_xlast, state, b * 8 * 8); H2D(h->d_states, u, b * 2 * 8);
    lpvmpc::PlantStepArgs pa{};
    pa.B = B; pa.plant = h->d_xlast; pa.u = h->d_states; pa.pc = lpvmpc_plant_cfg(h, n_sub, dt_sim, mu_sim); pa.act = a;
    HIP_TRY(h, lpvmpc::plant_step_launcher(lpvmpc::SF_ACT)(pa, st));
    D2H(state, h->d_xlast, b * 8 * 8);
    return lpvmpc_act_download(h, a, act_state, st);                // (synchronises)
}

extern "C" int lpvmpc_actuator_read(lpvmpc_handle *h, double *act_state, double *path_hist, double *tt_hist) {
    const lpvmpc::RaceDev *race = nullptr;
    const PlantSide *p = lpvmpc_plant_side(h, &race);
    if (race && !p->actuated) return fail(h, LPVMPC_E_ARG, "lpvmpc_actuator_read: the race was not started by lpvmpc_race_init_actuated");
    if (!p || !p->actuated)
        return fail(h, LPVMPC_E_ARG, "lpvmpc_actuator_read: no fleet or race started by lpvmpc_cl_init_actuated / lpvmpc_race_init_actuated");
    if (tt_hist && !race) return fail(h, LPVMPC_E_ARG, "lpvmpc_actuator_read: a lap-0 fleet has one controller (tt_hist must be NULL)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t n = (size_t)p->B * (2 + h->cfg.steering_delay) * 8;      // (a race's two controllers have one steering delay)
    if (path_hist) D2H(path_hist, h->d_uold, n);
    if (tt_hist) D2H(tt_hist, race->t_uold, n);
    if (act_state) { int rc = lpvmpc_act_download(h, p->act.d, act_state, st); if (rc) return rc; }
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}
