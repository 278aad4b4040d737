// model_params_api.hip -- C ABI of the per-vehicle model parameters (include/lpvmpc.h, "Per-vehicle model parameters"): the handle's
// table of model rows, its checks and the read-back.  The binding acts through the two launch wrappers of lpv_eval.hip, which every
// route that linearises calls with the handle's table (h->d_model); kernels: veh_lpv_eval.hip.
#include <vector>

#include "lpvmpc_handle.hpp"

static_assert(lpvmpc::kModelWords == LPVMPC_MODEL_WORDS && LPVMPC_MODEL_WORDS == LPVMPC_PLANT_WORDS,
              "model rows, plant rows and the device tables hold the same words");

int lpvmpc_model_check(lpvmpc_handle *h, int B, const char *who) {
    if (h->d_model && h->model_B != B)
        return fail(h, LPVMPC_E_ARG, "%s: B=%d, but the handle has model rows for %d vehicles bound (lpvmpc_set_model_params)", who, B, h->model_B);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_set_model_params(lpvmpc_handle *h, int32_t B, const double *model_params) {
    const char *who = "lpvmpc_set_model_params";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (busy(h))
        return fail(h, LPVMPC_E_ARG, "%s: this handle runs a %s; bind the model rows before it starts (lpvmpc_cl_release ends it)", who,
                    h->cl_plant ? "closed-loop fleet" : (h->race || h->race_owner) ? "race" : "planner + controller cascade");
    if (B < 0) return fail(h, LPVMPC_E_ARG, "%s: B=%d", who, B);
    if (B > 0 && !model_params) return fail(h, LPVMPC_E_ARG, "%s: model_params is NULL (B = 0 unbinds)", who);
    std::vector<double> tab;                                             // [7][B], checked by the plant rows' rules
    if (B > 0) { int rc = lpvmpc_plant_rows(h, B, model_params, h->cfg, 0.0, who, tab); if (rc) return rc; }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    ModelTable m;                                                        // B = 0: none
    if (B > 0) {
        HIP_TRY(h, m.model_mem.alloc(m.d_model, tab.size() * 8));
        if (hipMemcpy(m.d_model, tab.data(), tab.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
            return fail(h, LPVMPC_E_HIP, "%s: uploading the rows failed", who);
        m.model_B = B;
    }
    static_cast<ModelTable &>(*h) = std::move(m);                        // (freeing the old table waits for the launches that read it)
    return LPVMPC_OK;
}

// device [7][B] -> host [B][7]
extern "C" int lpvmpc_model_params_read(lpvmpc_handle *h, int32_t *B, double *model_params) {
    const char *who = "lpvmpc_model_params_read";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (!B) return fail(h, LPVMPC_E_ARG, "%s: B is NULL", who);
    *B = h->d_model ? h->model_B : 0;
    if (!h->d_model || !model_params) return LPVMPC_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t n = h->model_B;
    std::vector<double> t(n * LPVMPC_MODEL_WORDS);
    HIP_TRY(h, hipMemcpy(t.data(), h->d_model, t.size() * 8, hipMemcpyDeviceToHost));
    for (size_t b = 0; b < n; ++b)
        for (size_t i = 0; i < LPVMPC_MODEL_WORDS; ++i) model_params[b * LPVMPC_MODEL_WORDS + i] = t[i * n + b];
    return LPVMPC_OK;
}
