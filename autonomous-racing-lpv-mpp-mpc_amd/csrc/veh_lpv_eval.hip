// veh_lpv_eval.hip -- the per-vehicle forms of the LPV kernels that read vehicle words (lpv_eval.hip): vehicle b linearises with
// row b of the handle's model table [kModelWords][B] = lf, lr, m, Iz, Cf, Cr, mu (lpvmpc_set_model_params; include/lpvmpc.h,
// "Per-vehicle model parameters") instead of the words of the handle's configuration.  dt, N and the track table stay the handle's.
//
// The model row, the stage blocks and the bodies are in veh_lpv_model.hpp, which track_lpv_eval.hip includes as well; here their track
// is the configuration's.  In the controller roll-out the row's Cf stands for both axles, where the per-handle kernels take the
// call's cf_new (the reference passes Cf_new for both, CTRL:203-218); seed mode and the planner take the row's Cf and Cr.
#include "lpvmpc_device.hpp"
#include "veh_lpv_model.hpp"

namespace lpvmpc {

__global__ void __launch_bounds__(64) ctrl_lpv_veh_kernel(const DevCfg *__restrict__ cp, const double *__restrict__ model, int B,
                                                          const double *__restrict__ x0, const double *__restrict__ u_prev,
                                                          const double *__restrict__ vel_ref, const double *__restrict__ curv_ref, int lap,
                                                          double *__restrict__ states, double *__restrict__ AB,
                                                          const int32_t *__restrict__ active) {
    const DevCfg &c = *cp;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (active && !active[b])) return;
    const VehModel v = load_model(model, B, b);
    ctrl_lpv_body(c, OwnTrack{}, v, v.Cf, b, x0, u_prev, vel_ref, curv_ref, lap, states, AB);
}

__global__ void __launch_bounds__(64) ctrl_lpv_pre_veh_kernel(const DevCfg *__restrict__ cp, const double *__restrict__ model, int B,
                                                              const double *__restrict__ u_prev, const double *__restrict__ vel_ref,
                                                              double *__restrict__ AB, const int32_t *__restrict__ active) {
    const DevCfg &c = *cp;
    const int N = c.N;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * N) return;
    const int b = t / N, i = t - b * N;
    if (active && !active[b]) return;
    const VehModel v = load_model(model, B, b);
    ctrl_lpv_pre_body(c, v, v.Cf, b, i, t, u_prev, vel_ref, AB);
}

__global__ void __launch_bounds__(64) ctrl_abc_veh_kernel(const DevCfg *__restrict__ cp, const double *__restrict__ model, int B,
                                                          const double *__restrict__ xlast, const double *__restrict__ delta,
                                                          double *__restrict__ AB, const int32_t *__restrict__ active) {
    const DevCfg &c = *cp;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = c.N;
    if (t >= B * N || (active && !active[t / N])) return;
    ctrl_abc_body(c, OwnTrack{}, load_model(model, B, t / N), t, xlast, delta, AB);
}

__global__ void __launch_bounds__(64) plan_lpv_veh_kernel(const DevCfg *__restrict__ cp, const double *__restrict__ model, int B,
                                                          const double *__restrict__ x0, const double *__restrict__ u_prev,
                                                          const double *__restrict__ SS, double *__restrict__ states,
                                                          double *__restrict__ AB, const int32_t *__restrict__ active) {
    const DevCfg &c = *cp;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (active && !active[b])) return;
    plan_lpv_body(c, OwnTrack{}, load_model(model, B, b), b, x0, u_prev, SS, states, AB);
}

__global__ void __launch_bounds__(64) plan_abc_veh_kernel(const DevCfg *__restrict__ cp, const double *__restrict__ model, int B,
                                                          const double *__restrict__ xlast, const double *__restrict__ delta,
                                                          double *__restrict__ AB, const int32_t *__restrict__ active) {
    const DevCfg &c = *cp;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = c.N;
    if (t >= B * N || (active && !active[t / N])) return;
    plan_abc_body(c, OwnTrack{}, load_model(model, B, t / N), t, xlast, delta, AB);
}

void launch_ctrl_lpv_pre_veh(const DevCfg *dcfg, const double *model, int B, int N, const double *u_prev, const double *vel_ref, double *AB,
                             hipStream_t stream, const int32_t *active) {
    hipLaunchKernelGGL(ctrl_lpv_pre_veh_kernel, LPVMPC_GRID(B * N), 0, stream, dcfg, model, B, u_prev, vel_ref, AB, active);
}
void launch_lpv_veh(int kind, const DevCfg *dcfg, const double *model, int B, const double *x0, const double *u_prev, const double *vel_ref,
                    const double *curv_s, int lap, double *states, double *AB, hipStream_t stream, const int32_t *active) {
    if (kind == 0) hipLaunchKernelGGL(ctrl_lpv_veh_kernel, LPVMPC_GRID(B), 0, stream, dcfg, model, B, x0, u_prev, vel_ref, curv_s, lap, states, AB, active);
    else hipLaunchKernelGGL(plan_lpv_veh_kernel, LPVMPC_GRID(B), 0, stream, dcfg, model, B, x0, u_prev, curv_s, states, AB, active);
}
void launch_abc_veh(int kind, const DevCfg *dcfg, const double *model, int B, int N, const double *xlast, const double *delta, double *AB,
                    hipStream_t stream, const int32_t *active) {
    if (kind == 0) hipLaunchKernelGGL(ctrl_abc_veh_kernel, LPVMPC_GRID(B * N), 0, stream, dcfg, model, B, xlast, delta, AB, active);
    else hipLaunchKernelGGL(plan_abc_veh_kernel, LPVMPC_GRID(B * N), 0, stream, dcfg, model, B, xlast, delta, AB, active);
}

}  // namespace lpvmpc
