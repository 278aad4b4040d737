// track_lpv_eval.hip -- the bound forms of the LPV kernels that read the track (include/lpvmpc.h, "Per-vehicle tracks"): vehicle b
// looks its curvature up in its own entry of the handle's track palette (lpvmpc_set_tracks; TrackDev, track_view.hpp) instead of the
// table of the handle's configuration.  dt and N stay the handle's.
//
// They are per-vehicle-model forms all: the stage blocks and bodies are those of veh_lpv_model.hpp with the vehicle's track view as
// the curvature source (this object is compiled with -ffp-contract=off like lpv_eval.o and veh_lpv_eval.o), so a palette entry equal
// to the handle's table gives veh_lpv_eval.o's bits.  A handle without bound model rows runs them on the binding's table of the
// handle's own vehicle words.  The controller roll-out has its two-launch form only (every caller of the library wants [A | B]):
// ctrl_lpv_pre_kernel, or its per-vehicle form, reads no track and is launched as it is -- it is where the call's cf_new or the row's
// Cf enters -- and ctrl_lpv_roll_trk_kernel restates ctrl_lpv_roll_kernel of lpv_eval.hip, which reads no vehicle word: lpv_eval.hip
// shares no text (veh_lpv_model.hpp says what sharing with it moved).
#include "lpvmpc_device.hpp"
#include "track_view.hpp"
#include "veh_lpv_model.hpp"

namespace lpvmpc {

// ctrl_lpv_roll_kernel (lpv_eval.hip) on the vehicle's track: the state-dependent entries of the tiles that ctrl_lpv_pre_kernel (or
// its per-vehicle form) wrote, and the roll-out
__global__ void __launch_bounds__(64) ctrl_lpv_roll_trk_kernel(const DevCfg *__restrict__ cp, TrackDev trk, int B, const double *__restrict__ x0,
                                                               const double *__restrict__ u_prev, const double *__restrict__ curv_ref,
                                                               int lap, double *__restrict__ states, double *__restrict__ AB,
                                                               const int32_t *__restrict__ active) {
    const DevCfg &c = *cp;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (active && !active[b])) return;
    const TrackView tv = track_view(trk, b);
    const int N = c.N;
    const double dt = c.dt;
    double st[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) st[r] = x0[(size_t)b * 6 + r];
    for (int i = 0; i < N; ++i) {
        double *o = AB + ((size_t)b * N + i) * 48;
        const double a00 = o[0], a01 = o[1], p13 = o[2], a11 = o[9], a12_ = o[10], a21 = o[17], a22_ = o[18];
        const double b06 = o[6], b07 = o[7], b16 = o[14], b26 = o[22];
        const double vy = st[1], epsi = st[3], s = st[4], ey = st[5];
        const double cur = (lap == 0) ? track_curvature(tv, s) : curv_ref[(size_t)b * N + i];
        const double u0 = u_prev[((size_t)b * N + i) * 2 + 0], u1 = u_prev[((size_t)b * N + i) * 2 + 1];
        double se, ce;
        sincos(epsi, &se, &ce);
        const double den = 1.0 - ey * cur;
        const double a02 = dt * (p13 + vy);
        const double a30 = dt * ((1.0 / den) * (-ce * cur)), a31 = dt * ((1.0 / den) * (se * cur)), a32 = dt * 1.0;
        const double a40 = dt * (ce / den), a41 = dt * (se / den);
        const double a50 = dt * se, a51 = dt * ce;
        double nx[6];
        nx[0] = ((a00 * st[0] + a01 * st[1]) + a02 * st[2]) + (b06 * u0 + b07 * u1);
        nx[1] = (a11 * st[1] + a12_ * st[2]) + (b16 * u0 + 0.0 * u1);
        nx[2] = (a21 * st[1] + a22_ * st[2]) + (b26 * u0 + 0.0 * u1);
        nx[3] = (((a30 * st[0] + a31 * st[1]) + a32 * st[2]) + 1.0 * st[3]) + (0.0 * u0 + 0.0 * u1);
        nx[4] = ((a40 * st[0] + a41 * st[1]) + 1.0 * st[4]) + (0.0 * u0 + 0.0 * u1);
        nx[5] = ((a50 * st[0] + a51 * st[1]) + 1.0 * st[5]) + (0.0 * u0 + 0.0 * u1);
        o[2] = a02;
        o[24] = a30; o[25] = a31;
        o[32] = a40; o[33] = a41;
        o[40] = a50; o[41] = a51;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            st[r] = nx[r];
            if (states) states[((size_t)b * N + i) * 6 + r] = nx[r];
        }
    }
}

__global__ void __launch_bounds__(64) ctrl_abc_trk_kernel(const DevCfg *__restrict__ cp, TrackDev trk, const double *__restrict__ model, int B,
                                                          const double *__restrict__ xlast, const double *__restrict__ delta,
                                                          double *__restrict__ AB, const int32_t *__restrict__ active) {
    const DevCfg &c = *cp;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = c.N;
    if (t >= B * N || (active && !active[t / N])) return;
    ctrl_abc_body(c, track_view(trk, t / N), load_model(model, B, t / N), t, xlast, delta, AB);
}

__global__ void __launch_bounds__(64) plan_lpv_trk_kernel(const DevCfg *__restrict__ cp, TrackDev trk, const double *__restrict__ model, int B,
                                                          const double *__restrict__ x0, const double *__restrict__ u_prev,
                                                          const double *__restrict__ SS, double *__restrict__ states,
                                                          double *__restrict__ AB, const int32_t *__restrict__ active) {
    const DevCfg &c = *cp;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (active && !active[b])) return;
    plan_lpv_body(c, track_view(trk, b), load_model(model, B, b), b, x0, u_prev, SS, states, AB);
}

__global__ void __launch_bounds__(64) plan_abc_trk_kernel(const DevCfg *__restrict__ cp, TrackDev trk, const double *__restrict__ model, int B,
                                                          const double *__restrict__ xlast, const double *__restrict__ delta,
                                                          double *__restrict__ AB, const int32_t *__restrict__ active) {
    const DevCfg &c = *cp;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = c.N;
    if (t >= B * N || (active && !active[t / N])) return;
    plan_abc_body(c, track_view(trk, t / N), load_model(model, B, t / N), t, xlast, delta, AB);
}

void launch_ctrl_lpv_roll_trk(const DevCfg *dcfg, const TrackDev &trk, int B, const double *x0, const double *u_prev, const double *curv_ref,
                              int lap, double *states, double *AB, hipStream_t stream, const int32_t *active) {
    hipLaunchKernelGGL(ctrl_lpv_roll_trk_kernel, LPVMPC_GRID(B), 0, stream, dcfg, trk, B, x0, u_prev, curv_ref, lap, states, AB, active);
}
void launch_plan_lpv_trk(const DevCfg *dcfg, const TrackDev &trk, const double *model, int B, const double *x0, const double *u_prev,
                         const double *SS, double *states, double *AB, hipStream_t stream, const int32_t *active) {
    hipLaunchKernelGGL(plan_lpv_trk_kernel, LPVMPC_GRID(B), 0, stream, dcfg, trk, model, B, x0, u_prev, SS, states, AB, active);
}
void launch_abc_trk(int kind, const DevCfg *dcfg, const TrackDev &trk, const double *model, int B, int N, const double *xlast,
                    const double *delta, double *AB, hipStream_t stream, const int32_t *active) {
    if (kind == 0) hipLaunchKernelGGL(ctrl_abc_trk_kernel, LPVMPC_GRID(B * N), 0, stream, dcfg, trk, model, B, xlast, delta, AB, active);
    else hipLaunchKernelGGL(plan_abc_trk_kernel, LPVMPC_GRID(B * N), 0, stream, dcfg, trk, model, B, xlast, delta, AB, active);
}

}  // namespace lpvmpc
