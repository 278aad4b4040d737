// observer.hip -- gain-scheduled LPV state estimator and simulated sensors (include/lpvmpc.h, "Gain-scheduled LPV state
// estimator").  One lane per vehicle, like closed_loop.hip: the per-vehicle recipe is short and serial, the fleet is the
// parallel axis.
//
// Replaces, for a whole fleet at once:
//   Estimator.GS_LPV_Est / Continuous_AB_Comp / L_Gain_Comp   stateEstimator.py:349-492
//   the estimator's sensor callbacks (encoder stale rule)      stateEstimator.py:600-760
//   ImuClass / GpsClass / EncClass.update, GpsClass.gps_pub    vehicleSimulator.py:222-329
//
// The two gain tables with their limits (2 x (480 + 12) doubles, 7.7 KiB) are read by every lane on every observer step,
// mostly at the same address across the wavefront.  They are staged in LDS once per workgroup: constant memory would need a
// per-launch symbol copy (one table per handle, handles on different streams), and LDS reads of a common address broadcast.
#include "lpvmpc_device.hpp"
#include "observer_device.hpp"
#include "track_geometry.hpp"

namespace lpvmpc {

__global__ void __launch_bounds__(64) observer_step_kernel(const double *__restrict__ gains, int B, double *__restrict__ est,
                                                           const double *__restrict__ y, const double *__restrict__ u,
                                                           const int32_t *__restrict__ k, double dt, double *__restrict__ aux) {
    __shared__ double G[kObsGainWords];
    obs_stage_gains(G, gains);
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double x[6], yy[5], L[30], A[36], Bm[12];
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = est[(size_t)b * 6 + i];
#pragma unroll
    for (int i = 0; i < 5; ++i) yy[i] = y[(size_t)b * 5 + i];
    obs_step(G, x, yy, u[b * 2 + 0], u[b * 2 + 1], (double)k[b], dt, L, A, Bm);
#pragma unroll
    for (int i = 0; i < 6; ++i) est[(size_t)b * 6 + i] = x[i];
    if (aux) {
        double *o = aux + (size_t)b * kObsAux;
        for (int i = 0; i < 30; ++i) o[i] = L[i];
        for (int i = 0; i < 36; ++i) o[30 + i] = A[i];
        for (int i = 0; i < 12; ++i) o[66 + i] = Bm[i];
    }
}

// controller measurement from the estimate (the estimator path's cl_measure_kernel): [max(vx, 0.01), vy, psiDot] and the map's
// local frame of (x, y, yaw) with quirk Q9 as in closed_loop.hip
__device__ inline void obs_local_state(const DevCfg &c, double hw, double slack, int q9_swap, const double *e, double *ls) {
    double s, ey, epsi; int inside;
    local_position(c, hw, slack, e[3], e[4], e[5], s, ey, epsi, inside);
    ls[0] = e[0] < 0.01 ? 0.01 : e[0]; ls[1] = e[1]; ls[2] = e[2];
    ls[3] = q9_swap ? ey : epsi; ls[4] = s; ls[5] = q9_swap ? epsi : ey;
}

// (delayed copy of modes 0 / 1: cl_command_plant_observe_act_kernel in actuator.hip -- change both)
// cl_command_plant_measure_kernel with the estimator in the loop: per plant step, plant -> sensors -> observer; the next tick's
// measurement is made from the estimate.  mode 0: only the measurement of the current estimate with u_old = cmd (the first
// tick of a fleet; one kernel keeps local_position at a single call site, inlined).  mode 2 (the cascade): advance, then write the
// estimate in the plant's layout [x y vx vy 0 0 yaw psiDot] to local_next [B][8], which the cascade's measurement kernels read
// in place of the plant; u_old is left to them
__global__ void __launch_bounds__(64) cl_command_plant_observe_kernel(const DevCfg *__restrict__ cp, int B, int N, const double *__restrict__ uPred,
                                                                      double *__restrict__ cmd, double *__restrict__ plant, PlantCfg pc,
                                                                      double hw, double slack, int q9_swap, double *__restrict__ local_next,
                                                                      double *__restrict__ u_old, const double *__restrict__ gains,
                                                                      double *__restrict__ obs, ObsParams op, int mode) {
    __shared__ double G[kObsGainWords];
    if (mode != 0) obs_stage_gains(G, gains);
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double os[kObsStride];
#pragma unroll
    for (int i = 0; i < kObsStride; ++i) os[i] = obs[(size_t)b * kObsStride + i];
    double servo = cmd[b * 2 + 0], motor = cmd[b * 2 + 1];
    if (mode != 0) {
        servo = uPred[(size_t)b * N * 2 + 0]; motor = uPred[(size_t)b * N * 2 + 1];
        cmd[b * 2 + 0] = servo; cmd[b * 2 + 1] = motor;
        double st[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) st[i] = plant[(size_t)b * 8 + i];
        const long long vid = op.voff + b;
        for (int k = 0; k < pc.n_sub; ++k) {
            plant_step(pc, st, motor, servo);
            obs_substep(G, op, vid, os, st, servo, motor);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) plant[(size_t)b * 8 + i] = st[i];
#pragma unroll
        for (int i = 0; i < kObsStride; ++i) obs[(size_t)b * kObsStride + i] = os[i];
    }
    if (mode == 2) {
        double *v = local_next + (size_t)b * 8;
        v[0] = os[3]; v[1] = os[4]; v[2] = os[0]; v[3] = os[1]; v[4] = 0.0; v[5] = 0.0; v[6] = os[5]; v[7] = os[2];
        return;
    }
    obs_local_state(*cp, hw, slack, q9_swap, os, local_next + (size_t)b * 6);
    u_old[b * 2 + 0] = servo; u_old[b * 2 + 1] = motor;
}

#define LPVMPC_GRID(n) dim3(((n) + 63) / 64), dim3(64)
hipError_t launch_observer_step(const double *gains, int B, double *est, const double *y, const double *u, const int32_t *k, double dt,
                                double *aux, hipStream_t s) {
    hipLaunchKernelGGL(observer_step_kernel, LPVMPC_GRID(B), 0, s, gains, B, est, y, u, k, dt, aux);
    return hipGetLastError();
}
hipError_t launch_cl_observe_measure(const DevCfg *dcfg, int B, const double *obs, const double *cmd, double hw, double slack, int q9_swap,
                                     double *local_state, double *u_old, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_kernel, LPVMPC_GRID(B), 0, s, dcfg, B, 1, (const double *)nullptr, const_cast<double *>(cmd),
                       (double *)nullptr, PlantCfg{}, hw, slack, q9_swap, local_state, u_old, (const double *)nullptr, const_cast<double *>(obs),
                       ObsParams{}, 0);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_observe(const DevCfg *dcfg, int B, int N, const double *uPred, double *cmd, double *plant, PlantCfg pc,
                                          double hw, double slack, int q9_swap, double *local_next, double *u_old, const double *gains,
                                          double *obs, const ObsParams &op, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_kernel, LPVMPC_GRID(B), 0, s, dcfg, B, N, uPred, cmd, plant, pc, hw, slack, q9_swap,
                       local_next, u_old, gains, obs, op, 1);
    return hipGetLastError();
}
hipError_t launch_cascade_plant_observe(int B, int N, const double *uPred, double *cmd, double *plant, PlantCfg pc, double *est_view,
                                        const double *gains, double *obs, const ObsParams &op, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_kernel, LPVMPC_GRID(B), 0, s, (const DevCfg *)nullptr, B, N, uPred, cmd, plant, pc, 0.0, 0.0, 0,
                       est_view, (double *)nullptr, gains, obs, op, 2);
    return hipGetLastError();
}

}  // namespace lpvmpc
