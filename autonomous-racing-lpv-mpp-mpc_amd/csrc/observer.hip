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
// cl_command_plant_observe_kernel is in fleet_kernels.hpp (this file launches its plain form).
#include "lpvmpc_device.hpp"
#include "observer_device.hpp"
#include "track_geometry.hpp"
#include "fleet_kernels.hpp"

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

hipError_t launch_observer_step(const double *gains, int B, double *est, const double *y, const double *u, const int32_t *k, double dt,
                                double *aux, hipStream_t s) {
    hipLaunchKernelGGL(observer_step_kernel, LPVMPC_GRID(B), 0, s, gains, B, est, y, u, k, dt, aux);
    return hipGetLastError();
}
hipError_t launch_cl_observe_measure(const FleetMeasureArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_kernel<false>, LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, 1, (const double *)nullptr, const_cast<double *>(a.cmd),
                       (double *)nullptr, PlantCfg{}, a.hw, a.slack, a.q9, a.local_state, a.u_old, (const double *)nullptr, const_cast<double *>(a.obs),
                       ObsParams{}, 0, 0, ActDev{});
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_observe(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_kernel<false>, LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, a.N, a.uPred, a.cmd, a.plant, a.pc, a.hw, a.slack, a.q9,
                       a.local_next, a.u_old, a.gains.g, a.obs, a.op, 1, 0, ActDev{});
    return hipGetLastError();
}
hipError_t launch_cascade_plant_observe(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_kernel<false>, LPVMPC_GRID(a.B), 0, s, (const DevCfg *)nullptr, a.B, a.N, a.uPred, a.cmd, a.plant, a.pc, 0.0, 0.0,
                       0, a.local_next, (double *)nullptr, a.gains.g, a.obs, a.op, 2, 0, ActDev{});
    return hipGetLastError();
}

}  // namespace lpvmpc
