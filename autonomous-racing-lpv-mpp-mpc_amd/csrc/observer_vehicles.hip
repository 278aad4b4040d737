// observer_vehicles.hip -- the per-vehicle-estimator forms (include/lpvmpc.h, "Per-vehicle state estimator"): the stand-alone
// observer step with a model row and gain tables per instance, and the fused estimator kernels of fleet_kernels.hpp with
// kObsVeh = true -- the per-vehicle forms <true, true, false, true> and the tyre forms <true, true, true, true>, delayed forms all.
// Each observer step reads the vehicle's row of the binding's model table and its polytope's 480 gain words from the binding's
// planes [2][480][B]; limits, polytope switch and weights are the configuration's (LDS, as in the other forms).  This translation
// unit holds these forms and no other, so that the objects of the other forms compile to the code they have alone.
#include "fleet_kernels.hpp"

namespace lpvmpc {

// lpvmpc_observer_step_vehicles_batch: observer_step_kernel (observer.hip) with the flag; instance b is "vehicle" b of v
__global__ void __launch_bounds__(64) observer_step_vehicles_kernel(ObsVehGains v, int B, double *__restrict__ est, const double *__restrict__ y,
                                                                    const double *__restrict__ u, const int32_t *__restrict__ k, double dt,
                                                                    double *__restrict__ aux) {
    __shared__ double G[kObsGainWords];
    obs_stage_gains(G, v.g);
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double x[6], yy[5], L[30], A[36], Bm[12];
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = est[(size_t)b * 6 + i];
#pragma unroll
    for (int i = 0; i < 5; ++i) yy[i] = y[(size_t)b * 5 + i];
    obs_step<true>(G, x, yy, u[b * 2 + 0], u[b * 2 + 1], (double)k[b], dt, L, A, Bm, obs_veh(v), b);
#pragma unroll
    for (int i = 0; i < 6; ++i) est[(size_t)b * 6 + i] = x[i];
    if (aux) {
        double *o = aux + (size_t)b * kObsAux;
        for (int i = 0; i < 30; ++i) o[i] = L[i];
        for (int i = 0; i < 36; ++i) o[30 + i] = A[i];
        for (int i = 0; i < 12; ++i) o[66 + i] = Bm[i];
    }
}

hipError_t launch_observer_step_vehicles(const ObsVehGains &v, int B, double *est, const double *y, const double *u, const int32_t *k, double dt,
                                         double *aux, hipStream_t s) {
    hipLaunchKernelGGL(observer_step_vehicles_kernel, LPVMPC_GRID(B), 0, s, v, B, est, y, u, k, dt, aux);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_observe_veh_obsveh(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((cl_command_plant_observe_kernel<true, true, false, true>), LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, a.N, a.uPred, a.cmd, a.plant,
                       static_cast<const VehPlantCfg &>(a.tpc), a.hw, a.slack, a.q9, a.local_next, a.u_old, a.gains, a.obs, a.op, 1, a.sd, a.act);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_observe_tyre_obsveh(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((cl_command_plant_observe_kernel<true, true, true, true>), LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, a.N, a.uPred, a.cmd, a.plant, a.tpc, a.hw,
                       a.slack, a.q9, a.local_next, a.u_old, a.gains, a.obs, a.op, 1, a.sd, a.act);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_observe_veh_obsveh(const RaceStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((race_command_plant_observe_kernel<true, true, false, true>), LPVMPC_GRID(a.r.B), 0, s, a.r, static_cast<const VehPlantCfg &>(a.tpc),
                       a.gains, a.obs, a.op, a.act);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_observe_tyre_obsveh(const RaceStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((race_command_plant_observe_kernel<true, true, true, true>), LPVMPC_GRID(a.r.B), 0, s, a.r, a.tpc, a.gains, a.obs, a.op, a.act);
    return hipGetLastError();
}

}  // namespace lpvmpc
