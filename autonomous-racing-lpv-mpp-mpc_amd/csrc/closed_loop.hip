// closed_loop.hip -- device-side plant model, track coordinate transforms and the per-tick glue of a
// batched closed-loop run.  One lane per vehicle: every piece is a short serial
// recipe per vehicle, the parallel axis is the fleet.
//
// Replaces, for a whole fleet at once, the caller-side code of the reference:
//   Simulator.f                         vehicleSimulator.py:164-199  (bicycle model, linear tyres Fy = 60 alpha)
//   Map.getLocalPosition                Utilities/trackInitialization.py:283-383 (+ computeAngle :393-411)
//   Map.getGlobalPosition               Utilities/trackInitialization.py:205-262
//   lap-0 measurement / command glue    controllerMain.py:179-190, 289-298, 381-386
//   predicted_vectors_generation        controllerMain.py:510-553 (seed trajectories of the first 9 ticks)
//
// The kernels that advance the plant or write u_old are in fleet_kernels.hpp (this file launches their plain forms).
#include "lpvmpc_device.hpp"
#include "track_geometry.hpp"
#include "fleet_kernels.hpp"

namespace lpvmpc {

__global__ void __launch_bounds__(64) local_position_kernel(const DevCfg *__restrict__ cp, int B, const double *__restrict__ in,
                                                            double hw, double slack, double *__restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    local_position_body(*cp, hw, slack, b, in, out);
}
__global__ void __launch_bounds__(64) global_position_kernel(const DevCfg *__restrict__ cp, int B, const double *__restrict__ in,
                                                             double *__restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    global_position_body(*cp, b, in, out);
}
// predicted_vectors_generation (CMAIN:510-553): 20 fixed rows built on the local state; delta seeds are zero
__constant__ double kSeedDvx[20] = {0.05, 0.2, 0.4, 0.6, 0.7, 0.8, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9};
__constant__ double kSeedDs[20] = {0, 0.01, 0.02, 0.04, 0.07, 0.1, 0.14, 0.18, 0.23, 0.55, 0.66, 0.77, 0.89, 1.00, 1.19, 1.39, 1.59, 1.79, 1.89, 1.999};
__global__ void __launch_bounds__(64) cl_seed_kernel(int B, int N, const double *__restrict__ local_state, double *__restrict__ xlast,
                                                     double *__restrict__ delta) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * N) return;
    const int b = t / N, i = t - b * N;
    const double *ls = local_state + (size_t)b * 6;
    double *x = xlast + (size_t)t * 6;
    const int ii = i < 20 ? i : 19;
    x[0] = ls[0] + kSeedDvx[ii]; x[1] = ls[1]; x[2] = ls[2]; x[3] = 0.0001; x[4] = ls[4] + kSeedDs[ii]; x[5] = 0.0001;
    delta[t] = 0.0;
}

// command = first predicted input (CMAIN:381-386: servo = uPred[0,0], motor = uPred[0,1]); then the plant advances
// n_sub simulator steps under that command (u = [motor, servo], vehicleSimulator.py:330)
__global__ void __launch_bounds__(64) cl_command_plant_kernel(int B, int N, const double *__restrict__ uPred, double *__restrict__ cmd,
                                                              double *__restrict__ plant, PlantCfg pc) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double servo = uPred[(size_t)b * N * 2 + 0], motor = uPred[(size_t)b * N * 2 + 1];
    cmd[b * 2 + 0] = servo; cmd[b * 2 + 1] = motor;
    double st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = plant[(size_t)b * 8 + i];
    for (int k = 0; k < pc.n_sub; ++k) plant_step(pc, st, motor, servo);
#pragma unroll
    for (int i = 0; i < 8; ++i) plant[(size_t)b * 8 + i] = st[i];
}

hipError_t launch_local_position(const DevCfg *dcfg, int B, const double *xypsi, double hw, double slack, double *out, hipStream_t s) {
    hipLaunchKernelGGL(local_position_kernel, LPVMPC_GRID(B), 0, s, dcfg, B, xypsi, hw, slack, out);
    return hipGetLastError();
}
hipError_t launch_global_position(const DevCfg *dcfg, int B, const double *sey, double *out, hipStream_t s) {
    hipLaunchKernelGGL(global_position_kernel, LPVMPC_GRID(B), 0, s, dcfg, B, sey, out);
    return hipGetLastError();
}
hipError_t launch_plant(const PlantStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(plant_kernel<false>, LPVMPC_GRID(a.B), 0, s, a.B, a.plant, a.u, a.pc, ActDev{});
    return hipGetLastError();
}
hipError_t launch_cl_measure(const FleetMeasureArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_measure_kernel<false>, LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, a.plant, a.cmd, a.hw, a.slack, a.q9, a.local_state, a.u_old, 0);
    return hipGetLastError();
}
hipError_t launch_cl_seed(int B, int N, const double *local_state, double *xlast, double *delta, hipStream_t s) {
    hipLaunchKernelGGL(cl_seed_kernel, LPVMPC_GRID(B * N), 0, s, B, N, local_state, xlast, delta);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_kernel, LPVMPC_GRID(a.B), 0, s, a.B, a.N, a.uPred, a.cmd, a.plant, a.pc);
    return hipGetLastError();
}

hipError_t launch_cl_command_plant_measure(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_measure_kernel<false>, LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, a.N, a.uPred, a.cmd, a.plant, a.pc, a.hw, a.slack, a.q9,
                       a.local_next, a.u_old, 0, ActDev{});
    return hipGetLastError();
}

}  // namespace lpvmpc
