// sensor_faults.hip -- the kernels of the sensor faults (include/lpvmpc.h, "Sensor faults"; the stage itself: sensor_faults.hpp).
//   cl_command_plant_observe_faulted_kernel<kObsVeh>     restates cl_command_plant_observe_kernel<true, true, true, kObsVeh>
//                                                        (fleet_kernels.hpp), mode 1, with obs_substep_faulted for obs_substep
//   race_command_plant_observe_faulted_kernel<kObsVeh>   restates race_command_plant_observe_kernel<true, true, true, kObsVeh> alike
//   sensor_step_kernel<kObsVeh>                          one sub-step on caller arrays (lpvmpc_sensor_step_batch), healthy or faulted
// A tick with faults attached launches the faulted kernel IN PLACE of the kernel it restates.  Only the general form exists:
// actuated, per-vehicle plant row, tyre row (the _tyres starts), with the configuration's estimator or the per-vehicle one.  The
// bodies are restated here, not shared with fleet_kernels.hpp through a device function: the objects that instantiate those
// templates keep the code they have alone ("Sensor faults"), and tests/test_gpu_sensor_faults.py holds the two
// together word for word through an all-off row.  That was measured (tools/isa_equal.py): with the race kernel's body as a
// forced-inline function template over the sensor stage, called by both kernels, every form moved -- race_command_plant_observe_kernel
// <false> 6371 -> 6378 instructions and 24 B of scratch, which the build's gate refuses, <true> 5720 -> 5730, <true, true> 5732 -> 5740,
// <true, true, true> 6358 -> 6347, <true, true, false, true> 6747 -> 6750, <true, true, true, true> 7361 -> 7383, and here
// race_command_plant_observe_faulted_kernel<false> 6778 -> 6788, <true> 7805 -> 7816.  The fleet kernel's body moved every form of
// cl_command_plant_observe_kernel as a function already, without a stage parameter (track_vehicles.hip has the counts), so the fleet
// pair was not taken further.  One lane per vehicle, 64-lane blocks; the fault rows are word-major [word][B], so a
// wavefront's loads of one word coalesce, and a vehicle's 12 words are loaded once, in front of the sub-step loop.  The gain words
// are staged in LDS as in the kernels restated, behind the same compiler barrier.  Gated: no scratch.
#include "sensor_faults.hpp"

namespace lpvmpc {

template <bool kObsVeh>
__global__ void __launch_bounds__(64) cl_command_plant_observe_faulted_kernel(const DevCfg *__restrict__ cp, int B, int N, const double *__restrict__ uPred,
                                                                              double *__restrict__ cmd, double *__restrict__ plant, TyrePlantCfg pc,
                                                                              double hw, double slack, int q9_swap, double *__restrict__ local_next,
                                                                              double *__restrict__ u_old, typename ObsGainsArg<kObsVeh>::type gains,
                                                                              double *__restrict__ obs, ObsParams op, int sd, ActDev a, FaultDev f) {
    __shared__ double G[kObsGainWords];
    obs_stage_gains(G, obs_gain_words(gains));
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double os[kObsStride];
#pragma unroll
    for (int i = 0; i < kObsStride; ++i) os[i] = obs[(size_t)b * kObsStride + i];
    const double servo = uPred[(size_t)b * N * 2 + 0], motor = uPred[(size_t)b * N * 2 + 1];
    cmd[b * 2 + 0] = servo; cmd[b * 2 + 1] = motor;
    double st[8], w[kFaultWords];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = plant[(size_t)b * 8 + i];
    fault_row(f, b, w);
    const long long vid = op.voff + b, fvid = f.voff + b;
    const int k0 = a.k[b], La = a.La[b], Ld = a.Ld[b];
    double sv = a.servo[b];
    for (int k = 0; k < pc.n_sub; ++k) {
        // compiler-only barrier, as in the kernel restated: keeps the gain words' LDS loads inside the loop
        asm volatile("" ::: "memory");
        double ua, ud;
        act_stage(a, b, k0 + k, La, Ld, motor, servo, sv, ua, ud);
        plant_step_at(pc, b, st, ua, ud);
        obs_substep_faulted<kObsVeh>(G, op, vid, w, f.seed, fvid, os, st, servo, motor, obs_veh(gains), b);
    }
    a.k[b] = k0 + pc.n_sub; a.servo[b] = sv;
#pragma unroll
    for (int i = 0; i < 8; ++i) plant[(size_t)b * 8 + i] = st[i];
#pragma unroll
    for (int i = 0; i < kObsStride; ++i) obs[(size_t)b * kObsStride + i] = os[i];
    obs_local_state(*cp, hw, slack, q9_swap, os, local_next + (size_t)b * 6);
    uold_push(u_old + (size_t)b * (2 + sd), sd, servo, motor);
}

template <bool kObsVeh>
__global__ void __launch_bounds__(64) race_command_plant_observe_faulted_kernel(RaceDev r, TyrePlantCfg pc, typename ObsGainsArg<kObsVeh>::type gains,
                                                                                double *__restrict__ obs, ObsParams op, ActDev a, FaultDev f) {
    __shared__ double G[kObsGainWords];
    obs_stage_gains(G, obs_gain_words(gains));
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= r.B) return;
    const int src = r.src[b], n = r.nstep[b], N = r.N;
    if (src == 0) { r.iters[b] = r.p_iters[b]; r.status[b] = r.p_status[b]; }
    else if (src == 1) { r.iters[b] = r.t_iters[b]; r.status[b] = r.t_status[b]; }
    else r.iters[b] = 0;
    if (n == 0) return;                                                     // frozen: plant, actuator and observer stay put
    const double *u = (r.lap[b] == 0 ? r.p_uPred : r.t_uPred) + (size_t)b * N * 2;
    const double servo = u[0], motor = u[1];
    r.cmd[b * 2 + 0] = servo; r.cmd[b * 2 + 1] = motor;
    double st[8], os[kObsStride], w[kFaultWords];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = r.plant[(size_t)b * 8 + i];
#pragma unroll
    for (int i = 0; i < kObsStride; ++i) os[i] = obs[(size_t)b * kObsStride + i];
    fault_row(f, b, w);
    const long long vid = op.voff + b, fvid = f.voff + b;
    const int k0 = a.k[b], La = a.La[b], Ld = a.Ld[b];
    double sv = a.servo[b];
    for (int k = 0; k < n; ++k) {
        // compiler-only barrier, as in the kernel restated: without it the gain words' LDS loads are hoisted out of the loop and spill
        asm volatile("" ::: "memory");
        double ua, ud;
        act_stage(a, b, k0 + k, La, Ld, motor, servo, sv, ua, ud);
        plant_step_at(pc, b, st, ua, ud);
        obs_substep_faulted<kObsVeh>(G, op, vid, w, f.seed, fvid, os, st, servo, motor, obs_veh(gains), b);
    }
    a.k[b] = k0 + n; a.servo[b] = sv;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.plant[(size_t)b * 8 + i] = st[i];
#pragma unroll
    for (int i = 0; i < kObsStride; ++i) obs[(size_t)b * kObsStride + i] = os[i];
    double *v = r.estv + (size_t)b * 8;
    v[0] = os[3]; v[1] = os[4]; v[2] = os[0]; v[3] = os[1]; v[4] = 0.0; v[5] = 0.0; v[6] = os[5]; v[7] = os[2];
    r.step[b] += n;
}

// one sensors + observer sub-step on caller arrays; f.rows null: the healthy stage (obs_substep)
template <bool kObsVeh>
__global__ void __launch_bounds__(64) sensor_step_kernel(typename ObsGainsArg<kObsVeh>::type gains, int B, double *__restrict__ obs,
                                                         const double *__restrict__ plant, const double *__restrict__ servo,
                                                         const double *__restrict__ motor, ObsParams op, FaultDev f) {
    __shared__ double G[kObsGainWords];
    obs_stage_gains(G, obs_gain_words(gains));
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double os[kObsStride], st[8];
#pragma unroll
    for (int i = 0; i < kObsStride; ++i) os[i] = obs[(size_t)b * kObsStride + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = plant[(size_t)b * 8 + i];
    const long long vid = op.voff + b;
    if (f.rows) {
        double w[kFaultWords];
        fault_row(f, b, w);
        obs_substep_faulted<kObsVeh>(G, op, vid, w, f.seed, f.voff + b, os, st, servo[b], motor[b], obs_veh(gains), b);
    } else {
        obs_substep<kObsVeh>(G, op, vid, os, st, servo[b], motor[b], obs_veh(gains), b);
    }
#pragma unroll
    for (int i = 0; i < kObsStride; ++i) obs[(size_t)b * kObsStride + i] = os[i];
}

hipError_t launch_cl_command_plant_observe_faulted(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((cl_command_plant_observe_faulted_kernel<false>), LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, a.N, a.uPred, a.cmd, a.plant, a.tpc, a.hw, a.slack,
                       a.q9, a.local_next, a.u_old, a.gains.g, a.obs, a.op, a.sd, a.act, a.fault);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_observe_faulted_obsveh(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((cl_command_plant_observe_faulted_kernel<true>), LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, a.N, a.uPred, a.cmd, a.plant, a.tpc, a.hw, a.slack,
                       a.q9, a.local_next, a.u_old, a.gains, a.obs, a.op, a.sd, a.act, a.fault);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_observe_faulted(const RaceStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((race_command_plant_observe_faulted_kernel<false>), LPVMPC_GRID(a.r.B), 0, s, a.r, a.tpc, a.gains.g, a.obs, a.op, a.act, a.fault);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_observe_faulted_obsveh(const RaceStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((race_command_plant_observe_faulted_kernel<true>), LPVMPC_GRID(a.r.B), 0, s, a.r, a.tpc, a.gains, a.obs, a.op, a.act, a.fault);
    return hipGetLastError();
}
hipError_t launch_sensor_step(const ObsVehGains &v, int B, double *obs, const double *plant, const double *servo, const double *motor,
                              const ObsParams &op, const FaultDev &f, hipStream_t s) {
    if (v.L) hipLaunchKernelGGL((sensor_step_kernel<true>), LPVMPC_GRID(B), 0, s, v, B, obs, plant, servo, motor, op, f);
    else hipLaunchKernelGGL((sensor_step_kernel<false>), LPVMPC_GRID(B), 0, s, v.g, B, obs, plant, servo, motor, op, f);
    return hipGetLastError();
}

}  // namespace lpvmpc
