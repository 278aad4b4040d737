// track_vehicles.hip -- the bound forms of the stand-alone track transforms and of the lap-0 fleet's kernels that read the track
// (include/lpvmpc.h, "Per-vehicle tracks"): vehicle b is measured on its own entry of the handle's track palette, with that entry's
// half width and slack (lpvmpc_set_tracks).  The transforms themselves are the view forms of track_view.hpp.
//   local_position_trk_kernel, global_position_trk_kernel   local_position_kernel, global_position_kernel of closed_loop.hip
//   cl_measure_trk_kernel                                   cl_measure_kernel<true> of fleet_kernels.hpp
//   cl_command_plant_measure_trk_kernel                     cl_command_plant_measure_kernel<true, true, true>
//   cl_command_plant_observe_trk_kernel<kObsVeh>            cl_command_plant_observe_kernel<true, true, true, kObsVeh>
// The fleet forms exist for the most general start only (lpvmpc_cl_init_tyres: delayed forms with the plant and tyre tables).  They are
// kernels of their own and no further template flag of fleet_kernels.hpp: a track argument in the shared signature changes the
// kernel arguments of every form.  Their own object, so that closed_loop.o, tyre.o and observer_vehicles.o keep the code they have
// alone, compiled as those are, so that a palette entry equal to a handle's table gives that handle's words.
//
// The two transforms and cl_measure_trk_kernel share their body with the original (fleet_kernels.hpp: a function template over the
// track source, here the binding).  The two command / plant kernels restate their one form of the template with the vehicle's track
// view where the template passes the configuration, the same statements in the same order: with one body for both, every delayed
// form of the template moved (tools/isa_equal.py; DESIGN.md, "One source, one form per object"; instructions before -> after):
//   cl_command_plant_measure   <true> 3085 -> 3088 (actuator.o), <true, true> 3098 -> 3100 (plant_params.o), <true, true, true>
//                              3623 -> 3625 (tyre.o), cl_command_plant_measure_trk_kernel 3603 -> 3605; with the plant and actuator
//                              arguments by value 3086, 3099, 3624 and 3601
//   cl_command_plant_observe   <false> 6807 -> 6806 (observer.o), <true> 7345 -> 7333, <true, true> 7288 -> 7297, <true, true, true>
//                              7889 -> 7893, <true, true, false, true> 8294 -> 8317 and <true, true, true, true> 8921 -> 8891
//                              (observer_vehicles.o), cl_command_plant_observe_trk_kernel<false> 9148 -> 9140, <true> 8936 -> 8934
#include "fleet_kernels.hpp"
#include "track_view.hpp"

namespace lpvmpc {

__global__ void __launch_bounds__(64) local_position_trk_kernel(TrackDev trk, int B, const double *__restrict__ in, double *__restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    local_position_body(trk, 0.0, 0.0, b, in, out);
}
__global__ void __launch_bounds__(64) global_position_trk_kernel(TrackDev trk, int B, const double *__restrict__ in, double *__restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    global_position_body(trk, b, in, out);
}

// first tick of a fleet without an estimator: the measurement of the start state and the controller's history
__global__ void __launch_bounds__(64) cl_measure_trk_kernel(TrackDev trk, int B, const double *__restrict__ plant, const double *__restrict__ cmd,
                                                            int q9_swap, double *__restrict__ local_state, double *__restrict__ u_old, int sd) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    cl_measure_body(trk, b, plant, cmd, 0.0, 0.0, q9_swap, local_state, u_old, sd);
}

// command, n_sub simulator steps through the actuator stage with the vehicle's plant and tyre rows, then the next tick's measurement
__global__ void __launch_bounds__(64) cl_command_plant_measure_trk_kernel(TrackDev trk, int B, int N, const double *__restrict__ uPred,
                                                                          double *__restrict__ cmd, double *__restrict__ plant, TyrePlantCfg pc,
                                                                          int q9_swap, double *__restrict__ local_next,
                                                                          double *__restrict__ u_old, int sd, ActDev a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double servo = uPred[(size_t)b * N * 2 + 0], motor = uPred[(size_t)b * N * 2 + 1];
    cmd[b * 2 + 0] = servo; cmd[b * 2 + 1] = motor;
    double st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = plant[(size_t)b * 8 + i];
    const int k0 = a.k[b], La = a.La[b], Ld = a.Ld[b];
    double sv = a.servo[b];
    for (int k = 0; k < pc.n_sub; ++k) {
        double ua, ud;
        act_stage(a, b, k0 + k, La, Ld, motor, servo, sv, ua, ud);
        plant_step_at(pc, b, st, ua, ud);
    }
    a.k[b] = k0 + pc.n_sub; a.servo[b] = sv;
#pragma unroll
    for (int i = 0; i < 8; ++i) plant[(size_t)b * 8 + i] = st[i];
    double hw, slack;
    const TrackView v = track_view(trk, b, hw, slack);
    cl_local(v, hw, slack, q9_swap, st, local_next + (size_t)b * 6);
    uold_push(u_old + (size_t)b * (2 + sd), sd, servo, motor);
}

// the same with the estimator in the loop: per plant step, plant -> sensors -> observer; the next tick's measurement is made from
// the estimate.  mode 0: only the measurement of the current estimate with u_old = cmd (the first tick of a fleet)
template <bool kObsVeh>
__global__ void __launch_bounds__(64) cl_command_plant_observe_trk_kernel(TrackDev trk, int B, int N, const double *__restrict__ uPred,
                                                                          double *__restrict__ cmd, double *__restrict__ plant, TyrePlantCfg pc,
                                                                          int q9_swap, double *__restrict__ local_next, double *__restrict__ u_old,
                                                                          typename ObsGainsArg<kObsVeh>::type gains, double *__restrict__ obs,
                                                                          ObsParams op, int mode, int sd, ActDev a) {
    __shared__ double G[kObsGainWords];
    if (mode != 0) obs_stage_gains(G, obs_gain_words(gains));
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
        const int k0 = a.k[b], La = a.La[b], Ld = a.Ld[b];
        double sv = a.servo[b];
        for (int k = 0; k < pc.n_sub; ++k) {
            // compiler-only barrier, as in the template: keeps the gain words' LDS loads inside the loop
            asm volatile("" ::: "memory");
            double ua, ud;
            act_stage(a, b, k0 + k, La, Ld, motor, servo, sv, ua, ud);
            plant_step_at(pc, b, st, ua, ud);
            obs_substep<kObsVeh>(G, op, vid, os, st, servo, motor, obs_veh(gains), b);
        }
        a.k[b] = k0 + pc.n_sub; a.servo[b] = sv;
#pragma unroll
        for (int i = 0; i < 8; ++i) plant[(size_t)b * 8 + i] = st[i];
#pragma unroll
        for (int i = 0; i < kObsStride; ++i) obs[(size_t)b * kObsStride + i] = os[i];
    }
    double hw, slack;
    const TrackView v = track_view(trk, b, hw, slack);
    obs_local_state(v, hw, slack, q9_swap, os, local_next + (size_t)b * 6);
    uold_push(u_old + (size_t)b * (2 + sd), sd, servo, motor);
}

hipError_t launch_cl_measure_trk(const FleetMeasureArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_measure_trk_kernel, LPVMPC_GRID(a.B), 0, s, *a.trk, a.B, a.plant, a.cmd, a.q9, a.local_state, a.u_old, a.sd);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_measure_trk(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_measure_trk_kernel, LPVMPC_GRID(a.B), 0, s, *a.trk, a.B, a.N, a.uPred, a.cmd, a.plant, a.tpc, a.q9, a.local_next,
                       a.u_old, a.sd, a.act);
    return hipGetLastError();
}
hipError_t launch_cl_observe_measure_trk(const FleetMeasureArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_trk_kernel<false>, LPVMPC_GRID(a.B), 0, s, *a.trk, a.B, 1, (const double *)nullptr, const_cast<double *>(a.cmd),
                       (double *)nullptr, TyrePlantCfg{}, a.q9, a.local_state, a.u_old, (const double *)nullptr, const_cast<double *>(a.obs),
                       ObsParams{}, 0, a.sd, ActDev{});
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_observe_trk(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_trk_kernel<false>, LPVMPC_GRID(a.B), 0, s, *a.trk, a.B, a.N, a.uPred, a.cmd, a.plant, a.tpc, a.q9, a.local_next,
                       a.u_old, a.gains.g, a.obs, a.op, 1, a.sd, a.act);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_observe_trk_obsveh(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_trk_kernel<true>, LPVMPC_GRID(a.B), 0, s, *a.trk, a.B, a.N, a.uPred, a.cmd, a.plant, a.tpc, a.q9, a.local_next,
                       a.u_old, a.gains, a.obs, a.op, 1, a.sd, a.act);
    return hipGetLastError();
}
hipError_t launch_local_position_trk(const TrackDev &trk, int B, const double *xypsi, double *out, hipStream_t s) {
    hipLaunchKernelGGL(local_position_trk_kernel, LPVMPC_GRID(B), 0, s, trk, B, xypsi, out);
    return hipGetLastError();
}
hipError_t launch_global_position_trk(const TrackDev &trk, int B, const double *sey, double *out, hipStream_t s) {
    hipLaunchKernelGGL(global_position_trk_kernel, LPVMPC_GRID(B), 0, s, trk, B, sey, out);
    return hipGetLastError();
}

}  // namespace lpvmpc
