// actuator.hip -- the delayed forms of the fleet kernels that advance a plant (fleet_kernels.hpp, kAct = true): the reference
// simulator's actuator model on the device (include/lpvmpc.h, "Actuator delay and servo lag") and the controllers' steering-delay
// histories.  Only the launchers live here: this translation unit instantiates the <true> forms and no other, so that closed_loop.hip,
// observer.hip and race.hip, which instantiate <false>, compile to the code they have alone (fleet_kernels.hpp).
#include "fleet_kernels.hpp"

namespace lpvmpc {

hipError_t launch_plant_actuated(const PlantStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(plant_kernel<true>, LPVMPC_GRID(a.B), 0, s, a.B, a.plant, a.u, a.pc, a.act);
    return hipGetLastError();
}
hipError_t launch_cl_measure_act(const FleetMeasureArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_measure_kernel<true>, LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, a.plant, a.cmd, a.hw, a.slack, a.q9, a.local_state, a.u_old, a.sd);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_measure_act(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_measure_kernel<true>, LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, a.N, a.uPred, a.cmd, a.plant, a.pc, a.hw, a.slack, a.q9,
                       a.local_next, a.u_old, a.sd, a.act);
    return hipGetLastError();
}

hipError_t launch_cl_observe_measure_act(const FleetMeasureArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_kernel<true>, LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, 1, (const double *)nullptr, const_cast<double *>(a.cmd),
                       (double *)nullptr, PlantCfg{}, a.hw, a.slack, a.q9, a.local_state, a.u_old, (const double *)nullptr, const_cast<double *>(a.obs),
                       ObsParams{}, 0, a.sd, ActDev{});
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_observe_act(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_kernel<true>, LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, a.N, a.uPred, a.cmd, a.plant, a.pc, a.hw, a.slack, a.q9,
                       a.local_next, a.u_old, a.gains.g, a.obs, a.op, 1, a.sd, a.act);
    return hipGetLastError();
}

hipError_t launch_race_measure_act(const RaceMeasureArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(race_measure_kernel<true>, LPVMPC_GRID(a.r.B), 0, s, a.ccfg, a.r, a.seed_tick, a.sd);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_act(const RaceStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(race_command_plant_kernel<true>, LPVMPC_GRID(a.r.B), 0, s, a.r, a.pc, a.act);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_observe_act(const RaceStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(race_command_plant_observe_kernel<true>, LPVMPC_GRID(a.r.B), 0, s, a.r, a.pc, a.gains.g, a.obs, a.op, a.act);
    return hipGetLastError();
}

}  // namespace lpvmpc
