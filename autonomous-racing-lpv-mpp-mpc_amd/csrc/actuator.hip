// actuator.hip -- the delayed forms of the fleet kernels that advance a plant (fleet_kernels.hpp, kAct = true): the reference
// simulator's actuator model on the device (include/lpvmpc.h, "Actuator delay and servo lag") and the controllers' steering-delay
// histories.  Only the launchers live here: this translation unit instantiates the <true> forms and no other, so that closed_loop.hip,
// observer.hip and race.hip, which instantiate <false>, compile to the code they have alone (fleet_kernels.hpp).
#include "fleet_kernels.hpp"

namespace lpvmpc {

#define LPVMPC_GRID(n) dim3(((n) + 63) / 64), dim3(64)
hipError_t launch_plant_actuated(int B, double *plant, const double *u, PlantCfg pc, const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL(plant_kernel<true>, LPVMPC_GRID(B), 0, s, B, plant, u, pc, a);
    return hipGetLastError();
}
hipError_t launch_cl_measure_act(const DevCfg *dcfg, int B, const double *plant, const double *cmd, double hw, double slack, int q9_swap,
                                 double *local_state, double *u_old, int sd, hipStream_t s) {
    hipLaunchKernelGGL(cl_measure_kernel<true>, LPVMPC_GRID(B), 0, s, dcfg, B, plant, cmd, hw, slack, q9_swap, local_state, u_old, sd);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_measure_act(const DevCfg *dcfg, int B, int N, const double *uPred, double *cmd, double *plant, PlantCfg pc,
                                               double hw, double slack, int q9_swap, double *local_next, double *u_old, int sd,
                                               const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_measure_kernel<true>, LPVMPC_GRID(B), 0, s, dcfg, B, N, uPred, cmd, plant, pc, hw, slack, q9_swap,
                       local_next, u_old, sd, a);
    return hipGetLastError();
}

hipError_t launch_cl_observe_measure_act(const DevCfg *dcfg, int B, const double *obs, const double *cmd, double hw, double slack, int q9_swap,
                                         double *local_state, double *u_old, int sd, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_kernel<true>, LPVMPC_GRID(B), 0, s, dcfg, B, 1, (const double *)nullptr, const_cast<double *>(cmd),
                       (double *)nullptr, PlantCfg{}, hw, slack, q9_swap, local_state, u_old, (const double *)nullptr, const_cast<double *>(obs),
                       ObsParams{}, 0, sd, ActDev{});
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_observe_act(const DevCfg *dcfg, int B, int N, const double *uPred, double *cmd, double *plant, PlantCfg pc,
                                              double hw, double slack, int q9_swap, double *local_next, double *u_old, int sd,
                                              const double *gains, double *obs, const ObsParams &op, const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_kernel<true>, LPVMPC_GRID(B), 0, s, dcfg, B, N, uPred, cmd, plant, pc, hw, slack, q9_swap,
                       local_next, u_old, gains, obs, op, 1, sd, a);
    return hipGetLastError();
}

hipError_t launch_race_measure_act(const DevCfg *ccfg, const RaceDev &r, int seed_tick, int sd, hipStream_t s) {
    hipLaunchKernelGGL(race_measure_kernel<true>, LPVMPC_GRID(r.B), 0, s, ccfg, r, seed_tick, sd);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_act(const RaceDev &r, PlantCfg pc, const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL(race_command_plant_kernel<true>, LPVMPC_GRID(r.B), 0, s, r, pc, a);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_observe_act(const RaceDev &r, PlantCfg pc, const double *gains, double *obs, const ObsParams &op,
                                                const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL(race_command_plant_observe_kernel<true>, LPVMPC_GRID(r.B), 0, s, r, pc, gains, obs, op, a);
    return hipGetLastError();
}

}  // namespace lpvmpc
