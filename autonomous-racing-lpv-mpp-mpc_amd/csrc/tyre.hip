// tyre.hip -- the tyre forms of the fleet kernels that step the plant (fleet_kernels.hpp, kAct = kVeh = kTyre = true): each vehicle
// steps Simulator.f with its own plant row and its own tyre row [kind B C c_f] of the fleet's tyre table (include/lpvmpc.h, "Tyre
// model"; lpvmpc_*_tyres) -- the linear tyre of the plant row, or Simulator.pacejka on both axles.  Only the launchers live here:
// this translation unit instantiates the <true, true, true> forms (and the curve's own kernel) and no other, so that every other
// object compiles to the code it has alone (fleet_kernels.hpp).
#include "fleet_kernels.hpp"

namespace lpvmpc {

#define LPVMPC_GRID(n) dim3(((n) + 63) / 64), dim3(64)
hipError_t launch_plant_tyre(int B, double *plant, const double *u, const TyrePlantCfg &pc, const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL((plant_kernel<true, true, true>), LPVMPC_GRID(B), 0, s, B, plant, u, pc, a);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_measure_tyre(const DevCfg *dcfg, int B, int N, const double *uPred, double *cmd, double *plant,
                                                const TyrePlantCfg &pc, double hw, double slack, int q9_swap, double *local_next, double *u_old,
                                                int sd, const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL((cl_command_plant_measure_kernel<true, true, true>), LPVMPC_GRID(B), 0, s, dcfg, B, N, uPred, cmd, plant, pc, hw, slack,
                       q9_swap, local_next, u_old, sd, a);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_observe_tyre(const DevCfg *dcfg, int B, int N, const double *uPred, double *cmd, double *plant,
                                                const TyrePlantCfg &pc, double hw, double slack, int q9_swap, double *local_next, double *u_old,
                                                int sd, const double *gains, double *obs, const ObsParams &op, const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL((cl_command_plant_observe_kernel<true, true, true>), LPVMPC_GRID(B), 0, s, dcfg, B, N, uPred, cmd, plant, pc, hw, slack,
                       q9_swap, local_next, u_old, gains, obs, op, 1, sd, a);
    return hipGetLastError();
}

hipError_t launch_race_command_plant_tyre(const RaceDev &r, const TyrePlantCfg &pc, const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL((race_command_plant_kernel<true, true, true>), LPVMPC_GRID(r.B), 0, s, r, pc, a);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_observe_tyre(const RaceDev &r, const TyrePlantCfg &pc, const double *gains, double *obs, const ObsParams &op,
                                                 const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL((race_command_plant_observe_kernel<true, true, true>), LPVMPC_GRID(r.B), 0, s, r, pc, gains, obs, op, a);
    return hipGetLastError();
}

hipError_t launch_tyre_force(int B, const double *tyre, const double *m, const double *alpha, double *force, hipStream_t s) {
    hipLaunchKernelGGL((tyre_force_kernel<true>), LPVMPC_GRID(B), 0, s, B, tyre, m, alpha, force);
    return hipGetLastError();
}

}  // namespace lpvmpc
