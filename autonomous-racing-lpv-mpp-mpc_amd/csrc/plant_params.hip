// plant_params.hip -- the per-vehicle forms of the fleet kernels that step the plant (fleet_kernels.hpp, kAct = true, kVeh = true):
// each vehicle steps Simulator.f with its own row [lf lr m Iz Cf Cr mu] of the fleet's plant table (include/lpvmpc.h, "Per-vehicle
// plant parameters"; lpvmpc_*_vehicles).  Always the delayed forms: an all-off actuator passes the command through.  Only the
// launchers live here: this translation unit instantiates the <true, true> forms and no other, so that the plain objects and
// actuator.o compile to the code they have alone (fleet_kernels.hpp).  The measurement kernels need no per-vehicle form: the
// delayed fleets' first-tick measurements (actuator.hip) read no plant parameter.
#include "fleet_kernels.hpp"

namespace lpvmpc {

#define LPVMPC_GRID(n) dim3(((n) + 63) / 64), dim3(64)
hipError_t launch_plant_veh(int B, double *plant, const double *u, const VehPlantCfg &pc, const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL((plant_kernel<true, true>), LPVMPC_GRID(B), 0, s, B, plant, u, pc, a);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_measure_veh(const DevCfg *dcfg, int B, int N, const double *uPred, double *cmd, double *plant,
                                               const VehPlantCfg &pc, double hw, double slack, int q9_swap, double *local_next, double *u_old,
                                               int sd, const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL((cl_command_plant_measure_kernel<true, true>), LPVMPC_GRID(B), 0, s, dcfg, B, N, uPred, cmd, plant, pc, hw, slack,
                       q9_swap, local_next, u_old, sd, a);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_observe_veh(const DevCfg *dcfg, int B, int N, const double *uPred, double *cmd, double *plant,
                                               const VehPlantCfg &pc, double hw, double slack, int q9_swap, double *local_next, double *u_old,
                                               int sd, const double *gains, double *obs, const ObsParams &op, const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL((cl_command_plant_observe_kernel<true, true>), LPVMPC_GRID(B), 0, s, dcfg, B, N, uPred, cmd, plant, pc, hw, slack,
                       q9_swap, local_next, u_old, gains, obs, op, 1, sd, a);
    return hipGetLastError();
}

hipError_t launch_race_command_plant_veh(const RaceDev &r, const VehPlantCfg &pc, const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL((race_command_plant_kernel<true, true>), LPVMPC_GRID(r.B), 0, s, r, pc, a);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_observe_veh(const RaceDev &r, const VehPlantCfg &pc, const double *gains, double *obs, const ObsParams &op,
                                                const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL((race_command_plant_observe_kernel<true, true>), LPVMPC_GRID(r.B), 0, s, r, pc, gains, obs, op, a);
    return hipGetLastError();
}

}  // namespace lpvmpc
