// plant_params.hip -- the per-vehicle forms of the fleet kernels that step the plant (fleet_kernels.hpp, kAct = true, kVeh = true):
// each vehicle steps Simulator.f with its own row [lf lr m Iz Cf Cr mu] of the fleet's plant table (include/lpvmpc.h, "Per-vehicle
// plant parameters"; lpvmpc_*_vehicles).  Always the delayed forms: an all-off actuator passes the command through.  Only the
// launchers live here: this translation unit instantiates the <true, true> forms and no other, so that the plain objects and
// actuator.o compile to the code they have alone (fleet_kernels.hpp).  The measurement kernels need no per-vehicle form: the
// delayed fleets' first-tick measurements (actuator.hip) read no plant parameter.
#include "fleet_kernels.hpp"

namespace lpvmpc {

hipError_t launch_plant_veh(const PlantStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((plant_kernel<true, true>), LPVMPC_GRID(a.B), 0, s, a.B, a.plant, a.u, static_cast<const VehPlantCfg &>(a.tpc), a.act);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_measure_veh(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((cl_command_plant_measure_kernel<true, true>), LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, a.N, a.uPred, a.cmd, a.plant, static_cast<const VehPlantCfg &>(a.tpc), a.hw, a.slack,
                       a.q9, a.local_next, a.u_old, a.sd, a.act);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_observe_veh(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((cl_command_plant_observe_kernel<true, true>), LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, a.N, a.uPred, a.cmd, a.plant, static_cast<const VehPlantCfg &>(a.tpc), a.hw, a.slack,
                       a.q9, a.local_next, a.u_old, a.gains.g, a.obs, a.op, 1, a.sd, a.act);
    return hipGetLastError();
}

hipError_t launch_race_command_plant_veh(const RaceStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((race_command_plant_kernel<true, true>), LPVMPC_GRID(a.r.B), 0, s, a.r, static_cast<const VehPlantCfg &>(a.tpc), a.act);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_observe_veh(const RaceStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((race_command_plant_observe_kernel<true, true>), LPVMPC_GRID(a.r.B), 0, s, a.r, static_cast<const VehPlantCfg &>(a.tpc), a.gains.g, a.obs, a.op, a.act);
    return hipGetLastError();
}

}  // namespace lpvmpc
