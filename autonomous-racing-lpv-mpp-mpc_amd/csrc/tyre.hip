// tyre.hip -- the tyre forms of the fleet kernels that step the plant (fleet_kernels.hpp, kAct = kVeh = kTyre = true): each vehicle
// steps Simulator.f with its own plant row and its own tyre row [kind B C c_f] of the fleet's tyre table (include/lpvmpc.h, "Tyre
// model"; lpvmpc_*_tyres) -- the linear tyre of the plant row, or Simulator.pacejka on both axles.  Only the launchers live here:
// this translation unit instantiates the <true, true, true> forms (and the curve's own kernel) and no other, so that every other
// object compiles to the code it has alone (fleet_kernels.hpp).
#include "fleet_kernels.hpp"

namespace lpvmpc {

hipError_t launch_plant_tyre(const PlantStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((plant_kernel<true, true, true>), LPVMPC_GRID(a.B), 0, s, a.B, a.plant, a.u, a.tpc, a.act);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_measure_tyre(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((cl_command_plant_measure_kernel<true, true, true>), LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, a.N, a.uPred, a.cmd, a.plant, a.tpc, a.hw, a.slack,
                       a.q9, a.local_next, a.u_old, a.sd, a.act);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_observe_tyre(const FleetStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((cl_command_plant_observe_kernel<true, true, true>), LPVMPC_GRID(a.B), 0, s, a.dcfg, a.B, a.N, a.uPred, a.cmd, a.plant, a.tpc, a.hw, a.slack,
                       a.q9, a.local_next, a.u_old, a.gains.g, a.obs, a.op, 1, a.sd, a.act);
    return hipGetLastError();
}

hipError_t launch_race_command_plant_tyre(const RaceStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((race_command_plant_kernel<true, true, true>), LPVMPC_GRID(a.r.B), 0, s, a.r, a.tpc, a.act);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_observe_tyre(const RaceStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((race_command_plant_observe_kernel<true, true, true>), LPVMPC_GRID(a.r.B), 0, s, a.r, a.tpc, a.gains.g, a.obs, a.op, a.act);
    return hipGetLastError();
}

hipError_t launch_tyre_force(int B, const double *tyre, const double *m, const double *alpha, double *force, hipStream_t s) {
    hipLaunchKernelGGL((tyre_force_kernel<true>), LPVMPC_GRID(B), 0, s, B, tyre, m, alpha, force);
    return hipGetLastError();
}

}  // namespace lpvmpc
