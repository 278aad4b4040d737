// fleet_launch.hip -- binds the kernel enumerators of step_form.hpp to the launchers that stand next to their kernels (one form per
// translation unit: fleet_kernels.hpp).  Host code only, no kernel: the ticks and the stand-alone steps fill their family's argument
// struct, work out the form (step_form) and launch what the functions below return; null: the form has no kernel, the caller refuses.
#include "lpvmpc_device.hpp"
#include "step_form.hpp"

namespace lpvmpc {

template <class Fn> struct LaunchRow { int kernel; Fn *fn; };
// row i serves enumerator i, and every enumerator has its row
template <class Fn, int n> constexpr bool launch_rows_ok(const LaunchRow<Fn> (&tab)[n], int count) {
    for (int i = 0; i < n; ++i) if (tab[i].kernel != i) return false;
    return n == count;
}
template <class Fn, int n> static Fn *launcher(const LaunchRow<Fn> (&tab)[n], int kernel) { return kernel < 0 ? nullptr : tab[kernel].fn; }

static constexpr LaunchRow<FleetStepFn> kFleetStepFn[] = {
    {FS_TRK_OBS_OBSVEH, launch_cl_command_plant_observe_trk_obsveh}, {FS_TRK_OBS, launch_cl_command_plant_observe_trk},
    {FS_TRK, launch_cl_command_plant_measure_trk}, {FS_FAULT_OBSVEH, launch_cl_command_plant_observe_faulted_obsveh},
    {FS_FAULT, launch_cl_command_plant_observe_faulted}, {FS_TYRE_OBS_OBSVEH, launch_cl_command_plant_observe_tyre_obsveh},
    {FS_VEH_OBS_OBSVEH, launch_cl_command_plant_observe_veh_obsveh}, {FS_TYRE_OBS, launch_cl_command_plant_observe_tyre},
    {FS_TYRE, launch_cl_command_plant_measure_tyre}, {FS_VEH_OBS, launch_cl_command_plant_observe_veh},
    {FS_VEH, launch_cl_command_plant_measure_veh}, {FS_ACT_OBS, launch_cl_command_plant_observe_act}, {FS_ACT, launch_cl_command_plant_measure_act},
    {FS_OBS, launch_cl_command_plant_observe}, {FS_PLAIN, launch_cl_command_plant_measure},
};
static constexpr LaunchRow<FleetMeasureFn> kFleetMeasureFn[] = {
    {FM_TRK_OBS, launch_cl_observe_measure_trk}, {FM_TRK, launch_cl_measure_trk}, {FM_ACT_OBS, launch_cl_observe_measure_act},
    {FM_ACT, launch_cl_measure_act},             {FM_OBS, launch_cl_observe_measure}, {FM_PLAIN, launch_cl_measure},
};
static constexpr LaunchRow<RaceStepFn> kRaceStepFn[] = {
    {RS_FAULT_OBSVEH, launch_race_command_plant_observe_faulted_obsveh}, {RS_FAULT, launch_race_command_plant_observe_faulted},
    {RS_TYRE_OBS_OBSVEH, launch_race_command_plant_observe_tyre_obsveh}, {RS_VEH_OBS_OBSVEH, launch_race_command_plant_observe_veh_obsveh},
    {RS_TYRE_OBS, launch_race_command_plant_observe_tyre}, {RS_TYRE, launch_race_command_plant_tyre},
    {RS_VEH_OBS, launch_race_command_plant_observe_veh}, {RS_VEH, launch_race_command_plant_veh},
    {RS_ACT_OBS, launch_race_command_plant_observe_act}, {RS_ACT, launch_race_command_plant_act}, {RS_OBS, launch_race_command_plant_observe},
    {RS_PLAIN, launch_race_command_plant},
};
static constexpr LaunchRow<RaceMeasureFn> kRaceMeasureFn[] = {{RM_TRK, launch_race_measure_trk}, {RM_ACT, launch_race_measure_act}, {RM_PLAIN, launch_race_measure}};
static constexpr LaunchRow<PlantStepFn> kPlantStepFn[] = {{PS_TYRE, launch_plant_tyre}, {PS_VEH, launch_plant_veh}, {PS_ACT, launch_plant_actuated},
                                                          {PS_PLAIN, launch_plant}};
static_assert(launch_rows_ok(kFleetStepFn, FS_COUNT) && launch_rows_ok(kFleetMeasureFn, FM_COUNT) && launch_rows_ok(kRaceStepFn, RS_COUNT) &&
              launch_rows_ok(kRaceMeasureFn, RM_COUNT) && launch_rows_ok(kPlantStepFn, PS_COUNT), "one launcher per kernel enumerator, in the enumerators' order");

FleetStepFn *fleet_step_launcher(unsigned form) { return launcher(kFleetStepFn, fleet_step_kernel(form)); }
FleetMeasureFn *fleet_measure_launcher(unsigned form) { return launcher(kFleetMeasureFn, fleet_measure_kernel(form)); }
RaceStepFn *race_step_launcher(unsigned form) { return launcher(kRaceStepFn, race_step_kernel(form)); }
RaceMeasureFn *race_measure_launcher(unsigned form) { return launcher(kRaceMeasureFn, race_measure_kernel(form)); }
PlantStepFn *plant_step_launcher(unsigned form) { return launcher(kPlantStepFn, plant_step_kernel(form)); }

}  // namespace lpvmpc
