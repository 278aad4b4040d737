// step_form.hpp -- which kernel advances a plant: the form of a fleet, race or stand-alone step as a bit set, and per kernel family
// one table from the normalised form to the kernel that serves it.  Host only and free of HIP (a plain C++17 compiler takes it alone:
// tests/test_step_form_host.py); the launchers behind the enumerators are bound in fleet_launch.hip.  A form without a row has no
// kernel: the caller refuses it, it never falls through to a neighbouring kernel that would ignore a bound table.
#pragma once

namespace lpvmpc {

enum StepBit : unsigned {
    SF_ACT = 1,        // delayed kernels: actuator stage in the plant, controller histories
    SF_VEH = 2,        // the fleet's plant table
    SF_TYRE = 4,       // the fleet's tyre table
    SF_OBS = 8,        // the estimator in the loop
    SF_OBSVEH = 16,    // per-vehicle estimator gains
    SF_TRK = 32,       // per-vehicle tracks
    SF_FAULT = 64,     // sensor faults
};
using StepForm = unsigned;
constexpr StepForm SF_VEHS = SF_ACT | SF_VEH, SF_TYRES = SF_VEHS | SF_TYRE;   // the _vehicles and _tyres starts

// the raw facts of an engine, normalised: a tyre table comes with a plant table, a plant table with the delayed kernels, and the
// per-vehicle gains count only where an estimator runs on a plant table
constexpr StepForm step_form(bool actuated, bool plant_table, bool tyre_table, bool estimator, bool obsveh_bound, bool track_bound, bool faults) {
    const bool veh = plant_table || tyre_table, act = actuated || veh;
    return (act ? SF_ACT : 0u) | (veh ? SF_VEH : 0u) | (tyre_table ? SF_TYRE : 0u) | (estimator ? SF_OBS : 0u) |
           (obsveh_bound && estimator && veh ? SF_OBSVEH : 0u) | (track_bound ? SF_TRK : 0u) | (faults ? SF_FAULT : 0u);
}

struct StepRow { StepForm form; int kernel; const char *name; };
#define LPVMPC_STEP_ROW(form, k) {form, k, #k}
// the row of `form` among the bits the family looks at; -1: no kernel
template <int n> constexpr int step_kernel(const StepRow (&tab)[n], StepForm mask, StepForm form) {
    for (int i = 0; i < n; ++i) if (tab[i].form == (form & mask)) return tab[i].kernel;
    return -1;
}

// Fleet step (lpvmpc_cl_tick): the command / plant / measure-or-observe kernel at the end of a tick.  Tracks and faults come with the
// _tyres start only (lpvmpc_set_tracks, lpvmpc_set_sensor_faults), faults with an estimator; a fleet with faults and tracks is refused
// when the faults are attached (the faulted kernel has no track form), so that form has no row here.
enum FleetStepKernel { FS_TRK_OBS_OBSVEH, FS_TRK_OBS, FS_TRK, FS_FAULT_OBSVEH, FS_FAULT, FS_TYRE_OBS_OBSVEH, FS_VEH_OBS_OBSVEH, FS_TYRE_OBS,
                       FS_TYRE, FS_VEH_OBS, FS_VEH, FS_ACT_OBS, FS_ACT, FS_OBS, FS_PLAIN, FS_COUNT };
constexpr StepRow kFleetStep[] = {
    LPVMPC_STEP_ROW(SF_TRK | SF_TYRES | SF_OBS | SF_OBSVEH, FS_TRK_OBS_OBSVEH), LPVMPC_STEP_ROW(SF_TRK | SF_TYRES | SF_OBS, FS_TRK_OBS),
    LPVMPC_STEP_ROW(SF_TRK | SF_TYRES, FS_TRK), LPVMPC_STEP_ROW(SF_FAULT | SF_TYRES | SF_OBS | SF_OBSVEH, FS_FAULT_OBSVEH),
    LPVMPC_STEP_ROW(SF_FAULT | SF_TYRES | SF_OBS, FS_FAULT), LPVMPC_STEP_ROW(SF_TYRES | SF_OBS | SF_OBSVEH, FS_TYRE_OBS_OBSVEH),
    LPVMPC_STEP_ROW(SF_VEHS | SF_OBS | SF_OBSVEH, FS_VEH_OBS_OBSVEH), LPVMPC_STEP_ROW(SF_TYRES | SF_OBS, FS_TYRE_OBS),
    LPVMPC_STEP_ROW(SF_TYRES, FS_TYRE), LPVMPC_STEP_ROW(SF_VEHS | SF_OBS, FS_VEH_OBS), LPVMPC_STEP_ROW(SF_VEHS, FS_VEH),
    LPVMPC_STEP_ROW(SF_ACT | SF_OBS, FS_ACT_OBS), LPVMPC_STEP_ROW(SF_ACT, FS_ACT), LPVMPC_STEP_ROW(SF_OBS, FS_OBS), LPVMPC_STEP_ROW(0, FS_PLAIN),
};
constexpr int fleet_step_kernel(StepForm f) { return step_kernel(kFleetStep, ~0u, f); }

// Fleet first measurement (lpvmpc_cl_tick before the first step, which makes every later tick's measurement): the bound kernels
// read each vehicle's own track; otherwise the delayed form differs by its controller histories only
enum FleetMeasureKernel { FM_TRK_OBS, FM_TRK, FM_ACT_OBS, FM_ACT, FM_OBS, FM_PLAIN, FM_COUNT };
constexpr StepRow kFleetMeasure[] = {
    LPVMPC_STEP_ROW(SF_TRK | SF_ACT | SF_OBS, FM_TRK_OBS), LPVMPC_STEP_ROW(SF_TRK | SF_ACT, FM_TRK), LPVMPC_STEP_ROW(SF_ACT | SF_OBS, FM_ACT_OBS),
    LPVMPC_STEP_ROW(SF_ACT, FM_ACT),                       LPVMPC_STEP_ROW(SF_OBS, FM_OBS),          LPVMPC_STEP_ROW(0, FM_PLAIN),
};
constexpr int fleet_measure_kernel(StepForm f) { return step_kernel(kFleetMeasure, SF_TRK | SF_ACT | SF_OBS, f); }

// Race step (lpvmpc_race_tick): as the fleet's, but the step kernels of a race read no track (its measurement does), so the track bit
// is not looked at and a race with faults and tracks is served
enum RaceStepKernel { RS_FAULT_OBSVEH, RS_FAULT, RS_TYRE_OBS_OBSVEH, RS_VEH_OBS_OBSVEH, RS_TYRE_OBS, RS_TYRE, RS_VEH_OBS, RS_VEH, RS_ACT_OBS,
                      RS_ACT, RS_OBS, RS_PLAIN, RS_COUNT };
constexpr StepRow kRaceStep[] = {
    LPVMPC_STEP_ROW(SF_FAULT | SF_TYRES | SF_OBS | SF_OBSVEH, RS_FAULT_OBSVEH), LPVMPC_STEP_ROW(SF_FAULT | SF_TYRES | SF_OBS, RS_FAULT),
    LPVMPC_STEP_ROW(SF_TYRES | SF_OBS | SF_OBSVEH, RS_TYRE_OBS_OBSVEH), LPVMPC_STEP_ROW(SF_VEHS | SF_OBS | SF_OBSVEH, RS_VEH_OBS_OBSVEH),
    LPVMPC_STEP_ROW(SF_TYRES | SF_OBS, RS_TYRE_OBS), LPVMPC_STEP_ROW(SF_TYRES, RS_TYRE), LPVMPC_STEP_ROW(SF_VEHS | SF_OBS, RS_VEH_OBS),
    LPVMPC_STEP_ROW(SF_VEHS, RS_VEH), LPVMPC_STEP_ROW(SF_ACT | SF_OBS, RS_ACT_OBS), LPVMPC_STEP_ROW(SF_ACT, RS_ACT), LPVMPC_STEP_ROW(SF_OBS, RS_OBS),
    LPVMPC_STEP_ROW(0, RS_PLAIN),
};
constexpr int race_step_kernel(StepForm f) { return step_kernel(kRaceStep, ~(StepForm)SF_TRK, f); }

// Race measurement: the bound kernel (tracks come with the _tyres start, hence with the delayed form), the delayed one, the plain one
enum RaceMeasureKernel { RM_TRK, RM_ACT, RM_PLAIN, RM_COUNT };
constexpr StepRow kRaceMeasure[] = {LPVMPC_STEP_ROW(SF_TRK | SF_ACT, RM_TRK), LPVMPC_STEP_ROW(SF_ACT, RM_ACT), LPVMPC_STEP_ROW(0, RM_PLAIN)};
constexpr int race_measure_kernel(StepForm f) { return step_kernel(kRaceMeasure, SF_TRK | SF_ACT, f); }

// Stand-alone plant step (lpvmpc_plant_step_*_batch): the plant alone, no estimator, track or faults to look at
enum PlantStepKernel { PS_TYRE, PS_VEH, PS_ACT, PS_PLAIN, PS_COUNT };
constexpr StepRow kPlantStep[] = {LPVMPC_STEP_ROW(SF_TYRES, PS_TYRE), LPVMPC_STEP_ROW(SF_VEHS, PS_VEH), LPVMPC_STEP_ROW(SF_ACT, PS_ACT),
                                  LPVMPC_STEP_ROW(0, PS_PLAIN)};
constexpr int plant_step_kernel(StepForm f) { return step_kernel(kPlantStep, SF_TYRES, f); }
#undef LPVMPC_STEP_ROW

}  // namespace lpvmpc
