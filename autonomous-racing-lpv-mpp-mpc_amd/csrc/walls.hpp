// walls.hpp -- kernel argument of the walls (walls.hip; lpvmpc_race_walls, lpvmpc_wall_step_batch): the track a corner is located on,
// the model's words, what a tick reads and writes of each vehicle, and the outputs it keeps.  A struct of its own, as the
// interactions', so that RaceDev and the race kernels' arguments stay as they are.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lpvmpc.h"
#include "track_view.hpp"

namespace lpvmpc {

struct WallDev {                // passed by value
    int B;
    int rows;                                   // rows of tab in use (no tracks bound)
    const double *tab;                          // the handle's own track table [rows][6] on the device (DevCfg::track); unused when trk.tab
    double hw;                                  // the race's half width (no tracks bound)
    TrackDev trk;                               // the handle's track binding; trk.tab null: none, every vehicle is on tab
    double margin, reach, hl, hwc, restitution, friction, push;
    int yaw_response;
    // what a tick reads and writes.  Race form: plant = RaceDev::plant, nstep = RaceDev::nstep, m / Iz = rows 2 / 3 of the live plant
    // table [7][B].  Batch form: the caller's arrays
    double *plant;                              // [B][8] x y vx vy ax ay yaw psiDot, in / out
    const int32_t *nstep;                       // [B] simulator steps of this tick (null: every vehicle steps)
    const double *m, *Iz;                       // [B] each
    // carried state and outputs, channel-major and vehicle-minor
    double *carry_f;                            // [LPVMPC_WALL_CARRY_F64][B]
    int32_t *carry_i;                           // [LPVMPC_WALL_CARRY_I32][B]
    double *out_f;                              // [LPVMPC_WALL_F64][B]
    int32_t *out_i;                             // [LPVMPC_WALL_I32][B]
};

// one tick of the walls: four lanes per vehicle, 256-thread workgroups of 64 vehicles.  In front of the tick's command / plant kernel
// (behind the disturbances' and the interactions'); t the tick number before the increment.  The race and the batch call fill h from
// their own arrays and launch the same kernel
hipError_t launch_wall_tick(const WallDev &h, int t, hipStream_t s);

}  // namespace lpvmpc
