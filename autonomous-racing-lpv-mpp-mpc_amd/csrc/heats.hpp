// heats.hpp -- kernel argument of the heats (heats.hip; lpvmpc_race_heats, lpvmpc_heat_step_batch): the member lists, what a tick
// reads of each vehicle, and the standings it keeps.  A struct of its own, as the recorder's, so that RaceDev and the race kernels'
// arguments stay as they are.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lpvmpc.h"
#include "lpvmpc_device.hpp"
#include "track_view.hpp"

namespace lpvmpc {

struct HeatDev {                // passed by value
    int B, n_heats, K;                          // K = laps + 2 columns of the line tables (0: none kept, the batch form)
    double hl, hwc;                             // half extents of a footprint
    const int32_t *off, *members;               // [n_heats + 1] first member of each heat; [off[n_heats]] vehicle indices, ascending within a heat
    // what a tick reads: the race form takes the pose from plant and evaluates the track frame, the batch form reads all of it
    const double *plant;                        // [B][8] (race form)
    double hw, slack;                           // the race's half width and slack (race form, no tracks bound)
    const double *pose, *s, *L;                 // [B][3] x y yaw, [B], [B] (batch form)
    const int32_t *inside;                      // [B] (batch form)
    const int32_t *phase;                       // [B]
    // carried state and standings, channel-major and vehicle-minor
    double *carry_f;                            // [LPVMPC_HEAT_CARRY_F64][B]
    int32_t *carry_i;                           // [LPVMPC_HEAT_CARRY_I32][B]
    double *out_f;                              // [LPVMPC_HEAT_F64][B]
    int32_t *out_i;                             // [LPVMPC_HEAT_I32][B]
    int32_t *line_tick, *line_pos;              // [B][K] (null with K = 0)
};

// one tick of the heats: one workgroup per heat, `block` = 64 (no heat of the launch has more than 64 members: one wavefront) or 256.
// Race form, after the tick's command / plant kernel: ccfg the path handle's configuration, trk its track binding (null: unbound),
// t the race's tick number before the increment.  Batch form: everything from h
hipError_t launch_heat_tick(const DevCfg *ccfg, const TrackDev *trk, const HeatDev &h, int block, int t, hipStream_t s);
hipError_t launch_heat_step(const HeatDev &h, int block, int t, hipStream_t s);

}  // namespace lpvmpc
