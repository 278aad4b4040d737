// interactions.hpp -- kernel argument of the interactions (interactions.hip; lpvmpc_race_interactions, lpvmpc_interaction_step_batch):
// the heats' member lists and extents, the model's words, what a tick reads and writes of each vehicle, and the outputs it keeps.  A
// struct of its own, as the heats', so that RaceDev, HeatDev and the race kernels' arguments stay as they are.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lpvmpc.h"

namespace lpvmpc {

struct InterDev {               // passed by value
    int B, n_heats;
    double hl, hwc;                             // half extents of a footprint: the heats' own
    const int32_t *off, *members;               // the heats' lists: [n_heats + 1], [off[n_heats]] vehicle indices, ascending within a heat
    double draft_gain, wake_length, wake_half_width, restitution, push;
    int contact;
    // what a tick reads and writes.  Race form: plant = RaceDev::plant, nstep = RaceDev::nstep, m / mu_live = rows 2 / 6 of the live
    // plant table [7][B], mu_base the binding's copy of the caller's row 6.  Batch form: the caller's arrays
    double *plant;                              // [B][8] x y vx vy ax ay yaw psiDot, in / out
    const int32_t *nstep;                       // [B] simulator steps of this tick (null: every vehicle steps)
    const double *m, *mu_base;                  // [B] each
    double *mu_live;                            // [B] out
    // carried state and outputs, channel-major and vehicle-minor
    double *carry_f;                            // [LPVMPC_INTER_CARRY_F64][B]
    int32_t *carry_i;                           // [LPVMPC_INTER_CARRY_I32][B]
    double *out_f;                              // [LPVMPC_INTER_F64][B]
    int32_t *out_i;                             // [LPVMPC_INTER_I32][B]
};

// one tick of the interactions: one workgroup per heat, `block` = 64 (no heat of the launch has more than 64 members: one wavefront)
// or 256, the heats' own choice.  In front of the tick's command / plant kernel (behind the disturbances'); t the tick number before
// the increment.  The race and the batch call fill h from their own arrays and launch the same kernel
hipError_t launch_interaction_tick(const InterDev &h, int block, int t, hipStream_t s);

}  // namespace lpvmpc
