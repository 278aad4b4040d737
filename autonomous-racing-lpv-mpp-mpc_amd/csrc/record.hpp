// record.hpp -- kernel argument of the race recorder (record.hip, lpvmpc_race_record): the race state it reads and the recorder's
// own buffers.  A struct of its own, so that RaceDev and the race kernels' arguments stay as they are.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lpvmpc.h"
#include "lpvmpc_device.hpp"

namespace lpvmpc {

struct RecDev {                 // passed by value
    int B, N, laps, q9;                         // q9: the race's q9_swap (the lap-0 branch stores ey / epsi in slots 3 / 5)
    double hw, slack;
    // race state (read only)
    const double *plant, *local, *cmd;          // [B][8], [B][6], [B][2]
    const double *ref0, *t_vel;                 // [B][3] the racing measurement's reference point, [B][N+1] the tt handle's vel_ref
    const double *obs;                          // [B][kObsStride] the race's estimator state (null: none)
    const int32_t *phase, *lap, *rk, *src, *iters, *status, *m_plan;   // [B]
    const int32_t *q_iters, *q_status;          // [B] the planner handle's last solve
    // the recorder's buffers
    double *rec_f;                              // [capacity][LPVMPC_REC_F64][B]
    int32_t *rec_i;                             // [capacity][LPVMPC_REC_I32][B]
    double *stat_f;                             // [B][laps + 1][LPVMPC_LAPSTAT_F64]
    int32_t *stat_i;                            // [B][laps + 1][LPVMPC_LAPSTAT_I32]
    int32_t *prev_phase, *end_tick;             // [B] phase after the last recorded tick; tick the vehicle finished / was lost on
};

// one tick of the recorder after the tick's command / plant kernel: t = the race's tick number before the increment, slot = the
// ring slot this tick's record goes to (-1: the tick is not recorded; the lap statistics are updated on every tick)
hipError_t launch_race_record(const DevCfg *ccfg, const RecDev &r, int t, int slot, hipStream_t s);

}  // namespace lpvmpc
