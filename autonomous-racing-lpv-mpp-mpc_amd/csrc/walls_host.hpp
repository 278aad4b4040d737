// walls_host.hpp -- host side of the walls (lpvmpc_race_walls), shared by race_api.hip, which owns the binding and launches the tick's
// kernel, and walls_api.hip, which builds and reads it.  No other translation unit includes it.
#pragma once
#include "lpvmpc_handle.hpp"
#include "walls.hpp"

// walls attached to a race: the kernel argument with its device memory (carried state and outputs; track, plant and plant table are
// the race's) and the configuration as it was set.  Owned by the race
struct WallBinding {
    lpvmpc::WallDev d{};
    DevArena mem;
    lpvmpc_wall_config cfg{};
};

// race_api.hip: what lpvmpc_race_walls needs of the running race: the state a tick reads and writes, the race's half width, the plant
// side whose table holds m and Iz, and the slot that owns the binding (false: the handle owns no race)
struct RaceWallView {
    int B = 0;
    double hw = 0.0;
    double *plant = nullptr;
    const int32_t *nstep = nullptr;
    PlantSide *side = nullptr;
    std::unique_ptr<WallBinding> *slot = nullptr;
};
LPVMPC_HIDDEN bool lpvmpc_race_wall_view(lpvmpc_handle *h, RaceWallView &v);
