// walls_host.hpp -- host side of the walls (lpvmpc_race_walls), shared by race_api.hip, which owns the binding and launches the tick's
// kernel, and walls_api.hip, which builds and reads it.  No other translation unit includes it.
#pragma once
#include "race_attach.hpp"
#include "walls.hpp"

// walls attached to a race: the kernel argument with its device memory (carried state and outputs; track, plant and plant table are
// the race's) and the configuration as it was set.  Owned by the race
struct WallBinding {
    lpvmpc::WallDev d{};
    DevArena mem;
    lpvmpc_wall_config cfg{};
};
inline Planes lpvmpc_wall_planes(lpvmpc::WallDev &d, size_t B) {
    return lpvmpc_planes(d, B, LPVMPC_WALL_CARRY_F64, LPVMPC_WALL_CARRY_I32, LPVMPC_WALL_F64, LPVMPC_WALL_I32);
}
