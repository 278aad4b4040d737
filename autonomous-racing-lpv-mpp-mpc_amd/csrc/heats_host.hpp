// heats_host.hpp -- host side of the heats (lpvmpc_race_heats), shared by race_api.hip, which owns the attachment and launches the
// tick's kernel, heats_api.hip, which builds and reads it, and interactions_api.hip, whose binding reads the attachment's member lists
// and extents.  No other translation unit includes it, so heats.hpp stays out of lpvmpc_handle.hpp and of the other objects'
// dependencies.
#pragma once
#include "heats.hpp"
#include "race_attach.hpp"

// heats attached to a race: the kernel argument with its device memory -- member lists, carried state, standings and line tables --
// and the block size chosen for the largest heat.  Owned by the race, as the recorder
struct HeatsBinding { lpvmpc::HeatDev d{}; DevArena mem; int block = 64; };
inline Planes lpvmpc_heat_planes(lpvmpc::HeatDev &d, size_t B) {
    return lpvmpc_planes(d, B, LPVMPC_HEAT_CARRY_F64, LPVMPC_HEAT_CARRY_I32, LPVMPC_HEAT_F64, LPVMPC_HEAT_I32);
}

// heats_api.hip: the member lists of heat [B] with indices in [-1, n_heats) (off [n_heats + 1], members ascending within a heat,
// largest: the largest heat), and the check of the footprint's extents; both refuse with LPVMPC_E_ARG
LPVMPC_HIDDEN int lpvmpc_heat_members(lpvmpc_handle *h, const char *who, int B, int n_heats, const int32_t *heat, std::vector<int32_t> &off,
                                      std::vector<int32_t> &members, int &largest);
LPVMPC_HIDDEN int lpvmpc_heat_extents(lpvmpc_handle *h, const char *who, const lpvmpc_heats_config *cfg);
