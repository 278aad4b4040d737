// heats_host.hpp -- host side of the heats (lpvmpc_race_heats), shared by race_api.hip, which owns the attachment and launches the
// tick's kernel, and heats_api.hip, which builds and reads it.  No other translation unit includes it, so heats.hpp stays out of
// lpvmpc_handle.hpp and of the other objects' dependencies.
#pragma once
#include "heats.hpp"
#include "lpvmpc_handle.hpp"

// heats attached to a race: the kernel argument with its device memory -- member lists, carried state, standings and line tables --
// and the block size chosen for the largest heat.  Owned by the race, as the recorder
struct HeatsBinding { lpvmpc::HeatDev d{}; DevArena mem; int block = 64; };
