// events_host.hpp -- host side of the race event log (lpvmpc_race_events), shared by race_api.hip, which owns the binding and launches
// the tick's kernel, and events_api.hip, which builds and reads it.  No other translation unit includes it.
#pragma once
#include "events.hpp"
#include "race_attach.hpp"

// the log attached to a race: the kernel argument with its device memory (carry, outputs, the ring, the count, the table of each
// vehicle's heat), the configuration as it was set, and the serials of the heats' and the walls' slots that its last tick saw (known:
// it has seen one at all).  It holds no pointer of another layer.  Owned by the race
struct EventBinding {
    lpvmpc::EventDev d{};
    DevArena mem;
    lpvmpc_event_config cfg{};
    int32_t *heat_of = nullptr;                 // [B], filled at the first sight of an attachment of the heats
    uint32_t heats_serial = 0, walls_serial = 0;
    bool heats_known = false, walls_known = false;
};
inline Planes lpvmpc_event_planes(lpvmpc::EventDev &d, size_t B) {
    return lpvmpc_planes(d, B, LPVMPC_EVENT_CARRY_F64, LPVMPC_EVENT_CARRY_I32, 0, LPVMPC_EVENT_OUT_I32);
}
