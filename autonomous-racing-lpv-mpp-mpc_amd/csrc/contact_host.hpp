// contact_host.hpp -- host side of the contact model (lpvmpc_race_contact), shared by race_api.hip, which owns the binding and chooses
// the tick's launch and detaches it before the interactions change, and contact_api.hip, which builds and reads it.  No other
// translation unit includes it.
#pragma once
#include "contact.hpp"
#include "interactions_host.hpp"

// the contact model attached to a race: the kernel argument (the attached interactions' argument copied at the attach -- their binding
// outlives this one, since lpvmpc_race_interactions detaches the contact model first -- plus the model's words and its own device
// memory: carried state and planes), the interactions' block size and the configuration as it was set
struct ContactBinding {
    lpvmpc::ContactDev d{};
    DevArena mem;
    int block = 64;
    lpvmpc_contact_config cfg{};
};
inline Planes lpvmpc_contact_planes(lpvmpc::ContactDev &d, size_t B) {
    return lpvmpc_planes(d, B, LPVMPC_CONTACT_CARRY_F64, LPVMPC_CONTACT_CARRY_I32, LPVMPC_CONTACT_F64, LPVMPC_CONTACT_I32);
}
