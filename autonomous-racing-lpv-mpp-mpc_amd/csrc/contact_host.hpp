// contact_host.hpp -- host side of the contact model (lpvmpc_race_contact), shared by race_api.hip, which owns the binding and chooses
// the tick's launch, contact_api.hip, which builds and reads it, and interactions_api.hip, which detaches it before the interactions
// change.  No other translation unit includes it.
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

// race_api.hip: what lpvmpc_race_contact needs of the running race (false: the handle owns no race)
struct RaceContactView {
    int B = 0;
    PlantSide *side = nullptr;
    const HeatsBinding *heats = nullptr;
    const InterBinding *inter = nullptr;
    std::unique_ptr<ContactBinding> *slot = nullptr;
};
LPVMPC_HIDDEN bool lpvmpc_race_contact_view(lpvmpc_handle *h, RaceContactView &v);
// contact_api.hip: back to the centres form (no race or nothing attached: nothing to do)
LPVMPC_HIDDEN int lpvmpc_race_contact_detach(lpvmpc_handle *h);
