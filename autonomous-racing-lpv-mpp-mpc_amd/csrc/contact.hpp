// contact.hpp -- kernel argument of the contact model (contact.hip; lpvmpc_race_contact, lpvmpc_contact_step_batch): the interactions'
// argument as it is plus the corner form's words, what it reads more of each vehicle (Iz; psiDot is word 7 of the plant row) and the
// planes it keeps.  A struct of its own, so that InterDev and interaction_tick_kernel keep their layout.
#pragma once
#include "interactions.hpp"

namespace lpvmpc {

struct ContactDev {             // passed by value
    InterDev i;                                 // the attached interactions' argument: lists, extents, words, plant, planes and carry
    double friction;
    int yaw_response;
    const double *Iz;                           // [B]: row 3 of the live plant table (race form) or the caller's (batch form)
    double *carry_f;                            // [LPVMPC_CONTACT_CARRY_F64][B]
    int32_t *carry_i;                           // [LPVMPC_CONTACT_CARRY_I32][B]
    double *out_f;                              // [LPVMPC_CONTACT_F64][B]
    int32_t *out_i;                             // [LPVMPC_CONTACT_I32][B]
};

// one tick of the interactions with the corner form of the contact: launch_interaction_tick's launch shape and position, in its place
hipError_t launch_contact_tick(const ContactDev &d, int block, int t, hipStream_t s);

}  // namespace lpvmpc
