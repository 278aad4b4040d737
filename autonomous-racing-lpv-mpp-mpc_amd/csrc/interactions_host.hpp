// interactions_host.hpp -- host side of the interactions (lpvmpc_race_interactions), shared by race_api.hip, which owns the binding
// and launches the tick's kernel, and interactions_api.hip, which builds and reads it.  No other translation unit includes it.
#pragma once
#include "heats_host.hpp"
#include "interactions.hpp"

// interactions attached to a race: the kernel argument with its device memory (the base mu words, carried state and outputs; the
// member lists are the heats'), the heats' block size, the configuration as it was set and, on the host, the base mu words [B] that
// the read-backs return and a detach restores.  Owned by the race next to the heats
struct InterBinding {
    lpvmpc::InterDev d{};
    DevArena mem;
    int block = 64;
    lpvmpc_interaction_config cfg{};
    std::vector<double> mu_base;
};
inline Planes lpvmpc_interaction_planes(lpvmpc::InterDev &d, size_t B) {
    return lpvmpc_planes(d, B, LPVMPC_INTER_CARRY_F64, LPVMPC_INTER_CARRY_I32, LPVMPC_INTER_F64, LPVMPC_INTER_I32);
}

// interactions_api.hip: the interactions' configuration check, its words into the kernel argument, and the planes a vehicle reads
// before its first tick, for contact_api.hip, whose batch form takes the interactions' configuration and writes their planes
LPVMPC_HIDDEN int lpvmpc_interaction_check_config(lpvmpc_handle *h, const char *who, const lpvmpc_interaction_config *c);
LPVMPC_HIDDEN void lpvmpc_interaction_set_config(const lpvmpc_interaction_config &c, lpvmpc::InterDev &d);
LPVMPC_HIDDEN void lpvmpc_interaction_blank_outputs(size_t B, const int32_t *heat_of, const double *mu, std::vector<double> &f, std::vector<int32_t> &i);
