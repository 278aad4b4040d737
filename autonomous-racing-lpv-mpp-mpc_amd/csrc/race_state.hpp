// race_state.hpp -- the inventory of a race's per-vehicle state (lpvmpc_race_snapshot / _restore / _clone, include/lpvmpc.h "Race
// snapshot, restore and clone"): one descriptor per state array, shared by the host code that walks the table (race_state_api.hip),
// the function that fills it (race_api.hip: lpvmpc_race_state) and the two kernels of the clone (race_state.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace lpvmpc {

enum StateType { STATE_F64 = 0, STATE_I32 = 1 };               // = LPVMPC_SNAP_F64 / _I32
enum StateLayout { STATE_VEHICLE_MAJOR = 0, STATE_WORD_MAJOR = 1 };   // [B][W] / [W][B]  (= LPVMPC_SNAP_VEHICLE_MAJOR / _WORD_MAJOR)

// one state array on the device, as the clone's kernels read it: `stage` is the byte offset of its part of the staging buffer,
// which holds the moved vehicles' words in the array's own layout ([moved][W] or [W][moved]), 8-byte aligned
struct StateDescDev {
    void *ptr;
    unsigned long long stage;
    int32_t type, W, layout, pad;
};

// desc [n_desc]; srcv / dstv [moved]: moved vehicle m is written to slot dstv[m] from slot srcv[m].  Every index is checked on the
// host: 0 <= srcv[m], dstv[m] < B.  gather: arrays -> stage; scatter: stage -> arrays; the caller orders the two on one stream
hipError_t launch_race_gather(const StateDescDev *desc, int n_desc, int B, int moved, const int32_t *srcv, char *stage, size_t max_words,
                              hipStream_t s);
hipError_t launch_race_scatter(const StateDescDev *desc, int n_desc, int B, int moved, const int32_t *dstv, const char *stage, size_t max_words,
                               hipStream_t s);

}  // namespace lpvmpc
