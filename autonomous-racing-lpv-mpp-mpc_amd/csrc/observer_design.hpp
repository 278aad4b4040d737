// observer_design.hpp -- what observer_design.hip (kernel) and observer_design_api.hip (C ABI) share: the layout of the design's
// constant block on the device and the launcher.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lpvmpc {

// the words every problem of a design reads, made once on the host: Qo [6][6], G = C^T Ro^-1 C [6][6], C^T Ro^-1 [6][5] and the
// two limit tables [2][6][2] (LS, HS)
struct ObsDesignConst {
    static constexpr int kQo = 0, kG = 36, kCtRi = 72, kLim = 102, kWords = 126;
};

// rows [B][7], cst [ObsDesignConst::kWords]; gain element e of vertex i of vehicle b goes to L[b * stride_b + e * stride_e + i * stride_i];
// iters [B][2][16] or null
hipError_t launch_observer_design(int B, const double *rows, const double *cst, double *L_ls, double *L_hs, long long stride_b,
                                  long long stride_e, long long stride_i, int32_t *iters, hipStream_t s);

}  // namespace lpvmpc
