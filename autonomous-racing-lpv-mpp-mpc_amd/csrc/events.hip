// events.hip -- the race event log's kernels (include/lpvmpc.h, "Race event log"): one tick of events.hpp's device function in its two
// forms, and the table of each vehicle's heat.  One workgroup of kEventBlock threads per launch: the tick's slots come from a prefix
// sum over the vehicle index inside that workgroup ("Race event log", says why not three launches).  Its own
// translation unit, compiled as heats.o (PROGRESS[i] - PROGRESS[j] is one rounded subtraction) and gated alike: no scratch.
#include "events.hpp"

namespace lpvmpc {

__global__ void __launch_bounds__(kEventBlock) event_tick_kernel(EventDev e, EventSrc s, int t) {
    __shared__ int lds[64];
    event_tick<false>(e, s, t, lds);
}

__global__ void __launch_bounds__(kEventBlock) event_step_kernel(EventDev e, EventSrc s, int t) {
    __shared__ int lds[64];
    event_tick<true>(e, s, t, lds);
}

// member slot k of heat g: heat_of[members[k]] = g.  A vehicle is in at most one heat, so no two threads write one word
__global__ void __launch_bounds__(256) event_heat_of_kernel(int B, int n_heats, const int32_t *__restrict__ off,
                                                            const int32_t *__restrict__ members, int32_t *__restrict__ heat_of) {
    const int g = blockIdx.x;
    if (g >= n_heats) return;
    const int k1 = off[g + 1];
    for (int k = off[g] + threadIdx.x; k < k1; k += blockDim.x) {
        const int b = members[k];
        if ((unsigned)b < (unsigned)B) heat_of[b] = g;
    }
}

hipError_t launch_event_heat_of(int B, int n_heats, const int32_t *off, const int32_t *members, int32_t *heat_of, hipStream_t s) {
    hipError_t err = hipMemsetAsync(heat_of, 0xff, (size_t)B * 4, s);
    if (err != hipSuccess || n_heats <= 0) return err;
    hipLaunchKernelGGL(event_heat_of_kernel, dim3(n_heats), dim3(256), 0, s, B, n_heats, off, members, heat_of);
    return hipGetLastError();
}

hipError_t launch_event_tick(const EventDev &e, const EventSrc &s, int t, hipStream_t st) {
    if (e.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(event_tick_kernel, dim3(1), dim3(kEventBlock), 0, st, e, s, t);
    return hipGetLastError();
}

hipError_t launch_event_step(const EventDev &e, const EventSrc &s, int t, hipStream_t st) {
    if (e.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(event_step_kernel, dim3(1), dim3(kEventBlock), 0, st, e, s, t);
    return hipGetLastError();
}

}  // namespace lpvmpc
