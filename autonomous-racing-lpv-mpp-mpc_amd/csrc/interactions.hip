// interactions.hip -- the interactions (include/lpvmpc.h, "Interactions"): slipstream and contact response between the vehicles of a
// heat, on the plant side.  One kernel in front of the tick's command / plant kernel, which it leaves as it is (as disturbance.hip).
// One workgroup per heat, as heats.hip.  The tick's body is interaction_tick.hpp's, instantiated here in its through-the-centres form
// only (contact.hip instantiates the corner form: one form per object).  Phase 1: thread i takes member i and stages what the pairwise pass needs in LDS, a struct of
// arrays (seven f64 arrays and one i32 array: 15 KB at 256 members).  One barrier.  Phase 2: thread i runs ONE loop over the n members;
// every lane reads the same LDS address in a trip, so each read is a broadcast without bank conflicts.  The wake and overlap DECISIONS
// of a trip are plain mask arithmetic; the impulse sits behind its decision, so a wavefront none of whose lanes is in contact on that
// trip skips it (the compiler speculates the shelter's two divisions into the straight path).  The loop keeps the max and argmax of
// the shelter, the sums of du and dc in ascending member order and the hit flag.  Everything is computed from the staged (pre-tick)
// words, so the result does not depend on which pair is handled first (a Jacobi step); each thread writes only its own vehicle's
// plant row, live mu word, outputs and carry: no atomics, no traffic between workgroups.
//
// Its own translation unit, compiled with -ffp-contract=off as heats.o: every product and sum of the model is rounded on its own, and
// sep comes out the same word in both vehicles of a pair and the same word as the heats'.  Two block sizes, 64 and 256 threads, chosen
// by the heats' block.  The race and the batch call launch the same kernel on their own arrays (InterDev).
#include "interaction_tick.hpp"

namespace lpvmpc {

template <int BS> __global__ void __launch_bounds__(BS) interaction_tick_kernel(InterDev h, int t) {
    __shared__ InterLds<BS> l;
    // the heat's slice of the member list; a heat larger than the block (the host refuses it) is cut to the block
    const int g = blockIdx.x, o = h.off[g];
    int n = h.off[g + 1] - o;
    if (n > BS) n = BS;
    const bool active = (int)threadIdx.x < n;
    const int b = active ? h.members[o + threadIdx.x] : 0;
    interaction_tick<BS, false>(h, l, t, n, threadIdx.x, active, b);
}

hipError_t launch_interaction_tick(const InterDev &h, int block, int t, hipStream_t s) {
    if (h.n_heats <= 0) return hipSuccess;
    const dim3 grid(h.n_heats);
    if (block <= 64) hipLaunchKernelGGL(interaction_tick_kernel<64>, grid, dim3(64), 0, s, h, t);
    else hipLaunchKernelGGL(interaction_tick_kernel<256>, grid, dim3(256), 0, s, h, t);
    return hipGetLastError();
}

}  // namespace lpvmpc
