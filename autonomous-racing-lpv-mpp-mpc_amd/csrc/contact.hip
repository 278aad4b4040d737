// contact.hip -- the contact model (include/lpvmpc.h, "Contact model"): the interactions' tick with the corner form of the car-to-car
// contact, launched in place of interaction_tick_kernel while the model is attached.  One workgroup per heat with the heats' block size;
// the staging is the interactions' struct of arrays plus w and Iz (nine f64 arrays and one i32 array: 19 KB at 256 members), one
// barrier, one loop over the members with broadcast LDS reads.  The body is interaction_tick.hpp's, instantiated here in its corner
// form only: the contact point (at most three divisions) and the two impulses stand behind the overlap decision, so a wavefront none
// of whose lanes overlaps on a trip branches around them.  No atomics; reruns are bit-identical.
//
// Its own translation unit, compiled with -ffp-contract=off as interactions.o: every product and sum of the model is rounded on its own.
#include "interaction_tick.hpp"

namespace lpvmpc {

template <int BS> __global__ void __launch_bounds__(BS) contact_tick_kernel(ContactDev d, int t) {
    __shared__ ContactLds<BS> l;
    // the heat's slice of the member list; a heat larger than the block (the host refuses it) is cut to the block
    const int g = blockIdx.x, o = d.i.off[g];
    int n = d.i.off[g + 1] - o;
    if (n > BS) n = BS;
    const bool active = (int)threadIdx.x < n;
    const int b = active ? d.i.members[o + threadIdx.x] : 0;
    interaction_tick<BS, true>(d, l, t, n, threadIdx.x, active, b);
}

hipError_t launch_contact_tick(const ContactDev &d, int block, int t, hipStream_t s) {
    if (d.i.n_heats <= 0) return hipSuccess;
    const dim3 grid(d.i.n_heats);
    if (block <= 64) hipLaunchKernelGGL(contact_tick_kernel<64>, grid, dim3(64), 0, s, d, t);
    else hipLaunchKernelGGL(contact_tick_kernel<256>, grid, dim3(256), 0, s, d, t);
    return hipGetLastError();
}

}  // namespace lpvmpc
