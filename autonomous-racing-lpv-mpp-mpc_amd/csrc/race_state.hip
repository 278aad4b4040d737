// race_state.hip -- the device path of lpvmpc_race_clone: vehicle dstv[m] takes every state word of vehicle srcv[m], over the
// race's whole inventory (race_state.hpp), staged through a buffer so that a source that is also a destination (swaps, cycles,
// duplicates) is read before anything is written:
//   race_gather_kernel    arrays -> stage, the words of the source vehicles
//   race_scatter_kernel   stage -> arrays, into the destination vehicles
// launched in this order on one stream.  blockIdx.y is the descriptor; a grid-stride loop runs over the moved * W words of the
// array.  The stage keeps the array's own layout, so both sides of a copy coalesce:
//   vehicle-major [B][W]   consecutive lanes take consecutive words of one vehicle        (stage [moved][W])
//   word-major    [W][B]   consecutive lanes take consecutive moved vehicles of one word  (stage [W][moved])
// i32 and f64 words are copied at their own widths (the arrays are only as aligned as their elements).  No LDS; gated: no scratch.
//
// Its own translation unit, compiled as race.o, so that no kernel of another object changes.
#include "race_state.hpp"

namespace lpvmpc {

// the element of vehicle v, word w (stride: B for the array, moved for the stage) of an array in `layout`
__device__ inline size_t state_at(int layout, size_t v, size_t w, size_t W, size_t stride) {
    return layout == STATE_WORD_MAJOR ? w * stride + v : v * W + w;
}

// kGather: stage[m][w] = a[idx[m]][w]; else a[idx[m]][w] = stage[m][w]
template <class T, bool kGather>
__device__ inline void state_copy(T *__restrict__ a, T *__restrict__ stage, int layout, int W, int B, int moved, const int32_t *__restrict__ idx) {
    const size_t total = (size_t)moved * (size_t)W, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        size_t m, w;
        if (layout == STATE_WORD_MAJOR) { w = i / (size_t)moved; m = i - w * (size_t)moved; }
        else { m = i / (size_t)W; w = i - m * (size_t)W; }
        const size_t k = state_at(layout, (size_t)idx[m], w, W, B);
        if constexpr (kGather) stage[i] = a[k];
        else a[k] = stage[i];
    }
}

template <bool kGather>
__device__ inline void state_kernel_body(const StateDescDev *__restrict__ desc, int B, int moved, const int32_t *__restrict__ idx, char *stage) {
    const StateDescDev d = desc[blockIdx.y];
    if (d.type == STATE_I32) state_copy<int32_t, kGather>((int32_t *)d.ptr, (int32_t *)(stage + d.stage), d.layout, d.W, B, moved, idx);
    else state_copy<double, kGather>((double *)d.ptr, (double *)(stage + d.stage), d.layout, d.W, B, moved, idx);
}

__global__ void __launch_bounds__(256) race_gather_kernel(const StateDescDev *__restrict__ desc, int B, int moved, const int32_t *__restrict__ srcv,
                                                          char *__restrict__ stage) {
    state_kernel_body<true>(desc, B, moved, srcv, stage);
}

__global__ void __launch_bounds__(256) race_scatter_kernel(const StateDescDev *__restrict__ desc, int B, int moved, const int32_t *__restrict__ dstv,
                                                           char *__restrict__ stage) {
    state_kernel_body<false>(desc, B, moved, dstv, stage);
}

// max_words: the largest moved * W of the table; at most 1024 blocks per descriptor, the loop takes the rest
static dim3 state_grid(size_t max_words, int n_desc) {
    size_t gx = (max_words + 255) / 256;
    if (gx < 1) gx = 1;
    if (gx > 1024) gx = 1024;
    return dim3((unsigned)gx, (unsigned)n_desc);
}

hipError_t launch_race_gather(const StateDescDev *desc, int n_desc, int B, int moved, const int32_t *srcv, char *stage, size_t max_words,
                              hipStream_t s) {
    hipLaunchKernelGGL(race_gather_kernel, state_grid(max_words, n_desc), dim3(256), 0, s, desc, B, moved, srcv, stage);
    return hipGetLastError();
}
hipError_t launch_race_scatter(const StateDescDev *desc, int n_desc, int B, int moved, const int32_t *dstv, const char *stage, size_t max_words,
                               hipStream_t s) {
    hipLaunchKernelGGL(race_scatter_kernel, state_grid(max_words, n_desc), dim3(256), 0, s, desc, B, moved, dstv, const_cast<char *>(stage));
    return hipGetLastError();
}

}  // namespace lpvmpc
