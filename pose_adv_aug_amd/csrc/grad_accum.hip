// Gradient accumulation over micro-batches (utils.optim._FlatOptimizer.accumulate / step), in the shape of the optimizer kernels of
// elementwise.hip and of ema.hip.  Per element, in fp32:
//   dst = a + b                            one addition: no scaling (the mean over the micro-batches is taken by the step kernel's gscale),
//                                          no atomics, so the same input gives the same bits; the sum of a group is ((g1 + g2) + g3) + ...
//   dst = a                                COPY (b == NULL): the first micro-batch of a group
// dst may be exactly a or exactly b: a thread reads the elements it is about to write, and no other thread touches them, so the pointers
// carry no __restrict__.  inf, NaN and denormals are ordinary operands (no flush-to-zero flag in the build): inf + -inf = NaN reaches the
// half-precision build's finite check of the step behind the last fold.
// VEC: all three pointers 16-byte aligned (the flat arrays are).  A view into a flat array need not be: then one element per thread and
// trip, on the same capped grid.
#include "grad_accum.h"
#include "launch_plan.h"

template <bool COPY, bool VEC>
__global__ void grad_accum_kernel(float* dst, const float* a, const float* b, size_t n) {
    if (VEC) {
        size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
        const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
        for (; i + 3 < n; i += stride) {
            f32x4 v = *reinterpret_cast<const f32x4*>(a + i);
            if (!COPY) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(b + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = v[j] + w[j];
            }
            *reinterpret_cast<f32x4*>(dst + i) = v;
        }
        for (; i < n && i + 3 >= n; ++i) dst[i] = COPY ? a[i] : a[i] + b[i];          // tail (at most 3 elements, one thread)
    } else {
        size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
        const size_t stride = (size_t)gridDim.x * blockDim.x;
        for (; i < n; i += stride) dst[i] = COPY ? a[i] : a[i] + b[i];
    }
}

// the capped grid of pa_launch_rmsprop: one 16-byte chunk per thread and trip, grid-stride beyond 2048 workgroups
int pa_launch_grad_accumulate(float* dst, const float* a, const float* b, size_t n, hipStream_t st) {
    if (n == 0) return 0;
    const bool vec = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
    const int blocks = vec ? pa_grid_for(n / 4, 256, 2048) : pa_grid_for(n, 256, 2048);
    if (b) {
        if (vec) hipLaunchKernelGGL((grad_accum_kernel<false, true>), dim3(blocks), dim3(256), 0, st, dst, a, b, n);
        else hipLaunchKernelGGL((grad_accum_kernel<false, false>), dim3(blocks), dim3(256), 0, st, dst, a, b, n);
    } else {
        if (vec) hipLaunchKernelGGL((grad_accum_kernel<true, true>), dim3(blocks), dim3(256), 0, st, dst, a, b, n);
        else hipLaunchKernelGGL((grad_accum_kernel<true, false>), dim3(blocks), dim3(256), 0, st, dst, a, b, n);
    }
    return (int)hipGetLastError();
}
