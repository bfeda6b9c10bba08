// Exponential moving average of the weights (utils.optim.ModelEma), in the shape of the optimizer kernels of elementwise.hip.
// Per element, in fp32:
//   d   = src - ema
//   ema = fmaf(w, d, ema)                  torch.lerp(ema, src, w) for w < 0.5; one subtraction and one fused multiply-add, both written
//                                          out, so that the contraction setting of the build cannot change the rounding
// w = (float)(1.0 - decay) comes from the state: ema_advance_kernel (one thread) forms it in double, from the warm-up schedule when
// that is on, and counts the update -- or, when the optimizer's flag says that its step was skipped (half-precision build: a gradient
// with inf / NaN), clears `apply` and counts a held step.  The lerp launches behind it read apply and w, uniform over the grid, and
// return at once on a held step: the average moves exactly when the weights did, with no host synchronisation.
// The alignment padding of a flat array (src = ema = 0) stays exactly 0: fmaf(w, 0, 0) = 0.  src == ema gives ema.  No atomics: the
// same input gives the same bits.
#include "ema.h"
#include "launch_plan.h"

__global__ void ema_advance_kernel(PaEmaState* s, float decay, int warmup, const int* skip_flag) {
    if (skip_flag && skip_flag[0]) { s->apply = 0; s->held += 1; return; }
    double d = (double)decay;
    if (warmup) {
        const double u = (double)s->updates;
        const double ramp = (1.0 + u) / (10.0 + u);
        d = ramp < d ? ramp : d;
    }
    s->w = (float)(1.0 - d);
    s->decay_used = (float)d;
    s->apply = 1;
    s->updates += 1;
}

__global__ void ema_set_updates_kernel(PaEmaState* s, int updates) { s->updates = updates; }

template <bool COPY>
__device__ __forceinline__ float ema_update(float e, float p, float w) {
    if (COPY) return p;
    const float d = p - e;
    return fmaf(w, d, e);
}

template <bool COPY>
__global__ void ema_lerp_kernel(float* __restrict__ ema, const float* __restrict__ src, size_t n, const PaEmaState* s) {
    if (!s->apply) return;                  // uniform over the grid: every thread reads the same word (the prologue has counted the hold)
    const float w = s->w;
    size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
    for (; i + 3 < n; i += stride) {
        const f32x4 pp = *reinterpret_cast<const f32x4*>(src + i);
        f32x4 ee = pp;
        if (!COPY) ee = *reinterpret_cast<const f32x4*>(ema + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) ee[j] = ema_update<COPY>(ee[j], pp[j], w);
        *reinterpret_cast<f32x4*>(ema + i) = ee;
    }
    for (; i < n && i + 3 >= n; ++i) ema[i] = ema_update<COPY>(COPY ? 0.f : ema[i], src[i], w);          // tail (at most 3 elements, one thread)
}

int pa_launch_ema_advance(PaEmaState* s, float decay, int warmup, const int* skip_flag, hipStream_t st) {
    hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(1), 0, st, s, decay, warmup, skip_flag);
    return (int)hipGetLastError();
}

// the capped grid of pa_launch_rmsprop: one 16-byte chunk per thread and trip, grid-stride beyond 2048 workgroups
int pa_launch_ema_lerp(float* ema, const float* src, size_t n, const PaEmaState* s, bool copy, hipStream_t st) {
    if (n == 0) return 0;
    const int blocks = pa_grid_for(n / 4, 256, 2048);
    if (copy) hipLaunchKernelGGL(ema_lerp_kernel<true>, dim3(blocks), dim3(256), 0, st, ema, src, n, s);
    else hipLaunchKernelGGL(ema_lerp_kernel<false>, dim3(blocks), dim3(256), 0, st, ema, src, n, s);
    return (int)hipGetLastError();
}

int pa_ema_read_counts(const PaEmaState* s, long long* updates, long long* held, hipStream_t st) {
    PaEmaState h;
    hipError_t e = hipMemcpyAsync(&h, s, sizeof h, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    if (updates) *updates = h.updates;
    if (held) *held = h.held;
    return 0;
}

int pa_launch_ema_set_updates(PaEmaState* s, int updates, hipStream_t st) {
    hipLaunchKernelGGL(ema_set_updates_kernel, dim3(1), dim3(1), 0, st, s, updates);
    return (int)hipGetLastError();
}
