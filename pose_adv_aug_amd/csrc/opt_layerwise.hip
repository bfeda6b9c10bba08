// Layer-wise trust ratios on the flat arrays: LAMB (You et al. 2020) on Adam's moments, LARS (You, Gitman, Ginsburg 2017) and plain SGD
// with momentum / Nesterov, and per-tensor norms for logging (pa_lamb_step, pa_lars_step, pa_tensor_norms of include/poseadv.h).
//
// Unit of work.  The host cuts a flat array into SEGMENTS (pa_opt_segments_host): at every tensor start and then every
// PA_OPT_SEGMENT_FLOATS floats inside a tensor, so a segment lies inside ONE tensor, starts on a 16-byte boundary and covers no padding.
// One WAVE works on one segment, PA_LW_WAVES = 4 segments per 256-thread workgroup: a BatchNorm vector of 128 floats keeps half a wave
// busy instead of an eighth of a workgroup, and a per-segment sum is one wave reduction (no LDS, no barrier).  The segment index comes from
// blockIdx and the wave number through readfirstlane, so the 16-byte record, the group entry and the tensor's trust ratio are loaded once
// per wave with a uniform address and live in scalar registers.  The group table (at most 16 {lr, wd, c_dec, frozen}) travels by value and
// is staged in LDS by thread 0 with constant indices, as in elementwise.hip: indexing the argument itself would go through scratch.
//
// Sums.  No atomics.  A lane adds the squares of its elements in double in element order (chunks lane, lane + 64, ...; the at most 3 tail
// elements of a tensor's last segment go to lanes 0 .. 2 after their chunks), the 64 lane sums are added by an xor butterfly (32, 16, .. 1),
// and lane 0 writes ONE double per quantity and segment.  tensor_finish_kernel then adds a tensor's partials in segment order: the wave
// of the tensor's FIRST segment takes partials first + lane, first + lane + 64, ... and the same butterfly.  Both orders depend only on the
// tensor's own length, never on where the tensor lies: the same tensors in another layout give the same bits.
//
// Half-precision build: a reset + finite scan of the WHOLE gradient runs in front (the kernels of elementwise.hip repeated here under their
// own names: the library is built without relocatable device code, so a kernel cannot be launched from another translation unit); with
// the flag set every later kernel returns at once and the skip is counted once (LAMB: by the one-thread prologue; LARS: by the step kernel).
#include "common.h"
#include "kernels.h"
#include "launch_plan.h"

namespace {

__device__ __forceinline__ double wave_sum_double(double s) {       // every lane ends with the same sum
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

__device__ __forceinline__ float uniform_f(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

// this wave's segment (false: past the end); w = its index, uniform
__device__ __forceinline__ bool lw_segment(const PaOptSegment* __restrict__ segs, unsigned nsegs, unsigned& w, PaOptSegment& sg) {
    w = __builtin_amdgcn_readfirstlane(blockIdx.x * PA_LW_WAVES + (threadIdx.x >> 6));
    if (w >= nsegs) return false;
    const uint4 r = *reinterpret_cast<const uint4*>(segs + w);
    sg.chunk0 = __builtin_amdgcn_readfirstlane(r.x);
    sg.nfloats = __builtin_amdgcn_readfirstlane(r.y);
    sg.tensor = __builtin_amdgcn_readfirstlane((int)r.z);
    sg.group = __builtin_amdgcn_readfirstlane((int)r.w);
    return true;
}

__device__ __forceinline__ void lw_stage_groups(const PaOptGroupTable& tab, PaOptGroupK* lds) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < PA_OPT_GROUPS; ++k) lds[k] = tab.g[k];
    }
    __syncthreads();
}

__device__ __forceinline__ PaOptGroupK lw_group(const PaOptGroupK* lds, int group) {
    const PaOptGroupK e = lds[group & (PA_OPT_GROUPS - 1)];
    PaOptGroupK u;
    u.lr = uniform_f(e.lr); u.wd = uniform_f(e.wd); u.c_dec = uniform_f(e.c_dec); u.frozen = __builtin_amdgcn_readfirstlane(e.frozen);
    return u;
}

// ---- the finite scan of the half-precision build (grad_check_reset_kernel / grad_check_kernel of elementwise.hip)
__global__ void lw_grad_check_reset_kernel(int* state) { state[0] = 0; }

__global__ void lw_grad_check_kernel(const float* g, size_t n, int* state) {
    size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
    bool bad = false;
    for (; i + 3 < n; i += stride) {
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + i);
        bad |= !(isfinite(gg[0]) && isfinite(gg[1]) && isfinite(gg[2]) && isfinite(gg[3]));
    }
    for (; i < n && i + 3 >= n; ++i) bad |= !isfinite(g[i]);
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&state[0], 1);          // (an integer OR of the same bit: order-free)
}

// ---- per-tensor norms of scale * x
__global__ __launch_bounds__(256) void tensor_sqsum_kernel(const float* __restrict__ x, const PaOptSegment* __restrict__ segs, unsigned nsegs,
                                                           float scale, double* __restrict__ partial) {
    unsigned w; PaOptSegment sg;
    if (!lw_segment(segs, nsegs, w, sg)) return;
    const float* xs = x + (size_t)sg.chunk0 * 4;
    const unsigned lane = threadIdx.x & 63, nfull = sg.nfloats & ~3u;
    const double sc = (double)scale;
    double s = 0.0;
    for (unsigned i = lane * 4; i < nfull; i += 256) {
        const f32x4 xx = *reinterpret_cast<const f32x4*>(xs + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) { const double t = (double)xx[j] * sc; s += t * t; }
    }
    if (nfull + lane < sg.nfloats) { const double t = (double)xs[nfull + lane] * sc; s += t * t; }
    s = wave_sum_double(s);
    if (lane == 0) { partial[2 * (size_t)w] = s; partial[2 * (size_t)w + 1] = 0.0; }
}

// MODE 0: norms[t] = (float)sqrt(a).  MODE 1 (LAMB) and 2 (LARS): norms[t] = W, norms[ntensors + t] = U or G, trust[t] = r_t; a frozen
// tensor writes nothing.  a, b: the sums of the tensor's partials in segment order.
struct LwFinish { int always_adapt; float max_trust, trust_coef, lars_eps; };

template <int MODE>
__global__ __launch_bounds__(256) void tensor_finish_kernel(const PaOptSegment* __restrict__ segs, unsigned nsegs, const double* __restrict__ partial,
                                                            PaOptGroupTable tab, LwFinish f, int ntensors, float* __restrict__ norms,
                                                            float* __restrict__ trust, const int* flag) {
    __shared__ PaOptGroupK s_tab[PA_OPT_GROUPS];
    if (MODE != 0) lw_stage_groups(tab, s_tab);
    if (flag && flag[0]) return;            // uniform over the grid
    unsigned w; PaOptSegment sg;
    if (!lw_segment(segs, nsegs, w, sg)) return;
    if (w > 0 && __builtin_amdgcn_readfirstlane(segs[w - 1].tensor) == sg.tensor) return;       // not the tensor's first segment
    float wd = 0.f;
    if (MODE != 0) {
        const PaOptGroupK gk = lw_group(s_tab, sg.group);
        if (gk.frozen) return;
        wd = gk.wd;
    }
    const unsigned lane = threadIdx.x & 63;
    double a = 0.0, b = 0.0;
    for (unsigned j0 = w; ; j0 += 64) {
        const unsigned j = j0 + lane;
        const bool in = j < nsegs && segs[j].tensor == sg.tensor;
        if (in) { a += partial[2 * (size_t)j]; if (MODE != 0) b += partial[2 * (size_t)j + 1]; }
        if (__ballot(in) != ~0ull || j0 + 64 < j0) break;
    }
    a = wave_sum_double(a);
    if (MODE != 0) b = wave_sum_double(b);
    if (lane != 0) return;
    const int t = sg.tensor;
    const double W = sqrt(a), B = sqrt(b);
    norms[t] = (float)W;
    if (MODE == 0) return;
    norms[(size_t)ntensors + t] = (float)B;
    const bool adapt = (f.always_adapt || wd != 0.f) && a > 0.0 && b > 0.0;
    double r = 1.0;
    if (MODE == 1) {
        if (adapt) r = W / B;
        if (f.max_trust > 0.f) r = fmin(r, (double)f.max_trust);
    } else {
        if (f.trust_coef > 0.f && adapt) r = (double)f.trust_coef * W / (B + (double)wd * W + (double)f.lars_eps);
    }
    trust[t] = (float)r;
}

// ---- LAMB
// adam_prologue_kernel of elementwise.hip: advances the step count and writes the constants, or counts a skipped step
__global__ void lamb_prologue_kernel(PaAdamState* s, float lr, float beta1, float beta2) {
    if (s->flag) { s->skipped += 1; return; }
    const int t = s->step + 1;
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)t));
    const float bc2 = (float)(1.0 - pow((double)beta2, (double)t));
    s->step = t;
    s->bc1 = bc1;
    s->bc2 = bc2;
    s->step_size = lr / bc1;
    s->bc2s = sqrtf(bc2);
}

// u from the moments AFTER the update and the parameter BEFORE the step: evaluated by pass 1 (for its norm) and again by pass 2
__device__ __forceinline__ float lamb_u(float p, float m1, float v1, float bc1, float bc2s, float eps, float wd) {
    const float den = sqrtf(v1) / bc2s + eps;
    float u = (m1 / bc1) / den;
    if (wd != 0.f) u = u + wd * p;
    return u;
}

__device__ __forceinline__ float lamb_moments(float p, float g, float& m, float& v, const PaLambOpts& o, float gscale, bool clip, float coef,
                                              float bc1, float bc2s, float wd) {
    float gr = g * gscale;
    if (clip) gr = gr * coef;
    m = m + (gr - m) * o.om_b1;
    v = o.beta2 * v + (o.om_b2 * gr) * gr;
    return lamb_u(p, m, v, bc1, bc2s, o.eps, wd);
}

// pass 1: m', v' and the per-segment sums of p^2 and u^2
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, const PaOptSegment* __restrict__ segs, unsigned nsegs,
                                                           PaOptGroupTable tab, PaLambOpts o, float gscale, const float* clip_coef,
                                                           const PaAdamState* state, double* __restrict__ partial) {
    __shared__ PaOptGroupK s_tab[PA_OPT_GROUPS];
    lw_stage_groups(tab, s_tab);
    if (state->flag) return;                // uniform over the grid (the prologue has counted the skip)
    unsigned w; PaOptSegment sg;
    if (!lw_segment(segs, nsegs, w, sg)) return;
    const PaOptGroupK gk = lw_group(s_tab, sg.group);
    if (gk.frozen) return;                  // before any load
    const float bc1 = state->bc1, bc2s = state->bc2s;
    const bool clip = clip_coef != nullptr;
    const float coef = clip ? clip_coef[0] : 1.f;
    const size_t base = (size_t)sg.chunk0 * 4;
    const unsigned lane = threadIdx.x & 63, nfull = sg.nfloats & ~3u;
    double sw = 0.0, su = 0.0;
    for (unsigned i = lane * 4; i < nfull; i += 256) {
        const f32x4 pp = *reinterpret_cast<const f32x4*>(p + base + i), gg = *reinterpret_cast<const f32x4*>(g + base + i);
        f32x4 mm = *reinterpret_cast<f32x4*>(m + base + i), vv = *reinterpret_cast<f32x4*>(v + base + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float mj = mm[j], vj = vv[j];
            const float u = lamb_moments(pp[j], gg[j], mj, vj, o, gscale, clip, coef, bc1, bc2s, gk.wd);
            mm[j] = mj; vv[j] = vj;
            sw += (double)pp[j] * (double)pp[j];
            su += (double)u * (double)u;
        }
        *reinterpret_cast<f32x4*>(m + base + i) = mm;
        *reinterpret_cast<f32x4*>(v + base + i) = vv;
    }
    if (nfull + lane < sg.nfloats) {
        const size_t i = base + nfull + lane;
        const float pj = p[i];
        float mj = m[i], vj = v[i];
        const float u = lamb_moments(pj, g[i], mj, vj, o, gscale, clip, coef, bc1, bc2s, gk.wd);
        m[i] = mj; v[i] = vj;
        sw += (double)pj * (double)pj;
        su += (double)u * (double)u;
    }
    sw = wave_sum_double(sw);
    su = wave_sum_double(su);
    if (lane == 0) { partial[2 * (size_t)w] = sw; partial[2 * (size_t)w + 1] = su; }
}

// pass 2: p' = p - (lr_group * r_t) * u, u recomputed from m', v' and p
__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                         const PaOptSegment* __restrict__ segs, unsigned nsegs, PaOptGroupTable tab, float eps,
                                                         const float* __restrict__ trust, const PaAdamState* state) {
    __shared__ PaOptGroupK s_tab[PA_OPT_GROUPS];
    lw_stage_groups(tab, s_tab);
    if (state->flag) return;
    unsigned w; PaOptSegment sg;
    if (!lw_segment(segs, nsegs, w, sg)) return;
    const PaOptGroupK gk = lw_group(s_tab, sg.group);
    if (gk.frozen) return;
    const float bc1 = state->bc1, bc2s = state->bc2s;
    const float step = gk.lr * uniform_f(trust[sg.tensor]);
    const size_t base = (size_t)sg.chunk0 * 4;
    const unsigned lane = threadIdx.x & 63, nfull = sg.nfloats & ~3u;
    for (unsigned i = lane * 4; i < nfull; i += 256) {
        f32x4 pp = *reinterpret_cast<f32x4*>(p + base + i);
        const f32x4 mm = *reinterpret_cast<const f32x4*>(m + base + i), vv = *reinterpret_cast<const f32x4*>(v + base + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) pp[j] = pp[j] - step * lamb_u(pp[j], mm[j], vv[j], bc1, bc2s, eps, gk.wd);
        *reinterpret_cast<f32x4*>(p + base + i) = pp;
    }
    if (nfull + lane < sg.nfloats) {
        const size_t i = base + nfull + lane;
        p[i] = p[i] - step * lamb_u(p[i], m[i], v[i], bc1, bc2s, eps, gk.wd);
    }
}

// ---- LARS / SGD
// per-segment sums of p^2 and gr^2, gr = g gscale coef formed in double (the product of fp32 values as pa_grad_norm forms it)
__global__ __launch_bounds__(256) void lars_sqsum_kernel(const float* __restrict__ p, const float* __restrict__ g, const PaOptSegment* __restrict__ segs,
                                                         unsigned nsegs, PaOptGroupTable tab, float gscale, const float* clip_coef, const int* flag,
                                                         double* __restrict__ partial) {
    __shared__ PaOptGroupK s_tab[PA_OPT_GROUPS];
    lw_stage_groups(tab, s_tab);
#ifdef PA_FP16
    if (flag[0]) return;                    // uniform over the grid
#else
    (void)flag;
#endif
    unsigned w; PaOptSegment sg;
    if (!lw_segment(segs, nsegs, w, sg)) return;
    if (lw_group(s_tab, sg.group).frozen) return;
    const double sc = clip_coef ? (double)gscale * (double)clip_coef[0] : (double)gscale;
    const size_t base = (size_t)sg.chunk0 * 4;
    const unsigned lane = threadIdx.x & 63, nfull = sg.nfloats & ~3u;
    double sw = 0.0, sg2 = 0.0;
    for (unsigned i = lane * 4; i < nfull; i += 256) {
        const f32x4 pp = *reinterpret_cast<const f32x4*>(p + base + i), gg = *reinterpret_cast<const f32x4*>(g + base + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double t = (double)gg[j] * sc;
            sw += (double)pp[j] * (double)pp[j];
            sg2 += t * t;
        }
    }
    if (nfull + lane < sg.nfloats) {
        const size_t i = base + nfull + lane;
        const double t = (double)g[i] * sc;
        sw += (double)p[i] * (double)p[i];
        sg2 += t * t;
    }
    sw = wave_sum_double(sw);
    sg2 = wave_sum_double(sg2);
    if (lane == 0) { partial[2 * (size_t)w] = sw; partial[2 * (size_t)w + 1] = sg2; }
}

template <bool MOMENTUM, bool NESTEROV, bool TRUST>
__device__ __forceinline__ void lars_update(float& p, float g, float& buf, float gscale, bool clip, float coef, float lr, float wd, float mom, float r) {
    float gr = g * gscale;
    if (clip) gr = gr * coef;
    float d = gr;
    if (wd != 0.f) d = gr + wd * p;
    if (TRUST) d = r * d;
    if (MOMENTUM) {
        buf = mom * buf + d;
        d = NESTEROV ? d + mom * buf : buf;
    }
    p = p - lr * d;
}

template <bool MOMENTUM, bool NESTEROV, bool TRUST>
__global__ __launch_bounds__(256) void lars_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                        const PaOptSegment* __restrict__ segs, unsigned nsegs, PaOptGroupTable tab, float mom,
                                                        float gscale, const float* clip_coef, const float* __restrict__ trust, int* state) {
    __shared__ PaOptGroupK s_tab[PA_OPT_GROUPS];
#ifdef PA_FP16
    if (state[0]) {                         // uniform over the grid: every thread reads the same word
        if (blockIdx.x == 0 && threadIdx.x == 0) state[1] += 1;
        return;
    }
#endif
    lw_stage_groups(tab, s_tab);
    unsigned w; PaOptSegment sg;
    if (!lw_segment(segs, nsegs, w, sg)) return;
    const PaOptGroupK gk = lw_group(s_tab, sg.group);
    if (gk.frozen) return;
    const bool clip = clip_coef != nullptr;
    const float coef = clip ? clip_coef[0] : 1.f;
    const float r = TRUST ? uniform_f(trust[sg.tensor]) : 1.f;
    const size_t base = (size_t)sg.chunk0 * 4;
    const unsigned lane = threadIdx.x & 63, nfull = sg.nfloats & ~3u;
    for (unsigned i = lane * 4; i < nfull; i += 256) {
        f32x4 pp = *reinterpret_cast<f32x4*>(p + base + i);
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + base + i);
        f32x4 bb = {0.f, 0.f, 0.f, 0.f};
        if (MOMENTUM) bb = *reinterpret_cast<f32x4*>(buf + base + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = pp[j], bj = bb[j];
            lars_update<MOMENTUM, NESTEROV, TRUST>(pj, gg[j], bj, gscale, clip, coef, gk.lr, gk.wd, mom, r);
            pp[j] = pj; bb[j] = bj;
        }
        *reinterpret_cast<f32x4*>(p + base + i) = pp;
        if (MOMENTUM) *reinterpret_cast<f32x4*>(buf + base + i) = bb;
    }
    if (nfull + lane < sg.nfloats) {
        const size_t i = base + nfull + lane;
        float pj = p[i], bj = MOMENTUM ? buf[i] : 0.f;
        lars_update<MOMENTUM, NESTEROV, TRUST>(pj, g[i], bj, gscale, clip, coef, gk.lr, gk.wd, mom, r);
        p[i] = pj;
        if (MOMENTUM) buf[i] = bj;
    }
}

template <bool TRUST>
void lars_launch(bool mom, bool nesterov, dim3 grid, hipStream_t st, float* p, const float* g, float* buf, const PaOptSegment* segs, unsigned nsegs,
                 const PaOptGroupTable& tab, float momentum, float gscale, const float* clip_coef, const float* trust, int* state) {
    const dim3 block(256);
    if (mom && nesterov) hipLaunchKernelGGL((lars_step_kernel<true, true, TRUST>), grid, block, 0, st, p, g, buf, segs, nsegs, tab, momentum, gscale, clip_coef, trust, state);
    else if (mom) hipLaunchKernelGGL((lars_step_kernel<true, false, TRUST>), grid, block, 0, st, p, g, buf, segs, nsegs, tab, momentum, gscale, clip_coef, trust, state);
    else hipLaunchKernelGGL((lars_step_kernel<false, false, TRUST>), grid, block, 0, st, p, g, buf, segs, nsegs, tab, momentum, gscale, clip_coef, trust, state);
}

dim3 lw_grid(size_t nsegs) { return dim3((unsigned)((nsegs + PA_LW_WAVES - 1) / PA_LW_WAVES)); }

void lw_scan(const float* g, size_t n, int* flag, hipStream_t st) {
#ifdef PA_FP16
    hipLaunchKernelGGL(lw_grad_check_reset_kernel, dim3(1), dim3(1), 0, st, flag);
    hipLaunchKernelGGL(lw_grad_check_kernel, dim3(pa_grid_for(n / 4, 256, 2048)), dim3(256), 0, st, g, n, flag);
#else
    (void)g; (void)n; (void)flag; (void)st;
#endif
}

}  // namespace

size_t pa_opt_layer_workspace_size(size_t nsegs, int ntensors) {
    (void)ntensors;                         // (the finish launch finds a tensor's segments in the list itself: no table per tensor)
    return (nsegs ? nsegs : 1) * 2 * sizeof(double);
}

int pa_launch_tensor_norms(const float* x, const PaOptSegment* segs, size_t nsegs, int ntensors, float scale, void* workspace, float* norms,
                           hipStream_t st) {
    if (nsegs == 0) return 0;
    double* partial = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(tensor_sqsum_kernel, lw_grid(nsegs), dim3(256), 0, st, x, segs, (unsigned)nsegs, scale, partial);
    hipLaunchKernelGGL((tensor_finish_kernel<0>), lw_grid(nsegs), dim3(256), 0, st, segs, (unsigned)nsegs, partial, PaOptGroupTable(), LwFinish(),
                       ntensors, norms, (float*)nullptr, (const int*)nullptr);
    return (int)hipGetLastError();
}

// [scan] -> prologue -> pass 1 -> finish -> pass 2
int pa_launch_lamb(const PaLambOpts& o, const PaOptGroupTable& tab, const PaOptSegment* segs, size_t nsegs, int ntensors, float* p,
                   const float* g, float* m, float* v, size_t n, float gscale, const float* clip_coef, void* workspace, float* norms,
                   float* trust, PaAdamState* state, hipStream_t st) {
    if (n == 0) return 0;
    double* partial = reinterpret_cast<double*>(workspace);
    const dim3 grid = lw_grid(nsegs), block(256);
    lw_scan(g, n, &state->flag, st);
    hipLaunchKernelGGL(lamb_prologue_kernel, dim3(1), dim3(1), 0, st, state, tab.g[0].lr, o.beta1, o.beta2);
    hipLaunchKernelGGL(lamb_moments_kernel, grid, block, 0, st, p, g, m, v, segs, (unsigned)nsegs, tab, o, gscale, clip_coef, state, partial);
    const LwFinish f = {o.always_adapt, o.max_trust, 0.f, 0.f};
    hipLaunchKernelGGL((tensor_finish_kernel<1>), grid, block, 0, st, segs, (unsigned)nsegs, partial, tab, f, ntensors, norms, trust, &state->flag);
    hipLaunchKernelGGL(lamb_apply_kernel, grid, block, 0, st, p, m, v, segs, (unsigned)nsegs, tab, o.eps, trust, state);
    return (int)hipGetLastError();
}

// trust_coef > 0: [scan] -> sums -> finish -> step.  trust_coef == 0 (plain SGD): [scan] -> step, nothing else.
int pa_launch_lars(const PaLarsOpts& o, const PaOptGroupTable& tab, const PaOptSegment* segs, size_t nsegs, int ntensors, float* p,
                   const float* g, float* buf, size_t n, float gscale, const float* clip_coef, void* workspace, float* norms, float* trust,
                   int* state, hipStream_t st) {
    if (n == 0) return 0;
    const dim3 grid = lw_grid(nsegs), block(256);
    const bool mom = o.mom != 0.f;
    lw_scan(g, n, state, st);
    if (o.trust_coef > 0.f) {
        double* partial = reinterpret_cast<double*>(workspace);
        hipLaunchKernelGGL(lars_sqsum_kernel, grid, block, 0, st, p, g, segs, (unsigned)nsegs, tab, gscale, clip_coef, state, partial);
        const LwFinish f = {o.always_adapt, 0.f, o.trust_coef, o.lars_eps};
#ifdef PA_FP16
        const int* flag = state;
#else
        const int* flag = nullptr;          // the bf16 build never reads the pair
#endif
        hipLaunchKernelGGL((tensor_finish_kernel<2>), grid, block, 0, st, segs, (unsigned)nsegs, partial, tab, f, ntensors, norms, trust, flag);
        lars_launch<true>(mom, o.nesterov != 0, grid, st, p, g, buf, segs, (unsigned)nsegs, tab, o.mom, gscale, clip_coef, trust, state);
    } else {
        lars_launch<false>(mom, o.nesterov != 0, grid, st, p, g, buf, segs, (unsigned)nsegs, tab, o.mom, gscale, clip_coef, nullptr, state);
    }
    return (int)hipGetLastError();
}
