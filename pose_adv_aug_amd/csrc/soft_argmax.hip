// Soft-arg-max over heat maps (integral regression) and its backward pass.  Per map (b, j), with m its maximum, p the pixel index,
// x_p = p % W + 1, y_p = p / W + 1 (1-based, the row is p / W):
//   e_p = exp(beta (h_p - m)),  Z = sum e_p,  ex = sum x_p e_p / Z,  ey = sum y_p e_p / Z
//   dmaps_p = beta e_p / Z ((x_p - ex) gx + (y_p - ey) gy)
// All arithmetic in double (the maximum is found on the fp32 values, which is exact); coords = (float)ex, (float)ey, state = m, Z, ex, ey
// unrounded, dmaps rounded once.  No atomics and a fixed order of additions: the same input gives the same bits.
//
// Forward, two passes over the map (the maximum, then the three sums; the second pass reads from L2).  A thread adds its own terms in
// increasing p, the 64 lanes of a wave are added by an xor butterfly (every lane forms the same sums), the waves through LDS in wave order.
// Every term is >= 0, so each sum carries a relative error of (number of additions on the longest path) 2^-53: the bound of
// tests/soft_argmax_exact.py counts them from the constants of soft_argmax.h.
#include "soft_argmax.h"

__device__ __forceinline__ double sam_exp(double a) { return exp(a); }

__device__ __forceinline__ double sam_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float sam_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Joint-minor maps [B][H*W][16], 16-byte aligned.  One workgroup = one sample and four joints: a thread reads the 16 bytes of its four
// joints of a pixel (the four workgroups of a sample share every 64-byte line in L2) and keeps m, Z, Sx, Sy of four joints: 16 doubles.
// All 16 joints in one thread would be 64 doubles = 128 registers of running state alone, the whole budget of a 1024-thread workgroup.
__global__ __launch_bounds__(PA_SAM_THREADS) void soft_argmax_nhwc16_kernel(const float* maps, int H, int W, double beta, float* coords,
                                                                            double* state) {
    constexpr int NW = PA_SAM_THREADS / 64;
    __shared__ float smax[NW][4];
    __shared__ double ssum[NW][4][3];
    const int b = blockIdx.x >> 2, g = blockIdx.x & 3, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = H * W;
    const f32x4* base = reinterpret_cast<const f32x4*>(maps + (size_t)b * HW * 16) + g;          // pixel p: base[4 p]
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int p0 = tid; p0 < HW; p0 += PA_SAM_INFLIGHT * PA_SAM_THREADS) {
        f32x4 v[PA_SAM_INFLIGHT];
#pragma unroll
        for (int u = 0; u < PA_SAM_INFLIGHT; ++u) {
            const int p = p0 + u * PA_SAM_THREADS;
            v[u] = base[(size_t)(p < HW ? p : p0) * 4];              // clamped, unconditional loads (a repeated pixel does not move a maximum)
        }
#pragma unroll
        for (int u = 0; u < PA_SAM_INFLIGHT; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], v[u][r]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        mx[r] = sam_wave_max(mx[r]);
        if (lane == 0) smax[wave][r] = mx[r];
    }
    __syncthreads();
    double m[4], Z[4], Sx[4], Sy[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float t = smax[0][r];
#pragma unroll
        for (int w = 1; w < NW; ++w) t = fmaxf(t, smax[w][r]);
        m[r] = (double)t; Z[r] = 0.0; Sx[r] = 0.0; Sy[r] = 0.0;
    }
    for (int p0 = tid; p0 < HW; p0 += PA_SAM_INFLIGHT * PA_SAM_THREADS) {
        f32x4 v[PA_SAM_INFLIGHT];
#pragma unroll
        for (int u = 0; u < PA_SAM_INFLIGHT; ++u) {
            const int p = p0 + u * PA_SAM_THREADS;
            v[u] = base[(size_t)(p < HW ? p : p0) * 4];
        }
#pragma unroll
        for (int u = 0; u < PA_SAM_INFLIGHT; ++u) {
            const int p = p0 + u * PA_SAM_THREADS;
            if (p < HW) {
                const int y = p / W, x = p - y * W;
                const double xd = (double)(x + 1), yd = (double)(y + 1);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double e = sam_exp(beta * ((double)v[u][r] - m[r]));
                    Z[r] += e; Sx[r] += xd * e; Sy[r] += yd * e;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double z = sam_wave_sum(Z[r]), sx = sam_wave_sum(Sx[r]), sy = sam_wave_sum(Sy[r]);
        if (lane == 0) { ssum[wave][r][0] = z; ssum[wave][r][1] = sx; ssum[wave][r][2] = sy; }
    }
    __syncthreads();
    if (tid < 4) {
        float t = smax[0][tid];                                      // joint `tid` of the group (m[] is indexed by compile-time r only)
        double z = ssum[0][tid][0], sx = ssum[0][tid][1], sy = ssum[0][tid][2];
#pragma unroll
        for (int w = 1; w < NW; ++w) { t = fmaxf(t, smax[w][tid]); z += ssum[w][tid][0]; sx += ssum[w][tid][1]; sy += ssum[w][tid][2]; }
        const double ex = sx / z, ey = sy / z;
        const size_t map = (size_t)b * 16 + g * 4 + tid;
        coords[map * 2] = (float)ex; coords[map * 2 + 1] = (float)ey;
        state[map * 4] = (double)t; state[map * 4 + 1] = z; state[map * 4 + 2] = ex; state[map * 4 + 3] = ey;
    }
}

// Any J, either layout, any alignment: one workgroup per (sample, joint) map, element (b, j, p) at b sb + j sj + p sp (argmax_kernel's
// addressing).  The same two passes and the same order of additions with 256 threads.
__global__ __launch_bounds__(PA_SAM_GENERIC_THREADS) void soft_argmax_kernel(const float* maps, long sb, long sj, long sp, int J, int H, int W,
                                                                             double beta, float* coords, double* state) {
    constexpr int NW = PA_SAM_GENERIC_THREADS / 64;
    __shared__ float smax[NW];
    __shared__ double ssum[NW][3];
    const int map = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = map / J, j = map - b * J;
    const float* base = maps + b * sb + j * sj;
    const int HW = H * W;
    float mx = -INFINITY;
    for (int p = tid; p < HW; p += PA_SAM_GENERIC_THREADS) mx = fmaxf(mx, base[(long)p * sp]);
    mx = sam_wave_max(mx);
    if (lane == 0) smax[wave] = mx;
    __syncthreads();
    mx = smax[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) mx = fmaxf(mx, smax[w]);
    const double m = (double)mx;
    double Z = 0.0, Sx = 0.0, Sy = 0.0;
    for (int p = tid; p < HW; p += PA_SAM_GENERIC_THREADS) {
        const int y = p / W, x = p - y * W;
        const double e = sam_exp(beta * ((double)base[(long)p * sp] - m));
        Z += e; Sx += (double)(x + 1) * e; Sy += (double)(y + 1) * e;
    }
    Z = sam_wave_sum(Z); Sx = sam_wave_sum(Sx); Sy = sam_wave_sum(Sy);
    if (lane == 0) { ssum[wave][0] = Z; ssum[wave][1] = Sx; ssum[wave][2] = Sy; }
    __syncthreads();
    if (tid == 0) {
        double z = ssum[0][0], sx = ssum[0][1], sy = ssum[0][2];
#pragma unroll
        for (int w = 1; w < NW; ++w) { z += ssum[w][0]; sx += ssum[w][1]; sy += ssum[w][2]; }
        const double ex = sx / z, ey = sy / z;
        coords[(size_t)map * 2] = (float)ex; coords[(size_t)map * 2 + 1] = (float)ey;
        state[(size_t)map * 4] = m; state[(size_t)map * 4 + 1] = z; state[(size_t)map * 4 + 2] = ex; state[(size_t)map * 4 + 3] = ey;
    }
}

// Backward: one pass, every element of maps read once and every element of dmaps written once by the thread that read it.
//   c = beta / Z (once per thread and joint);  dmaps_p = (float)((c e_p) ((x_p - ex) gx + (y_p - ey) gy))
// Joint-minor: a thread owns one 16-byte chunk position (four joints, the same four on every trip: the stride is a multiple of 4 chunks)
// of the pixels of ONE sample (blockIdx.y), so m, c, ex, ey, gx, gy of its four joints stay in registers.
__global__ __launch_bounds__(PA_SAM_BWD_THREADS) void soft_argmax_bwd_nhwc16_kernel(const float* maps, int H, int W, double beta, const double* state,
                                                                                    const float* dcoords, float* dmaps) {
    const int b = blockIdx.y, q = threadIdx.x & 3;
    const int HW = H * W, n = HW * 4;
    double m[4], c[4], ex[4], ey[4], gx[4], gy[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const size_t map = (size_t)b * 16 + q * 4 + r;
        m[r] = state[map * 4]; c[r] = beta / state[map * 4 + 1]; ex[r] = state[map * 4 + 2]; ey[r] = state[map * 4 + 3];
        gx[r] = (double)dcoords[map * 2]; gy[r] = (double)dcoords[map * 2 + 1];
    }
    const f32x4* in = reinterpret_cast<const f32x4*>(maps + (size_t)b * HW * 16);
    f32x4* out = reinterpret_cast<f32x4*>(dmaps + (size_t)b * HW * 16);
    for (int i = blockIdx.x * PA_SAM_BWD_THREADS + threadIdx.x; i < n; i += gridDim.x * PA_SAM_BWD_THREADS) {
        const int p = i >> 2, y = p / W, x = p - y * W;
        const double xd = (double)(x + 1), yd = (double)(y + 1);
        const f32x4 v = in[i];
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double e = sam_exp(beta * ((double)v[r] - m[r]));
            o[r] = (float)((c[r] * e) * ((xd - ex[r]) * gx[r] + (yd - ey[r]) * gy[r]));
        }
        out[i] = o;
    }
}

// strided: one workgroup per (sample, joint) map
__global__ __launch_bounds__(PA_SAM_GENERIC_THREADS) void soft_argmax_bwd_kernel(const float* maps, long sb, long sj, long sp, int J, int H, int W,
                                                                                 double beta, const double* state, const float* dcoords, float* dmaps) {
    const int map = blockIdx.x;
    const int b = map / J, j = map - b * J;
    const long off = b * sb + j * sj;
    const int HW = H * W;
    const double m = state[(size_t)map * 4], c = beta / state[(size_t)map * 4 + 1], ex = state[(size_t)map * 4 + 2], ey = state[(size_t)map * 4 + 3];
    const double gx = (double)dcoords[(size_t)map * 2], gy = (double)dcoords[(size_t)map * 2 + 1];
    for (int p = threadIdx.x; p < HW; p += PA_SAM_GENERIC_THREADS) {
        const int y = p / W, x = p - y * W;
        const double e = sam_exp(beta * ((double)maps[off + (long)p * sp] - m));
        dmaps[off + (long)p * sp] = (float)((c * e) * (((double)(x + 1) - ex) * gx + ((double)(y + 1) - ey) * gy));
    }
}

static bool sam_fast(const void* a, const void* b, int layout, int J) {
    return J == 16 && layout == 1 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

int pa_launch_soft_argmax(const float* maps, int layout, int B, int J, int H, int W, float beta, float* coords, double* state, hipStream_t st) {
    const long HW = (long)H * W;
    if (sam_fast(maps, nullptr, layout, J)) {
        hipLaunchKernelGGL(soft_argmax_nhwc16_kernel, dim3((unsigned)B * 4), dim3(PA_SAM_THREADS), 0, st, maps, H, W, (double)beta, coords, state);
        return (int)hipGetLastError();
    }
    const long sb = HW * J, sj = layout == 0 ? HW : 1, sp = layout == 0 ? 1 : J;
    hipLaunchKernelGGL(soft_argmax_kernel, dim3((unsigned)B * J), dim3(PA_SAM_GENERIC_THREADS), 0, st, maps, sb, sj, sp, J, H, W, (double)beta,
                       coords, state);
    return (int)hipGetLastError();
}

int pa_launch_soft_argmax_bwd(const float* maps, int layout, int B, int J, int H, int W, float beta, const double* state, const float* dcoords,
                              float* dmaps, hipStream_t st) {
    const long HW = (long)H * W;
    if (sam_fast(maps, dmaps, layout, J) && B <= 65535) {
        const long per = (long)PA_SAM_BWD_THREADS * PA_SAM_BWD_CHUNKS;
        const unsigned gx = (unsigned)((HW * 4 + per - 1) / per);
        hipLaunchKernelGGL(soft_argmax_bwd_nhwc16_kernel, dim3(gx, (unsigned)B), dim3(PA_SAM_BWD_THREADS), 0, st, maps, H, W, (double)beta, state,
                           dcoords, dmaps);
        return (int)hipGetLastError();
    }
    const long sb = HW * J, sj = layout == 0 ? HW : 1, sp = layout == 0 ? 1 : J;
    hipLaunchKernelGGL(soft_argmax_bwd_kernel, dim3((unsigned)B * J), dim3(PA_SAM_GENERIC_THREADS), 0, st, maps, sb, sj, sp, J, H, W, (double)beta,
                       state, dcoords, dmaps);
    return (int)hipGetLastError();
}

__global__ void exp_probe_kernel(const double* x, double* y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = sam_exp(x[i]);
}

int pa_launch_exp_probe(const double* x, double* y, size_t n, hipStream_t st) {
    size_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(exp_probe_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, y, n);
    return (int)hipGetLastError();
}
