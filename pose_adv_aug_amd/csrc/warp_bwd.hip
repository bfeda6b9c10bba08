// Backward of the pure inverse-affine bilinear sampler (warp_kernel, pose_ops.hip) for gfx950: d loss / d tinv and d loss / d gain per
// sample from d loss / d image, and through the chain rule of warp_bwd.h d loss / d {cx, cy, scale, rot, gain}.
//
// The forward computes per output pixel (u, v) of sample b, in double:
//   sx = ti0 u + ti1 v + ti2,  sy = ti3 u + ti4 v + ti5,  (x0, y0) = floor,  (ax, ay) = the fractions,
//   S_c = sum over the 2 x 2 taps of w_k p_k,c / 255  (a tap outside the sample's own w_b x h_b frame is 0; the frame mirrored when flip),
//   o_c = clamp(g_c S_c, 0, 1).
// Inside a source cell S_c is bilinear in (sx, sy):
//   dS_c/dsx = (1 - ay)(p01 - p00) + ay (p11 - p10),   dS_c/dsy = (1 - ax)(p10 - p00) + ax (p11 - p01)       (/ 255)
// with the taps as the forward read them.  floor has derivative 0: at an integer sx (ax = 0) this is the derivative of the cell the forward
// sampled, the one to the right.  The clamp passes the gradient where 0 <= g_c S_c <= 1 (torch.clamp's rule, bounds included, on the
// double pre-clamp value: a pixel outside the frame is an exact 0, passes, and contributes exact zeros).  The float cast of the output and
// the rounding of out4 to the storage type are not differentiated.
//   gx = sum_c dimg_c m_c g_c dS_c/dsx (gy likewise);   dtinv = sum over pixels {gx u, gx v, gx, gy u, gy v, gy};   dgain_c = sum dimg_c m_c S_c
//
// Two launches, everything in double, no atomics (the same input gives the same bits), no host synchronisation:
//   1. warp_bwd_kernel: one 256-thread workgroup per strip of PA_WARP_BWD_ROWS output rows of one sample.  A thread keeps the nine sums of
//      its pixels in registers; one butterfly per wave at the end, the four waves combined through LDS in a fixed order, and lanes 0 .. 8
//      store the strip's nine doubles to workspace[b][strip][9] with one store instruction.
//   2. warp_bwd_finish_kernel: one 64-thread workgroup per sample adds the strips in ascending order, writes dtinv and dgain, and lane 0
//      applies the chain rule to the augmentation parameters.
// The two source pixels of a tap row are adjacent in memory whether or not the frame is mirrored (columns x0, x0 + 1, or w - 2 - x0,
// w - 1 - x0).  Where both lie inside the frame their six bytes are read from one address as one 4-byte and one 2-byte load (the address
// has no alignment), two such pairs per pixel; where the pair straddles the frame's edge the one pixel inside is read byte by byte.
#include "warp_bwd.h"

template <int LAYOUT>
__global__ __launch_bounds__(256) void warp_bwd_kernel(const unsigned char* __restrict__ src, int Hs, int Ws, const int* __restrict__ sizes,
                                                       const double* __restrict__ tinv, const double* __restrict__ params, int res,
                                                       int nstrips, const float* __restrict__ dimg, double* __restrict__ partial) {
    // every product and sum rounded on its own: where the compiler fuses a multiply-add depends on the code around it, and the two
    // layouts (two instantiations) must give the same bits
#pragma clang fp contract(off)
    __shared__ double lds[4][9];
    const int b = blockIdx.x / nstrips, strip = blockIdx.x - b * nstrips;
    const int v0 = strip * PA_WARP_BWD_ROWS;
    const int rows = res - v0 < PA_WARP_BWD_ROWS ? res - v0 : PA_WARP_BWD_ROWS;
    const int npix = rows * res;
    const double* ti = tinv + (size_t)b * 6;
    const double* p = params + (size_t)b * 8;
    const double t0 = ti[0], t1 = ti[1], t2 = ti[2], t3 = ti[3], t4 = ti[4], t5 = ti[5];
    const bool flip = p[4] != 0.0;
    const double g[3] = {p[5], p[6], p[7]};
    const double kc[3] = {g[0] / 255.0, g[1] / 255.0, g[2] / 255.0};
    int wb = sizes ? sizes[2 * b] : Ws, hb = sizes ? sizes[2 * b + 1] : Hs;
    wb = wb < Ws ? wb : Ws;                     // (a frame never exceeds the padded buffer: nothing outside src is read)
    hb = hb < Hs ? hb : Hs;
    const size_t hw = (size_t)res * res;
    double acc[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[j] = 0.0;

    for (int i = threadIdx.x; i < npix; i += 256) {
        const int dv = i / res, u = i - dv * res, v = v0 + dv;
        const size_t pix = (size_t)v * res + u;
        float d[3];
        if (LAYOUT == 1) {
            const f32x4 d4 = *reinterpret_cast<const f32x4*>(dimg + ((size_t)b * hw + pix) * 4);
            d[0] = d4[0]; d[1] = d4[1]; d[2] = d4[2];
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = dimg[((size_t)b * 3 + c) * hw + pix];
        }
        const double sx = t0 * u + t1 * v + t2, sy = t3 * u + t4 * v + t5;
        const double fx0 = floor(sx), fy0 = floor(sy);
        const double ax = sx - fx0, ay = sy - fy0;
        // cells far outside the frame (and a NaN coordinate) are taken to the nearest cell that has no tap inside it
        const int x0 = (int)fmin(fmax(fx0, -2.0), (double)wb), y0 = (int)fmin(fmax(fy0, -2.0), (double)hb);
        // memory order of the pair: columns lo, lo + 1; the forward's LEFT tap (xx = x0) is the second of them when the frame is mirrored
        const int lo = flip ? wb - 2 - x0 : x0;
        const bool okA = (unsigned)lo < (unsigned)wb, okB = (unsigned)(lo + 1) < (unsigned)wb;
        int tap[2][2][3];                       // [row][left / right of the forward][channel]
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int yy = y0 + r;
            int A[3] = {0, 0, 0}, Bp[3] = {0, 0, 0};
            if ((unsigned)yy < (unsigned)hb) {
                const long base = (((long)b * Hs + yy) * Ws + lo) * 3;
                if (okA && okB) {               // both columns inside the frame: the six bytes as one 4-byte and one 2-byte read (any alignment)
                    unsigned w0;
                    unsigned short w1;
                    __builtin_memcpy(&w0, src + base, 4);
                    __builtin_memcpy(&w1, src + base + 4, 2);
                    A[0] = w0 & 255; A[1] = (w0 >> 8) & 255; A[2] = (w0 >> 16) & 255;
                    Bp[0] = w0 >> 24; Bp[1] = w1 & 255; Bp[2] = w1 >> 8;
                } else if (okA) {               // the pair straddles the frame's edge: the one pixel inside it, byte by byte
                    A[0] = src[base]; A[1] = src[base + 1]; A[2] = src[base + 2];
                } else if (okB) {
                    Bp[0] = src[base + 3]; Bp[1] = src[base + 4]; Bp[2] = src[base + 5];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) { tap[r][0][c] = flip ? Bp[c] : A[c]; tap[r][1][c] = flip ? A[c] : Bp[c]; }
        }
        const double wx0 = 1.0 - ax, wy0 = 1.0 - ay;
        double gx = 0.0, gy = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int p00 = tap[0][0][c], p01 = tap[0][1][c], p10 = tap[1][0][c], p11 = tap[1][1][c];
            // S_c as the forward adds it (taps in its order)
            double S = (wx0 * wy0) * ((double)p00 / 255.0);
            S += (ax * wy0) * ((double)p01 / 255.0);
            S += (wx0 * ay) * ((double)p10 / 255.0);
            S += (ax * ay) * ((double)p11 / 255.0);
            const double pre = S * g[c];
            const double dm = (pre >= 0.0 && pre <= 1.0) ? (double)d[c] : 0.0;
            const double dxs = wy0 * (double)(p01 - p00) + ay * (double)(p11 - p10);          // byte differences are exact
            const double dys = wx0 * (double)(p10 - p00) + ax * (double)(p11 - p01);
            const double t = dm * kc[c];
            gx += t * dxs;
            gy += t * dys;
            acc[6 + c] += dm * S;
        }
        acc[0] += gx * u; acc[1] += gx * v; acc[2] += gx;
        acc[3] += gy * u; acc[4] += gy * v; acc[5] += gy;
    }

    // one butterfly per wave (wave64), then the four waves in a fixed order
#pragma unroll
    for (int j = 0; j < 9; ++j) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 9; ++j) lds[wave][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const int j = threadIdx.x;
        partial[(size_t)blockIdx.x * 9 + j] = ((lds[0][j] + lds[1][j]) + lds[2][j]) + lds[3][j];
    }
}

__global__ __launch_bounds__(64) void warp_bwd_finish_kernel(const double* __restrict__ partial, int nstrips, const double* __restrict__ params,
                                                             int res, double* dtinv, double* dgain, double* dparams) {
    __shared__ double s[9];
    const int b = blockIdx.x, j = threadIdx.x;
    if (j < 9) {
        const double* q = partial + (size_t)b * nstrips * 9 + j;
        double a = 0.0;
#pragma unroll 8
        for (int i = 0; i < nstrips; ++i) a += q[(size_t)i * 9];          // (unrolled: the loads of eight strips travel together; the order of the additions stays)
        s[j] = a;
        if (j < 6) { if (dtinv) dtinv[(size_t)b * 6 + j] = a; }
        else if (dgain) dgain[(size_t)b * 3 + (j - 6)] = a;
    }
    __syncthreads();
    if (j == 0 && dparams) {
        double G[6], dg[3], out[8];
#pragma unroll
        for (int i = 0; i < 6; ++i) G[i] = s[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) dg[i] = s[6 + i];
        pa_affine_params_chain(params + (size_t)b * 8, G, dg, (double)res, out);
#pragma unroll
        for (int i = 0; i < 8; ++i) dparams[(size_t)b * 8 + i] = out[i];
    }
}

int pa_launch_warp_bwd(const unsigned char* src, int Hs, int Ws, const int* sizes, const double* tinv, const double* params, int B, int res,
                       const float* dimg, int layout, void* workspace, double* dtinv, double* dgain, double* dparams, hipStream_t st) {
    const long nstrips = pa_warp_bwd_strips(B, res);          // (the arguments are checked once, in pa_affine_warp_bilinear_bwd)
    if (nstrips == 0) { pa_set_error_msg("pa_launch_warp_bwd: bad shape"); return 1; }
    double* partial = reinterpret_cast<double*>(workspace);
    const dim3 grid((unsigned)(nstrips * B));
    if (layout == 1) hipLaunchKernelGGL(warp_bwd_kernel<1>, grid, dim3(256), 0, st, src, Hs, Ws, sizes, tinv, params, res, (int)nstrips, dimg, partial);
    else hipLaunchKernelGGL(warp_bwd_kernel<0>, grid, dim3(256), 0, st, src, Hs, Ws, sizes, tinv, params, res, (int)nstrips, dimg, partial);
    hipLaunchKernelGGL(warp_bwd_finish_kernel, dim3(B), dim3(64), 0, st, partial, (int)nstrips, params, res, dtinv, dgain, dparams);
    return (int)hipGetLastError();
}
