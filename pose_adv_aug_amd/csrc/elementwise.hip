// Streaming (HBM-bound) kernels around the convolutions: BatchNorm bookkeeping, 2x2 max pool,
// nearest-upsample + add, their backward passes with the ReLU mask / BatchNorm-backward reductions
// fused in, RMSprop, weight re-packing and layout conversion.  NHWC bf16, 16-byte accesses
// (8 channels per thread), per-channel reductions staged through LDS atomics, one global atomic per
// channel per workgroup.
#include "common.h"
#include "kernels.h"
// wave priority of the main chain's finalize / pooling / upsampling kernels beside the weight-gradient group kernels (priority 0): 5.863 -> 5.842 ms (four interleaved pairs, round 5)
#ifndef PA_ELT_PRIO
#define PA_ELT_PRIO 2
#endif
#define PA_SET_ELT_PRIO() do { if (PA_ELT_PRIO > 0) __builtin_amdgcn_s_setprio(PA_ELT_PRIO); } while (0)
#include "bn_fin.h"
#include <type_traits>
#include <hip/hip_ext.h>
// TIMING EXPERIMENT (tuning builds, PA_FIN_ANYORDER=1; results may be WRONG): the finalize launches without the completion / cache round trip
// behind their producer (hipExtAnyOrderLaunch) -- what a tagged-row hand-off from the producers to the finalize kernel could return at most
static unsigned fin_launch_flags() { return pa_tuning().fin_anyorder ? hipExtAnyOrderLaunch : 0u; }
template <class... P, class... A>
static void fin_launch(void (*kernel)(P...), dim3 grid, int threads, hipStream_t st, A... args) {
    if (fin_launch_flags()) hipExtLaunchKernelGGL(kernel, grid, dim3(threads), 0, st, nullptr, nullptr, fin_launch_flags(), static_cast<P>(args)...);
    else hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, st, static_cast<P>(args)...);
}

// ------------------------------------------------------------------------------------------------
// BatchNorm bookkeeping (reference semantics: torch.nn.BatchNorm2d, eps 1e-5, momentum 0.1,
// biased variance for normalisation, unbiased for the running estimate).
// Sum `rows` partial rows [rows][C][2] for the FC channels of this workgroup: FT threads =
// FC channels x (FT / FC) row slices, float2 loads, LDS tree over the slices.  Result in LDS sums[FC][2].
// FC = 8: 16-32 workgroups per BatchNorm (the kernel is pure latency: launch + row loads in batches + tree; 32 channels per workgroup
// took 6 us; FC = 4 -- every common row count in ONE batch of loads, twice the workgroups -- measured 0.03 ms per step slower, round 4).
// workgroup shape of the finalize launches: FIN_T threads = FIN_C channels x FIN_T / FIN_C row slices.
// 512 threads (8 channels x 64 row slices): measured 6.44 - 6.49 ms per step against 6.50 - 6.54 with 1024-thread workgroups (three
// interleaved pairs; 256 threads, or 4 channels per workgroup: the same as 512 / 8) -- a 1024-thread workgroup has to find a whole CU's
// worth of wave slots next to the other queues' kernels, and the launch is all these kernels are
constexpr int FIN_T = 512, FIN_C = 8;
template <int FT, int FC>
__device__ __forceinline__ void reduce_partial_rows(const float* part, int rows, int C, int c0, float (*sums)[2]) {
    constexpr int SL = FT / FC;
    __shared__ __attribute__((aligned(16))) float red[SL][FC + 1][2];
    const int cl = threadIdx.x % FC, sl = threadIdx.x / FC;
    if (rows <= PA_FIN_SMALL_ROWS) {
        // the order the consumer-prologue form of the finalize uses too (bn_fin.h): sixteen interleaved chains, stride-halving tree;
        // here one thread per chain and channel pair (4 pairs x 16 chains), ONE round of <= 8 loads each
        constexpr int NP = FC / 2;                                       // channel pairs of this workgroup
        f32x4* part4 = reinterpret_cast<f32x4*>(&red[0][0][0]);          // [16][NP]
        if (threadIdx.x < 16 * NP) {
            const int pr = threadIdx.x % NP, j = threadIdx.x / NP;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            part4[j * NP + pr] = c0 + 2 * pr < C ? pa_fin_chain16(part, rows, C, c0 + 2 * pr, j) : z;
        }
        __syncthreads();
        if (threadIdx.x < FC) {
            const int c = threadIdx.x, half = c & 1;
            float a[16], b[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) { const f32x4 v = part4[i * NP + (c >> 1)]; a[i] = half ? v[2] : v[0]; b[i] = half ? v[3] : v[1]; }
#pragma unroll
            for (int n = 16; n > 1; n >>= 1)
#pragma unroll
                for (int i = 0; i < n / 2; ++i) { a[i] += a[i + n / 2]; b[i] += b[i + n / 2]; }
            sums[c][0] = a[0]; sums[c][1] = b[0];
        }
        __syncthreads();
        return;
    }
    float a = 0.f, b = 0.f;
    if (c0 + cl < C) {
        // the thread's rows sl, sl + SL, ... in batches of NB loads in flight (clamped, unconditional; the sums stay in increasing order):
        // hipcc compiled the plain loop `#pragma unroll 8` into a one-load-one-wait remainder loop in FRONT of the unrolled body, i.e. 3 / 6
        // serial memory round trips at 384 / 768 rows in a kernel that is nothing but latency.  NB = 4 up to 512 rows (one round trip,
        // <= 3 loads wasted), 8 above (768 rows: one round trip; 1536: two)
        auto batches = [&](auto nbc) {
            constexpr int NB = decltype(nbc)::value;
            for (int r0 = sl; r0 < rows; r0 += NB * SL) {
                f32x2 v[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int r = r0 + u * SL;
                    v[u] = *reinterpret_cast<const f32x2*>(part + ((size_t)(r < rows ? r : r0) * C + c0 + cl) * 2);
                }
#pragma unroll
                for (int u = 0; u < NB; ++u)
                    if (r0 + u * SL < rows) { a += v[u][0]; b += v[u][1]; }
            }
        };
        if (rows <= 4 * SL) batches(std::integral_constant<int, 4>{});
        else if (rows <= 8 * SL) batches(std::integral_constant<int, 8>{});
        else batches(std::integral_constant<int, 12>{});      // (1536 rows at 128 slices: ONE round trip instead of 8 + 4)
    }
    red[sl][cl][0] = a; red[sl][cl][1] = b;
    __syncthreads();
    // two-level tree over the SL slices: 16 groups of SL/16 slices, then the 16 group sums
    const bool act = threadIdx.x < FC * 16;
    const int tc = threadIdx.x % FC, tg = threadIdx.x / FC;
    float x2 = 0.f, y2 = 0.f;
    if (act) {
#pragma unroll
        for (int s = tg * (SL / 16); s < (tg + 1) * (SL / 16); ++s) { x2 += red[s][tc][0]; y2 += red[s][tc][1]; }
    }
    __syncthreads();
    if (act) { red[tg][tc][0] = x2; red[tg][tc][1] = y2; }
    __syncthreads();
    if (threadIdx.x < FC) {
        float x = 0.f, y = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) { x += red[s][threadIdx.x][0]; y += red[s][threadIdx.x][1]; }
        sums[threadIdx.x][0] = x; sums[threadIdx.x][1] = y;
    }
    __syncthreads();
}

// one finalize as PaBnFin describes it (bn_fin.h): forward here, backward below
__global__ __launch_bounds__(FIN_T) void bn_fin_fwd_kernel(PaBnFin f, int C) {
    PA_SET_ELT_PRIO();
    __shared__ float sums[FIN_C][2];
    const int c0 = blockIdx.x * FIN_C;
    // the channel's parameters are requested BEFORE the reduction (after it they were one more dependent memory round trip of a kernel that
    // is nothing but round trips)
    const bool mine = threadIdx.x < FIN_C && c0 + (int)threadIdx.x < C;
    float g = 0.f, bt = 0.f, rm = 0.f, rv = 0.f;
    if (mine) {
        g = f.gamma[c0 + threadIdx.x]; bt = f.beta[c0 + threadIdx.x];
        if (f.update_running) { rm = f.rmean[c0 + threadIdx.x]; rv = f.rvar[c0 + threadIdx.x]; }
    }
    reduce_partial_rows<FIN_T, FIN_C>(f.stats, f.rows, C, c0, sums);
    if (!mine) return;
    const int c = c0 + threadIdx.x;
    float s, sh, mu, is, var;
    pa_bn_fwd_consts(sums[threadIdx.x][0], sums[threadIdx.x][1], f.count, f.eps, g, bt, s, sh, mu, is, var);
    f.scale[c] = s; f.shift[c] = sh; f.mean[c] = mu; f.invstd[c] = is;
    if (f.update_running) {
        pa_bn_running(mu, var, f.count, f.momentum, rm, rv);
        f.rmean[c] = rm; f.rvar[c] = rv;
    }
}

__global__ void bn_eval_kernel(const PaBnEvalJob* jobs, float eps) {
    const PaBnEvalJob j = jobs[blockIdx.x];
    for (int c = threadIdx.x; c < j.C; c += blockDim.x) {
        float s = j.gamma[c] * rsqrtf(j.rvar[c] + eps);
        j.scale[c] = s;
        j.shift[c] = j.beta[c] - j.rmean[c] * s;
    }
}

int pa_launch_bn_eval(const PaBnEvalJob* jobs_dev, int njobs, float eps, hipStream_t st) {
    if (njobs <= 0) return 0;
    hipLaunchKernelGGL(bn_eval_kernel, dim3(njobs), dim3(256), 0, st, jobs_dev, eps);
    return (int)hipGetLastError();
}

// dx = s*(dz - S1/M - xhat*S2/M) = kA*dz + kB*x + kC    (per channel)
// one BatchNorm-backward finalize (gridDim.y == 1) or two in one launch (blockIdx.y picks the layer: the upsample-add backward feeds two at once)
__global__ __launch_bounds__(FIN_T) void bn_fin_bwd_kernel(PaBnFin f0, int C0, PaBnFin f1, int C1) {
    PA_SET_ELT_PRIO();
    const PaBnFin& f = blockIdx.y == 0 ? f0 : f1;
    const int C = blockIdx.y == 0 ? C0 : C1;
    __shared__ float sums[FIN_C][2];
    const int c0 = blockIdx.x * FIN_C;
    if (c0 >= C) return;
    const bool mine = threadIdx.x < FIN_C && c0 + (int)threadIdx.x < C;
    float sc = 0.f, is = 0.f, mu = 0.f;              // (requested before the reduction, see bn_fin_fwd_kernel)
    if (mine) { sc = f.scale[c0 + threadIdx.x]; is = f.invstd[c0 + threadIdx.x]; mu = f.mean[c0 + threadIdx.x]; }
    reduce_partial_rows<FIN_T, FIN_C>(f.stats, f.rows, C, c0, sums);
    if (!mine) return;
    const int c = c0 + threadIdx.x;
    float S1 = sums[threadIdx.x][0], S2 = sums[threadIdx.x][1];
    float ka, kb, kc;
    pa_bn_bwd_consts(S1, S2, f.count, sc, is, mu, ka, kb, kc);
    f.kA[c] = ka; f.kB[c] = kb; f.kC[c] = kc;
    if (f.dgamma) f.dgamma[c] = S2;
    if (f.dbeta) f.dbeta[c] = S1;
}

static const char* const fin_odd_c = "BatchNorm finalize: the statistics rows are read as 16-byte channel pairs -- C must be even (the networks pad to 64)";

int pa_launch_bn_fin(const PaBnFin& f, int C, hipStream_t st) {
    if (C & 1) { pa_set_error_msg(fin_odd_c); return 1; }
    const dim3 grid((C + FIN_C - 1) / FIN_C);
    if (f.bwd) fin_launch(bn_fin_bwd_kernel, grid, FIN_T, st, f, C, f, C);      // (one layer: gridDim.y == 1)
    else fin_launch(bn_fin_fwd_kernel, grid, FIN_T, st, f, C);
    return (int)hipGetLastError();
}

int pa_launch_bn_fin2(const PaBnFin& a, int Ca, const PaBnFin& b, int Cb, hipStream_t st) {
    if (!a.bwd || !b.bwd) { pa_set_error_msg("BatchNorm finalize: the pair launch takes two backward finalizes"); return 1; }
    if ((Ca | Cb) & 1) { pa_set_error_msg(fin_odd_c); return 1; }
    fin_launch(bn_fin_bwd_kernel, dim3(((Ca > Cb ? Ca : Cb) + FIN_C - 1) / FIN_C, 2), FIN_T, st, a, Ca, b, Cb);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// apply an epilogue to 8 channel values at element offset idx (channel c..c+7); s1/s2 accumulate the
// per-channel reductions of the STATS / BWD modes
__device__ __forceinline__ bf16x8 epilogue8(const PaEpilogue& ep, size_t idx, int c, const float (&v)[8],
                                            float (&s1)[8], float (&s2)[8]) {
    bf16x8 o;
    if (ep.mode == PA_OUT_BWD) {
        bf16x8 xr = *reinterpret_cast<const bf16x8*>(ep.xref + idx);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float x = (float)xr[j];
            float dz = (fmaf(ep.scale[c + j], x, ep.shift[c + j]) > 0.f) ? v[j] : 0.f;
            o[j] = (bf16)dz;
            float dzr = (float)o[j];
            s1[j] += dzr;
            s2[j] += dzr * (x - ep.mean[c + j]) * ep.invstd[c + j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            o[j] = (bf16)v[j];
            float r = (float)o[j];
            s1[j] += r;
            s2[j] += r * r;
        }
    }
    return o;
}

// block-level flush of per-thread channel partials: LDS float atomics, then this workgroup's own
// partial row gstats[blockIdx.x][C][2] (plain stores; the BatchNorm finalize kernels sum the rows)
// Per-workgroup partial row of the two per-channel reductions of a streaming kernel whose threads own the
// 8-channel group  c/8 = threadIdx.x % (C/8): shuffle-reduce the lanes of a wave that share a group, one LDS
// row per wave, then a tree over the waves.  (LDS float atomics here cost 8-32 k serialized atomics per
// workgroup: ~10 us of tail.)  red: [nwaves][2*C] floats of LDS.
__device__ __forceinline__ void flush_stats(float* red, float* gstats, int C, int c, const float (&s1)[8], const float (&s2)[8]) {
    const int CG = C / 8, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    float a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        a[j] = s1[j]; b[j] = s2[j];
        for (int o = 32; o >= CG; o >>= 1) { a[j] += __shfl_xor(a[j], o, 64); b[j] += __shfl_xor(b[j], o, 64); }
    }
    __syncthreads();                       // (callers may have used `red` before)
    if (lane < CG) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { red[wave * 2 * C + c + j] = a[j]; red[wave * 2 * C + C + c + j] = b[j]; }
    }
    __syncthreads();
    float* row = gstats + (size_t)blockIdx.x * C * 2;
    for (int i = threadIdx.x; i < C; i += blockDim.x) {
        float x = 0.f, y = 0.f;
        for (int w = 0; w < nw; ++w) { x += red[w * 2 * C + i]; y += red[w * 2 * C + C + i]; }
        f32x2 v = {x, y};
        *reinterpret_cast<f32x2*>(row + i * 2) = v;
    }
}

struct Bwd8 {            // one BatchNorm-backward epilogue on 8 channels: dz = g * [s*x+t > 0], sums of dz and dz*xhat
    __device__ __forceinline__ static bf16x8 apply(const float4* cst, int c, const bf16x8& xr, const float (&g)[8], float (&s1)[8], float (&s2)[8]) {
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4 k = cst[c + j];
            const float x = (float)xr[j];
            const float dz = (fmaf(k.x, x, k.y) > 0.f) ? g[j] : 0.f;
            o[j] = (bf16)dz;
            const float dzr = (float)o[j];
            s1[j] += dzr;
            s2[j] += dzr * (x - k.z) * k.w;
        }
        return o;
    }
};

__device__ __forceinline__ void stage_bwd_consts(float4* dst, const PaEpilogue& ep, int C) {
    for (int i = threadIdx.x; i < C; i += blockDim.x) dst[i] = make_float4(ep.scale[i], ep.shift[i], ep.mean[i], ep.invstd[i]);
}

// ------------------------------------------------------------------------------------------------
// 2x2/2 max pool (reference models/asn_stacked_hg.py:69,227), input transform applied on load
// MAP: also store the arg-max position k = 2 * row + col (first maximum in scan order, strict >: the rule of maxpool_bwd_*) of every pooled
// element as a byte, laid out like `out` -- the data gradient of the pool's other consumer routes the gradient through it (PA_LD_POOL)
template <bool MAP>
__global__ void maxpool_fwd_kernel(PaOperand in, bf16* out, unsigned char* map, int B, int H, int W, int C) {
    const int Ho = H / 2, Wo = W / 2, CG = C / 8;
    const size_t total = (size_t)B * Ho * Wo * CG;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        int cg = (int)(t % CG);
        size_t p = t / CG;
        int xo = (int)(p % Wo);
        size_t q = p / Wo;
        int yo = (int)(q % Ho), b = (int)(q / Ho);
        int c = cg * 8;
        float m[8], am[8];
        unsigned arg[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            size_t idx = (((size_t)b * H + 2 * yo + (k >> 1)) * W + 2 * xo + (k & 1)) * C + c;
            float v[8];
            pa_read8(in, idx, c, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                m[j] = (k == 0) ? v[j] : fmaxf(m[j], v[j]);
                if (MAP) { if (k == 0) { am[j] = v[j]; arg[j] = 0u; } else if (v[j] > am[j]) { am[j] = v[j]; arg[j] = (unsigned)k; } }
            }
        }
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (bf16)m[j];
        *reinterpret_cast<bf16x8*>(out + p * C + c) = o;
        if (MAP) {
            uint2 w;
            w.x = arg[0] | (arg[1] << 8) | (arg[2] << 16) | (arg[3] << 24);
            w.y = arg[4] | (arg[5] << 8) | (arg[6] << 16) | (arg[7] << 24);
            *reinterpret_cast<uint2*>(map + p * C + c) = w;
        }
    }
}

// out = nearest_upsample_x2(low) + skip   (reference models/asn_stacked_hg.py:193-203)
__global__ void upadd_fwd_kernel(PaOperand low, PaOperand skip, bf16* out, int B, int H, int W, int C) {
    const int CG = C / 8, Hl = H / 2, Wl = W / 2;
    const size_t total = (size_t)B * H * W * CG;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        int cg = (int)(t % CG);
        size_t p = t / CG;
        int x = (int)(p % W);
        size_t q = p / W;
        int y = (int)(q % H), b = (int)(q / H);
        int c = cg * 8;
        float a[8], s[8];
        pa_read8(low, (((size_t)b * Hl + (y >> 1)) * Wl + (x >> 1)) * C + c, c, a);
        pa_read8(skip, p * C + c, c, s);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (bf16)(a[j] + s[j]);
        *reinterpret_cast<bf16x8*>(out + p * C + c) = o;
    }
}


// ---- streaming forward variants (row indexing, template modes, thread-fixed channel constants in registers, all loads of an
// item issued first): OP 0 = 2x2 max pool of value(in), OP 1 = nearest-upsample(low) + value(skip); item = one low-resolution
// pixel x 8 channels (4 high-resolution pixels).  Operand modes PLAIN / BNRELU.
// MAP (OP 0): 1 = also the arg-max byte map (maxpool_fwd_kernel); 2 = the map and xmax, the RAW input value at the arg-max (the stem's pool: its
// backward reductions then need a quarter of the input, maxpool_bwd_stats_kernel)
template <int OP, int MA, int MB, int MAP = 0>
__global__ __launch_bounds__(256) void pool_up_fwd_s_kernel(PaOperand a, PaOperand b, bf16* __restrict__ out, int rows, int W, int C,
                                                            unsigned char* __restrict__ map = nullptr, bf16* __restrict__ xmax = nullptr) {
    PA_SET_ELT_PRIO();
    // rows = B * H/2 (low-resolution rows); W = high-resolution width
    const int CG = C / 8, Wl = W / 2;
    const unsigned row_items = (unsigned)Wl * CG;
    const int c = (threadIdx.x % CG) * 8;
    float a0[8], a1[8], b0[8], b1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (MA == PA_LD_BNRELU) { a0[j] = a.k0[c + j]; a1[j] = a.k1[c + j]; }
        if (OP == 1 && MB == PA_LD_BNRELU) { b0[j] = b.k0[c + j]; b1[j] = b.k1[c + j]; }
    }
    const unsigned rows_per_it = row_items >= blockDim.x ? 1u : blockDim.x / row_items;
    const unsigned rsub = row_items >= blockDim.x ? 0u : threadIdx.x / row_items;
    const unsigned i0 = row_items >= blockDim.x ? threadIdx.x : threadIdx.x % row_items;
    const bf16* __restrict__ pa = a.p;
    const bf16* __restrict__ pb = b.p;
    for (unsigned rb = blockIdx.x * rows_per_it; rb < (unsigned)rows; rb += gridDim.x * rows_per_it) {
        const unsigned r = rb + rsub;
        if (r >= (unsigned)rows) continue;
        for (unsigned i = i0; i < row_items; i += blockDim.x) {
            const unsigned xl = i / (unsigned)CG;
            const unsigned top = ((2u * r) * (unsigned)W + 2u * xl) * (unsigned)C + (unsigned)c;
            const unsigned wc = (unsigned)W * (unsigned)C;
            const unsigned off[4] = {top, top + (unsigned)C, top + wc, top + wc + (unsigned)C};
            const unsigned li = (r * (unsigned)Wl + xl) * (unsigned)C + (unsigned)c;
            bf16x8 hi[4], lo;
#pragma unroll
            for (int k = 0; k < 4; ++k) hi[k] = *reinterpret_cast<const bf16x8*>((OP == 0 ? pa : pb) + off[k]);
            if (OP == 1) lo = *reinterpret_cast<const bf16x8*>(pa + li);
            if (OP == 0) {
                bf16x8 o, xm;
                unsigned arg[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float m = 0.f, am = 0.f;
                    arg[j] = 0u;
                    xm[j] = hi[0][j];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float v = (float)hi[k][j];
                        if (MA == PA_LD_BNRELU) v = fmaxf(fmaf(a0[j], v, a1[j]), 0.f);
                        m = k == 0 ? v : fmaxf(m, v);
                        if (MAP) { if (k == 0) am = v; else if (v > am) { am = v; arg[j] = (unsigned)k; if (MAP == 2) xm[j] = hi[k][j]; } }
                    }
                    o[j] = (bf16)m;
                }
                *reinterpret_cast<bf16x8*>(out + li) = o;
                if (MAP) {
                    uint2 w;
                    w.x = arg[0] | (arg[1] << 8) | (arg[2] << 16) | (arg[3] << 24);
                    w.y = arg[4] | (arg[5] << 8) | (arg[6] << 16) | (arg[7] << 24);
                    *reinterpret_cast<uint2*>(map + li) = w;
                    if (MAP == 2) *reinterpret_cast<bf16x8*>(xmax + li) = xm;
                }
            } else {
                float l[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float v = (float)lo[j];
                    if (MA == PA_LD_BNRELU) v = fmaxf(fmaf(a0[j], v, a1[j]), 0.f);
                    l[j] = v;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    bf16x8 o;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float v = (float)hi[k][j];
                        if (MB == PA_LD_BNRELU) v = fmaxf(fmaf(b0[j], v, b1[j]), 0.f);
                        o[j] = (bf16)(l[j] + v);
                    }
                    *reinterpret_cast<bf16x8*>(out + off[k]) = o;
                }
            }
        }
    }
}

// OP 0: max pool of `a`; OP 1: upsample(a) + b.  The streaming kernel where the plan and the operand modes admit it, else the generic one.
template <int OP>
static int launch_pool_up_fwd(const PaOperand& a, const PaOperand& b, bf16* out, int B, int H, int W, int C, hipStream_t st, unsigned char* map = nullptr,
                              bf16* xmax = nullptr) {
    const bool ma = a.mode == PA_LD_PLAIN || a.mode == PA_LD_BNRELU, mb = OP == 0 || b.mode == PA_LD_PLAIN || b.mode == PA_LD_BNRELU;
    const int rows = B * (H / 2);
    const size_t items = (size_t)rows * (W / 2) * (C / 8);
    PaEltPlan p;
    if (pa_elt_plan(p, PA_ELT_FWD, items, B, H, W, C, false, ma && mb)) return 1;
    const bool A = a.mode == PA_LD_BNRELU, Bm = OP == 1 && b.mode == PA_LD_BNRELU;
    if (xmax && (!p.streaming || !map || !A)) { pa_set_error_msg("max pool: the value at the arg-max comes from the streaming kernel only (pa_pool_stats_route_supported)"); return 1; }
    if (!p.streaming) {
        // (the generic upsample-add walks the high-resolution pixels)
        if (OP == 0 && map) hipLaunchKernelGGL(maxpool_fwd_kernel<true>, dim3(p.blocks), dim3(p.threads), 0, st, a, out, map, B, H, W, C);
        else if (OP == 0) hipLaunchKernelGGL(maxpool_fwd_kernel<false>, dim3(p.blocks), dim3(p.threads), 0, st, a, out, map, B, H, W, C);
        else hipLaunchKernelGGL(upadd_fwd_kernel, dim3(pa_grid_for((size_t)B * H * W * (C / 8), p.threads, 4096)), dim3(p.threads), 0, st, a, b, out, B, H, W, C);
    }
    else if (OP == 0 && xmax) hipLaunchKernelGGL((pool_up_fwd_s_kernel<0, PA_LD_BNRELU, PA_LD_PLAIN, 2>), dim3(p.blocks), dim3(p.threads), 0, st, a, b, out, rows, W, C, map, xmax);
    else if (OP == 0 && map) {
        if (A) hipLaunchKernelGGL((pool_up_fwd_s_kernel<0, PA_LD_BNRELU, PA_LD_PLAIN, 1>), dim3(p.blocks), dim3(p.threads), 0, st, a, b, out, rows, W, C, map, nullptr);
        else hipLaunchKernelGGL((pool_up_fwd_s_kernel<0, PA_LD_PLAIN, PA_LD_PLAIN, 1>), dim3(p.blocks), dim3(p.threads), 0, st, a, b, out, rows, W, C, map, nullptr);
    }
    else if (A && Bm) hipLaunchKernelGGL((pool_up_fwd_s_kernel<OP, PA_LD_BNRELU, PA_LD_BNRELU>), dim3(p.blocks), dim3(p.threads), 0, st, a, b, out, rows, W, C, nullptr, nullptr);
    else if (A) hipLaunchKernelGGL((pool_up_fwd_s_kernel<OP, PA_LD_BNRELU, PA_LD_PLAIN>), dim3(p.blocks), dim3(p.threads), 0, st, a, b, out, rows, W, C, nullptr, nullptr);
    else if (Bm) hipLaunchKernelGGL((pool_up_fwd_s_kernel<OP, PA_LD_PLAIN, PA_LD_BNRELU>), dim3(p.blocks), dim3(p.threads), 0, st, a, b, out, rows, W, C, nullptr, nullptr);
    else hipLaunchKernelGGL((pool_up_fwd_s_kernel<OP, PA_LD_PLAIN, PA_LD_PLAIN>), dim3(p.blocks), dim3(p.threads), 0, st, a, b, out, rows, W, C, nullptr, nullptr);
    return (int)hipGetLastError();
}

int pa_launch_maxpool_fwd(const PaOperand& in, bf16* out, int B, int H, int W, int C, hipStream_t st, unsigned char* map, bf16* xmax) {
    return launch_pool_up_fwd<0>(in, in, out, B, H, W, C, st, map, xmax);
}

// gradient of the max pool: routed to the first maximum in scan order (torch semantics), plus an
// optional addend (other consumers' gradient), then the epilogue of the tensor being differentiated
__global__ __launch_bounds__(1024) void maxpool_bwd_kernel(const bf16* dout, PaOperand in, PaOperand add, PaEpilogue ep, bf16* din,
                                   int B, int H, int W, int C) {
    extern __shared__ float red[];
    const int Ho = H / 2, Wo = W / 2, CG = C / 8;
    const size_t total = (size_t)B * Ho * Wo * CG;
    // blockDim (256) is a multiple of CG (<= 32), so a thread keeps its channel group across the loop
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    const int cg = threadIdx.x % CG, c = cg * 8;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        size_t p = t / CG;
        int xo = (int)(p % Wo);
        size_t q = p / Wo;
        int yo = (int)(q % Ho), b = (int)(q / Ho);
        bf16x8 g = *reinterpret_cast<const bf16x8*>(dout + p * C + c);
        float v[4][8];
        size_t idx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            idx[k] = (((size_t)b * H + 2 * yo + (k >> 1)) * W + 2 * xo + (k & 1)) * C + c;
            pa_read8(in, idx[k], c, v[k]);
        }
        int arg[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int a = 0; float m = v[0][j];
#pragma unroll
            for (int k = 1; k < 4; ++k) if (v[k][j] > m) { m = v[k][j]; a = k; }
            arg[j] = a;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float e[8], r[8];
            pa_read8(add, idx[k], c, e);
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = (arg[j] == k ? (float)g[j] : 0.f) + e[j];
            *reinterpret_cast<bf16x8*>(din + idx[k]) = epilogue8(ep, idx[k], c, r, s1, s2);
        }
    }
    if (ep.mode != PA_OUT_PLAIN) flush_stats(red, ep.stats, C, c, s1, s2);
}


// maxpool backward, streaming variant (see upadd_bwd_bb_kernel): row r of the pooled map covers input rows 2r, 2r+1.
// INMODE: PLAIN / BNRELU value of the pooled tensor (argmax); HASADD: plain addend; EPMODE: PLAIN or BatchNorm-backward.
template <int INMODE, bool HASADD, int EPMODE>
__global__ __launch_bounds__(1024) void maxpool_bwd_s_kernel(const bf16* __restrict__ dout, PaOperand in, const bf16* __restrict__ add,
                                                             PaEpilogue ep, bf16* __restrict__ din, int rows, int W, int C) {
    PA_SET_ELT_PRIO();
    extern __shared__ float red[];     // [nwaves][2*C] partial statistics, then constants: float4 {scale, shift, mean, invstd} or float2 {k0, k1}
    float4* cst = reinterpret_cast<float4*>(red + (blockDim.x / 64) * 2 * C);
    float2* kin = reinterpret_cast<float2*>(cst + (EPMODE == PA_OUT_BWD ? C : 0));
    if (EPMODE == PA_OUT_BWD) stage_bwd_consts(cst, ep, C);
    if (INMODE == PA_LD_BNRELU)
        for (int i = threadIdx.x; i < C; i += blockDim.x) kin[i] = make_float2(in.k0[i], in.k1[i]);
    __syncthreads();
    const int CG = C / 8, Wo = W / 2;
    const unsigned row_items = (unsigned)Wo * CG;
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    const int c = (threadIdx.x % CG) * 8;
    const unsigned rows_per_it = row_items >= blockDim.x ? 1u : blockDim.x / row_items;
    const unsigned rsub = row_items >= blockDim.x ? 0u : threadIdx.x / row_items;
    const unsigned i0 = row_items >= blockDim.x ? threadIdx.x : threadIdx.x % row_items;
    const bf16* __restrict__ xin = in.p;
    for (unsigned rb = blockIdx.x * rows_per_it; rb < (unsigned)rows; rb += gridDim.x * rows_per_it) {
        const unsigned r = rb + rsub;
        if (r >= (unsigned)rows) continue;
        for (unsigned i = i0; i < row_items; i += blockDim.x) {
            const unsigned xo = i / (unsigned)CG;
            int cc = c;
            asm volatile("" : "+v"(cc));
            const unsigned top = ((2u * r) * (unsigned)W + 2u * xo) * (unsigned)C + (unsigned)c;
            const unsigned wc = (unsigned)W * (unsigned)C;
            const unsigned off[4] = {top, top + (unsigned)C, top + wc, top + wc + (unsigned)C};
            const bf16x8 g = *reinterpret_cast<const bf16x8*>(dout + (r * (unsigned)Wo + xo) * (unsigned)C + (unsigned)c);
            bf16x8 x[4], e[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                x[k] = *reinterpret_cast<const bf16x8*>(xin + off[k]);
                if (HASADD) e[k] = *reinterpret_cast<const bf16x8*>(add + off[k]);
            }
            __builtin_amdgcn_sched_barrier(0);
            float v[4][8];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float t = (float)x[k][j];
                    if (INMODE == PA_LD_BNRELU) { const float2 kk = kin[cc + j]; t = fmaxf(fmaf(kk.x, t, kk.y), 0.f); }
                    v[k][j] = t;
                }
            int arg[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                int a = 0; float m = v[0][j];
#pragma unroll
                for (int k = 1; k < 4; ++k) if (v[k][j] > m) { m = v[k][j]; a = k; }
                arg[j] = a;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float rr[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) rr[j] = (arg[j] == k ? (float)g[j] : 0.f) + (HASADD ? (float)e[k][j] : 0.f);
                bf16x8 o;
                if (EPMODE == PA_OUT_BWD) {
                    o = Bwd8::apply(cst, cc, x[k], rr, s1, s2);      // the tensor being differentiated IS the pooled tensor (launcher checks)
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) o[j] = (bf16)rr[j];
                }
                *reinterpret_cast<bf16x8*>(din + off[k]) = o;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if (EPMODE == PA_OUT_BWD) flush_stats(red, ep.stats, C, c, s1, s2);
}

template <int INMODE, bool HASADD>
static void launch_maxpool_bwd_s(const bf16* dout, const PaOperand& in, const bf16* add, const PaEpilogue& ep, bf16* din, int rows, int W, int C,
                                 const PaEltPlan& p, hipStream_t st) {
    if (ep.mode == PA_OUT_BWD)
        hipLaunchKernelGGL((maxpool_bwd_s_kernel<INMODE, HASADD, PA_OUT_BWD>), dim3(p.blocks), dim3(p.threads), p.lds, st, dout, in, add, ep, din, rows, W, C);
    else
        hipLaunchKernelGGL((maxpool_bwd_s_kernel<INMODE, HASADD, PA_OUT_PLAIN>), dim3(p.blocks), dim3(p.threads), p.lds, st, dout, in, add, ep, din, rows, W, C);
}

// The BatchNorm-backward reductions of maxpool_bwd_s_kernel<PA_LD_BNRELU, false, PA_OUT_BWD> WITHOUT its output, from a quarter of its input: the
// gradient of the pooled tensor and xmax, the raw input value at the arg-max (stored by the forward pool).  The three other positions of a
// window get dz = +0 there, which changes neither sum; with the same grid, thread -> item mapping, loop order and flush_stats tree the
// partial rows are the same bits.  The routed dz itself is formed by its reader (conv1x1_tile.hip, PIN).
__global__ __launch_bounds__(1024) void maxpool_bwd_stats_kernel(const bf16* __restrict__ dout, const bf16* __restrict__ xmax, PaEpilogue ep,
                                                                 int rows, int W, int C) {
    PA_SET_ELT_PRIO();
    extern __shared__ float red[];     // [nwaves][2*C] partial statistics, then float4 {scale, shift, mean, invstd}
    float4* cst = reinterpret_cast<float4*>(red + (blockDim.x / 64) * 2 * C);
    stage_bwd_consts(cst, ep, C);
    __syncthreads();
    const int CG = C / 8, Wo = W / 2;
    const unsigned row_items = (unsigned)Wo * CG;
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    const int c = (threadIdx.x % CG) * 8;
    const unsigned rows_per_it = row_items >= blockDim.x ? 1u : blockDim.x / row_items;
    const unsigned rsub = row_items >= blockDim.x ? 0u : threadIdx.x / row_items;
    const unsigned i0 = row_items >= blockDim.x ? threadIdx.x : threadIdx.x % row_items;
    for (unsigned rb = blockIdx.x * rows_per_it; rb < (unsigned)rows; rb += gridDim.x * rows_per_it) {
        const unsigned r = rb + rsub;
        if (r >= (unsigned)rows) continue;
        for (unsigned i = i0; i < row_items; i += blockDim.x) {
            const unsigned xo = i / (unsigned)CG;
            const unsigned li = (r * (unsigned)Wo + xo) * (unsigned)C + (unsigned)c;
            const bf16x8 g = *reinterpret_cast<const bf16x8*>(dout + li);
            const bf16x8 x = *reinterpret_cast<const bf16x8*>(xmax + li);
            float rr[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) rr[j] = (float)g[j] + 0.f;
            (void)Bwd8::apply(cst, c, x, rr, s1, s2);
        }
    }
    flush_stats(red, ep.stats, C, c, s1, s2);
}

// the plan both launches of a stats-routed pool share: forward (streaming, BatchNorm + ReLU input: it stores xmax) and backward (streaming,
// BatchNorm-backward epilogue on the pooled tensor itself: the partial rows the statistics kernel reproduces)
static bool pool_stats_plan(PaEltPlan& p, const PaOperand& in, const PaEpilogue& ep, int B, int H, int W, int C) {
    if (in.mode != PA_LD_BNRELU || ep.mode != PA_OUT_BWD || ep.xref != in.p || !pa_stats_groups_ok(C)) return false;
    PaEltPlan f;
    if (pa_elt_plan(f, PA_ELT_FWD, (size_t)B * (H / 2) * (W / 2) * (C / 8), B, H, W, C, false, true) || !f.streaming) return false;
    if (pa_elt_plan(p, PA_ELT_POOL_BWD, (size_t)B * (H / 2) * (W / 2) * (C / 8), B, H, W, C, true, true) || !p.streaming) return false;
    return true;
}
bool pa_pool_stats_route_supported(const PaOperand& in, const PaEpilogue& ep, int B, int H, int W, int C) {
    PaEltPlan p;
    return pool_stats_plan(p, in, ep, B, H, W, C);
}
int pa_launch_maxpool_bwd_stats(const bf16* dout, const bf16* xmax, const PaOperand& in, const PaEpilogue& ep, int B, int H, int W, int C,
                                hipStream_t st, int* stat_rows) {
    PaEltPlan p;
    if (!pool_stats_plan(p, in, ep, B, H, W, C)) { pa_set_error_msg("pa_launch_maxpool_bwd_stats: not a pool pa_pool_stats_route_supported() admits"); return 1; }
    if (stat_rows) *stat_rows = p.blocks;
    if (ep.rows_out) *ep.rows_out = p.blocks;
    hipLaunchKernelGGL(maxpool_bwd_stats_kernel, dim3(p.blocks), dim3(p.threads), p.lds, st, dout, xmax, ep, B * (H / 2), W, C);
    return (int)hipGetLastError();
}

int pa_launch_maxpool_bwd(const bf16* dout, const PaOperand& in, const PaOperand& add, const PaEpilogue& ep, bf16* din,
                          int B, int H, int W, int C, hipStream_t st, int* stat_rows) {
    const bool in_ok = in.mode == PA_LD_PLAIN || in.mode == PA_LD_BNRELU;
    const bool add_ok = add.mode == PA_LD_NONE || add.mode == PA_LD_PLAIN;
    // BatchNorm-backward epilogue: only when it refers to the pooled tensor itself (its raw values are already in registers)
    const bool ep_ok = ep.mode == PA_OUT_PLAIN || (ep.mode == PA_OUT_BWD && ep.xref == in.p);
    PaEltPlan p;
    if (pa_elt_plan(p, PA_ELT_POOL_BWD, (size_t)B * (H / 2) * (W / 2) * (C / 8), B, H, W, C, ep.mode != PA_OUT_PLAIN, in_ok && add_ok && ep_ok)) return 1;
    if (stat_rows) *stat_rows = p.blocks;
    if (ep.rows_out) *ep.rows_out = p.blocks;
    if (!p.streaming) {
        hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(p.blocks), dim3(p.threads), p.lds, st, dout, in, add, ep, din, B, H, W, C);
        return (int)hipGetLastError();
    }
    const int rows = B * (H / 2);
    const bool has_add = add.mode == PA_LD_PLAIN;
    if (in.mode == PA_LD_BNRELU) {
        if (has_add) launch_maxpool_bwd_s<PA_LD_BNRELU, true>(dout, in, add.p, ep, din, rows, W, C, p, st);
        else launch_maxpool_bwd_s<PA_LD_BNRELU, false>(dout, in, nullptr, ep, din, rows, W, C, p, st);
    } else {
        if (has_add) launch_maxpool_bwd_s<PA_LD_PLAIN, true>(dout, in, add.p, ep, din, rows, W, C, p, st);
        else launch_maxpool_bwd_s<PA_LD_PLAIN, false>(dout, in, nullptr, ep, din, rows, W, C, p, st);
    }
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
int pa_launch_upadd_fwd(const PaOperand& low, const PaOperand& skip, bf16* out, int B, int H, int W, int C, hipStream_t st) {
    return launch_pool_up_fwd<1>(low, skip, out, B, H, W, C, st);
}

// backward: dskip = epilogue_skip(dout), dlow = epilogue_low(sum of the 2x2 dout block)
__global__ __launch_bounds__(1024) void upadd_bwd_kernel(const bf16* dout, PaEpilogue epl, bf16* dlow, PaEpilogue eps, bf16* dskip,
                                 int B, int H, int W, int C) {
    extern __shared__ float red[];     // [nwaves][2*C]
    const int CG = C / 8, Hl = H / 2, Wl = W / 2;
    float l1[8], l2[8], k1[8], k2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { l1[j] = l2[j] = k1[j] = k2[j] = 0.f; }
    const int cg = threadIdx.x % CG, c = cg * 8;
    const size_t total = (size_t)B * Hl * Wl * CG;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        size_t p = t / CG;
        int xl = (int)(p % Wl);
        size_t q = p / Wl;
        int yl = (int)(q % Hl), b = (int)(q / Hl);
        float sum[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) sum[j] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            size_t idx = (((size_t)b * H + 2 * yl + (k >> 1)) * W + 2 * xl + (k & 1)) * C + c;
            bf16x8 g = *reinterpret_cast<const bf16x8*>(dout + idx);
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { v[j] = (float)g[j]; sum[j] += v[j]; }
            *reinterpret_cast<bf16x8*>(dskip + idx) = epilogue8(eps, idx, c, v, k1, k2);
        }
        size_t li = p * C + c;
        *reinterpret_cast<bf16x8*>(dlow + li) = epilogue8(epl, li, c, sum, l1, l2);
    }
    if (epl.mode != PA_OUT_PLAIN) flush_stats(red, epl.stats, C, c, l1, l2);
    if (eps.mode != PA_OUT_PLAIN) flush_stats(red, eps.stats, C, c, k1, k2);
}


// ---- streaming variants for the hot configurations (both epilogues BatchNorm-backward).  Measured COLD (operands not in
// the Infinity Cache, tools/bench_cold.py) the generic kernels above move 1.7-2.1 TB/s: runtime mode branches, 56 scratch
// accesses and per-use loads of the per-channel constants serialise their loads.  Here the modes are template parameters,
// the per-channel constants sit in LDS as float4 {scale, shift, mean, invstd}, and ALL loads of an item (9 x 16 bytes) are
// issued before the first use, so that a 1024-thread workgroup keeps ~150 KB in flight.
// LOW / SKIP: which of the two outputs this launch produces.  Both: the one-launch form.  One each: the hourglass' backward pass needs dlow on
// its main chain (the low-resolution path below) and dskip only on the side stream that runs the skip block's backward pass -- the main
// chain then waits for 75 MB of traffic instead of 175 (round 6)
template <bool LOW, bool SKIP>
__global__ __launch_bounds__(1024) void upadd_bwd_bb_kernel(const bf16* __restrict__ dout, PaEpilogue epl, bf16* __restrict__ dlow,
                                                            PaEpilogue eps, bf16* __restrict__ dskip, int rows, int W, int C) {
    PA_SET_ELT_PRIO();
    // rows = B * H/2 low-resolution rows; row r covers high-resolution rows 2r, 2r+1 (H = 2*Hl: no batch/row split needed).
    // blockDim is a multiple of the items of a row (Wl * C/8) or the other way round (launcher): no per-iteration division.
    extern __shared__ float red[];     // [nwaves][2*C] partial statistics, then the two constant tables
    float4* cl = reinterpret_cast<float4*>(red + (blockDim.x / 64) * 2 * C);
    float4* cs = cl + C;
    if (LOW) stage_bwd_consts(cl, epl, C);
    if (SKIP) stage_bwd_consts(cs, eps, C);
    __syncthreads();
    const int CG = C / 8, Wl = W / 2;
    const unsigned row_items = (unsigned)Wl * CG;
    float l1[8], l2[8], k1[8], k2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { l1[j] = l2[j] = k1[j] = k2[j] = 0.f; }
    const int c = (threadIdx.x % CG) * 8;
    const unsigned rows_per_it = row_items >= blockDim.x ? 1u : blockDim.x / row_items;
    const unsigned rsub = row_items >= blockDim.x ? 0u : threadIdx.x / row_items;
    const unsigned i0 = row_items >= blockDim.x ? threadIdx.x : threadIdx.x % row_items;
    const bf16* __restrict__ xsk = eps.xref;
    const bf16* __restrict__ xlo = epl.xref;
    for (unsigned rb = blockIdx.x * rows_per_it; rb < (unsigned)rows; rb += gridDim.x * rows_per_it) {
        const unsigned r = rb + rsub;
        if (r >= (unsigned)rows) continue;
        for (unsigned i = i0; i < row_items; i += blockDim.x) {
            const unsigned xl = i / (unsigned)CG;
            int cc = c;
            asm volatile("" : "+v"(cc));      // opaque per iteration: the constant tables stay in LDS (hoisted they are 64 registers)
            const unsigned top = ((2u * r) * (unsigned)W + 2u * xl) * (unsigned)C + (unsigned)c;
            const unsigned wc = (unsigned)W * (unsigned)C;
            const unsigned off[4] = {top, top + (unsigned)C, top + wc, top + wc + (unsigned)C};
            const unsigned li = (r * (unsigned)Wl + xl) * (unsigned)C + (unsigned)c;
            bf16x8 g[4], xs[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                g[k] = *reinterpret_cast<const bf16x8*>(dout + off[k]);
                if (SKIP) xs[k] = *reinterpret_cast<const bf16x8*>(xsk + off[k]);
            }
            bf16x8 xlow;
            if (LOW) xlow = *reinterpret_cast<const bf16x8*>(xlo + li);
            __builtin_amdgcn_sched_barrier(0);        // all nine loads are issued; the constant reads below stay next to their use
            float sum[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) sum[j] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) { v[j] = (float)g[k][j]; sum[j] += v[j]; }
                if (SKIP) {
                    *reinterpret_cast<bf16x8*>(dskip + off[k]) = Bwd8::apply(cs, cc, xs[k], v, k1, k2);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (LOW) *reinterpret_cast<bf16x8*>(dlow + li) = Bwd8::apply(cl, cc, xlow, sum, l1, l2);
        }
    }
    if (LOW) flush_stats(red, epl.stats, C, c, l1, l2);
    if (SKIP) flush_stats(red, eps.stats, C, c, k1, k2);
}

// the one plan of an upsample-add backward: pa_upadd_bwd_splits and the launch read the same answer
static int upadd_bwd_plan(PaEltPlan& p, const PaEpilogue& ep_low, const PaEpilogue& ep_skip, int B, int H, int W, int C) {
    return pa_elt_plan(p, PA_ELT_UPADD_BWD, (size_t)B * (H / 2) * (W / 2) * (C / 8), B, H, W, C, ep_low.mode != PA_OUT_PLAIN || ep_skip.mode != PA_OUT_PLAIN,
                       ep_low.mode == PA_OUT_BWD && ep_skip.mode == PA_OUT_BWD);
}

bool pa_upadd_bwd_splits(const PaEpilogue& ep_low, const PaEpilogue& ep_skip, int B, int H, int W, int C) {
    PaEltPlan p;
    return upadd_bwd_plan(p, ep_low, ep_skip, B, H, W, C) == 0 && p.streaming;
}

int pa_launch_upadd_bwd(const bf16* dout, const PaEpilogue& ep_low, bf16* dlow, const PaEpilogue& ep_skip, bf16* dskip,
                        int B, int H, int W, int C, hipStream_t st, int* stat_rows, int part) {
    PaEltPlan p;
    if (upadd_bwd_plan(p, ep_low, ep_skip, B, H, W, C)) return 1;
    // one output only: the streaming kernel or nothing (callers ask pa_upadd_bwd_splits first)
    if (part != 3 && (!p.streaming || (part != 1 && part != 2))) { pa_set_error_msg("pa_launch_upadd_bwd: this launch cannot be split"); return 1; }
    if (stat_rows) *stat_rows = p.blocks;
    if (ep_low.rows_out && (part & 1)) *ep_low.rows_out = p.blocks;
    if (ep_skip.rows_out && (part & 2)) *ep_skip.rows_out = p.blocks;
    const dim3 grid(p.blocks), block(p.threads);
    const int rows = B * (H / 2);
    if (!p.streaming) hipLaunchKernelGGL(upadd_bwd_kernel, grid, block, p.lds, st, dout, ep_low, dlow, ep_skip, dskip, B, H, W, C);
    else if (part == 1) hipLaunchKernelGGL((upadd_bwd_bb_kernel<true, false>), grid, block, p.lds, st, dout, ep_low, dlow, ep_skip, dskip, rows, W, C);
    else if (part == 2) hipLaunchKernelGGL((upadd_bwd_bb_kernel<false, true>), grid, block, p.lds, st, dout, ep_low, dlow, ep_skip, dskip, rows, W, C);
    else hipLaunchKernelGGL((upadd_bwd_bb_kernel<true, true>), grid, block, p.lds, st, dout, ep_low, dlow, ep_skip, dskip, rows, W, C);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// RMSprop exactly as torch.optim.RMSprop(alpha, eps, momentum=0, weight_decay=0, centered=False)
// (reference stack-hg.py:51-52): v = alpha v + (1-alpha) g^2 ; p -= lr g / (sqrt(v) + eps).
// gscale multiplies the gradient first (1/world_size after a sum all-reduce).
// the update, once for the vector body and the tail of both kernels: v' = alpha v + (1 - alpha) g^2, then p' = p - lr g / (sqrt(v') + eps)
__device__ __forceinline__ float rmsprop_v(float v, float gr, float alpha) { return alpha * v + (1.f - alpha) * gr * gr; }
__device__ __forceinline__ float rmsprop_p(float p, float v, float gr, float lr, float eps) { return p - lr * (gr / (sqrtf(v) + eps)); }
__global__ void rmsprop_kernel(float* p, const float* g, float* v, size_t n, float lr, float alpha, float eps, float gscale) {
    size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
    for (; i + 3 < n; i += stride) {
        f32x4 gg = *reinterpret_cast<const f32x4*>(g + i), vv = *reinterpret_cast<f32x4*>(v + i), pp = *reinterpret_cast<f32x4*>(p + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gr = gg[j] * gscale;
            vv[j] = rmsprop_v(vv[j], gr, alpha);
            pp[j] = rmsprop_p(pp[j], vv[j], gr, lr, eps);
        }
        *reinterpret_cast<f32x4*>(v + i) = vv;
        *reinterpret_cast<f32x4*>(p + i) = pp;
    }
    for (; i < n && i + 3 >= n; ++i) {          // tail (at most 3 elements, one thread)
        const float gr = g[i] * gscale;
        v[i] = rmsprop_v(v[i], gr, alpha);
        p[i] = rmsprop_p(p[i], v[i], gr, lr, eps);
    }
}

// Half-precision build only (gradients travel multiplied by PA_GRAD_SCALE, common.h): an overflow anywhere in the backward
// pass shows up as inf / NaN in the flat gradient.  A step whose gradient holds a non-finite value is SKIPPED (parameters and
// square_avg untouched, the loss-scaling convention) and counted; pa_rmsprop_skipped_steps reads the counter.
// The two state words belong to ONE optimizer: the caller passes its own device pair (pa_rmsprop_step_state), so that two optimizers
// stepping on different streams (pose net and agent in the joint stage) cannot see each other's flag; the process-wide pair below
// only serves the stateless entry point pa_rmsprop_step.
__device__ int g_grad_state[2];            // [0] this step's gradient holds a non-finite value, [1] steps skipped so far

__global__ void grad_check_reset_kernel(int* state) { (state ? state : g_grad_state)[0] = 0; }

__global__ void grad_check_kernel(const float* g, size_t n, int* state) {
    size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
    bool bad = false;
    for (; i + 3 < n; i += stride) {
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + i);
        bad |= !(isfinite(gg[0]) && isfinite(gg[1]) && isfinite(gg[2]) && isfinite(gg[3]));
    }
    for (; i < n && i + 3 >= n; ++i) bad |= !isfinite(g[i]);
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&(state ? state : g_grad_state)[0], 1);
}

__global__ void rmsprop_checked_kernel(float* p, const float* g, float* v, size_t n, float lr, float alpha, float eps, float gscale, int* state) {
    int* gs = state ? state : g_grad_state;
    if (gs[0]) {                            // uniform over the grid: every thread reads the same word
        if (blockIdx.x == 0 && threadIdx.x == 0) gs[1] += 1;
        return;
    }
    size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
    for (; i + 3 < n; i += stride) {
        f32x4 gg = *reinterpret_cast<const f32x4*>(g + i), vv = *reinterpret_cast<f32x4*>(v + i), pp = *reinterpret_cast<f32x4*>(p + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gr = gg[j] * gscale;
            vv[j] = rmsprop_v(vv[j], gr, alpha);
            pp[j] = rmsprop_p(pp[j], vv[j], gr, lr, eps);
        }
        *reinterpret_cast<f32x4*>(v + i) = vv;
        *reinterpret_cast<f32x4*>(p + i) = pp;
    }
    for (; i < n && i + 3 >= n; ++i) {
        const float gr = g[i] * gscale;
        v[i] = rmsprop_v(v[i], gr, alpha);
        p[i] = rmsprop_p(p[i], v[i], gr, lr, eps);
    }
}

int pa_launch_rmsprop(float* p, const float* g, float* v, size_t n, float lr, float alpha, float eps, float gscale, int* state, hipStream_t st) {
    if (n == 0) return 0;
    const int blocks = pa_grid_for(n / 4, 256, 2048);
#ifdef PA_FP16
    hipLaunchKernelGGL(grad_check_reset_kernel, dim3(1), dim3(1), 0, st, state);
    hipLaunchKernelGGL(grad_check_kernel, dim3(blocks), dim3(256), 0, st, g, n, state);
    hipLaunchKernelGGL(rmsprop_checked_kernel, dim3(blocks), dim3(256), 0, st, p, g, v, n, lr, alpha, eps, gscale, state);
#else
    (void)state;
    hipLaunchKernelGGL(rmsprop_kernel, dim3(blocks), dim3(256), 0, st, p, g, v, n, lr, alpha, eps, gscale);
#endif
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// The other options of torch.optim.RMSprop (momentum, centered, weight_decay: torch 2.10 _single_tensor_rmsprop) and the coefficient
// of torch.nn.utils.clip_grad_norm_, beside the kernels above (the reference itself trains with all of them off, stack-hg.py:51-52).
// Per element, every operation in fp32 and in this order:
//   gr  = (g * gscale) * coef            coef: ONE device float (pa_launch_grad_norm's out[1]); no multiply without a clip pointer
//   gr  = gr + wd * p                    only when wd != 0 (a "+ 0 * p" would already turn -0 into +0)
//   v'  = rmsprop_v(v, gr, alpha)
//   ga' = alpha ga + (1 - alpha) gr      centered
//   den = sqrtf(centered ? fmaxf(0, v' - ga' ga') : v') + eps
//   momentum > 0:  buf' = mom buf + gr / den ;  p' = p - lr buf'          else  p' = p - lr (gr / den)  (rmsprop_p when not centered)
// fmaxf(0, .) is the ONE deliberate difference from torch: v' - ga'^2 is >= 0 in exact arithmetic (a weighted mean of squares against
// the square of the same weighted mean), rounding can make it slightly negative, and torch then takes the root of it and returns NaN.
// The alignment padding of a flat array (p = g = v = buf = ga = 0) stays exactly 0: every term above is then 0 and den = eps > 0.
// Half-precision build: `state` is the optimizer's {flag, skipped} pair behind the same reset + grad_check_kernel scan as above; a
// skipped step leaves p, v, buf and ga untouched.
template <bool MOMENTUM, bool CENTERED>
__device__ __forceinline__ void rmsprop_opts_update(float& p, float g, float& v, float& buf, float& ga, const PaRmspropOpts& o, float gscale,
                                                    bool clip, float coef) {
    float gr = g * gscale;
    if (clip) gr = gr * coef;
    if (o.wd != 0.f) gr = gr + o.wd * p;
    v = rmsprop_v(v, gr, o.alpha);
    if (!MOMENTUM && !CENTERED) { p = rmsprop_p(p, v, gr, o.lr, o.eps); return; }
    float den;
    if (CENTERED) {
        ga = o.alpha * ga + (1.f - o.alpha) * gr;
        den = sqrtf(fmaxf(0.f, v - ga * ga)) + o.eps;
    } else {
        den = sqrtf(v) + o.eps;
    }
    if (MOMENTUM) {
        buf = o.mom * buf + gr / den;
        p = p - o.lr * buf;
    } else {
        p = p - o.lr * (gr / den);
    }
}

template <bool MOMENTUM, bool CENTERED>
__global__ void rmsprop_opts_kernel(float* p, const float* g, float* v, float* buf, float* ga, size_t n, PaRmspropOpts o, float gscale,
                                    const float* clip_coef, int* state) {
#ifdef PA_FP16
    if (state[0]) {                         // uniform over the grid: every thread reads the same word
        if (blockIdx.x == 0 && threadIdx.x == 0) state[1] += 1;
        return;
    }
#endif
    const bool clip = clip_coef != nullptr;
    const float coef = clip ? clip_coef[0] : 1.f;
    size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
    for (; i + 3 < n; i += stride) {
        f32x4 gg = *reinterpret_cast<const f32x4*>(g + i), vv = *reinterpret_cast<f32x4*>(v + i), pp = *reinterpret_cast<f32x4*>(p + i);
        f32x4 bb = {0.f, 0.f, 0.f, 0.f}, aa = {0.f, 0.f, 0.f, 0.f};
        if (MOMENTUM) bb = *reinterpret_cast<f32x4*>(buf + i);
        if (CENTERED) aa = *reinterpret_cast<f32x4*>(ga + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = pp[j], vj = vv[j], bj = bb[j], aj = aa[j];
            rmsprop_opts_update<MOMENTUM, CENTERED>(pj, gg[j], vj, bj, aj, o, gscale, clip, coef);
            pp[j] = pj; vv[j] = vj; bb[j] = bj; aa[j] = aj;
        }
        *reinterpret_cast<f32x4*>(v + i) = vv;
        *reinterpret_cast<f32x4*>(p + i) = pp;
        if (MOMENTUM) *reinterpret_cast<f32x4*>(buf + i) = bb;
        if (CENTERED) *reinterpret_cast<f32x4*>(ga + i) = aa;
    }
    for (; i < n && i + 3 >= n; ++i) {          // tail (at most 3 elements, one thread)
        float pj = p[i], vj = v[i], bj = MOMENTUM ? buf[i] : 0.f, aj = CENTERED ? ga[i] : 0.f;
        rmsprop_opts_update<MOMENTUM, CENTERED>(pj, g[i], vj, bj, aj, o, gscale, clip, coef);
        p[i] = pj; v[i] = vj;
        if (MOMENTUM) buf[i] = bj;
        if (CENTERED) ga[i] = aj;
    }
}

// buf is used iff o.mom > 0, ga iff centered (the C ABI checks that the pointers match).  With every option off and no clip pointer
// this IS pa_launch_rmsprop: the same launch, hence the same bits.
int pa_launch_rmsprop_opts(const PaRmspropOpts& o, bool centered, float* p, const float* g, float* v, float* buf, float* ga, size_t n,
                           float gscale, const float* clip_coef, int* state, hipStream_t st) {
    if (n == 0) return 0;
    const bool mom = o.mom > 0.f;
    if (!mom && !centered && o.wd == 0.f && !clip_coef) return pa_launch_rmsprop(p, g, v, n, o.lr, o.alpha, o.eps, gscale, state, st);
    const int blocks = pa_grid_for(n / 4, 256, 2048);
#ifdef PA_FP16
    hipLaunchKernelGGL(grad_check_reset_kernel, dim3(1), dim3(1), 0, st, state);
    hipLaunchKernelGGL(grad_check_kernel, dim3(blocks), dim3(256), 0, st, g, n, state);
#endif
    const dim3 grid(blocks), block(256);
    if (mom && centered) hipLaunchKernelGGL((rmsprop_opts_kernel<true, true>), grid, block, 0, st, p, g, v, buf, ga, n, o, gscale, clip_coef, state);
    else if (mom) hipLaunchKernelGGL((rmsprop_opts_kernel<true, false>), grid, block, 0, st, p, g, v, buf, ga, n, o, gscale, clip_coef, state);
    else if (centered) hipLaunchKernelGGL((rmsprop_opts_kernel<false, true>), grid, block, 0, st, p, g, v, buf, ga, n, o, gscale, clip_coef, state);
    else hipLaunchKernelGGL((rmsprop_opts_kernel<false, false>), grid, block, 0, st, p, g, v, buf, ga, n, o, gscale, clip_coef, state);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// torch.optim.Adam / AdamW with AMSGrad (torch 2.10 _single_tensor_adam, non-capturable branch), in the shape of the kernels above.
// Per element, every operation in fp32 and in this order:
//   gr  = (g * gscale) * coef            coef as above; no multiply without a clip pointer
//   DECAY 1 (coupled):    gr = gr + wd * p          DECAY 2 (decoupled):  p = p * c_dec,  c_dec = (float)(1.0 - (double)lr * (double)wd)
//   m'  = m + (gr - m) * (1.f - beta1)              (torch's lerp_ with a weight < 0.5)
//   v'  = beta2 * v + ((1.f - beta2) * gr) * gr
//   vmax' = fmaxf(vmax, v')                         AMSGRAD; vhat = AMSGRAD ? vmax' : v'
//   den = sqrtf(vhat) / bc2s + eps ;  p' = p - step_size * (m' / den)
// DECAY 0 computes neither decay (a "+ 0 * p" would turn -0 into +0, see rmsprop_opts_update); AMSGRAD off loads and stores no vmax.
// bc1 = (float)(1.0 - pow((double)beta1, (double)t)), bc2 likewise, bc2s = sqrtf(bc2), step_size = lr / bc1, t = steps TAKEN including
// this one: t lives in the optimizer's device state (PaAdamState), because the half-precision build decides on the device whether the
// step is taken.  adam_prologue_kernel (one thread) advances it and writes the constants, or counts a skipped step; the step kernel
// reads flag, bc2s and step_size, uniform over the grid, and returns at once when the flag is set.
// The alignment padding of a flat array (p = g = m = v = vmax = 0) stays exactly 0: every term is 0, den = eps > 0, the decoupled
// decay multiplies 0.
__global__ void adam_prologue_kernel(PaAdamState* s, float lr, float beta1, float beta2) {
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

__global__ void adam_set_steps_kernel(PaAdamState* s, int steps) { s->step = steps; }

template <bool AMSGRAD, int DECAY>
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float& vmax, const PaAdamOpts& o, float gscale,
                                            bool clip, float coef, float bc2s, float step_size) {
    float gr = g * gscale;
    if (clip) gr = gr * coef;
    if (DECAY == 1) gr = gr + o.wd * p;
    if (DECAY == 2) p = p * o.c_dec;
    m = m + (gr - m) * o.om_b1;
    v = o.beta2 * v + (o.om_b2 * gr) * gr;
    float vhat = v;
    if (AMSGRAD) { vmax = fmaxf(vmax, v); vhat = vmax; }
    const float den = sqrtf(vhat) / bc2s + o.eps;
    p = p - step_size * (m / den);
}

template <bool AMSGRAD, int DECAY>
__global__ void adam_kernel(float* p, const float* g, float* m, float* v, float* vmax, size_t n, PaAdamOpts o, float gscale,
                            const float* clip_coef, const PaAdamState* state) {
    if (state->flag) return;                // uniform over the grid: every thread reads the same word (the prologue has counted the skip)
    const float bc2s = state->bc2s, step_size = state->step_size;
    const bool clip = clip_coef != nullptr;
    const float coef = clip ? clip_coef[0] : 1.f;
    size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
    for (; i + 3 < n; i += stride) {
        f32x4 gg = *reinterpret_cast<const f32x4*>(g + i), mm = *reinterpret_cast<f32x4*>(m + i), vv = *reinterpret_cast<f32x4*>(v + i),
              pp = *reinterpret_cast<f32x4*>(p + i);
        f32x4 xx = {0.f, 0.f, 0.f, 0.f};
        if (AMSGRAD) xx = *reinterpret_cast<f32x4*>(vmax + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = pp[j], mj = mm[j], vj = vv[j], xj = xx[j];
            adam_update<AMSGRAD, DECAY>(pj, gg[j], mj, vj, xj, o, gscale, clip, coef, bc2s, step_size);
            pp[j] = pj; mm[j] = mj; vv[j] = vj; xx[j] = xj;
        }
        *reinterpret_cast<f32x4*>(m + i) = mm;
        *reinterpret_cast<f32x4*>(v + i) = vv;
        *reinterpret_cast<f32x4*>(p + i) = pp;
        if (AMSGRAD) *reinterpret_cast<f32x4*>(vmax + i) = xx;
    }
    for (; i < n && i + 3 >= n; ++i) {          // tail (at most 3 elements, one thread)
        float pj = p[i], mj = m[i], vj = v[i], xj = AMSGRAD ? vmax[i] : 0.f;
        adam_update<AMSGRAD, DECAY>(pj, g[i], mj, vj, xj, o, gscale, clip, coef, bc2s, step_size);
        p[i] = pj; m[i] = mj; v[i] = vj;
        if (AMSGRAD) vmax[i] = xj;
    }
}

template <bool AMSGRAD>
static void adam_launch_decay(int decay, dim3 grid, dim3 block, hipStream_t st, float* p, const float* g, float* m, float* v, float* vmax,
                              size_t n, const PaAdamOpts& o, float gscale, const float* clip_coef, const PaAdamState* state) {
    if (decay == 1) hipLaunchKernelGGL((adam_kernel<AMSGRAD, 1>), grid, block, 0, st, p, g, m, v, vmax, n, o, gscale, clip_coef, state);
    else if (decay == 2) hipLaunchKernelGGL((adam_kernel<AMSGRAD, 2>), grid, block, 0, st, p, g, m, v, vmax, n, o, gscale, clip_coef, state);
    else hipLaunchKernelGGL((adam_kernel<AMSGRAD, 0>), grid, block, 0, st, p, g, m, v, vmax, n, o, gscale, clip_coef, state);
}

// vmax is used iff amsgrad (the C ABI checks that the pointer matches).  bf16 build: prologue -> step (the flag is never set);
// half-precision build: the reset + grad_check_kernel scan of the RMSprop steps in front, on the state's first two words.
int pa_launch_adam(const PaAdamOpts& o, bool amsgrad, int decay, float* p, const float* g, float* m, float* v, float* vmax, size_t n,
                   float gscale, const float* clip_coef, PaAdamState* state, hipStream_t st) {
    if (n == 0) return 0;
    const int blocks = pa_grid_for(n / 4, 256, 2048);
#ifdef PA_FP16
    hipLaunchKernelGGL(grad_check_reset_kernel, dim3(1), dim3(1), 0, st, &state->flag);
    hipLaunchKernelGGL(grad_check_kernel, dim3(blocks), dim3(256), 0, st, g, n, &state->flag);
#endif
    hipLaunchKernelGGL(adam_prologue_kernel, dim3(1), dim3(1), 0, st, state, o.lr, o.beta1, o.beta2);
    const dim3 grid(blocks), block(256);
    if (amsgrad) adam_launch_decay<true>(decay, grid, block, st, p, g, m, v, vmax, n, o, gscale, clip_coef, state);
    else adam_launch_decay<false>(decay, grid, block, st, p, g, m, v, vmax, n, o, gscale, clip_coef, state);
    return (int)hipGetLastError();
}

int pa_adam_read_steps(const PaAdamState* state, long long* steps, long long* skipped, hipStream_t st) {
    PaAdamState h;
    hipError_t e = hipMemcpyAsync(&h, state, sizeof h, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    if (steps) *steps = h.step;
    if (skipped) *skipped = h.skipped;
    return 0;
}

int pa_launch_adam_set_steps(PaAdamState* state, int steps, hipStream_t st) {
    hipLaunchKernelGGL(adam_set_steps_kernel, dim3(1), dim3(1), 0, st, state, steps);
    return (int)hipGetLastError();
}

// Norm of gscale * g and the clip coefficient, in two launches, without floating-point atomics: the same inputs give the same bits.
//   1. grad_sqsum_kernel: every workgroup of the capped grid sums ((double)g[i] * (double)gscale)^2 over its grid-stride share in
//      double (the product of two fp32 values is exact in double) and writes ONE partial;
//   2. grad_norm_finish_kernel: one workgroup adds the partials in a fixed order, out[0] = (float)sqrt(sum), and
//      out[1] = fminf(1, max_norm / (out[0] + 1e-6f)) in fp32: the coefficient of torch.nn.utils.clip_grad_norm_.
// The step kernel reads out[1] on the device: no host synchronisation.
__device__ __forceinline__ double block_sum_double(double s, double* lds) {     // 256 threads; the result is valid in thread 0
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__global__ __launch_bounds__(256) void grad_sqsum_kernel(const float* g, size_t n, float gscale, double* partial) {
    __shared__ double lds[4];
    const double sc = (double)gscale;
    size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * 256 * 4;
    double s = 0.0;
    for (; i + 3 < n; i += stride) {
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) { const double t = (double)gg[j] * sc; s += t * t; }
    }
    for (; i < n && i + 3 >= n; ++i) { const double t = (double)g[i] * sc; s += t * t; }
    s = block_sum_double(s, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* partial, int nparts, float max_norm, float* out) {
    __shared__ double lds[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += partial[i];
    s = block_sum_double(s, lds);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        out[0] = norm;
        out[1] = fminf(1.f, max_norm / (norm + 1e-6f));
    }
}

size_t pa_grad_norm_workspace_size(size_t n) { return (size_t)pa_grid_for(n / 4, 256, 2048) * sizeof(double); }

int pa_launch_grad_norm(const float* g, size_t n, float gscale, float max_norm, void* workspace, float* out2, hipStream_t st) {
    const int blocks = pa_grid_for(n / 4, 256, 2048);
    double* partial = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(grad_sqsum_kernel, dim3(blocks), dim3(256), 0, st, g, n, gscale, partial);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, partial, blocks, max_norm, out2);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Parameter groups: per-group lr / weight_decay / frozen in the fused steps and the norm above.
// Every tensor of a flat array starts on a 16-byte boundary (Net::add_param) and the step kernels move one 16-byte chunk per thread
// and iteration, so the group is a property of the CHUNK: chunk_map[i / 4] (one byte, 0 .. 15) is the group of elements 4 (i / 4) ..
// 4 (i / 4) + 3, and the tail (at most 3 elements) reads chunk_map[n / 4].  The table of at most 16 {lr, wd, c_dec, frozen} entries
// comes by value in the kernel arguments (256 bytes); thread 0 of every workgroup copies it to LDS with constant indices (scalar
// loads of the argument segment), and a lane then reads its chunk's entry with one 16-byte LDS load: a per-lane index into the
// argument itself would send the table through scratch memory.  Entries at and above ngroups are marked frozen by the host, so a map
// byte out of range (masked to 4 bits) skips its chunk instead of reading anything undefined.
// The per-element arithmetic is rmsprop_opts_update<> / adam_update<> above, with the chunk's lr and wd (Adam: c_dec and step_size)
// in place of the optimizer's.  The decay mode is per chunk: wd == 0 executes no decay operation (rmsprop_opts_update tests o.wd at
// run time already; Adam picks DECAY 0), otherwise coupled or decoupled as the optimizer says.  A FROZEN chunk is skipped before any
// load: nothing of param, grad or the state arrays is read or written.  Alignment padding stays exactly 0 in every group by the
// argument above (p = g = state = 0; every term is 0 whatever lr and wd are) or is not touched at all.
// Half-precision build: the finite scan stays over the WHOLE gradient, frozen chunks included.  An overflow anywhere in the scaled
// backward pass has already propagated into the layers below it, and the scan is the only evidence of that: the whole step is skipped
// and counted once, as without groups.  No atomics in these kernels: the same input gives the same bits.
__device__ __forceinline__ void opt_groups_stage(const PaOptGroupTable& tab, PaOptGroupK* lds) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < PA_OPT_GROUPS; ++k) lds[k] = tab.g[k];
    }
}

template <bool MOMENTUM, bool CENTERED>
__global__ __launch_bounds__(256) void rmsprop_groups_kernel(float* p, const float* g, float* v, float* buf, float* ga, size_t n, PaRmspropOpts o,
                                                             PaOptGroupTable tab, const unsigned char* __restrict__ map, float gscale,
                                                             const float* clip_coef, int* state) {
    __shared__ PaOptGroupK s_tab[PA_OPT_GROUPS];
#ifdef PA_FP16
    if (state[0]) {                         // uniform over the grid: every thread reads the same word
        if (blockIdx.x == 0 && threadIdx.x == 0) state[1] += 1;
        return;
    }
#endif
    opt_groups_stage(tab, s_tab);
    __syncthreads();
    const bool clip = clip_coef != nullptr;
    const float coef = clip ? clip_coef[0] : 1.f;
    size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
    for (; i + 3 < n; i += stride) {
        const PaOptGroupK gk = s_tab[map[i >> 2] & (PA_OPT_GROUPS - 1)];
        if (gk.frozen) continue;
        PaRmspropOpts og = o;
        og.lr = gk.lr; og.wd = gk.wd;
        f32x4 gg = *reinterpret_cast<const f32x4*>(g + i), vv = *reinterpret_cast<f32x4*>(v + i), pp = *reinterpret_cast<f32x4*>(p + i);
        f32x4 bb = {0.f, 0.f, 0.f, 0.f}, aa = {0.f, 0.f, 0.f, 0.f};
        if (MOMENTUM) bb = *reinterpret_cast<f32x4*>(buf + i);
        if (CENTERED) aa = *reinterpret_cast<f32x4*>(ga + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = pp[j], vj = vv[j], bj = bb[j], aj = aa[j];
            rmsprop_opts_update<MOMENTUM, CENTERED>(pj, gg[j], vj, bj, aj, og, gscale, clip, coef);
            pp[j] = pj; vv[j] = vj; bb[j] = bj; aa[j] = aj;
        }
        *reinterpret_cast<f32x4*>(v + i) = vv;
        *reinterpret_cast<f32x4*>(p + i) = pp;
        if (MOMENTUM) *reinterpret_cast<f32x4*>(buf + i) = bb;
        if (CENTERED) *reinterpret_cast<f32x4*>(ga + i) = aa;
    }
    if (i < n && i + 3 >= n) {                  // tail (at most 3 elements, one thread): the group of chunk n / 4
        const PaOptGroupK gk = s_tab[map[n >> 2] & (PA_OPT_GROUPS - 1)];
        if (gk.frozen) return;
        PaRmspropOpts og = o;
        og.lr = gk.lr; og.wd = gk.wd;
        for (; i < n; ++i) {
            float pj = p[i], vj = v[i], bj = MOMENTUM ? buf[i] : 0.f, aj = CENTERED ? ga[i] : 0.f;
            rmsprop_opts_update<MOMENTUM, CENTERED>(pj, g[i], vj, bj, aj, og, gscale, clip, coef);
            p[i] = pj; v[i] = vj;
            if (MOMENTUM) buf[i] = bj;
            if (CENTERED) ga[i] = aj;
        }
    }
}

// With ONE group that is not frozen this IS pa_launch_rmsprop_opts with that group's lr and wd: the same launches, hence the same bits.
int pa_launch_rmsprop_groups(const PaRmspropOpts& o, bool centered, const PaOptGroupTable& tab, int ngroups, const unsigned char* map,
                             float* p, const float* g, float* v, float* buf, float* ga, size_t n, float gscale, const float* clip_coef,
                             int* state, hipStream_t st) {
    if (ngroups == 1 && !tab.g[0].frozen) {
        PaRmspropOpts o1 = o;
        o1.lr = tab.g[0].lr; o1.wd = tab.g[0].wd;
        return pa_launch_rmsprop_opts(o1, centered, p, g, v, buf, ga, n, gscale, clip_coef, state, st);
    }
    if (n == 0) return 0;
    const bool mom = o.mom > 0.f;
    const int blocks = pa_grid_for(n / 4, 256, 2048);
#ifdef PA_FP16
    hipLaunchKernelGGL(grad_check_reset_kernel, dim3(1), dim3(1), 0, st, state);
    hipLaunchKernelGGL(grad_check_kernel, dim3(blocks), dim3(256), 0, st, g, n, state);
#endif
    const dim3 grid(blocks), block(256);
    if (mom && centered) hipLaunchKernelGGL((rmsprop_groups_kernel<true, true>), grid, block, 0, st, p, g, v, buf, ga, n, o, tab, map, gscale, clip_coef, state);
    else if (mom) hipLaunchKernelGGL((rmsprop_groups_kernel<true, false>), grid, block, 0, st, p, g, v, buf, ga, n, o, tab, map, gscale, clip_coef, state);
    else if (centered) hipLaunchKernelGGL((rmsprop_groups_kernel<false, true>), grid, block, 0, st, p, g, v, buf, ga, n, o, tab, map, gscale, clip_coef, state);
    else hipLaunchKernelGGL((rmsprop_groups_kernel<false, false>), grid, block, 0, st, p, g, v, buf, ga, n, o, tab, map, gscale, clip_coef, state);
    return (int)hipGetLastError();
}

// adam_prologue_kernel with one step size per group: group_consts[k] = lr_k / bc1 for k < ngroups (the caller's device array of 16
// floats, which the step kernel reads and a test can read back), state->step_size = group_consts[0].  A skipped step leaves both.
__global__ void adam_prologue_groups_kernel(PaAdamState* s, PaOptGroupTable tab, int ngroups, float* group_consts, float beta1, float beta2) {
    if (s->flag) { s->skipped += 1; return; }
    const int t = s->step + 1;
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)t));
    const float bc2 = (float)(1.0 - pow((double)beta2, (double)t));
    s->step = t;
    s->bc1 = bc1;
    s->bc2 = bc2;
    s->bc2s = sqrtf(bc2);
#pragma unroll
    for (int k = 0; k < PA_OPT_GROUPS; ++k)
        if (k < ngroups) group_consts[k] = tab.g[k].lr / bc1;
    s->step_size = tab.g[0].lr / bc1;
}

template <bool AMSGRAD, bool DECOUPLED>
__device__ __forceinline__ void adam_groups_update(float& p, float g, float& m, float& v, float& vmax, const PaAdamOpts& og, float gscale,
                                                   bool clip, float coef, float bc2s, float step_size) {
    if (og.wd != 0.f) adam_update<AMSGRAD, DECOUPLED ? 2 : 1>(p, g, m, v, vmax, og, gscale, clip, coef, bc2s, step_size);
    else adam_update<AMSGRAD, 0>(p, g, m, v, vmax, og, gscale, clip, coef, bc2s, step_size);
}

template <bool AMSGRAD, bool DECOUPLED>
__global__ __launch_bounds__(256) void adam_groups_kernel(float* p, const float* g, float* m, float* v, float* vmax, size_t n, PaAdamOpts o,
                                                          PaOptGroupTable tab, int ngroups, const unsigned char* __restrict__ map,
                                                          const float* __restrict__ group_consts, float gscale, const float* clip_coef,
                                                          const PaAdamState* state) {
    __shared__ PaOptGroupK s_tab[PA_OPT_GROUPS];
    __shared__ float s_step[PA_OPT_GROUPS];
    if (state->flag) return;                // uniform over the grid (the prologue has counted the skip)
    opt_groups_stage(tab, s_tab);
    if (threadIdx.x < PA_OPT_GROUPS) s_step[threadIdx.x] = (int)threadIdx.x < ngroups ? group_consts[threadIdx.x] : 0.f;
    __syncthreads();
    const float bc2s = state->bc2s;
    const bool clip = clip_coef != nullptr;
    const float coef = clip ? clip_coef[0] : 1.f;
    size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
    for (; i + 3 < n; i += stride) {
        const int k = map[i >> 2] & (PA_OPT_GROUPS - 1);
        const PaOptGroupK gk = s_tab[k];
        if (gk.frozen) continue;
        const float step_size = s_step[k];
        PaAdamOpts og = o;
        og.wd = gk.wd; og.c_dec = gk.c_dec;
        f32x4 gg = *reinterpret_cast<const f32x4*>(g + i), mm = *reinterpret_cast<f32x4*>(m + i), vv = *reinterpret_cast<f32x4*>(v + i),
              pp = *reinterpret_cast<f32x4*>(p + i);
        f32x4 xx = {0.f, 0.f, 0.f, 0.f};
        if (AMSGRAD) xx = *reinterpret_cast<f32x4*>(vmax + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = pp[j], mj = mm[j], vj = vv[j], xj = xx[j];
            adam_groups_update<AMSGRAD, DECOUPLED>(pj, gg[j], mj, vj, xj, og, gscale, clip, coef, bc2s, step_size);
            pp[j] = pj; mm[j] = mj; vv[j] = vj; xx[j] = xj;
        }
        *reinterpret_cast<f32x4*>(m + i) = mm;
        *reinterpret_cast<f32x4*>(v + i) = vv;
        *reinterpret_cast<f32x4*>(p + i) = pp;
        if (AMSGRAD) *reinterpret_cast<f32x4*>(vmax + i) = xx;
    }
    if (i < n && i + 3 >= n) {                  // tail (at most 3 elements, one thread): the group of chunk n / 4
        const int k = map[n >> 2] & (PA_OPT_GROUPS - 1);
        const PaOptGroupK gk = s_tab[k];
        if (gk.frozen) return;
        const float step_size = s_step[k];
        PaAdamOpts og = o;
        og.wd = gk.wd; og.c_dec = gk.c_dec;
        for (; i < n; ++i) {
            float pj = p[i], mj = m[i], vj = v[i], xj = AMSGRAD ? vmax[i] : 0.f;
            adam_groups_update<AMSGRAD, DECOUPLED>(pj, g[i], mj, vj, xj, og, gscale, clip, coef, bc2s, step_size);
            p[i] = pj; m[i] = mj; v[i] = vj;
            if (AMSGRAD) vmax[i] = xj;
        }
    }
}

// ONE group that is not frozen: the launches of pa_launch_adam with that group's lr, wd and c_dec, hence its bits; with a
// group_consts array the prologue is the grouped one, which writes the same state words and group_consts[0] besides.
int pa_launch_adam_groups(const PaAdamOpts& o, bool amsgrad, bool decoupled, const PaOptGroupTable& tab, int ngroups, const unsigned char* map,
                          float* group_consts, float* p, const float* g, float* m, float* v, float* vmax, size_t n, float gscale,
                          const float* clip_coef, PaAdamState* state, hipStream_t st) {
    const bool single = ngroups == 1 && !tab.g[0].frozen;
    if (single && !group_consts) {
        PaAdamOpts o1 = o;
        o1.lr = tab.g[0].lr; o1.wd = tab.g[0].wd; o1.c_dec = tab.g[0].c_dec;
        return pa_launch_adam(o1, amsgrad, o1.wd != 0.f ? (decoupled ? 2 : 1) : 0, p, g, m, v, vmax, n, gscale, clip_coef, state, st);
    }
    if (n == 0) return 0;
    const int blocks = pa_grid_for(n / 4, 256, 2048);
#ifdef PA_FP16
    hipLaunchKernelGGL(grad_check_reset_kernel, dim3(1), dim3(1), 0, st, &state->flag);
    hipLaunchKernelGGL(grad_check_kernel, dim3(blocks), dim3(256), 0, st, g, n, &state->flag);
#endif
    hipLaunchKernelGGL(adam_prologue_groups_kernel, dim3(1), dim3(1), 0, st, state, tab, ngroups, group_consts, o.beta1, o.beta2);
    const dim3 grid(blocks), block(256);
    if (single) {
        PaAdamOpts o1 = o;
        o1.lr = tab.g[0].lr; o1.wd = tab.g[0].wd; o1.c_dec = tab.g[0].c_dec;
        const int decay = o1.wd != 0.f ? (decoupled ? 2 : 1) : 0;
        if (amsgrad) adam_launch_decay<true>(decay, grid, block, st, p, g, m, v, vmax, n, o1, gscale, clip_coef, state);
        else adam_launch_decay<false>(decay, grid, block, st, p, g, m, v, vmax, n, o1, gscale, clip_coef, state);
        return (int)hipGetLastError();
    }
    if (amsgrad && decoupled) hipLaunchKernelGGL((adam_groups_kernel<true, true>), grid, block, 0, st, p, g, m, v, vmax, n, o, tab, ngroups, map, group_consts, gscale, clip_coef, state);
    else if (amsgrad) hipLaunchKernelGGL((adam_groups_kernel<true, false>), grid, block, 0, st, p, g, m, v, vmax, n, o, tab, ngroups, map, group_consts, gscale, clip_coef, state);
    else if (decoupled) hipLaunchKernelGGL((adam_groups_kernel<false, true>), grid, block, 0, st, p, g, m, v, vmax, n, o, tab, ngroups, map, group_consts, gscale, clip_coef, state);
    else hipLaunchKernelGGL((adam_groups_kernel<false, false>), grid, block, 0, st, p, g, m, v, vmax, n, o, tab, ngroups, map, group_consts, gscale, clip_coef, state);
    return (int)hipGetLastError();
}

// grad_sqsum_kernel over the chunks whose group is not in the 16-bit mask `excluded` (the frozen groups): an excluded chunk adds
// nothing.  The grid, the per-thread order of additions, the block reduction and the finish kernel are pa_launch_grad_norm's, and
// s + (+0) == s for the non-negative partial sums, so the result is, bit for bit, that of pa_launch_grad_norm on a copy of the
// gradient with the excluded chunks set to +0 (inf and NaN in them included: they are not read).
__global__ __launch_bounds__(256) void grad_sqsum_groups_kernel(const float* g, size_t n, float gscale, double* partial,
                                                                const unsigned char* __restrict__ map, unsigned excluded) {
    __shared__ double lds[4];
    const double sc = (double)gscale;
    size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * 256 * 4;
    double s = 0.0;
    for (; i + 3 < n; i += stride) {
        if ((excluded >> (map[i >> 2] & (PA_OPT_GROUPS - 1))) & 1u) continue;
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) { const double t = (double)gg[j] * sc; s += t * t; }
    }
    if (i < n && i + 3 >= n && !((excluded >> (map[n >> 2] & (PA_OPT_GROUPS - 1))) & 1u))
        for (; i < n; ++i) { const double t = (double)g[i] * sc; s += t * t; }
    s = block_sum_double(s, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

int pa_launch_grad_norm_groups(const float* g, size_t n, const unsigned char* map, unsigned excluded, float gscale, float max_norm,
                               void* workspace, float* out2, hipStream_t st) {
    if (!excluded) return pa_launch_grad_norm(g, n, gscale, max_norm, workspace, out2, st);
    const int blocks = pa_grid_for(n / 4, 256, 2048);
    double* partial = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(grad_sqsum_groups_kernel, dim3(blocks), dim3(256), 0, st, g, n, gscale, partial, map, excluded);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, partial, blocks, max_norm, out2);
    return (int)hipGetLastError();
}

// plain streaming copy, 16 bytes per lane, 4 independent loads per thread and iteration: what "just moving the bytes" reaches on this
// part at a given size (bench.py roofline.floor calibrates with it instead of a framework kernel)
__global__ __launch_bounds__(256) void copy16_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16) {
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        const uint4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
        dst[i] = a; dst[i + stride] = b; dst[i + 2 * stride] = c; dst[i + 3 * stride] = d;
    }
    for (; i < n16; i += stride) dst[i] = src[i];
}

// form 1: ONE 16-byte chunk per thread, no loop (the guide's "float4 copy"); form 2: the grid-stride form with non-temporal loads / stores
__global__ __launch_bounds__(256) void copy16_flat_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) dst[i] = src[i];
}
__global__ __launch_bounds__(256) void copy16_nt_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    const u4* s = reinterpret_cast<const u4*>(src); u4* d = reinterpret_cast<u4*>(dst);
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        const u4 a = __builtin_nontemporal_load(s + i), b = __builtin_nontemporal_load(s + i + stride), c = __builtin_nontemporal_load(s + i + 2 * stride), e = __builtin_nontemporal_load(s + i + 3 * stride);
        __builtin_nontemporal_store(a, d + i); __builtin_nontemporal_store(b, d + i + stride); __builtin_nontemporal_store(c, d + i + 2 * stride); __builtin_nontemporal_store(e, d + i + 3 * stride);
    }
    for (; i < n16; i += stride) __builtin_nontemporal_store(__builtin_nontemporal_load(s + i), d + i);
}

int pa_launch_copy16(void* dst, const void* src, size_t bytes, hipStream_t st, int form) {
    const size_t n16 = bytes / 16;
    if (n16 == 0) return 0;
    if (form == 1) {
        hipLaunchKernelGGL(copy16_flat_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), n16);
        return (int)hipGetLastError();
    }
    const int blocks = pa_grid_for(n16, 1024, 256 * 16);        // 4 chunks per thread; 16 workgroups per CU, grid-stride beyond
    if (form == 2) hipLaunchKernelGGL(copy16_nt_kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), n16);
    else hipLaunchKernelGGL(copy16_kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), n16);
    return (int)hipGetLastError();
}

int pa_rmsprop_skipped(const int* state, long long* out, hipStream_t st) {
    int h[2] = {0, 0};
#ifdef PA_FP16
    hipError_t e = state ? hipMemcpyAsync(h, state, sizeof h, hipMemcpyDeviceToHost, st)
                         : hipMemcpyFromSymbolAsync(h, HIP_SYMBOL(g_grad_state), sizeof h, 0, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
#endif
    *out = h[1];
    return 0;
}

// ------------------------------------------------------------------------------------------------
// fp32 master weights (PyTorch layout [Cout][Cin][taps]) -> bf16 compute copies
//   wf[n][tap][c]            forward / wgrad layout, zero padded to pad_cout x pad_cin
//   wb[c][taps-1-tap][n]     dgrad layout (transposed, taps flipped)
// taps == 49 marks the 7x7 stem: wf[n][ky*32 + kx*4 + c] (K padded to 256), no wb.
__global__ __launch_bounds__(1024) void weight_prep_kernel(const PaPrepJob* jobs) {
    const PaPrepJob j = jobs[blockIdx.y];
    if (j.taps == 49) {
        const int total = j.pad_cout * 256;
        for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
            int n = e >> 8, k = e & 255;
            int ky = k >> 5, kx = (k & 31) >> 2, c = k & 3;
            float v = 0.f;
            if (n < j.Cout && ky < 7 && kx < 7 && c < j.Cin) v = j.w[((size_t)(n * j.Cin + c) * 7 + ky) * 7 + kx];
            j.wf[e] = (bf16)v;
        }
        return;
    }
    // 32 x 32 (n, c) tiles: the fp32 source is read once, in contiguous runs (taps floats per thread); wf is written along c,
    // wb along n through an LDS transpose (read element-wise per output the strided source fetched 10-20x its bytes)
    __shared__ bf16 tile[9][32][33];
    const int tn = threadIdx.x >> 5, tc = threadIdx.x & 31;
    const int tiles_c = j.pad_cin / 32, ntiles = (j.pad_cout / 32) * tiles_c;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int n0 = (t / tiles_c) * 32, c0 = (t % tiles_c) * 32;
        const int n = n0 + tn, c = c0 + tc;
        const bool ok = n < j.Cout && c < j.Cin;
        const float* src = j.w + ((size_t)n * j.Cin + c) * j.taps;
        for (int tap = 0; tap < j.taps; ++tap) {
            const bf16 v = (bf16)(ok ? src[tap] : 0.f);
            j.wf[((size_t)n * j.taps + tap) * j.pad_cin + c] = v;
            tile[tap][tn][tc] = v;
        }
        __syncthreads();
        if (j.wb) {
            // thread (tn, tc) now writes channel c0 + tn, output channel n0 + tc
            for (int tap = 0; tap < j.taps; ++tap)
                j.wb[((size_t)(c0 + tn) * j.taps + (j.taps - 1 - tap)) * j.pad_cout + n0 + tc] = tile[tap][tc][tn];
        }
        __syncthreads();
    }
}

int pa_launch_weight_prep(const PaPrepJob* jobs_dev, int njobs, int max_elems, hipStream_t st) {
    if (njobs <= 0) return 0;
    (void)max_elems;
    hipLaunchKernelGGL(weight_prep_kernel, dim3(32, njobs), dim3(1024), 0, st, jobs_dev);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// layout conversion
__global__ void nchw_to_nhwc4_kernel(const float* src, bf16* dst, int B, int H, int W) {
    const size_t total = (size_t)B * H * W;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        size_t hw = (size_t)H * W;
        size_t b = p / hw, r = p - b * hw;
        bf16x4 o;
        o[0] = (bf16)src[(b * 3 + 0) * hw + r];
        o[1] = (bf16)src[(b * 3 + 1) * hw + r];
        o[2] = (bf16)src[(b * 3 + 2) * hw + r];
        o[3] = (bf16)0.f;
        *reinterpret_cast<bf16x4*>(dst + p * 4) = o;
    }
}

int pa_launch_nchw_to_nhwc4(const float* src, bf16* dst, int B, int H, int W, hipStream_t st) {
    size_t total = (size_t)B * H * W;
    const int blocks = pa_grid_for(total, 256, 4096);
    hipLaunchKernelGGL(nchw_to_nhwc4_kernel, dim3(blocks), dim3(256), 0, st, src, dst, B, H, W);
    return (int)hipGetLastError();
}

__global__ void nhwc_to_nchw_f32_kernel(const float* src, float* dst, int B, int H, int W, int C) {
    const size_t total = (size_t)B * C * H * W;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        size_t hw = (size_t)H * W;
        size_t b = e / (C * hw), r = e - b * C * hw;
        size_t c = r / hw, p = r - c * hw;
        dst[e] = src[(b * hw + p) * C + c];
    }
}

int pa_launch_nhwc_to_nchw_f32(const float* src, float* dst, int B, int H, int W, int C, hipStream_t st) {
    size_t total = (size_t)B * H * W * C;
    const int blocks = pa_grid_for(total, 256, 4096);
    hipLaunchKernelGGL(nhwc_to_nchw_f32_kernel, dim3(blocks), dim3(256), 0, st, src, dst, B, H, W, C);
    return (int)hipGetLastError();
}

__global__ void nchw_f32_to_nhwc_bf16_kernel(const float* src, bf16* dst, int B, int C, int H, int W) {
    const size_t total = (size_t)B * C * H * W;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        size_t hw = (size_t)H * W;
        size_t c = e % C, p = e / C;           // destination order
        size_t b = p / hw, r = p - b * hw;
        dst[e] = (bf16)src[(b * C + c) * hw + r];
    }
}

int pa_launch_nchw_f32_to_nhwc_bf16(const float* src, bf16* dst, int B, int C, int H, int W, hipStream_t st) {
    size_t total = (size_t)B * H * W * C;
    const int blocks = pa_grid_for(total, 256, 4096);
    hipLaunchKernelGGL(nchw_f32_to_nhwc_bf16_kernel, dim3(blocks), dim3(256), 0, st, src, dst, B, C, H, W);
    return (int)hipGetLastError();
}

__global__ void nhwc_bf16_to_nchw_f32_kernel(PaOperand src, float* dst, int B, int C, int H, int W) {
    const size_t total = (size_t)B * C * H * W;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        size_t hw = (size_t)H * W;
        size_t c = e % C, p = e / C;           // source order
        size_t b = p / hw, r = p - b * hw;
        float v = (float)src.p[e];
        if (src.mode == PA_LD_BNRELU) v = fmaxf(fmaf(src.k0[c], v, src.k1[c]), 0.f);
        else if (src.mode == PA_LD_LIN2) v = fmaf(src.k0[c], v, fmaf(src.k1[c], (float)src.q[e], src.k2[c]));
        dst[(b * C + c) * hw + r] = v;
    }
}

int pa_launch_nhwc_bf16_to_nchw_f32(const PaOperand& src, float* dst, int B, int C, int H, int W, hipStream_t st) {
    size_t total = (size_t)B * H * W * C;
    const int blocks = pa_grid_for(total, 256, 4096);
    hipLaunchKernelGGL(nhwc_bf16_to_nchw_f32_kernel, dim3(blocks), dim3(256), 0, st, src, dst, B, C, H, W);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// apply an epilogue to a gradient tensor (e.g. mask + BatchNorm-backward reductions of a gradient
// that arrives from outside the conv kernels)
__global__ __launch_bounds__(1024) void ep_apply_kernel(PaOperand g, PaEpilogue ep, bf16* out, size_t M, int C) {
    extern __shared__ float red[];
    const int CG = C / 8;
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    const int c = (threadIdx.x % CG) * 8;
    const size_t total = M * CG;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t idx = (t / CG) * C + c;
        float v[8];
        pa_read8(g, idx, c, v);
        *reinterpret_cast<bf16x8*>(out + idx) = epilogue8(ep, idx, c, v, s1, s2);
    }
    if (ep.mode != PA_OUT_PLAIN) flush_stats(red, ep.stats, C, c, s1, s2);
}

int pa_launch_ep_apply(const PaOperand& g, const PaEpilogue& ep, bf16* out, size_t M, int C, hipStream_t st, int* stat_rows) {
    PaEltPlan p;
    if (pa_elt_plan(p, PA_ELT_APPLY, M * (C / 8), 0, 0, 0, C, ep.mode != PA_OUT_PLAIN, false)) return 1;
    if (stat_rows) *stat_rows = p.blocks;
    if (ep.rows_out) *ep.rows_out = p.blocks;
    hipLaunchKernelGGL(ep_apply_kernel, dim3(p.blocks), dim3(p.threads), p.lds, st, g, ep, out, M, C);
    return (int)hipGetLastError();
}

// Occlusion mask of the reference's _Hourglass._dropout (models/asn_stacked_hg.py:79-100): out = ep(value(x) * m),
// m = mask[b][4*(y / (H/4)) + x / (W/4)] -- the n x 1 x 4 x 4 cell mask, nearest-upsampled to the H x W map, times every
// channel.  Forward: ep = plain.  Backward: x = the gradient of the masked tensor, ep = the epilogue that finishes the
// gradient of the tensor that was masked (ReLU mask + BatchNorm-backward reductions).
__global__ __launch_bounds__(1024) void cell_mask_kernel(PaOperand x, const float* mask, PaEpilogue ep, bf16* out, int B, int H, int W, int C) {
    extern __shared__ float red[];
    const int CG = C / 8;
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    const int c = (threadIdx.x % CG) * 8;
    const size_t total = (size_t)B * H * W * CG;
    const int ch = H / 4, cw = W / 4;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t pix = t / CG;
        const size_t idx = pix * C + c;
        const int xw = (int)(pix % W);
        const size_t q = pix / W;
        const int y = (int)(q % H), b = (int)(q / H);
        const float m = mask[(size_t)b * 16 + 4 * (y / ch) + xw / cw];
        float v[8];
        pa_read8(x, idx, c, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= m;
        *reinterpret_cast<bf16x8*>(out + idx) = epilogue8(ep, idx, c, v, s1, s2);
    }
    if (ep.mode != PA_OUT_PLAIN) flush_stats(red, ep.stats, C, c, s1, s2);
}

int pa_launch_cell_mask(const PaOperand& x, const float* mask, const PaEpilogue& ep, bf16* out, int B, int H, int W, int C,
                        hipStream_t st) {
    if (H % 4 != 0 || W % 4 != 0 || C % 8 != 0) { pa_set_error_msg("pa_launch_cell_mask: the map must be a multiple of the 4x4 cell grid"); return 1; }
    PaEltPlan p;
    if (pa_elt_plan(p, PA_ELT_MASK, (size_t)B * H * W * (C / 8), B, H, W, C, ep.mode != PA_OUT_PLAIN, false)) return 1;
    if (ep.rows_out) *ep.rows_out = p.blocks;
    hipLaunchKernelGGL(cell_mask_kernel, dim3(p.blocks), dim3(p.threads), p.lds, st, x, mask, ep, out, B, H, W, C);
    return (int)hipGetLastError();
}

// end of a pose forward pass: hand the per-stack losses out (keep: the engine's own copy [n + 1]; out: the caller's [n], may be NULL), their
// sum (keep[n], *total -- the reference's `loss = sum over stacks`, stack-hg.py:156-159, without a framework reduction kernel between the
// backward pass and the optimizer) and clear the accumulators for the next pass (was a memset launch in front of every step)
__global__ void loss_out_kernel(float* acc, float* keep, float* out, float* total, int n) {
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) { const float v = acc[i]; s += v; keep[i] = v; if (out) out[i] = v; acc[i] = 0.f; }
        keep[n] = s;
        if (total) *total = s;
    }
}

int pa_launch_loss_out(float* acc, float* keep, float* out, float* total, int n, hipStream_t st) {
    hipLaunchKernelGGL(loss_out_kernel, dim3(1), dim3(64), 0, st, acc, keep, out, total, n);
    return (int)hipGetLastError();
}

__global__ void fill_kernel(float* p, float v, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

int pa_launch_fill(float* p, float v, size_t n, hipStream_t st) {
    const int blocks = pa_grid_for(n, 256, 1024);
    hipLaunchKernelGGL(fill_kernel, dim3(blocks), dim3(256), 0, st, p, v, n);
    return (int)hipGetLastError();
}
