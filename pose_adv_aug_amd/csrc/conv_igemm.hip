// Implicit-GEMM convolution (1x1 and 3x3 'same', stride 1) on bf16 MFMA for gfx950.
//
//   out[m][n] = epilogue( sum_{tap,c} load(in)[pixel(m)+tap][c] * w[n][tap][c] + bias[n] + add1 + add2 )
//
// m = flattened NHWC pixel (B*H*W rows), n = output channel.  The same kernel serves
//   * forward convs   (reference models/asn_stacked_hg.py:17-24, 241-248): the input's pending
//     BatchNorm+ReLU is applied while the tile is staged (PA_LD_BNRELU), the residual add and the
//     per-channel sum / sum^2 needed by the NEXT BatchNorm are done in the epilogue (PA_OUT_STATS);
//   * data gradients  (dgrad): `in` is the output gradient with the BatchNorm backward applied on
//     load (PA_LD_LIN2), `w` is the transposed/tap-flipped weight copy, and the epilogue masks by the
//     ReLU of the tensor the gradient belongs to and accumulates the two BatchNorm-backward
//     reductions (PA_OUT_BWD).
//
// Tiling: BMxBN output tile per 256-thread workgroup (4 waves as 2x2), K step 64.  Both operand
// tiles are staged global -> registers (transform) -> LDS as [row][64] bf16 with the 16-byte chunk
// index XOR-swizzled by (row & 7), so the ds_read_b128 fragment reads of
// v_mfma_f32_16x16x32_bf16 are bank-conflict free.  The weight fragment is the MFMA A operand and
// the activation fragment the B operand, so each lane ends up with 4 consecutive output channels of
// one pixel (8-byte bf16x4 stores, per-channel reductions over the 16 pixel lanes by DPP shuffles).
#include "common.h"
#include "kernels.h"
#include "common.h"
// cycle stamps (tuning builds, a.dbg & 64): entry / loads issued / constants (finalize prologue) / staged / barrier / K loop / epilogue parts
PA_STAMP_DECL(pa_conv1_clk, pa_debug_conv1_clocks)
#define PA_STAMP1(i) PA_STAMP_AT(pa_conv1_clk, a.dbg & 64, i)
#define PA_EPI_STAMP(i) PA_STAMP1(i)
#include "conv_epilogue.h"
#include <string.h>

// STEM: the A operand is the 4-channel-padded input image and the kernel computes the 7x7 stride-2
// stem conv (reference models/asn_stacked_hg.py:223) as a K=256 GEMM: k = ky*32 + kx*4 + c, i.e. one
// 16-byte chunk = 2 horizontally adjacent input pixels; a.H/a.W are the OUTPUT dims.
// FIN: the instance that can carry the input's BatchNorm finalize in its prologue (bn_fin.h) -- the 64 x 64 tiles of the small maps only;
// every other instance is the plain kernel, its register allocation untouched
template <int BM, int BN, int LDMODE, int TAPS, bool STEM = false, bool FIN = false>
__global__ __launch_bounds__(256, FIN ? 2 : 1) void conv_igemm_kernel(PaConvArgs a) {      // (FIN: left alone the prologue takes every register it can get -- 256, one workgroup per CU; the plain 64 x 64 instance runs at 116)
    constexpr int AI = BM / 32, BI = BN / 32;      // staged 16-byte chunks per thread (A / B tile)
    constexpr int MI = BM / 32, NI = BN / 32;      // 16x16 fragments per wave (wave tile BM/2 x BN/2)
    __shared__ __attribute__((aligned(16))) bf16 lds[(BM + BN) * 64];
    __shared__ float kst[LDMODE == PA_LD_PLAIN ? 4 : 3 * 512 + (FIN ? 2048 : 0)];      // per-channel constants of the input transform (+ the finalize prologue's scratch)
    bf16* As = lds;
    bf16* Bs = lds + BM * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int M = a.B * a.H * a.W, HW = a.H * a.W;
    const int K = TAPS * a.Cin;
    const int nK = K / 64;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int cc = tid & 7, r = tid >> 3;

    int am[AI], ay[AI], ax[AI], ab[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        int m = m0 + r + 32 * i;
        am[i] = m < M ? m : -1;
        ab[i] = m / HW;
        int rem = m - ab[i] * HW;
        ay[i] = rem / a.W;
        ax[i] = rem - ay[i] * a.W;
    }

    bf16x8 ra[AI], rq[AI], rb[BI];
    unsigned okmask = 0;
    int cur_c = 0;

    auto gload = [&](int kt) {
        if (STEM) {
            const int cidx = kt * 8 + cc, ky = cidx >> 2, q = cidx & 3;
            const int Hin = 2 * a.H, Win = 2 * a.W;
            okmask = 0;
#pragma unroll
            for (int i = 0; i < AI; ++i) {
                bf16x4 lo = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f}, hi = lo;
                const int yi = 2 * ay[i] + ky - 3, xi = 2 * ax[i] + 2 * q - 3;
                if (am[i] >= 0 && ky < 7 && (unsigned)yi < (unsigned)Hin) {
                    const bf16* rowp = a.in.p + ((size_t)ab[i] * Hin + yi) * Win * 4;
                    if ((unsigned)xi < (unsigned)Win) lo = *reinterpret_cast<const bf16x4*>(rowp + (size_t)xi * 4);
                    if ((unsigned)(xi + 1) < (unsigned)Win) hi = *reinterpret_cast<const bf16x4*>(rowp + (size_t)(xi + 1) * 4);
                }
                ra[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                okmask |= 1u << i;
            }
#pragma unroll
            for (int i = 0; i < BI; ++i)
                rb[i] = *reinterpret_cast<const bf16x8*>(a.w + (size_t)(n0 + r + 32 * i) * K + kt * 64 + cc * 8);
            return;
        }
        int tap = 0, c0 = kt * 64, dy = 0, dx = 0;
        if (TAPS == 9) { tap = c0 / a.Cin; c0 -= tap * a.Cin; dy = tap / 3 - 1; dx = tap - (tap / 3) * 3 - 1; }
        cur_c = c0 + cc * 8;
        okmask = 0;
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            bool ok = am[i] >= 0;
            if (TAPS == 9) ok = ok && (unsigned)(ay[i] + dy) < (unsigned)a.H && (unsigned)(ax[i] + dx) < (unsigned)a.W;
            if (ok) {
                size_t idx = (size_t)(am[i] + dy * a.W + dx) * a.Cin + cur_c;
                ra[i] = *reinterpret_cast<const bf16x8*>(a.in.p + idx);
                if (LDMODE == PA_LD_LIN2) rq[i] = *reinterpret_cast<const bf16x8*>(a.in.q + idx);
                okmask |= 1u << i;
            }
        }
#pragma unroll
        for (int i = 0; i < BI; ++i)
            rb[i] = *reinterpret_cast<const bf16x8*>(a.w + (size_t)(n0 + r + 32 * i) * K + kt * 64 + cc * 8);
    };

    auto lstore = [&]() {
        float k0[8], k1[8], k2[8];
        if (LDMODE != PA_LD_PLAIN) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { k0[j] = kst[cur_c + j]; k1[j] = kst[512 + cur_c + j]; }
            if (LDMODE == PA_LD_LIN2) {
#pragma unroll
                for (int j = 0; j < 8; ++j) k2[j] = kst[1024 + cur_c + j];
            }
        }
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            int row = r + 32 * i;
            bf16x8 o;
            if (okmask & (1u << i)) {
                if (LDMODE == PA_LD_PLAIN) {
                    o = ra[i];
                } else if (LDMODE == PA_LD_BNRELU) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) o[j] = (bf16)fmaxf(fmaf(k0[j], (float)ra[i][j], k1[j]), 0.f);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        o[j] = (bf16)fmaf(k0[j], (float)ra[i][j], fmaf(k1[j], (float)rq[i][j], k2[j]));
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (bf16)0.f;
            }
            *reinterpret_cast<bf16x8*>(As + row * 64 + ((cc ^ (row & 7)) << 3)) = o;
        }
#pragma unroll
        for (int i = 0; i < BI; ++i) {
            // weight rows are STORED permuted (conv_epilogue.h: pa_lds_row_of_weight_row) so that a lane's fragments
            // hold 8 CONSECUTIVE channels per 32-channel chunk (16-byte epilogue accesses) while the fragment reads
            // stay conflict-free
            const int lrow = pa_lds_row_of_weight_row<BN, NI>(r + 32 * i);
            *reinterpret_cast<bf16x8*>(Bs + lrow * 64 + ((cc ^ (lrow & 7)) << 3)) = rb[i];
        }
    };

    f32x4 acc[NI][MI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};

    gload(0);
    // per-channel constants of the input transform, behind the first tile's loads (they are in flight meanwhile)
    bool fin_done = false;
    if constexpr (FIN && LDMODE != PA_LD_PLAIN) {
        if (a.fin.rows > 0) {
            // the input's BatchNorm finalize (forward: scale / shift; backward: kA / kB / kC) from the producer's partial rows, bn_fin.h
            pa_bn_fin_prologue<256, 512>(a.fin, a.Cin, kst, kst + 3 * 512, blockIdx.x == 0 && blockIdx.y == 0);
            fin_done = true;
        }
    }
    if (LDMODE != PA_LD_PLAIN && !fin_done) {
        for (int c = threadIdx.x; c < a.Cin; c += 256) {
            kst[c] = a.in.k0[c]; kst[512 + c] = a.in.k1[c];
            if (LDMODE == PA_LD_LIN2) kst[1024 + c] = a.in.k2[c];
        }
    }
    __syncthreads();            // kst visible
    lstore();
    __syncthreads();

    const int frow = lane & 15, fchk = lane >> 4;
    for (int kt = 0; kt < nK; ++kt) {
        if (kt + 1 < nK) gload(kt + 1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 fa[MI], fw[NI];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                int row = wm * (BM / 2) + mi * 16 + frow;
                fa[mi] = *reinterpret_cast<const bf16x8*>(As + row * 64 + (((fchk + 4 * kk) ^ (row & 7)) << 3));
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                int row = wn * (BN / 2) + ni * 16 + frow;
                fw[ni] = *reinterpret_cast<const bf16x8*>(Bs + row * 64 + (((fchk + 4 * kk) ^ (row & 7)) << 3));
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
                    acc[ni][mi] = PA_MFMA_16x16x32(fw[ni], fa[mi], acc[ni][mi]);
        }
        __syncthreads();
        if (kt + 1 < nK) {
            lstore();
            __syncthreads();
        }
    }

    // ---------------------------------------------------------------- epilogue (conv_epilogue.h)
    pa_conv_epilogue_auto<BN, NI, MI>(a, acc, n0, wm, wn,
                                     [&](int wr, int mi, int p) { const int m = m0 + wr * (BM / 2) + mi * 16 + p; return m < M ? m : -1; },
                                     reinterpret_cast<float*>(lds), (int)blockIdx.x);
}

// ------------------------------------------------------------------------------------------------------------------
// ONE-SHOT 1x1 kernel for the small maps (64 x 64 tiles, Cin = 64 * NK <= 256): the whole K range of both operand tiles is requested
// at once (NK x 4 ... 6 sixteen-byte loads per thread in flight), transformed and staged into LDS in one pass, and the K loop runs
// without a global load or a barrier.  The generic kernel above walks K in 64-channel steps with a dependent memory round trip and
// two barriers per step: at 16 x 16 and below that chain of 2 - 4 round trips IS the kernel (6.5 - 7.8 us for 0.1 - 0.8 GFLOP).
// Same tile, same fragment layout, same epilogue and weight-row permutation as conv_igemm_kernel<64, 64, ...>: same results bit for bit
// (the MFMA accumulation order over K is unchanged).
// POOL: the instances whose second epilogue addend is pool-routed (PA_LD_POOL, conv_epilogue.h), one per epilogue
template <int NK, int LDMODE, bool FIN, int POOL = PA_POOL_EP_NONE>
__global__ __launch_bounds__(256, 2) void conv1x1_oneshot_kernel(PaConvArgs a) {
    PA_SET_MAIN_PRIO();
    PA_STAMP1(0);
    constexpr int BM = 64, BN = 64, AI = 2, BI = 2, MI = 2, NI = 2;
    __shared__ __attribute__((aligned(16))) bf16 lds[(BM + BN) * 64 * NK];
    __shared__ float kst[LDMODE == PA_LD_PLAIN ? 4 : 3 * 512 + (FIN ? 2048 : 0)];
    bf16* As = lds;
    bf16* Bs = lds + NK * BM * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int M = a.B * a.H * a.W;
    const int K = NK * 64;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int cc = tid & 7, r = tid >> 3;

    // ---- every load of the thread first
    bf16x8 xa[NK][AI], xq[NK][AI], xb[NK][BI];
    bool ok[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) ok[i] = m0 + r + 32 * i < M;
#pragma unroll
    for (int kt = 0; kt < NK; ++kt) {
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            const size_t idx = ok[i] ? (size_t)(m0 + r + 32 * i) * K + kt * 64 + cc * 8 : 0;       // clamped, unconditional
            xa[kt][i] = *reinterpret_cast<const bf16x8*>(a.in.p + idx);
            if (LDMODE == PA_LD_LIN2) xq[kt][i] = *reinterpret_cast<const bf16x8*>(a.in.q + idx);
        }
#pragma unroll
        for (int i = 0; i < BI; ++i)
            xb[kt][i] = *reinterpret_cast<const bf16x8*>(a.w + (size_t)(n0 + r + 32 * i) * K + kt * 64 + cc * 8);
    }
    PA_STAMP1(1);
    // ---- per-channel constants of the input transform (or the pending BatchNorm finalize, bn_fin.h), while the loads travel
    if (LDMODE != PA_LD_PLAIN) {
        bool fin_done = false;
        if constexpr (FIN) {
            if (a.fin.rows > 0) { pa_bn_fin_prologue<256, 512>(a.fin, K, kst, kst + 3 * 512, blockIdx.x == 0 && blockIdx.y == 0); fin_done = true; }
        }
        if (!fin_done) {
            for (int c = tid; c < K; c += 256) {
                kst[c] = a.in.k0[c]; kst[512 + c] = a.in.k1[c];
                if (LDMODE == PA_LD_LIN2) kst[1024 + c] = a.in.k2[c];
            }
            __syncthreads();
        }
    }
    PA_STAMP1(2);
    // ---- transform + stage the whole K range
#pragma unroll
    for (int kt = 0; kt < NK; ++kt) {
        const int c = kt * 64 + cc * 8;
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            const int row = r + 32 * i;
            bf16x8 o;
            if (LDMODE == PA_LD_PLAIN) {
                o = xa[kt][i];
            } else if (LDMODE == PA_LD_BNRELU) {
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (bf16)fmaxf(fmaf(kst[c + j], (float)xa[kt][i][j], kst[512 + c + j]), 0.f);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (bf16)fmaf(kst[c + j], (float)xa[kt][i][j], fmaf(kst[512 + c + j], (float)xq[kt][i][j], kst[1024 + c + j]));
            }
            if (!ok[i]) {
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (bf16)0.f;
            }
            *reinterpret_cast<bf16x8*>(As + kt * (BM * 64) + row * 64 + ((cc ^ (row & 7)) << 3)) = o;
        }
#pragma unroll
        for (int i = 0; i < BI; ++i) {
            const int lrow = pa_lds_row_of_weight_row<BN, NI>(r + 32 * i);
            *reinterpret_cast<bf16x8*>(Bs + kt * (BN * 64) + lrow * 64 + ((cc ^ (lrow & 7)) << 3)) = xb[kt][i];
        }
    }
    PA_STAMP1(3);
    __syncthreads();
    PA_STAMP1(4);

    f32x4 acc[NI][MI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15, fchk = lane >> 4;
#pragma unroll
    for (int kt = 0; kt < NK; ++kt)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 fa[MI], fw[NI];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const int row = wm * (BM / 2) + mi * 16 + frow;
                fa[mi] = *reinterpret_cast<const bf16x8*>(As + kt * (BM * 64) + row * 64 + (((fchk + 4 * kk) ^ (row & 7)) << 3));
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                const int row = wn * (BN / 2) + ni * 16 + frow;
                fw[ni] = *reinterpret_cast<const bf16x8*>(Bs + kt * (BN * 64) + row * 64 + (((fchk + 4 * kk) ^ (row & 7)) << 3));
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
                    acc[ni][mi] = PA_MFMA_16x16x32(fw[ni], fa[mi], acc[ni][mi]);
        }
    PA_STAMP1(5);
    __syncthreads();            // every wave is done with the tiles before the epilogue reuses the LDS
    pa_conv_epilogue_auto<BN, NI, MI, true, false, 256, false, POOL>(a, acc, n0, wm, wn,
                                     [&](int wr, int mi, int p) { const int m = m0 + wr * (BM / 2) + mi * 16 + p; return m < M ? m : -1; },
                                     reinterpret_cast<float*>(lds), (int)blockIdx.x);
    PA_STAMP1(6);
}

// the variant of an instance id (conv_plan.h) picks the load mode, the finalize prologue and the pool-routed forms
template <int NK>
static void launch_oneshot(const PaConvArgs& a0, int variant, dim3 grid, hipStream_t st) {
    PaConvArgs a = a0; a.dbg = pa_tuning().conv1_dbg;      // tuning builds: cycle stamps
    if constexpr (NK == 2) {             // the pool-routed second addend: 128 input channels only
        if (variant == PA_CV_POOL_BWD) { hipLaunchKernelGGL((conv1x1_oneshot_kernel<2, PA_LD_LIN2, false, PA_POOL_EP_BWD>), grid, dim3(256), 0, st, a); return; }
        if (variant == PA_CV_POOL_PLAIN) { hipLaunchKernelGGL((conv1x1_oneshot_kernel<2, PA_LD_LIN2, false, PA_POOL_EP_PLAIN>), grid, dim3(256), 0, st, a); return; }
    }
    switch (variant) {
        case PA_LD_PLAIN: hipLaunchKernelGGL((conv1x1_oneshot_kernel<NK, PA_LD_PLAIN, false>), grid, dim3(256), 0, st, a); break;
        case PA_LD_BNRELU: hipLaunchKernelGGL((conv1x1_oneshot_kernel<NK, PA_LD_BNRELU, false>), grid, dim3(256), 0, st, a); break;
        case PA_CV_BNRELU_FIN: hipLaunchKernelGGL((conv1x1_oneshot_kernel<NK, PA_LD_BNRELU, true>), grid, dim3(256), 0, st, a); break;
        case PA_CV_LIN2_FIN: hipLaunchKernelGGL((conv1x1_oneshot_kernel<NK, PA_LD_LIN2, true>), grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((conv1x1_oneshot_kernel<NK, PA_LD_LIN2, false>), grid, dim3(256), 0, st, a); break;
    }
}

template <int BM, int BN, int TAPS>
static void launch_ld(const PaConvArgs& a, int variant, dim3 grid, hipStream_t st) {
    if constexpr (BM == 64 && BN == 64) {      // the tier that exists with the finalize prologue
        if (variant == PA_CV_BNRELU_FIN) { hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, PA_LD_BNRELU, TAPS, false, true>), grid, dim3(256), 0, st, a); return; }
        if (variant == PA_CV_LIN2_FIN) { hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, PA_LD_LIN2, TAPS, false, true>), grid, dim3(256), 0, st, a); return; }
    }
    switch (variant) {
        case PA_LD_PLAIN: hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, PA_LD_PLAIN, TAPS>), grid, dim3(256), 0, st, a); break;
        case PA_LD_BNRELU: hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, PA_LD_BNRELU, TAPS>), grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, PA_LD_LIN2, TAPS>), grid, dim3(256), 0, st, a); break;
    }
}

int pa_launch_stem_conv(const PaConvArgs& a, hipStream_t st, int* stat_rows) {
    // a.in.p = img4 [B][2H][2W][4]; a.w = [64][256]; a.Cin must be 256 (virtual), a.Cout 64
    if (a.Cin != 256 || a.Cout != 64 || a.in.mode != PA_LD_PLAIN) { pa_set_error_msg("pa_launch_stem_conv: bad arguments"); return 1; }
    const int M = a.B * a.H * a.W;
    const int bm = pa_conv_big_m(M) ? 128 : 64, rows = (M + bm - 1) / bm;
    if (stat_rows) *stat_rows = rows; if (a.ep.rows_out) *a.ep.rows_out = rows;
    if (bm == 128) hipLaunchKernelGGL((conv_igemm_kernel<128, 64, PA_LD_PLAIN, 1, true>), dim3(rows, 1), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conv_igemm_kernel<64, 64, PA_LD_PLAIN, 1, true>), dim3(rows, 1), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

static int g_log[1024][14], g_nlog = -1;      // test hook pa_conv_launch_log (-1: off): the distinct launches, as pa_conv_plan_describe takes them
static void log_launch(const PaConvShape& s) {
    const int r[14] = {s.B, s.H, s.W, s.Cin, s.Cout, s.taps, s.in_mode, s.add1_mode, s.add2_mode, s.ep_mode, s.ep2_mode, s.fin_rows,
                       s.bias | s.out2 << 1 | s.want_dz << 2 | s.in_map << 3 | s.in_q << 4 | s.ep2_affine << 5 | s.add2_map << 6, s.cus};
    int i = 0; while (i < g_nlog && memcmp(g_log[i], r, sizeof r)) ++i;
    if (i == g_nlog && i < 1024) memcpy(g_log[g_nlog++], r, sizeof r);
}
int pa_launch_conv(const PaConvArgs& a0, const PaConvPlan& p, hipStream_t st, int* stat_rows) {
    if (p.path == PA_CVP_REFUSED) { pa_set_error_msg(p.why); return 1; }
    if (g_nlog >= 0) log_launch(pa_conv_shape(a0));
    PaConvArgs a = a0; a.xcd = p.xcd; if (!p.stores_dz) a.dz_out = nullptr;
    if (stat_rows) *stat_rows = p.rows;
    if (int* r = p.rows2 ? a.ep2.rows_out : a.ep.rows_out) *r = p.rows;      // (ROW_UP: the statistics are the second output's)
    if (p.path == PA_CVP_TILE3) return pa_launch_conv3x3_tile(a, p, st);
    if (p.path == PA_CVP_ROW || p.path == PA_CVP_ROW_UP) return pa_launch_conv1x1_tile(a, p, st);
    const dim3 grid(p.gx, p.gy); const int v = p.variant();
    switch (p.tiling()) {
        case PA_CT_G128x128_1: launch_ld<128, 128, 1>(a, v, grid, st); break;
        case PA_CT_G128x128_9: launch_ld<128, 128, 9>(a, v, grid, st); break;
        case PA_CT_G128x64_1: launch_ld<128, 64, 1>(a, v, grid, st); break;
        case PA_CT_G128x64_9: launch_ld<128, 64, 9>(a, v, grid, st); break;
        case PA_CT_G64x128_1: launch_ld<64, 128, 1>(a, v, grid, st); break;
        case PA_CT_G64x128_9: launch_ld<64, 128, 9>(a, v, grid, st); break;
        case PA_CT_G64x64_1: launch_ld<64, 64, 1>(a, v, grid, st); break;
        case PA_CT_G64x64_9: launch_ld<64, 64, 9>(a, v, grid, st); break;
        case PA_CT_OS2: launch_oneshot<2>(a, v, grid, st); break;
        case PA_CT_OS4: launch_oneshot<4>(a, v, grid, st); break;
        default: pa_set_error_msg("pa_launch_conv: the plan names no instance of conv_igemm.hip"); return 1;
    }
    return (int)hipGetLastError();
}

// include/poseadv.h (diagnostics): the plan of a launch as integers.  No HIP call: it answers without a device (cus: the caller's count)
extern "C" int pa_conv_plan_describe(int B, int H, int W, int Cin, int Cout, int taps, int in_mode, int add1_mode, int add2_mode, int ep_mode,
                                     int ep2_mode, int fin_rows, int flags, int cus, int* out, int cap) {
    if (!out || cap < 16) { pa_set_error_msg("pa_conv_plan_describe: out is NULL or holds fewer than 16 ints"); return -1; }
    const PaConvPlan p = pa_conv_plan(PaConvShape{B, H, W, Cin, Cout, taps, in_mode, add1_mode, add2_mode, ep_mode, ep2_mode, fin_rows, bool(flags & 1),
                                                  bool(flags & 2), bool(flags & 4), bool(flags & 8), bool(flags & 16), bool(flags & 32), bool(flags & 64), cus});
    static const float some_bias = 0.f;
    PaConvArgs a{};          // the kernels' own copy of the LDS-epilogue rule, for the test that holds the two together
    a.xcd = p.xcd; a.add1.mode = add1_mode; a.add2.mode = add2_mode; a.bias = (flags & 1) ? &some_bias : nullptr;
    const int v[16] = {p.path, p.inst, p.gx, p.gy, p.threads, p.nbw, p.rows, p.rows2, p.xcd, p.takes_fin, p.stores_dz, p.pool_route, p.pool_in,
                       p.bwd_lds, p.path != PA_CVP_REFUSED && pa_conv_inst_cannot_trap(p.inst), pa_bwd_epilogue_lds_ok(a)};
    memcpy(out, v, sizeof v); if (p.path == PA_CVP_REFUSED) pa_set_error_msg(p.why);      // (an admitted plan leaves the last error as it is)
    return 16;
}
// out NULL: clear the launch log and switch it on; else copy up to cap launches of 14 ints (the first 14 arguments above), switch it off, return their number
extern "C" int pa_conv_launch_log(int* out, int cap) {
    const int n = !out || g_nlog < 0 ? 0 : g_nlog < cap ? g_nlog : cap;
    if (out) memcpy(out, g_log, sizeof(int) * 14 * n);
    g_nlog = out ? -1 : 0; return n;
}
