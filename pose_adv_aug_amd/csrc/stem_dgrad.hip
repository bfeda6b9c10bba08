// Data gradient of the 7x7 stride-2 stem convolution (reference models/asn_stacked_hg.py:223): d loss / d image for gfx950.
//
//   dimg[b][y][x][c] = sum_{n,ky,kx} g[b][(y+3-ky)/2][(x+3-kx)/2][n] * w[n][c][ky][kx]        (taps whose two quotients are integers inside the map)
//
// As a GEMM: one ROW is the 2 x 2 block of image pixels at (2i, 2j), its N = 16 outputs are (parity py, px) x 4 channels, and its
// K = 1024 operand is the 4 x 4 window i-1..i+2, j-1..j+2 of g x 64 channels: window row wy meets image row 2i + py through tap
// ky = py + 5 - 2 wy (3 taps for an even row, 4 for an odd one; the same in x), every other entry of the [1024][16] weight tile is
// zero, and so is the 4th channel.  N = 16 is the N of PA_MFMA_16x16x32: the weight tile is the A operand, the window the B operand,
// and a lane ends up with the 4 channels of ONE image pixel (parity lane >> 4 of block lane & 15) -- one 16-byte store.
//
// A 256-thread workgroup builds the weight tile once in LDS (32 KB, from the stem's packed forward copy wf[n][ky*32 + kx*4 + c]: no
// second packed copy) and then walks tiles of 8 x 8 blocks: the 11 x 11 x 64 window of g is loaded once (the BatchNorm backward applied
// on load, fp32, rounded once to the storage type), staged in LDS (15.1 KB), and each wave runs 16 blocks through ONE chain of 32
// MFMAs (K = 1024 into one fp32 accumulator per output).  Borders and partial tiles by predication: nothing outside g is read,
// nothing outside dimg is written.
#include "common.h"
#include "kernels.h"

#define SD_TB 8                              // blocks per tile side
#define SD_TP (SD_TB + 3)                    // g pixels per tile side (the windows of 8 blocks span i0-1 .. i0+9)
#define SD_NPIX (SD_TP * SD_TP)
#define SD_ITEMS (SD_NPIX * 8)               // 16-byte chunks of a staged tile
#define SD_U ((SD_ITEMS + 255) / 256)        // chunks per thread

// 16-byte chunk q of staged pixel P: XOR swizzle so that the fragment reads of neighbouring pixels spread over the banks
__device__ __forceinline__ int sd_slot(int P, int q) { return P * 64 + ((q ^ ((P >> 1) & 7)) << 3); }

template <int LDMODE>
__global__ __launch_bounds__(256, 2) void stem_dgrad_kernel(PaStemDgradArgs a) {
    __shared__ __attribute__((aligned(16))) bf16 Wt[1024 * 16];      // [k / 8][16 outputs][8]: lane l of K step s reads chunk s * 64 + l
    __shared__ __attribute__((aligned(16))) bf16 Gt[SD_NPIX * 64];
    __shared__ float kst[3 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- the weight tile: Wt[(wy, wx, n)][(py, px, c)] = w[n][c][py + 5 - 2 wy][px + 5 - 2 wx] or 0
    for (int e = tid; e < 2048; e += 256) {
        const int kc = e >> 4, o = e & 15;
        const int wp = kc >> 3, n0 = (kc & 7) * 8, wy = wp >> 2, wx = wp & 3;
        const int c = o & 3, py = o >> 3, px = (o >> 2) & 1;
        const int ky = py + 5 - 2 * wy, kx = px + 5 - 2 * wx;
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (bf16)0.f;
        if (ky >= 0 && ky < 7 && kx >= 0 && kx < 7 && c < 3) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = a.wf[(n0 + j) * 256 + ky * 32 + kx * 4 + c];
        }
        *reinterpret_cast<bf16x8*>(Wt + e * 8) = v;
    }
    if (LDMODE == PA_LD_LIN2 && tid < 64) { kst[tid] = a.g.k0[tid]; kst[64 + tid] = a.g.k1[tid]; kst[128 + tid] = a.g.k2[tid]; }
    __syncthreads();

    const int tj_n = (a.Wm + SD_TB - 1) / SD_TB, ti_n = (a.Hm + SD_TB - 1) / SD_TB;
    const int ntiles = a.B * ti_n * tj_n;
    const int H = 2 * a.Hm, W = 2 * a.Wm;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int b = t / (ti_n * tj_n), tr = t - b * (ti_n * tj_n);
        const int i0 = (tr / tj_n) * SD_TB, j0 = (tr % tj_n) * SD_TB;
        // ---- stage the window: every load of the thread first, then transform and store
        bf16x8 rp[SD_U], rq[SD_U];
        bool ok[SD_U];
#pragma unroll
        for (int u = 0; u < SD_U; ++u) {
            const int e = tid + 256 * u, P = e >> 3, q = e & 7;
            const int gy = i0 - 1 + P / SD_TP, gx = j0 - 1 + P % SD_TP;
            ok[u] = e < SD_ITEMS && (unsigned)gy < (unsigned)a.Hm && (unsigned)gx < (unsigned)a.Wm;
            if (ok[u]) {
                const size_t idx = (((size_t)b * a.Hm + gy) * a.Wm + gx) * 64 + q * 8;
                rp[u] = *reinterpret_cast<const bf16x8*>(a.g.p + idx);
                if (LDMODE == PA_LD_LIN2) rq[u] = *reinterpret_cast<const bf16x8*>(a.g.q + idx);
            }
        }
#pragma unroll
        for (int u = 0; u < SD_U; ++u) {
            const int e = tid + 256 * u, P = e >> 3, q = e & 7;
            if (e >= SD_ITEMS) continue;
            bf16x8 o;
            if (!ok[u]) {
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (bf16)0.f;
            } else if (LDMODE == PA_LD_LIN2) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    o[j] = (bf16)fmaf(kst[q * 8 + j], (float)rp[u][j], fmaf(kst[64 + q * 8 + j], (float)rq[u][j], kst[128 + q * 8 + j]));
            } else {
                o = rp[u];
            }
            *reinterpret_cast<bf16x8*>(Gt + sd_slot(P, q)) = o;
        }
        __syncthreads();

        // ---- 16 blocks per wave (two rows of the tile), K = 1024 in one accumulator chain
        const int col = lane & 15, br = 2 * wave + (col >> 3), bc = col & 7, kq = lane >> 4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int s = 0; s < 32; ++s) {
            const int wp = s >> 1, P = (br + (wp >> 2)) * SD_TP + bc + (wp & 3);
            const bf16x8 fb = *reinterpret_cast<const bf16x8*>(Gt + sd_slot(P, (s & 1) * 4 + kq));
            const bf16x8 fa = *reinterpret_cast<const bf16x8*>(Wt + (s * 64 + lane) * 8);
            acc = PA_MFMA_16x16x32(fa, fb, acc);
        }
        const int i = i0 + br, j = j0 + bc;
        if (i < a.Hm && j < a.Wm) {
            const int y = 2 * i + (kq >> 1), x = 2 * j + (kq & 1);
            if (a.layout == 1) {
                *reinterpret_cast<f32x4*>(a.out + (((size_t)b * H + y) * W + x) * 4) = f32x4{acc[0] * a.scale, acc[1] * a.scale, acc[2] * a.scale, 0.f};
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) a.out[(((size_t)b * 3 + c) * H + y) * W + x] = acc[c] * a.scale;
            }
        }
        __syncthreads();            // Gt is staged again by the next tile
    }
}

int pa_launch_stem_dgrad(const PaStemDgradArgs& a, hipStream_t st) {
    if (!a.g.p || !a.wf || !a.out || a.B < 1 || a.Hm < 1 || a.Wm < 1 || (a.layout != 0 && a.layout != 1) ||
        (a.g.mode != PA_LD_PLAIN && a.g.mode != PA_LD_LIN2) || (a.g.mode == PA_LD_LIN2 && (!a.g.q || !a.g.k0 || !a.g.k1 || !a.g.k2)) ||
        (reinterpret_cast<uintptr_t>(a.out) & 15)) {
        pa_set_error_msg("pa_launch_stem_dgrad: bad arguments");
        return 1;
    }
    const long ntiles = (long)a.B * ((a.Hm + SD_TB - 1) / SD_TB) * ((a.Wm + SD_TB - 1) / SD_TB);
    if (ntiles > 0x7fffffffL) { pa_set_error_msg("pa_launch_stem_dgrad: too many tiles"); return 1; }
    // (every workgroup builds the weight tile once and then walks tiles: three workgroups per CU, what 47 KB of LDS each allow)
    const int cus = pa_conv_cus() > 0 ? pa_conv_cus() : 256;
    const int grid = (int)(ntiles < 3L * cus ? ntiles : 3L * cus);
    if (a.g.mode == PA_LD_LIN2) hipLaunchKernelGGL(stem_dgrad_kernel<PA_LD_LIN2>, dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(stem_dgrad_kernel<PA_LD_PLAIN>, dim3(grid), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

// fp32 [64][3][7][7] -> the stem's packed forward copy wf[n][ky*32 + kx*4 + c] (what weight_prep_kernel makes for the net): pa_stem_dgrad
__global__ __launch_bounds__(256) void stem_pack_kernel(const float* w, bf16* wf) {
    const int e = blockIdx.x * 256 + threadIdx.x;            // 64 * 256 elements
    const int n = e >> 8, k = e & 255, ky = k >> 5, kx = (k & 31) >> 2, c = k & 3;
    float v = 0.f;
    if (ky < 7 && kx < 7 && c < 3) v = w[((size_t)(n * 3 + c) * 7 + ky) * 7 + kx];
    wf[e] = (bf16)v;
}

int pa_launch_stem_pack(const float* w, bf16* wf, hipStream_t st) {
    hipLaunchKernelGGL(stem_pack_kernel, dim3(64), dim3(256), 0, st, w, wf);
    return (int)hipGetLastError();
}
