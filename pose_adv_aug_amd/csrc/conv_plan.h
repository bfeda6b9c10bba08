// Which kernel instance takes a forward or data-gradient convolution, over which grid, into how many partial-statistics rows, and what the
// launch can carry (a pending finalize, a stored dz, a pool-routed operand): decided in ONE place.  Host code only; no HIP types.  The launchers
// (conv_igemm.hip, conv1x1_tile.hip, conv3x3_tile.hip) switch over the instance the plan names, net.hip reads the plan's fields, and these switches
// of tuning.h are read here only: conv1_old, conv3_old, conv3_nosmall, igemm_oneshot, epi_bwd_direct, conv3_noxcd, no_dz3, no_dz2.
#pragma once
#include "tuning.h"
#include "modes.h"
// Everything the dispatch depends on, and nothing else (kernels.h: pa_conv_shape fills it from a launch)
struct PaConvShape {
    int B, H, W, Cin, Cout, taps;
    int in_mode, add1_mode, add2_mode;       // PA_LD_*
    int ep_mode, ep2_mode, fin_rows;         // PA_OUT_* (ep2: the second output's, out2); partial rows of a pending finalize of the input (0: none)
    bool bias, out2, want_dz;                // want_dz: the caller has a buffer for the transformed input
    bool in_map, in_q, ep2_affine, add2_map; // operands of the pool-routed forms: in.map, in.q, ep2.scale && ep2.shift, add2.map
    int cus;                                 // compute units of the device (0: unknown)
};
// refused (PaConvPlan::why says why) | conv_igemm.hip: conv_igemm_kernel, K in 64-channel steps | conv1x1_oneshot_kernel (64 x 64 tiles, 128 / 256 input channels) |
// conv1x1_tile.hip: row tiles of 64 / 128 pixels | ... the instance that also stores the low-resolution half of the upsample-add backward (out2 / ep2) | conv3x3_tile.hip
enum PaConvPath { PA_CVP_REFUSED, PA_CVP_GENERIC, PA_CVP_ONESHOT, PA_CVP_ROW, PA_CVP_ROW_UP, PA_CVP_TILE3 };
// An instance id is tiling * PA_CV_N + variant: one value per template instantiation.  Tilings -- G<BM>x<BN>_<taps> generic | OS<NK> one-shot | R<CIN>_<BM>_<BN> row tile (K32: 32-channel weight slices, three workgroups per CU;
// PIN: pool-routed input; UP: 2 image rows x 32 columns) | T16x8 / T16x4 / TS8 / TS4 _<CIN>_<BN> halo tiles (T512: 512 threads)
enum PaConvTiling {
    PA_CT_G128x128_1, PA_CT_G128x128_9, PA_CT_G128x64_1, PA_CT_G128x64_9, PA_CT_G64x128_1, PA_CT_G64x128_9, PA_CT_G64x64_1, PA_CT_G64x64_9,
    PA_CT_OS2, PA_CT_OS4,
    PA_CT_R256_64_128_K32, PA_CT_R256_64_128, PA_CT_R256_64_64, PA_CT_R128_64_128, PA_CT_R128_64_64, PA_CT_R128_128_128, PA_CT_R128_128_64,
    PA_CT_R64_64_128, PA_CT_R64_128_128, PA_CT_R64_128_64, PA_CT_R128_64_64_PIN, PA_CT_R128_64_128_UP,
    PA_CT_T16x8_128_128, PA_CT_T16x8_128_64, PA_CT_T16x8_64_128, PA_CT_T16x8_64_64, PA_CT_T16x4_128_64_T512, PA_CT_T16x4_128_64,
    PA_CT_TS8_128_64_T512, PA_CT_TS8_64_64, PA_CT_TS4_128_64_T512, PA_CT_TS4_64_64,
    PA_CT_N
};
// Variants: the load mode the instance is compiled for (PA_LD_PLAIN / BNRELU / LIN2 = 0 / 1 / 2), + the finalize prologue, pool-routed add2 per epilogue
enum { PA_CV_BNRELU_FIN = 4, PA_CV_LIN2_FIN = 5, PA_CV_POOL_BWD = 6, PA_CV_POOL_PLAIN = 7, PA_CV_N = 8 };
struct PaConvPlan {
    int path, inst;          // PaConvPath; tiling * PA_CV_N + variant
    int gx, gy, threads;     // grid and workgroup size
    int nbw;                 // row tiles: output-channel blocks a workgroup loops over
    int rows, rows2;         // partial-statistics rows the launch writes (stat_rows / ep.rows_out); of the second output (ROW_UP: ep2.rows_out), else 0
    int xcd;                 // PaConvArgs::xcd: bit 0 one contiguous range of tiles per XCD, bit 1 the direct BatchNorm-backward epilogue is forced
    bool takes_fin, stores_dz; // the instance exists with the finalize prologue (launched with it when fin_rows > 0); the launch stores its transformed input
    bool pool_route, pool_in; // add2 / the input is pool-routed and the instance carries the mode
    bool bwd_lds;            // the LDS form of the BatchNorm-backward epilogue takes the launch
    const char* why;         // REFUSED: the message
    int tiling() const { return inst / PA_CV_N; } int variant() const { return inst % PA_CV_N; }
};
// the LDS form of the BatchNorm-backward epilogue (conv_epilogue.h) takes: addend 1 none / plain / LIN2, addend 2 none / plain, no bias, and
// is not switched off (xcd bit 1); pa_bwd_epilogue_lds_ok is the kernels' copy of this rule
inline bool pa_bwd_lds_modes_ok(int xcd, bool bias, int add1_mode, int add2_mode) {
    return xcd < 2 && !bias && (add1_mode == PA_LD_NONE || add1_mode == PA_LD_PLAIN || add1_mode == PA_LD_LIN2) &&
           (add2_mode == PA_LD_NONE || add2_mode == PA_LD_PLAIN);
}
// small problems get 64-row tiles so that the grid still covers the 256 CUs (generic kernel and the stem)
inline bool pa_conv_big_m(long long M) { return M >= 128 * 256; }
inline PaConvPlan pa_conv_refuse(const char* why) { PaConvPlan p{}; p.path = PA_CVP_REFUSED; p.inst = -1; p.why = why; return p; }

inline PaConvPlan pa_conv_plan(const PaConvShape& s) {
    const PaTuning& t = pa_tuning();
    const long long M = (long long)s.B * s.H * s.W;
    const bool bigN = s.Cout % 128 == 0, even = s.H % 2 == 0 && s.W % 2 == 0, bwd = s.ep_mode == PA_OUT_BWD;
    const bool fits32 = (unsigned long long)M * (unsigned long long)(s.Cin > s.Cout ? s.Cin : s.Cout) < (1ull << 31);   // the epilogues index with 32 bits
    PaConvPlan p{};
    p.xcd = t.epi_bwd_direct ? 2 : 0;
    p.bwd_lds = pa_bwd_lds_modes_ok(p.xcd, s.bias, s.add1_mode, s.add2_mode);
    const bool need_direct = bwd && !p.bwd_lds;       // a BatchNorm-backward epilogue the LDS form does not take
    const bool add1_ok = s.add1_mode == PA_LD_NONE || s.add1_mode == PA_LD_PLAIN || s.add1_mode == PA_LD_LIN2;
    const bool ep_pool_ok = s.ep_mode == PA_OUT_PLAIN || (bwd && p.xcd < 2);       // the pool-routed instances carry these two epilogues
    // ---- the row-tile 1x1 kernel: 64, 128 or 256 input channels and at least 192 row tiles.  64-row tiles also for 128 input channels: at
    // B = 24, 64 x 64 maps the 768 tiles of 128 rows fill 256 CUs x 2 workgroups 1.5 times; 1536 tiles of 64 rows at 3 workgroups / CU are 2 full rounds
    bool row = !t.conv1_old && s.taps == 1 && (s.Cin == 64 || s.Cin == 128 || s.Cin == 256) && s.Cout % 64 == 0 && fits32;
    // the POOL instances: 128 -> 128 k channels, BatchNorm backward on load, plain output or the LDS BatchNorm-backward epilogue
    if (s.add2_mode == PA_LD_POOL && !(s.Cin == 128 && bigN && s.in_mode == PA_LD_LIN2 && !s.bias && !s.out2 && s.fin_rows == 0 && even && add1_ok && ep_pool_ok)) row = false;
    // the PIN instance: 128 -> 64 channels, the transformed tile stored, the table form of the BatchNorm-backward epilogue
    if (s.in_mode == PA_LD_POOL && !(s.Cin == 128 && !bigN && s.in_map && s.in_q && s.want_dz && !s.bias && !s.out2 && s.fin_rows == 0 && even &&
                                     s.add1_mode == PA_LD_NONE && s.add2_mode == PA_LD_NONE && bwd && p.xcd < 2 && s.ep2_affine)) row = false;
    // (64 -> 64 channels: every instance carries the table form of the BatchNorm-backward epilogue only)
    if (s.Cin == 64 && !bigN && need_direct) row = false;
    int bm = s.Cin == 64 ? 128 : 64;
    if (row && (M + bm - 1) / bm < 192) row = false;           // smaller problems: generic kernel with 64 x 64 tiles
    // ---- pool-routed operands: only instances of their own carry them -- the input the PIN instance (which stores dz: not under no_dz3), the
    // second addend the row-tile POOL instances or the one-shot kernel's for 128 input channels
    const bool oneshot_m = !pa_conv_big_m(M) && !(bigN && M >= 64 * 256);      // the 64 x 64 tier of the generic dispatch
    const bool pool2 = s.add2_mode == PA_LD_POOL && s.add2_map && s.taps == 1 && s.Cin == 128 && s.Cout % 64 == 0 && s.in_mode == PA_LD_LIN2 && !s.bias &&
                       !s.out2 && s.fin_rows == 0 && even && add1_ok && ep_pool_ok && fits32 && (row || (oneshot_m && t.igemm_oneshot != 0));
    if (s.add1_mode == PA_LD_POOL || (s.in_mode == PA_LD_POOL && !(row && !t.no_dz3)) || (s.add2_mode == PA_LD_POOL && !pool2))
        return pa_conv_refuse("pa_launch_conv: a pool-routed operand is the second addend of a 1x1 data gradient with 128 input channels that reaches a row-tile or one-shot instance, or the input of one that reaches the 128 -> 64 row-tile instance (conv_plan.h)");
    if ((s.taps != 1 && s.taps != 9) || s.Cin % 64 != 0 || s.Cout % 64 != 0 || s.Cin > 512)
        return pa_conv_refuse("pa_launch_conv: channel counts must be multiples of 64 and taps 1 or 9");
    if (!fits32) return pa_conv_refuse("pa_launch_conv: tensors of 2^31 elements or more are not supported (split the batch)");
    p.pool_route = s.add2_mode == PA_LD_POOL; p.pool_in = s.in_mode == PA_LD_POOL; p.threads = 256;
    const bool fin_mode = s.in_mode == PA_LD_BNRELU || s.in_mode == PA_LD_LIN2;      // (the prologue computes scale / shift or kA / kB / kC)
    const int ld_variant = s.in_mode == PA_LD_PLAIN || s.in_mode == PA_LD_BNRELU ? s.in_mode : PA_LD_LIN2;
    const int fin_variant = s.in_mode == PA_LD_BNRELU ? PA_CV_BNRELU_FIN : PA_CV_LIN2_FIN;
    // ---- the halo-tile 3x3 kernel: 64 or 128 input channels; 16 x 8 tiles, 16 x 4 tiles (3 workgroups per CU) where those would leave CUs idle
    // (measured 64 x 64 maps, 768 tiles: 39.8 vs 42.8 us in favour of 16 x 8; 32 x 32 maps, 192 tiles: 17.6 vs 14.6 us in favour of 16 x 4), and 8 x 8 / 4 x 4 tiles for maps
    // with sides multiples of 8 (that the 16 x 8 tiles do not take) or of 4; any other map up to 8 x 8 -- the 6 x 6 necks of the 384 x 384 configuration -- is ONE masked 8 x 8 tile
    const bool big16 = s.H % 8 == 0 && s.W % 16 == 0;
    const int side = big16 || t.conv3_nosmall ? 0 : (s.H % 8 == 0 && s.W % 8 == 0) ? 8 : (s.H % 4 == 0 && s.W % 4 == 0) ? 4 : (s.H <= 8 && s.W <= 8) ? 8 : 0;
    // the 512-thread instances (small tiles with 128 input channels, 16 x 4 tiles at one workgroup per CU) carry the LDS form only: a small-tile
    // launch that needs the direct form goes to the generic kernel, a 16 x 4 one to the 256-thread instance
    if (!t.conv3_old && s.taps == 9 && (s.Cin == 64 || s.Cin == 128) && (big16 || (side && !(s.Cin == 128 && need_direct)))) {
        p.path = PA_CVP_TILE3;
        const int tiles128 = big16 ? s.B * (s.H / 8) * (s.W / 16) : 0;
        const bool half = big16 && s.Cin == 128 && tiles128 < 512;
        const int img = side ? 128 / (side * side) : 1;                        // sub-tiles per workgroup
        const int tiles = side ? (s.B * ((s.H + side - 1) / side) * ((s.W + side - 1) / side) + img - 1) / img : half ? 2 * tiles128 : tiles128;
        // the low-resolution levels have 3..12 pixel tiles: 64-channel halves double the number of workgroups, and so do the 16 x 4 tiles:
        // 64-channel blocks halve the serial chain of a workgroup -- 32 x 32: 16.5 -> 16.1 / 19.3 -> 17.8 us (forward / data gradient)
        const bool n128 = bigN && big16 && !half;
        p.gx = p.rows = tiles; p.gy = s.Cout / (n128 ? 128 : 64);
        p.xcd |= !t.conv3_noxcd && big16 && tiles % 8 == 0 ? 1 : 0;      // one contiguous range of tiles per XCD: +0.3 % on the step (halo re-reads served by the XCD's own L2)
        int tl;
        // 16 x 4: 512 threads when the launch is at most one workgroup per CU (the 16 x 16 maps: 192 workgroups, 12.0 -> 8.6 us); with two
        // workgroups per CU (32 x 32) the 256-thread workgroups already overlap each other and 512 measured slower (16.1 vs 18.2)
        if (half) tl = p.gx * p.gy <= s.cus && !need_direct ? PA_CT_T16x4_128_64_T512 : PA_CT_T16x4_128_64;
        else if (big16) tl = s.Cin == 128 ? (n128 ? PA_CT_T16x8_128_128 : PA_CT_T16x8_128_64) : (n128 ? PA_CT_T16x8_64_128 : PA_CT_T16x8_64_64);
        else if (side == 8) tl = s.Cin == 128 ? PA_CT_TS8_128_64_T512 : PA_CT_TS8_64_64;
        else tl = s.Cin == 128 ? PA_CT_TS4_128_64_T512 : PA_CT_TS4_64_64;
        if (tl == PA_CT_T16x4_128_64_T512 || tl == PA_CT_TS8_128_64_T512 || tl == PA_CT_TS4_128_64_T512) p.threads = 512;
        const bool withfin = side || half || tl == PA_CT_T16x8_64_64;          // the tilings that exist with the finalize prologue
        p.takes_fin = withfin && fin_mode; p.stores_dz = s.want_dz && s.in_mode == PA_LD_LIN2 && !t.no_dz2; p.inst = tl * PA_CV_N + (withfin && s.fin_rows > 0 ? fin_variant : ld_variant);
        return p;
    }
    if (row) {      // ---- the row-tile 1x1 kernel
        if (s.fin_rows > 0) return pa_conv_refuse("pa_launch_conv: a pending finalize was handed to the row-tile 1x1 kernel (it has no prologue: PaConvPlan::takes_fin)");
        p.stores_dz = (s.want_dz && s.in_mode == PA_LD_LIN2 && !t.no_dz3) || p.pool_in;
        if (s.out2) {
            // the UP instance: 128 -> 128 k channels, BatchNorm backward on load, one plain addend, plain output, rows multiples of 32 pixels, even row count
            if (s.Cin != 128 || !bigN || s.in_mode != PA_LD_LIN2 || s.bias || s.want_dz || s.add1_mode != PA_LD_PLAIN || s.add2_mode != PA_LD_NONE ||
                s.ep_mode != PA_OUT_PLAIN || s.ep2_mode != PA_OUT_BWD || s.W % 32 != 0 || s.H % 2 != 0)
                return pa_conv_refuse("pa_launch_conv1x1_tile: not a launch of the 2 x 32-pixel instance (conv_plan.h: PA_CVP_ROW_UP)");
            p.path = PA_CVP_ROW_UP; p.inst = PA_CT_R128_64_128_UP * PA_CV_N + PA_LD_LIN2;
            p.gx = p.rows = p.rows2 = (int)(M / 64);
            p.nbw = p.gx >= 512 ? s.Cout / 128 : 1; p.gy = s.Cout / 128 / p.nbw;
            return p;
        }
        p.path = PA_CVP_ROW;
        // 64 input channels, 128 output channels: 64-row tiles at three workgroups per CU (the 128-row instance spills at 168 registers); the
        // 64-row instances of 64 and (BatchNorm backward on load) 128 input channels have the LDS epilogue only
        if (s.Cin == 64 && bigN && !need_direct) bm = 64;
        if (s.Cin == 128 && s.in_mode == PA_LD_LIN2 && need_direct && !p.pool_route) bm = 128;
        const int nb = s.Cout / (bigN ? 128 : 64);
        p.gx = p.rows = (int)((M + bm - 1) / bm);
        p.nbw = p.gx >= 512 ? nb : 1; p.gy = nb / p.nbw;          // enough row tiles: loop over the channel blocks inside (input read once)
        int tl, v = ld_variant;
        if (p.pool_in) { tl = PA_CT_R128_64_64_PIN; v = PA_LD_LIN2; }
        else if (p.pool_route) { tl = PA_CT_R128_64_128; v = bwd ? PA_CV_POOL_BWD : PA_CV_POOL_PLAIN; }
        // 256 channels: the three-workgroup instance (32-channel weight slices) unless the launch needs the direct BatchNorm-backward epilogue
        else if (s.Cin == 256) tl = !bigN ? PA_CT_R256_64_64 : need_direct ? PA_CT_R256_64_128 : PA_CT_R256_64_128_K32;
        else if (s.Cin == 128) tl = bm == 64 ? (bigN ? PA_CT_R128_64_128 : PA_CT_R128_64_64) : (bigN ? PA_CT_R128_128_128 : PA_CT_R128_128_64);
        else tl = bm == 64 ? PA_CT_R64_64_128 : bigN ? PA_CT_R64_128_128 : PA_CT_R64_128_64;
        p.inst = tl * PA_CV_N + v;
        return p;
    }
    // ---- the generic kernel; its 64 x 64 tier (the only one with the finalize prologue) is the one-shot kernel for the 1x1 layers with 128 / 256 input channels
    p.takes_fin = fin_mode && s.Cin <= 256 && oneshot_m;
    if (s.fin_rows > 0 && (s.fin_rows > PA_FIN_SMALL_ROWS || !p.takes_fin))
        return pa_conv_refuse("pa_launch_conv: finalize prologue needs <= 128 partial rows, <= 256 channels and an instance that carries it (PaConvPlan::takes_fin)");
    const bool bigM = pa_conv_big_m(M);
    p.gx = p.rows = (int)((M + (bigM ? 127 : 63)) / (bigM ? 128 : 64)); p.gy = s.Cout / (bigN && !oneshot_m ? 128 : 64);
    if (oneshot_m && t.igemm_oneshot != 0 && s.taps == 1 && (s.Cin == 128 || s.Cin == 256)) {
        p.path = PA_CVP_ONESHOT;
        p.inst = (s.Cin == 128 ? PA_CT_OS2 : PA_CT_OS4) * PA_CV_N +
                 (p.pool_route ? (bwd ? PA_CV_POOL_BWD : PA_CV_POOL_PLAIN) : s.fin_rows > 0 ? fin_variant : ld_variant);
        return p;
    }
    p.path = PA_CVP_GENERIC;
    const int tl = (bigM ? (bigN ? PA_CT_G128x128_1 : PA_CT_G128x64_1) : !oneshot_m ? PA_CT_G64x128_1 : PA_CT_G64x64_1) + (s.taps == 9 ? 1 : 0);
    p.inst = tl * PA_CV_N + (s.fin_rows > 0 ? fin_variant : ld_variant);
    return p;
}
// can a launch the LDS form does not take run on the instance without reaching the trap of pa_conv_epilogue_auto?  Not on the table-form row tiles (CTAB
// of conv1x1_tile_kernel) and the 512-thread halo tiles (NT != 256 of conv3x3_tile_kernel): a HAND-KEPT copy of those two template constants, a new instance
// must be entered here.  The POOL variants and the UP instance have no direct epilogue either but one of their own, and return before the trap
inline bool pa_conv_inst_cannot_trap(int inst) {
    const int tl = inst / PA_CV_N, v = inst % PA_CV_N;
    if (v == PA_CV_POOL_BWD || v == PA_CV_POOL_PLAIN || tl == PA_CT_R128_64_128_UP) return true;
    return !(tl == PA_CT_T16x4_128_64_T512 || tl == PA_CT_TS8_128_64_T512 || tl == PA_CT_TS4_128_64_T512 || tl == PA_CT_R256_64_128_K32 ||
             tl == PA_CT_R128_64_64_PIN || tl == PA_CT_R64_64_128 || tl == PA_CT_R64_128_64 ||
             ((tl == PA_CT_R128_64_128 || tl == PA_CT_R128_64_64) && v == PA_LD_LIN2));
}
