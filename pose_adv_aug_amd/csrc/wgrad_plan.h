// Which kernel takes a layer's weight gradient, with which channel blocks, over how many pixel tiles, into how many slabs: decided in ONE
// place.  Host code only; no HIP types.  The slab count fixes the memory Net::layout_conv allocates, the grid every launcher builds and the
// summation order of the result's bits, so the layout (pa_wgrad_plan, pa_wgrad_layer_splits) and the launchers (pa_wgrad_launch_plan) all
// read it here, and the policy numbers of tuning.h are read here only.
#pragma once
#include "tuning.h"

enum PaWgradPath {
    PA_WGP_GENERIC,          // conv_wgrad.hip: any pixel count, 8x8 register transposes
    PA_WGP_TILE,             // conv_wgrad_tile.hip: 128-pixel tiles (1x1) / 8 x 16-pixel tiles with their halo (3x3)
    PA_WGP_STEM_TILE,        // the 7x7/2 stem as a K = 256 GEMM on the tile kernel: 64 output channels x 256 patch elements per workgroup
    PA_WGP_STEM_GENERIC      // ... on the generic kernel, 64 x 128
};
// bodies of wgrad_group_kernel: 3x3 64 x 64 (n x c) with a plain / BatchNorm-backward dy operand (fixed modes: the 144-accumulator body has
// no registers to spare for both) | 1x1 128 x 128 | 128 x 64 | 64 x 128 | 64 x 64
enum { PA_WGK_9_44 = 0, PA_WGK_9_44L, PA_WGK_1_44, PA_WGK_1_42, PA_WGK_1_24, PA_WGK_1_22, PA_WGK_N };

struct PaWgradPlan {
    int path;                // PaWgradPath
    int nb, cb;              // output- / input-channel block of a workgroup (generic kernel: TN / TK)
    int ntiles;              // pixel tiles (tile paths) or pixel steps (generic) the splits share
    int splits;              // slab count of the layer launched alone
    int group_splits;        // slab count as a job of a group launch; 0: the grouped kernel does not take the shape
    int group_kind;          // body of wgrad_group_kernel for a plain dy operand (-1: none); PA_WGK_9_44L is picked from dy.mode at launch
    int blocks;              // workgroups per split: (Cout / nb) * (Cin / cb), times the taps on the generic kernel (one tap each)
};

// `s` workgroups over `ntiles` tiles, balanced
inline int pa_wgrad_balanced(int ntiles, int s) {
    const int per = (ntiles + s - 1) / s;          // tiles per workgroup
    return (ntiles + per - 1) / per;
}

// the generic kernel takes every shape (channel counts: multiples of 64, taps 1 or 9); M pixels
inline PaWgradPlan pa_wgrad_generic_plan(int M, int Cin, int Cout, int taps, bool stem) {
    const PaTuning& t = pa_tuning();
    PaWgradPlan p{};
    p.path = stem ? PA_WGP_STEM_GENERIC : PA_WGP_GENERIC; p.group_kind = -1;
    const int f = taps == 1 ? t.wgrad_tile1 : t.wgrad_tile9;       // experiments: 1 = 64x64, 2 = 128x64, 3 = 64x128
    p.nb = Cout % 128 == 0 && f != 1 && f != 3 ? 128 : 64;
    p.cb = Cin % 128 == 0 && f != 1 && f != 2 ? 128 : 64;
    p.blocks = (Cout / p.nb) * (taps * Cin / p.cb);
    const int ms = p.nb + p.cb <= 128 ? 128 : 64;       // pixels per step: 128 for the 64x64 tile (all 256 threads stage an 8x8 block each)
    p.ntiles = (M + ms - 1) / ms;
    // enough workgroups to keep every CU busy with several of them (measured on MI355X: 512 for the 1x1 layers, 1024 for the 3x3 layers;
    // PA_WGRAD_BLOCKS overrides for experiments), a multiple of 8 splits
    const int target = t.wgrad_blocks >= 8 ? t.wgrad_blocks : (taps == 9 ? 1024 : 512);
    const int s = ((target + p.blocks - 1) / p.blocks + 7) & ~7;
    p.splits = s > p.ntiles ? (p.ntiles < 1 ? 1 : p.ntiles) : s;
    // the stem's instance is 64 x 128 over 64-pixel steps whatever the switches say (its split count follows the rule above all the same)
    if (stem) { p.nb = 64; p.cb = 128; p.ntiles = (M + 63) / 64; p.blocks = 2; }
    return p;
}

// H <= 0 or W <= 0: spatial shape unknown, B counts the pixels (generic kernel only).  stem: Cin = 256 (the padded 7 x 7 x 4 patch),
// Cout = 64, taps = 1, H / W the OUTPUT map.
inline PaWgradPlan pa_wgrad_plan(int B, int H, int W, int Cin, int Cout, int taps, bool stem) {
    const PaTuning& t = pa_tuning();
    const bool shaped = H > 0 && W > 0;
    const int M = shaped ? B * H * W : B;
    PaWgradPlan p = pa_wgrad_generic_plan(M, Cin, Cout, taps, stem);
    if (stem) {
        // 64 KB slabs, so two workgroups per CU (their load / MFMA phases overlap); 512: 6.96 vs 7.00 ms (256).  More splits than tiles:
        // the count above, and the generic kernel at launch
        const int ntiles = (M + 127) / 128;
        if (t.stem_splits > 0 && t.stem_splits <= ntiles) p.splits = t.stem_splits;
        if (!t.wgrad_old && !t.stem_wgrad_old) { p.path = PA_WGP_STEM_TILE; p.nb = 64; p.cb = 256; p.ntiles = ntiles; p.blocks = 1; }
        return p;
    }
    if (t.wgrad_old || !shaped || Cin % 64 || Cout % 64 || (taps != 1 && taps != 9)) return p;
    const int nb = taps == 1 && Cout % 128 == 0 ? 128 : 64, cb = taps == 1 && Cin % 128 == 0 ? 128 : 64;
    const int ntiles = taps == 9 ? B * (H / 8) * (W / 16) : (M + 127) / 128;
    if (taps == 9 && (H % 8 || W % 16 || ntiles < 48)) return p;
    if (taps == 1 && ntiles < t.wgrad_min1) return p;          // (3: also the 16x16 ... 4x4 levels: 6.90 vs 6.97 ms (96))
    p.path = PA_WGP_TILE; p.nb = nb; p.cb = cb; p.ntiles = ntiles; p.blocks = (Cout / nb) * (Cin / cb);
    // alone: one workgroup per CU (<= 256 workgroups: the fp32 slabs grow with the workgroup count)
    int s = (taps == 9 ? t.wgrad_wgs9 : t.wgrad_wgs1) / p.blocks;
    p.splits = pa_wgrad_balanced(ntiles, s < 1 ? 1 : s > ntiles ? ntiles : s);
    if (!t.wg_group) return p;
    // as a job of a group launch: a WORKGROUP budget per job (64 each: three jobs of a residual block stay below the 256-workgroup cap of a
    // group launch, Net::launch_pending_wgrads -- 5.91 vs 5.98 ms for 96 / 128 without a cap), at least minper tiles per workgroup
    s = (taps == 9 ? t.wg_group_wgs9 : t.wg_group_wgs1) / p.blocks;
    const int minper = taps == 9 ? t.wg_group_minper9 : t.wg_group_minper1;
    if (s * minper > ntiles) s = ntiles / minper;
    p.group_splits = pa_wgrad_balanced(ntiles, s < 1 ? 1 : s);
    p.group_kind = taps == 9 ? PA_WGK_9_44 : nb == 128 ? (cb == 128 ? PA_WGK_1_44 : PA_WGK_1_42) : (cb == 128 ? PA_WGK_1_24 : PA_WGK_1_22);
    return p;
}

// the slab count a layer is laid out with: the grouped one where its launches can be jobs of a group (as_job: the layer's batch and map
// are known at layout time) and the grouped kernel takes the shape, else the count of the layer launched alone
inline int pa_wgrad_layer_splits(const PaWgradPlan& p, bool as_job) { return as_job && p.group_splits > 0 ? p.group_splits : p.splits; }

// a launch into `splits` slabs, the count the layer was laid out with, with (bias_grad) or without the bias-gradient partials: a tile kernel
// that cannot run with that count, or a 3x3 launch with a bias gradient (the 144-accumulator body has none), goes to the generic kernel
inline PaWgradPlan pa_wgrad_launch_plan(int B, int H, int W, int Cin, int Cout, int taps, bool stem, int splits, bool bias_grad) {
    const PaWgradPlan p = pa_wgrad_plan(B, H, W, Cin, Cout, taps, stem);
    const bool refused = splits < 1 || splits > p.ntiles || (taps == 9 && bias_grad);
    return (p.path == PA_WGP_TILE || p.path == PA_WGP_STEM_TILE) && refused ? pa_wgrad_generic_plan(B * H * W, Cin, Cout, taps, stem) : p;
}
