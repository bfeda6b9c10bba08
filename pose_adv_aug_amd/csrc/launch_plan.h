// Launch geometry of the streaming kernels of elementwise.hip (2x2 max pool, nearest-upsample + add, their backward passes, epilogue
// application, cell mask), decided in ONE place.  Host code only; no HIP types.
//
// The contract every one of those kernels rests on:
//   - a thread keeps the 8-channel group threadIdx.x % (C / 8) over its whole walk: the workgroup size is a multiple of C / 8;
//   - flush_stats reduces the lanes of a wave that share a group by xor shuffles: with a statistics epilogue C / 8 is a power of two
//     <= 64 (one wave wide);
//   - the streaming (row-walk) forms need blockDim and the items of a map row, (W / 2) * (C / 8), to divide one another, even H and W,
//     and 32-bit element offsets, B * H * W * C < 2^31.  Shapes outside go to the generic kernels.
#pragma once
#include <stddef.h>
#include "tuning.h"

void pa_set_error_msg(const char* msg);

// C / 8 a power of two <= 64: what a statistics epilogue needs.  The networks (chan % 128 == 0) are left with 128, 256 and 512.
inline bool pa_stats_groups_ok(int C) {
    const int CG = C / 8;
    return C > 0 && C % 8 == 0 && CG <= 64 && (CG & (CG - 1)) == 0;
}
#define PA_STATS_GROUPS_MSG "C / 8 (chan / 8) must be a power of two <= 64 -- chan 128, 256 or 512 for the networks: the per-channel reductions are shuffled inside one wave"

// workgroups of a grid-stride launch: one per `per_block` items, between 1 and `cap`
inline int pa_grid_for(size_t total, size_t per_block, size_t cap) {
    const size_t b = (total + per_block - 1) / per_block;
    return (int)(b > cap ? cap : b < 1 ? 1 : b);
}

enum PaEltKind {
    PA_ELT_FWD,          // max pool / upsample-add forward: 256 threads, no reductions
    PA_ELT_POOL_BWD,     // max pool backward
    PA_ELT_UPADD_BWD,    // upsample-add backward
    PA_ELT_APPLY,        // epilogue application (no streaming form)
    PA_ELT_MASK          // cell mask (no streaming form)
};

struct PaEltPlan {
    int blocks, threads;     // blocks = partial-statistics rows: it fixes the summation order of the reductions
    size_t lds;              // dynamic LDS bytes of the kernel that `streaming` selects
    bool streaming;          // the row-walk kernel takes the shape (false: the generic kernel)
};

// items: (low-resolution) pixels x channel groups the launch walks; B, H, W: the high-resolution map (0 for the kinds without a streaming
// form); stats: the launch carries a statistics epilogue; want_stream: the launcher's own mode checks admit the streaming kernel.
// Returns 0 and fills `p`, or 1 with the message set.
inline int pa_elt_plan(PaEltPlan& p, PaEltKind kind, size_t items, int B, int H, int W, int C, bool stats, bool want_stream) {
    if (C < 8 || C % 8 != 0) { pa_set_error_msg("streaming launch: C must be a multiple of 8 (16-byte accesses)"); return 1; }
    const int CG = C / 8;
    if (stats && !pa_stats_groups_ok(C)) { pa_set_error_msg("streaming launch with a statistics epilogue: " PA_STATS_GROUPS_MSG); return 1; }
    if (CG > 1024) { pa_set_error_msg("streaming launch: C / 8 exceeds the workgroup size"); return 1; }
    const bool fwd = kind == PA_ELT_FWD;
    // One partial-statistics row per workgroup (<= 512 rows), so big tensors get larger workgroups: 512 of them still keep enough loads in
    // flight (256-thread ones, measured ALONE, left HBM half idle: 3.3 TB/s vs 6+ TB/s for a plain copy of the same size).  512 threads, not
    // 1024 (6.465 vs 6.434 ms per step over three interleaved pairs): a 1024-thread workgroup needs a whole CU's wave slots at once next
    // to the other queues' kernels; 512 workgroups x 512 threads x 9 loads of 16 bytes are still 38 MB in flight.
    int threads = !fwd && items >= (size_t)512 * 1024 ? 512 : 256;
    // 256 / 512 serve every power of two; otherwise the largest multiple of C / 8 below (C = 24: 255, 384: 240)
    if (threads % CG != 0) threads = CG > threads ? CG : threads / CG * CG;
    p.blocks = pa_grid_for(items, threads, fwd ? 4096 : 512);
    p.threads = threads;
    // The row walk: the forward kernels are built for 256 threads at the most and take the shape or not.  The backward launches try 512 / 256
    // where the first choice does not fit (96 x 96 maps of the 384 x 384 configuration: 1536 items per row) and 384 / 192 / 128 (its
    // 24 x 24 and 12 x 12 maps: 12 / 6 low-resolution pixels x 32 channel groups per row), and keep the fitted size for the generic kernel
    // too.  `blocks` stays as first computed: the walk strides over rows, and the number of partial rows is part of the results' bits.
    bool fits = false;
    if (W >= 2 && (kind == PA_ELT_FWD || kind == PA_ELT_POOL_BWD || kind == PA_ELT_UPADD_BWD)) {
        const size_t row_items = (size_t)(W / 2) * CG;
        const int tries[] = {threads, 512, 256, 384, 192, 128};
        for (int i = 0; i < (fwd ? 1 : 6) && !fits; ++i) {
            const int t = tries[i];
            if (t % CG == 0 && (row_items % t == 0 || t % row_items == 0) && !(fwd && t > 256)) { p.threads = t; fits = true; }
        }
    }
    p.streaming = fits && want_stream && !pa_tuning().eltwise_old && H % 2 == 0 && W % 2 == 0 && (size_t)B * H * W * C < ((size_t)1 << 31);
    // one row of 2 * C floats per wave for flush_stats (a plain cell mask never reaches it), then the constant tables of the streaming
    // backward kernels: float4 {scale, shift, mean, invstd} + float2 {k0, k1} (pool), two float4 tables (upsample-add)
    const size_t rows = (size_t)((p.threads + 63) / 64) * 2 * C * sizeof(float);
    p.lds = fwd || (kind == PA_ELT_MASK && !stats) ? 0 : rows;
    if (p.streaming && kind == PA_ELT_POOL_BWD) p.lds += (size_t)C * 24;
    if (p.streaming && kind == PA_ELT_UPADD_BWD) p.lds += (size_t)C * 32;
    return 0;
}
