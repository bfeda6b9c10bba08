// The switches of the tuning build (PA_TUNING=1 bash build.sh -> -DPA_TUNING), ONE table.
// The release library reads no environment at all: pa_tuning() is a constant there and every switch below folds to its
// release value.  A tuning build fills the table from the environment once, on the first call.  All values are integers
// (PA_X=0 is "off" for the on/off switches as well).
#pragma once
#include <stdlib.h>

//   field, environment name, release value, meaning
#define PA_TUNING_TABLE(X)                                                                                                           \
    /* bisecting switches: force an already-tested generic path */                                                                  \
    X(conv1_old,        "PA_CONV1_OLD",        0,   "1x1 convolutions on the generic kernel (no row-tile kernel, no fused upsample-add gradient)") \
    X(conv3_old,        "PA_CONV3_OLD",        0,   "3x3 convolutions on the generic kernel (no halo-tile kernel)")                 \
    X(wgrad_old,        "PA_WGRAD_OLD",        0,   "weight gradients on the generic kernel (no tile kernel, stem included)")       \
    X(stem_wgrad_old,   "PA_STEM_WGRAD_OLD",   0,   "the stem's weight gradient on the generic kernel")                            \
    X(eltwise_old,      "PA_ELTWISE_OLD",      0,   "pooling / upsample-add / cell-mask launches in their first, unvectorised form") \
    X(conv3_nosmall,    "PA_CONV3_NOSMALL",    0,   "no 8 x 8 / 4 x 4 halo tiles: the small maps go to the generic kernel")        \
    X(igemm_oneshot,    "PA_IGEMM_ONESHOT",    1,   "0: the small 1x1 layers on the K-stepping generic kernel instead of the one-shot one") \
    X(no_dz3,           "PA_NO_DZ3",           0,   "conv3's data gradient does not store dz3 (its readers recompute it)")         \
    X(no_dz2,           "PA_NO_DZ2",           0,   "conv2's data gradient does not store dz2")                                    \
    X(epi_bwd_direct,   "PA_EPI_BWD_DIRECT",   0,   "direct (no LDS) BatchNorm-backward epilogue wherever an instance carries both") \
    X(conv3_noxcd,      "PA_CONV3_NOXCD",      0,   "3x3 tiles in launch order instead of one contiguous range per XCD")           \
    X(wg_group,         "PA_WG_GROUP",         1,   "0: one launch per weight gradient instead of group launches")                 \
    X(wg_red_in_group,  "PA_WG_RED_IN_GROUP",  1,   "0: slab reductions as launches of their own instead of inside the next group launch") \
    X(wgrad_anyorder,   "PA_WGRAD_ANYORDER",   1,   "0: ungrouped weight gradients of one flush as ordinary in-order launches")    \
    X(wgrad_nopipe,     "PA_WGRAD_NOPIPE",     0,   "plain instead of pipelined tile weight gradients")                            \
    X(upadd_fuse,       "PA_UPADD_FUSE",       1,   "0: the upsample-add backward's low-resolution half as a launch of its own")   \
    X(upadd_split,      "PA_UPADD_SPLIT",      1,   "0: both halves of the upsample-add backward in one launch on the main stream") \
    X(pool_route,       "PA_POOL_ROUTE",       3,   "pool gradients through the forward pools' arg-max maps: bit 0 the hourglass pools, bit 1 the stem's pool (0: a pool backward launch each)") \
    X(fin_prologue,     "PA_FIN_PROLOGUE",     128, "most partial rows a consumer finalizes in its prologue (0: always a finalize launch; at most 128)") \
    X(fin_mask,         "PA_FIN_MASK",         7,   "which finalizes may ride in a consumer: 1 forward x1 / x2, 2 backward x2, 4 backward x3") \
    X(single_stream,    "PA_SINGLE_STREAM",    0,   "everything on the caller's stream")                                           \
    X(no_wstream,       "PA_NO_WSTREAM",       0,   "side streams, but the weight gradients on the stream that produced their operands") \
    X(stem_on_main,     "PA_STEM_ON_MAIN",     1,   "0: the stem's weight gradient on the weight-gradient stream")                 \
    /* policy numbers (tests/conv_exact.py mirrors the release values) */                                                          \
    X(wgrad_wgs1,       "PA_WGRAD_WGS1",       256, "workgroup target of a 1x1 tile weight gradient launched alone")               \
    X(wgrad_wgs9,       "PA_WGRAD_WGS9",       256, "the same for 3x3")                                                            \
    X(wgrad_min1,       "PA_WGRAD_MIN1",       3,   "fewest 128-pixel tiles for which a 1x1 weight gradient takes the tile kernel") \
    X(wg_group_wgs1,    "PA_WG_GROUP_WGS1",    64,  "workgroup budget of a 1x1 job of a group launch")                             \
    X(wg_group_wgs9,    "PA_WG_GROUP_WGS9",    64,  "the same for 3x3")                                                            \
    X(wg_group_minper1, "PA_WG_GROUP_MINPER1", 2,   "fewest tiles per workgroup of a 1x1 job")                                     \
    X(wg_group_minper9, "PA_WG_GROUP_MINPER9", 4,   "the same for 3x3")                                                            \
    X(wg_group_cap,     "PA_WG_GROUP_CAP",     256, "most workgroups of one group launch")                                         \
    X(wg_red_wgs,       "PA_WG_RED_WGS",       256, "workgroups of the slab reduction inside a group launch")                      \
    X(wreduce_lag,      "PA_WREDUCE_LAG",      2,   "flushes whose slabs wait in the stash before they are summed")                \
    X(stem_splits,      "PA_STEM_SPLITS",      512, "splits (slabs) of the stem's weight gradient")                                \
    X(wgrad_tile1,      "PA_WGRAD_TILE1",      0,   "generic 1x1 weight gradient: forced tile variant (0: by shape)")              \
    X(wgrad_tile9,      "PA_WGRAD_TILE9",      0,   "the same for 3x3")                                                            \
    X(wgrad_blocks,     "PA_WGRAD_BLOCKS",     0,   "generic weight gradient: forced split count (0: by shape)")                   \
    /* instruments: WRONG RESULTS or timing only */                                                                                \
    X(ablate,           "PA_ABLATE",           0,   "INSTRUMENT, wrong results: mask of launch classes that are skipped (net.hip)") \
    X(ablate_h,         "PA_ABLATE_H",         8,   "INSTRUMENT: largest map height the low-resolution bits of PA_ABLATE skip")    \
    X(conv3_dbg,        "PA_CONV3_DBG",        0,   "INSTRUMENT, wrong results: phase ablation / tap rotation / cycle stamps of the 3x3 tile kernel") \
    X(conv1_dbg,        "PA_CONV1_DBG",        0,   "INSTRUMENT, timing only: cycle stamps of the one-shot 1x1 kernel")            \
    X(conv1t_dbg,       "PA_CONV1T_DBG",       0,   "INSTRUMENT, timing only: cycle stamps of the row-tile 1x1 kernel")            \
    X(fin_anyorder,     "PA_FIN_ANYORDER",     0,   "INSTRUMENT, results may be wrong: finalize launches without ordering behind their producer")

struct PaTuning {
#define PA_TUNING_FIELD(field, env, value, doc) int field = value;
    PA_TUNING_TABLE(PA_TUNING_FIELD)
#undef PA_TUNING_FIELD
};

#ifdef PA_TUNING
inline const PaTuning& pa_tuning() {
    static const PaTuning t = [] {
        PaTuning v;
#define PA_TUNING_READ(field, env, value, doc) if (const char* e = getenv(env)) v.field = atoi(e);
        PA_TUNING_TABLE(PA_TUNING_READ)
#undef PA_TUNING_READ
        return v;
    }();
    return t;
}
#else
inline const PaTuning& pa_tuning() {
    static constexpr PaTuning t{};
    return t;
}
#endif
