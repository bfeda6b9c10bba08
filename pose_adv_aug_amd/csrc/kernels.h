// Host-side launch interface of the HIP kernels (internal; the public C ABI is include/poseadv.h).
#pragma once
#include "common.h"
#include "bn_fin.h"
#include "launch_plan.h"
#include "wgrad_plan.h"
#include "conv_plan.h"

struct PaConvArgs {
    PaOperand in;        // [B][H][W][Cin] NHWC bf16
    const bf16* w;       // [Cout][taps*Cin] bf16 (tap-major, channel-minor)
    const float* bias;   // [Cout] or nullptr
    PaOperand add1;      // optional epilogue addends over [M][Cout]
    PaOperand add2;
    PaEpilogue ep;
    bf16* out;           // [M][Cout]
    int B, H, W, Cin, Cout, taps;
    bf16* dz_out;        // optional (tile kernels, LIN2 input; PaConvPlan::stores_dz): the transformed input tile is also stored here [M][Cin] --
                         // later consumers of the same BatchNorm-backward gradient read ONE tensor instead of recomputing it from two
    PaBnFin fin;         // pending BatchNorm finalize of `in`, done in the kernel's prologue (fin.rows > 0; only launches whose plan says takes_fin)
    int low_prio;        // != 0: a launch of a side branch (skip blocks beside the main chain): the kernel keeps wave priority 0 instead of PA_MAIN_PRIO
    int dbg;             // tuning builds only (0 in the release library): conv3x3_tile.hip phase ablation bits 1 / 2 / 4, bit 8 = per-workgroup tap rotation
    int xcd;             // set by the launchers from the plan: bit 0: workgroup i works on tile (i % 8) * (tiles / 8) + i / 8 (one contiguous range per XCD)
    // round 6 -- the LOW half of the upsample-add backward (reference models/asn_stacked_hg.py:192-203) folded into the 1x1 data gradient that
    // produces d(merged) (conv_plan.h: PA_CVP_ROW_UP): besides `out` = d(merged) [B][H][W][Cout] the launch stores
    // out2 [B][H/2][W/2][Cout] = ep2(sum of the 2x2 block of d(merged)) with ep2's BatchNorm-backward mask and its two partial reductions
    PaEpilogue ep2;
    bf16* out2;          // nullptr = off
};
// Which instance takes a launch, its grid, its partial rows and what it can carry: conv_plan.h ONLY.  pa_conv_shape: the planner's input of a launch
int pa_conv_cus();       // compute units of the current device, asked once (0: unknown)
inline PaConvShape pa_conv_shape(const PaConvArgs& a) {
    return PaConvShape{a.B, a.H, a.W, a.Cin, a.Cout, a.taps, a.in.mode, a.add1.mode, a.add2.mode, a.ep.mode, a.ep2.mode, a.fin.rows, a.bias != nullptr,
                       a.out2 != nullptr, a.dz_out != nullptr, a.in.map != nullptr, a.in.q != nullptr, a.ep2.scale && a.ep2.shift, a.add2.map != nullptr,
                       pa_conv_cus()};
}
// Plans the launch (or takes the caller's plan of the same arguments) and runs the plan's instance; refused: message set, 1.  stat_rows: PaConvPlan::rows
int pa_launch_conv(const PaConvArgs& a, const PaConvPlan& p, hipStream_t st, int* stat_rows = nullptr);
inline int pa_launch_conv(const PaConvArgs& a, hipStream_t st, int* stat_rows = nullptr) { return pa_launch_conv(a, pa_conv_plan(pa_conv_shape(a)), st, stat_rows); }
// the tile kernels, called by pa_launch_conv with the plan that chose them: halo-tile 3x3 (conv3x3_tile.hip), row-tile 1x1 (conv1x1_tile.hip)
int pa_launch_conv3x3_tile(const PaConvArgs& a, const PaConvPlan& p, hipStream_t st);
int pa_launch_conv1x1_tile(const PaConvArgs& a, const PaConvPlan& p, hipStream_t st);
// upper bound of stat rows any conv / elementwise launch writes for a tensor with M pixels
inline int pa_max_stat_rows(int M) { int r = (M + 63) / 64; return r < 512 ? 512 : r; }

// Weight gradient: dw[n][tap][c] = sum_m dy(m)[n] * x(pixel(m)+tap)[c], split over m into `splits`
// deterministic partial slabs part[split][Cout][taps*Cin] (fp32); optional bias-gradient partials
// dbpart[split][Cout] (column sums of dy).
struct PaWgradArgs {
    PaOperand dy;        // [M][Cout]  (PLAIN or LIN2)
    PaOperand x;         // [B][H][W][Cin] (PLAIN or BNRELU)
    float* part;
    float* dbpart;       // or nullptr
    int B, H, W, Cin, Cout, taps, splits;
};
// kernel, channel blocks, tiles and slab counts: wgrad_plan.h (pa_wgrad_layer_splits set `splits` at layout time, pa_wgrad_launch_plan at launch)
int pa_launch_wgrad(const PaWgradArgs& a, hipStream_t st);
// tile kernels (conv_wgrad_tile.hip), called by pa_launch_wgrad / pa_launch_stem_wgrad with the plan that chose them
int pa_launch_stem_wgrad_tile(const PaWgradArgs& a, const PaWgradPlan& p, hipStream_t st);
int pa_launch_wgrad_tile(const PaWgradArgs& a, const PaWgradPlan& p, hipStream_t st);
// several independent weight gradients in one launch (conv_wgrad_tile.hip): workgroups of this launch as a job (0: it cannot be one -- slab
// count, tile shape or operand modes the grouped kernel does not take), launch n <= 8 jobs
int pa_wgrad_job_workgroups(const PaWgradArgs& a);
struct PaWgradReduceJob;
// keep_order: jobs in the caller's order (default: longest first); red_*: red_n <= PA_RED_LIST_MAX entries of the reduce table whose slabs
// (complete on `st` before this launch) are summed by a few more workgroups of the same launch
int pa_launch_wgrad_group(const PaWgradArgs* const* jobs, int n, hipStream_t st, bool keep_order = false,
                          const PaWgradReduceJob* red_jobs = nullptr, const int* red_idx = nullptr, int red_n = 0);
void pa_wgrad_set_launch_flags(unsigned flags);      // hipExtAnyOrderLaunch for the tile weight gradients launched next by this thread (0 = in-order)

// reduce partial slabs into the fp32 gradient in PyTorch layout  dst[n][c][tap]  (real_cin/real_cout
// select the un-padded sub-block for the 16-channel head layers)
struct PaWgradReduceJob {
    const float* part; float* dst; const float* dbpart; float* dbdst;
    int Cout, Cin, taps, splits, real_cout, real_cin;
};
int pa_launch_wgrad_reduce(const PaWgradReduceJob* jobs_dev, int njobs, int max_elems, hipStream_t st);
#define PA_RED_LIST_MAX 24
struct PaRedList { int idx[PA_RED_LIST_MAX]; };
int pa_launch_wgrad_reduce_list(const PaWgradReduceJob* jobs_dev, const int* idx, int n, int max_elems, hipStream_t st);      // any n <= 24 jobs of the table

// ---- BatchNorm bookkeeping
// the finalize as a launch of its own, described by PaBnFin (bn_fin.h) like the consumer-prologue form, over C (even) channels: forward
// (rows of sum, sumsq -> scale/shift/mean/invstd, running stats update) or backward (rows of sum dz, sum dz*xhat -> LIN2 coefficients, dgamma, dbeta)
int pa_launch_bn_fin(const PaBnFin& f, int C, hipStream_t st);
int pa_launch_bn_fin2(const PaBnFin& a, int Ca, const PaBnFin& b, int Cb, hipStream_t st);      // two backward finalizes in one launch
// eval: scale/shift from running stats, for `n` BatchNorms described by a device table
struct PaBnEvalJob { const float* gamma; const float* beta; const float* rmean; const float* rvar; float* scale; float* shift; int C; };
int pa_launch_bn_eval(const PaBnEvalJob* jobs_dev, int njobs, float eps, hipStream_t st);

// ---- pooling / upsampling (NHWC bf16).  These launches, pa_launch_ep_apply and pa_launch_cell_mask take their geometry from pa_elt_plan
// (launch_plan.h), which also refuses what the kernels cannot do: a statistics epilogue needs C / 8 a power of two <= 64
// map (optional, [B][H/2][W/2][C] bytes): the arg-max position 2 * row + col of every pooled element (first maximum in scan order, the rule of
// pa_launch_maxpool_bwd); nullptr = do not write
// xmax (optional, with map, like out): the RAW input value at the arg-max (streaming kernel, BatchNorm + ReLU input only)
int pa_launch_maxpool_fwd(const PaOperand& in, bf16* out, int B, int H, int W, int C, hipStream_t st, unsigned char* map = nullptr, bf16* xmax = nullptr);
// The partial rows of pa_launch_maxpool_bwd(dout, in, none, ep, ...) with a BatchNorm-backward epilogue on the pooled tensor itself, same bits,
// from dout and xmax alone (a quarter of the traffic, no output): for a pool whose routed gradient is formed by its reader
// (PaConvPlan::pool_in).  supported: both launches of the pool take their streaming kernels.
bool pa_pool_stats_route_supported(const PaOperand& in, const PaEpilogue& ep, int B, int H, int W, int C);
int pa_launch_maxpool_bwd_stats(const bf16* dout, const bf16* xmax, const PaOperand& in, const PaEpilogue& ep, int B, int H, int W, int C,
                                hipStream_t st, int* stat_rows = nullptr);
// grad of 2x2 max pool routed to the arg-max (first max in scan order), + optional addend, then epilogue
int pa_launch_maxpool_bwd(const bf16* dout, const PaOperand& in, const PaOperand& add, const PaEpilogue& ep, bf16* din,
                          int B, int H, int W, int C, hipStream_t st, int* stat_rows = nullptr);
// out = nearest_up2(low) + skip        (low: [B][H/2][W/2][C], skip/out: [B][H][W][C])
int pa_launch_upadd_fwd(const PaOperand& low, const PaOperand& skip, bf16* out, int B, int H, int W, int C, hipStream_t st);
// part: 3 = both outputs in one launch; 1 = dlow only, 2 = dskip only (two launches on two streams: pa_upadd_bwd_splits() says whether the
// streaming kernel, the only one with the one-output forms, takes the shape)
int pa_launch_upadd_bwd(const bf16* dout, const PaEpilogue& ep_low, bf16* dlow, const PaEpilogue& ep_skip, bf16* dskip,
                        int B, int H, int W, int C, hipStream_t st, int* stat_rows = nullptr, int part = 3);
bool pa_upadd_bwd_splits(const PaEpilogue& ep_low, const PaEpilogue& ep_skip, int B, int H, int W, int C);

// ---- stem 7x7 stride-2 conv as a K=256 GEMM over the 4-channel-padded NHWC bf16 image
// (in.p / x.p = img4 [B][2H][2W][4], Cin = 256 virtual patch length, Cout = 64, H/W = OUTPUT dims)
int pa_launch_stem_conv(const PaConvArgs& a, hipStream_t st, int* stat_rows = nullptr);
int pa_launch_stem_wgrad(const PaWgradArgs& a, hipStream_t st);
// reduce the stem's partial slabs [splits][64][256] into PyTorch layout dst[64][3][7][7]
int pa_launch_stem_wgrad_reduce(const float* part, int splits, float* dst, hipStream_t st, float* zero64 = nullptr);      // zero64: 64 floats the launch also clears (the stem's bias gradient)

// data gradient of the stem (stem_dgrad.hip): d loss / d image from the gradient at the RAW stem output
struct PaStemDgradArgs {
    PaOperand g;         // [B][Hm][Wm][64] (PLAIN or LIN2: the BatchNorm backward on load, rounded once to the storage type)
    const bf16* wf;      // the stem's packed forward copy [64][256]: wf[n][ky*32 + kx*4 + c]
    float* out;          // fp32, 16-byte aligned, fully overwritten; layout 0: [B][3][2Hm][2Wm], 1: [B][2Hm][2Wm][4] (4th float 0)
    int B, Hm, Wm, layout;
    float scale;         // the fp32 result is multiplied by this (1 / PA_GRAD_SCALE in the net: a power of two, exact)
};
int pa_launch_stem_dgrad(const PaStemDgradArgs& a, hipStream_t st);
int pa_launch_stem_pack(const float* w, bf16* wf, hipStream_t st);      // fp32 [64][3][7][7] -> wf as above

// ---- optimizer / weight preparation
int pa_launch_rmsprop(float* p, const float* g, float* v, size_t n, float lr, float alpha, float eps, float gscale, int* state, hipStream_t st);   // state: the optimizer's own {flag, skipped} device pair or NULL (process-wide pair)
// the step with torch.optim.RMSprop's other options (momentum buffer iff mom > 0, grad_avg iff centered) and an optional clip coefficient
// read from the device; all off and clip_coef NULL: the launch of pa_launch_rmsprop.  state as above, never NULL in the half-precision build.
struct PaRmspropOpts { float lr, alpha, eps, mom, wd; };
int pa_launch_rmsprop_opts(const PaRmspropOpts& o, bool centered, float* p, const float* g, float* v, float* buf, float* ga, size_t n,
                           float gscale, const float* clip_coef, int* state, hipStream_t st);
// out2 = {norm of gscale * g, fminf(1, max_norm / (norm + 1e-6f))}: two deterministic launches, double partial sums in workspace
size_t pa_grad_norm_workspace_size(size_t n);
int pa_launch_grad_norm(const float* g, size_t n, float gscale, float max_norm, void* workspace, float* out2, hipStream_t st);
// torch.optim.Adam / AdamW step (elementwise.hip).  decay: 0 none, 1 coupled (gr += wd p), 2 decoupled (p *= c_dec); om_b1 / om_b2 =
// 1.f - beta in fp32.  PaAdamState is pa_adam_state of include/poseadv.h: a one-thread prologue advances step and writes the four
// constants (or counts a skipped step when flag is set), the step kernel reads flag, bc2s and step_size from it.
struct PaAdamOpts { float lr, beta1, beta2, eps, wd, c_dec, om_b1, om_b2; };
struct PaAdamState { int flag, skipped, step, reserved; float bc1, bc2, step_size, bc2s; };
int pa_launch_adam(const PaAdamOpts& o, bool amsgrad, int decay, float* p, const float* g, float* m, float* v, float* vmax, size_t n,
                   float gscale, const float* clip_coef, PaAdamState* state, hipStream_t st);
int pa_adam_read_steps(const PaAdamState* state, long long* steps, long long* skipped, hipStream_t st);
int pa_launch_adam_set_steps(PaAdamState* state, int steps, hipStream_t st);
// Parameter groups (elementwise.hip): chunk_map[i / 4] = group of the 16-byte chunk of element i; the table of PA_OPT_GROUPS entries goes
// to the kernels by value (256 bytes).  c_dec = (float)(1.0 - (double)lr * (double)wd); entries at and above ngroups: frozen = 1.
// One group that is not frozen: the launches of the calls above.  excluded: bit k set = group k adds nothing to the norm.
constexpr int PA_OPT_GROUPS = 16;
struct PaOptGroupK { float lr, wd, c_dec; int frozen; };
struct PaOptGroupTable { PaOptGroupK g[PA_OPT_GROUPS]; };
int pa_launch_rmsprop_groups(const PaRmspropOpts& o, bool centered, const PaOptGroupTable& tab, int ngroups, const unsigned char* map,
                             float* p, const float* g, float* v, float* buf, float* ga, size_t n, float gscale, const float* clip_coef,
                             int* state, hipStream_t st);
int pa_launch_adam_groups(const PaAdamOpts& o, bool amsgrad, bool decoupled, const PaOptGroupTable& tab, int ngroups, const unsigned char* map,
                          float* group_consts, float* p, const float* g, float* m, float* v, float* vmax, size_t n, float gscale,
                          const float* clip_coef, PaAdamState* state, hipStream_t st);
int pa_launch_grad_norm_groups(const float* g, size_t n, const unsigned char* map, unsigned excluded, float gscale, float max_norm,
                               void* workspace, float* out2, hipStream_t st);
// Layer-wise trust ratios (opt_layerwise.hip): LAMB, LARS / SGD and per-tensor norms over a SEGMENT list.  PaOptSegment is
// pa_opt_segment of include/poseadv.h (chunk0 = first float / 4; a segment lies inside one tensor and covers no padding); one wave works
// on one segment, PA_LW_WAVES segments per 256-thread workgroup.  workspace: two double partial sums per segment.  norms: [2][ntensors]
// floats (W, then U or G); trust: ntensors floats.  The group table travels by value as above and is staged in LDS.
struct PaOptSegment { unsigned chunk0, nfloats; int tensor, group; };
constexpr int PA_LW_WAVES = 4;
struct PaLambOpts { float beta1, beta2, eps, om_b1, om_b2, max_trust; int always_adapt; };
struct PaLarsOpts { float mom, trust_coef, lars_eps; int nesterov, always_adapt; };
size_t pa_opt_layer_workspace_size(size_t nsegs, int ntensors);
int pa_launch_tensor_norms(const float* x, const PaOptSegment* segs, size_t nsegs, int ntensors, float scale, void* workspace, float* norms,
                           hipStream_t st);
int pa_launch_lamb(const PaLambOpts& o, const PaOptGroupTable& tab, const PaOptSegment* segs, size_t nsegs, int ntensors, float* p,
                   const float* g, float* m, float* v, size_t n, float gscale, const float* clip_coef, void* workspace, float* norms,
                   float* trust, PaAdamState* state, hipStream_t st);
int pa_launch_lars(const PaLarsOpts& o, const PaOptGroupTable& tab, const PaOptSegment* segs, size_t nsegs, int ntensors, float* p,
                   const float* g, float* buf, size_t n, float gscale, const float* clip_coef, void* workspace, float* norms, float* trust,
                   int* state, hipStream_t st);
int pa_launch_loss_out(float* acc, float* keep, float* out, float* total, int n, hipStream_t st);      // per-stack losses + their sum out, accumulators cleared
int pa_launch_copy16(void* dst, const void* src, size_t bytes, hipStream_t st, int form = 0);      // plain 16-B/lane streaming copy (bandwidth calibration)
int pa_rmsprop_skipped(const int* state, long long* out, hipStream_t st);     // half-precision build: steps skipped for a non-finite gradient
struct PaPrepJob { const float* w; bf16* wf; bf16* wb; int Cout, Cin, taps, pad_cout, pad_cin; };
int pa_launch_weight_prep(const PaPrepJob* jobs_dev, int njobs, int max_elems, hipStream_t st);

// ---- layout helpers
int pa_launch_nchw_to_nhwc4(const float* src, bf16* dst, int B, int H, int W, hipStream_t st);
int pa_launch_nhwc_to_nchw_f32(const float* src, float* dst, int B, int H, int W, int C, hipStream_t st);
int pa_launch_nchw_f32_to_nhwc_bf16(const float* src, bf16* dst, int B, int C, int H, int W, hipStream_t st);
int pa_launch_nhwc_bf16_to_nchw_f32(const PaOperand& src, float* dst, int B, int C, int H, int W, hipStream_t st);

int pa_launch_cell_mask(const PaOperand& x, const float* mask, const PaEpilogue& ep, bf16* out, int B, int H, int W, int C,
                        hipStream_t st);
int pa_launch_ep_apply(const PaOperand& g, const PaEpilogue& ep, bf16* out, size_t M, int C, hipStream_t st, int* stat_rows = nullptr);
int pa_launch_fill(float* p, float v, size_t n, hipStream_t st);
