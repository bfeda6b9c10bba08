// extern "C" boundary of libposeadv_hip.so (declared in include/poseadv.h).
#include "../../include/poseadv.h"
#include "net.h"
#include "warp_bwd.h"
#include "soft_argmax.h"
#include "ema.h"
#include "grad_accum.h"
#include <stdio.h>
#include <string.h>
#include <new>
#include <string>

static thread_local char g_err[1024] = "";
void pa_set_error(const char* what, hipError_t e, const char* file, int line) {
    snprintf(g_err, sizeof g_err, "%s:%d: %s -> %s", file, line, what, hipGetErrorString(e));
}
void pa_set_error_msg(const char* msg) { snprintf(g_err, sizeof g_err, "%s", msg); }

struct pa_net { Net n; };
#define ST(s) reinterpret_cast<hipStream_t>(s)
#undef TRY       // (net.h's plain form; at the C boundary a failure also leaves a message)
#define TRY(x) do { int _r = (x); if (_r) { if (!g_err[0]) pa_set_error("kernel launch", (hipError_t)_r, __FILE__, __LINE__); return _r; } } while (0)
// argument checks of the pose-library operators: decided on the host before any device call, the message names the argument
#define NEED_PTR(fn, p) do { if (!(p)) { pa_set_error_msg(fn ": " #p " is NULL"); return 1; } } while (0)
#define NEED_POS(fn, v) do { if ((v) < 1) { pa_set_error_msg(fn ": " #v " must be >= 1"); return 1; } } while (0)

extern "C" {

const char* pa_last_error(void) { return g_err; }
float pa_grad_scale(void) { return PA_GRAD_SCALE; }
int pa_dtype(void) { return PA_DTYPE_ID; }
int pa_version(void) { return 1; }

int pa_gaussian_heatmap(const double* pts, float* out, int B, int J, int H, int W, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_gaussian_heatmap", pts); NEED_PTR("pa_gaussian_heatmap", out);
    NEED_POS("pa_gaussian_heatmap", B); NEED_POS("pa_gaussian_heatmap", J); NEED_POS("pa_gaussian_heatmap", H); NEED_POS("pa_gaussian_heatmap", W);
    TRY(pa_launch_gaussian_heatmap(pts, out, B, J, H, W, ST(s))); return 0;
}
int pa_weighted_l2(const float* pred, const float* gt, const float* weight, size_t n, float* loss, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_weighted_l2", pred); NEED_PTR("pa_weighted_l2", gt); NEED_PTR("pa_weighted_l2", loss);
    if (n == 0) { pa_set_error_msg("pa_weighted_l2: n must be >= 1"); return 1; }
    TRY(pa_launch_weighted_l2(pred, gt, weight, n, loss, ST(s))); return 0;
}
int pa_get_preds(const float* maps, int B, int J, int H, int W, float* preds, float* maxval, void* s) {
    TRY(pa_launch_argmax(maps, (long)J * H * W, (long)H * W, 1, B, J, H, W, preds, maxval, ST(s))); return 0;
}
int pa_final_preds(const float* maps, const float* center, const float* scale, const float* rot, int B, int J, int H, int W,
                   float* out, float* scratch_preds, void* s) {
    TRY(pa_launch_argmax(maps, (long)J * H * W, (long)H * W, 1, B, J, H, W, scratch_preds, nullptr, ST(s)));
    TRY(pa_launch_final_preds(maps, (long)J * H * W, (long)H * W, 1, scratch_preds, center, scale, rot, B, J, H, W, out, ST(s)));
    return 0;
}
// joint-minor maps [B][H*W][J]: the strides Net::heat_argmax and pa_hg_pckh use on the engine's own heat maps
int pa_get_preds_nhwc(const float* maps, int B, int J, int H, int W, float* preds, float* maxval, void* s) {
    TRY(pa_launch_argmax(maps, (long)H * W * J, 1, J, B, J, H, W, preds, maxval, ST(s))); return 0;
}
int pa_final_preds_nhwc(const float* maps, const float* center, const float* scale, const float* rot, int B, int J, int H, int W,
                        float* out, float* scratch_preds, void* s) {
    TRY(pa_launch_argmax(maps, (long)H * W * J, 1, J, B, J, H, W, scratch_preds, nullptr, ST(s)));
    TRY(pa_launch_final_preds(maps, (long)H * W * J, 1, J, scratch_preds, center, scale, rot, B, J, H, W, out, ST(s)));
    return 0;
}
int pa_pck(const float* pred, const float* gt, const float* norm, float boundary, const int32_t* idxs, int nidx, float thr,
           const float* vis, int B, int J, float* acc, float* person, float* dists, void* s) {
    TRY(pa_launch_pck(pred, gt, norm, boundary, idxs, nidx, thr, vis, B, J, acc, person, dists, ST(s))); return 0;
}
int pa_affine_params(const double* params, int B, int res_in, int res_out, double* t_out, double* tinv_in, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_affine_params", params); NEED_PTR("pa_affine_params", t_out); NEED_PTR("pa_affine_params", tinv_in);
    NEED_POS("pa_affine_params", B); NEED_POS("pa_affine_params", res_in); NEED_POS("pa_affine_params", res_out);
    TRY(pa_launch_affine_params(params, B, res_in, res_out, t_out, tinv_in, ST(s))); return 0;
}
int pa_transform_pts(const float* pts, const double* params, const double* t, int B, int J, float width, double* out,
                     float* pts_img, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_transform_pts", pts); NEED_PTR("pa_transform_pts", params); NEED_PTR("pa_transform_pts", t); NEED_PTR("pa_transform_pts", out);
    NEED_POS("pa_transform_pts", B); NEED_POS("pa_transform_pts", J);
    TRY(pa_launch_transform_pts(pts, params, t, B, J, width, nullptr, out, pts_img, ST(s))); return 0;
}
int pa_transform_pts_sized(const float* pts, const double* params, const double* t, int B, int J, const int32_t* sizes, double* out,
                           float* pts_img, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_transform_pts_sized", pts); NEED_PTR("pa_transform_pts_sized", params); NEED_PTR("pa_transform_pts_sized", t);
    NEED_PTR("pa_transform_pts_sized", sizes); NEED_PTR("pa_transform_pts_sized", out);
    NEED_POS("pa_transform_pts_sized", B); NEED_POS("pa_transform_pts_sized", J);
    TRY(pa_launch_transform_pts(pts, params, t, B, J, 0.f, sizes, out, pts_img, ST(s))); return 0;
}
int pa_affine_warp_bilinear(const uint8_t* src, int Hs, int Ws, const double* tinv, const double* params, int B, int res,
                            void* out4, float* outf, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_affine_warp_bilinear", src); NEED_PTR("pa_affine_warp_bilinear", tinv); NEED_PTR("pa_affine_warp_bilinear", params);
    NEED_POS("pa_affine_warp_bilinear", Hs); NEED_POS("pa_affine_warp_bilinear", Ws); NEED_POS("pa_affine_warp_bilinear", B); NEED_POS("pa_affine_warp_bilinear", res);
    if (!out4 && !outf) { pa_set_error_msg("pa_affine_warp_bilinear: out4 and outf are both NULL"); return 1; }
    TRY(pa_launch_warp(src, Hs, Ws, nullptr, tinv, params, B, res, reinterpret_cast<bf16*>(out4), outf, ST(s))); return 0;
}
int pa_affine_warp_bilinear_sized(const uint8_t* src, int Hs, int Ws, const int32_t* sizes, const double* tinv, const double* params,
                                  int B, int res, void* out4, float* outf, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_affine_warp_bilinear_sized", src); NEED_PTR("pa_affine_warp_bilinear_sized", sizes); NEED_PTR("pa_affine_warp_bilinear_sized", tinv);
    NEED_PTR("pa_affine_warp_bilinear_sized", params);
    NEED_POS("pa_affine_warp_bilinear_sized", Hs); NEED_POS("pa_affine_warp_bilinear_sized", Ws); NEED_POS("pa_affine_warp_bilinear_sized", B);
    NEED_POS("pa_affine_warp_bilinear_sized", res);
    if (!out4 && !outf) { pa_set_error_msg("pa_affine_warp_bilinear_sized: out4 and outf are both NULL"); return 1; }
    TRY(pa_launch_warp(src, Hs, Ws, sizes, tinv, params, B, res, reinterpret_cast<bf16*>(out4), outf, ST(s))); return 0;
}
// backward of the bilinear sampler (warp_bwd.hip): d loss / d tinv, d gain and, through the chain rule of warp_bwd.h, d params
size_t pa_affine_warp_bwd_workspace_bytes(int B, int res) { return pa_warp_bwd_workspace_size(B, res); }
int pa_affine_warp_bilinear_bwd(const uint8_t* src, int Hs, int Ws, const int32_t* sizes, const double* tinv, const double* params, int B,
                                int res, const float* dimg, int layout, void* workspace, double* dtinv, double* dgain, double* dparams, void* s) {
    g_err[0] = 0;
    if (!src || !tinv || !params || !dimg || !workspace) { pa_set_error_msg("pa_affine_warp_bilinear_bwd: src, tinv, params, dimg and workspace must not be NULL"); return 1; }
    if (B < 1 || res < 1 || Hs < 1 || Ws < 1) { pa_set_error_msg("pa_affine_warp_bilinear_bwd: B >= 1, res >= 1 and a frame of at least one pixel"); return 1; }
    if (pa_warp_bwd_strips(B, res) == 0) { pa_set_error_msg("pa_affine_warp_bilinear_bwd: too many strips (B * ceil(res / 8) must stay below 2^31)"); return 1; }
    if (layout != 0 && layout != 1) { pa_set_error_msg("pa_affine_warp_bilinear_bwd: layout must be 0 ([B][3][res][res]) or 1 ([B][res][res][4])"); return 1; }
    if (reinterpret_cast<uintptr_t>(dimg) & 15) { pa_set_error_msg("pa_affine_warp_bilinear_bwd: dimg must be 16-byte aligned"); return 1; }
    if (reinterpret_cast<uintptr_t>(workspace) & 7) { pa_set_error_msg("pa_affine_warp_bilinear_bwd: workspace must be 8-byte aligned (double partial sums)"); return 1; }
    if (!dtinv && !dgain && !dparams) { pa_set_error_msg("pa_affine_warp_bilinear_bwd: dtinv, dgain and dparams are all NULL"); return 1; }
    TRY(pa_launch_warp_bwd(src, Hs, Ws, sizes, tinv, params, B, res, dimg, layout, workspace, dtinv, dgain, dparams, ST(s))); return 0;
}
int pa_affine_params_bwd_host(const double* params_host, const double* dtinv_host, const double* dgain_host, int B, int res_in, double* dparams_host) {
    g_err[0] = 0;
    if (!params_host || !dtinv_host || !dparams_host) { pa_set_error_msg("pa_affine_params_bwd_host: params, dtinv and dparams must not be NULL"); return 1; }
    if (B < 1 || res_in < 1) { pa_set_error_msg("pa_affine_params_bwd_host: B >= 1 and res_in >= 1"); return 1; }
    for (int b = 0; b < B; ++b)
        pa_affine_params_chain(params_host + (size_t)b * 8, dtinv_host + (size_t)b * 6, dgain_host ? dgain_host + (size_t)b * 3 : nullptr,
                               (double)res_in, dparams_host + (size_t)b * 8);
    return 0;
}
// soft-arg-max over heat maps and its backward pass (soft_argmax.hip); every refusal is decided here, before any device call
static int soft_argmax_args(const char* fn, int layout, int B, int J, int H, int W, float beta) {
    std::string f(fn);
    if (B < 1 || J < 1 || H < 1 || W < 1) { pa_set_error_msg((f + ": B, J, H and W must be >= 1").c_str()); return 1; }
    if ((long long)H * W >= (1LL << 27) || (long long)B * J > 0x7fffffffLL) { pa_set_error_msg((f + ": H * W must stay below 2^27 and B * J below 2^31").c_str()); return 1; }
    if (layout != 0 && layout != 1) { pa_set_error_msg((f + ": layout must be 0 ([B][J][H][W]) or 1 ([B][H*W][J])").c_str()); return 1; }
    if (!(beta > 0.f) || !(beta <= 3.402823466e38f)) { pa_set_error_msg((f + ": beta must be finite and > 0").c_str()); return 1; }
    return 0;
}
int pa_soft_argmax(const float* maps, int layout, int B, int J, int H, int W, float beta, float* coords, double* state, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_soft_argmax", maps); NEED_PTR("pa_soft_argmax", coords); NEED_PTR("pa_soft_argmax", state);
    if (soft_argmax_args("pa_soft_argmax", layout, B, J, H, W, beta)) return 1;
    TRY(pa_launch_soft_argmax(maps, layout, B, J, H, W, beta, coords, state, ST(s))); return 0;
}
int pa_soft_argmax_bwd(const float* maps, int layout, int B, int J, int H, int W, float beta, const double* state, const float* dcoords,
                       float* dmaps, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_soft_argmax_bwd", maps); NEED_PTR("pa_soft_argmax_bwd", state); NEED_PTR("pa_soft_argmax_bwd", dcoords); NEED_PTR("pa_soft_argmax_bwd", dmaps);
    if (soft_argmax_args("pa_soft_argmax_bwd", layout, B, J, H, W, beta)) return 1;
    if (dmaps == maps) { pa_set_error_msg("pa_soft_argmax_bwd: dmaps must not alias maps"); return 1; }
    TRY(pa_launch_soft_argmax_bwd(maps, layout, B, J, H, W, beta, state, dcoords, dmaps, ST(s))); return 0;
}
// calibration of the soft-arg-max bound: y[i] = the device's double exp(x[i]), the function those kernels call
int pa_exp_probe(const double* x, double* y, size_t n, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_exp_probe", x); NEED_PTR("pa_exp_probe", y);
    if (n == 0) { pa_set_error_msg("pa_exp_probe: n must be >= 1"); return 1; }
    TRY(pa_launch_exp_probe(x, y, n, ST(s))); return 0;
}
size_t pa_crop_workspace_bytes(int B, int Hs, int Ws, int res) { return pa_crop_workspace_size(B, Hs, Ws, res); }
int pa_crop_design_bytes(int B, int Hs, int Ws, int res, double* out) { if (!out) return 1; pa_crop_bytes_bound(B, Hs, Ws, res, out, out + 1); return 0; }
// calibration kernel of bench.py's floor (elementwise.hip): dst[i] = src[i], 16 bytes per lane, grid-stride over `bytes` (a multiple of 16)
int pa_copy_probe(void* dst, const void* src, size_t bytes, void* s) {
    g_err[0] = 0;
    if (!dst || !src || (bytes & 15)) { pa_set_error_msg("pa_copy_probe: NULL buffer or a size that is not a multiple of 16"); return 1; }
    TRY(pa_launch_copy16(dst, src, bytes, ST(s))); return 0;
}
// the same copy in another form (1: one 16-byte chunk per thread, no loop; 2: grid-stride with non-temporal accesses; 0 = pa_copy_probe):
// bench.py reports which form reaches what on the box, beside the guide's 6.29 TB/s "float4 copy"
int pa_copy_probe_form(void* dst, const void* src, size_t bytes, int form, void* s) {
    g_err[0] = 0;
    if (!dst || !src || (bytes & 15) || form < 0 || form > 2) { pa_set_error_msg("pa_copy_probe_form: NULL buffer, a size that is not a multiple of 16, or form not in 0..2"); return 1; }
    TRY(pa_launch_copy16(dst, src, bytes, ST(s), form)); return 0;
}
// fp32 copies of the augmentation parameters the metrics take (c [B][2], s [B], r [B]; data.py handed them over through three framework
// elementwise kernels per step): csr = [4 B] floats = c | s | r, from params [B][8] float64
int pa_params_csr(const double* params, int B, float* csr, void* s) {
    g_err[0] = 0;
    if (!params || !csr || B < 1) { pa_set_error_msg("pa_params_csr: bad arguments"); return 1; }
    TRY(pa_launch_params_csr(params, B, csr, ST(s))); return 0;
}
int pa_crop(const uint8_t* src, int Hs, int Ws, const int32_t* sizes, const double* params, int B, int res, void* workspace,
            void* out4, float* outf, uint8_t* out8, void* s) {
    if (!src || !params || !workspace || B <= 0 || res <= 0) { pa_set_error_msg("pa_crop: bad arguments"); return 1; }
    TRY(pa_launch_crop(src, Hs, Ws, sizes, params, B, res, workspace, reinterpret_cast<bf16*>(out4), outf, out8, ST(s))); return 0;
}
size_t pa_crop_stretch_workspace_bytes(int B, int Hs, int Ws, int res) { return pa_crop_stretch_workspace_size(B, Hs, Ws, res); }
int pa_crop_stretch(const uint8_t* src, int Hs, int Ws, const int32_t* sizes, const double* params, int B, int res, void* workspace,
                    void* out4, float* outf, uint8_t* out8, void* s) {
    if (!src || !params || !workspace || B <= 0 || res <= 0) { pa_set_error_msg("pa_crop_stretch: bad arguments"); return 1; }
    TRY(pa_launch_crop_stretch(src, Hs, Ws, sizes, params, B, res, workspace, reinterpret_cast<bf16*>(out4), outf, out8, ST(s))); return 0;
}
int pa_flip_lr_nhwc4(const void* src, void* dst, int B, int H, int W, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_flip_lr_nhwc4", src); NEED_PTR("pa_flip_lr_nhwc4", dst);
    NEED_POS("pa_flip_lr_nhwc4", B); NEED_POS("pa_flip_lr_nhwc4", H); NEED_POS("pa_flip_lr_nhwc4", W);
    TRY(pa_launch_flip_lr_nhwc4(reinterpret_cast<const bf16*>(src), reinterpret_cast<bf16*>(dst), B, H, W, ST(s))); return 0;
}
int pa_flip_tta_merge(const float* out, const float* out_flipped, float* merged, int B, int J, int H, int W, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_flip_tta_merge", out); NEED_PTR("pa_flip_tta_merge", out_flipped); NEED_PTR("pa_flip_tta_merge", merged);
    NEED_POS("pa_flip_tta_merge", B); NEED_POS("pa_flip_tta_merge", H); NEED_POS("pa_flip_tta_merge", W);
    if (J != 16) { pa_set_error_msg("pa_flip_tta_merge: J must be 16, the left/right joint table is MPII's (16 joints)"); return 1; }
    TRY(pa_launch_flip_tta_merge(out, out_flipped, merged, B, H, W, ST(s))); return 0;
}
int pa_sample_aug(const float* meta, const int32_t* scale_idx, const int32_t* rot_idx, int mode, uint64_t seed, uint64_t step,
                  int B, double* params, void* s) {
    if (B < 1) { pa_set_error_msg("pa_sample_aug: B >= 1"); return 1; }
    if (mode != 0 && ((mode != 3 && !scale_idx) || (mode != 2 && !rot_idx))) { pa_set_error_msg("pa_sample_aug: the agent laws need bin indices"); return 1; }
    TRY(pa_launch_sample_aug(meta, scale_idx, rot_idx, mode, seed, step, nullptr, B, params, ST(s))); return 0;
}
int pa_sample_aug_given(const float* meta, const int32_t* scale_idx, const int32_t* rot_idx, int mode, const double* draws,
                        int B, double* params, void* s) {
    if (!draws) { pa_set_error_msg("pa_sample_aug_given: draws is NULL"); return 1; }
    if (B < 1) { pa_set_error_msg("pa_sample_aug_given: B >= 1"); return 1; }
    if (mode != 0 && ((mode != 3 && !scale_idx) || (mode != 2 && !rot_idx))) { pa_set_error_msg("pa_sample_aug_given: the agent laws need bin indices"); return 1; }
    TRY(pa_launch_sample_aug(meta, scale_idx, rot_idx, mode, 0, 0, draws, B, params, ST(s))); return 0;
}
int pa_sample_categorical(const float* logits, int B, int K, uint64_t seed, uint64_t step, unsigned slot, float* probs,
                          int32_t* idx, void* s) {
    if (K < 1 || K > 64) { pa_set_error_msg("pa_sample_categorical: 1 <= K <= 64"); return 1; }
    if (B < 1) { pa_set_error_msg("pa_sample_categorical: B >= 1"); return 1; }
    // the stream key holds the slot in 8 bits: slot 256 + s of sample b would be slot s of sample b + 1
    if (slot > 255) { pa_set_error_msg("pa_sample_categorical: slot <= 255"); return 1; }
    TRY(pa_launch_sample_categorical(logits, B, K, seed, step, slot, probs, idx, ST(s))); return 0;
}
int pa_sample_dropout_masks(const float* logits, int B, int cells, int dropout_num, uint64_t seed, uint64_t step, const double* uniforms,
                            float* probs, float* masks, int32_t* indexes, void* s) {
    if (cells < 1 || cells > 64 || dropout_num < 0 || dropout_num >= cells || !masks) {
        pa_set_error_msg("pa_sample_dropout_masks: need 1 <= cells <= 64, 0 <= dropout_num < cells, masks != NULL"); return 1;
    }
    if (B < 1) { pa_set_error_msg("pa_sample_dropout_masks: B >= 1"); return 1; }
    TRY(pa_launch_sample_dropout_masks(logits, B, cells, dropout_num, seed, step, uniforms, probs, masks, indexes, ST(s))); return 0;
}
int pa_cell_mask(const void* x, const float* masks, void* out, int B, int H, int W, int C, void* s) {
    PaEpilogue e; memset(&e, 0, sizeof e); e.mode = PA_OUT_PLAIN;
    TRY(pa_launch_cell_mask(pa_plain(reinterpret_cast<const bf16*>(x)), masks, e, reinterpret_cast<bf16*>(out), B, H, W, C, ST(s))); return 0;
}
int pa_rmsprop_step(float* p, const float* g, float* v, size_t n, float lr, float alpha, float eps, float gscale, void* s) {
    TRY(pa_launch_rmsprop(p, g, v, n, lr, alpha, eps, gscale, nullptr, ST(s))); return 0;
}
int pa_rmsprop_skipped_steps(long long* count, void* s) { if (!count) return 1; TRY(pa_rmsprop_skipped(nullptr, count, ST(s))); return 0; }
// the same step with the optimizer's OWN skip state (two int32 on the device, zeroed by the caller once): optimizers on different
// streams do not share the "this gradient is non-finite" flag
int pa_rmsprop_step_state(float* p, const float* g, float* v, size_t n, float lr, float alpha, float eps, float gscale, int32_t* state, void* s) {
    if (!state) { pa_set_error_msg("pa_rmsprop_step_state: state is NULL (two int32 on the device)"); return 1; }
    TRY(pa_launch_rmsprop(p, g, v, n, lr, alpha, eps, gscale, state, ST(s))); return 0;
}
int pa_rmsprop_skipped_steps_state(const int32_t* state, long long* count, void* s) {
    if (!count || !state) return 1;
    TRY(pa_rmsprop_skipped(state, count, ST(s))); return 0;
}
// torch.optim.RMSprop's other options and clip_grad_norm_'s coefficient (the reference trains with all of them off, stack-hg.py:51-52:
// no reference counterpart beyond torch's option set).  An argument error launches nothing.
int pa_rmsprop_step_opts(const pa_rmsprop_opts* o, float* p, const float* g, float* v, float* buf, float* ga, size_t n, float gscale,
                         const float* clip_coef, int32_t* state, void* s) {
    g_err[0] = 0;
    if (!o || !p || !g || !v || !state) { pa_set_error_msg("pa_rmsprop_step_opts: opts, param, grad, square_avg or state is NULL"); return 1; }
    if (!(o->momentum >= 0.f) || !(o->weight_decay >= 0.f)) { pa_set_error_msg("pa_rmsprop_step_opts: momentum and weight_decay must be >= 0"); return 1; }
    if ((o->momentum > 0.f) != (buf != nullptr)) { pa_set_error_msg("pa_rmsprop_step_opts: momentum_buf is required when momentum > 0 and must be NULL otherwise"); return 1; }
    if ((o->centered != 0) != (ga != nullptr)) { pa_set_error_msg("pa_rmsprop_step_opts: grad_avg is required when centered and must be NULL otherwise"); return 1; }
    const PaRmspropOpts k = {o->lr, o->alpha, o->eps, o->momentum, o->weight_decay};
    TRY(pa_launch_rmsprop_opts(k, o->centered != 0, p, g, v, buf, ga, n, gscale, clip_coef, state, ST(s))); return 0;
}
size_t pa_grad_norm_workspace_bytes(size_t n) { return pa_grad_norm_workspace_size(n); }
int pa_grad_norm(const float* g, size_t n, float gscale, float max_norm, void* workspace, float* out2, void* s) {
    g_err[0] = 0;
    if (!g || !workspace || !out2) { pa_set_error_msg("pa_grad_norm: grad, workspace or out2 is NULL"); return 1; }
    if (!(max_norm > 0.f)) { pa_set_error_msg("pa_grad_norm: max_norm must be > 0"); return 1; }
    if (reinterpret_cast<uintptr_t>(workspace) & 7) { pa_set_error_msg("pa_grad_norm: workspace must be 8-byte aligned (double partial sums)"); return 1; }
    TRY(pa_launch_grad_norm(g, n, gscale, max_norm, workspace, out2, ST(s))); return 0;
}
// torch.optim.Adam / AdamW (no reference counterpart beyond torch's option set); the step count and the bias-correction constants live in
// the optimizer's device state.  An argument error launches nothing.
static_assert(sizeof(pa_adam_state) == 32 && sizeof(PaAdamState) == 32, "pa_adam_state is 32 bytes");
static bool adam_state_ok(const char* who, const void* state) {
    if (state && !(reinterpret_cast<uintptr_t>(state) & 15)) return true;
    pa_set_error_msg((std::string(who) + (state ? ": state must be 16-byte aligned" : ": state is NULL (a pa_adam_state on the device)")).c_str());
    return false;
}
int pa_adam_step(const pa_adam_opts* o, float* p, const float* g, float* m, float* v, float* vmax, size_t n, float gscale,
                 const float* clip_coef, pa_adam_state* state, void* s) {
    g_err[0] = 0;
    if (!o || !p || !g || !m || !v) { pa_set_error_msg("pa_adam_step: opts, param, grad, exp_avg or exp_avg_sq is NULL"); return 1; }
    if (!adam_state_ok("pa_adam_step", state)) return 1;
    if ((o->amsgrad != 0) != (vmax != nullptr)) { pa_set_error_msg("pa_adam_step: max_exp_avg_sq is required when amsgrad and must be NULL otherwise"); return 1; }
    if (!(o->beta1 >= 0.f && o->beta1 < 1.f) || !(o->beta2 >= 0.f && o->beta2 < 1.f)) { pa_set_error_msg("pa_adam_step: beta1 and beta2 must be in [0, 1)"); return 1; }
    if (!(o->eps > 0.f)) { pa_set_error_msg("pa_adam_step: eps must be > 0"); return 1; }
    if (!(o->weight_decay >= 0.f)) { pa_set_error_msg("pa_adam_step: weight_decay must be >= 0"); return 1; }
    const PaAdamOpts k = {o->lr, o->beta1, o->beta2, o->eps, o->weight_decay, (float)(1.0 - (double)o->lr * (double)o->weight_decay),
                          1.f - o->beta1, 1.f - o->beta2};
    const int decay = o->weight_decay != 0.f ? (o->decoupled ? 2 : 1) : 0;
    TRY(pa_launch_adam(k, o->amsgrad != 0, decay, p, g, m, v, vmax, n, gscale, clip_coef, reinterpret_cast<PaAdamState*>(state), ST(s))); return 0;
}
int pa_adam_steps(const pa_adam_state* state, long long* steps, long long* skipped, void* s) {
    g_err[0] = 0;
    if (!adam_state_ok("pa_adam_steps", state)) return 1;
    TRY(pa_adam_read_steps(reinterpret_cast<const PaAdamState*>(state), steps, skipped, ST(s))); return 0;
}
int pa_adam_set_steps(pa_adam_state* state, long long steps, void* s) {
    g_err[0] = 0;
    if (!adam_state_ok("pa_adam_set_steps", state)) return 1;
    if (steps < 0 || steps > 2147483647LL) { pa_set_error_msg("pa_adam_set_steps: steps must be in 0 .. 2^31 - 1"); return 1; }
    TRY(pa_launch_adam_set_steps(reinterpret_cast<PaAdamState*>(state), (int)steps, ST(s))); return 0;
}
// Parameter groups: per-group lr / weight_decay / frozen through a chunk map (elementwise.hip).  The map builder is host only; the three
// device entry points check every argument before the first device call, so an argument error launches nothing.
static_assert(sizeof(pa_opt_group) == 16 && PA_OPT_GROUPS_MAX == PA_OPT_GROUPS, "pa_opt_group is 16 bytes, 16 groups");
size_t pa_opt_chunk_map_bytes(size_t n) { return n / 4 + (n % 4 != 0); }
int pa_opt_chunk_map_host(const size_t* offsets, const size_t* numels, const int32_t* group, int ntensors, size_t n, int ngroups,
                          uint8_t* map) {
    g_err[0] = 0;
    const char* who = "pa_opt_chunk_map_host";
    if (!offsets || !numels || !group || !map) { pa_set_error_msg((std::string(who) + ": offsets, numels, group or map is NULL").c_str()); return 1; }
    if (ntensors < 1) { pa_set_error_msg((std::string(who) + ": ntensors must be >= 1").c_str()); return 1; }
    if (ngroups < 1 || ngroups > PA_OPT_GROUPS_MAX) { pa_set_error_msg((std::string(who) + ": ngroups must be in 1 .. 16").c_str()); return 1; }
    size_t end = 0;
    for (int t = 0; t < ntensors; ++t) {
        const std::string at = std::string(who) + ": tensor " + std::to_string(t);
        if (offsets[t] & 3) { pa_set_error_msg((at + ": offset is not a multiple of 4").c_str()); return 1; }
        if (offsets[t] < end) { pa_set_error_msg((at + ": out of order or overlapping the tensor in front of it").c_str()); return 1; }
        if (numels[t] > n || offsets[t] > n - numels[t]) { pa_set_error_msg((at + ": ends past n").c_str()); return 1; }
        if (group[t] < 0 || group[t] >= ngroups) { pa_set_error_msg((at + ": group id outside 0 .. ngroups - 1").c_str()); return 1; }
        end = offsets[t] + numels[t];
    }
    const size_t chunks = pa_opt_chunk_map_bytes(n);
    size_t c = 0;
    uint8_t cur = 0;                        // a chunk no tensor touches: the group of the tensor in front of it (0 in front of the first)
    for (int t = 0; t < ntensors; ++t) {
        if (numels[t] == 0) continue;
        const size_t first = offsets[t] / 4, last = (offsets[t] + numels[t] - 1) / 4;
        for (; c < first; ++c) map[c] = cur;
        cur = (uint8_t)group[t];
        for (; c <= last; ++c) map[c] = cur;
    }
    for (; c < chunks; ++c) map[c] = cur;
    return 0;
}
// groups_host -> the kernels' table; false with the error set
static bool opt_groups_table(const char* who, const pa_opt_group* groups, int ngroups, const uint8_t* chunk_map, PaOptGroupTable* tab) {
    const std::string w(who);
    if (!groups) { pa_set_error_msg((w + ": groups_host is NULL").c_str()); return false; }
    if (ngroups < 1 || ngroups > PA_OPT_GROUPS_MAX) { pa_set_error_msg((w + ": ngroups must be in 1 .. 16").c_str()); return false; }
    bool frozen = false;
    for (int k = 0; k < PA_OPT_GROUPS; ++k) {
        PaOptGroupK& e = tab->g[k];
        if (k >= ngroups) { e.lr = e.wd = 0.f; e.c_dec = 1.f; e.frozen = 1; continue; }
        if (!(groups[k].lr >= 0.f) || !std::isfinite(groups[k].lr)) { pa_set_error_msg((w + ": lr of group " + std::to_string(k) + " must be finite and >= 0").c_str()); return false; }
        if (!(groups[k].weight_decay >= 0.f) || !std::isfinite(groups[k].weight_decay)) {
            pa_set_error_msg((w + ": weight_decay of group " + std::to_string(k) + " must be finite and >= 0").c_str()); return false;
        }
        e.lr = groups[k].lr; e.wd = groups[k].weight_decay;
        e.c_dec = (float)(1.0 - (double)e.lr * (double)e.wd);
        e.frozen = groups[k].frozen != 0;
        frozen |= e.frozen != 0;
    }
    if (!chunk_map && (ngroups > 1 || frozen)) { pa_set_error_msg((w + ": chunk_map is NULL with more than one group or a frozen group").c_str()); return false; }
    return true;
}
int pa_rmsprop_step_groups(const pa_rmsprop_opts* o, const pa_opt_group* groups, int ngroups, const uint8_t* chunk_map, float* p,
                           const float* g, float* v, float* buf, float* ga, size_t n, float gscale, const float* clip_coef, int32_t* state,
                           void* s) {
    g_err[0] = 0;
    if (!o || !p || !g || !v || !state) { pa_set_error_msg("pa_rmsprop_step_groups: opts, param, grad, square_avg or state is NULL"); return 1; }
    if (!(o->momentum >= 0.f)) { pa_set_error_msg("pa_rmsprop_step_groups: momentum must be >= 0"); return 1; }
    if ((o->momentum > 0.f) != (buf != nullptr)) { pa_set_error_msg("pa_rmsprop_step_groups: momentum_buf is required when momentum > 0 and must be NULL otherwise"); return 1; }
    if ((o->centered != 0) != (ga != nullptr)) { pa_set_error_msg("pa_rmsprop_step_groups: grad_avg is required when centered and must be NULL otherwise"); return 1; }
    PaOptGroupTable tab;
    if (!opt_groups_table("pa_rmsprop_step_groups", groups, ngroups, chunk_map, &tab)) return 1;
    const PaRmspropOpts k = {0.f, o->alpha, o->eps, o->momentum, 0.f};
    TRY(pa_launch_rmsprop_groups(k, o->centered != 0, tab, ngroups, chunk_map, p, g, v, buf, ga, n, gscale, clip_coef, state, ST(s))); return 0;
}
int pa_adam_step_groups(const pa_adam_opts* o, const pa_opt_group* groups, int ngroups, const uint8_t* chunk_map, float* group_consts,
                        float* p, const float* g, float* m, float* v, float* vmax, size_t n, float gscale, const float* clip_coef,
                        pa_adam_state* state, void* s) {
    g_err[0] = 0;
    if (!o || !p || !g || !m || !v) { pa_set_error_msg("pa_adam_step_groups: opts, param, grad, exp_avg or exp_avg_sq is NULL"); return 1; }
    if (!adam_state_ok("pa_adam_step_groups", state)) return 1;
    if ((o->amsgrad != 0) != (vmax != nullptr)) { pa_set_error_msg("pa_adam_step_groups: max_exp_avg_sq is required when amsgrad and must be NULL otherwise"); return 1; }
    if (!(o->beta1 >= 0.f && o->beta1 < 1.f) || !(o->beta2 >= 0.f && o->beta2 < 1.f)) { pa_set_error_msg("pa_adam_step_groups: beta1 and beta2 must be in [0, 1)"); return 1; }
    if (!(o->eps > 0.f)) { pa_set_error_msg("pa_adam_step_groups: eps must be > 0"); return 1; }
    PaOptGroupTable tab;
    if (!opt_groups_table("pa_adam_step_groups", groups, ngroups, chunk_map, &tab)) return 1;
    if (!group_consts && (ngroups > 1 || tab.g[0].frozen)) { pa_set_error_msg("pa_adam_step_groups: group_consts is NULL with more than one group or a frozen group"); return 1; }
    const PaAdamOpts k = {0.f, o->beta1, o->beta2, o->eps, 0.f, 1.f, 1.f - o->beta1, 1.f - o->beta2};
    TRY(pa_launch_adam_groups(k, o->amsgrad != 0, o->decoupled != 0, tab, ngroups, chunk_map, group_consts, p, g, m, v, vmax, n, gscale,
                              clip_coef, reinterpret_cast<PaAdamState*>(state), ST(s)));
    return 0;
}
int pa_grad_norm_groups(const float* g, size_t n, const uint8_t* chunk_map, uint32_t excluded, float gscale, float max_norm,
                        void* workspace, float* out2, void* s) {
    g_err[0] = 0;
    if (!g || !workspace || !out2) { pa_set_error_msg("pa_grad_norm_groups: grad, workspace or out2 is NULL"); return 1; }
    if (!(max_norm > 0.f)) { pa_set_error_msg("pa_grad_norm_groups: max_norm must be > 0"); return 1; }
    if (reinterpret_cast<uintptr_t>(workspace) & 7) { pa_set_error_msg("pa_grad_norm_groups: workspace must be 8-byte aligned (double partial sums)"); return 1; }
    if (excluded >> PA_OPT_GROUPS_MAX) { pa_set_error_msg("pa_grad_norm_groups: excluded_groups has bits at or above 16"); return 1; }
    if (excluded && !chunk_map) { pa_set_error_msg("pa_grad_norm_groups: chunk_map is NULL with excluded groups"); return 1; }
    TRY(pa_launch_grad_norm_groups(g, n, chunk_map, excluded, gscale, max_norm, workspace, out2, ST(s))); return 0;
}
// Layer-wise trust ratios (opt_layerwise.hip; utils.optim.SGD / LARS / LAMB): the segment plan is host only; the device entry points check
// every argument before the first device call, so an argument error launches nothing.
static_assert(sizeof(pa_opt_segment) == 16 && sizeof(PaOptSegment) == 16 && PA_OPT_SEGMENT_FLOATS % 4 == 0, "pa_opt_segment is 16 bytes");
size_t pa_opt_segments_host(const size_t* offsets, const size_t* numels, const int32_t* group, int ntensors, size_t n, pa_opt_segment* segs,
                            size_t cap) {
    g_err[0] = 0;
    const std::string who = "pa_opt_segments_host";
    if (!offsets || !numels || !group) { pa_set_error_msg((who + ": offsets, numels or group is NULL").c_str()); return 0; }
    if (ntensors < 1) { pa_set_error_msg((who + ": ntensors must be >= 1").c_str()); return 0; }
    size_t end = 0, count = 0;
    for (int t = 0; t < ntensors; ++t) {                // every input error first: nothing is written on an error
        const std::string at = who + ": tensor " + std::to_string(t);
        if (offsets[t] & 3) { pa_set_error_msg((at + ": offset is not a multiple of 4").c_str()); return 0; }
        if (offsets[t] < end) { pa_set_error_msg((at + ": out of order or overlapping the tensor in front of it").c_str()); return 0; }
        if (numels[t] > n || offsets[t] > n - numels[t]) { pa_set_error_msg((at + ": ends past n").c_str()); return 0; }
        if (group[t] < 0 || group[t] >= PA_OPT_GROUPS_MAX) { pa_set_error_msg((at + ": group id outside 0 .. 15").c_str()); return 0; }
        if (offsets[t] / 4 + numels[t] / 4 > 0xffffffffull) { pa_set_error_msg((at + ": lies past 2^34 floats (chunk0 is 32 bits)").c_str()); return 0; }
        end = offsets[t] + numels[t];
        count += (numels[t] + PA_OPT_SEGMENT_FLOATS - 1) / PA_OPT_SEGMENT_FLOATS;
    }
    if (count == 0) { pa_set_error_msg((who + ": every tensor is empty").c_str()); return 0; }
    if (count > 0xffffffffull) { pa_set_error_msg((who + ": more than 2^32 - 1 segments").c_str()); return 0; }
    if (!segs) return count;
    if (cap < count) { pa_set_error_msg((who + ": cap " + std::to_string(cap) + " is smaller than the " + std::to_string(count) + " segments").c_str()); return 0; }
    size_t k = 0;
    for (int t = 0; t < ntensors; ++t)
        for (size_t done = 0; done < numels[t]; done += PA_OPT_SEGMENT_FLOATS, ++k) {
            const size_t left = numels[t] - done;
            segs[k].chunk0 = (uint32_t)((offsets[t] + done) / 4);
            segs[k].nfloats = (uint32_t)(left < PA_OPT_SEGMENT_FLOATS ? left : PA_OPT_SEGMENT_FLOATS);
            segs[k].tensor = t;
            segs[k].group = group[t];
        }
    return count;
}
size_t pa_opt_layer_workspace_bytes(size_t nsegs, int ntensors) { return pa_opt_layer_workspace_size(nsegs, ntensors); }
// what pa_tensor_norms, pa_lamb_step and pa_lars_step share: the segment list against n and the arrays of the two norm launches
static bool layer_args_ok(const std::string& w, const void* segs, size_t nsegs, int ntensors, size_t n, bool need_ws, const void* workspace,
                          const void* norms, const void* trust) {
    if (!segs && nsegs) { pa_set_error_msg((w + ": segs is NULL").c_str()); return false; }
    if (nsegs == 0 && n > 0) { pa_set_error_msg((w + ": nsegs is 0 with n > 0").c_str()); return false; }
    if (nsegs > 0xffffffffull) { pa_set_error_msg((w + ": nsegs must stay below 2^32").c_str()); return false; }
    if (ntensors < 1) { pa_set_error_msg((w + ": ntensors must be >= 1").c_str()); return false; }
    if (reinterpret_cast<uintptr_t>(segs) & 15) { pa_set_error_msg((w + ": segs must be 16-byte aligned").c_str()); return false; }
    if (need_ws && (!workspace || !norms || !trust)) { pa_set_error_msg((w + ": workspace, norms or trust is NULL").c_str()); return false; }
    if (reinterpret_cast<uintptr_t>(workspace) & 7) { pa_set_error_msg((w + ": workspace must be 8-byte aligned (double partial sums)").c_str()); return false; }
    return true;
}
static bool finite_nonneg(float v) { return v >= 0.f && std::isfinite(v); }
int pa_tensor_norms(const float* x, const pa_opt_segment* segs, size_t nsegs, int ntensors, float scale, void* workspace, float* norms, void* s) {
    g_err[0] = 0;
    if (!x || !segs || !workspace || !norms) { pa_set_error_msg("pa_tensor_norms: x, segs, workspace or norms is NULL"); return 1; }
    if (nsegs == 0) { pa_set_error_msg("pa_tensor_norms: nsegs must be >= 1"); return 1; }
    if (!layer_args_ok("pa_tensor_norms", segs, nsegs, ntensors, 1, false, workspace, norms, nullptr)) return 1;
    if (reinterpret_cast<uintptr_t>(x) & 15) { pa_set_error_msg("pa_tensor_norms: x must be 16-byte aligned"); return 1; }
    if (!std::isfinite(scale)) { pa_set_error_msg("pa_tensor_norms: scale must be finite"); return 1; }
    TRY(pa_launch_tensor_norms(x, reinterpret_cast<const PaOptSegment*>(segs), nsegs, ntensors, scale, workspace, norms, ST(s))); return 0;
}
int pa_lamb_step(const pa_lamb_opts* o, const pa_opt_group* groups, int ngroups, const pa_opt_segment* segs, size_t nsegs, int ntensors,
                 float* p, const float* g, float* m, float* v, size_t n, float gscale, const float* clip_coef, void* workspace, float* norms,
                 float* trust, pa_adam_state* state, void* s) {
    g_err[0] = 0;
    if (!o || !p || !g || !m || !v) { pa_set_error_msg("pa_lamb_step: opts, param, grad, exp_avg or exp_avg_sq is NULL"); return 1; }
    if (!adam_state_ok("pa_lamb_step", state)) return 1;
    if (o->amsgrad) { pa_set_error_msg("pa_lamb_step: amsgrad is not supported with LAMB"); return 1; }
    if (!(o->beta1 >= 0.f && o->beta1 < 1.f) || !(o->beta2 >= 0.f && o->beta2 < 1.f)) { pa_set_error_msg("pa_lamb_step: beta1 and beta2 must be in [0, 1)"); return 1; }
    if (!(o->eps > 0.f) || !std::isfinite(o->eps)) { pa_set_error_msg("pa_lamb_step: eps must be finite and > 0"); return 1; }
    if (!finite_nonneg(o->max_trust)) { pa_set_error_msg("pa_lamb_step: max_trust must be finite and >= 0 (0: no cap)"); return 1; }
    if (!layer_args_ok("pa_lamb_step", segs, nsegs, ntensors, n, true, workspace, norms, trust)) return 1;
    if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) {
        pa_set_error_msg("pa_lamb_step: param, grad, exp_avg and exp_avg_sq must be 16-byte aligned"); return 1;
    }
    PaOptGroupTable tab;          // (the segment list stands where the grouped steps take their chunk map: it carries the group ids)
    if (!opt_groups_table("pa_lamb_step", groups, ngroups, reinterpret_cast<const uint8_t*>(segs ? (const void*)segs : (const void*)o), &tab)) return 1;
    const PaLambOpts k = {o->beta1, o->beta2, o->eps, 1.f - o->beta1, 1.f - o->beta2, o->max_trust, o->always_adapt != 0};
    TRY(pa_launch_lamb(k, tab, reinterpret_cast<const PaOptSegment*>(segs), nsegs, ntensors, p, g, m, v, n, gscale, clip_coef, workspace, norms,
                       trust, reinterpret_cast<PaAdamState*>(state), ST(s)));
    return 0;
}
int pa_lars_step(const pa_lars_opts* o, const pa_opt_group* groups, int ngroups, const pa_opt_segment* segs, size_t nsegs, int ntensors,
                 float* p, const float* g, float* buf, size_t n, float gscale, const float* clip_coef, void* workspace, float* norms,
                 float* trust, int32_t* state, void* s) {
    g_err[0] = 0;
    if (!o || !p || !g || !state) { pa_set_error_msg("pa_lars_step: opts, param, grad or state is NULL"); return 1; }
    if (!finite_nonneg(o->momentum) || !finite_nonneg(o->trust_coef) || !finite_nonneg(o->lars_eps)) {
        pa_set_error_msg("pa_lars_step: momentum, trust_coef and lars_eps must be finite and >= 0"); return 1;
    }
    if ((o->momentum != 0.f) != (buf != nullptr)) { pa_set_error_msg("pa_lars_step: momentum_buf is required when momentum != 0 and must be NULL otherwise"); return 1; }
    if (o->nesterov && o->momentum == 0.f) { pa_set_error_msg("pa_lars_step: nesterov needs momentum != 0"); return 1; }
    if (!layer_args_ok("pa_lars_step", segs, nsegs, ntensors, n, o->trust_coef > 0.f, workspace, norms, trust)) return 1;
    if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(buf)) & 15) {
        pa_set_error_msg("pa_lars_step: param, grad and momentum_buf must be 16-byte aligned"); return 1;
    }
    PaOptGroupTable tab;
    if (!opt_groups_table("pa_lars_step", groups, ngroups, reinterpret_cast<const uint8_t*>(segs ? (const void*)segs : (const void*)o), &tab)) return 1;
    const PaLarsOpts k = {o->momentum, o->trust_coef, o->lars_eps, o->nesterov != 0, o->always_adapt != 0};
    TRY(pa_launch_lars(k, tab, reinterpret_cast<const PaOptSegment*>(segs), nsegs, ntensors, p, g, buf, n, gscale, clip_coef, workspace, norms,
                       trust, state, ST(s)));
    return 0;
}
// Weight EMA (ema.hip; utils.optim.ModelEma): the update count, the hold decision and the weight w live in the caller's device state.  An
// argument error launches nothing.
static_assert(sizeof(pa_ema_state) == 32 && sizeof(PaEmaState) == 32, "pa_ema_state is 32 bytes");
int pa_ema_advance(pa_ema_state* state, float decay, int warmup, const int32_t* skip_flag, void* s) {
    g_err[0] = 0;
    if (!state || (reinterpret_cast<uintptr_t>(state) & 3)) { pa_set_error_msg("pa_ema_advance: state is NULL or misaligned (a pa_ema_state on the device)"); return 1; }
    if (!(decay >= 0.f && decay < 1.f)) { pa_set_error_msg("pa_ema_advance: decay must be finite and in [0, 1)"); return 1; }
    TRY(pa_launch_ema_advance(reinterpret_cast<PaEmaState*>(state), decay, warmup != 0, skip_flag, ST(s))); return 0;
}
int pa_ema_lerp(float* ema, const float* src, size_t n, const pa_ema_state* state, int copy, void* s) {
    g_err[0] = 0;
    if (!state || !ema || !src) { pa_set_error_msg("pa_ema_lerp: state, ema or src is NULL"); return 1; }
    if (ema == src) { pa_set_error_msg("pa_ema_lerp: ema and src are the same array"); return 1; }
    if ((reinterpret_cast<uintptr_t>(ema) | reinterpret_cast<uintptr_t>(src)) & 15) { pa_set_error_msg("pa_ema_lerp: ema and src must be 16-byte aligned"); return 1; }
    if (n == 0) return 0;
    TRY(pa_launch_ema_lerp(ema, src, n, reinterpret_cast<const PaEmaState*>(state), copy != 0, ST(s))); return 0;
}
int pa_ema_counts(const pa_ema_state* state, long long* updates, long long* held, void* s) {
    g_err[0] = 0;
    if (!state) { pa_set_error_msg("pa_ema_counts: state is NULL"); return 1; }
    TRY(pa_ema_read_counts(reinterpret_cast<const PaEmaState*>(state), updates, held, ST(s))); return 0;
}
int pa_ema_set_updates(pa_ema_state* state, long long updates, void* s) {
    g_err[0] = 0;
    if (!state) { pa_set_error_msg("pa_ema_set_updates: state is NULL"); return 1; }
    if (updates < 0 || updates > 2147483647LL) { pa_set_error_msg("pa_ema_set_updates: updates must be in 0 .. 2^31 - 1"); return 1; }
    TRY(pa_launch_ema_set_updates(reinterpret_cast<PaEmaState*>(state), (int)updates, ST(s))); return 0;
}
// Gradient accumulation (grad_accum.hip; utils.optim accumulate() / step()): dst = a + b, or dst = a with b == NULL.  Every pair of the
// three ranges is either the same range or disjoint; an argument error launches nothing.
int pa_grad_accumulate(float* dst, const float* a, const float* b, size_t n, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_grad_accumulate", dst); NEED_PTR("pa_grad_accumulate", a);
    if (n < 1 || n > ((size_t)-1) / sizeof(float)) { pa_set_error_msg("pa_grad_accumulate: n must be >= 1 (and n floats addressable)"); return 1; }
    const uintptr_t bytes = (uintptr_t)n * sizeof(float);
    const uintptr_t r[3] = { reinterpret_cast<uintptr_t>(dst), reinterpret_cast<uintptr_t>(a), reinterpret_cast<uintptr_t>(b) };
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j) {
            if (!r[j] || r[i] == r[j]) continue;          // (b == NULL: the copy form; the same range: in place, or a read twice)
            const uintptr_t lo = r[i] < r[j] ? r[i] : r[j], hi = r[i] < r[j] ? r[j] : r[i];
            if (hi - lo < bytes) { pa_set_error_msg("pa_grad_accumulate: dst, a and b overlap in part (each pair must be the same range or disjoint)"); return 1; }
        }
    if (!b && dst == a) return 0;
    TRY(pa_launch_grad_accumulate(dst, a, b, n, ST(s))); return 0;
}
int pa_nchw_to_nhwc(const float* src, void* dst, int B, int C, int H, int W, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_nchw_to_nhwc", src); NEED_PTR("pa_nchw_to_nhwc", dst);
    NEED_POS("pa_nchw_to_nhwc", B); NEED_POS("pa_nchw_to_nhwc", C); NEED_POS("pa_nchw_to_nhwc", H); NEED_POS("pa_nchw_to_nhwc", W);
    TRY(pa_launch_nchw_f32_to_nhwc_bf16(src, reinterpret_cast<bf16*>(dst), B, C, H, W, ST(s))); return 0;
}
int pa_nhwc_to_nchw(const void* src, float* dst, int B, int C, int H, int W, void* s) {
    g_err[0] = 0;
    NEED_PTR("pa_nhwc_to_nchw", src); NEED_PTR("pa_nhwc_to_nchw", dst);
    NEED_POS("pa_nhwc_to_nchw", B); NEED_POS("pa_nhwc_to_nchw", C); NEED_POS("pa_nhwc_to_nchw", H); NEED_POS("pa_nhwc_to_nchw", W);
    TRY(pa_launch_nhwc_bf16_to_nchw_f32(pa_plain(reinterpret_cast<const bf16*>(src)), dst, B, C, H, W, ST(s))); return 0;
}

// ---------------------------------------------------------------------------- residual block op
struct ResidualOp {
    Net n; Residual r; Act in;
    size_t build(int B, int H, int W, int C, char* base) {
        Arena a; a.base = base;
        n.loss_dev = a.get<float>(64);
        a.take(0);
        n.stats_arena = reinterpret_cast<float*>(base); n.stats_arena_floats = a.off / sizeof(float);
        n.prep_jobs = a.get<PaPrepJob>(n.convs.size());
        n.red_jobs = a.get<PaWgradReduceJob>(n.convs.size());
        n.bneval_jobs = a.get<PaBnEvalJob>(n.bns.size());
        in = n.new_act(a, B, H, W, C, nullptr, true);
        r.layout(n, a, B, H, W, true);
        a.take(0);
        return a.off;
    }
};

size_t pa_residual_workspace_bytes(int B, int H, int W, int C) {
    ResidualOp op; op.n.is_agent = true; op.n.B = B; op.r.declare(op.n, "", C, C, false);      // (same state as pa_residual_fwd_bwd: the layout depends on it)
    return op.build(B, H, W, C, nullptr);
}

int pa_residual_fwd_bwd(const float* x, const float* dy, const float* params, float* y, float* dx, float* grads, float* buffers,
                        int B, int C, int H, int W, void* ws, void* s) {
    g_err[0] = 0;
    // (before any launch: the block's gradient enters through pa_launch_ep_apply with a statistics epilogue)
    if (!pa_stats_groups_ok(C)) { pa_set_error_msg("pa_residual_fwd_bwd: " PA_STATS_GROUPS_MSG); return 1; }
    ResidualOp op; Net& n = op.n;
    n.is_agent = true; n.B = B; n.st = ST(s);
    op.r.declare(n, "", C, C, false);
    op.build(B, H, W, C, reinterpret_cast<char*>(ws));
    n.params = const_cast<float*>(params); n.grads = grads; n.buffers = buffers;
    TRY(n.upload_tables());
    TRY(n.prepare_weights());
    TRY(n.begin_step());
    n.train_bn = true;
    TRY(pa_launch_nchw_f32_to_nhwc_bf16(x, op.in.raw, B, C, H, W, n.st));
    TRY(op.r.fwd(n, op.in));
    TRY(pa_launch_nhwc_bf16_to_nchw_f32(n.op(op.r.x3), y, B, C, H, W, n.st));
    if (dy) {
        bf16* g = op.r.x1.grad;    // borrow as staging for the incoming gradient (overwritten later by bwd)
        // x1 is narrower than x3: stage in the input's gradient buffer instead
        g = op.in.grad;
        TRY(pa_launch_nchw_f32_to_nhwc_bf16(dy, g, B, C, H, W, n.st));
        TRY(pa_launch_ep_apply(pa_plain(g), n.final_ep(op.r.x3), op.r.x3.grad, (size_t)B * H * W, C, n.st));
        TRY(n.finish_grad(op.r.x3));
        TRY(op.r.bwd(n, op.in, pa_none(), true));
        TRY(n.reduce_grads());
        TRY(pa_launch_nhwc_bf16_to_nchw_f32(pa_plain(op.in.grad), dx, B, C, H, W, n.st));
    }
    PA_CHECK(hipStreamSynchronize(n.st));
    return 0;
}

// ---------------------------------------------------------------------------- single convolution ops
// Plain conv2d (k = 1 or 3, stride 1, 'same') through the implicit-GEMM kernels: NCHW fp32 in/out,
// PyTorch-layout fp32 weights; bf16 operands, fp32 accumulation.  mode: 0 forward (y = conv(x,w)+b),
// 1 data gradient (dx = conv^T(dy, w)), 2 weight gradient (dw, db from dy and x).
struct ConvOp {
    Net n; ConvLayer c; bf16 *xin = nullptr, *yout = nullptr;
    size_t build(int B, int H, int W, char* base) {
        Arena a; a.base = base;
        n.prep_jobs = a.get<PaPrepJob>(1); n.red_jobs = a.get<PaWgradReduceJob>(1); n.bneval_jobs = a.get<PaBnEvalJob>(1);
        n.layout_conv(c, a, B * H * W, H, W);
        xin = a.get<bf16>((size_t)B * H * W * c.pcin);
        yout = a.get<bf16>((size_t)B * H * W * c.pcout);
        a.take(0);
        return a.off;
    }
};

// An upper bound: laid out without the net's batch, the layer gets the slab count of a launch alone (PaWgradPlan::splits); pa_conv2d lays it
// out with the batch and may get the grouped count, which is never larger (tests/test_conv_exact_cpu.py sweeps the rule).
size_t pa_conv2d_workspace_bytes(int B, int Cin, int Cout, int H, int W, int k) {
    ConvOp op; op.n.is_agent = true; op.n.declare_conv(op.c, "c", Cin, Cout, k, false);
    return op.build(B, H, W, nullptr);
}

int pa_conv2d(int mode, const float* a_in, const float* b_in, const float* w, const float* bias, float* out, float* out2,
              int B, int Cin, int Cout, int H, int W, int k, void* ws, void* s) {
    g_err[0] = 0;
    if (Cin % 64 || Cout % 64 || (k != 1 && k != 3)) { pa_set_error_msg("pa_conv2d: channels % 64 == 0, k in {1,3}"); return 1; }
    ConvOp op; Net& n = op.n; n.is_agent = true; n.B = B; n.st = ST(s);
    // mode 2 without out2: no bias gradient wanted (the case of every conv in front of a BatchNorm)
    n.declare_conv(op.c, "c", Cin, Cout, k, mode == 2 && out2 == nullptr);
    op.build(B, H, W, reinterpret_cast<char*>(ws));
    // parameter block: [weight | bias] as declared
    float* pbuf = nullptr; float* gbuf = nullptr;
    PA_CHECK(hipMallocAsync((void**)&pbuf, n.n_params * sizeof(float) * 2 + 64, n.st));
    gbuf = pbuf + ((n.n_params + 3) & ~(size_t)3);
    PA_CHECK(hipMemsetAsync(pbuf, 0, n.n_params * sizeof(float) * 2 + 64, n.st));
    PA_CHECK(hipMemcpyAsync(pbuf + op.c.p_w, w, (size_t)Cout * Cin * k * k * sizeof(float), hipMemcpyDeviceToDevice, n.st));
    if (bias) PA_CHECK(hipMemcpyAsync(pbuf + op.c.p_b, bias, Cout * sizeof(float), hipMemcpyDeviceToDevice, n.st));
    n.params = pbuf; n.grads = gbuf; n.buffers = pbuf;
    TRY(n.upload_tables());
    TRY(n.prepare_weights());
    n.train_bn = false;
    if (mode == 0) {
        TRY(pa_launch_nchw_f32_to_nhwc_bf16(a_in, op.xin, B, Cin, H, W, n.st));
        TRY(n.conv_fwd(op.c, pa_plain(op.xin), B, H, W, pa_none(), pa_none(), op.yout, nullptr));
        TRY(pa_launch_nhwc_bf16_to_nchw_f32(pa_plain(op.yout), out, B, Cout, H, W, n.st));
    } else if (mode == 1) {
        PaEpilogue ep; memset(&ep, 0, sizeof ep); ep.mode = PA_OUT_PLAIN;
        TRY(pa_launch_nchw_f32_to_nhwc_bf16(a_in, op.yout, B, Cout, H, W, n.st));
        TRY(n.conv_dgrad(op.c, pa_plain(op.yout), B, H, W, pa_none(), pa_none(), ep, op.xin));
        TRY(pa_launch_nhwc_bf16_to_nchw_f32(pa_plain(op.xin), out, B, Cin, H, W, n.st));
    } else {
        TRY(pa_launch_nchw_f32_to_nhwc_bf16(a_in, op.yout, B, Cout, H, W, n.st));
        TRY(pa_launch_nchw_f32_to_nhwc_bf16(b_in, op.xin, B, Cin, H, W, n.st));
        TRY(n.conv_wgrad(op.c, pa_plain(op.yout), pa_plain(op.xin), B, H, W));
        TRY(n.reduce_grads());
        PA_CHECK(hipMemcpyAsync(out, gbuf + op.c.p_w, (size_t)Cout * Cin * k * k * sizeof(float), hipMemcpyDeviceToDevice, n.st));
        if (out2) PA_CHECK(hipMemcpyAsync(out2, gbuf + op.c.p_b, Cout * sizeof(float), hipMemcpyDeviceToDevice, n.st));
    }
    PA_CHECK(hipStreamSynchronize(n.st));
    PA_CHECK(hipFree(pbuf));
    return 0;
}

// ---------------------------------------------------------------------------- grouped weight gradients
// n <= 8 INDEPENDENT weight gradients (the three or four of a residual block, reference models/asn_stacked_hg.py:17-24) as the training
// step submits them: ONE wgrad_group_kernel launch (conv_wgrad_tile.hip) + the slab reduction -- or, for comparison, the same layers
// launched one by one.  The operator-level door to the group kernel for the parity tests (tests/test_gpu_conv.py).
struct WgradGroupOp {
    Net n; ConvLayer c[PA_WG_GROUP_MAX]; bf16 *dy[PA_WG_GROUP_MAX], *dyq[PA_WG_GROUP_MAX], *x[PA_WG_GROUP_MAX];
    float *pbuf = nullptr, *gbuf = nullptr;
    size_t build(const pa_wgrad_job* jobs, int nj, char* base) {
        Arena a; a.base = base;
        n.prep_jobs = a.get<PaPrepJob>(nj); n.red_jobs = a.get<PaWgradReduceJob>(nj); n.bneval_jobs = a.get<PaBnEvalJob>(1);
        for (int j = 0; j < nj; ++j) {
            const pa_wgrad_job& q = jobs[j];
            n.B = q.B;                                      // (layout_conv picks the grouped split count for M == B * H * W)
            n.layout_conv(c[j], a, q.B * q.H * q.W, q.H, q.W);
            const size_t M = (size_t)q.B * q.H * q.W;
            dy[j] = a.get<bf16>(M * c[j].pcout);
            dyq[j] = q.dy_q ? a.get<bf16>(M * c[j].pcout) : nullptr;
            x[j] = a.get<bf16>(M * c[j].pcin);
        }
        pbuf = a.get<float>(n.n_params + 8);
        gbuf = a.get<float>(n.n_params + 8);
        a.take(0);
        return a.off;
    }
    int declare(const pa_wgrad_job* jobs, int nj) {
        if (nj < 1 || nj > PA_WG_GROUP_MAX) { pa_set_error_msg("pa_wgrad_group: 1 .. 8 jobs"); return 1; }
        n.is_agent = true;
        for (int j = 0; j < nj; ++j) {
            const pa_wgrad_job& q = jobs[j];
            if (q.Cin % 64 || q.Cout % 64 || (q.k != 1 && q.k != 3) || q.B < 1 || q.H < 1 || q.W < 1) { pa_set_error_msg("pa_wgrad_group: channels % 64 == 0, k in {1,3}"); return 1; }
            if ((q.dy_q == nullptr) != (q.dy_k == nullptr)) { pa_set_error_msg("pa_wgrad_group: dy_q and dy_k come together"); return 1; }
            char name[16]; snprintf(name, sizeof name, "j%d", j);
            n.declare_conv(c[j], name, q.Cin, q.Cout, q.k, q.db == nullptr);
        }
        return 0;
    }
};

size_t pa_wgrad_group_workspace_bytes(const pa_wgrad_job* jobs, int njobs) {
    g_err[0] = 0;
    WgradGroupOp op;
    if (op.declare(jobs, njobs)) return 0;
    return op.build(jobs, njobs, nullptr);
}

int pa_wgrad_group(const pa_wgrad_job* jobs, int njobs, int mode, void* ws, void* s) {
    g_err[0] = 0;
    WgradGroupOp op; Net& n = op.n;
    TRY(op.declare(jobs, njobs));
    n.st = ST(s);
    op.build(jobs, njobs, reinterpret_cast<char*>(ws));
    PA_CHECK(hipMemsetAsync(op.gbuf, 0, (n.n_params + 8) * sizeof(float), n.st));
    n.params = op.pbuf; n.grads = op.gbuf; n.buffers = op.pbuf;
    TRY(n.upload_tables());
    PaWgradArgs args[PA_WG_GROUP_MAX]; const PaWgradArgs* ptrs[PA_WG_GROUP_MAX];
    for (int j = 0; j < njobs; ++j) {
        const pa_wgrad_job& q = jobs[j];
        ConvLayer& c = op.c[j];
        TRY(pa_launch_nchw_f32_to_nhwc_bf16(q.dy, op.dy[j], q.B, q.Cout, q.H, q.W, n.st));
        if (q.dy_q) TRY(pa_launch_nchw_f32_to_nhwc_bf16(q.dy_q, op.dyq[j], q.B, q.Cout, q.H, q.W, n.st));
        TRY(pa_launch_nchw_f32_to_nhwc_bf16(q.x, op.x[j], q.B, q.Cin, q.H, q.W, n.st));
        PaWgradArgs& a = args[j]; memset(&a, 0, sizeof a);
        a.dy = pa_plain(op.dy[j]);
        if (q.dy_q) { a.dy.mode = PA_LD_LIN2; a.dy.q = op.dyq[j]; a.dy.k0 = q.dy_k; a.dy.k1 = q.dy_k + q.Cout; a.dy.k2 = q.dy_k + 2 * q.Cout; }
        a.x = pa_plain(op.x[j]);
        if (q.x_k) { a.x.mode = PA_LD_BNRELU; a.x.k0 = q.x_k; a.x.k1 = q.x_k + q.Cin; }
        a.part = c.part; a.dbpart = c.dbpart;
        a.B = q.B; a.H = q.H; a.W = q.W; a.Cin = c.pcin; a.Cout = c.pcout; a.taps = c.taps(); a.splits = c.splits;
        ptrs[j] = &a;
    }
    if (mode == 0) {
        for (int j = 0; j < njobs; ++j) TRY(pa_launch_wgrad(args[j], n.st));
    } else {
        for (int j = 0; j < njobs; ++j)
            if (pa_wgrad_job_workgroups(args[j]) == 0) { pa_set_error_msg("pa_wgrad_group: a job the grouped kernel does not take (shape / operand modes)"); return 2; }
        TRY(pa_launch_wgrad_group(ptrs, njobs, n.st, mode == 2));
    }
    TRY(pa_launch_wgrad_reduce(n.red_jobs, n.n_red, n.red_max, n.st));
    for (int j = 0; j < njobs; ++j) {
        const pa_wgrad_job& q = jobs[j];
        PA_CHECK(hipMemcpyAsync(q.dw, op.gbuf + op.c[j].p_w, (size_t)q.Cout * q.Cin * q.k * q.k * sizeof(float), hipMemcpyDeviceToDevice, n.st));
        if (q.db) PA_CHECK(hipMemcpyAsync(q.db, op.gbuf + op.c[j].p_b, q.Cout * sizeof(float), hipMemcpyDeviceToDevice, n.st));
    }
    PA_CHECK(hipStreamSynchronize(n.st));
    return 0;
}

// micro-benchmark of ONE conv launch (tools/bench_conv.py): variant bits select what the launch does
//   bit0: input transform BNRELU (fwd) / LIN2 (dgrad, wgrad dy)      bit1: epilogue STATS (fwd) / BWD (dgrad)
//   bit2: one residual addend                                         bit3 (wgrad): x operand BNRELU
// Returns the average milliseconds per launch over `iters` launches (HIP events on the stream).
int pa_conv2d_time(int mode, int variant, int B, int Cin, int Cout, int H, int W, int k, int iters, void* ws, float* ms_out, void* s) {
    g_err[0] = 0;
    ConvOp op; Net& n = op.n; n.is_agent = true; n.B = B; n.st = ST(s);
    n.declare_conv(op.c, "c", Cin, Cout, k, false);
    BNLayer bn_in, bn_out;
    n.declare_bn(bn_in, "bi", mode == 0 ? Cin : Cout);
    n.declare_bn(bn_out, "bo", mode == 0 ? Cout : Cin);
    Arena a; a.base = reinterpret_cast<char*>(ws);
    a.off = op.build(B, H, W, a.base);
    for (BNLayer* b : n.bns) n.layout_bn(*b, a, B * H * W);
    const size_t M = (size_t)B * H * W;
    bf16* extra = a.get<bf16>(M * (Cin > Cout ? Cin : Cout));      // residual addend / xref / second LIN2 operand
    bf16* extra2 = a.get<bf16>(M * (Cin > Cout ? Cin : Cout));
    float* pbuf = a.get<float>(2 * (n.n_params + 8));
    n.params = pbuf; n.grads = pbuf + n.n_params + 8; n.buffers = pbuf;
    TRY(n.upload_tables());
    auto mk = [&](const bf16* p, BNLayer& b, int md) { PaOperand o = pa_plain(p); o.mode = md; o.q = extra2; o.k0 = b.scale; o.k1 = b.shift; o.k2 = b.kA; return o; };
    hipEvent_t e0, e1;
    PA_CHECK(hipEventCreate(&e0)); PA_CHECK(hipEventCreate(&e1));
    auto once = [&]() -> int {
        if (mode == 0) {
            PaConvArgs c; memset(&c, 0, sizeof c);
            c.in = mk(op.xin, bn_in, (variant & 1) ? PA_LD_BNRELU : PA_LD_PLAIN); c.w = op.c.wf; c.bias = pbuf; c.out = op.yout;
            c.add1 = (variant & 4) ? pa_plain(extra) : pa_none(); c.add2 = pa_none();
            c.B = B; c.H = H; c.W = W; c.Cin = Cin; c.Cout = Cout; c.taps = k * k;
            c.ep.mode = (variant & 2) ? PA_OUT_STATS : PA_OUT_PLAIN; c.ep.stats = bn_out.stats;
            return pa_launch_conv(c, n.st);
        } else if (mode == 1) {
            PaConvArgs c; memset(&c, 0, sizeof c);
            c.in = mk(op.yout, bn_in, (variant & 1) ? PA_LD_LIN2 : PA_LD_PLAIN); c.w = op.c.wb; c.out = op.xin;
            c.add1 = (variant & 4) ? pa_plain(extra) : pa_none(); c.add2 = pa_none();
            c.B = B; c.H = H; c.W = W; c.Cin = Cout; c.Cout = Cin; c.taps = k * k;
            c.ep.mode = (variant & 2) ? PA_OUT_BWD : PA_OUT_PLAIN; c.ep.stats = bn_out.bstats; c.ep.xref = extra;
            c.ep.scale = bn_out.scale; c.ep.shift = bn_out.shift; c.ep.mean = bn_out.mean; c.ep.invstd = bn_out.invstd;
            return pa_launch_conv(c, n.st);
        } else {
            PaWgradArgs g; memset(&g, 0, sizeof g);
            g.dy = mk(op.yout, bn_in, (variant & 1) ? PA_LD_LIN2 : PA_LD_PLAIN);
            g.x = mk(op.xin, bn_out, (variant & 8) ? PA_LD_BNRELU : PA_LD_PLAIN);
            g.part = op.c.part; g.dbpart = nullptr; g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.taps = k * k; g.splits = op.c.splits;
            return pa_launch_wgrad(g, n.st);
        }
    };
    for (int i = 0; i < 3; ++i) TRY(once());
    float ms = 0.f;
    if (variant & 16) {            // COLD: 640 MB of other traffic between launches (the Infinity Cache holds 256 MB), one event pair per launch
        char* scratch = a.get<char>((size_t)640 << 20);
        for (int i = 0; i < iters; ++i) {
            PA_CHECK(hipMemsetAsync(scratch, i & 1, (size_t)640 << 20, n.st));
            PA_CHECK(hipEventRecord(e0, n.st));
            TRY(once());
            PA_CHECK(hipEventRecord(e1, n.st));
            PA_CHECK(hipEventSynchronize(e1));
            float t = 0.f;
            PA_CHECK(hipEventElapsedTime(&t, e0, e1));
            ms += t;
        }
    } else {
        PA_CHECK(hipEventRecord(e0, n.st));
        for (int i = 0; i < iters; ++i) TRY(once());
        PA_CHECK(hipEventRecord(e1, n.st));
        PA_CHECK(hipEventSynchronize(e1));
        PA_CHECK(hipEventElapsedTime(&ms, e0, e1));
    }
    *ms_out = ms / iters;
    hipEventDestroy(e0); hipEventDestroy(e1);
    return 0;
}

// ---------------------------------------------------------------------------- networks
static pa_net* hg_create(const char* who, int num_stacks, int num_modules, int num_classes, int chan, int B, int res) {
    g_err[0] = 0;
    char msg[160];
    if (num_modules < 1 || num_modules > 8) {
        snprintf(msg, sizeof msg, "%s: need 1 <= num_modules <= 8", who);
        pa_set_error_msg(msg);
        return nullptr;
    }
    if (num_classes != 16 || chan % 128 != 0 || chan > 2048 || res % 64 != 0 || B < 1 || num_stacks < 1) {
        snprintf(msg, sizeof msg, "%s: need num_classes == 16, chan %% 128 == 0, res %% 64 == 0", who);
        pa_set_error_msg(msg);
        return nullptr;
    }
    if (!pa_stats_groups_ok(chan)) { snprintf(msg, sizeof msg, "%s: " PA_STATS_GROUPS_MSG, who); pa_set_error_msg(msg); return nullptr; }
    pa_net* p = new (std::nothrow) pa_net;
    if (!p) return nullptr;
    Net& n = p->n;
    n.stacks = num_stacks; n.modules = num_modules; n.classes = num_classes; n.chan = chan; n.B = B; n.res = res;
    n.declare_pose();
    n.workspace_bytes = n.layout_all(nullptr);
    return p;
}

pa_net* pa_hg_create(int num_stacks, int num_classes, int chan, int B, int res) {
    return hg_create("pa_hg_create", num_stacks, 1, num_classes, chan, B, res);
}

pa_net* pa_hg_create_modules(int num_stacks, int num_modules, int num_classes, int chan, int B, int res) {
    return hg_create("pa_hg_create_modules", num_stacks, num_modules, num_classes, chan, B, res);
}

int pa_net_num_modules(const pa_net* net) { return net->n.is_agent ? 1 : net->n.modules; }

pa_net* pa_asn_create(int chan, int scale_num, int rotation_num, int B, int res) {
    g_err[0] = 0;
    if (chan % 128 != 0 || chan > 512 || res % 64 != 0 || B < 1 || scale_num < 1 || rotation_num < 1 || scale_num + rotation_num > 64) {
        pa_set_error_msg("pa_asn_create: need chan % 128 == 0, res % 64 == 0, scale_num + rotation_num <= 64");
        return nullptr;
    }
    if (!pa_stats_groups_ok(chan)) { pa_set_error_msg("pa_asn_create: " PA_STATS_GROUPS_MSG); return nullptr; }
    // the head is AvgPool2d(4) + view + Linear(chan, K) (reference :375, :430-436): the pool of the res / 64 top map must have exactly
    // one output (a map below 4 x 4 has none: the reference raises; from 8 x 8 on there are four and its Linear does not fit)
    if (res / 64 < 4 || res / 64 > 7) {
        pa_set_error_msg("pa_asn_create: need 256 <= res <= 448 (a res / 64 top map of 4 x 4 .. 7 x 7: one AvgPool2d(4) window)");
        return nullptr;
    }
    pa_net* p = new (std::nothrow) pa_net;
    if (!p) return nullptr;
    Net& n = p->n;
    n.chan = chan; n.B = B; n.res = res; n.scale_num = scale_num; n.rot_num = rotation_num; n.stacks = 0;
    n.declare_asn();
    n.workspace_bytes = n.layout_asn(nullptr);
    return p;
}

pa_net* pa_asn_create_dropout(int chan, int B, int res) {
    g_err[0] = 0;
    if (chan % 128 != 0 || chan > 512 || res != 256 || B < 1) {      // the 4x4 cell mask is the neck map of a 256 input (reference :79-100)
        pa_set_error_msg("pa_asn_create_dropout: need chan % 128 == 0 and res == 256 (4x4 neck map)");
        return nullptr;
    }
    if (!pa_stats_groups_ok(chan)) { pa_set_error_msg("pa_asn_create_dropout: " PA_STATS_GROUPS_MSG); return nullptr; }
    pa_net* p = new (std::nothrow) pa_net;
    if (!p) return nullptr;
    Net& n = p->n;
    n.chan = chan; n.B = B; n.res = res; n.stacks = 0; n.asn_dropout = true;
    n.declare_asn();
    n.workspace_bytes = n.layout_asn(nullptr);
    return p;
}

static int check_agent_pair(const pa_net* asn, const pa_net* pose, const char* who) {
    if (!asn->n.is_agent || pose->n.is_agent || asn->n.B != pose->n.B || asn->n.chan != pose->n.chan || asn->n.res != pose->n.res) {
        char buf[160]; snprintf(buf, sizeof buf, "%s: agent and pose net must be built for the same batch, width and resolution", who);
        pa_set_error_msg(buf);
        return 1;
    }
    return 0;
}

int pa_asn_forward_masks(pa_net* asn, pa_net* pose, int train, float* mask_logits) {
    g_err[0] = 0;
    TRY(check_agent_pair(asn, pose, "pa_asn_forward_masks"));
    asn->n.bn_update = (train == 2) ? 0 : 1;
    const int r = asn->n.asn_forward_masks(pose->n, train != 0, mask_logits);
    asn->n.bn_update = 1;
    return r;
}

int pa_asn_backward_masks(pa_net* asn, pa_net* pose, const float* dlogits) {
    g_err[0] = 0;
    TRY(check_agent_pair(asn, pose, "pa_asn_backward_masks"));
    if (!dlogits) { pa_set_error_msg("pa_asn_backward_masks: dlogits == NULL"); return 1; }
    return asn->n.asn_backward_masks(pose->n, dlogits);
}

int pa_hg_set_dropout_masks(pa_net* net, const float* masks) {
    g_err[0] = 0;
    if (net->n.is_agent) { pa_set_error_msg("pa_hg_set_dropout_masks: not a pose net"); return 1; }
    if (masks && net->n.res != 256) { pa_set_error_msg("pa_hg_set_dropout_masks: the 4x4 cell mask needs res == 256 (4x4 neck map)"); return 1; }
    net->n.drop_mask = masks;
    return 0;
}

int pa_hg_set_heat_grads(pa_net* net, const float* const* grads_host, int layout) {
    g_err[0] = 0;
    Net& n = net->n;
    if (n.is_agent) { pa_set_error_msg("pa_hg_set_heat_grads: not a pose net"); return 1; }
    if (!grads_host) { n.heat_grads_on = false; n.heat_grads.clear(); return 0; }
    if (layout != 0 && layout != 1) { pa_set_error_msg("pa_hg_set_heat_grads: layout must be 0 ([B][16][H][W]) or 1 ([B][H*W][16])"); return 1; }
    bool any = false;
    for (int i = 0; i < n.stacks; ++i) {
        any = any || grads_host[i] != nullptr;
        if (reinterpret_cast<uintptr_t>(grads_host[i]) & 15) { pa_set_error_msg("pa_hg_set_heat_grads: every gradient must be 16-byte aligned"); return 1; }
    }
    if (!any) { pa_set_error_msg("pa_hg_set_heat_grads: every entry is NULL (pass grads_host == NULL to switch the given gradients off)"); return 1; }
    n.heat_grads.assign(grads_host, grads_host + n.stacks);
    n.heat_grads_layout = layout;
    n.heat_grads_on = true;
    return 0;
}

int pa_hg_set_image_grad(pa_net* net, float* dimg, int layout) {
    g_err[0] = 0;
    Net& n = net->n;
    if (n.is_agent) { pa_set_error_msg("pa_hg_set_image_grad: not a pose net"); return 1; }
    if (!dimg) { n.image_grad = nullptr; n.image_grad_layout = 0; return 0; }
    if (layout != 0 && layout != 1) { pa_set_error_msg("pa_hg_set_image_grad: layout must be 0 ([B][3][res][res]) or 1 ([B][res][res][4])"); return 1; }
    if (reinterpret_cast<uintptr_t>(dimg) & 15) { pa_set_error_msg("pa_hg_set_image_grad: the gradient must be 16-byte aligned"); return 1; }
    n.image_grad = dimg; n.image_grad_layout = layout;
    return 0;
}

// The stem's data gradient as an operator (tests/test_gpu_image_grad.py): dy and w are rounded once to the storage type, the result is the plain
// transposed convolution (no gradient scale).  Workspace: dy as NHWC 16-bit + the packed weight copy.
static size_t stem_dgrad_ws(int B, int H, int W, size_t* wf_off) {
    const size_t g = ((size_t)B * (H / 2) * (W / 2) * 64 * sizeof(bf16) + 255) & ~(size_t)255;
    if (wf_off) *wf_off = g;
    return g + 64 * 256 * sizeof(bf16);
}
size_t pa_stem_dgrad_workspace_bytes(int B, int H, int W) {
    if (B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return 0;
    return stem_dgrad_ws(B, H, W, nullptr);
}
int pa_stem_dgrad(const float* dy, const float* w, float* dx, int B, int H, int W, int layout, void* ws, void* s) {
    g_err[0] = 0;
    if (!dy || !w || !dx || !ws) { pa_set_error_msg("pa_stem_dgrad: dy, w, dx and ws must not be NULL"); return 1; }
    if (B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) { pa_set_error_msg("pa_stem_dgrad: B >= 1, H and W even and >= 2"); return 1; }
    if (layout != 0 && layout != 1) { pa_set_error_msg("pa_stem_dgrad: layout must be 0 ([B][3][H][W]) or 1 ([B][H][W][4])"); return 1; }
    if ((reinterpret_cast<uintptr_t>(dx) & 15) || (reinterpret_cast<uintptr_t>(ws) & 15)) { pa_set_error_msg("pa_stem_dgrad: dx and ws must be 16-byte aligned"); return 1; }
    size_t wf_off = 0; stem_dgrad_ws(B, H, W, &wf_off);
    bf16* g16 = reinterpret_cast<bf16*>(ws);
    bf16* wf = reinterpret_cast<bf16*>(reinterpret_cast<char*>(ws) + wf_off);
    TRY(pa_launch_nchw_f32_to_nhwc_bf16(dy, g16, B, 64, H / 2, W / 2, ST(s)));
    TRY(pa_launch_stem_pack(w, wf, ST(s)));
    PaStemDgradArgs d; memset(&d, 0, sizeof d);
    d.g = pa_plain(g16); d.wf = wf; d.out = dx; d.B = B; d.Hm = H / 2; d.Wm = W / 2; d.layout = layout; d.scale = 1.f;
    TRY(pa_launch_stem_dgrad(d, ST(s)));
    return 0;
}

int pa_weighted_l2_grad(const float* pred, const float* gt, const float* weight, size_t n, const float* gout_dev, float* dpred, void* s) {
    g_err[0] = 0;
    if (!pred || !gt || !gout_dev || !dpred) { pa_set_error_msg("pa_weighted_l2_grad: pred, gt, gout_dev and dpred must not be NULL"); return 1; }
    TRY(pa_launch_weighted_l2_grad(pred, gt, weight, n, gout_dev, dpred, ST(s))); return 0;
}

int pa_hg_forward_half(pa_net* net, const float* img, const void* img4, int train) {
    g_err[0] = 0;
    if (!img && !img4) { pa_set_error_msg("pa_hg_forward_half: need img or img4"); return 1; }
    net->n.bn_update = (train == 2) ? 0 : 1;        // train == 2: batch statistics, running estimates untouched
    const int r = net->n.forward_half(img, reinterpret_cast<const bf16*>(img4), train != 0);
    net->n.bn_update = 1;
    return r;
}

int pa_asn_forward(pa_net* asn, pa_net* pose, int train, float* logits_scale, float* logits_rot) {
    g_err[0] = 0;
    if (!asn->n.is_agent || pose->n.is_agent || asn->n.B != pose->n.B || asn->n.chan != pose->n.chan || asn->n.res != pose->n.res) {
        pa_set_error_msg("pa_asn_forward: agent and pose net must be built for the same batch, width and resolution");
        return 1;
    }
    asn->n.bn_update = (train == 2) ? 0 : 1;       // train == 2: batch statistics, running estimates untouched
    TRY(asn->n.asn_forward(pose->n, train != 0, logits_scale, logits_rot));
    asn->n.bn_update = 1;
    return 0;
}

int pa_asn_backward(pa_net* asn, pa_net* pose, const float* target_scale, const float* target_rot, float* loss) {
    g_err[0] = 0;
    TRY(asn->n.asn_backward(pose->n, target_scale, target_rot, loss));
    return 0;
}

const float* pa_asn_probs(const pa_net* asn) { return asn->n.asn_probs; }
int pa_asn_set_log_eps(pa_net* asn, float eps) { asn->n.asn_log_eps = eps; return 0; }

void pa_net_destroy(pa_net* net) { if (net) { net->n.release_streams(); delete net; } }

int pa_net_num_tensors(const pa_net* net) { return (int)net->n.tensors.size(); }

int pa_net_tensor_info(const pa_net* net, int i, char* name, int name_cap, int* shape4, int* ndim, size_t* offset, size_t* numel,
                       int* kind) {
    if (i < 0 || i >= (int)net->n.tensors.size()) { pa_set_error_msg("pa_net_tensor_info: index out of range"); return 1; }
    const TensorInfo& t = net->n.tensors[i];
    snprintf(name, name_cap, "%s", t.name.c_str());
    for (int k = 0; k < 4; ++k) shape4[k] = t.shape[k];
    *ndim = t.ndim; *offset = t.offset; *numel = t.numel; *kind = t.is_buffer;
    return 0;
}

size_t pa_net_param_floats(const pa_net* net) { return net->n.n_params; }
size_t pa_net_buffer_floats(const pa_net* net) { return net->n.n_buffers; }
size_t pa_net_workspace_bytes(const pa_net* net) { return net->n.workspace_bytes; }

int pa_net_bind(pa_net* net, float* params, float* grads, float* buffers, void* workspace, void* s) {
    g_err[0] = 0;
    Net& n = net->n;
    n.release_graph();                    // (a captured step holds the old pointers)
    n.params = params; n.grads = grads; n.buffers = buffers; n.workspace = reinterpret_cast<char*>(workspace); n.st = ST(s);
    const size_t bytes = n.is_agent ? n.layout_asn(n.workspace) : n.layout_all(n.workspace);
    // the layout relies on zeros in a few places (padding channels of the 16-channel head tensors, statistic accumulators):
    // clear the whole workspace here, once, so that the caller does not have to
    PA_CHECK(hipMemsetAsync(n.workspace, 0, bytes, n.st));
    TRY(n.upload_tables());
    return n.prepare_weights();
}

int pa_net_prepare_weights(pa_net* net) { g_err[0] = 0; TRY(net->n.prepare_weights()); return 0; }

int pa_hg_forward(pa_net* net, const float* img, const void* img4, const double* pts, int train, float* loss_per_stack) {
    g_err[0] = 0;
    if (!img && !img4) { pa_set_error_msg("pa_hg_forward: need img or img4"); return 1; }
    TRY(net->n.forward_pose(img, reinterpret_cast<const bf16*>(img4), pts, train != 0, loss_per_stack));
    return 0;
}

const float* pa_hg_heatmap_nhwc(const pa_net* net, int stack) { return net->n.heat[stack]; }

int pa_hg_heatmap_nchw(pa_net* net, int stack, float* out) {
    Net& n = net->n;
    TRY(pa_launch_nhwc_to_nchw_f32(n.heat[stack], out, n.B, n.res / 4, n.res / 4, 16, n.st));
    return 0;
}

int pa_hg_backward(pa_net* net) { g_err[0] = 0; TRY(net->n.backward_pose()); return 0; }

int pa_hg_backward_phase(pa_net* net, int phase) {
    g_err[0] = 0;
    Net& n = net->n;
    if (phase < 0 || phase > n.stacks) { pa_set_error_msg("pa_hg_backward_phase: phase out of range"); return 1; }
    TRY(n.ensure_streams());
    if (phase == n.stacks) return n.backward_stem();
    return n.backward_stack(n.stacks - 1 - phase);
}

int pa_hg_bucket_range(const pa_net* net, int stack, size_t* lo, size_t* hi) {
    const Net& n = net->n;
    char prefix[32]; snprintf(prefix, sizeof prefix, "hg.%d.", stack);
    size_t a = (size_t)-1, b = 0;
    for (const TensorInfo& t : n.tensors)
        if (t.is_buffer == 0 && t.name.compare(0, strlen(prefix), prefix) == 0) { if (t.offset < a) a = t.offset; if (t.offset + t.numel > b) b = t.offset + t.numel; }
    if (b == 0) { pa_set_error_msg("pa_hg_bucket_range: no such stack"); return 1; }
    // the caller all-reduces [lo, hi) EARLY and skips it at the end: no other parameter may live inside the range (this holds
    // by the declaration order of declare_pose; a parameter interleaved later would be reduced before its gradient is final)
    for (const TensorInfo& t : n.tensors)
        if (t.is_buffer == 0 && t.name.compare(0, strlen(prefix), prefix) != 0 && t.offset < b && t.offset + t.numel > a) {
            pa_set_error_msg("pa_hg_bucket_range: a parameter of another module lies inside the stack's range");
            return 1;
        }
    *lo = a; *hi = b;
    return 0;
}

int pa_hg_bucket_wait(pa_net* net, int stack, void* stream) {
    g_err[0] = 0;
    Net& n = net->n;
    const int r = n.mark_bucket(stack);
    if (r < 0) return -1;                      // no early bucket in this stream mode: exchange everything at the end
    if (r > 0) return r;
    PA_CHECK(hipStreamWaitEvent(ST(stream), n.ev_bucket[stack], 0));
    return 0;
}

int pa_hg_train_step(pa_net* net, const void* img4, const double* pts, int train, int use_graph, float* loss_per_stack) {
    g_err[0] = 0;
    Net& n = net->n;
    if (!img4 || !pts) { pa_set_error_msg("pa_hg_train_step: img4 and pts are required"); return 1; }
    // (a captured graph holds the pointers of its capture: the same rule as for dropout masks, refused before anything is enqueued)
    if (use_graph && n.image_grad) { pa_set_error_msg("pa_hg_train_step: no captured graph while an image gradient is set (pa_hg_set_image_grad)"); return 1; }
    if (use_graph && n.heat_grads_on) { pa_set_error_msg("pa_hg_train_step: no captured graph while heat-map gradients are set (pa_hg_set_heat_grads)"); return 1; }
    if (!use_graph) {
        TRY(n.forward_pose(nullptr, reinterpret_cast<const bf16*>(img4), pts, train != 0, loss_per_stack));
        return n.backward_pose();
    }
    // the graph reads the engine's own input buffers: bring the caller's tensors there first (12.6 MB + 6 KB at B = 24)
    if (img4 != n.img4) PA_CHECK(hipMemcpyAsync(n.img4, img4, (size_t)n.B * n.res * n.res * 4 * sizeof(bf16), hipMemcpyDeviceToDevice, n.st));
    if (pts != n.pts_dev) PA_CHECK(hipMemcpyAsync(n.pts_dev, pts, (size_t)n.B * n.classes * 2 * sizeof(double), hipMemcpyDeviceToDevice, n.st));
    TRY(n.train_step_graph(train != 0));
    if (loss_per_stack) PA_CHECK(hipMemcpyAsync(loss_per_stack, n.loss_keep, n.stacks * sizeof(float), hipMemcpyDeviceToDevice, n.st));
    if (n.loss_total_out) PA_CHECK(hipMemcpyAsync(n.loss_total_out, n.loss_keep + n.stacks, sizeof(float), hipMemcpyDeviceToDevice, n.st));
    return 0;
}

// total_dev: a device float that every later pa_hg_forward / pa_hg_train_step with `pts` also writes the SUM of the per-stack losses to
// (NULL: off).  The reference sums them on the host side of autograd (stack-hg.py:156-159); here the caller gets the scalar without a
// reduction launch of its own between the backward pass and the optimizer.
int pa_hg_set_loss_total(pa_net* net, float* total_dev) {
    g_err[0] = 0;
    if (net->n.loss_total_out != total_dev) { net->n.loss_total_out = total_dev; net->n.release_graph(); }      // (a captured step holds the pointer by value)
    return 0;
}

int pa_hg_accuracy(pa_net* net, int stack, const int32_t* idxs, int nidx, float* acc, float* scratch) {
    g_err[0] = 0;
    Net& n = net->n;
    const int H = n.res / 4, J = 16, B = n.B;
    float* tgt = scratch;                         // [B][16][H][H]
    float* gp = tgt + (size_t)B * J * H * H + (size_t)B * J * 2;      // [B][16][2]
    float* norm = gp + (size_t)B * J * 2;         // [B]
    const float* pp = nullptr;                    // [B][16][2] arg-max of the heat maps (shared with pa_hg_pckh)
    hipStream_t ms;
    TRY(n.meter_stream(&ms));
    TRY(n.heat_argmax(stack, &pp, ms));
    TRY(pa_launch_gaussian_heatmap(n.pts_dev, tgt, B, J, H, H, ms));
    TRY(pa_launch_argmax(tgt, (long)J * H * H, (long)H * H, 1, B, J, H, H, gp, nullptr, ms));
    TRY(pa_launch_fill(norm, (float)H / 10.f, B, ms));
    TRY(pa_launch_pck(pp, gp, norm, 1.f, idxs, nidx, 0.5f, nullptr, B, J, acc, nullptr, nullptr, ms));
    return n.meter_done(ms);
}

// pa_net_meters_async (include/poseadv.h): on != 0 -- pa_hg_accuracy / pa_hg_pckh calls are launched on the engine's meter stream, behind
// everything the main stream holds at the call and beside whatever it is given next; the main stream joins them at the end of the next
// pa_hg_backward / the last pa_hg_backward_phase (or in front of the next forward pass).  Until then their outputs and scratch buffers
// must stay allocated and unread.
int pa_net_meters_async(pa_net* net, int on) { g_err[0] = 0; net->n.meters_async = on != 0; return 0; }


// Evaluation.accuracy_origin_res (pylib/Evaluation.py:77-97) and per_person_pckh (:99-167) of stack i's
// heat maps, straight from the engine's NHWC fp32 maps (no layout copy, no host sync)
int pa_hg_pckh(pa_net* net, int stack, const float* center, const float* scale, const float* rot, const float* gt_pts,
               const float* norm, const int32_t* idxs, int nidx, float* acc, float* person, float* scratch) {
    g_err[0] = 0;
    Net& n = net->n;
    const int H = n.res / 4, J = 16, B = n.B;
    const float* pp = nullptr;                    // [B][16][2] arg-max (computed once per forward, shared with pa_hg_accuracy)
    hipStream_t ms;
    TRY(n.meter_stream(&ms));
    TRY(n.heat_argmax(stack, &pp, ms));
    float* fp = scratch + (size_t)B * J * 2;      // [B][16][2] back-projected predictions
    float* vis = fp + (size_t)B * J * 2;          // [B][16][2] arg-max of the augmented target
    float* tgt = vis + (size_t)B * J * 2;         // [B][16][H][H] (only when person != NULL)
    TRY(pa_launch_final_preds(n.heat[stack], (long)H * H * 16, 1, 16, pp, center, scale, rot, B, J, H, H, fp, ms));
    if (person) {
        TRY(pa_launch_gaussian_heatmap(n.pts_dev, tgt, B, J, H, H, ms));
        TRY(pa_launch_argmax(tgt, (long)J * H * H, (long)H * H, 1, B, J, H, H, vis, nullptr, ms));
    }
    TRY(pa_launch_pck(fp, gt_pts, norm, 0.f, idxs, nidx, 0.5f, person ? vis : nullptr, B, J, acc, person, nullptr, ms));
    return n.meter_done(ms);
}

// per-launch HIP-event timing of the MFMA kernels (bench.py roofline): enable, run steps, then report.
int pa_net_profile_begin(pa_net* net) { net->n.prof.used = 0; net->n.prof.on = true; return 0; }
// out[cap_classes][4] = {total ms, launches, algorithmic bytes, flops} per class (include/poseadv.h).  Reporting synchronises and disables.
int pa_net_profile_report(pa_net* net, double* out, int cap_classes, int* n_classes) {
    net->n.prof.on = false;
    double full[PA_PROF_NCLS * 4];
    int r = net->n.prof.report(full);
    if (r) { pa_set_error("profile report", (hipError_t)r, __FILE__, __LINE__); return r; }
    for (int c = 0; c < PA_PROF_NCLS && c < cap_classes; ++c)
        for (int j = 0; j < 4; ++j) out[c * 4 + j] = full[c * 4 + j];
    if (n_classes) *n_classes = PA_PROF_NCLS;
    return 0;
}
int pa_net_set_fin_prologue(pa_net* net, int max_rows) {
    net->n.fin_rows_max = max_rows < 0 ? 0 : (max_rows > PA_FIN_SMALL_ROWS ? PA_FIN_SMALL_ROWS : max_rows);
    net->n.release_graph();
    return 0;
}
int pa_net_set_pool_route(pa_net* net, int on) {
    net->n.pool_route = on ? 3 : 0;
    net->n.release_graph();
    return 0;
}
int pa_net_design_bytes(const pa_net* net, double* out) { out[0] = net->n.dbytes_rd; out[1] = net->n.dbytes_wr; return 0; }

int pa_net_profile_classes(const pa_net* net, int32_t* out, int cap) {
    const std::vector<int>& q = net->n.prof.last_seq;
    for (int i = 0; i < cap && i < (int)q.size(); ++i) out[i] = q[i];
    return (int)q.size();
}

int pa_net_set_multi_stream(pa_net* net, int on) {
    if (net->n.ensure_streams()) return 1;
    net->n.release_graph();
    net->n.multi_stream = on != 0 && net->n.side != nullptr;
    return 0;
}

// the views of an activation the debug hooks copy out (include/poseadv.h): 0 value (pending BatchNorm+ReLU applied), 1 stored gradient
// (dz = masked gradient with a pending BatchNorm, the plain gradient otherwise), 2 raw stored tensor, 3 gradient with respect to the raw
// tensor (kA * dz + kB * raw + kC with a pending BatchNorm: Net::gradop), 4 that gradient as the data-gradient kernel of its consumer
// stored it for the later readers (Residual::dz3 / dz2; `mat` = nullptr when this step did not materialise it)
static int debug_copy(Net& n, const Act& a, int grad, float* out, int* shape4, const char* who, const bf16* mat) {
    if (grad < 0 || grad > 4) { pa_set_error_msg((std::string(who) + ": grad must be 0 .. 4").c_str()); return 1; }
    if ((grad == 1 || grad == 3) && !a.grad) { pa_set_error_msg((std::string(who) + ": this tensor has no gradient buffer").c_str()); return 1; }
    if (grad == 4 && !mat) { pa_set_error_msg((std::string(who) + ": no stored BatchNorm-backward gradient of this tensor in this step").c_str()); return 1; }
    shape4[0] = a.B; shape4[1] = a.C; shape4[2] = a.H; shape4[3] = a.W;
    if (!out) return 0;
    const PaOperand src = grad == 0 ? n.op(a) : grad == 1 ? pa_plain(a.grad) : grad == 2 ? pa_plain(a.raw) : grad == 3 ? n.gradop(a) : pa_plain(mat);
    TRY(pa_launch_nhwc_bf16_to_nchw_f32(src, out, a.B, a.C, a.H, a.W, n.st));
    return 0;
}

// debug / test hook: copy an internal activation (BatchNorm+ReLU applied) or its gradient buffer out as
// NCHW fp32.  which: "stem", "res1", "pool0", "res2", "res3", "hg<i>.skip<k>", "hg<i>.pool<k>",
// "hg<i>.down<k>", "hg<i>.neck", "hg<i>.up<k>", "hg<i>.merge<k>", "post<i>", "lin<i>", "xin<i>" (k = 1..4)
// and "<name>.x1"/".x2" for the inner tensors of a residual block; the names of the sites of num_modules blocks (skip / down / neck / up /
// post) mean the site's output, i.e. its last block, and "<site>.m<j>" names block j ("hg0.up3.m0", "post1.m1.x2"); "hg<i>.maskedskip<k>", "hg<i>.maskedneck" (occlusion branch);
// "heat<i>": the heat maps in the storage type as in_conv reads them (64 channels, 16..63 zero), gradient: d heat as out_conv's
// weight gradient reads it; "heat<i>.in": in_conv's data gradient (its part of d heat); "forth<i>": forth_conv's output
// (forth_conv(lin) + xin), in_conv's addend; "hg<i>.poolgrad<k>": the gradient pool k routes back to its input (plus, k = 1, the
// gradient reaching the hourglass input from outside), the second addend of skip k's conv1 data gradient.
// grad: which view (debug_copy above).
int pa_hg_debug_tensor(pa_net* net, const char* which, int grad, float* out, int* shape4) {
    Net& n = net->n;
    std::string w(which);
    const Act* a = nullptr;
    const bf16* mat = nullptr;       // view 4: the block's stored dz2 / dz3
    auto pick_res = [&](Residual& r, const std::string& rest) -> const Act* {
        if (rest == ".x1") return &r.x1;
        if (rest == ".x2") { mat = r.dz2_valid ? r.dz2 : nullptr; return &r.x2; }
        mat = r.dz3_valid ? r.dz3 : nullptr;
        return &r.x3;
    };
    // a site of num_modules blocks: "<site>" is its output (the last block), "<site>.m<j>" block j; ".x1" / ".x2" come behind either
    bool bad_block = false;
    auto pick_chain = [&](Chain& c, std::string rest) -> const Act* {
        size_t j = c.m.size() - 1;
        if (rest.size() >= 3 && rest[0] == '.' && rest[1] == 'm' && rest[2] >= '0' && rest[2] <= '9') { j = (size_t)(rest[2] - '0'); rest = rest.substr(3); }
        if (j >= c.m.size()) { bad_block = true; return nullptr; }
        return pick_res(c.m[j], rest);
    };
    auto starts = [&](const char* p) { return w.rfind(p, 0) == 0; };
    Act head;                        // buffers that are no activation of their own: "heat<i>", "heat<i>.in", "forth<i>", "hg<i>.poolgrad<k>"
    head.B = n.B; head.H = head.W = n.res / 4;
    if (starts("heat")) {
        const bool in = w.size() == 8 && w.compare(5, 3, ".in") == 0;
        const int i = (w.size() == 5 || in) ? w[4] - '0' : -1;
        if (i >= 0 && i < (int)n.heat64.size() && n.heat64[i]) {
            if (in) { if (i < (int)n.forth_tmp.size() && n.forth_tmp[i]) { head.raw = n.dheat_in[i]; head.C = 64; a = &head; } }
            else { head.raw = n.heat64[i]; head.grad = n.dheat64[i]; head.C = 64; a = &head; }
        }
    } else if (starts("forth")) {
        const int i = w.size() == 6 ? w[5] - '0' : -1;
        if (i >= 0 && i < (int)n.forth_tmp.size() && n.forth_tmp[i]) { head.raw = n.forth_tmp[i]; head.C = n.chan; a = &head; }
    } else if (starts("stem")) a = &n.a0;
    else if (starts("res1")) {
        a = pick_res(n.res1, w.substr(4));
        // (a routed step never wrote residual1's gradient buffer: the pool backward launch runs now, same bits)
        if (out && a == &n.res1.x3 && (grad == 1 || grad == 3) && n.stem_routed) TRY(n.fill_stem_grad());
    }
    else if (starts("pool0")) a = &n.pool0;
    else if (starts("res2")) a = pick_res(n.res2, w.substr(4));
    else if (starts("res3")) a = pick_res(n.res3, w.substr(4));
    else if (starts("post")) { int i = w[4] - '0'; a = pick_chain(n.post[i], w.substr(5)); }
    else if (starts("lin")) { int i = w[3] - '0'; a = &n.lin_out[i]; }
    else if (starts("xin")) { int i = w[3] - '0'; a = &n.xin[i]; }
    else if (starts("hg")) {
        int i = w[2] - '0';
        std::string r = w.substr(4);
        Hourglass& h = n.hg[i];
        if (r.rfind("neck", 0) == 0) a = pick_chain(h.neck, r.substr(4));
        else if (r == "maskedneck") a = &h.neckm;                                  // occlusion branch: neck * cell mask
        else if (r.rfind("maskedskip", 0) == 0) a = &h.skipm[r[10] - '1'];
        else if (r.rfind("poolgrad", 0) == 0) {                                     // the pool's gradient routed to its input (+ extra0)
            const int k = r.size() == 9 ? r[8] - '1' : -1;
            if (k >= 0 && k < 4 && h.poolgrad[k]) {
                const Act& x = h.skip[k].out();
                // (a routed level never wrote the buffer: the pool backward launch runs now, from the still-resident gradient of the pooled
                // tensor, the pool's input and the addend)
                if (out && h.routed[k]) TRY(h.fill_poolgrad(n, k, n.xin[i]));
                head.raw = h.poolgrad[k]; head.B = x.B; head.H = x.H; head.W = x.W; head.C = x.C; a = &head;
            }
        } else {
            int k = r[r.find_first_of("1234")] - '1';
            std::string rest = r.substr(r.find_first_of("1234") + 1);
            if (r.rfind("skip", 0) == 0) a = pick_chain(h.skip[k], rest);
            else if (r.rfind("down", 0) == 0) a = pick_chain(h.down[k], rest);
            else if (r.rfind("up", 0) == 0) a = pick_chain(h.up[k], rest);
            else if (r.rfind("pool", 0) == 0) a = &h.pooled[k];
            else if (r.rfind("merge", 0) == 0) a = &h.merged[k];
        }
    }
    if (bad_block) { pa_set_error_msg("pa_hg_debug_tensor: no such block in the site's chain"); return 1; }
    if (!a) { pa_set_error_msg("pa_hg_debug_tensor: unknown tensor name"); return 1; }
    return debug_copy(n, *a, grad, out, shape4, "pa_hg_debug_tensor", mat);
}


// test hook for the agent, like pa_hg_debug_tensor: names "in<k>" (k=0..4: residual_skip1-4, residual_neck),
// "pa<k>", "merge<k>" (k=0..3), "deep<k>" (k=0..2), optional ".x1"/".x2"
int pa_asn_debug_tensor(pa_net* net, const char* which, int grad, float* out, int* shape4) {
    Net& n = net->n;
    std::string w(which);
    const Act* a = nullptr;
    const bf16* mat = nullptr;
    auto pick = [&](Residual& r, const std::string& rest) -> const Act* {
        if (rest == ".x1") return &r.x1;
        if (rest == ".x2") { mat = r.dz2_valid ? r.dz2 : nullptr; return &r.x2; }
        mat = r.dz3_valid ? r.dz3 : nullptr;
        return &r.x3;
    };
    auto starts = [&](const char* p) { return w.rfind(p, 0) == 0; };
    if (starts("in")) a = pick(n.asn_in[w[2] - '0'], w.substr(3));
    else if (starts("pa")) a = &n.asn_pa[w[2] - '0'];
    else if (starts("merge")) a = pick(n.asn_merge[w[5] - '0'], w.substr(6));
    else if (starts("deep")) a = pick(n.asn_deep[w[4] - '0'], w.substr(5));
    if (!a) { pa_set_error_msg("pa_asn_debug_tensor: unknown tensor name"); return 1; }
    return debug_copy(n, *a, grad, out, shape4, "pa_asn_debug_tensor", mat);
}

}  // extern "C"
