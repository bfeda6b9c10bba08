/* poseadv.h -- C ABI of libposeadv_hip.so: the MI355X (gfx950) hot path of the stacked-hourglass
 * pose trainer with adversarial scale/rotation augmentation.
 *
 * Conventions:
 *   - every function returns 0 on success, otherwise a hipError_t / library error code;
 *     pa_last_error() gives the message.  No C++ exception crosses the ABI.
 *   - all pointers are CALLER-OWNED DEVICE pointers unless the name ends in _host; the library
 *     never allocates persistent device memory: a network runs inside one caller-provided workspace
 *     whose size comes from pa_net_workspace_bytes() (cleared by pa_net_bind).
 *   - calls are asynchronous on the given hipStream_t (passed as void*); one host thread per net.
 *   - activations are NHWC bf16 inside the library; the entry points that mirror the reference's
 *     Python signatures take/return NCHW fp32 exactly like the reference's torch tensors.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference
 * checkout zhiqiangdon/pose-adv-aug).
 */
#ifndef POSEADV_H
#define POSEADV_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* pa_last_error(void);
int pa_version(void);
/* Which build this is: 0 = bfloat16 storage (libposeadv_hip.so), 1 = IEEE-half storage (libposeadv_hip_fp16.so: "fp16 MFMA
 * 1x1 convs" of the deep-stack configuration).  Same ABI; "bf16" in the comments below means this 16-bit type.
 * pa_grad_scale: the factor every fp32 gradient the library returns carries (1 for bf16; the fp16 build runs its backward pass
 * on scaled gradients so that they stay inside half's range): pass gscale = 1 / (world * pa_grad_scale()) to pa_rmsprop_step. */
int pa_dtype(void);
float pa_grad_scale(void);

/* ---------------------------------------------------------------- pose library (pylib/) ---- */

/* HumanPts.pts2heatmap (pylib/HumanPts.py:36-46) + draw_gaussian (:82-116), batched.
 * pts: [B][J][2] float64 (x, y) in heat-map pixels; out: [B][J][H][W] fp32, any H, W, J >= 1 (a joint is valid for 0 < x <= W, 0 < y <= H).
 * Errors (non-zero, pa_last_error set, nothing launched): pts or out NULL; B, J, H or W < 1. */
int pa_gaussian_heatmap(const double* pts, float* out, int B, int J, int H, int W, void* stream);

/* Criterion.weighted_L2 (pylib/Criterion.py:12-18); weight may be NULL (== 1), which is the inline
 * loss term of stack-hg.py:156-159.  *loss (fp32, device) is ACCUMULATED into: zero it first.  The partial sums of the workgroups are
 * added with atomics: two runs may differ in the last bits.
 * Errors (non-zero, pa_last_error set, nothing launched): pred, gt or loss NULL; n == 0. */
int pa_weighted_l2(const float* pred, const float* gt, const float* weight, size_t n, float* loss, void* stream);
/* d/dpred of pa_weighted_l2: dpred[e] = 2 * (weight ? weight[e] : 1) * (pred[e] - gt[e]) * (*gout_dev) / n ;
 * gout_dev: ONE device float (the gradient arriving at the loss; no host synchronisation).  dpred is overwritten; it may be pred
 * itself.  pred, gt, gout_dev or dpred == NULL is an error. */
int pa_weighted_l2_grad(const float* pred, const float* gt, const float* weight, size_t n, const float* gout_dev,
                        float* dpred, void* stream);

/* Evaluation.get_preds (pylib/Evaluation.py:6-23): maps [B][J][H][W] fp32 -> preds [B][J][2]
 * (1-based x, y; zero where the maximum is <= 0).  maxval [B][J] may be NULL. */
int pa_get_preds(const float* maps, int B, int J, int H, int W, float* preds, float* maxval, void* stream);

/* Evaluation.final_preds (pylib/Evaluation.py:169-193 + transform_preds :195-211 + TransformPts
 * :240-248): quarter-pixel refinement, +0.5, back-projection to original-image pixels (integer
 * valued).  center [B][2], scale [B], rot [B] fp32; out [B][J][2] fp32. */
int pa_final_preds(const float* maps, const float* center, const float* scale, const float* rot,
                   int B, int J, int H, int W, float* out, float* scratch_preds, void* stream);

/* The same two operations on joint-minor maps [B][H*W][J] fp32 -- the layout of the engine's own heat maps
 * (pa_hg_heatmap_nhwc), which pa_hg_accuracy / pa_hg_pckh read in place.  With J = 16 and a 16-byte-aligned `maps`
 * the arg-max is the one-workgroup-per-sample kernel those two use; any other J or alignment takes the generic
 * kernel with a stride of J floats between pixels. */
int pa_get_preds_nhwc(const float* maps, int B, int J, int H, int W, float* preds, float* maxval, void* stream);
int pa_final_preds_nhwc(const float* maps, const float* center, const float* scale, const float* rot,
                        int B, int J, int H, int W, float* out, float* scratch_preds, void* stream);

/* Soft-arg-max over heat maps (integral regression): the differentiable prediction beside the hard arg-max of pa_get_preds.  Per map
 * (b, j), with m its maximum, p the pixel index, x_p = p % W + 1 and y_p = p / W + 1 (1-based like pa_get_preds; the row is p / W):
 *   e_p = exp(beta (h_p - m)),  Z = sum e_p,  ex = sum x_p e_p / Z,  ey = sum y_p e_p / Z.
 * maps: fp32 on the device, finite; layout 0 = [B][J][H][W], 1 = [B][H*W][J] (pa_hg_set_heat_grads' numbers; 1 is what
 * pa_hg_heatmap_nhwc points at).  beta: the inverse temperature.  coords [B][J][2] fp32 = (float)ex, (float)ey; state [B][J][4] float64 =
 * m, Z, ex, ey unrounded (what the backward pass reads).  All arithmetic in double, no atomics, a fixed order of additions: the same
 * input gives the same bits.  J == 16 with layout 1 and a 16-byte-aligned maps takes 16-byte loads, one workgroup per sample and group of
 * four joints; everything else a strided kernel, one workgroup per map.  Enqueued on `stream`, no synchronisation; the same code in both
 * builds.
 * Errors (non-zero, pa_last_error set, nothing launched): a NULL pointer; B, J, H or W < 1; H * W >= 2^27 or B * J >= 2^31; a layout
 * other than 0 or 1; beta not finite or <= 0. */
int pa_soft_argmax(const float* maps, int layout, int B, int J, int H, int W, float beta, float* coords, double* state, void* stream);
/* Its backward pass: dmaps_p = (float)(beta e_p / Z ((x_p - ex) gx + (y_p - ey) gy)) with (gx, gy) = dcoords [B][J][2] fp32 (d loss /
 * d coords), e_p recomputed from maps and state (pa_soft_argmax's, same maps, layout and beta).  One pass: maps is read once and every
 * element of dmaps (fp32, the layout of maps: layout 1 goes straight into pa_hg_set_heat_grads) is written once.  dmaps must not be
 * maps.  The fast path additionally needs a 16-byte-aligned dmaps.
 * Errors: as above, and dmaps == maps. */
int pa_soft_argmax_bwd(const float* maps, int layout, int B, int J, int H, int W, float beta, const double* state, const float* dcoords,
                       float* dmaps, void* stream);
/* Calibration of the soft-arg-max error bound (tools/bench_soft_argmax.py): y[i] = the device's double exp(x[i]), the function the two
 * kernels above evaluate; x, y: n float64 on the device.  Errors: x or y NULL, n == 0. */
int pa_exp_probe(const double* x, double* y, size_t n, void* stream);

/* PCK from point sets: Evaluation.calc_dists/dist_acc/accuracy (pylib/Evaluation.py:25-75; boundary
 * 1), accuracy_origin_res (:77-97; boundary 0), per_person_pckh (:99-167; `person` output with the
 * visibility points `vis`), HumanAcc.approx_PCKh (pylib/HumanAcc.py:7-44; boundary 0, norm = res/10
 * with Python-2 integer division done by the caller).
 * pred, gt: [B][J][2]; norm: [B]; idxs: int32 [nidx] (device); acc: [nidx+1] or NULL;
 * person: [B] or NULL; vis: [B][J][2] or NULL; dists: [J][B] (calc_dists' matrix) or NULL. */
int pa_pck(const float* pred, const float* gt, const float* norm, float boundary, const int32_t* idxs, int nidx,
           float thr, const float* vis, int B, int J, float* acc, float* person, float* dists, void* stream);

/* HumanAug.GetTransform (pylib/HumanAug.py:10-35) for a batch: params [B][8] float64 =
 * {cx, cy, scale, rot_deg, flip, gain_r, gain_g, gain_b}; t_out [B][6] float64 = forward transform
 * at res_out (first two rows), tinv_in [B][6] = INVERSE transform at res_in (what the warp samples with).  Both outputs are required.
 * Errors (non-zero, pa_last_error set, nothing launched): params, t_out or tinv_in NULL; B, res_in or res_out < 1. */
int pa_affine_params(const double* params, int B, int res_in, int res_out, double* t_out, double* tinv_in, void* stream);
/* fp32 copies of c, s, r as the metric calls take them (`c = meta['center']`, `s = meta['scale']`, `r = meta['rot']` of the reference's
 * batches, stack-hg.py:140-143): csr [4 B] floats = c [B][2] | s [B] | r [B] from params [B][8]. */
int pa_params_csr(const double* params, int B, float* csr, void* stream);

/* HumanAug.TransformPts (pylib/HumanAug.py:45-54) + shufflelr (:236-257) + the invalid-joint rule of
 * data/mpii_for_mpii.py:142-146.  pts [B][J][2] fp32 image pixels -> out [B][J][2] float64 heat-map
 * coords (0 for invalid joints); pts_img (optional) = mirrored/swapped image-space joints.
 * A sample with flip != 0 has every joint mirrored (x <- width - x, in fp32).  The left / right partners are MPII's: with J == 16 a flipped
 * sample's joint j is read from its partner (0,5) (1,4) (2,3) (10,15) (11,14) (12,13); with any other J the joints are mirrored but NOT swapped
 * (there is no partner table for them).  A joint whose mirrored x or whose y is <= 0 gives exactly (0, 0).
 * Errors (non-zero, pa_last_error set, nothing launched): pts, params, t or out NULL (and sizes, for pa_transform_pts_sized); B or J < 1. */
int pa_transform_pts(const float* pts, const double* params, const double* t, int B, int J, float width,
                     double* out, float* pts_img, void* stream);

/* The PURE inverse-affine bilinear sampler (2 x 2 taps, no pre-filter): the geometry of HumanAug.crop
 * (pylib/HumanAug.py:117-176) + flip / colour gain of data/mpii_for_mpii.py:126-135 as one gather.  NOT the reference's
 * pixels (those are pa_crop below, which the training / validation paths use); kept as an operator.  src: uint8 [B][Hs][Ws][3]; out4: bf16 [B][res][res][4]
 * (network input layout, 4th channel +0; channels 0..2 are outf rounded to nearest even) and/or outf: fp32 [B][3][res][res]; either may
 * be NULL, not both.
 * Errors (non-zero, pa_last_error set, nothing launched): src, tinv or params NULL (and sizes, for pa_affine_warp_bilinear_sized); out4 and outf
 * both NULL; Hs, Ws, B or res < 1. */
int pa_affine_warp_bilinear(const uint8_t* src, int Hs, int Ws, const double* tinv, const double* params,
                            int B, int res, void* out4, float* outf, void* stream);
/* The same two calls for a batch of frames of DIFFERENT sizes stored top-left aligned in a padded [B][Hs][Ws][3] buffer
 * (real MPII images: data/mpii_for_mpii.py:97-135 loads one JPEG per person).  sizes: int32 [B][2] = width, height of
 * each sample's own frame: the zero padding outside it, the mirror of a flipped frame (x <- w_b - 1 - x) and the
 * mirror of its joints (x <- w_b - x, pylib/HumanAug.py:236-257) use the sample's own width. */
int pa_affine_warp_bilinear_sized(const uint8_t* src, int Hs, int Ws, const int32_t* sizes, const double* tinv,
                                  const double* params, int B, int res, void* out4, float* outf, void* stream);
int pa_transform_pts_sized(const float* pts, const double* params, const double* t, int B, int J, const int32_t* sizes,
                           double* out, float* pts_img, void* stream);

/* The backward pass of the bilinear sampler above: from dimg = d loss / d (its fp32 output) to the six coefficients of tinv, the colour
 * gains and the augmentation parameters.  With sx = ti0 u + ti1 v + ti2, sy = ti3 u + ti4 v + ti5, (ax, ay) their fractions,
 * S_c = sum of the 2 x 2 taps w_k p_k,c / 255 (as the forward read them: 0 outside the sample's frame, mirrored when flip), per pixel:
 *   m_c = 1 iff 0 <= gain_c S_c <= 1 (torch.clamp's rule on the double pre-clamp value; bounds included, so a pixel outside the frame
 *   passes and contributes exact zeros);  dS_c/dsx = (1 - ay)(p01 - p00) + ay (p11 - p10),  dS_c/dsy = (1 - ax)(p10 - p00) + ax (p11 - p01)
 *   (floor has derivative 0: at an integer sx this is the derivative of the cell the forward sampled, the right-hand one);
 *   gx = sum_c dimg_c m_c gain_c dS_c/dsx, gy likewise;  dtinv = sum over pixels {gx u, gx v, gx, gy u, gy v, gy};  dgain_c = sum dimg_c m_c S_c.
 * The float cast of the output and the rounding of out4 to the storage type are not differentiated.  dparams [B][8] = d loss /
 * d {cx, cy, scale, rot (per degree), flip (always 0), gain r, g, b} by the chain rule through pa_affine_params: it assumes that tinv
 * came from pa_affine_params(params, res_in = res); a caller with a tinv of its own takes dtinv.  cx is the centre after the mirror, as
 * everywhere in params.
 * dimg: fp32 on the device, 16-byte aligned, the two layouts pa_hg_set_image_grad writes: 0 [B][3][res][res], 1 [B][res][res][4] (the 4th
 * float is ignored); unscaled in both builds.  sizes: as for pa_affine_warp_bilinear_sized, or NULL (every frame fills [Hs][Ws]).
 * workspace: pa_affine_warp_bwd_workspace_bytes(B, res) bytes on the device (0: bad shape; host only, no device call), 8-byte aligned.
 * dtinv [B][6], dgain [B][3], dparams [B][8]: float64 on the device, each may be NULL but not all three; fully overwritten.
 * Everything in double, two launches (partial sums per strip of output rows stored, then added in a fixed order), no atomics: the same
 * input gives the same bits.  Enqueued on `stream`, no synchronisation.  The same code in both builds.
 * Errors (non-zero, pa_last_error set, nothing launched): a NULL src / tinv / params / dimg / workspace, all three outputs NULL, a layout
 * other than 0 or 1, a dimg that is not 16-byte aligned, a workspace that is not 8-byte aligned, B < 1, res < 1, Hs < 1, Ws < 1,
 * B * ceil(res / 8) above 2^31 - 1. */
size_t pa_affine_warp_bwd_workspace_bytes(int B, int res);
int pa_affine_warp_bilinear_bwd(const uint8_t* src, int Hs, int Ws, const int32_t* sizes, const double* tinv, const double* params,
                                int B, int res, const float* dimg, int layout, void* workspace, double* dtinv, double* dgain,
                                double* dparams, void* stream);
/* The chain rule alone, on the host (no device call): params_host [B][8], dtinv_host [B][6], dgain_host [B][3] or NULL (zeros) ->
 * dparams_host [B][8], with tinv = pa_affine_params(params, res_in).  The code the device's second launch runs. */
int pa_affine_params_bwd_host(const double* params_host, const double* dtinv_host, const double* dgain_host, int B, int res_in,
                              double* dparams_host);

/* HumanAug.crop (pylib/HumanAug.py:117-176) behind the dataset's pre-processing (data/mpii_for_mpii.py:114-135,
 * utils/imutils.py:31-40), stage for stage with the arithmetic of the libraries the reference delegates its pixels to
 * (scipy.misc.pilutil over Pillow): source bytes = fp32 frame / 255, mirrored, times gain, clamped; for
 * scale * 200 / res >= 2 the antialiased whole-frame pre-downscale (:121-133); the int-truncated, rotation-padded,
 * zero-filled window (:136-164); PIL's bilinear rotate about the window centre (:166-170); PIL's bilinear (triangle
 * filter) resize to res x res (:175); uint8 / 255.
 * What each entry point is exact against: scipy's toimage() maps every non-uint8 array from its own [min, max] to [0, 255]
 * (the whole fp32 frame in front of the pre-downscale, in fp32; the zero-padded window, in double).
 *   pa_crop          (the default) scales by the full range instead: byte-exact against the reference's crop over Pillow 12
 *                    only for crops whose window holds a pure black and a pure white pixel, and against the same pipeline
 *                    without the stretch (oracle/crop.py, quirk=False) for every crop.
 *   pa_crop_stretch  (opt-in) applies both stretches: byte-exact against the reference's crop over Pillow 12 for every crop
 *                    (oracle/crop.py, quirk=True).  Same arguments and outputs; its workspace is
 *                    pa_crop_stretch_workspace_bytes() bytes (larger; scratch, no initialisation needed).  It costs three more
 *                    launches and one more read of every pre-downscaled sample's frame.  A window wholly outside the frame,
 *                    where the reference raises, gives zeros from both.
 * src: uint8 [B][Hs][Ws][3]; sizes: int32 [B][2] = (width, height) of each sample's own frame inside the padded
 * buffer, or NULL (all Ws x Hs); params: [B][8] as for pa_affine_params (centre AFTER the mirror);
 * workspace: pa_crop_workspace_bytes() bytes (scratch, no initialisation needed);
 * out4: bf16 [B][res][res][4] network input, outf: fp32 [B][3][res][res], out8: uint8 [B][res][res][3]; any may be NULL. */
size_t pa_crop_workspace_bytes(int B, int Hs, int Ws, int res);
/* Upper bound of the bytes one pa_crop call reads (out[0]) and writes (out[1]), from the geometry of its own stage buffers at their
 * worst-case window sizes (bench.py's roofline.floor; the reference's crop, pylib/HumanAug.py:117-176, has no such notion). */
int pa_crop_design_bytes(int B, int Hs, int Ws, int res, double* out_host);
int pa_crop(const uint8_t* src, int Hs, int Ws, const int32_t* sizes, const double* params, int B, int res, void* workspace,
            void* out4, float* outf, uint8_t* out8, void* stream);
size_t pa_crop_stretch_workspace_bytes(int B, int Hs, int Ws, int res);
int pa_crop_stretch(const uint8_t* src, int Hs, int Ws, const int32_t* sizes, const double* params, int B, int res, void* workspace,
                    void* out4, float* outf, uint8_t* out8, void* stream);

/* JPEG decode split between host and device (the reference decodes on the host inside its DataLoader workers: utils/imutils.py:38-41
 * over data/mpii_for_mpii.py:97): the serial Huffman stage runs on the host, everything after the coefficients (dequantisation,
 * 8x8 inverse DCT, chroma upsampling, colour conversion, padding) on the device, byte-exact with libjpeg's integer pipeline
 * (jidctint / jdsample "fancy" / jdcolor) and therefore with Pillow's Image.open(f).convert('RGB').
 *
 * Supported files: SOF0 / SOF1 (8-bit, Huffman), ONE interleaved scan with all components (or the single component of a grayscale
 * file), chroma components 1x1 with luma 1x1, 2x1 or 2x2, and a colour space that libjpeg resolves to YCbCr or grayscale (a JFIF
 * marker; or Adobe transform 1; or neither marker and component ids that are not 'R','G','B').  Everything else that is a
 * well-formed JPEG -- progressive or arithmetic coding, 12-bit samples, several scans, CMYK / YCCK / RGB, other sampling factors,
 * a subsampled component narrower than 3 samples (libjpeg switches to its plain upsampler there) -- returns PA_JPEG_UNSUPPORTED;
 * corrupt or truncated input returns PA_JPEG_CORRUPT, a coefficient buffer that is too small PA_JPEG_CAPACITY, both with a message.
 *
 * The two *_host functions are pure host code (no HIP call, no global state, re-entrant from many threads, usable without a GPU).
 * pa_jpeg_info_host parses the markers up to SOS and fills the descriptor; pa_jpeg_entropy_host does the same parse and then
 * decodes the scan into coef_host (never reading past data_host + n, never writing past capacity_elems): per component the blocks
 * in raster order over its MCU-padded block grid (3 components: mcus_w * h x mcus_h * v blocks; 1 component: ceil(W/8) x ceil(H/8)),
 * 64 int16 per block in natural (row-major) order, NOT dequantised, DC prediction resolved. */
#define PA_JPEG_UNSUPPORTED 19024
#define PA_JPEG_CORRUPT 19025
#define PA_JPEG_CAPACITY 19026
typedef struct pa_jpeg_comp {
    int32_t h, v;              /* sampling factors (1x1 for a single-component file, whatever its header says) */
    int32_t bw, bh;            /* block grid of the coefficient plane */
    int64_t offset;            /* of the plane inside the image's coefficients, in int16 elements */
} pa_jpeg_comp;
typedef struct pa_jpeg_desc {
    int32_t width, height;
    int32_t ncomp;             /* 1 or 3; 0 = "not decoded here" for pa_jpeg_decode */
    int32_t restart_interval;  /* in MCUs, 0 = none */
    int64_t total_elems;       /* int16 elements of all planes */
    pa_jpeg_comp comp[3];
    uint16_t quant[3][64];     /* per COMPONENT, natural order */
} pa_jpeg_desc;
int pa_jpeg_info_host(const uint8_t* data_host, size_t n, pa_jpeg_desc* desc_host);
int pa_jpeg_entropy_host(const uint8_t* data_host, size_t n, int16_t* coef_host, size_t capacity_elems, pa_jpeg_desc* desc_host);
/* The device half for a batch: coef (int16), descs [B], coef_base int64 [B] (image b's offset into coef, a multiple of 8 elements)
 * are DEVICE pointers; frames: uint8 [B][Hs][Ws][3] top-left aligned, zero outside each image, sizes: int32 [B][2] = (w, h) --
 * what pa_crop consumes.  An entry with ncomp == 0 (and any entry whose descriptor is not one the host functions produce, or does not
 * fit Hs x Ws) gets an all-zero frame and its sizes row is left untouched: the caller fills both in.  Two launches: (a) dequantise +
 * inverse DCT + range limit into uint8 component planes inside `workspace` (pa_jpeg_workspace_bytes() bytes, no initialisation
 * needed), (b) upsampling + colour conversion + padding into frames. */
size_t pa_jpeg_workspace_bytes(int B, int Hs, int Ws);
int pa_jpeg_decode(const int16_t* coef, const pa_jpeg_desc* descs, const int64_t* coef_base, int B, int Hs, int Ws, void* workspace,
                   uint8_t* frames, int32_t* sizes, void* stream);

/* Validation with flip test-time augmentation (stack-hg.py:222-230).
 * pa_flip_lr_nhwc4: mirror the bf16 NHWC4 network input along W (img.numpy()[:, :, :, ::-1], :223).
 * pa_flip_tta_merge: merged = (out + shuffle_channels_for_horizontal_flipping(flip_channels(out_flipped))) / 2
 * (pylib/HumanAug.py:198-210, :179-196, stack-hg.py:228-230) over NCHW fp32 heat maps [B][16][H][W].
 * Errors (non-zero, pa_last_error set, nothing launched): a NULL pointer; B, H or W < 1; for pa_flip_tta_merge J != 16. */
int pa_flip_lr_nhwc4(const void* src, void* dst, int B, int H, int W, void* stream);
int pa_flip_tta_merge(const float* out, const float* out_flipped, float* merged, int B, int J, int H, int W, void* stream);

/* augmentation laws: mode 0 = data/mpii_for_mpii.py:119-135 (regular), 1 = agent bins
 * (data/joint_train_s_r_agent.py:15-16,33-36,134-139), 2 = agent scale only, 3 = agent rotation only.
 * meta [B][4] = {objpos_x, objpos_y, scale, frame_width}; params [B][8] as above. */
int pa_sample_aug(const float* meta, const int32_t* scale_idx, const int32_t* rot_idx, int mode,
                  uint64_t seed, uint64_t step, int B, double* params, void* stream);
/* the same laws with CALLER-GIVEN draws instead of the engine's counter-based stream: draws [B][7] float64 =
 * {N(0,1) scale, N(0,1) rotation, U "rotation forced to 0", U flip, U gain_r, U gain_g, U gain_b} -- with the draws of
 * np.random in the reference's call order the result equals the reference's parameters value for value. */
int pa_sample_aug_given(const float* meta, const int32_t* scale_idx, const int32_t* rot_idx, int mode,
                        const double* draws, int B, double* params, void* stream);

/* softmax + np.random.choice(K, p) of joint-train-pose-s-r-agent.py:252-271.  logits [B][K], B >= 1, 1 <= K <= 64;
 * probs [B][K] and idx int32 [B] may be NULL.  Row b draws the uniform u of the engine's stream at (seed, step, b, slot),
 * slot <= 255 (the key holds the slot in 8 bits: a larger one would be a draw of another sample).  The pick is the inverse CDF
 * as np.random.choice normalises it: the first k whose float64 running sum of the fp32 probs exceeds u * (their float64 sum),
 * else the last k of positive probability -- never a class of probability 0. */
int pa_sample_categorical(const float* logits, int B, int K, uint64_t seed, uint64_t step, unsigned slot,
                          float* probs, int32_t* idx, void* stream);

/* _Hourglass._sample_mask (models/asn_stacked_hg.py:102-136): softmax over the `cells` (= 16) mask logits of each sample,
 * `dropout_num` (= 2) distinct cells drawn with those probabilities (the law of np.random.choice(replace=False)),
 * masks [B][cells] fp32 = 1 except 0 at the drawn cells, indexes int32 [B][dropout_num] (may be NULL), probs [B][cells]
 * (may be NULL).  uniforms: NULL = the engine's counter-based stream (seed, step); else float64 [B][dropout_num] in (0,1). */
int pa_sample_dropout_masks(const float* logits, int B, int cells, int dropout_num, uint64_t seed, uint64_t step,
                            const double* uniforms, float* probs, float* masks, int32_t* indexes, void* stream);
/* _Hourglass._dropout (models/asn_stacked_hg.py:79-100) on one NHWC bf16 tensor [B][H][W][C]: the [B][16] 4x4 cell mask,
 * nearest-upsampled to H x W (H, W multiples of 4), times every channel. */
int pa_cell_mask(const void* x_bf16, const float* masks, void* out_bf16, int B, int H, int W, int C, void* stream);

/* torch.optim.RMSprop(alpha, eps, momentum=0) step (stack-hg.py:51-52) on flat fp32 arrays;
 * gscale multiplies the gradient first (1/world after a sum all-reduce). */
int pa_rmsprop_step(float* param, const float* grad, float* square_avg, size_t n, float lr, float alpha,
                    float eps, float gscale, void* stream);
/* Half-precision build (pa_dtype() == 1) only: a step whose gradient holds inf / NaN (an fp16 overflow in the scaled backward
 * pass) is SKIPPED -- parameters and square_avg untouched, the loss-scaling convention the reference's fp32 path never needs --
 * and counted.  *count = steps skipped so far in this process (synchronises `stream`); always 0 in the bf16 build. */
int pa_rmsprop_skipped_steps(long long* count, void* stream);
/* The same two calls with the skip state owned by the OPTIMIZER instead of the process: `state` = two int32 on the device
 * ({this gradient is non-finite, steps skipped so far}), zeroed once by the caller.  Two optimizers that step on different streams
 * (pose net and agent, joint-train-pose-s-r-agent.py:86-94) each pass their own pair; pa_rmsprop_step shares one pair per process. */
int pa_rmsprop_step_state(float* param, const float* grad, float* square_avg, size_t n, float lr, float alpha,
                          float eps, float gscale, int32_t* state, void* stream);
int pa_rmsprop_skipped_steps_state(const int32_t* state, long long* count, void* stream);

/* The other options of torch.optim.RMSprop (momentum, weight_decay, centered) and the coefficient of
 * torch.nn.utils.clip_grad_norm_.  The reference trains with all of them off (stack-hg.py:51-52): these calls have no reference
 * counterpart beyond torch's option set.  Per element, in fp32 (torch 2.10 _single_tensor_rmsprop):
 *   gr = (grad * gscale) * clip_coef[0] + weight_decay * param;  v = alpha v + (1 - alpha) gr^2;  ga = alpha ga + (1 - alpha) gr;
 *   den = sqrt(centered ? max(0, v - ga^2) : v) + eps;  momentum > 0: buf = momentum buf + gr / den, param -= lr buf;
 *   else param -= lr gr / den.
 * max(0, .) is the one difference from torch, which returns NaN where rounding makes v - ga^2 slightly negative.
 * momentum_buf: n floats, required iff momentum > 0; grad_avg: n floats, required iff centered; clip_coef: one device float
 * (out2 + 1 of the norm call below) or NULL; state: two device int32 as for pa_rmsprop_step_state (required).  With momentum 0,
 * weight_decay 0, centered 0 and clip_coef NULL the call is pa_rmsprop_step_state, bit for bit.  Half-precision build: a step whose
 * gradient holds inf / NaN leaves param, square_avg, momentum_buf and grad_avg untouched and counts once in state.
 * Errors (non-zero, pa_last_error set, nothing launched): a NULL opts / param / grad / square_avg / state, a missing or superfluous
 * momentum_buf / grad_avg, momentum < 0, weight_decay < 0. */
typedef struct pa_rmsprop_opts { float lr, alpha, eps, momentum, weight_decay; int32_t centered; } pa_rmsprop_opts;
int pa_rmsprop_step_opts(const pa_rmsprop_opts* o, float* param, const float* grad, float* square_avg, float* momentum_buf,
                         float* grad_avg, size_t n, float gscale, const float* clip_coef, int32_t* state, void* stream);
/* out2 (device) = {norm of gscale * grad, min(1, max_norm / (norm + 1e-6))}: squares summed in double, two launches, no atomics (the
 * same input gives the same bits), no host synchronisation.  workspace: pa_grad_norm_workspace_bytes(n) bytes on the device, 8-byte
 * aligned.  Errors: a NULL grad / workspace / out2, max_norm <= 0. */
size_t pa_grad_norm_workspace_bytes(size_t n);
int pa_grad_norm(const float* grad, size_t n, float gscale, float max_norm, void* workspace, float* out2, void* stream);

/* torch.optim.Adam / AdamW (with AMSGrad) as one fused step on flat fp32 arrays.  The reference trains with RMSprop only: these calls have
 * no reference counterpart beyond torch's option set.  Per element, in fp32 and in this order (torch 2.10 _single_tensor_adam,
 * non-capturable branch):
 *   gr = (grad * gscale) * clip_coef[0];   coupled decay (decoupled 0, weight_decay != 0): gr += weight_decay * param;
 *   decoupled decay (decoupled 1, weight_decay != 0): param *= (float)(1.0 - (double)lr * (double)weight_decay);
 *   m = m + (gr - m) * (1.f - beta1);  v = beta2 v + ((1.f - beta2) gr) gr;  vmax = max(vmax, v) (amsgrad);
 *   den = sqrtf(amsgrad ? vmax : v) / bc2s + eps;  param -= step_size * (m / den)
 * with bc1 = (float)(1.0 - pow((double)beta1, (double)t)), bc2 likewise, bc2s = sqrtf(bc2), step_size = lr / bc1, t = the number of
 * steps TAKEN including this one.  t lives on the device, in `state`, because the half-precision build decides on the device whether
 * a step is taken (a gradient that holds inf / NaN: the step is skipped, every array untouched): a host counter would drift from the
 * moments after the first skipped step.
 * state: 32 bytes on the device, 16-byte aligned, zeroed once by the caller and owned by ONE optimizer.  flag / skipped are the pair
 * of pa_rmsprop_step_state (pa_rmsprop_skipped_steps_state may be pointed at it); step = steps taken so far; bc1, bc2, step_size,
 * bc2s = the constants the last TAKEN step used.  A one-thread launch in front of the step advances `step` and writes the constants,
 * or, with the flag set, counts a skipped step and leaves them.
 * exp_avg, exp_avg_sq: n floats; max_exp_avg_sq: n floats, required iff amsgrad; clip_coef: one device float (out2 + 1 of
 * pa_grad_norm) or NULL.
 * Errors (non-zero, pa_last_error set, nothing launched): a NULL opts / param / grad / exp_avg / exp_avg_sq / state, a missing or
 * superfluous max_exp_avg_sq, beta1 or beta2 outside [0, 1), eps <= 0, weight_decay < 0, a state that is not 16-byte aligned. */
typedef struct pa_adam_opts  { float lr, beta1, beta2, eps, weight_decay; int32_t amsgrad, decoupled; } pa_adam_opts;
typedef struct pa_adam_state { int32_t flag, skipped, step, reserved; float bc1, bc2, step_size, bc2s; } pa_adam_state;
int pa_adam_step(const pa_adam_opts* o, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                 float* max_exp_avg_sq, size_t n, float gscale, const float* clip_coef, pa_adam_state* state, void* stream);
/* *steps = steps taken, *skipped = steps skipped so far (either may be NULL); synchronises `stream`.  Errors: a NULL or misaligned state. */
int pa_adam_steps(const pa_adam_state* state, long long* steps, long long* skipped, void* stream);
/* state->step = steps, on `stream` (load_state_dict); the other words stay.  Errors: a NULL or misaligned state, steps < 0 or > INT32_MAX. */
int pa_adam_set_steps(pa_adam_state* state, long long steps, void* stream);

/* Parameter groups: one lr, one weight_decay and a frozen bit per GROUP of tensors, inside the fused steps and the norm above
 * (torch.optim's param_groups; the reference trains with one group, stack-hg.py:51-52, so these calls have no reference counterpart).
 * Every tensor of a flat parameter array starts on a 16-byte boundary, so a group is a property of a 16-byte CHUNK: chunk_map, a device
 * array of pa_opt_chunk_map_bytes(n) = ceil(n / 4) bytes owned by the caller, holds the group id (0 .. ngroups - 1) of chunk i / 4;
 * the last, partial chunk (n % 4 elements) is chunk n / 4.  groups_host: ngroups entries on the HOST, read during the call (they
 * travel in the kernel arguments: nothing is uploaded and the array may change after the call returns).
 * o->lr and o->weight_decay are IGNORED by the _groups calls: the groups carry them.  Every other option is the optimizer's, shared
 * by all groups.  Per element the formula, the order of operations and the fp32 types are those of pa_rmsprop_step_opts /
 * pa_adam_step with the chunk's group supplying lr and weight_decay (Adam: step_size_k = lr_k / bc1 and
 * c_dec_k = (float)(1.0 - (double)lr_k * (double)wd_k) too).  A group with weight_decay == 0 executes NO decay operation; otherwise
 * the decay is coupled or decoupled as the optimizer says.  A FROZEN chunk is skipped entirely: nothing is loaded from or stored to
 * param or any state array, and grad is not read there (inf / NaN in it are harmless in the bf16 build).  Zero padding stays zero.
 * pa_opt_chunk_map_host (host only, no device call): tensor t covers floats [offsets[t], offsets[t] + numels[t]); offsets are multiples
 * of 4, ascending, non-overlapping.  Every chunk a tensor touches gets group_host[t]; a chunk no tensor touches gets the group of the
 * tensor in front of it (group 0 in front of the first).  map_host: pa_opt_chunk_map_bytes(n) bytes; the caller uploads it.
 * pa_adam_step_groups: the one-thread launch in front of the step behaves as pa_adam_step's and also writes group_consts[k] =
 * lr_k / bc1 for k < ngroups (group_consts: PA_OPT_GROUPS_MAX floats on the device, owned by the caller, read by the step kernel) and
 * state->step_size = group_consts[0]; a skipped step leaves both as they were.
 * pa_grad_norm_groups: pa_grad_norm over the chunks whose group is not in the 16-bit mask excluded_groups (bit k = group k; the frozen
 * groups: clip_grad_norm_ over the trainable parameters).  The grid, the order of additions and the second launch are pa_grad_norm's,
 * so out2 equals, bit for bit, pa_grad_norm's on a copy of grad with the excluded chunks set to +0.
 * One group that is not frozen: chunk_map and group_consts may be NULL, and the call IS pa_rmsprop_step_opts / pa_adam_step with that
 * group's lr and weight_decay (the same launches, the same bits; a non-NULL group_consts[0] is still written).  excluded_groups == 0:
 * pa_grad_norm, chunk_map may be NULL.
 * Nothing is synchronised with the host; no atomics, the same input gives the same bits.
 * Half-precision build: the finite scan in front of the step reads the WHOLE gradient, frozen chunks included: an overflow anywhere in
 * the scaled backward pass has already propagated into the layers below it, and the scan is the only evidence of that.  One
 * non-finite value anywhere skips the whole step (every array, step and group_consts untouched) and counts once.
 * Errors (non-zero, pa_last_error set with the function's name in front, nothing launched): every error of the ungrouped call (without
 * those on o->weight_decay); a NULL groups_host; ngroups outside 1 .. 16; a NULL chunk_map with ngroups > 1 or a frozen group (norm:
 * with excluded_groups != 0); a NULL group_consts with ngroups > 1 or a frozen group; an lr or weight_decay that is negative or not
 * finite; excluded_groups with bits at or above 16.  Map builder: a NULL pointer, ntensors < 1, ngroups outside 1 .. 16, an offset that
 * is not a multiple of 4, tensors out of order or overlapping, a tensor that ends past n, a group id outside 0 .. ngroups - 1. */
#define PA_OPT_GROUPS_MAX 16
typedef struct pa_opt_group { float lr, weight_decay; int32_t frozen, reserved; } pa_opt_group;
size_t pa_opt_chunk_map_bytes(size_t n);
int pa_opt_chunk_map_host(const size_t* offsets_host, const size_t* numels_host, const int32_t* group_host, int ntensors,
                          size_t n, int ngroups, uint8_t* map_host);
int pa_rmsprop_step_groups(const pa_rmsprop_opts* o, const pa_opt_group* groups_host, int ngroups, const uint8_t* chunk_map,
                           float* param, const float* grad, float* square_avg, float* momentum_buf, float* grad_avg, size_t n,
                           float gscale, const float* clip_coef, int32_t* state, void* stream);
int pa_adam_step_groups(const pa_adam_opts* o, const pa_opt_group* groups_host, int ngroups, const uint8_t* chunk_map,
                        float* group_consts, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                        float* max_exp_avg_sq, size_t n, float gscale, const float* clip_coef, pa_adam_state* state, void* stream);
int pa_grad_norm_groups(const float* grad, size_t n, const uint8_t* chunk_map, uint32_t excluded_groups, float gscale,
                        float max_norm, void* workspace, float* out2, void* stream);

/* Layer-wise trust ratios: LAMB (You et al. 2020) on Adam's moments, LARS (You, Gitman, Ginsburg 2017) on SGD with momentum, plain SGD
 * (torch.optim.SGD), and per-tensor norms for logging.  The reference trains with RMSprop only: these calls have no reference counterpart.
 * All of them work on a SEGMENT list instead of a chunk map: a per-tensor norm needs to know the tensor, and a net has more tensors
 * than a byte holds.
 *
 * pa_opt_segments_host (host only, no device call).  Tensor t covers floats [offsets[t], offsets[t] + numels[t]); offsets are multiples
 * of 4, ascending, non-overlapping; the gaps are zero padding.  The array is cut at every tensor start and then every
 * PA_OPT_SEGMENT_FLOATS floats inside a tensor: segments are ascending, lie inside ONE tensor, cover no padding, a tensor's segments
 * are contiguous in the list, and only a tensor's last segment may have nfloats % 4 != 0.  chunk0 = first float / 4; group =
 * group_host[t] (0 .. 15).  An empty tensor has no segment.  Returns the number of segments; segs_host == NULL: count only; otherwise cap
 * is the room in segs_host (in segments).  Returns 0 with pa_last_error set, and writes nothing, on: a NULL offsets / numels / group,
 * ntensors < 1, an offset that is not a multiple of 4, tensors out of order or overlapping, a tensor that ends past n, a group id outside
 * 0 .. 15, cap too small, an array past 2^34 floats.  The caller uploads the list (16-byte aligned) and owns it.
 *
 * Work and sums.  One wave works on one segment, four segments per 256-thread workgroup.  A per-tensor sum of squares is formed in
 * double without atomics: one partial per segment (lanes add their elements in element order, then a fixed butterfly over the 64
 * lanes), and a second launch adds a tensor's partials in segment order.  The order depends only on the tensor's length: the same input
 * gives the same bits, and the same tensor gives the same norm wherever it lies.  workspace: pa_opt_layer_workspace_bytes(nsegs,
 * ntensors) bytes on the device, 8-byte aligned (two doubles per segment).  Every value is stored by ordinary vector stores.
 *
 * pa_tensor_norms: norms[t] = (float)sqrt(sum over tensor t of ((double)x[i] * (double)scale)^2), ntensors floats on the device; the entry
 * of an empty tensor is not written.  Two launches (sums, finish).  Errors: a NULL x / segs / workspace / norms, nsegs == 0,
 * ntensors < 1, a misaligned x / segs / workspace, a scale that is not finite.
 *
 * Groups.  groups_host: 1 .. 16 entries {lr, weight_decay, frozen} on the HOST as for the _groups calls above; a segment's group field
 * selects the entry; one group is group 0 everywhere (there is no ungrouped path).  A FROZEN segment is skipped before any load: nothing
 * of param, grad or a state array is read or written there, it adds to no norm, and its tensor's norms and trust ratio stay as they were.
 * Padding is covered by no segment and is never touched.  adapt_t = always_adapt || weight_decay of the tensor's group != 0 (the default
 * of apex FusedLAMB and timm: tensors without decay are not adapted).
 * norms: 2 * ntensors floats on the device, norms[t] = W_t = (float)sqrt(sum p^2) of the parameters BEFORE the step and
 * norms[ntensors + t] = U_t (LAMB) or G_t (LARS); trust: ntensors floats, r_t, to be set to 1 once by the caller.  clip_coef: one device
 * float (out2 + 1 of pa_grad_norm) or NULL.
 *
 * pa_lamb_step, per element in fp32 and in this order:
 *   gr = (grad * gscale) * clip_coef[0]                        (no multiply without a clip pointer)
 *   m' = m + (gr - m) * (1.f - beta1);   v' = beta2 * v + ((1.f - beta2) * gr) * gr
 *   den = sqrtf(v') / bc2s + eps;   u = (m' / bc1) / den;   weight_decay of the group != 0:  u = u + weight_decay * param
 *   per tensor: W = sqrt(sum param^2), U = sqrt(sum u^2), squares and sums in double;
 *   r_t = (adapt_t && W > 0 && U > 0) ? W / U : 1;  max_trust > 0: r_t = min(r_t, max_trust)     (double, rounded once to float)
 *   param' = param - (lr_group * r_t) * u
 * state, bc1, bc2s and the step count t: pa_adam_step's pa_adam_state and its one-thread launch in front (step_size = lr of group 0 / bc1
 * is written and not used).  Launches: prologue; pass 1 (m', v' and the per-segment sums of param^2 and u^2); finish (norms, trust);
 * pass 2 (the step, u recomputed from m', v' and param: 10 floats moved per element, no scratch array).
 * Errors (non-zero, pa_last_error set with the function's name in front, nothing launched): a NULL opts / param / grad / exp_avg /
 * exp_avg_sq / state / segs / workspace / norms / trust / groups_host; a state or an array that is not 16-byte aligned; amsgrad != 0;
 * beta1 or beta2 outside [0, 1); eps <= 0 or not finite; max_trust negative or not finite; an lr or weight_decay that is negative or not
 * finite; ngroups outside 1 .. 16; ntensors < 1; nsegs == 0 with n > 0.
 *
 * pa_lars_step, per element in fp32 and in this order:
 *   gr = (grad * gscale) * clip_coef[0]
 *   per tensor: W = sqrt(sum param^2), G = sqrt(sum gr^2), gr formed and squared in double as pa_grad_norm does;
 *   r_t = (trust_coef > 0 && adapt_t && W > 0 && G > 0) ? trust_coef * W / (G + weight_decay * W + lars_eps) : 1     (double, rounded once)
 *   d = gr;  weight_decay != 0: d = gr + weight_decay * param;  trust_coef > 0: d = r_t * d
 *   momentum != 0:  buf' = momentum * buf + d;  d = nesterov ? d + momentum * buf' : buf'
 *   param' = param - lr_group * d
 * trust_coef == 0 is torch.optim.SGD(momentum, weight_decay, nesterov, dampening = 0) from a zero momentum buffer: ONE step launch, no
 * norm launch; workspace, norms and trust may then be NULL.  Otherwise: sums, finish, step.  state: the two device int32 of
 * pa_rmsprop_step_state.  momentum_buf: n floats, required iff momentum != 0.
 * Errors: a NULL opts / param / grad / state / segs / groups_host, with trust_coef > 0 a NULL workspace / norms / trust; a missing or
 * superfluous momentum_buf; nesterov with momentum == 0; a momentum, trust_coef, lars_eps, lr or weight_decay that is negative or not
 * finite; an array that is not 16-byte aligned; ngroups outside 1 .. 16; ntensors < 1; nsegs == 0 with n > 0.
 *
 * Half-precision build: the reset + finite scan of the WHOLE gradient (n floats, frozen segments and padding included) runs in front.
 * With the flag set every later launch returns at once: param, every state array, the step count and its constants, norms and trust
 * stay bit for bit, and the skip is counted once (pa_adam_steps / pa_rmsprop_skipped_steps_state read it).
 * segs must be the list pa_opt_segments_host made for arrays of n floats: the kernels trust it.  n == 0: nothing is launched. */
#define PA_OPT_SEGMENT_FLOATS 1024
typedef struct pa_opt_segment { uint32_t chunk0, nfloats; int32_t tensor, group; } pa_opt_segment;   /* chunk0 = first float / 4 */
typedef struct pa_lamb_opts { float beta1, beta2, eps, max_trust; int32_t always_adapt, amsgrad; } pa_lamb_opts;
typedef struct pa_lars_opts { float momentum, trust_coef, lars_eps; int32_t nesterov, always_adapt; } pa_lars_opts;
size_t pa_opt_segments_host(const size_t* offsets_host, const size_t* numels_host, const int32_t* group_host, int ntensors, size_t n,
                            pa_opt_segment* segs_host, size_t cap);
size_t pa_opt_layer_workspace_bytes(size_t nsegs, int ntensors);
int pa_tensor_norms(const float* x, const pa_opt_segment* segs, size_t nsegs, int ntensors, float scale, void* workspace, float* norms,
                    void* stream);
int pa_lamb_step(const pa_lamb_opts* o, const pa_opt_group* groups_host, int ngroups, const pa_opt_segment* segs, size_t nsegs,
                 int ntensors, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float gscale,
                 const float* clip_coef, void* workspace, float* norms, float* trust, pa_adam_state* state, void* stream);
int pa_lars_step(const pa_lars_opts* o, const pa_opt_group* groups_host, int ngroups, const pa_opt_segment* segs, size_t nsegs,
                 int ntensors, float* param, const float* grad, float* momentum_buf, size_t n, float gscale, const float* clip_coef,
                 void* workspace, float* norms, float* trust, int32_t* state, void* stream);

/* Exponential moving average of the weights, updated on the device (utils.optim.ModelEma): ema += w (src - ema) after an optimizer
 * step, w = 1 - decay.  No reference counterpart: the reference validates and saves the raw weights.
 * state: 32 bytes on the device, zeroed once by the caller and owned by ONE average.  updates = averaging steps applied so far; held =
 * steps on which the average stayed because the optimizer skipped its own step; apply, w, decay_used = what the last pa_ema_advance
 * decided.  They live on the device for the reason pa_adam_state's step does: the half-precision build decides there whether the
 * optimizer's step is taken, and the average must not move (nor its warm-up count advance) on a skipped one.
 * pa_ema_advance: one one-thread launch, no host synchronisation.  skip_flag: NULL, or word 0 of the optimizer's own state (the int32
 * pair of pa_rmsprop_step_state, or a pa_adam_state), read on the device behind that optimizer's step.  Non-zero: apply = 0, held += 1,
 * nothing else changes.  Otherwise, in double, d = warmup ? min(decay, (1 + updates) / (10 + updates)) : decay; w = (float)(1.0 - d),
 * decay_used = (float)d, apply = 1, updates += 1.
 * pa_ema_lerp: apply == 0: every element untouched.  Otherwise per element, in fp32, ema = copy ? src : fmaf(w, src - ema, ema): one
 * subtraction, one fused multiply-add (torch.lerp(ema, src, w) for w < 0.5).  ema, src: n floats, 16-byte aligned, distinct arrays.
 * Zero padding stays zero; no atomics, the same input gives the same bits.  n == 0: returns 0, launches nothing.
 * Errors (non-zero, pa_last_error set, nothing launched): a NULL state / ema / src, ema == src, a misaligned ema or src, decay outside
 * [0, 1) or not finite, updates < 0 or > INT32_MAX. */
typedef struct pa_ema_state { int32_t updates, held, apply, reserved; float w, decay_used, reserved_f[2]; } pa_ema_state;
int pa_ema_advance(pa_ema_state* state, float decay, int warmup, const int32_t* skip_flag, void* stream);
int pa_ema_lerp(float* ema, const float* src, size_t n, const pa_ema_state* state, int copy, void* stream);
/* *updates, *held (either may be NULL); synchronises `stream`. */
int pa_ema_counts(const pa_ema_state* state, long long* updates, long long* held, void* stream);
/* state->updates = updates, on `stream` (loading a file); the other words stay. */
int pa_ema_set_updates(pa_ema_state* state, long long updates, void* stream);

/* Gradient accumulation over micro-batches (utils.optim: optimizer.accumulate() after a backward pass, then step()).  No reference
 * counterpart: the reference steps on every batch.
 * dst[i] = a[i] + b[i] for i < n: one fp32 addition per element, no scaling, no atomics, so the same input gives the same bits and a
 * group's sum is ((g1 + g2) + g3) + ... in the order of the calls; the mean is taken by the gscale of the step that follows.  inf, NaN
 * and denormal operands and results are ordinary values (inf + -inf = NaN).
 * b == NULL: a copy, dst[i] = a[i] (the first micro-batch of a group); with dst == a as well: returns 0, launches nothing.
 * dst may be exactly a or exactly b (in place), and a may be b; ranges that overlap in any other way are refused.  The pointers need
 * 4-byte alignment only: with all three 16-byte aligned (the flat arrays are) the kernel moves 16-byte chunks, otherwise (a view into a
 * flat array) single floats.
 * Errors (non-zero, pa_last_error set, nothing launched): a NULL dst or a, n < 1, ranges that overlap in part. */
int pa_grad_accumulate(float* dst, const float* a, const float* b, size_t n, void* stream);

/* ---------------------------------------------------------------- operator level ---------- */
/* One residual bottleneck block _Residual(C, C) (models/asn_stacked_hg.py:11-49), forward + backward,
 * NCHW fp32 in/out, parameters in the block's own state_dict order (flat fp32).  Used by the parity
 * tests; the networks below run the same kernels.  ws: zero-filled workspace of
 * pa_residual_workspace_bytes(). */
size_t pa_residual_workspace_bytes(int B, int H, int W, int C);
int pa_residual_fwd_bwd(const float* x, const float* dy, const float* params, float* y, float* dx, float* grads,
                        float* buffers, int B, int C, int H, int W, void* ws, void* stream);

/* One plain convolution (k = 1 or 3, stride 1, 'same'; nn.Conv2d of models/asn_stacked_hg.py:17-24)
 * through the implicit-GEMM kernels, NCHW fp32 in/out, PyTorch-layout fp32 weights.
 *   mode 0: out  = conv(a_in = x, w) + bias
 *   mode 1: out  = data gradient for a_in = dy
 *   mode 2: out  = weight gradient, out2 = bias gradient, for a_in = dy, b_in = x
 * ws: pa_conv2d_workspace_bytes() bytes. */
size_t pa_conv2d_workspace_bytes(int B, int Cin, int Cout, int H, int W, int k);
int pa_conv2d(int mode, const float* a_in, const float* b_in, const float* w, const float* bias, float* out, float* out2,
              int B, int Cin, int Cout, int H, int W, int k, void* ws, void* stream);

/* The data gradient of the 7x7 stride-2 pad-3 stem convolution, operator level like pa_conv2d: dy [B][64][H/2][W/2], w [64][3][7][7] fp32
 * (both rounded once to the storage type), dx fp32 and 16-byte aligned, fully overwritten: layout 0 [B][3][H][W], 1 [B][H][W][4] (4th
 * float 0).  The plain transposed convolution: no gradient scale in either build.  H, W even and >= 2; ws: pa_stem_dgrad_workspace_bytes()
 * bytes (0: bad shape), 16-byte aligned.  Enqueued on `stream`, no synchronisation. */
size_t pa_stem_dgrad_workspace_bytes(int B, int H, int W);
int pa_stem_dgrad(const float* dy, const float* w, float* dx, int B, int H, int W, int layout, void* ws, void* stream);

/* Several INDEPENDENT weight gradients the way the training step submits them (the conv1 / conv2 / conv3 / adapter gradients of one
 * _Residual, models/asn_stacked_hg.py:17-24, wait for one event and leave as ONE grouped launch): jobs[j] describes layer j
 * (device pointers, NCHW fp32 operands, PyTorch-layout fp32 outputs).
 *   dy_q / dy_k given: the dy operand arrives through the BatchNorm backward, dy_eff = kA[c] dy + kB[c] dy_q + kC[c], dy_k = [3][Cout]
 *   x_k given        : the x operand arrives through BatchNorm + ReLU,        x_eff  = max(0, k0[c] x + k1[c]),     x_k  = [2][Cin]
 *   db               : bias gradient (1x1 layers only) or NULL
 * mode 0: every layer as a launch of its own; 1: one grouped launch (jobs ordered longest first, as the step does); 2: one grouped
 * launch with the jobs in the caller's order.  Modes 1 / 2 return 2 when a job is not a shape / operand mode the grouped kernel takes
 * (3x3: Cin, Cout % 64 == 0, H % 8 == 0, W % 16 == 0, >= 48 tiles of 8 x 16 pixels, x through BatchNorm + ReLU; 1x1: >= 3 tiles of 128 pixels).
 * ws: pa_wgrad_group_workspace_bytes() bytes. */
#define PA_WG_GROUP_MAX 8
typedef struct pa_wgrad_job {
    int B, Cin, Cout, H, W, k;
    const float* dy;   const float* dy_q; const float* dy_k;
    const float* x;    const float* x_k;
    float* dw;         float* db;
} pa_wgrad_job;
size_t pa_wgrad_group_workspace_bytes(const pa_wgrad_job* jobs, int njobs);
int pa_wgrad_group(const pa_wgrad_job* jobs, int njobs, int mode, void* ws, void* stream);

/* NCHW fp32 <-> NHWC bf16 (fp32 -> storage type: round to nearest even).
 * Errors (non-zero, pa_last_error set, nothing launched): src or dst NULL; B, C, H or W < 1. */
int pa_nchw_to_nhwc(const float* src, void* dst_bf16, int B, int C, int H, int W, void* stream);
int pa_nhwc_to_nchw(const void* src_bf16, float* dst, int B, int C, int H, int W, void* stream);

/* ---------------------------------------------------------------- networks ---------------- */
typedef struct pa_net pa_net;

/* create_hg(num_stacks, num_modules=1, num_classes=16, chan) (models/asn_stacked_hg.py:344-347) for a
 * fixed per-GPU batch B and input resolution res (256).  chan must be a multiple of 128. */
pa_net* pa_hg_create(int num_stacks, int num_classes, int chan, int B, int res);
/* create_hg with num_modules residual blocks per site (models/asn_stacked_hg.py:73-77, :272-276): each of the 13 sites of an
 * hourglass and post_res is a chain of num_modules blocks, named "hg.<i>.<site>.<j>." (sites in the order down1-4, up1-4,
 * skip1-4, neck; j = 0 .. num_modules-1) and "post_res.<i>.<j>.".  1 <= num_modules <= 8, anything else returns NULL with
 * pa_last_error() set; every other condition is pa_hg_create's.  pa_hg_create is the num_modules == 1 case of the same code
 * (same tensor table, counts and workspace size). */
pa_net* pa_hg_create_modules(int num_stacks, int num_modules, int num_classes, int chan, int B, int res);
/* blocks per site of a pose net; 1 for an agent */
int pa_net_num_modules(const pa_net* net);
/* create_asn(chan, chan, scale_num, rotation_num, is_aug=True) (models/asn_stacked_hg.py:441-444) bound
 * to the feature shapes of a pose net with neck resolution res/64.  The head is the reference's AvgPool2d(4) + view +
 * Linear(chan, K): the mean of the TOP-LEFT 4 x 4 window of the res/64 top map (the whole map at res 256), gradient df / 16 inside
 * that window and 0 outside.  256 <= res <= 448 (one pool window); any other res returns NULL with pa_last_error() set. */
pa_net* pa_asn_create(int chan, int scale_num, int rotation_num, int B, int res);
/* create_asn(chan, chan, is_dropout=True) (models/asn_stacked_hg.py:378-379,437-439): the same trunk with the occlusion
 * head out_conv = Conv2d(chan, 1, 1) on the 4x4 map.  res must be 256 (the mask is the 4x4 neck map). */
pa_net* pa_asn_create_dropout(int chan, int B, int res);
void pa_net_destroy(pa_net* net);

/* state_dict description (names, shapes, offsets) in the reference's registration order */
int pa_net_num_tensors(const pa_net* net);
/* kind: 0 parameter (offset into the flat parameter array), 1 running_mean/var (offset into the flat
 * buffer array), 2 num_batches_tracked (no storage in the library) */
int pa_net_tensor_info(const pa_net* net, int i, char* name, int name_cap, int* shape4, int* ndim,
                       size_t* offset, size_t* numel, int* kind);
size_t pa_net_param_floats(const pa_net* net);
size_t pa_net_buffer_floats(const pa_net* net);
size_t pa_net_workspace_bytes(const pa_net* net);

/* params / grads / buffers: flat fp32 device arrays of pa_net_param_floats / pa_net_buffer_floats;
 * workspace: pa_net_workspace_bytes bytes; pa_net_bind clears it (no initialisation needed from the caller). */
int pa_net_bind(pa_net* net, float* params, float* grads, float* buffers, void* workspace, void* stream);
/* refresh the bf16 compute copies of the weights (after load_state_dict / an optimizer step) */
int pa_net_prepare_weights(pa_net* net);

/* _Hourglass_Wrapper.forward (models/asn_stacked_hg.py:282-342) + loss (stack-hg.py:156-159).
 * img: NCHW fp32 [B][3][res][res], or img4: bf16 NHWC4 from pa_affine_warp_bilinear (one of them).
 * pts: [B][16][2] float64 heat-map coordinates of the target joints, or NULL (no loss).
 * train != 0: BatchNorm uses batch statistics and updates the running estimates.
 * loss_per_stack: device fp32 [num_stacks] or NULL. */
int pa_hg_forward(pa_net* net, const float* img, const void* img4, const double* pts, int train, float* loss_per_stack);
/* heat maps of stack i: NHWC fp32 [B][H/4][W/4][16] inside the workspace (valid until the next forward) */
const float* pa_hg_heatmap_nhwc(const pa_net* net, int stack);
/* copy stack i's heat maps out as NCHW fp32 [B][16][res/4][res/4] (the reference's output tensors) */
int pa_hg_heatmap_nchw(pa_net* net, int stack, float* out);
/* loss.backward() (stack-hg.py:164): fills the flat gradient array bound with pa_net_bind */
int pa_hg_backward(pa_net* net);

/* loss.backward() in phases, for a data-parallel gradient exchange that overlaps the backward pass:
 * phase p = 0 .. num_stacks-1 enqueues the backward pass of stack num_stacks-1-p (its head layers, post block and hourglass),
 * phase num_stacks the stem and the final reductions; all phases in order == pa_hg_backward.
 * pa_hg_bucket_range: [lo, hi) = the contiguous range of the flat parameter / gradient array that holds hg.<stack> (13
 * sites of num_modules residual blocks each: 42 % of a 2-stack net's parameters per stack at num_modules 1).
 * pa_hg_bucket_wait: call after the phase of `stack`: makes `stream` (the caller's communication stream) wait until every
 * gradient in that range is final -- the main chain's work so far AND the slab reductions of the engine's weight-gradient
 * stream.  Returns 0, or -1 if the current stream mode finishes gradients only at the end (exchange everything after the
 * last phase then). */
int pa_hg_backward_phase(pa_net* net, int phase);
int pa_hg_bucket_range(const pa_net* net, int stack, size_t* lo, size_t* hi);
int pa_hg_bucket_wait(pa_net* net, int stack, void* stream);

/* pa_hg_forward(img4, pts) + pa_hg_backward in ONE call (stack-hg.py:153-164 without the optimizer).  use_graph != 0: the
 * ~650 launches of the two passes (main stream + the engine's side / weight-gradient streams, their fork / join events as
 * edges) are captured into a HIP graph on the first call and replayed afterwards; img4 / pts are copied into the engine's
 * own input buffers first (the graph's pointers are fixed).  Not available while dropout masks are set or the launch
 * profiler runs.  The gradient lands in the bound flat array; loss_per_stack (device, [num_stacks]) may be NULL. */
int pa_hg_train_step(pa_net* net, const void* img4, const double* pts, int train, int use_graph, float* loss_per_stack);
/* total_dev (device float, or NULL = off): every later pa_hg_forward / pa_hg_train_step that is given `pts` also writes
 * sum_stacks loss there -- `loss = sum(criterion(o, target))` of stack-hg.py:156-159 as one device scalar, so that the caller needs no
 * reduction launch of its own between the backward pass and the optimizer. */
int pa_hg_set_loss_total(pa_net* net, float* total_dev);

/* The backward pass from heat-map gradients of the caller's own loss (any loss of the heat maps: weighted, mined, distilled ...)
 * instead of the built-in MSE against the Gaussian target.
 * layout 0: [B][16][H][W] fp32 (what pa_hg_heatmap_nchw returns); 1: [B][H*W][16] fp32 (pa_hg_heatmap_nhwc's).
 * grads_host: HOST array of num_stacks DEVICE pointers, copied at the call; a NULL entry = zero gradient for that stack;
 * grads_host == NULL switches the door off (the built-in MSE gradient again).
 * Sticky, like pa_hg_set_dropout_masks: while set, pa_hg_backward and every pa_hg_backward_phase form stack i's heat-map gradient as
 *   storage(G_i * pa_grad_scale() (+ in_conv's data gradient for an inner stack))
 * in one launch per stack (the launch the MSE gradient takes otherwise) and run the unchanged backward pass from there; the gradients
 * are passed UNSCALED (the half-precision build applies its scale here; a value that leaves half's range becomes inf and the optimizer
 * skips that step like any overflow).  The joints (`pts`) are not read: a forward pass without them is enough.  The buffers are read in
 * stream order by the backward pass: keep them alive until it has run.  Works in train and eval mode and together with dropout masks.
 * Errors (nothing changes): an agent, a layout other than 0 / 1, every entry NULL, a pointer that is not 16-byte aligned; and
 * pa_hg_train_step(use_graph != 0) is refused while gradients are set. */
int pa_hg_set_heat_grads(pa_net* net, const float* const* grads_host, int layout);

/* d loss / d image of the next backward passes.  dimg: caller-owned device fp32, 16-byte aligned; layout 0: [B][3][res][res]
 * (the shape of `img`), 1: [B][res][res][4] (img4's pixel order, 4th float 0); NULL = off (default).  Sticky like
 * pa_hg_set_heat_grads.  While set, pa_hg_backward / the LAST pa_hg_backward_phase also write the gradient with respect to
 * the image the last forward pass read (img, or img4 as stored), UNSCALED (the half-precision build divides pa_grad_scale() out; a
 * gradient that overflowed there stays inf / NaN), fully overwritten, ordered on the net's stream when the call returns.  Works with
 * the built-in MSE gradient and with pa_hg_set_heat_grads, with dropout masks, in train and eval mode.  One more launch behind the
 * stem's weight gradient (the data gradient of the 7x7 stride-2 convolution); with dimg == NULL the step is launch for launch what it
 * is without this call.  Errors (nothing changes): an agent, layout not 0 / 1, a misaligned pointer; pa_hg_train_step(use_graph != 0)
 * is refused while set. */
int pa_hg_set_image_grad(pa_net* net, float* dimg, int layout);

/* Half-hourglass forward (models/asn_stacked_hg.py:300-304 with is_half_hg): stem + the down path of
 * hg[0] up to the neck -- everything the agent reads.  train != 0 updates the BatchNorm running
 * statistics of those layers, as the reference does on the agent-augmentation steps (Appendix A.9);
 * train == 2: batch statistics without touching the running estimates (the occlusion branch's whole-hourglass
 * call runs this pass, samples the masks and then the full forward, which does the one update). */
int pa_hg_forward_half(pa_net* net, const float* img, const void* img4, int train);

/* ASN.forward (models/asn_stacked_hg.py:401-436) on the pose net's detached features of the last
 * (half or full) forward (:159-164): logits [B][scale_num] and [B][rotation_num] (device, may be NULL).
 * train selects the agent's BatchNorm mode. */
int pa_asn_forward(pa_net* asn, pa_net* pose, int train, float* logits_scale, float* logits_rot);
/* softmax of the last pa_asn_forward's logits: [B][scale_num + rotation_num] (scale first), in the workspace */
const float* pa_asn_probs(const pa_net* asn);
/* KL loss of joint-train-pose-s-r-agent.py:399-407 against the target distributions (gen_groundtruth,
 * utils/util.py:147) + backward into the agent's flat gradient; no gradient reaches the pose net.
 * target_* [B][K] fp32 device; loss: device fp32 scalar or NULL. */
int pa_asn_backward(pa_net* asn, pa_net* pose, const float* target_scale, const float* target_rot, float* loss);
/* eps of log(softmax + eps) in that loss: 1e-7 (default, joint-train-pose-s-r-agent.py:399-404) or 0 for the agent
 * pre-training, which uses LogSoftmax (pretrain-s-r-agent.py:177-190). */
int pa_asn_set_log_eps(pa_net* asn, float eps);

/* Occlusion branch.
 * pa_asn_forward_masks: ASN.forward(is_dropout=True) (:437-439) on the pose net's detached features: mask_logits [B][16]
 * (cell = 4 * y + x), device, may be NULL.  train as in pa_asn_forward.
 * pa_asn_backward_masks: backward of the agent from a caller-provided d(loss)/d(mask_logits) [B][16] into the agent's flat
 * gradient (the reference ships no loss for this branch); nothing reaches the pose net.
 * pa_hg_set_dropout_masks: masks [B][16] fp32 (caller-owned device memory, e.g. from pa_sample_dropout_masks), or NULL to
 * switch the branch off.  While set, pa_hg_forward multiplies the neck and the four skip tensors of EVERY stack's hourglass by
 * the nearest-upsampled mask (:172-190, :322-324) and pa_hg_backward differentiates through it. */
int pa_asn_forward_masks(pa_net* asn, pa_net* pose, int train, float* mask_logits);
int pa_asn_backward_masks(pa_net* asn, pa_net* pose, const float* dlogits);
int pa_hg_set_dropout_masks(pa_net* net, const float* masks);

/* Evaluation.accuracy (pylib/Evaluation.py:54-75) of stack i's heat maps against the Gaussian target
 * of the joints given to the last forward: acc [nidx+1]. */
int pa_hg_accuracy(pa_net* net, int stack, const int32_t* idxs, int nidx, float* acc, float* scratch);

/* Evaluation.accuracy_origin_res (pylib/Evaluation.py:77-97) and, when person != NULL,
 * per_person_pckh (:99-167) of stack i's heat maps of the last forward, read in place (NHWC fp32).
 * center [B][2], scale [B], rot [B], gt_pts [B][16][2], norm [B] fp32; idxs int32 [nidx];
 * acc [nidx+1] or NULL; person [B] or NULL; scratch: 6*B*16 (+ B*16*(res/4)^2 if person) floats. */
int pa_hg_pckh(pa_net* net, int stack, const float* center, const float* scale, const float* rot, const float* gt_pts,
               const float* norm, const int32_t* idxs, int nidx, float* acc, float* person, float* scratch);

/* The meters of a TRAINING step beside its backward pass.  stack-hg.py:171-180 computes the accuracies of a batch from the forward pass's
 * heat maps after the optimizer step; they only read those maps, so a caller may ask for them between pa_hg_forward and pa_hg_backward:
 * with on != 0 the pa_hg_accuracy / pa_hg_pckh calls that follow are launched on a stream of the engine's own, behind everything the net's
 * stream holds at the call, and run beside the launches that stream is given next.  The net's stream waits for them at the end of the
 * next pa_hg_backward (the last pa_hg_backward_phase) or in front of the next forward pass; until then `acc`, `person`, `scratch` and the
 * meters' inputs must stay allocated and must not be read.  on == 0 (default): the meters run on the net's stream, ordered like every
 * other call.  Same values either way. */
int pa_net_meters_async(pa_net* net, int on);

/* Per-launch HIP-event timing of the MFMA kernels on the net's stream (bench.py's `roofline`).
 * begin: start recording; report: synchronise, stop recording and fill out_host[c][4] = {total ms, launches, algorithmic
 * bytes, flops} for the classes c = 0 fwd 1x1, 1 fwd 3x3, 2 dgrad 1x1, 3 dgrad 3x3, 4 wgrad 1x1, 5 wgrad 3x3 (maps of >= 16384
 * pixels: 32 x 32 and larger at batch 24), 6 stem fwd, 7 stem wgrad, 8 unused (the fused
 * low-resolution launch of rounds 3-4, removed: DESIGN.md), 9 / 10 / 11 forward / data-gradient / weight-gradient launches of the smaller maps (latency-bound).
 * out_host is a HOST array of `cap_classes` rows; classes beyond the capacity are dropped (never written).  Returns the library's
 * number of classes (PA_PROF_CLASSES = 12 today) through *n_classes when it is not NULL. */
#define PA_PROF_CLASSES 12
int pa_net_profile_begin(pa_net* net);
int pa_net_profile_report(pa_net* net, double* out_host, int cap_classes, int* n_classes);
/* class (0..11 as above) of every timed launch of the last reported pass, in launch order: returns their number and fills
 * out_host[0..min(cap, n)) (HOST array).  tools/trace_classes.py matches a rocprofv3 kernel trace of the same pass with it. */
int pa_net_profile_classes(const pa_net* net, int32_t* out_host, int cap);
/* BatchNorm finalize (models/asn_stacked_hg.py:19,22,25 in training mode) of a residual block's inner tensors at the low-resolution
 * levels: with at most `max_rows` partial statistics rows (default and upper limit 128: the 16 x 16 and smaller maps at batch 24) the
 * consumer convolution computes scale / shift (forward) or the BatchNorm-backward coefficients (backward) in its own prologue instead
 * of a finalize launch in front of it; 0 = always a launch.  Results are bit-identical either way (one summation order). */
int pa_net_set_fin_prologue(pa_net* net, int max_rows);
/* Gradient of the hourglass max pools (models/asn_stacked_hg.py:69): on (default) = the forward pool also stores a one-byte arg-max map per
 * pooled element and the data gradient of the skip branch beside the pool reads the pool's gradient through that map in its epilogue --
 * no pool backward launch and no full-resolution routed tensor, wherever the skip block's kernel has an instance for it; the stem's pool
 * likewise (its forward also stores the value at the arg-max: the pool's BatchNorm-backward reductions come from a quarter-size launch, the
 * routed gradient is formed on load by residual1's conv3 data gradient); off (0) = a pool backward launch per pool.  Results are
 * bit-identical either way.  Takes effect with the next forward pass. */
int pa_net_set_pool_route(pa_net* net, int on);
/* Bytes THIS design moves per step, from the engine's own launch table (bench.py's `roofline.design_bytes_per_step`): every operand
 * a launch of the last forward + backward pass reads or writes, counted once per launch at its storage width -- activations, the
 * second operand of a BatchNorm-backward load, reference tensors of the masked epilogues, shortcut addends, stored dz tensors, fp32
 * weight-gradient slabs written and read back, weights; halo re-reads and cache hits are NOT modelled (it is a floor for this set
 * of fusions, above the "every activation once" figure of SURVEY.md section 8d).  out_host[0] = bytes read, [1] = bytes written. */
int pa_net_design_bytes(const pa_net* net, double* out_host);
/* Bandwidth calibration for the same floor: dst[i] = src[i] with the engine's own plain 16-byte-per-lane streaming kernel (`bytes` a
 * multiple of 16).  Not part of the reference's surface (stack-hg.py has no roofline); bench.py times it on cold buffers of the step's
 * tensor sizes and on GB-sized ones. */
int pa_copy_probe(void* dst, const void* src, size_t bytes, void* stream);
/* ... in a chosen form: 0 = pa_copy_probe (grid-stride, four chunks in flight per thread), 1 = one 16-byte chunk per thread and no loop
 * (the "float4 copy" /opt/skills/guides/MI355X_MICROARCH.md quotes 6.29 TB/s for), 2 = form 0 with non-temporal loads / stores. */
int pa_copy_probe_form(void* dst, const void* src, size_t bytes, int form, void* stream);
/* Micro-benchmark of ONE convolution launch (tools/bench_conv*.py; no reference counterpart): mode 0 forward, 1 data gradient,
 * 2 weight gradient; variant bits: 1 input transform (BatchNorm+ReLU / BatchNorm backward on load), 2 statistics / masked epilogue,
 * 4 one residual addend, 8 (weight gradient) BatchNorm+ReLU on the x operand, 16: cold protocol is the caller's business.  `ws` =
 * caller-provided device workspace (>= 1 GiB for the benchmark's shapes); *ms_out = average milliseconds per launch over `iters`
 * launches (HIP events on `stream`). */
int pa_conv2d_time(int mode, int variant, int B, int Cin, int Cout, int H, int W, int k, int iters, void* ws, float* ms_out, void* stream);
/* Which kernel instance a forward / data-gradient convolution launch would take, as the launchers themselves plan it (csrc/conv_plan.h);
 * read-only, no device call, so it answers on a machine without a GPU.  Modes: operand loads -1 none, 0 plain, 1 BatchNorm + ReLU,
 * 2 BatchNorm backward, 3 pool-routed; epilogues 0 plain, 1 statistics, 2 BatchNorm backward (ep2: the second output's).  fin_rows: partial
 * rows of a pending finalize of the input (0 none).  flags: 1 bias, 2 second output (upsample-add backward), 4 a dz buffer is offered,
 * 8 in.map, 16 in.q, 32 ep2 scale / shift, 64 add2.map.  cus: compute units of the device (0 unknown).  Fills out[0..16) (HOST array, cap
 * >= 16) and returns 16: {path (0 refused, 1 generic, 2 one-shot, 3 row tile, 4 row tile with the second output, 5 halo tile),
 * instance id (tiling * 8 + variant, the enums of conv_plan.h), grid x, grid y, threads, channel blocks per workgroup, partial rows, partial
 * rows of the second output, xcd bits, takes a finalize, stores dz, pool-routed addend, pool-routed input, the LDS BatchNorm-backward
 * epilogue takes the launch, the instance cannot reach the kernels' trap for a launch that form does not take, the kernels' own copy of
 * that LDS rule}.  A refused launch also sets pa_last_error() to the reason; an admitted one leaves the last error as it is. */
int pa_conv_plan_describe(int B, int H, int W, int Cin, int Cout, int taps, int in_mode, int add1_mode, int add2_mode, int ep_mode,
                          int ep2_mode, int fin_rows, int flags, int cus, int* out, int cap);
/* Test hook: which convolution launches ran.  out == NULL clears the log and switches it on; every forward / data-gradient launch of this
 * process is then noted once (at most 1024 distinct ones) as the first 14 arguments of pa_conv_plan_describe.  out != NULL copies up to cap
 * launches of 14 ints each (HOST array), switches the log off and returns their number.  Not thread-safe; off by default. */
int pa_conv_launch_log(int* out, int cap);

/* The engine enqueues independent branches (hourglass skip blocks, weight gradients) on internal side
 * streams that fork from / join into the caller's stream by events.  on = 0 serialises everything on
 * the caller's stream (clean per-kernel timings: bench.py's roofline pass); on = 1 restores the default. */
int pa_net_set_multi_stream(pa_net* net, int on);

/* Test hook: copy one view of an internal activation out as NCHW fp32; shape4 receives {B, C, H, W} (out may be NULL to query the
 * shape).  grad selects the view:
 *   0  the value: the stored tensor with its pending BatchNorm+ReLU applied (in fp32, not rounded to the storage type);
 *   1  the stored gradient buffer: dz = d(value) * [value > 0] for an activation with a pending BatchNorm, the plain gradient otherwise;
 *   2  the raw stored tensor (BatchNorm not applied);
 *   3  the gradient with respect to the raw tensor: kA * dz + kB * raw + kC (in fp32) for an activation with a pending BatchNorm,
 *      the plain gradient otherwise;
 *   4  (the inner tensors ".x2" and the outputs of residual blocks) the same gradient as the data-gradient kernel of the tensor's
 *      consumer stored it, in the storage type, for the weight gradient and the shortcut addend (dz2 / dz3); an error when this step
 *      did not store it (the consumer's kernel computed it on the fly) or for any other tensor.
 * 1 and 3 return an error for a tensor without a gradient buffer; any other grad value is an error.  Every buffer the hook names keeps
 * its value to the end of the step (the arena gives each tensor its own storage).
 * Names: "stem", "res1".."res3", "pool0", "hg<i>.skip<k>|pool<k>|down<k>|up<k>|merge<k>|neck" (k=1..4),
 * "post<i>", "lin<i>", "xin<i>", optional suffix ".x1"/".x2" for a block's inner tensors.  A site of num_modules blocks (skip /
 * down / up / neck / post): the plain name is the site's output, i.e. its LAST block; "<site>.m<j>" names block j of the chain
 * ("hg0.up3.m0", "post1.m1.x2": ".x1"/".x2" come behind it), ".m<num_modules-1>" is the same tensor as the plain name, a j past the
 * chain is an error.  "heat<i>" (the heat maps as stored for
 * in_conv, 64 channels of which 16..63 are zero; its gradient: d heat as stored for out_conv's weight gradient), "heat<i>.in"
 * (in_conv's data gradient, 64 channels, no gradient) and "forth<i>" (forth_conv's stored output forth_conv(lin) + xin, no gradient)
 * for the head layers between stacks i and i + 1; "hg<i>.poolgrad<k>" (no gradient): the gradient max pool k routes back to its
 * input, plus for k = 1 the gradient reaching the hourglass input from the next stack, as skip k's conv1 data gradient adds it.  With
 * pool routing (pa_net_set_pool_route) the step does not store this tensor: asking for it runs the pool backward launch into its buffer
 * first, from the operands of the last step (same bits as a step without routing stores). */
int pa_hg_debug_tensor(pa_net* net, const char* which, int grad, float* out, int* shape4);

/* The same hook (and the same views) for the agent: "in<k>" (k = 0..4: residual_skip1-4, residual_neck), "pa<k>", "merge<k>"
 * (k = 0..3), "deep<k>" (k = 0..2), optional suffix ".x1"/".x2". */
int pa_asn_debug_tensor(pa_net* net, const char* which, int grad, float* out, int* shape4);

#ifdef __cplusplus
}
#endif
#endif
