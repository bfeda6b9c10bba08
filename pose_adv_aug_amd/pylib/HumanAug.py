"""pylib/HumanAug.py of the reference, on the GPU: similarity transforms, joint transforms and the
scale/rotation crop (pre-downscale, window, rotate, resize: the reference's own pixel pipeline) on the device."""
from .. import _lib
from ._dev import lib, check, ptr, stream, dev, to_dev, np, torch

FLIP_PAIRS = ((0, 5), (1, 4), (2, 3), (10, 15), (11, 14), (12, 13))          # pylib/HumanAug.py:241-244
FLIP_CHANNELS = ((1, 4), (0, 5), (12, 13), (11, 14), (10, 15), (2, 3))        # pylib/HumanAug.py:182


def _scalar(v):
    return float(np.asarray(v, dtype=np.float64).reshape(-1)[0])


def make_params(center, scale, rot, flip=None, gain=None):
    """[B][8] float64 {cx, cy, scale, rot, flip, gain_r, gain_g, gain_b} (layout of include/poseadv.h)."""
    c = np.asarray(center, dtype=np.float64).reshape(-1, 2)
    B = c.shape[0]
    p = np.zeros((B, 8), dtype=np.float64)
    p[:, 0:2] = c
    p[:, 2] = np.asarray(scale, dtype=np.float64).reshape(-1)
    p[:, 3] = np.asarray(rot, dtype=np.float64).reshape(-1)
    p[:, 4] = 0 if flip is None else np.asarray(flip, dtype=np.float64).reshape(-1)
    p[:, 5:8] = 1 if gain is None else np.asarray(gain, dtype=np.float64).reshape(-1, 3)
    return torch.from_numpy(p).to(dev())


def affine_params(params, res_in=256, res_out=64):
    """device: params [B][8] -> (T at res_out [B][6] float64, T^-1 at res_in [B][6] float64)."""
    B = params.shape[0]
    t = torch.empty((B, 6), dtype=torch.float64, device=dev())
    ti = torch.empty((B, 6), dtype=torch.float64, device=dev())
    check(lib().pa_affine_params(ptr(params), B, res_in, res_out, ptr(t), ptr(ti), stream()), 'pa_affine_params')
    return t, ti


def GetTransform(center, scale, rot, res, size):
    """pylib/HumanAug.py:10-35 -> 3x3 float64 numpy."""
    if size != 200:
        raise ValueError('the reference always uses size == 200')
    p = make_params(np.asarray(center, dtype=np.float64).reshape(1, 2), [_scalar(scale)], [_scalar(rot)])
    t, _ = affine_params(p, res_in=int(res), res_out=int(res))
    out = np.eye(3)
    out[:2, :] = t.cpu().numpy().reshape(2, 3)
    return out


def TransformPts(pts, center, scale, rot, res, size, invert=0):
    """pylib/HumanAug.py:45-54 (0-based, float result)."""
    t = GetTransform(center, scale, rot, res, size)
    if invert:
        t = np.linalg.inv(t)
    p = np.concatenate((np.asarray(pts, dtype=np.float64), np.ones((len(pts), 1))), axis=1).T
    return np.dot(t, p)[0:2, :].T


def transform_pts_batch(pts, params, t, width, sizes=None):
    """device: joints [B][J][2] fp32 image px -> (heat-map coords [B][J][2] float64 with invalid joints
    zeroed, mirrored/swapped image-space joints [B][J][2] fp32).  pylib/HumanAug.py:45-54,236-257 and
    data/mpii_for_mpii.py:138-146."""
    p = to_dev(pts, torch.float32)
    B, J = p.shape[0], p.shape[1]
    out = torch.empty((B, J, 2), dtype=torch.float64, device=dev())
    img = torch.empty((B, J, 2), dtype=torch.float32, device=dev())
    if sizes is not None:          # frames of different sizes: every sample mirrors about its own width
        check(lib().pa_transform_pts_sized(ptr(p), ptr(params), ptr(t), B, J, ptr(sizes), ptr(out), ptr(img), stream()),
              'pa_transform_pts_sized')
    else:
        check(lib().pa_transform_pts(ptr(p), ptr(params), ptr(t), B, J, float(width), ptr(out), ptr(img), stream()),
              'pa_transform_pts')
    return out, img


_CROP_WS = {}


def _crop_workspace(B, Hs, Ws, res, stretch=False):
    """scratch of pa_crop / pa_crop_stretch (intermediate images of the staged crop), sized for the mode in use (the stretch
    mode's is the same layout plus its accumulators and tables): ONE grow-only buffer per (device, stream it is used
    on), re-allocated only when pa_crop_workspace_bytes asks for more than it holds -- the MPII feed pads every batch to its
    own (Hs, Ws), a cache per shape would grow by ~90 MB per new shape.  Keyed by the stream so that the crop enqueued one step
    ahead on the augmentation stream (data.AugmentAhead) and a crop on the main stream (validate) never share scratch; a
    buffer that is outgrown is released through torch's stream-ordered allocator on the stream that used it."""
    need = int((lib().pa_crop_stretch_workspace_bytes if stretch else lib().pa_crop_workspace_bytes)(B, Hs, Ws, res))
    key = (str(dev()), int(getattr(stream(), 'value', stream()) or 0))
    ws = _CROP_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _CROP_WS[key] = torch.empty(need, dtype=torch.uint8, device=dev())
    return ws


def crop_batch(frames, params, res=256, want_nchw=False, want_nhwc4=True, want_u8=False, sizes=None, stretch=False):
    """device: uint8 frames [B][Hs][Ws][3] + params [B][8] -> network input (bf16 NHWC4) and/or fp32 NCHW and/or the uint8
    crop [B][res][res][3].  crop (pylib/HumanAug.py:117-176: pre-downscale, int-truncated window, PIL rotate, PIL resize)
    behind flip + colour gain (data/mpii_for_mpii.py:126-135).  stretch=False (the default, pa_crop): the frame is scaled by
    its full range -- byte-exact against the reference over Pillow only for crops that hold a pure black and a pure white
    pixel.  stretch=True (pa_crop_stretch): scipy's toimage() min/max byte stretch of the frame (pre-downscale case) and of
    the window is reproduced -- byte-exact against the reference for every crop, for three more launches and one more read of
    every pre-downscaled frame."""
    f = frames if (isinstance(frames, torch.Tensor) and frames.device == dev()) else to_dev(frames, torch.uint8)
    B, Hs, Ws, _ = f.shape
    out4 = torch.empty((B, res, res, 4), dtype=_lib.act_dtype(), device=dev()) if want_nhwc4 else None
    outf = torch.empty((B, 3, res, res), dtype=torch.float32, device=dev()) if want_nchw else None
    out8 = torch.empty((B, res, res, 3), dtype=torch.uint8, device=dev()) if want_u8 else None
    fn, name = (lib().pa_crop_stretch, 'pa_crop_stretch') if stretch else (lib().pa_crop, 'pa_crop')
    check(fn(ptr(f), Hs, Ws, ptr(sizes), ptr(params), B, res, ptr(_crop_workspace(B, Hs, Ws, res, stretch)), ptr(out4), ptr(outf),
             ptr(out8), stream()), name)
    return out4, outf, out8


def warp_batch(frames, tinv, params, res=256, want_nchw=False, want_nhwc4=True, sizes=None):
    """device: the PURE inverse-affine bilinear sampler (2 x 2 taps at T^-1(u, v), no pre-filter) -- an operator, not the
    reference's crop pixels (crop_batch is what the loops use)."""
    f = frames if (isinstance(frames, torch.Tensor) and frames.device == dev()) else to_dev(frames, torch.uint8)
    B, Hs, Ws, _ = f.shape
    out4 = torch.empty((B, res, res, 4), dtype=_lib.act_dtype(), device=dev()) if want_nhwc4 else None
    outf = torch.empty((B, 3, res, res), dtype=torch.float32, device=dev()) if want_nchw else None
    if sizes is not None:
        check(lib().pa_affine_warp_bilinear_sized(ptr(f), Hs, Ws, ptr(sizes), ptr(tinv), ptr(params), B, res, ptr(out4), ptr(outf),
                                                  stream()), 'pa_affine_warp_bilinear_sized')
    else:
        check(lib().pa_affine_warp_bilinear(ptr(f), Hs, Ws, ptr(tinv), ptr(params), B, res, ptr(out4), ptr(outf), stream()),
              'pa_affine_warp_bilinear')
    return out4, outf


_WARP_LAYOUTS = {'nchw': 0, 'nhwc4': 1}


def _want(t, what, dtype, shape):
    """ValueError unless t is a contiguous GPU tensor of `dtype` and `shape` (None = any extent)"""
    if not isinstance(t, torch.Tensor):
        raise ValueError('%s must be a torch tensor' % what)
    if t.dtype != dtype:
        raise ValueError('%s must be %s, not %s' % (what, dtype, t.dtype))
    if t.dim() != len(shape) or any(w is not None and int(s) != int(w) for s, w in zip(t.shape, shape)):
        raise ValueError('%s must have shape %s, not %s' % (what, list(shape), list(t.shape)))
    if not t.is_cuda:
        raise ValueError('%s must be on the GPU' % what)
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous' % what)


def warp_batch_backward(frames, tinv, params, dimg, layout='nchw', sizes=None):
    """device: the backward pass of warp_batch (pa_affine_warp_bilinear_bwd).  dimg = d loss / d (its fp32 output): fp32
    [B][3][res][res] (layout 'nchw') or [B][res][res][4] ('nhwc4', 4th float ignored), the two forms HourglassNet.backward(input_grad=...)
    delivers.  Returns (dtinv [B][6], dgain [B][3], dparams [B][8]) in float64; dparams = d loss / d {cx, cy, scale, rot per degree,
    0, gain r g b} assumes tinv = affine_params(params, res_in=res)[1].  A wrong shape, dtype or device raises ValueError before any launch."""
    if layout not in _WARP_LAYOUTS:
        raise ValueError("layout must be 'nchw' or 'nhwc4', not %r" % (layout,))
    _want(frames, 'frames', torch.uint8, (None, None, None, 3))
    B, Hs, Ws, _ = frames.shape
    if B < 1 or Hs < 1 or Ws < 1:
        raise ValueError('frames must hold at least one pixel')
    _want(tinv, 'tinv', torch.float64, (B, 6))
    _want(params, 'params', torch.float64, (B, 8))
    if not isinstance(dimg, torch.Tensor) or dimg.dim() != 4:
        raise ValueError('dimg must be a 4-d torch tensor')
    res = int(dimg.shape[2])
    _want(dimg, 'dimg', torch.float32, (B, 3, res, res) if layout == 'nchw' else (B, res, res, 4))
    if res < 1:
        raise ValueError('dimg must hold at least one pixel')
    if dimg.data_ptr() % 16:
        raise ValueError('dimg must be 16-byte aligned')
    if sizes is not None:
        _want(sizes, 'sizes', torch.int32, (B, 2))
    if len({t.device for t in (frames, tinv, params, dimg) + ((sizes,) if sizes is not None else ())}) != 1:
        raise ValueError('frames, tinv, params, dimg and sizes must be on one device')
    d = frames.device
    ws = torch.empty(int(lib().pa_affine_warp_bwd_workspace_bytes(B, res)), dtype=torch.uint8, device=d)
    dtinv = torch.empty((B, 6), dtype=torch.float64, device=d)
    dgain = torch.empty((B, 3), dtype=torch.float64, device=d)
    dparams = torch.empty((B, 8), dtype=torch.float64, device=d)
    check(lib().pa_affine_warp_bilinear_bwd(ptr(frames), Hs, Ws, ptr(sizes), ptr(tinv), ptr(params), B, res, ptr(dimg),
                                            _WARP_LAYOUTS[layout], ptr(ws), ptr(dtinv), ptr(dgain), ptr(dparams), stream()),
          'pa_affine_warp_bilinear_bwd')
    return dtinv, dgain, dparams


class _WarpFn(torch.autograd.Function):
    """pa_affine_params + the bilinear sampler -> (fp32 NCHW, storage-type NHWC4 or None); backward: pa_affine_warp_bilinear_bwd"""

    @staticmethod
    def forward(ctx, params, frames, res, sizes, want_nhwc4):
        p = params.detach().contiguous()
        _, tinv = affine_params(p, res_in=res, res_out=res)
        out4, outf = warp_batch(frames, tinv, p, res=res, want_nchw=True, want_nhwc4=want_nhwc4, sizes=sizes)
        ctx.frames, ctx.sizes = frames, sizes
        ctx.save_for_backward(params, tinv)          # (saved, not just kept: an in-place change of params before backward() is then an error)
        if out4 is None:
            return outf, None
        ctx.mark_non_differentiable(out4)
        return outf, out4

    @staticmethod
    def backward(ctx, dimg, _d4=None):
        if dimg is None:
            return None, None, None, None, None
        params, tinv = ctx.saved_tensors
        g = dimg.to(torch.float32).contiguous()
        if g.data_ptr() % 16:
            g = g.clone()
        _, _, dparams = warp_batch_backward(ctx.frames, tinv, params.detach().contiguous(), g, 'nchw', ctx.sizes)
        return dparams, None, None, None, None


def _warp_inputs(frames, params):
    f = frames if (isinstance(frames, torch.Tensor) and frames.device == dev()) else to_dev(frames, torch.uint8)
    if not isinstance(params, torch.Tensor) or params.dtype != torch.float64 or params.dim() != 2 or params.shape[1] != 8 or \
            params.shape[0] != f.shape[0] or not params.is_cuda:
        raise ValueError('params must be a float64 [B][8] tensor on the GPU')
    return f.contiguous()


def warp_autograd(frames, params, res=256, sizes=None, want_nhwc4=False):
    """device: affine_params + warp_batch as ONE differentiable operator of the augmentation parameters: uint8 frames [B][Hs][Ws][3],
    params float64 [B][8] -> fp32 NCHW [B][3][res][res] (the sampler's `outf`: the gradient that comes back is fp32, not rounded to the
    storage type).  With params.requires_grad the result carries a grad_fn and backward() leaves d loss / d {cx, cy, scale, rot per
    degree, gain} in params.grad (float64 [B][8], flip column 0); changing params in place between the two is an error.  Within a source
    cell the sampler is smooth; the clamp passes the gradient where 0 <= gain * S <= 1 and floor is taken as locally constant
    (include/poseadv.h).  The frames get no gradient.  Without params.requires_grad this is warp_batch and nothing else is launched.
    want_nhwc4: return (fp32 NCHW, the same launch's storage-type NHWC4 copy, which carries no gradient) instead of the one tensor.
    (crop_batch, the reference's PIL-exact crop, stays non-differentiable.)"""
    f = _warp_inputs(frames, params)
    if not (params.requires_grad and torch.is_grad_enabled()):
        p = params.detach().contiguous()
        _, tinv = affine_params(p, res_in=res, res_out=res)
        out4, outf = warp_batch(f, tinv, p, res=res, want_nchw=True, want_nhwc4=bool(want_nhwc4), sizes=sizes)
    else:
        outf, out4 = _WarpFn.apply(params, f, int(res), sizes, bool(want_nhwc4))
    return (outf, out4) if want_nhwc4 else outf


def crop(img, center, scale, rot, res, size, stretch=False):
    """Reference signature (pylib/HumanAug.py:117): H x W x 3 image (float [0,1] or uint8) -> res x res x 3 uint8, with the
    reference's pixels (its PIL arithmetic restated on the device).  stretch=False: without scipy's per-image min/max byte
    stretching.  stretch=True: with it -- exact for float images whose values are k / 255 (k = 0..255, what a loaded uint8
    image divided by 255 holds: the image is taken back to those bytes and the device works from them); other float values
    are rounded to the nearest k / 255 first, and the result is then not the reference's."""
    if size != 200:
        raise ValueError('the reference always uses size == 200')
    a = np.asarray(img)
    if a.dtype != np.uint8:
        a = (np.clip(a.astype(np.float64) * 255.0, 0, 255) + 0.5).astype(np.uint8)      # toimage() with the full range
    p = make_params(np.asarray(center, dtype=np.float64).reshape(1, 2), [_scalar(scale)], [_scalar(rot)])
    _, _, out8 = crop_batch(np.ascontiguousarray(a)[None], p, res=int(res), want_nhwc4=False, want_u8=True, stretch=stretch)
    return out8[0].cpu().numpy()


def shufflelr(x, width, dataset='mpii'):
    """pylib/HumanAug.py:236-257 (in place on a 16 x 2 tensor, like the reference)."""
    assert dataset == 'mpii'
    x[:, 0] = width - x[:, 0]
    for a, b in FLIP_PAIRS:
        tmp = x[a, :].clone(); x[a, :] = x[b, :]; x[b, :] = tmp
    return x


def fliplr(x):
    """pylib/HumanAug.py:260-266: mirror the last axis of a CHW / NCHW numpy array."""
    return np.ascontiguousarray(np.asarray(x)[..., ::-1]).astype(float)


def flip_channels(maps):
    """pylib/HumanAug.py:198-210."""
    return maps.flip(-1).float()


def flip_lr_img4(img4):
    """device: mirror the bf16 NHWC4 network input along W (stack-hg.py:223 `img.numpy()[:, :, :, ::-1]`)."""
    B, H, W, _ = img4.shape
    out = torch.empty_like(img4)
    check(lib().pa_flip_lr_nhwc4(ptr(img4), ptr(out), B, H, W, stream()), 'pa_flip_lr_nhwc4')
    return out


def flip_tta_merge(output, output_flipped):
    """device, one kernel: (output + shuffle_channels_for_horizontal_flipping(flip_channels(output_flipped))) / 2
    (stack-hg.py:228-230) for NCHW fp32 MPII heat maps."""
    a = to_dev(output, torch.float32); b = to_dev(output_flipped, torch.float32)
    B, J, H, W = a.shape
    out = torch.empty_like(a)
    check(lib().pa_flip_tta_merge(ptr(a), ptr(b), ptr(out), B, J, H, W, stream()), 'pa_flip_tta_merge')
    return out


def shuffle_channels_for_horizontal_flipping(maps):
    """pylib/HumanAug.py:179-196 (in place)."""
    dim = 1 if maps.dim() == 4 else 0
    for a, b in FLIP_CHANNELS:
        tmp = maps.narrow(dim, a, 1).clone()
        maps.narrow(dim, a, 1).copy_(maps.narrow(dim, b, 1))
        maps.narrow(dim, b, 1).copy_(tmp)
    return maps
