"""pylib/Criterion.py of the reference, on the GPU."""
from ._dev import lib, check, ptr, stream, dev, to_dev, torch


def _loss(p, g, w, scale):
    loss = torch.zeros(1, dtype=torch.float32, device=dev())
    check(lib().pa_weighted_l2(ptr(p), ptr(g), ptr(w), p.numel(), ptr(loss), stream()), 'pa_weighted_l2')
    return loss[0] * scale


class _WeightedL2(torch.autograd.Function):
    """weighted_L2 for a `pred` that requires grad: forward pa_weighted_l2, backward pa_weighted_l2_grad (the gradient arriving at the
    loss stays a device float: no host synchronisation); gt and weight get no gradient."""

    @staticmethod
    def forward(ctx, pred, p, g, w, scale):
        ctx.p, ctx.g, ctx.w, ctx.scale = p, g, w, scale          # (p: pred's detached device copy, what the kernels read)
        return _loss(p, g, w, scale)

    @staticmethod
    def backward(ctx, gout):
        go = gout.detach().to(torch.float32).reshape(1)
        if ctx.scale != 1.0:
            go = go * ctx.scale
        go = go.contiguous()
        dpred = torch.empty_like(ctx.p)
        check(lib().pa_weighted_l2_grad(ptr(ctx.p), ptr(ctx.g), ptr(ctx.w), ctx.p.numel(), ptr(go), ptr(dpred), stream()),
              'pa_weighted_l2_grad')
        return dpred, None, None, None, None


def weighted_L2(pred, gt, weight):
    """((pred - gt)^2 * weight).sum() / numel  (pylib/Criterion.py:12-18).  `weight` may be a scalar
    1 (the inline loss of stack-hg.py:156-159) or a tensor of pred's shape.  Returns a 0-d GPU tensor.
    Differentiable in `pred` (a GPU tensor that requires grad, e.g. a heat map of HourglassNet.forward_autograd): the result then
    carries a grad_fn whose backward is the engine's kernel; gt and weight are constants."""
    p = to_dev(pred, torch.float32)
    g = to_dev(gt, torch.float32)
    w = None
    if isinstance(weight, torch.Tensor) and weight.numel() > 1:
        w = to_dev(weight.expand_as(p) if weight.shape != p.shape else weight, torch.float32)
    scale = 1.0
    if w is None:
        scale = float(weight) if not isinstance(weight, torch.Tensor) else float(weight.reshape(-1)[0])
    if isinstance(pred, torch.Tensor) and pred.requires_grad and torch.is_grad_enabled():
        if pred.device != p.device or pred.dtype != torch.float32:
            raise ValueError('weighted_L2: a pred that requires grad must be a float32 tensor on the HIP device')
        return _WeightedL2.apply(pred, p, g, w, scale)
    return _loss(p, g, w, scale)


def coord_L1(pred_xy, pts, valid=None, size=None):
    """Mean absolute coordinate error over the valid joints: sum(|pred_xy - pts| over x, y of the valid joints) / (2 * their number),
    0 when no joint is valid.  pred_xy: [B][J][2] predictions in heat-map coordinates (Evaluation.soft_argmax of the maps), pts: [B][J][2]
    targets (1-based, any float dtype).  valid: [B][J] bool; None: the reference's rule on pts, 0 < x <= W and 0 < y <= H with
    size = (W, H) of the heat maps (pylib/HumanPts.py:36-46: a joint outside gets an all-zero target map) -- without `size` only the
    lower half, x > 0 and y > 0, can be applied.  Plain torch on B * J * 2 numbers: differentiable in pred_xy, no host synchronisation.
    Returns a 0-d tensor."""
    if not isinstance(pred_xy, torch.Tensor) or pred_xy.dim() != 3 or pred_xy.shape[-1] != 2:
        raise ValueError('coord_L1: pred_xy must be a [B][J][2] tensor')
    t = torch.as_tensor(pts).to(device=pred_xy.device, dtype=pred_xy.dtype)
    if t.shape != pred_xy.shape:
        raise ValueError('coord_L1: pts %s does not match pred_xy %s' % (tuple(t.shape), tuple(pred_xy.shape)))
    if valid is None:
        v = (t[..., 0] > 0) & (t[..., 1] > 0)
        if size is not None:
            v = v & (t[..., 0] <= size[0]) & (t[..., 1] <= size[1])
    else:
        v = torch.as_tensor(valid).to(device=pred_xy.device, dtype=torch.bool)
        if v.shape != pred_xy.shape[:2]:
            raise ValueError('coord_L1: valid %s must be [B][J] = %s' % (tuple(v.shape), tuple(pred_xy.shape[:2])))
    w = v.to(pred_xy.dtype).unsqueeze(-1)
    return ((pred_xy - t).abs() * w).sum() / (2.0 * w.sum()).clamp(min=1.0)
