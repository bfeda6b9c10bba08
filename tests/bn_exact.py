"""Exact checks of the code that links the convolutions: every BatchNorm (statistics, finalize, running estimates, parameter gradients,
backward, eval mode), every max pool forward and every upsample-add (forward and backward) of the hourglass net, each recomputed in
float64 from the tensors the engine itself stored after ONE training step (pa_hg_debug_tensor views 0-4, include/poseadv.h).  That step is
the first one after the bind ('fresh') or one behind a history of optimizer steps, graph replays, eval-mode and unfinished forwards, entered
as bench.py enters its timed steps (tests/exact_history.py); parameters and running estimates are those held immediately before it.

What 'bn backward' covers: view 3 applies the finalize's kA / kB / kC to dz and raw in the hook's own fp32 load, so that check pins the
backward finalize constants (kB, kC carry the backward sums; kA the forward's invstd).  The tensors the data-gradient kernels store for
the later readers (dz2 / dz3 of every residual block that materialises them: weight gradients, shortcut addends) are view 4; 'stored
bn backward' compares them bit for bit with view 3 rounded once to the storage type -- the kernels' own fmaf(kA, dz, fmaf(kB, x, kC)).
Where a block's consumer computes that gradient on the fly instead (not stored), the kernel's operand load is covered only through
the node tests (tests/test_gpu_local.py).

tests/test_gpu_bn_exact.py runs the legs; for the IEEE-half build it runs this file as a child process (one storage type per process,
like tests/fp16_check.py).  tests/test_bn_exact_cpu.py shows on synthetic tensors that the bounds exclude the defects they are for.

Bounds.  Nothing here is fitted to observed errors: every bound is a first-order forward error analysis of the fp32 evaluation of the
formula the engine implements (bn_fin.h pa_bn_fwd_consts / pa_bn_running / pa_bn_bwd_consts, the epilogues' sums of dz and
dz * (x - mean) * invstd, bn_eval_kernel), with u = 2^-24 and these rules (class E below):
  * an fp32 add / sub / mul / correctly rounded division of two quantities known to within e_a, e_b adds |a| e_b + |b| e_a + e_a e_b of
    propagated error and u (|result| + propagated error) of rounding; fmaf rounds once;
  * rsqrtf (v_rsq_f32) is within 1 ulp = 2u: its bound is the exact interval [rsqrt(t + e), rsqrt(t - e)] widened by 2u;
    sqrtf (the optimizer, tests/optim_exact.py) by the same rule: [sqrt(t - e), sqrt(t + e)] widened by 2u;
  * expf / logf (the agent's softmax and KL loss, tests/asn_exact.py): the exact interval of the function over its argument's interval,
    widened by 2 ulp = 4u of the result -- an ASSUMPTION (see tests/asn_exact.py);
  * a per-channel sum of n fp32 values computed by any tree in which no value passes through more than D additions is within
    D u sum|x_i| of the exact sum.  D (sum_depth) is derived from the kernels of the release build, in two parts:
      - inside one partial row: a conv epilogue's row covers at most 128 pixels (the 1 x 1 / 3 x 3 tile kernels and the implicit-GEMM
        kernels write 64- or 128-pixel rows, the fused upsample-add epilogue 16 low-resolution pixels; the three-tile 384-pixel 3 x 3
        workgroups are not compiled in), and any tree over P values is at most P - 1 deep: <= 127.  A streaming kernel (max-pool /
        upsample-add backward, ep_apply) keeps one channel group per thread: a chain over its items (<= ceil(n C / (8 * 65536)) + 4
        pixels: <= 512 workgroups of >= 128 threads), at most 6 shuffle levels and a chain over <= 16 waves;
      - the finalize over R partial rows: the launch form chains ceil(R / 64) rows per slice, then two 16-wide levels (+ 20); the
        consumer-prologue form (R <= 128) is 8 + 4 deep.  R is at most the statistics capacity max(512, ceil(n / 64)), four times
        that for the backward rows of bn3 in the up blocks (Residual::b3_rows_scale).
    At C = 512 (the chan-512 legs; re-derived from launch_plan.h, kernels.h and bn_fin.h, nothing changes in D): C / 8 = 64 channel
    groups fill a wave, so flush_stats shuffles over no level at all (<= 6) and the workgroups tried (512 / 256; 384, 192 and 128 are
    no multiples of 64) have <= 8 waves (<= 16); the item count per thread is the same formula in C; the row capacity
    pa_max_stat_rows = max(512, ceil(n / 64)) does not depend on C; and the consumer-prologue finalize, which the plan's takes_fin does not
    admit above 256 input channels, is replaced by the launch form, whose order for R <= 128 rows is the prologue's own (8 + 4 deep,
    reduce_partial_rows) and for more rows ceil(R / 64) + 20 as above.
    At the input resolutions 320 / 448 / 192 / 64 (maps 80 ... 5, 112 ... 7, 48 ... 3, 16 ... 1; re-derived from launch_plan.h,
    elementwise.hip, conv_plan.h and conv3x3_tile.hip, nothing changes in D): the streaming launches whose row items
    (W / 2) * (C / 8) fit none of the tried workgroup sizes 512 / 256 / 384 / 192 / 128 (W 20 / 28 / 10 / 14 at chan 256, also W 40 / 56
    at chan 128) run the generic grid-stride kernels with the first-computed 256 or 512 threads (>= 128) in <= 512 workgroups, the same
    one-group-per-thread chain, shuffle levels and <= 16 waves, so the streaming term stands as written (these launches stay below 512
    workgroups: one item, four pixels, per thread); where a size fits it is one of the tried ones, all >= 128.  The generic conv kernel
    takes the 3 x 3 layers of the 10 x 10 / 14 x 14 maps in 64-pixel rows, and the ONE masked 8 x 8 tile of the 5 x 5 / 7 x 7 / 3 x 3 /
    1 x 1 maps writes one row per workgroup of two images, at most 2 * 49 of its 128 pixels alive: both inside the <= 127 of a row.
    The row counts (<= 200 for the 80 x 80 maps at B 2, 1 ... 4 at the necks) stay below the capacity 512 the finalize term assumes.
  * the backward sum of dz * xhat is written in two forms: per term dz * (x - mean) * invstd (epilogue8, Bwd8, pa_conv_epilogue),
    or per partial row invstd * (sum dz x - mean sum dz) (pa_conv_epilogue_lds_bwd, pa_conv_epilogue_lds_up), which cancels when
    |mean| >> sigma.  The bound covers both: the rounding terms are taken over |dz| (|x - mean| + 2 |mean|), which bounds
    |dz x| + |mean dz| as well as |dz (x - mean)|.
  * a bound that has lost its meaning (the interval of invstd wider than 1 %: at these depths a channel whose |mean| / sigma exceeds
    about 10) is reported as a failure of its own ('degenerate bound') instead of passing every check of that BatchNorm.
The parameters, running estimates and stored tensors are fp32 / storage-type values, exact in float64.  Gradient quantities are compared
in the engine's own units (the fp16 build carries pa_grad_scale() in every gradient: all checks are homogeneous in it).

Pool forward, merge forward and merge backward involve no accumulation: one fp32 max / add / 2 x 2 sum in a fixed order, rounded once to
the storage type (round to nearest even, the conversion of gfx950 and of torch), so they are compared bit for bit.

Pool backward (maxpool_bwd_kernel and the streaming maxpool_bwd_s_kernel of elementwise.hip, both `if (v[k] > m)` over
k = 0..3 = top-left, top-right, bottom-left, bottom-right: the FIRST maximum in scan order keeps the gradient) is bit-exact too: the
value compared is the fp32 BatchNorm+ReLU value view 0 (the kernels' own fmaxf(fmaf(k0, raw, k1), 0)), the routed gradient takes at
most one fp32 add (the addend: d xin<i+1> into poolgrad1 of an inner stack, Hourglass::bwd net.hip:807) and one rounding; with a
BatchNorm-backward epilogue (pool0 into res1, net.hip:986; the agent's merges) the stored view 1 is the ReLU-masked routed gradient.
After ReLU most windows of a map hold several zeros, so ties are the common case: a leg must have met tied windows ('tied pool
windows'), or 'first maximum' was not tested.

The step with occlusion masks (run_leg(masks=...)): the decoder reads copies of the skip and neck outputs multiplied by the 4 x 4 cell
mask.  The copies, the merges over them, the copies' gradients (d merged itself: a plain tensor) and the gradients the cell mask's
backward launch hands to skip<k> / neck (times the mask, times the tensor's own ReLU mask) are bit for bit; that launch's epilogue also
produces the backward sums of skip<k>.bn3 / neck.bn3, which check_bn_site recomputes from view 1 like everywhere else.

check_bn_site / check_bn_eval_site are the per-BatchNorm checks; the probe of the tensor is an argument, so tests/asn_exact.py runs
the same checks (one definition of each bound) over the agent's BatchNorms through AsnProbe."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS, MOMENTUM = 1e-5, 0.1
_F32 = lambda v: float(np.float32(v))
# the fp32 constants the engine uses for eps, momentum and 1 - momentum, as (value, distance from the exact constant)
EPS32 = (EPS, abs(_F32(EPS) - EPS))
MOM32 = (MOMENTUM, abs(_F32(MOMENTUM) - MOMENTUM))
ONE_MINUS_MOM32 = (1.0 - MOMENTUM, abs(_F32(np.float32(1.0) - np.float32(MOMENTUM)) - (1.0 - MOMENTUM)))


def sum_depth(n, C, rows_scale=1):
    """D: the most additions any value passes through in a per-channel sum over n pixels of C channels (module docstring)."""
    stream = -(-n * C // (8 * 65536)) + 4 + 6 + 16
    rows = rows_scale * max(512, -(-n // 64))
    return max(127, stream) + -(-rows // 64) + 20


# ---------------------------------------------------------------------------------------------------------------------------------
# first-order error propagation of an fp32 evaluation: E(v, e) = the exact value v (float64) and a bound e on |fp32 result - v|
class E(object):
    def __init__(self, v, e=None):
        self.v = v if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else (e if torch.is_tensor(e) else torch.full_like(self.v, float(e)))

    @staticmethod
    def _r(v, e):
        return E(v, e + U * (v.abs() + e))

    def __add__(self, o):
        return E._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return E._r(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return E._r(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    def __truediv__(self, n):           # by an exact positive count
        return E._r(self.v / n, self.e / n)

    def __neg__(self):
        return E(-self.v, self.e)

    def div(self, o):                   # by another E whose interval excludes 0: correctly rounded (hipcc's default for fp32 '/')
        v = self.v / o.v
        return E._r(v, (self.e + v.abs() * o.e) / (o.v.abs() - o.e).clamp_min(1e-300))

    def exp(self, ulps=2):              # expf within `ulps` ulp (1 ulp <= 2u relative) of the exact exponential of its fp32 argument
        v = self.v.exp()
        e = v * torch.expm1(self.e)
        return E(v, e + ulps * 2 * U * (v + e))

    def log(self, ulps=2):              # logf of a positive quantity
        v = self.v.log()
        lo = (self.v - self.e).clamp_min(1e-300).log()
        hi = (self.v + self.e).log()
        e = torch.maximum(v - lo, hi - v)
        return E(v, e + ulps * 2 * U * (v.abs() + e))

    def rsqrt(self):
        lo = (self.v + self.e).rsqrt()
        hi = (self.v - self.e).clamp_min(1e-300).rsqrt()
        v = self.v.rsqrt()
        return E(v, torch.maximum(v - lo, hi - v) + 2 * U * hi)

    def sqrt(self):                     # sqrtf of a quantity >= 0 (the optimizer, tests/optim_exact.py): the rule of rsqrt
        lo = (self.v - self.e).clamp_min(0).sqrt()
        hi = (self.v + self.e).sqrt()
        v = self.v.sqrt()
        return E(v, torch.maximum(v - lo, hi - v) + 2 * U * hi)


def fma(a, x, b):
    """fmaf(a, x, b) with x exact (a tensor): one rounding."""
    v = a.v * x + b.v
    return E._r(v, a.e * x.abs() + b.e)


def _chan(t):
    return t.sum(dim=(0, 2, 3))


def _bc(t):
    return t.view(1, -1, 1, 1)


DEGENERATE = 1e-2       # relative width of the invstd interval beyond which a bound says nothing


def fwd_consts(raw, gamma, beta, rows_scale=1, chan=None):
    """Reference statistics of raw (NCHW float64) and the engine's BatchNorm constants (pa_bn_fwd_consts) with their bounds.
    rows_scale: capacity factor of the BatchNorm's BACKWARD partial rows (4 for bn3 of the up blocks); chan: the layer's channel count
    for sum_depth when raw holds only some of its channels (tests/test_bn_exact_cpu.py)."""
    n = raw.shape[0] * raw.shape[2] * raw.shape[3]
    chan = chan or raw.shape[1]
    D = sum_depth(n, chan, 1)
    S1 = E(_chan(raw), D * U * _chan(raw.abs()))
    S2 = E(_chan(raw * raw), D * U * _chan(raw * raw))
    mu = S1 / n
    var = S2 / n - mu * mu
    mu_ref = _chan(raw) / n
    var_ref = _chan((raw - _bc(mu_ref)) ** 2) / n                    # two-pass in float64: the reference's biased variance
    var = E(var_ref, var.e)
    inv = (var + E(*EPS32)).rsqrt()
    scale = E(gamma) * inv
    shift = E(beta) - mu * scale
    return dict(n=n, mu=mu, var=var, inv=inv, scale=scale, shift=shift, S1=S1, S2=S2, Db=sum_depth(n, chan, rows_scale),
                degenerate=float((inv.e / inv.v).max()))


def _ratio(got, ref, bound):
    d = (got.double() - ref).abs()
    return float((d / bound.clamp_min(1e-300)).max())


def check_forward(raw, val, k):
    """val (view 0) = relu(gamma (raw - mean) / sqrt(var + eps) + beta) per element."""
    pre = fma(_bc_e(k['scale']), raw, _bc_e(k['shift']))
    return _ratio(val, pre.v.clamp_min(0), pre.e)


def _bc_e(a):
    return E(_bc(a.v), _bc(a.e))


def check_running(k, rm0, rv0, rm1, rv1):
    """running_mean / running_var after the step: momentum 0.1, UNBIASED variance (pa_bn_running)."""
    n = k['n']
    unb = k['var'] * E(torch.full_like(k['var'].v, float(n))) / (n - 1)
    em = E(*ONE_MINUS_MOM32) * E(rm0.double()) + E(*MOM32) * k['mu']
    ev = E(*ONE_MINUS_MOM32) * E(rv0.double()) + E(*MOM32) * unb
    return max(_ratio(rm1, em.v, em.e), _ratio(rv1, ev.v, ev.e))


def bwd_sums(raw, dz, k):
    """sum dz and sum dz * xhat (reference, float64) with the bounds of the engine's fp32 sums of dz and dz * (x - mean) * invstd."""
    D = k['Db']
    mu, inv = _bc_e(k['mu']), _bc_e(k['inv'])
    xc = raw - mu.v
    T1 = E(_chan(dz), D * U * _chan(dz.abs()))
    # |(x - mean_e) invstd_e - (x - mean) invstd| <= e_mu (inv + e_inv) + |x - mean| e_inv; then the roundings of either form: three per
    # term or per row (products, the row's subtraction and scaling) and D in the sums, all on values <= |dz| (|x - mean| + 2 |mean| + e_mu)
    adz = dz.abs()
    e2 = _chan(adz * (mu.e * (inv.v + inv.e) + xc.abs() * inv.e)) + \
        (D + 3) * U * _chan(adz * (xc.abs() + 2 * mu.v.abs() + mu.e) * (inv.v + inv.e))
    T2 = E(_chan(dz * xc * inv.v), e2)
    return T1, T2


def check_param_grads(T1, T2, dgamma, dbeta):
    return max(_ratio(dbeta, T1.v, T1.e), _ratio(dgamma, T2.v, T2.e))


def check_backward(raw, dz, dx, k, T1, T2):
    """dx (view 3) = gamma invstd (dz - mean(dz) - xhat mean(dz xhat)) per element (pa_bn_bwd_consts, then fmaf(kA, dz, fmaf(kB, x, kC)))."""
    n = k['n']
    s, inv, mu = k['scale'], k['inv'], k['mu']
    b = (-s * inv * T2) / n
    kC = (-s * T1) / n - b * mu
    inner = fma(_bc_e(b), raw, _bc_e(kC))
    out = fma(_bc_e(s), dz, inner)
    xhat = (raw - _bc(mu.v)) * _bc(inv.v)
    ref = _bc(s.v) * (dz - _bc(T1.v / n) - xhat * _bc(T2.v / n))
    return _ratio(dx, ref, out.e)


def check_eval(raw, val, gamma, beta, rm, rv):
    """eval mode: relu(gamma (raw - running_mean) / sqrt(running_var + eps) + beta) (bn_eval_kernel, then the BNRELU load)."""
    s = E(gamma.double()) * (E(rv.double()) + E(*EPS32)).rsqrt()
    sh = E(beta.double()) - E(rm.double()) * s
    pre = fma(_bc_e(s), raw, _bc_e(sh))
    ref = (_bc(gamma.double()) * (raw - _bc(rm.double())) / _bc((rv.double() + EPS).sqrt()) + _bc(beta.double())).clamp_min(0)
    return _ratio(val, ref, pre.e)


# ---- bit-exact checks: the number of elements that differ
def _mismatch(got, exp):
    return int((got != exp).sum())


def rnd(x, dtype):
    return x.to(dtype).float()


def check_pool(val_in, pooled, dtype):
    """pooled = the 2 x 2 maximum of the (BatchNorm+ReLU-applied, fp32) input, rounded once to the storage type."""
    return _mismatch(pooled, rnd(F.max_pool2d(val_in.float(), 2, 2), dtype))


def _win(x):
    """the four pixels of every 2 x 2 window in scan order: top-left, top-right, bottom-left, bottom-right"""
    return torch.stack([x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]], 0)


def _unwin(w):
    out = torch.zeros(w.shape[1], w.shape[2], 2 * w.shape[3], 2 * w.shape[4], dtype=w.dtype, device=w.device)
    out[:, :, 0::2, 0::2], out[:, :, 0::2, 1::2], out[:, :, 1::2, 0::2], out[:, :, 1::2, 1::2] = w[0], w[1], w[2], w[3]
    return out


def route(g, val_in, last=False):
    """the pooled map's gradient g sent to the FIRST maximum (scan order) of every 2 x 2 window of val_in (fp32), 0 elsewhere; returns
    (routed, number of windows with two or more equal maxima).  last=True: the last maximum (a defect, tests/test_asn_exact_cpu.py)."""
    v = _win(val_in.float())
    eq = v == v.max(0).values
    order = eq.flip(0) if last else eq
    first = order & (order.cumsum(0) == 1)
    first = first.flip(0) if last else first
    return _unwin(first.float() * g.float().unsqueeze(0)), int((eq.sum(0) >= 2).sum())


def check_pool_bwd(dpooled, val_in, got, dtype, addend=None, masked=False):
    """got = round(route(d pooled) + addend) (one fp32 add, one rounding), times [val_in > 0] under a BatchNorm-backward epilogue.
    Returns (differing elements, tied windows)."""
    r, ties = route(dpooled, val_in)
    if addend is not None:
        r = rnd(r + addend.float(), dtype)
    if masked:
        r = r * (val_in > 0).float()
    return _mismatch(got, r), ties


def up2(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def check_merge_fwd(val_up, val_skip, merged, dtype):
    """merged = round(up2(up) + skip), the sum in fp32."""
    return _mismatch(merged, rnd(up2(val_up.float()) + val_skip.float(), dtype))


def sum2x2(d):
    """((top-left + top-right) + bottom-left) + bottom-right in fp32 (the fused epilogue's and the streaming kernels' order)."""
    d = d.float()
    return ((d[:, :, 0::2, 0::2] + d[:, :, 0::2, 1::2]) + d[:, :, 1::2, 0::2]) + d[:, :, 1::2, 1::2]


def check_merge_bwd(dmerged, val_up, val_skip, dup, dskip, dtype):
    """d up = round(2 x 2 sum of d merged) masked by up > 0; d skip = d merged masked by skip > 0."""
    e_up = rnd(sum2x2(dmerged), dtype) * (val_up > 0).float()
    e_sk = dmerged.float() * (val_skip > 0).float()
    return _mismatch(dup, e_up) + _mismatch(dskip, e_sk)


# ---- the occlusion branch (cell_mask_kernel, elementwise.hip; Hourglass::encode / decode / bwd under Net::drop_mask): the skip and neck
# outputs enter the decoder through copies multiplied by the [B][1][4][4] cell mask.  A product with 0 / 1 is exact, so all of it is
# bit for bit.
def up4(M, H):
    """the cell mask repeated to an H x H map (nearest): cell (y // (H / 4), x // (H / 4))"""
    return M.float().repeat_interleave(H // 4, dim=2).repeat_interleave(H // 4, dim=3)


def check_mask_fwd(val, M, masked, dtype):
    """masked = round(value of the tensor) * up4(M)."""
    return _mismatch(masked, rnd(val.float(), dtype) * up4(M, val.shape[2]))


def check_merge_bwd_masked(dmerged, val_up, dup, dmasked, dtype):
    """the upsample-add backward with a masked copy as its skip operand: d up as in check_merge_bwd; the copy is a plain tensor (no
    BatchNorm, no ReLU mask of its own): its gradient is d merged itself."""
    return _mismatch(dup, rnd(sum2x2(dmerged), dtype) * (val_up > 0).float()) + _mismatch(dmasked, dmerged.float())


def check_mask_bwd(dmasked, M, val, dgot):
    """d x = d (masked x) * up4(M) * [x > 0]: the cell mask's backward launch, through the ReLU mask of x's own pending BatchNorm."""
    return _mismatch(dgot, dmasked.float() * up4(M, val.shape[2]) * (val > 0).float())


# ---------------------------------------------------------------------------------------------------------------------------------
# the legs (GPU)
def bn_sites(stacks):
    """(parameter prefix of the BatchNorm, debug-hook name of the tensor it normalises) for every BatchNorm of the pose net."""
    blocks = [('residual1.', 'res1'), ('residual2.', 'res2'), ('residual3.', 'res3')]
    for i in range(stacks):
        for k in (1, 2, 3, 4):
            for kind in ('skip', 'down', 'up'):
                blocks.append(('hg.%d.%s%d.0.' % (i, kind, k), 'hg%d.%s%d' % (i, kind, k)))
        blocks.append(('hg.%d.neck.0.' % i, 'hg%d.neck' % i))
        blocks.append(('post_res.%d.0.' % i, 'post%d' % i))
    sites = [('bn1', 'stem')]
    for p, t in blocks:
        sites += [(p + 'bn1', t + '.x1'), (p + 'bn2', t + '.x2'), (p + 'bn3', t)]
    return sites + [('linear.%d.1' % i, 'lin%d' % i) for i in range(stacks)]


def pool_sites(stacks):
    """(pool output, its input) for pool0 and every hourglass pool."""
    s = [('pool0', 'res1')]
    for i in range(stacks):
        s += [('hg%d.pool%d' % (i, k), 'xin%d' % i if k == 1 else 'hg%d.down%d' % (i, k - 1)) for k in (1, 2, 3, 4)]
    return s


# Names whose buffers do not hold their value at the end of the step (arena reuse) and are therefore not checked: none -- every
# activation and gradient the hook names has storage of its own (Net::new_act).  A name added here needs its reason next to it.
NOT_HELD = {}


class Probe(object):
    def __init__(self, net):
        import ctypes
        from pose_adv_aug_amd._lib import lib, check, ptr
        self.C, self.lib, self.check, self.ptr = ctypes, lib(), check, ptr
        self.h = net._net(net._last_B)
        self.fn = self.lib.pa_hg_debug_tensor

    def has(self, name, view):
        shp = (self.C.c_int * 4)()
        return self.fn(self.h, name.encode(), view, None, shp) == 0

    def get(self, name, view):
        assert name not in NOT_HELD, name
        shp = (self.C.c_int * 4)()
        self.check(self.fn(self.h, name.encode(), view, None, shp))
        out = torch.empty(tuple(shp), device='cuda')
        self.check(self.fn(self.h, name.encode(), view, self.ptr(out), shp))
        return out


class AsnProbe(Probe):
    """the same views of the agent's tensors (pa_asn_debug_tensor: in0..4, pa0..3, merge0..3, deep0..2, .x1 / .x2)"""
    def __init__(self, agent):
        Probe.__init__(self, agent)
        self.fn = self.lib.pa_asn_debug_tensor


KINDS = ('bn forward', 'running stats', 'beta/gamma grads', 'bn backward', 'stored bn backward', 'eval forward', 'pool forward',
         'merge forward', 'merge backward', 'degenerate bound', 'pool backward', 'mask forward')


def make_note(worst, fails):
    def note(kind, what, r, bit=False):
        worst[kind] = max(worst[kind], r)
        if (r != 0) if bit else not (r <= 1.0):          # ('degenerate bound': width / DEGENERATE, the same rule)
            fails.append((kind, what, r))
    return note


def check_bn_site(P, pre, name, sd, before, grads, dtype, note, stored, rows_scale=1):
    """every check of ONE BatchNorm after a training step.  P: probe of the net that owns the tensor `name`; pre: its parameter prefix
    in sd (after the step) / before (the running estimates before it) / grads; stored: counters of the blocks that stored dz2 / dz3."""
    raw = P.get(name, 2).double()
    gamma, beta = sd[pre + '.weight'].double(), sd[pre + '.bias'].double()
    k = fwd_consts(raw, gamma, beta, rows_scale=rows_scale)
    note('degenerate bound', pre, k['degenerate'] / DEGENERATE)
    note('bn forward', name, check_forward(raw, P.get(name, 0), k))
    note('running stats', pre, check_running(k, before[pre + '.running_mean'], before[pre + '.running_var'],
                                            sd[pre + '.running_mean'], sd[pre + '.running_var']))
    dz = P.get(name, 1).double()
    T1, T2 = bwd_sums(raw, dz, k)
    note('beta/gamma grads', pre, check_param_grads(T1, T2, grads[pre + '.weight'], grads[pre + '.bias']))
    dx = P.get(name, 3)
    note('bn backward', name, check_backward(raw, dz, dx, k, T1, T2))
    if P.has(name, 4):
        stored['.x2' if name.endswith('.x2') else ''] += 1
        note('stored bn backward', name, _mismatch(P.get(name, 4), rnd(dx, dtype)), bit=True)


def check_bn_eval_site(P, pre, name, sd, note):
    """eval mode: view 0 of the tensor against the running estimates in sd"""
    note('eval forward', name, check_eval(P.get(name, 2).double(), P.get(name, 0), sd[pre + '.weight'], sd[pre + '.bias'],
                                          sd[pre + '.running_mean'], sd[pre + '.running_var']))


def run_leg(stacks, chan, B, res, seed, log=print, stored_expected=('.x2', ''), history='fresh', masks=None):
    """One training step (loss_and_backward, default multi-stream mode, as bench.py runs it) behind `history` (tests/exact_history.py:
    'fresh' = the first step after the bind), then every check.  Returns {kind: worst error / bound (bit-exact kinds: differing
    elements)} and the list of failures.  stored_expected: the inner tensors ('.x2': dz2) and block outputs ('': dz3) of which at
    least one block must have stored its BatchNorm-backward gradient.  masks (a seed): the checked step runs with occlusion masks
    (tests/exact_history.py); the masked copies, the merges over them and the cell mask's backward launches are then checked bit for
    bit, and check_bn_site over skip<k>.bn3 / neck.bn3 is the check of cell_mask_kernel's statistics epilogue (their backward sums
    come from it)."""
    from pose_adv_aug_amd._lib import act_dtype
    from tests import exact_history
    assert stacks <= 9, 'stack indexes are read as one character (int(out[2]) below, w[3] - \'0\' in pa_hg_debug_tensor)'
    dtype = act_dtype()
    sites = bn_sites(stacks)
    S = exact_history.pose_step(stacks, chan, B, res, seed, history, masks=masks)
    net, before, img, grads = S.net, S.before, S.img, S.grads
    sd = net.state_dict()
    assert sorted(p for p, _ in sites) == sorted(k[:-len('.running_mean')] for k in sd if k.endswith('.running_mean')), \
        'bn_sites must name every BatchNorm of the net'
    P = Probe(net)
    worst = dict((k, 0.0) for k in KINDS)
    fails = []
    note = make_note(worst, fails)
    stored = {'.x2': 0, '': 0}
    for pre, name in sites:
        up_bn3 = '.up' in name and not name.endswith(('.x1', '.x2'))
        check_bn_site(P, pre, name, sd, before, grads, dtype, note, stored, rows_scale=4 if up_bn3 else 1)
    # (a leg that expects a kind must have met it: the check must not go quiet because the kernels stopped storing)
    for suf, cnt in stored.items():
        if cnt == 0 and suf in stored_expected:
            fails.append(('stored bn backward', 'no block stored its dz%s' % ('2' if suf else '3'), 0))
    ties = 0
    middle = 0          # middle stacks met: pool 1 over a plain xin<i> (no pending BatchNorm) with a nonzero addend d xin<i+1>
    for out, src in pool_sites(stacks):
        vin = P.get(src, 0)
        note('pool forward', out, check_pool(vin, P.get(out, 0), dtype), bit=True)
        # pool backward (module docstring): pool0 writes d res1 through res1's BatchNorm-backward epilogue (view 1: the masked gradient);
        # hourglass pool k writes poolgrad<k>, with d xin<i+1> added for k = 1 of an inner stack
        if out == 'pool0':
            r, n = check_pool_bwd(P.get(out, 1), vin, P.get(src, 1), dtype, masked=True)
        else:
            i, k = int(out[2]), int(out[-1])
            add = P.get('xin%d' % (i + 1), 1) if (k == 1 and i + 1 < stacks) else None
            r, n = check_pool_bwd(P.get(out, 1), vin, P.get('hg%d.poolgrad%d' % (i, k), 2), dtype, addend=add)
            if add is not None and i >= 1 and bool((add != 0).any()):
                middle += 1
        note('pool backward', out, r, bit=True)
        ties += n
        del vin
    if ties == 0:
        fails.append(('pool backward', 'no 2 x 2 window of this leg had tied maxima: first-maximum routing was not tested', 0))
    if middle != max(stacks - 2, 0):
        fails.append(('pool backward', '%d of %d middle stacks had a nonzero addend over a plain input' % (middle, stacks - 2), 0))
    M = S.masks
    changed = leaked = 0        # elements the masks zeroed in the forward pass; nonzero gradient elements inside a dropped cell
    for i in range(stacks):
        for k in (1, 2, 3, 4):
            m, up, sk = 'hg%d.merge%d' % (i, k), 'hg%d.up%d' % (i, k), 'hg%d.skip%d' % (i, k)
            vu, vs = P.get(up, 0), P.get(sk, 0)
            if M is None:
                note('merge forward', m, check_merge_fwd(vu, vs, P.get(m, 0), dtype), bit=True)
                note('merge backward', m, check_merge_bwd(P.get(m, 1), vu, vs, P.get(up, 1), P.get(sk, 1), dtype), bit=True)
                continue
            # the decoder reads maskedskip<k> in place of skip<k> (Hourglass::decode); in the backward pass the upsample-add writes the
            # copy's plain gradient and the cell mask's launch turns it into d skip<k> (Hourglass::bwd, net.hip:773-775)
            ms = 'hg%d.maskedskip%d' % (i, k)
            vm, dm, dsk = P.get(ms, 0), P.get(ms, 1), P.get(sk, 1)
            note('mask forward', ms, check_mask_fwd(vs, M, vm, dtype), bit=True)
            note('merge forward', m, check_merge_fwd(vu, vm, P.get(m, 0), dtype), bit=True)
            note('merge backward', m, check_merge_bwd_masked(P.get(m, 1), vu, P.get(up, 1), dm, dtype), bit=True)
            note('merge backward', sk, check_mask_bwd(dm, M, vs, dsk), bit=True)
            changed += _mismatch(vm, rnd(vs, dtype))
            leaked += int((dsk * (1 - up4(M, dsk.shape[2])) != 0).sum())
        if M is not None:
            nk, mn = 'hg%d.neck' % i, 'hg%d.maskedneck' % i
            vn = P.get(nk, 0)
            note('mask forward', mn, check_mask_fwd(vn, M, P.get(mn, 0), dtype), bit=True)
            note('merge backward', nk, check_mask_bwd(P.get(mn, 1), M, vn, P.get(nk, 1)), bit=True)
    # (a masked leg must have been masked: the checks above compare with the masks applied and would also pass on an all-ones mask)
    if M is not None and changed == 0:
        fails.append(('mask forward', 'no maskedskip differs from its skip tensor', 0))
    if leaked:
        fails.append(('merge backward', 'gradient of a skip tensor inside a dropped cell', leaked))
    # eval mode: a forward pass with the running estimates this step left
    net.eval()
    net(img)
    torch.cuda.synchronize()
    for pre, name in sites:
        check_bn_eval_site(P, pre, name, sd, note)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('bn_exact %s %s stacks %d chan %d B %d res %d: worst error / bound (bit-exact kinds: differing elements): %s'
            % ('fp16' if dtype == torch.float16 else 'bf16', history + (' masked' if M is not None else ''), stacks, chan, B, res,
               ', '.join('%s %.3g' % (k, worst[k]) for k in KINDS)) + '; stored dz2 / dz3 checked in %d / %d blocks'
            % (stored['.x2'], stored['']) + '; %d tied pool windows' % ties)
    return worst, fails


def _child_kw(args):
    """the optional arguments of the child-process entry points behind the five numbers: the history, then the seed of the masks"""
    kw = {'history': args[0]} if args else {}
    if len(args) > 1:
        kw['masks'] = int(args[1])
    return kw


def _child_stored(args):
    """(the arguments without it, run_leg's stored_expected or None) of an optional 'stored=x2' / 'stored=x2,x3' / 'stored=' argument:
    the kinds a leg expects some block to have stored (x2: dz2, x3: dz3), for the sizes at which no launch stores one of them"""
    rest = [a for a in args if not a.startswith('stored=')]
    opt = [a[len('stored='):] for a in args if a.startswith('stored=')]
    if not opt:
        return rest, None
    kinds = [k for k in opt[-1].split(',') if k]
    assert all(k in ('x2', 'x3') for k in kinds), opt
    return rest, tuple({'x2': '.x2', 'x3': ''}[k] for k in kinds)


if __name__ == '__main__':          # the fp16 legs: tests/test_gpu_bn_exact.py runs this with POSEADV_DTYPE=fp16
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pose_adv_aug_amd._lib import lib as _l
    assert _l().pa_dtype() == 1, 'run with POSEADV_DTYPE=fp16'
    _rest, _stored = _child_stored(sys.argv[6:])
    _kw = _child_kw(_rest)
    if _stored is not None:
        _kw['stored_expected'] = _stored
    worst, fails = run_leg(*[int(a) for a in sys.argv[1:6]], log=lambda s: print(s, flush=True), **_kw)
    print('FAILURES %d %s' % (len(fails), fails[:20]))
    print('FP16 BN EXACT ' + ('PASSED' if not fails else 'FAILED'), flush=True)
    sys.exit(1 if fails else 0)
