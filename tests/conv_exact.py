"""Exact checks of the convolutions of the hourglass net: every conv's forward output, every data gradient (the inner tensors of every
residual block; every block input as mask * (conv1^T + the epilogue's one or two addends), the skip blocks' inputs with the pool's routed
gradient as the second addend; post, lin and in_conv's gradient of the heat maps), every weight gradient and every bias gradient, each
recomputed in float64 from the operands the engine itself used in ONE training step (pa_hg_debug_tensor views 0-4 and the head / pool
buffers it names, include/poseadv.h), and the same bounds over the standalone shapes of tests/test_gpu_conv.py.  That step is the first
one after the bind ('fresh') or one behind a history of optimizer steps (repacked weight copies), graph replays, eval-mode and unfinished
forwards, entered as bench.py enters its timed steps (tests/exact_history.py); the weights are those held immediately before it.

Why this is exact up to a derived bound.  Every conv prologue computes its operand in fp32 and rounds it ONCE to the storage type: the
BatchNorm+ReLU value fmaxf(fmaf(k0, raw, k1), 0) (view 0) or the BatchNorm-backward gradient fmaf(k0, p, fmaf(k1, q, k2)) (view 3); where
a data-gradient kernel stored that gradient for its later readers, view 4 is it (bit-equal to rnd(view 3): tests/bn_exact.py).  So
rnd(view 0), rnd(view 3) and the weights rounded to the storage type are exactly the MFMA operands.  Products of two bf16 or two fp16
values are exact in float64, so a float64 convolution of those operands is the exact result; the kernel may differ from it only by its
fp32 accumulation and the final rounding.

Rounding unit.  Vector-ALU adds and FMAs round to nearest even with u = 2^-24 (tests/bn_exact.py).  Inside one v_mfma_f32_16x16x32
(the only MFMA of the conv kernels, common.h PA_MFMA_16x16x32: K = 32) each of the 32 products and the add into the accumulator count as
one addition at 2u -- the ISA does not specify the internal order or rounding, so this bounds any of them.  Every addition below is
charged 2u.

Depth D: the most additions any product passes through.  The release kernels keep one accumulator per output element and chain the
MFMAs over the reduction (conv_igemm.hip:194/323, conv1x1_tile.hip:195, conv3x3_tile.hip:334/379, conv_wgrad.hip:195,
conv_wgrad_tile.hip:157/171, pose_ops.hip:137): no split of the reduction across waves.
  * forward and data gradient: D = 32 + ceil(K / 32) + A, where K = Cin * taps (Cout * taps for the data gradient) over the padded
    channel counts (multiples of 64; 256 for the stem's 7 x 7 x 4 patch) and A the epilogue adds (bias, add1, add2).  Nothing in it
    depends on the channel count beyond K: at chan 512 the generic kernel chains 16 MFMAs (K = 512) or 72 (the 3 x 3 layer, K = 2304)
    into the same single accumulator (conv_igemm.hip:194), whichever of its tiles <64,64> ... <128,128> the launch takes.
  * weight gradient: a split owns a contiguous (conv_wgrad.hip: steps of 64 / 128 pixels) or strided (conv_wgrad_tile.hip: tiles of
    128 pixels) share of the ceil(M / P) tiles of P <= 128 pixels, at most M / S + 2 P pixels, one MFMA per 32 of them; the slabs of the S
    splits are then chained in split order (wgrad_reduce.h; the stem's reducer: four slices of S / 4 plus three adds, stem_wgrad_reduce_kernel):
    D = 32 + ceil((M / S + 256) / 32) + S.
  * bias gradient (convs without a BatchNorm behind them): any tree over the <= M / S + 256 values of a split (per-thread column sums
    and their LDS sum, conv_wgrad_tile.hip:466, conv_wgrad.hip:222), then the chain over S: D = M / S + 256 + S.
  At the input resolutions 320 / 448 / 192 / 64 (re-derived for the shapes that leave the halo tiles; nothing changes): the 3 x 3 layers of
  the 10 x 10 / 14 x 14 maps run the generic kernel, whose chain of 9 * Cin / 32 MFMAs into one accumulator is the forward formula's (an
  M tile that wraps image rows changes which pixels a tile holds, not the reduction of any of them); the masked 8 x 8 tile of the 7 x 7 /
  5 x 5 / 3 x 3 / 1 x 1 maps chains all nine taps whether a tap meets a pixel or the zero halo (conv3x3_tile.hip:342-382), the same depth
  with zero terms.  The weight-gradient plans there are tile plans with a ragged last tile (1 * 56 * 56 pixels = 24.5 tiles of 128) and
  generic plans with S = 1 for M = 3 ... 49 pixels, less than one 32-pixel MFMA step: both inside the M / S + 2 P pixels of a split.
  S is the split count Net::layout_conv gives the layer: pa_wgrad_layer_splits over the layer's pa_wgrad_plan (csrc/wgrad_plan.h) -- the
  count of the layer launched alone (the tile kernels' where they take the shape, else the generic kernel's), replaced by the grouped
  count where the grouped kernel takes the layer, and 512 for the stem.  The plan is not exported: wgrad_plan() mirrors it for the
  release build, which reads no tuning variable (csrc/tuning.h); tests/test_gpu_conv_exact.py checks the mirror against the workspace
  sizes the library reports.  A shape no kernel takes raises instead of getting a default.

Per-element bound (16-bit storage output):  |got - ref| <= e + 1/2 ulp_T(|ref| + e),  e = 2u D (sum |a w| + |bias| + sum |addends|),
where sum |a w| is the float64 convolution of the absolute operands and ulp_T the storage type's ulp at that magnitude (bf16: 2^-7
relative; fp16: 2^-10 relative with the subnormal floor 2^-24).  An addend the engine rounded to the storage type before the sum without a
view that exposes it (the adapter's output) enters with its own e and one more half ulp.  fp32 outputs (weight and bias gradients, the
heat maps) use u |ref| in place of the half ulp.  A masked data gradient (BatchNorm-backward epilogue) is mask * (that bound), the mask
taken from view 0 of the tensor (the epilogue's fmaf(scale, raw, shift) > 0 is the same fp32 expression).

Reference.  Float64 on the device of the operands (the GPU legs: torch's fp64 GEMM; the CPU test: <= 16 threads), one matrix product
per tap (conv64 and friends below).  Its own error is below 2^-53 * K * sum |a w|, nine orders below every bound here.

A bound is reported as 'degenerate' (a failure of its own) when it no longer says anything: more than half of the elements of a check
have a bound of at least 1 % of the sum of the absolute values of their terms (sum |a w| + |bias| + sum |addends|), so that losing a
hundredth of the terms could pass.  (Relative to the result itself it cannot be judged: the bias gradients of forth_conv / in_conv sum a
gradient whose per-channel sums nearly cancel -- it has passed through BatchNorm backward passes -- to values far below any fp32 sum's
error.)"""
import collections
import os
import sys

import torch
import torch.nn.functional as F

U = 2.0 ** -24
K_MFMA = 32
TILE_PIX = 128          # the largest pixel tile any weight-gradient kernel walks (conv_wgrad_tile.hip: 128; conv_wgrad.hip: 64 / 128)


def rnd(x, dtype):
    return x.to(dtype).to(x.dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references: one matrix product per tap, NHWC inside
def _taps(x, k, stride, pad, Ho, Wo):
    """x NCHW -> (ky, kx, NHWC view of the input pixels tap (ky, kx) reads for every output pixel)."""
    xp = F.pad(x, (pad, pad, pad, pad)).permute(0, 2, 3, 1)
    for ky in range(k):
        for kx in range(k):
            yield ky, kx, xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :]


def conv64(x, w, stride=1, pad=None):
    """conv2d(x, w) in float64 (no bias)."""
    k = w.shape[2]
    pad = k // 2 if pad is None else pad
    B, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x, w = x.double(), w.double()
    out = torch.zeros(B, Ho, Wo, w.shape[0], dtype=torch.float64, device=x.device)
    for ky, kx, xs in _taps(x, k, stride, pad, Ho, Wo):
        out += xs.reshape(-1, C).matmul(w[:, :, ky, kx].t()).view(B, Ho, Wo, -1)
    return out.permute(0, 3, 1, 2)


def dgrad64(dy, w):
    """data gradient of a stride-1 'same' conv: conv_transpose2d(dy, w)."""
    return conv64(dy, w.flip(2, 3).transpose(0, 1))


def wgrad64(x, dy, k, stride=1, pad=None):
    """weight gradient sum over pixels of dy (x) x, PyTorch layout [Cout][Cin][k][k]."""
    pad = k // 2 if pad is None else pad
    B, C = x.shape[:2]
    Ho, Wo = dy.shape[2:]
    x = x.double()
    g = dy.double().permute(0, 2, 3, 1).reshape(-1, dy.shape[1])
    out = torch.zeros(dy.shape[1], C, k, k, dtype=torch.float64, device=x.device)
    for ky, kx, xs in _taps(x, k, stride, pad, Ho, Wo):
        out[:, :, ky, kx] = g.t().matmul(xs.reshape(-1, C))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# depths (module docstring)
def depth_fwd(K, adds):
    return K_MFMA + -(-K // K_MFMA) + adds


def depth_wgrad(M, S):
    return K_MFMA + -(-(-(-M // S) + 2 * TILE_PIX) // K_MFMA) + S


def depth_bgrad(M, S):
    return -(-M // S) + 2 * TILE_PIX + S


def pad64(c):
    return (c + 63) // 64 * 64


# ---- split counts of the release build (not exported): pa_wgrad_plan and pa_wgrad_layer_splits of csrc/wgrad_plan.h, field for field
WgradPlan = collections.namedtuple('WgradPlan', 'path nb cb ntiles splits group_splits group_kind blocks')


def _balanced(ntiles, s):
    """pa_wgrad_balanced"""
    per = -(-ntiles // s)
    return -(-ntiles // per)


def _has_kernel(Cin, Cout, taps):
    return taps in (1, 9) and Cin % 64 == 0 and Cout % 64 == 0


def wgrad_plan(B, H, W, Cin, Cout, taps, stem=False):
    """pa_wgrad_plan (over pa_wgrad_generic_plan) at the release values of csrc/tuning.h.  H <= 0 or W <= 0: spatial shape unknown, B
    counts the pixels.  group_kind: the name of the wgrad_group_kernel body, None for -1."""
    if not _has_kernel(Cin, Cout, taps):
        raise ValueError('no weight-gradient kernel for Cin %d Cout %d taps %d' % (Cin, Cout, taps))
    shaped = H > 0 and W > 0
    M = B * H * W if shaped else B
    # pa_wgrad_generic_plan
    nb, cb = (128 if Cout % 128 == 0 else 64), (128 if Cin % 128 == 0 else 64)
    blocks = (Cout // nb) * (taps * Cin // cb)
    ms = 128 if nb + cb <= 128 else 64
    ntiles = -(-M // ms)
    s = (-(-(1024 if taps == 9 else 512) // blocks) + 7) & ~7
    p = WgradPlan('stem generic' if stem else 'generic', nb, cb, ntiles, max(min(s, ntiles), 1), 0, None, blocks)
    if stem:
        p = p._replace(nb=64, cb=128, ntiles=-(-M // 64), blocks=2)
        ntiles = -(-M // 128)
        if 512 <= ntiles:
            p = p._replace(splits=512)
        return p._replace(path='stem tile', nb=64, cb=256, ntiles=ntiles, blocks=1)
    if not shaped:
        return p
    if taps == 9:
        if H % 8 or W % 16:
            return p
        nb = cb = 64
        ntiles = B * (H // 8) * (W // 16)
        if ntiles < 48:
            return p
    else:
        ntiles = -(-M // 128)
        if ntiles < 3:
            return p
    blocks = (Cout // nb) * (Cin // cb)
    splits = _balanced(ntiles, min(max(256 // blocks, 1), ntiles))
    s = 64 // blocks
    minper = 4 if taps == 9 else 2
    if s * minper > ntiles:
        s = ntiles // minper
    kind = 'PA_WGK_9_44' if taps == 9 else 'PA_WGK_1_%d%d' % (nb // 32, cb // 32)
    return WgradPlan('tile', nb, cb, ntiles, splits, _balanced(ntiles, max(s, 1)), kind, blocks)


def wgrad_splits(M, H, W, Cin, Cout, taps):
    """PaWgradPlan::splits, the count of the layer launched alone, as Net::layout_conv asks for it: M pixels, a map only where it divides
    them."""
    shaped = H > 0 and W > 0 and M % (H * W) == 0
    return (wgrad_plan(M // (H * W), H, W, Cin, Cout, taps) if shaped else wgrad_plan(M, 0, 0, Cin, Cout, taps)).splits


def group_splits(B, H, W, Cin, Cout, taps):
    """PaWgradPlan::group_splits; 0: the grouped kernel does not take the shape."""
    return wgrad_plan(B, H, W, Cin, Cout, taps).group_splits if _has_kernel(Cin, Cout, taps) else 0


def layer_splits(B, H, W, Cin, Cout, k):
    """S of a layer of the net (pa_wgrad_layer_splits as Net::layout_conv calls it, the batch known); Cin / Cout real, padded here."""
    if k == 7:
        return wgrad_plan(B, H, W, 256, pad64(Cout), 1, stem=True).splits
    p = wgrad_plan(B, H, W, pad64(Cin), pad64(Cout), k * k)
    return p.group_splits if p.group_splits > 0 else p.splits


# ---------------------------------------------------------------------------------------------------------------------------------
# bounds and checks
_P = {torch.bfloat16: (7, 2.0 ** -133), torch.float16: (10, 2.0 ** -24)}


def ulp(v, dtype):
    """the storage type's ulp at magnitude |v| (float64 tensor)."""
    p, floor = _P[dtype]
    a = v.abs()
    _, ex = torch.frexp(a)                      # |v| = m 2^ex, m in [0.5, 1); frexp(0) = (0, 0): zero takes the floor
    return torch.where(a == 0, torch.full_like(a, floor), torch.clamp(torch.ldexp(torch.ones_like(a), ex - 1 - p), min=floor))


def bound16(ref, e, dtype):
    return e + 0.5 * ulp(ref.abs() + e, dtype)


def bound32(ref, e):
    return e + U * (ref.abs() + e)


def ratio(got, ref, bound):
    """worst |got - ref| / bound; inf where got is not finite."""
    d = (got.double() - ref).abs()
    r = d / bound.clamp_min(1e-300)
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float('inf')))
    return float(r.max()) if r.numel() else 0.0


def degenerate(mag, bound):
    """fraction of the elements (with any nonzero term) whose bound is at least 1 % of sum |terms| (module docstring)."""
    nz = mag > 0
    n = int(nz.sum())
    return float((bound[nz] >= 0.01 * mag[nz]).sum()) / n if n else 0.0


DEGENERATE = 0.5


class Term(object):
    """a float64 value with the bound e of the fp32 evaluation that produced it (before any rounding to the storage type)."""
    def __init__(self, v, e, mag=None):
        self.v, self.e, self.mag = v, e, (v.abs() if mag is None else mag)


def conv_term(x, w, k_pad, bias=None, addends=(), stride=1, pad=None):
    """forward conv + bias + addends (Terms or exact tensors) as the kernel's fp32 accumulation: value and e (module docstring).
    k_pad: the reduction length over the padded channels (Cin_pad * taps)."""
    v = conv64(x, w, stride, pad)
    mag = conv64(x.abs(), w.abs(), stride, pad)
    e_in = torch.zeros_like(v)
    adds = 0
    if bias is not None:
        v = v + bias.double().view(1, -1, 1, 1)
        mag = mag + bias.double().abs().view(1, -1, 1, 1)
        adds += 1
    for a in addends:
        if isinstance(a, Term):
            v = v + a.v
            mag = mag + a.v.abs() + a.e
            e_in = e_in + a.e
        else:
            v = v + a.double()
            mag = mag + a.double().abs()
        adds += 1
    return Term(v, 2 * U * depth_fwd(k_pad, adds) * mag + e_in, mag)


def dgrad_term(dy, w, k_pad, addends=()):
    """data gradient (stride 1, 'same') + addends: conv_term over the flipped, transposed weights.  k_pad: Cout_pad * taps."""
    return conv_term(dy, w.flip(2, 3).transpose(0, 1), k_pad, None, addends)


def rounded(t, dtype):
    """a Term rounded to the storage type (not observed): one more half ulp on its bound."""
    return Term(t.v, bound16(t.v, t.e, dtype), t.mag)


def check16(got, t, dtype, mask=None):
    """(worst ratio, degenerate fraction) of a storage-type output against a Term; mask: a BatchNorm-backward epilogue's ReLU mask."""
    b = bound16(t.v, t.e, dtype)
    ref, mag = t.v, t.mag
    if mask is not None:
        ref, b, mag = ref * mask, b * mask, mag * mask
    return ratio(got, ref, b), degenerate(mag, b)


def check32(got, t):
    b = bound32(t.v, t.e)
    return ratio(got, t.v, b), degenerate(t.mag, b)


def wgrad_check(got, x, dy, k, S, stride=1, pad=None):
    """weight gradient (fp32, PyTorch layout) of storage-type operands x, dy over S splits."""
    M = dy.shape[0] * dy.shape[2] * dy.shape[3]
    mag = wgrad64(x.abs(), dy.abs(), k, stride, pad)
    return check32(got, Term(wgrad64(x, dy, k, stride, pad), 2 * U * depth_wgrad(M, S) * mag, mag))


def bgrad_check(got, dy, S):
    M = dy.shape[0] * dy.shape[2] * dy.shape[3]
    mag = dy.double().abs().sum(dim=(0, 2, 3))
    return check32(got, Term(dy.double().sum(dim=(0, 2, 3)), 2 * U * depth_bgrad(M, S) * mag, mag))


# ---------------------------------------------------------------------------------------------------------------------------------
# the net (GPU legs)
def block_sites(stacks, masked=False):
    """(parameter prefix of the residual block, debug-hook name of its output, hook name of its input, has adapter), every block of the
    pose net, wired as Net::forward_pose_body / Hourglass::encode / decode (net.hip:703-742, 912-942).  masked: the step ran with
    occlusion masks -- up4 reads maskedneck, the neck's output times the cell mask (a plain tensor); no other block's input changes
    (the skip blocks read xin / down, up3..1 and post read merges, which then hold the masked skip tensors)."""
    s = [('residual1.', 'res1', 'stem', True), ('residual2.', 'res2', 'pool0', False), ('residual3.', 'res3', 'res2', True)]
    for i in range(stacks):
        for k in (1, 2, 3, 4):
            s.append(('hg.%d.skip%d.0.' % (i, k), 'hg%d.skip%d' % (i, k), 'xin%d' % i if k == 1 else 'hg%d.down%d' % (i, k - 1), False))
            s.append(('hg.%d.down%d.0.' % (i, k), 'hg%d.down%d' % (i, k), 'hg%d.pool%d' % (i, k), False))
            s.append(('hg.%d.up%d.0.' % (i, k), 'hg%d.up%d' % (i, k), ('hg%d.maskedneck' if masked else 'hg%d.neck') % i if k == 4 else 'hg%d.merge%d' % (i, k + 1), False))
        s.append(('hg.%d.neck.0.' % i, 'hg%d.neck' % i, 'hg%d.down4' % i, False))
        s.append(('post_res.%d.0.' % i, 'post%d' % i, 'hg%d.merge1' % i, False))
    return s


def conv_names(stacks):
    """every conv weight of the pose net, as the checks below name them."""
    n = ['conv1']
    for p, _, _, ad in block_sites(stacks):
        n += [p + 'conv1', p + 'conv2', p + 'conv3'] + ([p + 'adapter'] if ad else [])
    for i in range(stacks):
        n += ['linear.%d.0' % i, 'out_conv.%d' % i]
        if i + 1 < stacks:
            n += ['forth_conv.%d' % i, 'in_conv.%d' % i]
    return n


KINDS = ('conv forward', 'conv data gradient', 'weight gradient', 'bias gradient', 'zero bias gradient', 'degenerate bound', 'heat gradient',
         'loss')


class Checker(object):
    """The bookkeeping and the per-block checks of one leg over ONE net's parameters: sd0 (its state_dict before the step), grads (its
    named gradients after it), B.  The probes of the tensors are arguments of every check, so a block may read its input from another
    net (the agent's five input blocks read the pose net's features in place: tests/asn_exact.py)."""
    def __init__(self, sd0, grads, dtype, B):
        self.sd0, self.grads, self.dtype, self.B = sd0, grads, dtype, B
        self.worst = dict((k, 0.0) for k in KINDS)
        self.fails = []
        self.met = {'group': 0}
        self.checked = set()         # (conv, kind): what each conv's checks covered

    def W(self, n):
        return rnd(self.sd0[n + '.weight'].double(), self.dtype)

    def bias(self, n):
        return self.sd0[n + '.bias'].double()

    def note(self, kind, what, r_deg, convs=()):
        for c in convs:
            self.checked.add((c, 'bias' if kind.endswith('bias gradient') else kind))
        r, deg = r_deg
        self.worst[kind] = max(self.worst[kind], r)
        self.worst['degenerate bound'] = max(self.worst['degenerate bound'], deg / DEGENERATE)
        if not (r <= 1.0):
            self.fails.append((kind, what, r))
        if deg > DEGENERATE:
            self.fails.append(('degenerate bound', '%s %s' % (kind, what), deg))

    def grad_op(self, P, name):
        """the gradient operand the consumers of `name` read: view 4 where the step stored it, else rnd(view 3)."""
        return (P.get(name, 4) if P.has(name, 4) else rnd(P.get(name, 3), self.dtype)).double()

    def wg(self, conv, x, dy, k, H, stride=1, pad=None, has_bias=False):
        B, grads = self.B, self.grads
        S = layer_splits(B, H, H, x.shape[1], dy.shape[1], k)
        if k != 7 and group_splits(B, H, H, pad64(x.shape[1]), pad64(dy.shape[1]), k * k) > 0:
            self.met['group'] += 1
        self.note('weight gradient', conv, wgrad_check(grads[conv + '.weight'], x, dy, k, S, stride, pad), (conv,))
        if has_bias:
            self.note('bias gradient', conv, bgrad_check(grads[conv + '.bias'], dy, S), (conv,))
        else:
            z = grads[conv + '.bias']
            self.worst['zero bias gradient'] = max(self.worst['zero bias gradient'], float(z.abs().max()))
            self.checked.add((conv, 'bias'))
            if bool((z != 0).any()):
                self.fails.append(('zero bias gradient', conv, float(z.abs().max())))

    def block(self, p, out, Po, Pi, inp, input_grad=True, ad=False, add2=None, in_masked=True):
        """One residual block (Residual::fwd / bwd_a / bwd_b, net.hip:638-690): forward of conv1 / conv2 / conv3 (+ adapter), the inner data
        gradients, the weight gradients at the layer's split count, zero bias gradients, and -- input_grad -- the data gradient of the
        block's input.  p: parameter prefix; out: hook name of the output in probe Po; inp: hook name of the input in probe Pi;
        ad: the block has an adapter; add2: a second addend of the input's data gradient (the pool's routed gradient); in_masked: the
        input has a pending BatchNorm (its gradient is stored ReLU-masked).  input_grad=False (Residual::bwd with need_dx = false): the
        input belongs to another net and gets no gradient; the caller asserts that net's gradients stayed zero."""
        dtype, note, W, bias, wg = self.dtype, self.note, self.W, self.bias, self.wg
        grad_op = lambda n: self.grad_op(Po, n)
        sv0 = lambda n: rnd(Po.get(n, 0), dtype).double()
        cin = Pi.get(inp, 0).shape[1]
        H = Po.get(out, 2).shape[2]
        mid = Po.get(out + '.x1', 2).shape[1]
        xin = Pi.get(inp, 0).double()
        x_in = rnd(xin, dtype)
        t1 = conv_term(x_in, W(p + 'conv1'), pad64(cin), bias(p + 'conv1'))
        note('conv forward', p + 'conv1', check16(Po.get(out + '.x1', 2), t1, dtype), (p + 'conv1',))
        del t1
        x1v = sv0(out + '.x1')
        t2 = conv_term(x1v, W(p + 'conv2'), 9 * pad64(mid), bias(p + 'conv2'))
        note('conv forward', p + 'conv2', check16(Po.get(out + '.x2', 2), t2, dtype), (p + 'conv2',))
        del t2
        x2v = sv0(out + '.x2')
        if ad:      # x3 = conv3(x2) + b3 + adout, adout = rnd(adapter(in) + b_ad): not exposed, one more half ulp
            short = rounded(conv_term(x_in, W(p + 'adapter'), pad64(cin), bias(p + 'adapter')), dtype)
        else:       # the identity shortcut: the block input's fp32 value (the epilogue's BNRELU / plain load)
            short = xin
        t3 = conv_term(x2v, W(p + 'conv3'), pad64(mid), bias(p + 'conv3'), (short,))
        note('conv forward', p + 'conv3', check16(Po.get(out, 2), t3, dtype), (p + 'conv3',) + ((p + 'adapter',) if ad else ()))
        del t3, short
        # inner data gradients: one consumer each, masked by the ReLU of the tensor's own value
        g3 = grad_op(out)
        g2 = grad_op(out + '.x2')
        m2 = (Po.get(out + '.x2', 0) > 0).double()
        note('conv data gradient', p + 'conv3', check16(Po.get(out + '.x2', 1), dgrad_term(g3, W(p + 'conv3'), pad64(g3.shape[1])), dtype, m2),
             (p + 'conv3',))
        m1 = (Po.get(out + '.x1', 0) > 0).double()
        note('conv data gradient', p + 'conv2', check16(Po.get(out + '.x1', 1), dgrad_term(g2, W(p + 'conv2'), 9 * pad64(mid)), dtype, m1),
             (p + 'conv2',))
        g1 = grad_op(out + '.x1')
        wg(p + 'conv3', x2v, g3, 1, H)
        wg(p + 'conv2', x1v, g2, 3, H)
        wg(p + 'conv1', x_in, g1, 1, H)
        if ad:
            wg(p + 'adapter', x_in, g3, 1, H)
        if not input_grad:
            return
        # d in = mask * (conv1^T(g1) + add1 [+ add2]) (Residual::bwd_b, net.hip:678-690)
        if ad:      # add1 = adgrad = rnd(adapter^T(g3)), not exposed; residual1 / residual3 have no other reader of their input
            adds = (rounded(dgrad_term(g3, W(p + 'adapter'), pad64(g3.shape[1])), dtype),)
        else:       # add1: the x3 gradient as conv1's epilogue loads it, dz3 (view 4) or the LIN2 value in fp32 (view 3)
            adds = ((Po.get(out, 4) if Po.has(out, 4) else Po.get(out, 3)).double(),)
        if add2 is not None:
            adds += (add2.double(),)
        mask = (xin > 0).double() if in_masked else None
        note('conv data gradient', inp, check16(Pi.get(inp, 1), dgrad_term(g1, W(p + 'conv1'), pad64(mid), adds), dtype, mask),
             (p + 'conv1',) + ((p + 'adapter',) if ad else ()))


def loss_depth(M):
    """the most additions a squared difference passes through in head_fwd_kernel's loss (pose_ops.hip:107-166, the launch :173-178):
    a lane adds its 4 joints of every group it visits, groups = ceil(M / 16) strided over 4 waves of blocks = min(768, ceil(groups / 4))
    workgroups; 6 shuffle levels; 3 adds of the waves' sums; up to blocks - 1 atomic adds in any order."""
    groups = -(-M // 16)
    blocks = min(768, -(-groups // 4))
    return 4 * -(-groups // (4 * blocks)) + 6 + 3 + (blocks - 1)


def loss_check(got, heat, target):
    """one stack's MSE (fp32) against float64 over the returned fp32 heat maps: per term d = heat - target and d * d (two roundings, or
    one with the sum's fma), loss_depth additions, then the product with the fp32 1 / (M * 16) (two roundings).  All terms are >= 0."""
    from tests.bn_exact import E
    d2 = ((heat.double() - target.double()) ** 2).sum()
    M = heat.shape[0] * heat.shape[2] * heat.shape[3]
    s = E(d2, (loss_depth(M) + 3) * U * d2) * E(1.0 / (16.0 * M), U / (16.0 * M))
    return s, ratio(got.reshape(1), s.v.reshape(1), s.e.reshape(1))


def heat_grad_check(got, heat, target, gscale, add, dtype):
    """d heat (storage type) against 2 (heat - target) gscale (+ add): heat_grad_kernel pose_ops.hip:198-200 -- a subtraction, the exact
    doubling, the product with the fp32 gscale = grad_scale / (B * 16 * H * H) (itself one rounded division, net.hip:949), the add of
    in_conv's data gradient: three or four roundings, fewer where the compiler contracts the product and the add into one fma (a
    first-order bound over the separate operations admits both); then the half ulp of the storage type."""
    from tests.bn_exact import E
    g = (E(heat.double()) - E(target.double())) * E(torch.full_like(heat.double(), 2.0 * gscale), 2.0 * gscale * U)
    mag = 2.0 * gscale * (heat.double().abs() + target.double().abs())
    if add is not None:
        g = g + E(add.double())
        mag = mag + add.double().abs()
    return check16(got, Term(g.v, g.e, mag), dtype)


def run_leg(stacks, chan, B, res, seed, log=print, expect=(), history='fresh', masks=None):
    """One training step (loss_and_backward, default multi-stream mode) behind `history` (tests/exact_history.py: 'fresh' = the first
    step after the bind), then every check.  Returns {kind: worst error / bound} and the failures.  expect: weight-gradient split
    kinds this leg must meet ('group': a layer whose split count is the grouped kernel's).  masks (a seed): the checked step runs with
    occlusion masks (tests/exact_history.py)."""
    from pose_adv_aug_amd._lib import act_dtype, grad_scale
    from tests import exact_history, inputs
    from tests.bn_exact import Probe
    from tests.test_gpu_net import t
    assert stacks <= 9, 'stack indexes are read as one character (w[3] - \'0\' in pa_hg_debug_tensor)'
    dtype = act_dtype()
    S = exact_history.pose_step(stacks, chan, B, res, seed, history, masks=masks)
    net, sd0, img, pts_np, outs, loss_total, grads = S.net, S.sd0, S.img, S.pts_np, S.outs, S.loss_total, S.grads
    names = conv_names(stacks)
    assert sorted(names) == sorted(k[:-len('.weight')] for k in sd0 if k.endswith('.weight') and sd0[k].dim() == 4), \
        'conv_names must name every conv of the net'
    P = Probe(net)
    ck = Checker(sd0, grads, dtype, B)
    W, bias, note, wg, worst, fails, met, checked = ck.W, ck.bias, ck.note, ck.wg, ck.worst, ck.fails, ck.met, ck.checked
    grad_op = lambda n: ck.grad_op(P, n)
    v0 = lambda n: P.get(n, 0).double()
    sv0 = lambda n: rnd(P.get(n, 0), dtype).double()

    # ---- stem: 7 x 7 stride 2 over the image (rounded to the storage type by the layout converter), K = 7 x 7 x 4 padded to 256
    xs = rnd(img.double(), dtype)
    a0 = conv_term(xs, W('conv1'), 256, bias('conv1'), stride=2, pad=3)
    note('conv forward', 'conv1', check16(P.get('stem', 2), a0, dtype), ('conv1',))
    wg('conv1', xs, grad_op('stem'), 7, res // 2, stride=2, pad=3)
    del a0
    # ---- residual blocks (Residual::fwd / bwd_a, net.hip:638-687)
    # The input of skip block k of hourglass i (xin<i>, hg<i>.down<k-1>) also feeds max pool k: Hourglass::bwd routes the pool's
    # gradient back (plus, k = 1, d xin<i+1> from the next stack's forth_conv addend) into poolgrad[k] (net.hip:803-807, stored in the
    # storage type), and skip k's conv1 data gradient adds it as its SECOND addend (Residual::bwd_b, net.hip:687).  res1's output has
    # no conv reader (pool0 only): nothing to check here.  (That the pool routed correctly: tests/bn_exact.py 'pool backward'.)
    skip_k = dict([('xin%d' % i, (i, 1)) for i in range(stacks)] + [('hg%d.down%d' % (i, k), (i, k + 1)) for i in range(stacks) for k in (1, 2, 3)])
    # a pending BatchNorm (masked gradient): the stem and block outputs (xin0 is residual3's); not the pools, merges, xin<i>, i >= 1, or
    # the occlusion branch's maskedneck (d maskedneck = conv1^T + dz3 of up4 through a plain epilogue: no ReLU mask)
    has_bn = lambda n: not ('pool' in n or 'merge' in n or 'masked' in n or (n.startswith('xin') and n != 'xin0'))
    for p, out, inp, ad in block_sites(stacks, masked=S.masks is not None):
        add2 = P.get('hg%d.poolgrad%d' % skip_k[inp], 2) if inp in skip_k else None          # the pool's routed gradient
        ck.block(p, out, P, P, inp, True, ad, add2, has_bn(inp))
        del add2
    # ---- head (Net::forward_pose_body / backward_stack, net.hip:930-977)
    Hh = res // 4
    target = t(inputs.heatmaps_from_pts(pts_np, res=Hh)).cuda()
    loss_sum = None
    for i in range(stacks):
        lin = 'linear.%d.0' % i
        pv = sv0('post%d' % i)
        note('conv forward', lin, check16(P.get('lin%d' % i, 2), conv_term(pv, W(lin), chan, bias(lin)), dtype), (lin,))
        gl = grad_op('lin%d' % i)
        wg(lin, pv, gl, 1, Hh)
        # post<i>'s only reader is linear.i: d post = mask * linear^T(d lin)
        note('conv data gradient', 'post%d' % i, check16(P.get('post%d' % i, 1), dgrad_term(gl, W(lin), chan), dtype,
                                                          (P.get('post%d' % i, 0) > 0).double()), (lin,))
        del gl
        lv = sv0('lin%d' % i)
        oc = 'out_conv.%d' % i
        heat = conv_term(lv, W(oc), chan, bias(oc))                     # fp32 heat maps (the head kernel), then rnd for heat64
        note('conv forward', oc, check32(outs[i].double(), heat), (oc,))
        note('conv forward', oc + ' (stored)', check16(P.get('heat%d' % i, 2)[:, :16], heat, dtype), (oc,))
        dh64 = P.get('heat%d' % i, 1)
        dheat = dh64[:, :16].double()
        wg(oc, lv, dheat, 1, Hh, has_bias=True)
        # the loss and its gradient, from the returned fp32 heat maps and the oracle's Gaussian maps of the same joints (exact in fp32:
        # pa_gauss_tab, pose_ops.hip:13-19, is the reference's table)
        inner_add = P.get('heat%d.in' % i, 2)[:, :16] if i + 1 < stacks else None
        note('heat gradient', 'heat%d' % i, heat_grad_check(dh64[:, :16], outs[i], target, grad_scale() / (B * 16.0 * Hh * Hh), inner_add, dtype))
        if bool((dh64[:, 16:] != 0).any()):
            fails.append(('heat gradient', 'heat%d padded channels' % i, float('inf')))
        ls, r = loss_check(S.losses[i], outs[i], target)
        note('loss', 'stack %d' % i, (r, 0.0))
        loss_sum = ls if loss_sum is None else loss_sum + ls                # loss_out_kernel (elementwise.hip): s += v, from 0
        del dh64, inner_add
        if i + 1 < stacks:
            fc, ic = 'forth_conv.%d' % i, 'in_conv.%d' % i
            ft = conv_term(lv, W(fc), chan, bias(fc), (v0('xin%d' % i),))
            note('conv forward', fc, check16(P.get('forth%d' % i, 2), ft, dtype), (fc,))
            h64 = P.get('heat%d' % i, 2)[:, :16].double()
            xt = conv_term(h64, W(ic), 64, bias(ic), (P.get('forth%d' % i, 2).double(),))
            note('conv forward', ic, check16(P.get('xin%d' % (i + 1), 2), xt, dtype), (ic,))
            gx = P.get('xin%d' % (i + 1), 1).double()
            # in_conv's data gradient dheat_in (its only reader is the heat-loss gradient kernel): rnd(in_conv^T(d xin<i+1>)); the
            # padded channels 16..63 come from zero weight rows and must be exactly zero
            dhi = P.get('heat%d.in' % i, 2)
            note('conv data gradient', ic, check16(dhi[:, :16], dgrad_term(gx, W(ic), chan), dtype), (ic,))
            if bool((dhi[:, 16:] != 0).any()):
                fails.append(('conv data gradient', ic + ' padded channels', float('inf')))
            wg(fc, lv, gx, 1, Hh, has_bias=True)
            wg(ic, h64, gx, 1, Hh, has_bias=True)
        # d lin<i> = mask * (forth^T(d xin<i+1>) + lgrad_tmp), lgrad_tmp = rnd(out_conv^T(d heat)) (net.hip:958-966); the last stack:
        # mask * out_conv^T(d heat)
        lm = (P.get('lin%d' % i, 0) > 0).double()
        oct_ = dgrad_term(dheat, W(oc), 64)
        if i + 1 < stacks:
            t = dgrad_term(gx, W(fc), chan, (rounded(oct_, dtype),))
        else:
            t = oct_
        note('conv data gradient', 'lin%d' % i, check16(P.get('lin%d' % i, 1), t, dtype, lm), (oc,) + ((fc,) if i + 1 < stacks else ()))
        del lm, oct_, t
    note('loss', 'total', (ratio(loss_total.reshape(1), loss_sum.v.reshape(1), loss_sum.e.reshape(1)), 0.0))
    # coverage: every conv of the net has each kind of check (the stem has no data gradient: its input is the image)
    want = set((c, k) for c in names for k in ('conv forward', 'weight gradient', 'bias') + (('conv data gradient',) if c != 'conv1' else ()))
    if want - checked:
        fails.append(('coverage', 'checks missing: %s' % sorted(want - checked)[:20], 0))
    # GEOMETRIC guard only: some layer of the leg has a shape the grouped weight-gradient kernel takes (the mirror's rule; which kernel
    # the engine launched is not observed)
    for kind in expect:
        if not met[kind]:
            fails.append(('coverage', 'no layer of this leg has a shape of the %s weight-gradient split' % kind, 0))
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('conv_exact %s %s stacks %d chan %d B %d res %d: worst error / bound: %s; %d convs, %d with grouped splits'
            % ('fp16' if dtype == torch.float16 else 'bf16', history + (' masked' if S.masks is not None else ''), stacks, chan, B, res,
               ', '.join('%s %.3g' % (k, worst[k]) for k in KINDS), len(set(c for c, _ in checked)), met['group']))
    return worst, fails


if __name__ == '__main__':          # the fp16 legs: tests/test_gpu_conv_exact.py runs this with POSEADV_DTYPE=fp16
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pose_adv_aug_amd._lib import lib as _l
    assert _l().pa_dtype() == 1, 'run with POSEADV_DTYPE=fp16'
    from tests.bn_exact import _child_kw
    worst, fails = run_leg(*[int(a) for a in sys.argv[1:6]], log=lambda s: print(s, flush=True), **_child_kw(sys.argv[6:]))
    print('FAILURES %d %s' % (len(fails), fails[:20]))
    print('FP16 CONV EXACT ' + ('PASSED' if not fails else 'FAILED'), flush=True)
    sys.exit(1 if fails else 0)
