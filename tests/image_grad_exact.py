"""The gradient with respect to the input image -- the data gradient of the 7 x 7 stride-2 pad-3 stem convolution (csrc/stem_dgrad.hip;
pa_stem_dgrad, pa_hg_set_image_grad) -- against float64, element by element, with the bound of tests/conv_exact.py.

Reference.  dimg[b][c][y][x] = sum_{n,ky,kx} g[b][n][(y+3-ky)/2][(x+3-kx)/2] w[n][c][ky][kx] over the taps whose two quotients are integers
inside the H/2 x W/2 map: stem_dgrad64, one float64 matrix product per tap, scattered with stride 2.  g and w are the kernel's operands:
rnd(g) (the BatchNorm-backward gradient fmaf(kA, dz, fmaf(kB, raw, kC)) of the stem output, computed in fp32 and rounded once to the
storage type; view 3 of "stem") and rnd(w) (the packed 16-bit copy the forward pass reads).  Their products are exact in float64.

Bound.  |got - ref| <= e + u |ref|, e = 2 u D sum |g w|, u = 2^-24 (conv_exact.bound32: an fp32 output).  D = 32 + ceil(K / 32) with
K = 1024: the kernel treats a 2 x 2 block of image pixels as one GEMM row whose operand is the 4 x 4 window of g x 64 channels and chains
all 32 MFMAs of that K = 1024 into ONE fp32 accumulator per output (stem_dgrad.hip: `acc = PA_MFMA_16x16x32(fa, fb, acc)`, s = 0 .. 31):
no split of the reduction, no combining tree.  The zero entries of the weight tile (the taps a parity class lacks, the 4th channel) add
exact zeros.  The product with 1 / pa_grad_scale() (a power of two) is exact.  D = 64.

Eval mode.  The backward pass of an eval-mode forward runs the same launches; the check reads the operand the kernel read (view 3), so it
holds whatever that gradient means.  In the IEEE-half build the (2 stacks, res 64, B 1) leg's eval-mode gradient leaves half's range
upstream of the stem (its 1 x 1 maps: BatchNorm-backward constants of a one-element batch against eval-mode activations), and view 3 is
NaN: poisoned_check then asks what the interface promises -- an overflowed gradient stays inf / NaN in the output -- and holds every
element no non-finite operand reaches to the bound.  With finite operands it is the plain check over every element.

block_gemm64 is that GEMM formulation in float64 (weight tile [1024][16], window gather), index for index as the kernel builds it: the
CPU test holds it against stem_dgrad64, so the tap arithmetic ky = py + 5 - 2 wy is checked without a GPU."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))        # (run as a script by the fp16 leg)
from tests import conv_exact as X  # noqa: E402

K_CHAIN = 1024                               # 4 x 4 window x 64 channels, one accumulator chain
DEPTH = X.depth_fwd(K_CHAIN, 0)              # 32 + 32


def stem_dgrad64(g, w):
    """g [B][N][Hm][Wm], w [N][C][7][7] -> d image [B][C][2 Hm][2 Wm] in float64: y + 3 = 2 i + ky, x + 3 = 2 j + kx."""
    g, w = g.double(), w.double()
    B, N, Hm, Wm = g.shape
    C = w.shape[1]
    out = torch.zeros(B, C, 2 * Hm + 6, 2 * Wm + 6, dtype=torch.float64, device=g.device)
    gm = g.permute(0, 2, 3, 1).reshape(-1, N)
    for ky in range(7):
        for kx in range(7):
            t = gm.matmul(w[:, :, ky, kx]).view(B, Hm, Wm, C).permute(0, 3, 1, 2)
            out[:, :, ky:ky + 2 * Hm:2, kx:kx + 2 * Wm:2] += t
    return out[:, :, 3:3 + 2 * Hm, 3:3 + 2 * Wm].contiguous()


def block_gemm64(g, w):
    """The kernel's formulation in float64: row = the 2 x 2 block at (2i, 2j), 16 outputs (py, px, c: c = 3 zero), K = (wy, wx, n) over
    the window i-1 .. i+2, j-1 .. j+2; weight tile entry = w[n][c][py + 5 - 2 wy][px + 5 - 2 wx] where both taps are in 0 .. 6."""
    g, w = g.double(), w.double()
    B, N, Hm, Wm = g.shape
    wt = torch.zeros(4, 4, N, 2, 2, 4, dtype=torch.float64)
    for wy in range(4):
        for wx in range(4):
            for py in range(2):
                for px in range(2):
                    ky, kx = py + 5 - 2 * wy, px + 5 - 2 * wx
                    if 0 <= ky < 7 and 0 <= kx < 7:
                        wt[wy, wx, :, py, px, :3] = w[:, :, ky, kx]
    gp = F.pad(g, (1, 2, 1, 2)).permute(0, 2, 3, 1)                      # zero outside the map: rows -1 .. Hm + 1
    win = torch.stack([torch.stack([gp[:, wy:wy + Hm, wx:wx + Wm, :] for wx in range(4)], 3) for wy in range(4)], 3)      # [B][Hm][Wm][wy][wx][N]
    o = win.reshape(B * Hm * Wm, 16 * N).matmul(wt.reshape(16 * N, 16)).view(B, Hm, Wm, 2, 2, 4)
    return o.permute(0, 5, 1, 3, 2, 4).reshape(B, 4, 2 * Hm, 2 * Wm)     # [B][c][i][py][j][px]


def term(g, w, scale=1.0):
    """the kernel's result as a conv_exact.Term: value, e = 2 u D sum |g w|, magnitude; scale (a power of two) multiplies all three"""
    v = stem_dgrad64(g, w) * scale
    mag = stem_dgrad64(g.abs(), w.abs()) * scale
    return X.Term(v, 2 * X.U * DEPTH * mag, mag)


def bound_check(got_nchw, g, w, scale=1.0):
    """(worst |got - ref| / bound over EVERY element, degenerate fraction) of an fp32 [B][3][H][W] gradient against rnd-ed operands"""
    return X.check32(got_nchw, term(g, w, scale))


def poisoned_check(got_nchw, g, w, scale=1.0):
    """bound_check for an operand that may hold inf / NaN (the half-precision build: a gradient that left half's range upstream of the stem
    stays inf / NaN).  Returns (worst ratio, degenerate fraction, finite results where the reference is not finite).  With a finite g this
    IS bound_check, over every element.  Otherwise: the reference is not finite at the 7 x 7 tap footprint of a non-finite pixel of g, and
    there the result must not be finite either; the kernel multiplies the whole 4 x 4 window of a 2 x 2 block, zero weights included
    (0 x NaN = NaN), so the 8 x 8 pixels of the blocks whose window holds such a pixel may be non-finite -- they are left out of the bound;
    every other element is held to the bound computed with the non-finite operands set to 0 (none of them enters its window)."""
    fin = torch.isfinite(g)
    if bool(fin.all()):
        return bound_check(got_nchw, g, w, scale) + (0,)
    nf = (~fin).any(dim=1, keepdim=True).double()                                                        # [B][1][Hm][Wm]
    ref_nf = stem_dgrad64(nf, torch.ones(1, 1, 7, 7, dtype=torch.float64, device=g.device)) > 0       # the taps' footprint
    poison = F.max_pool2d(F.pad(nf, (1, 2, 1, 2)), 4, 1) > 0                                          # blocks whose window i-1 .. i+2 holds one
    poison = poison.repeat_interleave(2, 2).repeat_interleave(2, 3).expand_as(got_nchw)
    t = term(torch.where(fin, g, torch.zeros_like(g)), w, scale)
    b = X.bound32(t.v, t.e)
    keep = ~poison
    stayed_finite = int((torch.isfinite(got_nchw) & ref_nf.expand_as(got_nchw)).sum())
    if not bool(keep.any()):
        return 0.0, 0.0, stayed_finite
    return X.ratio(got_nchw[keep], t.v[keep], b[keep]), X.degenerate(t.mag[keep], b[keep]), stayed_finite


def nhwc4_to_nchw(d):
    """[B][H][W][4] -> ([B][3][H][W], the 4th floats)"""
    return d[..., :3].permute(0, 3, 1, 2).contiguous(), d[..., 3]


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU legs (shared by tests/test_gpu_image_grad.py and the fp16 child below)
OP_SHAPES = [(1, 64, 64), (2, 128, 128), (3, 34, 66), (1, 2, 2)]      # a single tile, whole tiles, odd maps with partial tiles, the 1 x 1 map
NET_LEGS = [(1, 128, 2, 71), (2, 64, 1, 72), (1, 192, 3, 73)]         # stacks, res, B, seed (chan 128)
SENTINEL = -777.25
PAD = 64                                                              # floats in front of and behind the output (keeps the 16-byte alignment)


def _verdict(fails, what, r_deg, log):
    r, deg = r_deg
    log('image_grad %s: worst error / bound %.3g, degenerate %.3g' % (what, r, deg))
    if not (r <= 1.0):
        fails.append((what, 'outside the bound', r))
    if deg > X.DEGENERATE:
        fails.append((what, 'degenerate', deg))


def operator_leg(B, H, W, layout, log=print):
    """pa_stem_dgrad against the bound; layout 1: the 4th float exactly 0; nothing written in front of or behind the output"""
    import numpy as np
    from pose_adv_aug_amd._lib import act_dtype, check, lib, ptr, stream
    from tests import inputs
    import ctypes as C
    L, dtype, fails = lib(), act_dtype(), []
    g = inputs.rng(500, B, H, W)
    dy = torch.from_numpy(g.standard_normal((B, 64, H // 2, W // 2)).astype(np.float32)).cuda()
    w = torch.from_numpy((g.standard_normal((64, 3, 7, 7)) / np.sqrt(147.0)).astype(np.float32)).cuda()
    n = B * H * W * (4 if layout else 3)
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device='cuda')
    nws = L.pa_stem_dgrad_workspace_bytes(B, H, W)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device='cuda')
    check(L.pa_stem_dgrad(ptr(dy), ptr(w), C.c_void_p(buf.data_ptr() + 4 * PAD), B, H, W, layout, ptr(ws), stream()), 'pa_stem_dgrad')
    torch.cuda.synchronize()
    what = 'operator B %d %d x %d layout %d' % (B, H, W, layout)
    if not (bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + n:] == SENTINEL).all())):
        fails.append((what, 'wrote outside the output', 0))
    out = buf[PAD:PAD + n]
    if bool((out == SENTINEL).any()):
        fails.append((what, 'elements not written', int((out == SENTINEL).sum())))
    if layout:
        got, pad4 = nhwc4_to_nchw(out.view(B, H, W, 4))
        if bool((pad4 != 0).any()):
            fails.append((what, '4th float not 0', float(pad4.abs().max())))
    else:
        got = out.view(B, 3, H, W)
    _verdict(fails, what, bound_check(got, X.rnd(dy.double(), dtype), X.rnd(w.double(), dtype)), log)
    return fails


def make_img4(img):
    """[B][3][res][res] fp32 -> [B][res][res][4] in the storage type (4th channel 0), as the device warp delivers it"""
    from pose_adv_aug_amd._lib import act_dtype
    return F.pad(img.permute(0, 2, 3, 1), (0, 1)).to(act_dtype()).contiguous()


def net_inputs(B, res, seed):
    from tests import inputs
    img = torch.from_numpy(inputs.images(seed + 100, B, res)).cuda()
    pts = torch.from_numpy(inputs.heat_pts(seed + 101, B, res=res // 4)).cuda()
    return img, make_img4(img), pts


def check_net_grad(net, got_nchw, what, fails, log):
    """the image gradient of the last backward pass against stem_dgrad64(rnd(view 3 of "stem"), rnd(stem weight)) / grad_scale"""
    from pose_adv_aug_amd._lib import act_dtype, grad_scale
    from tests.bn_exact import Probe
    torch.cuda.synchronize()
    dtype = act_dtype()
    g = X.rnd(Probe(net).get('stem', 3).double(), dtype)
    w = X.rnd(net.state_dict()['conv1.weight'].double(), dtype)
    if not bool((g != 0).any()):
        fails.append((what, 'the stem gradient is zero', 0))
    r, deg, stayed_finite = poisoned_check(got_nchw, g, w, 1.0 / grad_scale())
    if not bool(torch.isfinite(g).all()):
        log('image_grad %s: %d of %d operand elements not finite' % (what, int((~torch.isfinite(g)).sum()), g.numel()))
        if dtype != torch.float16:
            fails.append((what, 'a non-finite stem gradient outside the half-precision build', 0))
    if stayed_finite:
        fails.append((what, 'finite results where the reference is not finite', stayed_finite))
    _verdict(fails, what, (r, deg), log)


def net_leg(stacks, res, B, seed, log=print):
    """the gradient inside the net: a training step from img4 (both layouts), the caller's heat gradients, eval mode, the NCHW input"""
    from pose_adv_aug_amd.pylib import HumanPts
    from tests.heat_grads_exact import make_net
    fails = []
    net = make_net(stacks, B, res, seed)
    img, img4, pts = net_inputs(B, res, seed)
    tag = '%d stacks res %d B %d ' % (stacks, res, B)
    net.loss_and_backward(img4=img4, pts=pts, input_grad=True)
    d = net.last_input_grad
    if tuple(d.shape) != (B, 3, res, res) or d.dtype != torch.float32:
        fails.append((tag, 'shape', tuple(d.shape)))
    check_net_grad(net, d, tag + 'train img4', fails, log)
    # the other store form of the same step (batch statistics: the running estimates do not enter a training pass)
    net.loss_and_backward(img4=img4, pts=pts, input_grad='nhwc4')
    torch.cuda.synchronize()
    d4 = net.last_input_grad
    if tuple(d4.shape) != (B, res, res, 4):
        fails.append((tag, 'nhwc4 shape', tuple(d4.shape)))
    else:
        d3, pad4 = nhwc4_to_nchw(d4)
        if not torch.equal(d3, d):
            fails.append((tag, 'the two layouts differ', float((d3 - d).abs().max())))
        if bool((pad4 != 0).any()):
            fails.append((tag, '4th float not 0', float(pad4.abs().max())))
    net.loss_and_backward(img4=img4, pts=pts)
    if net.last_input_grad is not None:
        fails.append((tag, 'last_input_grad not reset', 0))
    # the MSE's own gradient handed in by the caller
    outs = net(img4=img4)
    T = HumanPts.pts2heatmap_batch(pts, res // 4, res // 4)
    dg = net.backward([2 * (o - T) / o.numel() for o in outs], input_grad=True)
    check_net_grad(net, dg, tag + 'given heat gradients', fails, log)
    # eval mode (running estimates), then the NCHW fp32 entry in training mode
    net.eval()
    net.loss_and_backward(img4=img4, pts=pts, input_grad=True)
    check_net_grad(net, net.last_input_grad, tag + 'eval', fails, log)
    net.train()
    net.loss_and_backward(x=img, pts=pts, input_grad=True)
    check_net_grad(net, net.last_input_grad, tag + 'train x', fails, log)
    return fails


def launch_rows(step):
    """the distinct rows pa_conv_launch_log records while step() runs"""
    import ctypes as C
    from pose_adv_aug_amd._lib import lib
    L = lib()
    L.pa_conv_launch_log(None, 0)
    try:
        step()
    finally:
        buf = (C.c_int * (14 * 1024))()
        n = L.pa_conv_launch_log(buf, 1024)
    return sorted(tuple(buf[14 * i:14 * i + 14]) for i in range(n))


def same_leg(stacks=2, res=128, B=2, seed=81, log=print):
    """two nets, same seed and inputs, door on and off: gradients, heat maps and BatchNorm buffers bit for bit; the losses; the launch log.
    The per-stack losses: head_fwd_kernel adds one partial sum per workgroup with atomicAdd (pose_ops.hip), in whatever order the
    workgroups arrive, so two runs of the SAME step differ in the last bits with or without the feature (measured: two door-off twins
    differ too).  What is deterministic is what the sum is made of: the fp32 heat maps must be bit-identical, and each net's loss must lie
    within conv_exact.loss_check's bound (any order of the additions) of the float64 MSE of those heat maps."""
    from pose_adv_aug_amd.pylib import HumanPts
    from tests.heat_grads_exact import make_net
    fails = []
    img, img4, pts = net_inputs(B, res, seed)
    T = HumanPts.pts2heatmap_batch(pts, res // 4, res // 4)
    res_ = {}
    for on in (False, True):
        net = make_net(stacks, B, res, seed)
        keep = {}
        rows = launch_rows(lambda: keep.update(outs=net.loss_and_backward(img4=img4, pts=pts, input_grad=on, want_outputs=True)[1]))
        torch.cuda.synchronize()
        res_[on] = (net.flat_grads.clone(), torch.stack(keep['outs']), net.flat_buffers.clone(), rows, net)
        for i in range(stacks):
            r = X.loss_check(net._last_losses[i], keep['outs'][i], T)[1]
            if not (r <= 1.0):
                fails.append(('door %s' % ('on' if on else 'off'), 'loss of stack %d outside its bound' % i, r))
    log('image_grad door on / off: per-stack losses bit-equal: %s' % bool(torch.equal(res_[False][4]._last_losses, res_[True][4]._last_losses)))
    for i, name in enumerate(('flat_grads', 'heat maps (the terms of the per-stack losses)', 'BatchNorm buffers')):
        if not torch.equal(res_[False][i], res_[True][i]):
            fails.append(('door on / off', name + ' differ', 0))
    if not (float(res_[True][0].abs().max()) > 0 and bool(torch.isfinite(res_[True][0]).all())):
        fails.append(('door on / off', 'gradients zero or not finite', 0))
    if res_[True][4].last_input_grad is None or res_[False][4].last_input_grad is not None:
        fails.append(('door on / off', 'last_input_grad', 0))
    net = res_[False][4]
    again = launch_rows(lambda: net.loss_and_backward(img4=img4, pts=pts))
    if not (len(again) > 0 and again == res_[False][3]):
        fails.append(('launch log', 'two door-off steps differ', len(again)))
    if res_[True][3] != res_[False][3]:
        fails.append(('launch log', 'the door-on step added or lost a row', len(res_[True][3]) - len(res_[False][3])))
    log('image_grad door on / off: %d launch rows, %d failures' % (len(again), len(fails)))
    return fails


if __name__ == '__main__':          # the fp16 legs: tests/test_gpu_image_grad.py runs this with POSEADV_DTYPE=fp16
    from pose_adv_aug_amd._lib import lib as _l
    assert _l().pa_dtype() == 1, 'run with POSEADV_DTYPE=fp16'
    _log = lambda s: print(s, flush=True)
    fails = []
    for (_B, _H, _W) in OP_SHAPES:
        for _lay in (0, 1):
            fails += operator_leg(_B, _H, _W, _lay, _log)
    for _leg in NET_LEGS:
        fails += net_leg(*_leg, log=_log)
    fails += same_leg(log=_log)
    print('FAILURES %d %s' % (len(fails), fails[:20]))
    print('FP16 IMAGE GRAD ' + ('PASSED' if not fails else 'FAILED'), flush=True)
    sys.exit(1 if fails else 0)
