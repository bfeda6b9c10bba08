"""Exact checks of the backward pass from GIVEN heat-map gradients (pa_hg_set_heat_grads, HourglassNet.backward / forward_autograd).

The injected gradient.  For stack i the engine writes, per pixel m and joint j < 16,
    dheat64[i][m][j] = storage( G_i[m][j] * s  (+ a[m][j]) ),   s = pa_grad_scale() (1 or 32768: exact in fp32),
a = in_conv's data gradient of an inner stack (storage type, the debug view 'heat<i>.in'), in fp32: the product, the add, the rounding
to the storage type (heat_inject_*_kernel, csrc/pose_ops.hip).  The bound is heat_grad_check's construction (tests/conv_exact.py) with
G * s in place of 2 (heat - target) gscale: one rounding of the product, one of the add (bn_exact.E), half an ulp of the storage type
(conv_exact.check16).  A compiler that contracts the product and the add into one fma rounds the exact G s + a once: inside the same
bound.  Channels 16..63 of dheat64 must stay exactly 0.

Everything behind the injected tensor is the unchanged engine: out_conv's weight / bias gradients and lin's data gradient are checked
from the injected tensor with conv_exact's own bounds (consumers()).

same_bits(): with G = 2 (out - T) / numel formed in fp32 by the caller, where numel is a power of two, every scaling on either side is
exact, so backward([G]) must leave the bits loss_and_backward leaves (also with occlusion masks, through the phased backward pass, and
when called twice), and a loss_and_backward afterwards must give its own bits again (the given gradients are off).

Run as a script with POSEADV_DTYPE=fp16 this is the half-precision child of tests/test_gpu_heat_grads.py."""
import os
import sys

import torch

G_STD = 1e-4            # G ~ N(0, G_STD^2): the size of a mean-reduced loss's gradient on a small map; the addend the same times s


def inject_term(G, scale, add):
    """the Term (value, fp32 error bound, sum of absolute terms) of G * scale (+ add); G fp32, add storage-type values, any float dtype."""
    from tests.bn_exact import E
    from tests.conv_exact import Term
    Gd = G.double()
    g = E(Gd) * E(torch.full_like(Gd, float(scale)))
    mag = Gd.abs() * float(scale)
    if add is not None:
        g = g + E(add.double())
        mag = mag + add.double().abs()
    return Term(g.v, g.e, mag)


def inject_check(got, G, scale, add, dtype):
    """(worst |got - ref| / bound, degenerate fraction) of an injected gradient (storage-type values in any float dtype)"""
    from tests.conv_exact import check16
    return check16(got, inject_term(G, scale, add), dtype)


def outside(got, G, scale, add, dtype):
    """fraction of the elements outside their bound"""
    from tests.conv_exact import bound16
    t = inject_term(G, scale, add)
    return float(((got.double() - t.v).abs() > bound16(t.v, t.e, dtype)).double().mean())


def emul_mul_add(G, scale, add, dtype):
    """fp32: round the product, round the sum, round to the storage type"""
    g = G.float() * torch.tensor(scale, dtype=torch.float32)
    if add is not None:
        g = g + add.float()
    return g.to(dtype).float()


def emul_fma(G, scale, add, dtype):
    """fp32 fma: the exact G * scale + add (float64 holds it: 24 + 16 significant bits, exponents close) rounded ONCE to fp32"""
    g = G.double() * float(scale)
    if add is not None:
        g = g + add.double()
    return g.float().to(dtype).float()


def move_one_ulp(x, dtype, up=True):
    """every element one storage-type ulp away from zero (up) or towards it"""
    b = x.to(dtype).view(torch.int16)
    return (b + (1 if up else -1)).view(dtype).float()


def cpu_data(seed, n, scale, dtype):
    """G ~ N(0, G_STD^2) fp32 and a storage-type addend of the magnitude of G * scale"""
    g = torch.Generator().manual_seed(seed)
    G = torch.randn(n, generator=g) * G_STD
    add = (torch.randn(n, generator=g) * (G_STD * scale)).to(dtype).float()
    return G, add


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU legs (shared by tests/test_gpu_heat_grads.py and the fp16 child below)
def make_net(stacks, B, res, seed, chan=128):
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    torch.cuda.set_device(0)
    net = create_hg(stacks, 1, 16, chan, res=res, default_batch=B)
    net.reset_parameters(seed=seed)
    net.train()
    return net


def rand_grads(seed, stacks, B, Hh, none_stack=None):
    g = torch.Generator().manual_seed(seed)
    return [None if i == none_stack else (torch.randn(B, 16, Hh, Hh, generator=g) * G_STD).cuda() for i in range(stacks)]


def read_injected(P, stacks):
    """[(d heat as stored [B][64][H][H], in_conv's data gradient [B][16][H][H] or None)] of the last backward pass"""
    out = []
    for i in range(stacks):
        add = P.get('heat%d.in' % i, 2)[:, :16].clone() if i + 1 < stacks else None
        out.append((P.get('heat%d' % i, 1).clone(), add))
    return out


def consumers(ck, P, stacks, chan, Hh):
    """out_conv.<i>'s weight and bias gradients and lin<i>'s data gradient from the injected d heat: conv_exact.run_leg's head checks"""
    from tests.conv_exact import check16, dgrad_term, rnd, rounded
    dtype = ck.dtype
    for i in range(stacks):
        oc, fc = 'out_conv.%d' % i, 'forth_conv.%d' % i
        lv = rnd(P.get('lin%d' % i, 0), dtype).double()
        dheat = P.get('heat%d' % i, 1)[:, :16].double()
        ck.wg(oc, lv, dheat, 1, Hh, has_bias=True)
        lm = (P.get('lin%d' % i, 0) > 0).double()
        oct_ = dgrad_term(dheat, ck.W(oc), 64)
        if i + 1 < stacks:
            gx = P.get('xin%d' % (i + 1), 1).double()
            t = dgrad_term(gx, ck.W(fc), chan, (rounded(oct_, dtype),))
        else:
            t = oct_
        ck.note('conv data gradient', 'lin%d' % i, check16(P.get('lin%d' % i, 1), t, dtype, lm), (oc,))


def inject_leg(stacks, B, res, seed, none_stack=None, check_consumers=False, log=print):
    """forward; backward from random G in both layouts (the second one through the phased backward pass); returns the failures"""
    from pose_adv_aug_amd._lib import act_dtype, grad_scale
    from tests import inputs
    from tests.bn_exact import Probe
    from tests.conv_exact import Checker, DEGENERATE
    dtype, scale, chan, Hh = act_dtype(), grad_scale(), 128, res // 4
    fails = []
    net = make_net(stacks, B, res, seed)
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    img = torch.from_numpy(inputs.images(seed + 100, B, res)).cuda()
    net(img)
    G = rand_grads(seed + 1, stacks, B, Hh, none_stack)
    net.backward(G)
    torch.cuda.synchronize()
    P = Probe(net)
    first = read_injected(P, stacks)
    for i, (dh, add) in enumerate(first):
        Gi = G[i] if G[i] is not None else torch.zeros(B, 16, Hh, Hh, device='cuda')
        r, deg = inject_check(dh[:, :16], Gi, scale, add, dtype)
        log('inject stacks %d B %d res %d stack %d%s: worst error / bound %.3g, degenerate %.3g' % (stacks, B, res, i, ' (None)' if G[i] is None else '', r, deg))
        if not r <= 1.0:
            fails.append(('injected gradient', 'heat%d' % i, r))
        if deg > DEGENERATE:
            fails.append(('degenerate bound', 'heat%d' % i, deg))
        if bool((dh[:, 16:] != 0).any()):
            fails.append(('injected gradient', 'heat%d padded channels' % i, float('inf')))
    if check_consumers:
        ck = Checker(sd0, {n: g.clone() for n, g in net.named_grads()}, dtype, B)
        consumers(ck, P, stacks, chan, Hh)
        log('consumers: %s' % ', '.join('%s %.3g' % kv for kv in ck.worst.items() if kv[1]))
        fails += ck.fails
    grads_first = net.flat_grads.clone()
    # the joint-minor layout of the same G, through the phased backward pass: the same buffers, the same parameter gradients
    done = []
    net.on_stack_done = done.append
    try:
        net.backward([None if g is None else g.permute(0, 2, 3, 1).contiguous() for g in G], layout='nhwc')
    finally:
        net.on_stack_done = None
    torch.cuda.synchronize()
    if done != list(range(stacks - 1, -1, -1)):
        fails.append(('phases', 'on_stack_done calls %s' % done, 0))
    for i, ((dh, add), (dh2, add2)) in enumerate(zip(first, read_injected(P, stacks))):
        if not torch.equal(dh, dh2) or (add is not None and not torch.equal(add, add2)):
            fails.append(('layouts', 'heat%d differs between the two layouts' % i, float('inf')))
    if not torch.equal(grads_first, net.flat_grads):
        fails.append(('layouts', 'parameter gradients differ between the two layouts', float('inf')))
    return fails


def mse_grad(out, pts, Hh):
    """d/d out of mean((out - gaussian(pts))^2) in fp32: one rounding (the difference) where numel is a power of two"""
    from pose_adv_aug_amd.pylib import HumanPts
    T = HumanPts.pts2heatmap_batch(pts, Hh, Hh)
    n = out.numel()
    assert n & (n - 1) == 0, 'numel must be a power of two for the scalings to be exact'
    return 2 * (out - T) / n


def same_bits(res, seed, masked=False, log=print):
    """1 stack, B 2: backward([G]) with the MSE's own gradient against loss_and_backward, bit for bit (module docstring)"""
    from tests import exact_history, inputs
    B, Hh = 2, res // 4
    fails = []
    net = make_net(1, B, res, seed)
    img = torch.from_numpy(inputs.images(seed + 100, B, res)).cuda()
    pts = torch.from_numpy(inputs.heat_pts(seed + 101, B, res=Hh)).cuda()
    M = exact_history.drop_masks(seed, B).cuda() if masked else None
    net.loss_and_backward(img, pts, dropout_masks=M)
    ref = net.flat_grads.clone()
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0

    def expect(what):
        torch.cuda.synchronize()
        if not torch.equal(net.flat_grads, ref):
            d = (net.flat_grads - ref).abs()
            fails.append(('same bits', '%s%s: %d elements differ, max %.3g' % (what, ' (masked)' if masked else '', int((d != 0).sum()), float(d.max())), 0))
        net.flat_grads.zero_()

    net.flat_grads.zero_()
    outs = net(img, dropout_masks=M)
    G = [mse_grad(outs[0], pts, Hh)]
    net.backward(G)
    expect('backward([G])')
    net.backward(G)
    expect('a second backward([G])')
    done = []
    net.on_stack_done = done.append
    try:
        net.backward(G)
    finally:
        net.on_stack_done = None
    expect('the phased backward([G])')
    if done != [0]:
        fails.append(('phases', 'on_stack_done calls %s' % done, 0))
    net.loss_and_backward(img, pts, dropout_masks=M)
    expect('loss_and_backward after backward() returned')
    log('same bits res %d%s: %d failures' % (res, ' masked' if masked else '', len(fails)))
    return fails


if __name__ == '__main__':          # the fp16 legs: tests/test_gpu_heat_grads.py runs this with POSEADV_DTYPE=fp16
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pose_adv_aug_amd._lib import lib as _l
    assert _l().pa_dtype() == 1, 'run with POSEADV_DTYPE=fp16'
    log = lambda s: print(s, flush=True)
    fails = inject_leg(2, 2, 128, 41, none_stack=0, check_consumers=True, log=log)
    fails += inject_leg(2, 3, 128, 42, none_stack=1, log=log)
    fails += inject_leg(1, 1, 192, 43, log=log)
    fails += same_bits(128, 44, log=log)
    fails += same_bits(256, 45, masked=True, log=log)
    print('FAILURES %d %s' % (len(fails), fails[:20]))
    print('FP16 HEAT GRADS ' + ('PASSED' if not fails else 'FAILED'), flush=True)
    sys.exit(1 if fails else 0)
