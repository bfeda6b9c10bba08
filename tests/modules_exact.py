"""The exact checks of tests/conv_exact.py and tests/bn_exact.py over a pose net with num_modules > 1: every site of an hourglass and
post_res is a chain of residual blocks (Chain, csrc/net.h).  ONE training step; then every convolution is recomputed in float64 block
by block (conv_exact.Checker.block with the parameter prefix '<site>.<j>.', the hook name '<site>.m<j>' and, as its input, the previous
block's hook or the site's input), every BatchNorm, pool, merge and cell mask with the site checks of bn_exact on the chain-aware
lists below, and the head as conv_exact.run_leg does, with its coverage assertion.  The bounds are those modules' own: nothing here
defines a tolerance.

What a chain changes, and where it shows:
  * block j >= 1 reads a tensor with a pending BatchNorm that has two readers (conv1 and conv3's shortcut addend), and its input
    gradient goes through that BatchNorm's backward epilogue: 'conv forward' / 'conv data gradient' of the block, 'bn backward' of
    block j - 1's bn3;
  * the routed pool gradient poolgrad<k> is the second addend of the FIRST block of skip<k> only (add2 below); the other blocks of a
    skip chain run their whole backward pass on the side stream;
  * the upsample-add, the pools and the cell masks read / write the LAST block of a chain (the plain hook names), and only that block of
    up<k> has the four-fold capacity of backward partial rows (rows_scale).

tests/test_gpu_modules.py runs the legs; for the IEEE-half build it runs this file as a child process."""
import os
import sys

import numpy as np
import torch

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import bn_exact as BN
from tests import conv_exact as X


def chain_sites(stacks, modules, masked=False):
    """(parameter prefix of the site, hook name of the site, hook name of the site's input, (i, k) of the pool whose routed gradient the
    site's first block adds or None), every chain of the net in the engine's forward order."""
    s = []
    for i in range(stacks):
        for k in (1, 2, 3, 4):
            s.append(('hg.%d.skip%d.' % (i, k), 'hg%d.skip%d' % (i, k), 'xin%d' % i if k == 1 else 'hg%d.down%d' % (i, k - 1), (i, k)))
            s.append(('hg.%d.down%d.' % (i, k), 'hg%d.down%d' % (i, k), 'hg%d.pool%d' % (i, k), None))
            s.append(('hg.%d.up%d.' % (i, k), 'hg%d.up%d' % (i, k),
                      ('hg%d.maskedneck' if masked else 'hg%d.neck') % i if k == 4 else 'hg%d.merge%d' % (i, k + 1), None))
        s.append(('hg.%d.neck.' % i, 'hg%d.neck' % i, 'hg%d.down4' % i, None))
        s.append(('post_res.%d.' % i, 'post%d' % i, 'hg%d.merge1' % i, None))
    return s


def block_sites(stacks, modules, masked=False):
    """(parameter prefix of the block, hook name of its output, hook name of its input, has adapter, pool (i, k) of its second addend or
    None, capacity factor of bn3's backward rows), every residual block of the net."""
    b = [('residual1.', 'res1', 'stem', True, None, 1), ('residual2.', 'res2', 'pool0', False, None, 1), ('residual3.', 'res3', 'res2', True, None, 1)]
    for p, site, inp, pool in chain_sites(stacks, modules, masked):
        for j in range(modules):
            last = j == modules - 1
            b.append(('%s%d.' % (p, j), '%s.m%d' % (site, j), inp if j == 0 else '%s.m%d' % (site, j - 1), False,
                      pool if j == 0 else None, 4 if (last and '.up' in site) else 1))
    return b


def conv_names(stacks, modules):
    n = ['conv1']
    for p, _, _, ad, _, _ in block_sites(stacks, modules):
        n += [p + 'conv1', p + 'conv2', p + 'conv3'] + ([p + 'adapter'] if ad else [])
    for i in range(stacks):
        n += ['linear.%d.0' % i, 'out_conv.%d' % i]
        if i + 1 < stacks:
            n += ['forth_conv.%d' % i, 'in_conv.%d' % i]
    return n


def bn_sites(stacks, modules):
    """(parameter prefix of the BatchNorm, hook name of the tensor it normalises, capacity factor of its backward rows)"""
    sites = [('bn1', 'stem', 1)]
    for p, out, _, _, _, rows in block_sites(stacks, modules):
        sites += [(p + 'bn1', out + '.x1', 1), (p + 'bn2', out + '.x2', 1), (p + 'bn3', out, rows)]
    return sites + [('linear.%d.1' % i, 'lin%d' % i, 1) for i in range(stacks)]


def hg_pair(stacks, modules, chan, B, res, seed):
    """the oracle with deterministic weights and the engine's net holding the same ones (tests/test_gpu_net.py _hg_pair with modules)"""
    from oracle import model as om
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    ref = om.create_hg(stacks, modules, 16, chan)
    om.deterministic_fill_(ref, seed=seed)
    net = create_hg(stacks, modules, 16, chan, res=res, default_batch=B)
    rsd = ref.state_dict()
    assert list(net.state_dict().keys()) == list(rsd.keys()), 'state_dict names/order must match the reference module tree'
    for (k, a), b in zip(net.state_dict().items(), rsd.values()):
        assert tuple(a.shape) == tuple(b.shape), k
    net.load_state_dict(rsd)
    return ref, net


def pose_step(stacks, modules, chan, B, res, seed, history='fresh', masks=None):
    """tests/exact_history.py pose_step for a net with `modules` blocks per site: 'fresh' (seeded NCHW images, the first step after the
    bind) or 'warm' (here: TWO train_step calls with RMSprop in front of the checked step, entered as bench.py enters its steps)."""
    from pose_adv_aug_amd.stack_hg import train_step
    from pose_adv_aug_amd.utils.optim import RMSprop
    from tests import exact_history as H
    from tests import inputs
    from tests.test_gpu_net import t
    assert history in ('fresh', 'warm') and (masks is None or history == 'fresh')
    torch.cuda.set_device(0)
    ref, net = hg_pair(stacks, modules, chan, B, res, seed)
    del ref
    S = H.Step()
    S.net, S.history = net, history
    S.masks = None if masks is None else H.drop_masks(masks, B).cuda()
    net.train()
    if history == 'fresh':
        S.sd0, S.before = H._snapshot(net)
        S.img = t(inputs.images(seed + 100, B, res)).cuda()
        S.pts_np = inputs.heat_pts(seed + 101, B, res=res // 4)
        S.pts = t(S.pts_np).cuda()
        loss, S.outs = net.loss_and_backward(S.img, S.pts, want_outputs=True, dropout_masks=S.masks)
    else:
        feed = H.Feed(B, res, seed)
        opt = RMSprop(net, lr=H.LR)
        for _ in range(2):
            train_step(net, opt, feed.aug, feed.next_batch())
        data = feed.next_data()
        torch.cuda.synchronize()
        S.sd0, S.before = H._snapshot(net)
        S.img, S.pts = H.img_of(data['img4']), data['pts']
        S.pts_np = S.pts.cpu().numpy().astype(np.float64)
        loss, S.outs = net.loss_and_backward(img4=data['img4'], pts=data['pts'], want_outputs=True, after_forward=H._meters(net, data))
        S.data = data
    S.loss_total = loss.clone()
    S.losses = net._last_losses
    torch.cuda.synchronize()
    S.grads = {n: g.clone() for n, g in net.named_grads()}
    return S


def check_convs(S, P, stacks, modules, chan, B, res, dtype, expect=()):
    """every conv of the net: the stem, every block of every chain, the head (conv_exact.run_leg, the head part copied as it stands)."""
    from pose_adv_aug_amd._lib import grad_scale
    from tests import inputs
    from tests.test_gpu_net import t
    sd0, img, pts_np, outs, loss_total, grads = S.sd0, S.img, S.pts_np, S.outs, S.loss_total, S.grads
    names = conv_names(stacks, modules)
    assert sorted(names) == sorted(k[:-len('.weight')] for k in sd0 if k.endswith('.weight') and sd0[k].dim() == 4), \
        'conv_names must name every conv of the net'
    ck = X.Checker(sd0, grads, dtype, B)
    W, bias, note, wg, worst, fails, met, checked = ck.W, ck.bias, ck.note, ck.wg, ck.worst, ck.fails, ck.met, ck.checked
    rnd, conv_term, dgrad_term, check16, check32, rounded = X.rnd, X.conv_term, X.dgrad_term, X.check16, X.check32, X.rounded
    grad_op = lambda n: ck.grad_op(P, n)
    v0 = lambda n: P.get(n, 0).double()
    sv0 = lambda n: rnd(P.get(n, 0), dtype).double()
    xs = rnd(img.double(), dtype)
    a0 = conv_term(xs, W('conv1'), 256, bias('conv1'), stride=2, pad=3)
    note('conv forward', 'conv1', check16(P.get('stem', 2), a0, dtype), ('conv1',))
    wg('conv1', xs, grad_op('stem'), 7, res // 2, stride=2, pad=3)
    del a0
    # a pending BatchNorm (masked gradient): the stem and every block output (xin0 is residual3's); not the pools, merges, xin<i>, i >= 1,
    # or the occlusion branch's maskedneck
    has_bn = lambda n: not ('pool' in n or 'merge' in n or 'masked' in n or (n.startswith('xin') and n != 'xin0'))
    for p, out, inp, ad, pool, _ in block_sites(stacks, modules, masked=S.masks is not None):
        add2 = P.get('hg%d.poolgrad%d' % pool, 2) if pool is not None else None          # first block of a skip chain only
        ck.block(p, out, P, P, inp, True, ad, add2, has_bn(inp))
        del add2
    Hh = res // 4
    target = t(inputs.heatmaps_from_pts(pts_np, res=Hh)).cuda()
    loss_sum = None
    for i in range(stacks):
        lin = 'linear.%d.0' % i
        pv = sv0('post%d' % i)
        note('conv forward', lin, check16(P.get('lin%d' % i, 2), conv_term(pv, W(lin), chan, bias(lin)), dtype), (lin,))
        gl = grad_op('lin%d' % i)
        wg(lin, pv, gl, 1, Hh)
        note('conv data gradient', 'post%d' % i, check16(P.get('post%d' % i, 1), dgrad_term(gl, W(lin), chan), dtype,
                                                          (P.get('post%d' % i, 0) > 0).double()), (lin,))
        del gl
        lv = sv0('lin%d' % i)
        oc = 'out_conv.%d' % i
        heat = conv_term(lv, W(oc), chan, bias(oc))
        note('conv forward', oc, check32(outs[i].double(), heat), (oc,))
        note('conv forward', oc + ' (stored)', check16(P.get('heat%d' % i, 2)[:, :16], heat, dtype), (oc,))
        dh64 = P.get('heat%d' % i, 1)
        dheat = dh64[:, :16].double()
        wg(oc, lv, dheat, 1, Hh, has_bias=True)
        inner_add = P.get('heat%d.in' % i, 2)[:, :16] if i + 1 < stacks else None
        note('heat gradient', 'heat%d' % i, X.heat_grad_check(dh64[:, :16], outs[i], target, grad_scale() / (B * 16.0 * Hh * Hh), inner_add, dtype))
        if bool((dh64[:, 16:] != 0).any()):
            fails.append(('heat gradient', 'heat%d padded channels' % i, float('inf')))
        ls, r = X.loss_check(S.losses[i], outs[i], target)
        note('loss', 'stack %d' % i, (r, 0.0))
        loss_sum = ls if loss_sum is None else loss_sum + ls
        del dh64, inner_add
        if i + 1 < stacks:
            fc, ic = 'forth_conv.%d' % i, 'in_conv.%d' % i
            ft = conv_term(lv, W(fc), chan, bias(fc), (v0('xin%d' % i),))
            note('conv forward', fc, check16(P.get('forth%d' % i, 2), ft, dtype), (fc,))
            h64 = P.get('heat%d' % i, 2)[:, :16].double()
            xt = conv_term(h64, W(ic), 64, bias(ic), (P.get('forth%d' % i, 2).double(),))
            note('conv forward', ic, check16(P.get('xin%d' % (i + 1), 2), xt, dtype), (ic,))
            gx = P.get('xin%d' % (i + 1), 1).double()
            dhi = P.get('heat%d.in' % i, 2)
            note('conv data gradient', ic, check16(dhi[:, :16], dgrad_term(gx, W(ic), chan), dtype), (ic,))
            if bool((dhi[:, 16:] != 0).any()):
                fails.append(('conv data gradient', ic + ' padded channels', float('inf')))
            wg(fc, lv, gx, 1, Hh, has_bias=True)
            wg(ic, h64, gx, 1, Hh, has_bias=True)
        lm = (P.get('lin%d' % i, 0) > 0).double()
        oct_ = dgrad_term(dheat, W(oc), 64)
        tt = dgrad_term(gx, W(fc), chan, (rounded(oct_, dtype),)) if i + 1 < stacks else oct_
        note('conv data gradient', 'lin%d' % i, check16(P.get('lin%d' % i, 1), tt, dtype, lm), (oc,) + ((fc,) if i + 1 < stacks else ()))
        del lm, oct_, tt
    note('loss', 'total', (X.ratio(loss_total.reshape(1), loss_sum.v.reshape(1), loss_sum.e.reshape(1)), 0.0))
    # coverage: every conv of the net has each kind of check (the stem has no data gradient: its input is the image)
    want = set((c, k) for c in names for k in ('conv forward', 'weight gradient', 'bias') + (('conv data gradient',) if c != 'conv1' else ()))
    if want - checked:
        fails.append(('coverage', 'checks missing: %s' % sorted(want - checked)[:20], 0))
    for kind in expect:
        if not met[kind]:
            fails.append(('coverage', 'no layer of this leg has a shape of the %s weight-gradient split' % kind, 0))
    return worst, fails, met


def check_links(S, P, stacks, modules, dtype, stored_expected=('.x2', '')):
    """every BatchNorm, pool, merge and cell mask of the step (bn_exact.run_leg over the chain-aware site list; the pools, merges and
    masks name the sites' outputs, i.e. the last blocks, by their plain hook names)"""
    net, before, grads, M = S.net, S.before, S.grads, S.masks
    sd = net.state_dict()
    sites = bn_sites(stacks, modules)
    assert sorted(p for p, _, _ in sites) == sorted(k[:-len('.running_mean')] for k in sd if k.endswith('.running_mean')), \
        'bn_sites must name every BatchNorm of the net'
    worst = dict((k, 0.0) for k in BN.KINDS)
    fails = []
    note = BN.make_note(worst, fails)
    stored = {'.x2': 0, '': 0}
    for pre, name, rows in sites:
        BN.check_bn_site(P, pre, name, sd, before, grads, dtype, note, stored, rows_scale=rows)
    for suf, cnt in stored.items():
        if cnt == 0 and suf in stored_expected:
            fails.append(('stored bn backward', 'no block stored its dz%s' % ('2' if suf else '3'), 0))
    # '<site>.m<last>' is the same tensor as '<site>'
    for _, site, _, _ in chain_sites(stacks, modules):
        for view in (1, 2):
            if not torch.equal(P.get(site, view), P.get('%s.m%d' % (site, modules - 1), view)):
                fails.append(('hook names', site, view))
    ties = 0
    for out, src in BN.pool_sites(stacks):
        vin = P.get(src, 0)
        note('pool forward', out, BN.check_pool(vin, P.get(out, 0), dtype), bit=True)
        if out == 'pool0':
            r, n = BN.check_pool_bwd(P.get(out, 1), vin, P.get(src, 1), dtype, masked=True)
        else:
            i, k = int(out[2]), int(out[-1])
            add = P.get('xin%d' % (i + 1), 1) if (k == 1 and i + 1 < stacks) else None
            r, n = BN.check_pool_bwd(P.get(out, 1), vin, P.get('hg%d.poolgrad%d' % (i, k), 2), dtype, addend=add)
        note('pool backward', out, r, bit=True)
        ties += n
        del vin
    if ties == 0:
        fails.append(('pool backward', 'no 2 x 2 window of this leg had tied maxima: first-maximum routing was not tested', 0))
    changed = leaked = 0
    for i in range(stacks):
        for k in (1, 2, 3, 4):
            m, up, sk = 'hg%d.merge%d' % (i, k), 'hg%d.up%d' % (i, k), 'hg%d.skip%d' % (i, k)
            vu, vs = P.get(up, 0), P.get(sk, 0)
            if M is None:
                note('merge forward', m, BN.check_merge_fwd(vu, vs, P.get(m, 0), dtype), bit=True)
                note('merge backward', m, BN.check_merge_bwd(P.get(m, 1), vu, vs, P.get(up, 1), P.get(sk, 1), dtype), bit=True)
                continue
            ms = 'hg%d.maskedskip%d' % (i, k)
            vm, dm, dsk = P.get(ms, 0), P.get(ms, 1), P.get(sk, 1)
            note('mask forward', ms, BN.check_mask_fwd(vs, M, vm, dtype), bit=True)
            note('merge forward', m, BN.check_merge_fwd(vu, vm, P.get(m, 0), dtype), bit=True)
            note('merge backward', m, BN.check_merge_bwd_masked(P.get(m, 1), vu, P.get(up, 1), dm, dtype), bit=True)
            note('merge backward', sk, BN.check_mask_bwd(dm, M, vs, dsk), bit=True)
            changed += BN._mismatch(vm, BN.rnd(vs, dtype))
            leaked += int((dsk * (1 - BN.up4(M, dsk.shape[2])) != 0).sum())
        if M is not None:
            nk, mn = 'hg%d.neck' % i, 'hg%d.maskedneck' % i
            vn = P.get(nk, 0)
            note('mask forward', mn, BN.check_mask_fwd(vn, M, P.get(mn, 0), dtype), bit=True)
            note('merge backward', nk, BN.check_mask_bwd(P.get(mn, 1), M, vn, P.get(nk, 1)), bit=True)
    if M is not None and changed == 0:
        fails.append(('mask forward', 'no maskedskip differs from its skip tensor', 0))
    if leaked:
        fails.append(('merge backward', 'gradient of a skip tensor inside a dropped cell', leaked))
    # eval mode: a forward pass with the running estimates this step left
    net.eval()
    net(S.img)
    torch.cuda.synchronize()
    for pre, name, _ in sites:
        BN.check_bn_eval_site(P, pre, name, sd, note)
    net.train()
    return worst, fails


def run_leg(stacks, modules, chan, B, res, seed, log=print, expect=(), history='fresh', masks=None, stored_expected=('.x2', '')):
    """One training step (loss_and_backward, default multi-stream mode) of a net with `modules` blocks per site, then every check.
    expect: weight-gradient split kinds the leg must meet ('group'); stored_expected: the inner tensors ('.x2': dz2) and block outputs
    ('': dz3) of which at least one block must have stored its BatchNorm-backward gradient (both as in conv_exact / bn_exact).
    Returns ({kind: worst error / bound}, failures)."""
    from pose_adv_aug_amd._lib import act_dtype
    assert stacks <= 9 and modules <= 8
    dtype = act_dtype()
    S = pose_step(stacks, modules, chan, B, res, seed, history, masks)
    P = BN.Probe(S.net)
    worst, fails, met = check_convs(S, P, stacks, modules, chan, B, res, dtype, expect)
    w2, f2 = check_links(S, P, stacks, modules, dtype, stored_expected)
    worst = dict(list(worst.items()) + [('bn: ' + k, v) for k, v in w2.items()])
    fails = fails + f2
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('modules_exact %s %s stacks %d modules %d chan %d B %d res %d: worst error / bound: %s; %d layers with grouped splits'
            % ('fp16' if dtype == torch.float16 else 'bf16', history + (' masked' if masks is not None else ''), stacks, modules, chan, B, res,
               ', '.join('%s %.3g' % kv for kv in worst.items()), met['group']))
    return worst, fails


if __name__ == '__main__':          # the fp16 leg: tests/test_gpu_modules.py runs this with POSEADV_DTYPE=fp16
    from pose_adv_aug_amd._lib import lib as _l
    assert _l().pa_dtype() == 1, 'run with POSEADV_DTYPE=fp16'
    a = sys.argv[1:]
    worst, fails = run_leg(*[int(v) for v in a[:6]], log=lambda s: print(s, flush=True), expect=tuple(a[7:]), history=a[6] if len(a) > 6 else 'fresh')
    print('FAILURES %d %s' % (len(fails), fails[:20]))
    print('FP16 MODULES EXACT ' + ('PASSED' if not fails else 'FAILED'), flush=True)
    sys.exit(1 if fails else 0)
