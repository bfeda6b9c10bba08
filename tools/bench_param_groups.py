#!/usr/bin/env python3
"""What parameter groups cost in the fused optimizer steps (profiles/param_groups.txt): pa_rmsprop_step_opts / pa_adam_step against
pa_rmsprop_step_groups / pa_adam_step_groups on the flat parameter array of the benchmark net (2 stacks, chan 256), without and with the
gradient norm + clip coefficient in front.

    python tools/bench_param_groups.py [--out profiles/param_groups.txt] [--rounds 20] [--calls 200]

Rows, for RMSprop(momentum, weight_decay, centered) and for AdamW(amsgrad):
  ungrouped          the call an optimizer without groups makes (the parent's launches)
  one group          the _groups call with one group: the same launches by construction
  realistic          --no_decay_1d 1 --freeze '^(conv1|bn1|residual[123])\\.' --lr_group 'hg\\.1\\.:0.1' (utils.optim.group_specs on the net's table)
  adversarial        chunk c in group c % 16, no group frozen: neighbouring lanes never share a group
Same process, HIP events around `calls` back-to-back calls of one variant, every variant warmed first, the variants interleaved over
`rounds` rounds (tools/bench_optim.py's method: the arrays partly stay in the last-level cache back to back, so these are relative
costs).  GB/s = the bytes the step must move over the live (not frozen) elements, plus one byte per four elements for the map, over
the median.  Also recorded, as information: whether a 16-group call whose groups all carry the same lr and weight_decay gives the bits of the
ungrouped call (the compiler may contract the shared update function differently in a second kernel)."""
import argparse
import ctypes as C
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

LR, ALPHA, EPS, MOM, WD = 2.5e-4, 0.99, 1e-8, 0.9, 1e-4
A_LR, A_WD = 1e-3, 1e-2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'param_groups.txt'))
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--calls', type=int, default=200)
    args = ap.parse_args()
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    from pose_adv_aug_amd.utils import optim
    torch.cuda.set_device(0)
    L = lib()
    net = create_hg(2, 1, 16, 256, default_batch=1)
    net._ensure_table()
    n = net.flat_params.numel()
    chunks = (n + 3) // 4

    def table(groups):
        tab = (_lib.OptGroup * len(groups))()
        for k, (lr, wd, frozen) in enumerate(groups):
            tab[k].lr, tab[k].weight_decay, tab[k].frozen = lr, wd, int(frozen)
        return tab

    # the realistic layout: the command line's groups on the net's own table, through the optimizer class (which builds the map)
    cmd = types.SimpleNamespace(optimizer='adamw', no_decay_1d=1, freeze=r'^(conv1|bn1|residual[123])\.', lr_group=[r'hg\.1\.:0.1'], weight_decay=A_WD)
    o = optim.make_optimizer(cmd, net, A_LR)
    real_map = o._map
    real_desc = o.describe_groups()
    real_groups = [(g['lr_mult'], bool(g['weight_decay']), g['frozen']) for g in o.param_groups]
    real = lambda lr, wd: [(lr * mult, wd if decays else 0.0, frozen) for mult, decays, frozen in real_groups]
    frozen_floats = sum(4 for k in real_map.tolist() if real_groups[k][2])
    adv_map = (torch.arange(chunks, device='cuda') % 16).to(torch.uint8)
    adv = lambda lr, wd: [(lr * (1.0 if k % 3 else 0.1), wd if k % 2 else 0.0, False) for k in range(16)]
    same = lambda lr, wd: [(lr, wd, False)] * 16
    del net, o

    g = torch.Generator(device='cuda').manual_seed(1)
    grads = [torch.randn(n, device='cuda', generator=g) * 1e-3 for _ in range(4)]
    p0 = torch.randn(n, device='cuda', generator=g) * 0.05
    p, v, buf, x = (torch.zeros(n, device='cuda') for _ in range(4))          # buf: momentum_buffer / exp_avg; x: grad_avg / max_exp_avg_sq
    skip = torch.zeros(2, dtype=torch.int32, device='cuda')
    state = torch.zeros(8, dtype=torch.int32, device='cuda')
    consts = torch.zeros(16, device='cuda')
    ws = torch.empty(int(L.pa_grad_norm_workspace_bytes(n)) // 8, dtype=torch.float64, device='cuda')
    out2 = torch.zeros(2, device='cuda')

    def reset():
        p.copy_(p0)
        for a in (v, buf, x, state, skip):
            a.zero_()

    ro = _lib.RmspropOpts(LR, ALPHA, EPS, MOM, WD, 1)
    ao = _lib.AdamOpts(A_LR, 0.9, 0.999, 1e-8, A_WD, 1, 1)

    def norm_call(gk, cmap, mask):
        if mask:
            check(L.pa_grad_norm_groups(ptr(gk), n, ptr(cmap), mask, 1.0, 0.01, ptr(ws), ptr(out2), stream()))
        else:
            check(L.pa_grad_norm(ptr(gk), n, 1.0, 0.01, ptr(ws), ptr(out2), stream()))

    def rms(groups, cmap, norm):
        tab = None if groups is None else table(groups)
        mask = 0 if groups is None else sum(1 << k for k, gr in enumerate(groups) if gr[2])

        def call(k):
            gk = grads[k % 4]
            if norm:
                norm_call(gk, cmap, mask)
            coef = ptr(out2[1:]) if norm else None
            if tab is None:
                check(L.pa_rmsprop_step_opts(C.byref(ro), ptr(p), ptr(gk), ptr(v), ptr(buf), ptr(x), n, 1.0, coef, ptr(skip), stream()))
            else:
                check(L.pa_rmsprop_step_groups(C.byref(ro), tab, len(groups), None if cmap is None else ptr(cmap), ptr(p), ptr(gk), ptr(v), ptr(buf),
                                               ptr(x), n, 1.0, coef, ptr(skip), stream()))
        return call

    def adam(groups, cmap, norm):
        tab = None if groups is None else table(groups)
        mask = 0 if groups is None else sum(1 << k for k, gr in enumerate(groups) if gr[2])

        def call(k):
            gk = grads[k % 4]
            if norm:
                norm_call(gk, cmap, mask)
            coef = ptr(out2[1:]) if norm else None
            if tab is None:
                check(L.pa_adam_step(C.byref(ao), ptr(p), ptr(gk), ptr(buf), ptr(v), ptr(x), n, 1.0, coef, ptr(state), stream()))
            else:
                check(L.pa_adam_step_groups(C.byref(ao), tab, len(groups), None if cmap is None else ptr(cmap), ptr(consts), ptr(p), ptr(gk), ptr(buf),
                                            ptr(v), ptr(x), n, 1.0, coef, ptr(state), stream()))
        return call

    variants = []
    for kind, make, lr, wd in (('RMSprop(momentum, weight_decay, centered)', rms, LR, WD), ('AdamW(amsgrad)', adam, A_LR, A_WD)):
        for norm in (False, True):
            tag = '%s%s' % (kind, ' + norm, clip' if norm else '')
            for layout, groups, cmap, live in (('ungrouped', None, None, n), ('one group', [(lr, wd, False)], None, n),
                                               ('realistic', real(lr, wd), real_map, n - frozen_floats), ('adversarial', adv(lr, wd), adv_map, n)):
                floats = (9 + norm) * live
                variants.append(('%-52s %s' % (tag, layout), make(groups, cmap, norm), floats * 4 + (0 if cmap is None else chunks * (1 + norm)), kind + str(norm)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = dict((name, []) for name, _, _, _ in variants)
    for r in range(args.rounds + 1):            # round 0 warms every variant and is not counted
        for name, call, _, _ in variants:
            reset()
            call(0)
            e0.record()
            for k in range(args.calls):
                call(k)
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)
            if not bool(torch.isfinite(p).all()):
                raise RuntimeError('non-finite parameters after %s' % name)
    # information: 16 groups that all carry the optimizer's values against the ungrouped call, one step from the same state
    same_bits = []
    for kind, make, lr, wd in (('RMSprop', rms, LR, WD), ('AdamW', adam, A_LR, A_WD)):
        outs = []
        for groups, cmap in ((None, None), (same(lr, wd), adv_map)):
            reset()
            v.fill_(1e-6)
            make(groups, cmap, True)(0)
            torch.cuda.synchronize()
            outs.append([a.clone().view(torch.int32) for a in (p, v, buf, x)])
        diff = [int((a != b).sum()) for a, b in zip(*outs)]
        same_bits.append('%s, 16 groups with the optimizer\'s own lr and weight_decay against the ungrouped call, one step: %s' % (
            kind, 'bit for bit the same' if not any(diff) else 'elements that differ in p / second moment / first moment or buffer / third array: %s of %d' % (diff, n)))
    lines = ['parameter groups in the fused optimizer steps on n = %d floats (2-stack chan-256 pose net), %s build, %s' % (n, _lib.DTYPE, torch.cuda.get_device_name(0)),
             'HIP events around %d back-to-back calls, %d interleaved rounds after one warm-up round; us per step: median (min .. max)' % (args.calls, args.rounds),
             'bytes = 9 floats (+ 1 for the norm) per live element + 1 byte per chunk of 4 elements for the map (+ 1 for the grouped norm); GB/s = bytes / median;',
             'x ungrouped = median / median of the ungrouped row of the same optimizer and clipping in this run',
             'realistic layout: %d of %d floats frozen; %s' % (frozen_floats, n, '; '.join(real_desc)),
             '%-66s %8s %20s %12s %8s %11s' % ('variant', 'us', '(min .. max)', 'bytes', 'GB/s', 'x ungrouped')]
    base = {}
    for name, _, nbytes, key in variants:
        t = np.array(times[name])
        med = float(np.median(t))
        base.setdefault(key, med)
        lines.append('%-66s %8.2f %20s %12d %8.0f %11.3f' % (name, med, '(%.2f .. %.2f)' % (t.min(), t.max()), nbytes, nbytes / med / 1e3, med / base[key]))
    lines += same_bits
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fd:
        fd.write(text)


if __name__ == '__main__':
    main()
