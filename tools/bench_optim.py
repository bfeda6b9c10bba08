#!/usr/bin/env python3
"""What the optimizer's options cost (profiles/optim_variants.txt): the plain step (pa_rmsprop_step_state) and pa_rmsprop_step_opts under
each of the eight combinations of momentum / weight decay / centered, without and with the gradient norm + clip coefficient in front
(pa_grad_norm), on flat arrays of the 2-stack chan-256 pose net's parameter count.

    python tools/bench_optim.py [--out profiles/optim_variants.txt] [--rounds 20] [--calls 200]

Same process, HIP events around `calls` back-to-back calls of one variant, every variant warmed first, the variants interleaved over
`rounds` rounds (median and spread per variant, each compared with the plain entry of the same run).  Back to back the arrays of one step
(5 to 10 n floats, n = 6.57 M) partly stay in the last-level cache, as they do not behind a training step's other traffic: these are
relative costs.  Effective GB/s = the bytes the algorithm must move (plain: read p, g, v, write p, v = 5 n floats; + 2 n for the momentum
buffer, + 2 n for grad_avg, + n for the norm's read of g) over the time.  Four gradient arrays are used in turn, so that the centered
variance stays away from 0 and the values stay finite over the thousands of steps of a run.

    python tools/bench_optim.py --adam [--out profiles/adam_variants.txt]

times the Adam step (pa_adam_step: Adam, Adam with amsgrad, AdamW behind pa_grad_norm) beside RMSprop() and RMSprop(momentum=0.9) in the
same process and the same way.  Plain Adam moves the seven streams of momentum RMSprop (reads p, g and two state arrays, writes p and
both), so that is its yardstick; each row also gives its rate as a fraction of what pa_copy_probe -- the copy kernel of bench.py's
roofline floor -- reaches back to back on the same number of bytes."""
import argparse
import ctypes as C
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

LR, ALPHA, EPS, MOM, WD = 2.5e-4, 0.99, 1e-8, 0.9, 1e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--adam', action='store_true', help='the Adam rows beside RMSprop() and RMSprop(momentum=0.9) -> profiles/adam_variants.txt')
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'adam_variants.txt' if args.adam else 'optim_variants.txt')
    if args.adam:
        return adam_main(args)
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    torch.cuda.set_device(0)
    L = lib()
    net = create_hg(2, 1, 16, 256, default_batch=1)
    net._ensure_table()
    n = net.flat_params.numel()
    del net
    g = torch.Generator(device='cuda').manual_seed(1)
    grads = [torch.randn(n, device='cuda', generator=g) * 1e-3 for _ in range(4)]
    p0 = torch.randn(n, device='cuda', generator=g) * 0.05
    p, v, buf, ga = (torch.zeros(n, device='cuda') for _ in range(4))
    state = torch.zeros(2, dtype=torch.int32, device='cuda')
    ws = torch.empty(int(L.pa_grad_norm_workspace_bytes(n)) // 8, dtype=torch.float64, device='cuda')
    out2 = torch.zeros(2, device='cuda')

    def reset():
        p.copy_(p0)
        for a in (v, buf, ga):
            a.zero_()

    def plain(k):
        check(L.pa_rmsprop_step_state(ptr(p), ptr(grads[k % 4]), ptr(v), n, LR, ALPHA, EPS, 1.0, ptr(state), stream()))

    def variant(mom, wd, centered, norm):
        o = _lib.RmspropOpts(LR, ALPHA, EPS, mom, wd, int(centered))

        def call(k):
            gk = grads[k % 4]
            if norm:
                check(L.pa_grad_norm(ptr(gk), n, 1.0, 0.01, ptr(ws), ptr(out2), stream()))
            check(L.pa_rmsprop_step_opts(C.byref(o), ptr(p), ptr(gk), ptr(v), ptr(buf) if mom > 0 else None, ptr(ga) if centered else None,
                                         n, 1.0, ptr(out2[1:]) if norm else None, ptr(state), stream()))
        return call

    variants = [('plain entry (pa_rmsprop_step_state)', plain, 5)]
    for norm in (False, True):
        for mom, wd, centered in itertools.product((0.0, MOM), (0.0, WD), (False, True)):
            name = 'opts momentum %-3g weight_decay %-6g centered %d %s' % (mom, wd, centered, 'norm+clip' if norm else '         ')
            variants.append((name, variant(mom, wd, centered, norm), 5 + 2 * (mom > 0) + 2 * centered + norm))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = dict((name, []) for name, _, _ in variants)
    for r in range(args.rounds + 1):            # round 0 warms every variant and is not counted
        for name, call, _ in variants:
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
    base = float(np.median(times[variants[0][0]]))
    lines = ['optimizer step variants on n = %d floats (2-stack chan-256 pose net), %s build, %s' % (n, _lib.DTYPE, torch.cuda.get_device_name(0)),
             'HIP events around %d back-to-back calls, %d interleaved rounds after one warm-up round; us per step: median (min .. max)' % (args.calls, args.rounds),
             'bytes = floats moved by design x 4 n; GB/s = bytes / median; x plain = median / median of the plain entry in this run',
             '%-64s %8s %20s %7s %8s %8s' % ('variant', 'us', '(min .. max)', 'floats', 'GB/s', 'x plain')]
    for name, _, floats in variants:
        t = np.array(times[name])
        med = float(np.median(t))
        lines.append('%-64s %8.2f %20s %5d n %8.0f %8.2f' % (name, med, '(%.2f .. %.2f)' % (t.min(), t.max()), floats, floats * 4.0 * n / med / 1e3, med / base))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fd:
        fd.write(text)


def adam_main(args):
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    torch.cuda.set_device(0)
    L = lib()
    net = create_hg(2, 1, 16, 256, default_batch=1)
    net._ensure_table()
    n = net.flat_params.numel()
    del net
    g = torch.Generator(device='cuda').manual_seed(1)
    grads = [torch.randn(n, device='cuda', generator=g) * 1e-3 for _ in range(4)]
    p0 = torch.randn(n, device='cuda', generator=g) * 0.05
    p, v, buf, vmax = (torch.zeros(n, device='cuda') for _ in range(4))          # buf: momentum_buffer / exp_avg
    skip = torch.zeros(2, dtype=torch.int32, device='cuda')
    state = torch.zeros(8, dtype=torch.int32, device='cuda')
    ws = torch.empty(int(L.pa_grad_norm_workspace_bytes(n)) // 8, dtype=torch.float64, device='cuda')
    out2 = torch.zeros(2, device='cuda')
    src, dst = torch.randn(5 * n, device='cuda', generator=g), torch.empty(5 * n, device='cuda')

    def reset():
        p.copy_(p0)
        for a in (v, buf, vmax, state):
            a.zero_()

    def rmsprop(mom):
        o = _lib.RmspropOpts(LR, ALPHA, EPS, mom, 0.0, 0)
        if mom == 0:
            return lambda k: check(L.pa_rmsprop_step_state(ptr(p), ptr(grads[k % 4]), ptr(v), n, LR, ALPHA, EPS, 1.0, ptr(skip), stream()))
        return lambda k: check(L.pa_rmsprop_step_opts(C.byref(o), ptr(p), ptr(grads[k % 4]), ptr(v), ptr(buf), None, n, 1.0, None, ptr(skip), stream()))

    def adam(wd, decoupled, amsgrad, norm):
        o = _lib.AdamOpts(1e-3, 0.9, 0.999, 1e-8, wd, int(amsgrad), int(decoupled))

        def call(k):
            gk = grads[k % 4]
            if norm:
                check(L.pa_grad_norm(ptr(gk), n, 1.0, 0.01, ptr(ws), ptr(out2), stream()))
            check(L.pa_adam_step(C.byref(o), ptr(p), ptr(gk), ptr(buf), ptr(v), ptr(vmax) if amsgrad else None, n, 1.0,
                                 ptr(out2[1:]) if norm else None, ptr(state), stream()))
        return call

    def copy(floats):           # pa_copy_probe moving `floats` n floats in all (half read, half written)
        nbytes = floats * n * 4 // 2 // 16 * 16
        return lambda k: check(L.pa_copy_probe(ptr(dst), ptr(src), nbytes, stream()))

    variants = [('RMSprop()                        pa_rmsprop_step_state', rmsprop(0.0), 5),
                ('RMSprop(momentum=0.9)            pa_rmsprop_step_opts', rmsprop(MOM), 7),
                ('Adam()                           prologue + pa_adam_step', adam(0.0, False, False, False), 7),
                ('Adam(amsgrad=True)', adam(0.0, False, True, False), 9),
                ('AdamW(max_grad_norm)             pa_grad_norm + decoupled decay 1e-2', adam(1e-2, True, False, True), 8)]
    variants += [('pa_copy_probe moving %d n floats' % fl, copy(fl), fl) for fl in (5, 7, 8, 9)]
    # what the launches themselves cost back to back: the same two calls on 4 floats (one launch against prologue + step launch)
    o4, a4 = _lib.RmspropOpts(LR, ALPHA, EPS, MOM, 0.0, 0), _lib.AdamOpts(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0)
    tiny = [('RMSprop(momentum=0.9) on 4 floats: one launch',
             lambda k: check(L.pa_rmsprop_step_opts(C.byref(o4), ptr(p), ptr(grads[k % 4]), ptr(v), ptr(buf), None, 4, 1.0, None, ptr(skip), stream()))),
            ('Adam() on 4 floats: prologue + step launch',
             lambda k: check(L.pa_adam_step(C.byref(a4), ptr(p), ptr(grads[k % 4]), ptr(buf), ptr(v), None, 4, 1.0, None, ptr(state), stream())))]
    variants += [(name, call, 0) for name, call in tiny]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = dict((name, []) for name, _, _ in variants)
    for r in range(args.rounds + 1):            # round 0 warms every variant and is not counted
        for name, call, _ in variants:
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
    med = dict((name, float(np.median(times[name]))) for name, _, _ in variants)
    copy_us = dict((fl, med['pa_copy_probe moving %d n floats' % fl]) for fl in (5, 7, 8, 9))
    base = med[variants[1][0]]
    lines = ['Adam step variants on n = %d floats (2-stack chan-256 pose net), %s build, %s' % (n, _lib.DTYPE, torch.cuda.get_device_name(0)),
             'HIP events around %d back-to-back calls, %d interleaved rounds after one warm-up round; us per step: median (min .. max)' % (args.calls, args.rounds),
             'bytes = floats moved by design x 4 n; GB/s = bytes / median; x mom = median / median of RMSprop(momentum=0.9) in this run;',
             'of copy = GB/s over the GB/s of pa_copy_probe (the copy kernel of bench.py\'s roofline floor) moving the same bytes the same way',
             '%-72s %8s %20s %7s %8s %8s %8s' % ('variant', 'us', '(min .. max)', 'floats', 'GB/s', 'x mom', 'of copy')]
    for name, _, floats in variants:
        t = np.array(times[name])
        if not floats:
            lines.append('%-72s %8.2f %20s' % (name, med[name], '(%.2f .. %.2f)' % (t.min(), t.max())))
            continue
        lines.append('%-72s %8.2f %20s %5d n %8.0f %8.2f %8.2f' % (name, med[name], '(%.2f .. %.2f)' % (t.min(), t.max()), floats,
                                                                   floats * 4.0 * n / med[name] / 1e3, med[name] / base, copy_us[floats] / med[name]))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fd:
        fd.write(text)


if __name__ == '__main__':
    main()
