#!/usr/bin/env python3
"""What the weight EMA costs (profiles/ema.txt), on the 2-stack chan-256 pose net (6 570 784 parameters and its BatchNorm buffers).

    python tools/bench_ema.py [--out profiles/ema.txt] [--rounds 20] [--calls 200] [--steps 30] [--bs 24]

1. The launches alone: the prologue (pa_ema_advance), the lerp over the parameters, the lerp over the buffers, and the three as
   ModelEma.update() issues them.  HIP events around `calls` back-to-back calls of one variant, every variant warmed first, the variants
   interleaved over `rounds` rounds (median and spread).  A lerp moves 12 bytes per element by design (reads the average and the
   parameter, writes the average); beside it pa_copy_probe -- the copy kernel of bench.py's roofline floor -- moving the same number
   of bytes (half read, half written) in the same process.  Back to back the three arrays (79 MB) stay in the 256 MiB last-level cache,
   as they do not behind a training step's other traffic: the copy probe beside it is measured the same way.
2. The shipped step (stack_hg.train_step on synthetic MPII-shape people, batch `bs`, RMSprop, the next batch's augmentation one step
   ahead, as bench.py runs it) with the EMA off and on: blocks of `steps` steps, off and on alternating over `rounds` rounds in one
   process, a host clock around each block that ends in a device synchronise."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def launches(args, net, lines):
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    L = lib()
    n, nb = net.flat_params.numel(), net.flat_buffers.numel()
    g = torch.Generator(device='cuda').manual_seed(1)
    p, e = torch.randn(n, device='cuda', generator=g) * 0.05, torch.randn(n, device='cuda', generator=g) * 0.05
    bp, be = torch.rand(nb, device='cuda', generator=g), torch.rand(nb, device='cuda', generator=g)
    state = torch.zeros(8, dtype=torch.int32, device='cuda')
    flag = torch.zeros(2, dtype=torch.int32, device='cuda')
    src, dst = torch.randn(3 * n // 2 + 16, device='cuda', generator=g), torch.empty(3 * n // 2 + 16, device='cuda')
    advance = lambda: check(L.pa_ema_advance(ptr(state), 0.999, 0, ptr(flag), stream()))
    lerp_p = lambda: check(L.pa_ema_lerp(ptr(e), ptr(p), n, ptr(state), 0, stream()))
    lerp_b = lambda: check(L.pa_ema_lerp(ptr(be), ptr(bp), nb, ptr(state), 0, stream()))

    def update():
        advance(); lerp_p(); lerp_b()

    def copy(elems):            # pa_copy_probe moving 12 bytes per element in all
        nbytes = elems * 12 // 2 // 16 * 16
        return lambda: check(L.pa_copy_probe(ptr(dst), ptr(src), nbytes, stream()))

    variants = [('prologue alone (pa_ema_advance)', advance, 0), ('lerp over the parameters (%d floats)' % n, lerp_p, n),
                ('lerp over the buffers (%d floats)' % nb, lerp_b, nb), ('ModelEma.update(): prologue + both lerps', update, n + nb),
                ('pa_copy_probe, the bytes of the parameter lerp', copy(n), n), ('pa_copy_probe, the bytes of the buffer lerp', copy(nb), nb)]
    advance()                   # apply = 1: the lerp launches do their work
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = dict((name, []) for name, _, _ in variants)
    for r in range(args.rounds + 1):            # round 0 warms every variant and is not counted
        for name, call, _ in variants:
            call()
            e0.record()
            for _ in range(args.calls):
                call()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)
    if not bool(torch.isfinite(e).all()):
        raise RuntimeError('non-finite average')
    lines += ['1. the launches alone: HIP events around %d back-to-back calls, %d interleaved rounds after one warm-up round; us per call: median (min .. max)'
              % (args.calls, args.rounds),
              '   bytes = 12 per element (read average, read parameter, write average); GB/s = bytes / median',
              '%-56s %8s %20s %10s %8s' % ('variant', 'us', '(min .. max)', 'bytes', 'GB/s')]
    for name, _, elems in variants:
        t = np.array(times[name])
        med = float(np.median(t))
        rate = '%10d %8.0f' % (12 * elems, 12.0 * elems / med / 1e3) if elems else ''
        lines.append('%-56s %8.2f %20s %s' % (name, med, '(%.2f .. %.2f)' % (t.min(), t.max()), rate))


def shipped_step(args, net, lines):
    from pose_adv_aug_amd.data import AugmentAhead, Augmenter, DeviceBatch
    from pose_adv_aug_amd.stack_hg import train_step
    from pose_adv_aug_amd.utils.optim import ModelEma, RMSprop
    B = args.bs
    opt = RMSprop(net, lr=2.5e-4, alpha=0.99, eps=1e-8)
    ema = ModelEma(net, decay=0.999)
    aug = Augmenter(seed=100)
    batches = [DeviceBatch.synthetic(B, seed=k) for k in range(2)]
    ahead = AugmentAhead(aug)
    net.train()

    def run(n, which):
        ahead.start(batches[0])
        for i in range(n):
            data = ahead.take()
            ahead.start(batches[(i + 1) % 2] if i + 1 < n else None)
            train_step(net, opt, aug, batches[i % 2], data=data, ema=which)

    times = {'off': [], 'on': []}
    for r in range(args.rounds + 1):            # round 0 warms both and is not counted
        for name, which in (('off', None), ('on', ema)) if r % 2 else (('on', ema), ('off', None)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(args.steps, which)
            torch.cuda.synchronize()
            if r:
                times[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    if ema.updates() != (args.rounds + 1) * args.steps or not bool(torch.isfinite(ema.module.flat_params).all()):
        raise RuntimeError('the EMA did not follow every step')
    off, on = np.array(times['off']), np.array(times['on'])
    lines += ['', '2. the shipped step (stack_hg.train_step, batch %d, RMSprop, augmentation one step ahead) with the EMA off and on: blocks of %d steps,'
              % (B, args.steps), '   off / on alternating (the order swaps every round) over %d rounds after one warm-up round, host clock around a block '
              'that ends in a device synchronise; ms per step: median (min .. max)' % args.rounds]
    for name, t in (('EMA off', off), ('EMA on (decay 0.999, buffers averaged)', on)):
        lines.append('%-56s %8.3f %20s %8.1f img/s' % (name, float(np.median(t)), '(%.3f .. %.3f)' % (t.min(), t.max()), B * 1e3 / float(np.median(t))))
    d = float(np.median(on)) - float(np.median(off))
    lines.append('difference of the medians: %+.1f us per step (%+.2f %%); spread of the off blocks: %.1f us'
                 % (d * 1e3, 100.0 * d / float(np.median(off)), (off.max() - off.min()) * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'ema.txt'))
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--bs', type=int, default=24)
    args = ap.parse_args()
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    _lib.require_gpu()
    torch.cuda.set_device(0)
    net = create_hg(2, 1, 16, 256, default_batch=args.bs)
    net.reset_parameters(seed=0)
    lines = ['weight EMA on the 2-stack chan-256 pose net (%d parameters in %d floats, %d buffer floats), %s build, %s'
             % (net.num_params(), net.flat_params.numel(), net.flat_buffers.numel(), _lib.DTYPE, torch.cuda.get_device_name(0)), '']
    launches(args, net, lines)
    shipped_step(args, net, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fd:
        fd.write(text)


if __name__ == '__main__':
    main()
