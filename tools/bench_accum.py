#!/usr/bin/env python3
"""What gradient accumulation costs (profiles/grad_accum.txt).

    python tools/bench_accum.py [--out profiles/grad_accum.txt] [--rounds 20] [--calls 200] [--iters 32] [--bs 24]

1. The launches alone, on arrays of the size of the flat gradient of the benchmark net (2 stacks, chan 256) and of the 8-stack 384 x 384
   net: the copy form (accumulate() of a group's first micro-batch; 8 bytes per element: read the gradient, write the sum), the
   in-place addition (accumulate() of the later ones) and the fold of step() (flat_grads = _acc + flat_grads), 12 bytes per element each.
   HIP events around `calls` back-to-back calls of one variant, every variant warmed first, the variants interleaved over `rounds` rounds
   (median and spread).  Beside them pa_copy_probe -- the copy kernel of bench.py's roofline floor -- moving the same number of bytes
   (half read, half written) in the same process.  Back to back the two arrays of the benchmark net (53 MB) stay in the 256 MiB
   last-level cache, as they do not behind a training step's other traffic: the copy probe beside it is measured the same way.  At the
   8-stack size the footprints differ: an addition in place touches TWO arrays (2 x 102 MB, inside the cache) for its 12 bytes per
   element, the probe moving the same bytes reads 153 MB and writes another 153 MB (beyond it).
2. The loop of stack_hg (stack_hg.train over `iters` synthetic MPII-shape batches of `bs`, RMSprop, the next batch's augmentation one
   step ahead) with --accum_steps 1, 2 and 4: whole calls of train(), alternating over `rounds` rounds in one process, a host clock
   around each call (it ends in the host read of the meters); ms per ITERATION, i.e. per micro-batch."""
import argparse
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def launches(args, what, n, lines):
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    L = lib()
    g = torch.Generator(device='cuda').manual_seed(1)
    grads, acc = torch.randn(n, device='cuda', generator=g) * 1e-3, torch.zeros(n, device='cuda')
    src, dst = torch.randn(3 * n // 2 + 16, device='cuda', generator=g), torch.empty(3 * n // 2 + 16, device='cuda')
    first = lambda: check(L.pa_grad_accumulate(ptr(acc), ptr(grads), None, n, stream()))
    later = lambda: check(L.pa_grad_accumulate(ptr(acc), ptr(acc), ptr(grads), n, stream()))
    fold = lambda: check(L.pa_grad_accumulate(ptr(grads), ptr(acc), ptr(grads), n, stream()))

    def copy(per_elem):         # pa_copy_probe moving per_elem bytes per element in all
        nbytes = n * per_elem // 2 // 16 * 16
        return lambda: check(L.pa_copy_probe(ptr(dst), ptr(src), nbytes, stream()))

    def settle():               # every block starts from _acc = 0: the fold then leaves the gradient as it is, and the in-place addition ends
        acc.zero_()             # at (calls + 1) g, so the values stay finite over any number of rounds

    variants = [('accumulate(), first of a group: _acc = g', first, 8), ('pa_copy_probe, the same bytes', copy(8), 8),
                ('accumulate(), later ones: _acc = _acc + g', later, 12), ('step(): flat_grads = _acc + flat_grads', fold, 12),
                ('pa_copy_probe, the same bytes', copy(12), 12)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = [[] for _ in variants]
    for r in range(args.rounds + 1):            # round 0 warms every variant and is not counted
        for k, (name, call, _) in enumerate(variants):
            settle()
            call()
            e0.record()
            for _ in range(args.calls):
                call()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1) * 1e3 / args.calls)
    if not bool(torch.isfinite(grads).all() and torch.isfinite(acc).all()):
        raise RuntimeError('non-finite gradient')
    lines += ['', '%s: %d floats' % (what, n), '%-48s %8s %20s %6s %10s %8s' % ('variant', 'us', '(min .. max)', 'B/elem', 'bytes', 'GB/s')]
    for (name, _, per_elem), t in zip(variants, times):
        t = np.array(t)
        med = float(np.median(t))
        lines.append('%-48s %8.2f %20s %6d %10d %8.0f' % (name, med, '(%.2f .. %.2f)' % (t.min(), t.max()), per_elem, per_elem * n, per_elem * n / med / 1e3))


def loop(args, net, lines):
    from pose_adv_aug_amd import stack_hg
    from pose_adv_aug_amd.data import Augmenter, DeviceBatch
    from pose_adv_aug_amd.utils.optim import RMSprop
    B = args.bs
    aug = Augmenter(seed=100)
    two = [DeviceBatch.synthetic(B, seed=k) for k in range(2)]
    batches = [two[i % 2] for i in range(args.iters)]
    opts = dict((N, RMSprop(net, lr=2.5e-4, alpha=0.99, eps=1e-8)) for N in (1, 2, 4))          # (one net: one optimizer at a time steps it)
    quiet = lambda m: None
    times = dict((N, []) for N in opts)
    order = [1, 2, 4]
    for r in range(args.rounds + 1):            # round 0 warms every setting and is not counted
        for N in order:
            o = types.SimpleNamespace(print_freq=10 ** 9, accum_steps=N, bs=B)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stack_hg.train(batches, net, opts[N], aug, 0, o, log=quiet)
            torch.cuda.synchronize()
            if r:
                times[N].append((time.perf_counter() - t0) * 1e3 / args.iters)
        order = order[1:] + order[:1]
    if any(opts[N].steps != (args.rounds + 1) * (args.iters // N) for N in opts) or not bool(torch.isfinite(net.flat_params).all()):
        raise RuntimeError('the optimizers did not take the steps of the plan')
    lines += ['', '2. stack_hg.train over %d batches of %d (RMSprop, augmentation one step ahead) with --accum_steps 1, 2 and 4: whole calls, the order '
              'rotating over %d rounds' % (args.iters, B, args.rounds), '   after one warm-up round, host clock around a call; ms per iteration (micro-batch): median (min .. max)']
    base = float(np.median(times[1]))
    for N in (1, 2, 4):
        t = np.array(times[N])
        med = float(np.median(t))
        lines.append('%-48s %8.3f %20s %8.1f img/s  %+7.1f us against --accum_steps 1' % ('--accum_steps %d (%d optimizer steps)' % (N, args.iters // N), med,
                                                                                    '(%.3f .. %.3f)' % (t.min(), t.max()), B * 1e3 / med, (med - base) * 1e3))
    t = np.array(times[1])
    lines.append('spread of the --accum_steps 1 calls: %.1f us per iteration' % ((t.max() - t.min()) * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'grad_accum.txt'))
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--iters', type=int, default=32, help='batches per call of stack_hg.train (a multiple of 4)')
    ap.add_argument('--bs', type=int, default=24)
    args = ap.parse_args()
    if args.iters % 4:
        ap.error('--iters must be a multiple of 4')
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    _lib.require_gpu()
    torch.cuda.set_device(0)
    net = create_hg(2, 1, 16, 256, default_batch=args.bs)
    net.reset_parameters(seed=0)
    big = create_hg(8, 1, 16, 256, res=384, default_batch=1)          # (only the size of its flat gradient is used)
    big._ensure_table()
    n_big = big.flat_grads.numel()
    del big
    lines = ['gradient accumulation (pa_grad_accumulate), %s build, %s' % (_lib.DTYPE, torch.cuda.get_device_name(0)), '',
             '1. the launches alone: HIP events around %d back-to-back calls, %d interleaved rounds after one warm-up round; us per call: median (min .. max)'
             % (args.calls, args.rounds), '   GB/s = bytes / median; pa_copy_probe moves the same bytes, half read and half written']
    launches(args, 'the benchmark net (2 stacks, chan 256)', net.flat_grads.numel(), lines)
    launches(args, 'the 8-stack 384 x 384 net', n_big, lines)
    loop(args, net, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fd:
        fd.write(text)


if __name__ == '__main__':
    main()
