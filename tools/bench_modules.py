#!/usr/bin/env python3
"""What num_modules costs: the full training step of the benchmark configuration (2 stacks, chan 256, B 24, 256 x 256,
stack_hg.train_step with the augmentation one step ahead, as bench.py runs it) at num_modules 1, 2 and 3, in ONE process on one
device.  Per configuration: warm-up, then the median of the per-step HIP-event intervals over --steps steps, and the workspace
size.  The numbers are recorded, not targeted (profiles/num_modules.txt).

  python tools/bench_modules.py [--steps 60] [--warmup 15] [--modules 1,2,3] [--out profiles/num_modules.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(modules, stacks, chan, B, res, warmup, steps):
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd.data import AugmentAhead, Augmenter, DeviceBatch
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    from pose_adv_aug_amd.stack_hg import train_step
    from pose_adv_aug_amd.utils.optim import RMSprop
    net = create_hg(stacks, modules, 16, chan, res=res, default_batch=B)
    net.reset_parameters(seed=0)
    opt = RMSprop(net, lr=2.5e-4, alpha=0.99, eps=1e-8)
    aug = Augmenter(seed=100, inp_res=res, out_res=res // 4)
    batches = [DeviceBatch.synthetic(B, seed=k) for k in range(2)]
    net.train()
    ahead = AugmentAhead(aug)

    def run(n, mark=None):
        out = None
        ahead.start(batches[0])
        for i in range(n):
            data = ahead.take()
            ahead.start(batches[(i + 1) % 2] if i + 1 < n else None)
            out = train_step(net, opt, aug, batches[i % 2], data=data)
            if mark is not None:
                mark(i)
        return out
    run(warmup)
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    evs[0].record()
    loss, _, _ = run(steps, mark=lambda i: evs[i + 1].record())
    torch.cuda.synchronize()
    per = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))
    ws = _lib.lib().pa_net_workspace_bytes(net._net(B))
    return dict(modules=modules, median_ms=per[steps // 2], min_ms=per[0], p90_ms=per[(9 * steps) // 10], workspace_bytes=int(ws),
                params=net.num_params(), loss=float(loss))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=15)
    ap.add_argument('--modules', default='1,2,3')
    ap.add_argument('--stacks', type=int, default=2)
    ap.add_argument('--chan', type=int, default=256)
    ap.add_argument('--bs', type=int, default=24)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--out', default=None, help='append the table to this file')
    args = ap.parse_args()
    assert args.steps >= 50, 'the median is taken over at least 50 steps'
    torch.cuda.set_device(0)
    lines = ['# tools/bench_modules.py: %d stacks, chan %d, B %d, %d x %d; median of %d per-step event intervals after %d warm-up steps; %s'
             % (args.stacks, args.chan, args.bs, args.res, args.res, args.steps, args.warmup, torch.cuda.get_device_name(0)),
             '# num_modules  ms/step(median)  min  p90  img/s  workspace_bytes  parameters  loss(last step)']
    for m in [int(v) for v in args.modules.split(',')]:
        r = measure(m, args.stacks, args.chan, args.bs, args.res, args.warmup, args.steps)
        lines.append('%d  %.3f  %.3f  %.3f  %.1f  %d  %d  %.5f' % (m, r['median_ms'], r['min_ms'], r['p90_ms'], 1000.0 * args.bs / r['median_ms'],
                                                                 r['workspace_bytes'], r['params'], r['loss']))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(text)


if __name__ == '__main__':
    main()
