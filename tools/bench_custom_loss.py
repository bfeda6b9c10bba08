#!/usr/bin/env python3
"""What a loss of your own costs beside the built-in one (profiles/custom_loss.txt), at the benchmark configuration (2 stacks, chan 256,
B 24, 256 x 256):

    python tools/bench_custom_loss.py [--out profiles/custom_loss.txt] [--rounds 8] [--steps 20] [--note 'line to append' ...]

  * ms/step of loss_and_backward (the fused MSE step: forward, loss in the head kernel, backward) and of forward_autograd +
    Criterion.weighted_L2(w = 1) per stack + loss.backward() (the same loss through torch.autograd and pa_hg_set_heat_grads); HIP
    events around `steps` back-to-back steps, the two interleaved over `rounds` rounds after a warm-up round; no optimizer step;
  * from ONE `rocprofv3 --kernel-trace --stats` run (no counters) of a child process (this file with --trace-child): the time per launch
    of heat_inject_nchw_kernel and heat_inject_nhwc_kernel beside heat_grad_kernel's, and of weighted_l2_kernel / weighted_l2_grad_kernel.
All three move the same bytes per pixel (64 B of fp32 in, 32 B of addend in for the inner stack, 32 B out)."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

STACKS, CHAN, B, RES = 2, 256, 24, 256
KERNELS = ('heat_grad_kernel', 'heat_inject_nchw_kernel', 'heat_inject_nhwc_kernel', 'weighted_l2_kernel', 'weighted_l2_grad_kernel', 'head_fwd_kernel')


def setup():
    from pose_adv_aug_amd.data import Augmenter, DeviceBatch
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    from pose_adv_aug_amd.pylib import Criterion, HumanPts
    torch.cuda.set_device(0)
    net = create_hg(STACKS, 1, 16, CHAN, res=RES, default_batch=B)
    net.reset_parameters(seed=1)
    net.train()
    data = Augmenter(seed=1234, inp_res=RES, out_res=RES // 4).regular(DeviceBatch.synthetic(B, seed=0))
    target = HumanPts.pts2heatmap_batch(data['pts'], RES // 4, RES // 4)

    def builtin():
        net.loss_and_backward(img4=data['img4'], pts=data['pts'])

    def custom():
        outs = net.forward_autograd(img4=data['img4'])
        sum(Criterion.weighted_L2(o, target, 1) for o in outs).backward()

    def custom_nhwc():          # the same gradients handed over joint-minor (the autograd path delivers them planar)
        outs = net.forward(img4=data['img4'])
        n = outs[0].numel()
        net.backward([(2 * (o - target) / n).permute(0, 2, 3, 1).contiguous() for o in outs], layout='nhwc')
    return builtin, custom, custom_nhwc


def trace_child():
    fns = setup()
    for _ in range(6):
        for f in fns:
            f()
    torch.cuda.synchronize()


def kernel_table():
    """{kernel: (calls, average us, min us, max us)} of one traced child run"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'cl', '--', sys.executable, os.path.abspath(__file__), '--trace-child']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if r.returncode != 0 or not files:
            raise RuntimeError('the traced child failed: %s' % (r.stdout + r.stderr)[-2000:])
        out = {}
        for row in csv.DictReader(open(files[0])):
            for k in KERNELS:
                if row['Name'].split('(')[0].split('<')[0].strip().endswith(k):
                    c, t, lo, hi = out.get(k, (0, 0.0, float('inf'), 0.0))
                    out[k] = (c + int(row['Calls']), t + float(row['TotalDurationNs']), min(lo, float(row.get('MinNs') or row['AverageNs'])),
                              max(hi, float(row.get('MaxNs') or row['AverageNs'])))
        return {k: (c, t / c / 1e3, lo / 1e3, hi / 1e3) for k, (c, t, lo, hi) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'custom_loss.txt'))
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--note', action='append', default=[], help='a line appended to the file (e.g. the bench.py lines of the two trees)')
    ap.add_argument('--trace-child', action='store_true')
    args = ap.parse_args()
    if args.trace_child:
        return trace_child()
    table = kernel_table()                      # first: the child has the device to itself
    from pose_adv_aug_amd import _lib
    builtin, custom, _ = setup()
    variants = [('loss_and_backward (built-in MSE)', builtin), ('forward_autograd + weighted_L2(w=1) per stack + backward', custom)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = dict((name, []) for name, _ in variants)
    for r in range(args.rounds + 1):            # round 0 warms up and is not counted
        for name, step in variants:
            step()
            e0.record()
            for _ in range(args.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[name].append(e0.elapsed_time(e1) / args.steps)
    M = B * (RES // 4) ** 2
    lines = ['a loss of your own beside the built-in one: %d stacks, chan %d, B %d, %d x %d, %s build, %s' % (STACKS, CHAN, B, RES, RES, _lib.DTYPE, torch.cuda.get_device_name(0)),
             'forward + loss + backward, no optimizer step; HIP events around %d back-to-back steps, %d interleaved rounds after one warm-up round' % (args.steps, args.rounds),
             '%-60s %9s %20s' % ('step', 'ms/step', '(min .. max)')]
    for name, _ in variants:
        t = np.array(times[name])
        lines.append('%-60s %9.3f %20s' % (name, float(np.median(t)), '(%.3f .. %.3f)' % (t.min(), t.max())))
    lines += ['', 'per launch, one rocprofv3 --kernel-trace --stats run (no counters) of 6 x (built-in step, autograd step, nhwc backward):',
              'bytes by design per launch of the three gradient kernels: %.2f MB (last stack) / %.2f MB (inner stack)' % (M * 96 / 1e6, M * 128 / 1e6),
              '%-28s %7s %9s %20s' % ('kernel', 'calls', 'avg us', '(min .. max)')]
    for k in KERNELS:
        if k in table:
            c, avg, lo, hi = table[k]
            lines.append('%-28s %7d %9.2f %20s' % (k, c, avg, '(%.2f .. %.2f)' % (lo, hi)))
        else:
            lines.append('%-28s %7s' % (k, 'absent'))
    lines += [''] + args.note if args.note else []
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fd:
        fd.write(text)


if __name__ == '__main__':
    main()
