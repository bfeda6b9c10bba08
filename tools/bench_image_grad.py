#!/usr/bin/env python3
"""What d loss / d image costs (profiles/image_grad.txt), at the benchmark configuration (2 stacks, chan 256, B 24, 256 x 256):

    python tools/bench_image_grad.py [--out profiles/image_grad.txt] [--rounds 8] [--steps 20] [--note 'line to append' ...]

  * ms/step of loss_and_backward (forward, loss, backward) with input_grad off, 'nchw' and 'nhwc4': HIP events around `steps` back-to-back
    steps, the variants interleaved over `rounds` rounds after a warm-up round; no optimizer step;
  * the launch alone through pa_stem_dgrad (dy [24][64][128][128] fp32 -> storage type, weight pack, the kernel), both layouts: HIP events
    around `steps` calls -- this includes the operator's two conversion launches;
  * from ONE `rocprofv3 --kernel-trace --stats` run (no counters) of a child process (this file with --trace-child): the time per launch of
    stem_dgrad_kernel in the step (BatchNorm backward on load: reads dz and the raw stem output) and in the operator (plain operand), with
    the bytes each moves by design and the rate that gives."""
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
KERNELS = ('stem_dgrad_kernel', 'stem_pack_kernel', 'nchw_f32_to_nhwc_bf16_kernel')


def setup():
    from pose_adv_aug_amd._lib import check, lib, ptr, stream
    from pose_adv_aug_amd.data import Augmenter, DeviceBatch
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    torch.cuda.set_device(0)
    net = create_hg(STACKS, 1, 16, CHAN, res=RES, default_batch=B)
    net.reset_parameters(seed=1)
    net.train()
    data = Augmenter(seed=1234, inp_res=RES, out_res=RES // 4).regular(DeviceBatch.synthetic(B, seed=0))
    g = torch.Generator().manual_seed(5)
    dy = torch.randn(B, 64, RES // 2, RES // 2, generator=g).cuda()
    w = (torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5).cuda()
    ws = torch.empty(lib().pa_stem_dgrad_workspace_bytes(B, RES, RES), dtype=torch.uint8, device='cuda')
    dx = torch.empty(B * RES * RES * 4, dtype=torch.float32, device='cuda')

    def step(input_grad):
        return lambda: net.loss_and_backward(img4=data['img4'], pts=data['pts'], input_grad=input_grad)

    def op(layout):
        return lambda: check(lib().pa_stem_dgrad(ptr(dy), ptr(w), ptr(dx), B, RES, RES, layout, ptr(ws), stream()), 'pa_stem_dgrad')
    return [('loss_and_backward, input_grad off', step(False)), ("loss_and_backward, input_grad 'nchw'", step('nchw')),
            ("loss_and_backward, input_grad 'nhwc4'", step('nhwc4')), ('pa_stem_dgrad layout 0 (3 launches)', op(0)),
            ('pa_stem_dgrad layout 1 (3 launches)', op(1))]


def trace_child():
    fns = setup()
    for _ in range(6):
        for _, f in fns:
            f()
    torch.cuda.synchronize()


def kernel_table():
    """{kernel name as traced: (calls, average us, min us, max us)} of one traced child run, the kernels of KERNELS"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'ig', '--', sys.executable, os.path.abspath(__file__), '--trace-child']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if r.returncode != 0 or not files:
            raise RuntimeError('the traced child failed: %s' % (r.stdout + r.stderr)[-2000:])
        out = {}
        for row in csv.DictReader(open(files[0])):
            if any(k in row['Name'] for k in KERNELS):
                name = row['Name'].replace('void ', '').split('(')[0].strip()
                out[name] = (int(row['Calls']), float(row['TotalDurationNs']) / int(row['Calls']) / 1e3,
                             float(row.get('MinNs') or row['AverageNs']) / 1e3, float(row.get('MaxNs') or row['AverageNs']) / 1e3)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'image_grad.txt'))
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--note', action='append', default=[], help='a line appended to the file (e.g. the bench.py lines of the two trees)')
    ap.add_argument('--trace-child', action='store_true')
    args = ap.parse_args()
    if args.trace_child:
        return trace_child()
    table = kernel_table()                      # first: the child has the device to itself
    from pose_adv_aug_amd import _lib
    variants = setup()
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
    M = B * (RES // 2) ** 2
    by_lin2, by_plain = M * 64 * 2 * 2 + 64 * 256 * 2, M * 64 * 2 + 64 * 256 * 2
    wr4, wr3 = B * RES * RES * 16, B * RES * RES * 12
    lines = ['d loss / d image: %d stacks, chan %d, B %d, %d x %d, %s build, %s' % (STACKS, CHAN, B, RES, RES, _lib.DTYPE, torch.cuda.get_device_name(0)),
             'forward + loss + backward, no optimizer step / the operator alone; HIP events around %d back-to-back calls, %d interleaved rounds after one warm-up round' % (args.steps, args.rounds),
             '%-44s %9s %20s' % ('call', 'ms/call', '(min .. max)')]
    for name, _ in variants:
        t = np.array(times[name])
        lines.append('%-44s %9.3f %20s' % (name, float(np.median(t)), '(%.3f .. %.3f)' % (t.min(), t.max())))
    lines += ['', 'per launch, one rocprofv3 --kernel-trace --stats run (no counters) of 6 x (the five calls above):',
              'bytes by design of stem_dgrad_kernel: in the step (dz + raw stem output, 16-bit) %.1f MB read, in the operator (plain) %.1f MB read; %.1f MB (layout 1) / %.1f MB (layout 0) written'
              % (by_lin2 / 1e6, by_plain / 1e6, wr4 / 1e6, wr3 / 1e6),
              '(<2>: BatchNorm backward on load, the step; <0>: plain operand, the operator; each instance ran both layouts)',
              '%-44s %7s %9s %20s %12s' % ('kernel', 'calls', 'avg us', '(min .. max)', 'GB/s by design')]
    for k in sorted(table):
        c, avg, lo, hi = table[k]
        rate = ''
        if 'stem_dgrad_kernel' in k:
            rd = by_lin2 if '2' in k.split('stem_dgrad_kernel')[1] else by_plain
            rate = '%.0f' % ((rd + (wr4 + wr3) / 2.0) / (avg * 1e-6) / 1e9)
        lines.append('%-44s %7d %9.2f %20s %12s' % (k, c, avg, '(%.2f .. %.2f)' % (lo, hi), rate))
    if not any('stem_dgrad_kernel' in k for k in table):
        lines.append('%-44s %7s' % ('stem_dgrad_kernel', 'absent'))
    lines += [''] + args.note if args.note else []
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fd:
        fd.write(text)


if __name__ == '__main__':
    main()
