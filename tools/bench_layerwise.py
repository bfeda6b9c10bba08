#!/usr/bin/env python3
"""What the layer-wise optimizers cost (profiles/layerwise_optim.txt): LAMB beside AdamW, LARS with momentum and plain SGD beside RMSprop with
momentum, pa_tensor_norms beside pa_grad_norm, on the flat array of the 2-stack chan-256 pose net (the benchmark net: 6.57 M floats) with
its real tensor table, so the segment list is the one training uses.

    python tools/bench_layerwise.py [--out profiles/layerwise_optim.txt] [--rounds 20] [--calls 200] [--kernel-stats FILE]

Same process, HIP events around `calls` back-to-back calls of one variant, every variant warmed first, the variants interleaved over
`rounds` rounds; median (min .. max) per variant, as tools/bench_optim.py does.  Beside every time: the floats the design moves per element,
the rate that gives, and the time pa_copy_probe (the copy kernel of bench.py's roofline floor) needs for the same bytes in the same process
(x copy = time / that time: the byte model at the copy probe's rate).  Back to back the arrays partly stay in the last-level cache, as
they do not behind a training step's other traffic: these are relative costs.
--kernel-stats FILE: a kernel-trace statistics CSV of a run of this tool under the profiler (Name, Calls, TotalDurationNs, AverageNs, ...);
the rows of the optimizer kernels are appended as the time of each launch."""
import argparse
import csv
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'layerwise_optim.txt'))
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    torch.cuda.set_device(0)
    L = lib()
    net = create_hg(2, 1, 16, 256, default_batch=1)
    net._ensure_table()
    n = net.flat_params.numel()
    params = [t for t in net._table if t[4] == 0]
    del net
    nt = len(params)
    arr = lambda typ, v: (typ * len(v))(*v)
    offsets, numels = arr(C.c_size_t, [t[2] for t in params]), arr(C.c_size_t, [t[3] for t in params])
    group = arr(C.c_int32, [1 if len(t[1]) <= 1 else 0 for t in params])          # --no_decay_1d: the 1-D tensors in a group without decay
    nsegs = int(L.pa_opt_segments_host(offsets, numels, group, nt, n, None, 0))
    host = (_lib.OptSegment * nsegs)()
    assert int(L.pa_opt_segments_host(offsets, numels, group, nt, n, host, nsegs)) == nsegs
    segs = torch.frombuffer(host, dtype=torch.int32).clone().cuda()
    short = sum(1 for s in host if s.nfloats < _lib.OPT_SEGMENT_FLOATS)
    tab = (_lib.OptGroup * 2)()
    tab[0].lr, tab[0].weight_decay, tab[1].lr, tab[1].weight_decay = 1e-3, 1e-2, 1e-3, 0.0
    one = (_lib.OptGroup * 1)()
    one[0].lr, one[0].weight_decay = 1e-3, 1e-4

    g = torch.Generator(device='cuda').manual_seed(1)
    used = torch.zeros(n, dtype=torch.bool, device='cuda')
    for t in params:
        used[t[2]:t[2] + t[3]] = True
    grads = [torch.where(used, torch.randn(n, device='cuda', generator=g) * 1e-3, torch.zeros(n, device='cuda')) for _ in range(4)]
    p0 = torch.where(used, torch.randn(n, device='cuda', generator=g) * 0.05, torch.zeros(n, device='cuda'))
    p, v, buf = (torch.zeros(n, device='cuda') for _ in range(3))                 # buf: momentum_buffer / exp_avg
    skip = torch.zeros(2, dtype=torch.int32, device='cuda')
    state = torch.zeros(8, dtype=torch.int32, device='cuda')
    ws = torch.empty(int(L.pa_grad_norm_workspace_bytes(n)) // 8, dtype=torch.float64, device='cuda')
    lws = torch.empty(int(L.pa_opt_layer_workspace_bytes(nsegs, nt)) // 8, dtype=torch.float64, device='cuda')
    out2, norms, trust = torch.zeros(2, device='cuda'), torch.zeros(2 * nt, device='cuda'), torch.ones(nt, device='cuda')
    src, dst = torch.randn(5 * n, device='cuda', generator=g), torch.empty(5 * n, device='cuda')

    def reset():
        p.copy_(p0)
        for a in (v, buf, state):
            a.zero_()

    rms = _lib.RmspropOpts(2.5e-4, 0.99, 1e-8, 0.9, 0.0, 0)
    adamw = _lib.AdamOpts(1e-3, 0.9, 0.999, 1e-8, 1e-2, 0, 1)
    lamb = _lib.LambOpts(0.9, 0.999, 1e-6, 0.0, 0, 0)

    def lars(mom, tc, groups, ng):
        o = _lib.LarsOpts(mom, tc, 1e-8, 0, 0)
        return lambda k: check(L.pa_lars_step(C.byref(o), groups, ng, ptr(segs), nsegs, nt, ptr(p), ptr(grads[k % 4]), ptr(buf) if mom else None, n, 1.0,
                                              None, ptr(lws), ptr(norms), ptr(trust), ptr(skip), stream()), 'pa_lars_step')

    def copy(floats):           # pa_copy_probe moving `floats` n floats in all (half read, half written)
        nbytes = floats * n * 4 // 2 // 16 * 16
        return lambda k: check(L.pa_copy_probe(ptr(dst), ptr(src), nbytes, stream()))

    variants = [
        ('RMSprop(momentum=0.9)              pa_rmsprop_step_opts', lambda k: check(L.pa_rmsprop_step_opts(C.byref(rms), ptr(p), ptr(grads[k % 4]), ptr(v), ptr(buf), None, n, 1.0, None, ptr(skip), stream())), 7),
        ('SGD(momentum=0.9)                  pa_lars_step, one launch', lars(0.9, 0.0, one, 1), 5),
        ('SGD()                              pa_lars_step, one launch', lars(0.0, 0.0, one, 1), 3),
        ('LARS(momentum=0.9)                 sums + finish + step', lars(0.9, 1e-3, one, 1), 7),
        ('LARS(momentum=0.9), no_decay_1d    sums + finish + step, 2 groups', lars(0.9, 1e-3, tab, 2), 7),
        ('AdamW()                            prologue + pa_adam_step', lambda k: check(L.pa_adam_step(C.byref(adamw), ptr(p), ptr(grads[k % 4]), ptr(buf), ptr(v), None, n, 1.0, None, ptr(state), stream())), 7),
        ('LAMB()                             prologue + pass 1 + finish + pass 2', lambda k: check(L.pa_lamb_step(C.byref(lamb), one, 1, ptr(segs), nsegs, nt, ptr(p), ptr(grads[k % 4]), ptr(buf), ptr(v), n, 1.0, None, ptr(lws), ptr(norms), ptr(trust), ptr(state), stream())), 10),
        ('LAMB(), no_decay_1d                the same, 2 groups', lambda k: check(L.pa_lamb_step(C.byref(lamb), tab, 2, ptr(segs), nsegs, nt, ptr(p), ptr(grads[k % 4]), ptr(buf), ptr(v), n, 1.0, None, ptr(lws), ptr(norms), ptr(trust), ptr(state), stream())), 10),
        ('pa_grad_norm                       sums + finish', lambda k: check(L.pa_grad_norm(ptr(grads[k % 4]), n, 1.0, 0.01, ptr(ws), ptr(out2), stream())), 1),
        ('pa_tensor_norms                    sums + finish', lambda k: check(L.pa_tensor_norms(ptr(grads[k % 4]), ptr(segs), nsegs, nt, 1.0, ptr(lws), ptr(norms), stream())), 1)]
    variants += [('pa_copy_probe moving %d n floats' % fl, copy(fl), fl) for fl in (1, 3, 5, 7, 10)]
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
    copy_us = dict((fl, med['pa_copy_probe moving %d n floats' % fl]) for fl in (1, 3, 5, 7, 10))
    lines = ['layer-wise optimizer steps on n = %d floats (2-stack chan-256 pose net: %d tensors, %d segments of at most %d floats, %d of them shorter), %s build, %s'
             % (n, nt, nsegs, _lib.OPT_SEGMENT_FLOATS, short, _lib.DTYPE, torch.cuda.get_device_name(0)),
             'HIP events around %d back-to-back calls, %d interleaved rounds after one warm-up round; us per call: median (min .. max)' % (args.calls, args.rounds),
             'floats = floats moved per element by design; GB/s = floats x 4 n / median; x copy = median / median of pa_copy_probe moving the same bytes in this run',
             '%-76s %8s %20s %7s %8s %8s' % ('variant', 'us', '(min .. max)', 'floats', 'GB/s', 'x copy')]
    for name, _, floats in variants:
        t = np.array(times[name])
        lines.append('%-76s %8.2f %20s %5d n %8.0f %8.2f' % (name, med[name], '(%.2f .. %.2f)' % (t.min(), t.max()), floats,
                                                             floats * 4.0 * n / med[name] / 1e3, med[name] / copy_us[floats]))
    if args.kernel_stats and os.path.isfile(args.kernel_stats):
        lines += ['', 'time of each launch (kernel trace of a run of this tool; us, average over the calls):']
        for row in csv.DictReader(open(args.kernel_stats)):
            name = row.get('Name', '')
            if any(k in name for k in ('lamb_', 'lars_', 'tensor_', 'lw_grad', 'adam_', 'rmsprop_', 'grad_sqsum', 'grad_norm_finish', 'copy16')):
                lines.append('%-100s calls %7s  average %9.2f us' % (name[:100], row.get('Calls', '?'), float(row.get('AverageNs', 'nan')) / 1e3))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fd:
        fd.write(text)


if __name__ == '__main__':
    main()
