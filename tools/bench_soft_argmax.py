#!/usr/bin/env python3
"""What the soft-arg-max operator pair costs and how exact it is (profiles/soft_argmax.txt):

    python tools/bench_soft_argmax.py [--out profiles/soft_argmax.txt] [--rounds 8] [--steps 20] [--note 'line to append' ...]
    python tools/bench_soft_argmax.py --exp-error          # only the error of the device's double exp (the one measured constant of the bound)

  * the error of the device's double exp (pa_exp_probe: the function the kernels call) on 2^21 arguments over [-745, 0] against
    numpy.longdouble: the largest relative error where the result is a normal double, the largest absolute error in units of 2^-1074
    where it is subnormal; tests/soft_argmax_exact.py uses twice these (EXP_REL, EXP_SUB);
  * the worst |error| / bound per case family of tests/soft_argmax_exact.py (the legs the GPU tests assert on);
  * ms/call, HIP events around `steps` back-to-back calls, the variants interleaved over `rounds` rounds after a warm-up round, one process:
    pa_soft_argmax and pa_soft_argmax_bwd on joint-minor maps (B 24, 64 x 64 and B 16, 96 x 96; J 16), pa_copy_probe moving the same
    bytes, the torch composition a user writes today on the NCHW copy (softmax over the flattened map, two weighted sums; autograd
    backward), and forward + loss + backward of a 2-stack chan-256 net through forward_autograd without and with the coordinate term."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = ((24, 64, 64), (16, 96, 96))
REGISTERS = ('kernel resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, both builds alike; no kernel uses scratch):',
             '  soft_argmax_nhwc16_kernel       78 VGPRs, 81 SGPRs, scratch 0, LDS 1792 B, 1024 threads',
             '  soft_argmax_bwd_nhwc16_kernel   85 VGPRs, 68 SGPRs, scratch 0, LDS 0,      256 threads',
             '  soft_argmax_kernel              50 VGPRs, 42 SGPRs, scratch 0, LDS 112 B,  256 threads',
             '  soft_argmax_bwd_kernel          40 VGPRs, 43 SGPRs, scratch 0, LDS 0,      256 threads')


def exp_error(n=1 << 21):
    """(largest relative error over normal results, largest absolute error over subnormal results in units of 2^-1074, count of
    arguments, exp(0) == 1, every argument below -746 gives 0) of the device's double exp against numpy.longdouble"""
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    if np.finfo(np.longdouble).nmant <= 52:
        raise RuntimeError('numpy.longdouble is no wider than double on this host')
    gen = np.random.Generator(np.random.PCG64(11))
    x = np.concatenate([gen.uniform(-745.0, 0.0, n), -np.arange(0.0, 746.0), -np.ldexp(1.0, -np.arange(1, 60)),
                        gen.uniform(-745.2, -708.0, n // 16)])
    far = np.array([-746.0, -750.0, -1e3, -6e4, -1e300, -6e35])
    xd = torch.from_numpy(np.concatenate([x, far])).cuda()
    yd = torch.full_like(xd, float('nan'))
    check(lib().pa_exp_probe(ptr(xd), ptr(yd), xd.numel(), stream()), 'pa_exp_probe')
    y = yd.cpu().numpy()
    want = np.exp(x.astype(np.longdouble))
    got = y[:x.size].astype(np.longdouble)
    normal = want >= np.longdouble(2.0) ** -1022
    rel = float(np.max(np.abs(got[normal] - want[normal]) / want[normal]))
    sub = float(np.max(np.abs(got[~normal] - want[~normal])) / np.longdouble(2.0) ** -1074) if (~normal).any() else 0.0
    return rel, sub, int(x.size), bool(y[n] == 1.0), bool(np.all(y[x.size:] == 0.0))


def exp_lines():
    rel, sub, n, one, zero = exp_error()
    return ['device double exp (pa_exp_probe) against numpy.longdouble, %d arguments over [-745, 0] (uniform, every integer, -2^-k, a denser leg below -708):' % n,
            '  largest relative error, normal results      %.4e  = %.3f x 2^-53' % (rel, rel * 2.0 ** 53),
            '  largest absolute error, subnormal results   %.3f x 2^-1074' % sub,
            '  exp(0) == 1: %s;  exp(x) == 0 for x in {-746, -750, -1e3, -6e4, -6e35, -1e300}: %s' % (one, zero)]


def accuracy_lines():
    from tests import soft_argmax_exact as S
    lines = ['worst |error| / bound per case family (tests/soft_argmax_exact.py; <= 1 passes; EXP_REL = %.3e, EXP_SUB = %.1f as committed there):' % (S.EXP_REL, S.EXP_SUB),
             '%-34s %12s %12s %12s' % ('family', 'coords', 'state', 'dmaps')]
    for name in S.CASES:
        fails, worst = S.operator_leg(name)
        lines.append('%-34s %12.4f %12.4f %12.4f%s' % (name, worst['coords'], worst['state'], worst['dmaps'], '   FAILS: %r' % (fails[:2],) if fails else ''))
    return lines


def torch_soft_argmax(h, beta):
    """the composition a user writes today, on [B][J][H][W]"""
    B, J, H, W = h.shape
    p = torch.softmax(beta * h.reshape(B, J, H * W), dim=2)
    idx = torch.arange(H * W, device=h.device)
    x, y = (idx % W + 1).to(h.dtype), (idx // W + 1).to(h.dtype)
    return torch.stack(((p * x).sum(2), (p * y).sum(2)), dim=2)


def operator_variants(B, H, W):
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    L = lib()
    g = torch.Generator().manual_seed(B)
    maps = (torch.randn(B, H * W, 16, generator=g) * 2).cuda()
    nchw = maps.reshape(B, H, W, 16).permute(0, 3, 1, 2).contiguous()
    dco = torch.randn(B, 16, 2, generator=g).cuda()
    coords, state = torch.empty(B, 16, 2, device='cuda'), torch.empty(B, 16, 4, dtype=torch.float64, device='cuda')
    dmaps, copy = torch.empty_like(maps), torch.empty_like(maps)
    check(L.pa_soft_argmax(ptr(maps), 1, B, 16, H, W, 1.0, ptr(coords), ptr(state), stream()))
    tag = 'B %d, %d x %d: ' % (B, H, W)

    def t_fwd():
        with torch.no_grad():
            torch_soft_argmax(nchw, 1.0)

    def t_both():
        h = nchw.detach().requires_grad_()
        (torch_soft_argmax(h, 1.0) * dco).sum().backward()

    def t_convert():
        with torch.no_grad():
            maps.reshape(B, H, W, 16).permute(0, 3, 1, 2).contiguous()
    nbytes = maps.numel() * 4
    return [(tag + 'pa_soft_argmax', lambda: check(L.pa_soft_argmax(ptr(maps), 1, B, 16, H, W, 1.0, ptr(coords), ptr(state), stream())), nbytes),
            (tag + 'pa_soft_argmax_bwd', lambda: check(L.pa_soft_argmax_bwd(ptr(maps), 1, B, 16, H, W, 1.0, ptr(state), ptr(dco), ptr(dmaps), stream())), 2 * nbytes),
            (tag + 'pa_copy_probe, the same bytes as bwd', lambda: check(L.pa_copy_probe(ptr(copy), ptr(maps), nbytes, stream())), 2 * nbytes),
            (tag + 'torch forward (NCHW copy given)', t_fwd, 0), (tag + 'torch forward + autograd backward', t_both, 0),
            (tag + 'torch NHWC -> NCHW copy (per stack)', t_convert, 0)]


def step_variants():
    from pose_adv_aug_amd.data import Augmenter, DeviceBatch
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    from pose_adv_aug_amd.pylib import Criterion
    from pose_adv_aug_amd.stack_hg import coord_criterion
    B, res = 24, 256
    net = create_hg(2, 1, 16, 256, res=res, default_batch=B)
    net.reset_parameters(seed=1)
    net.train()
    data = Augmenter(seed=1234, inp_res=res, out_res=res // 4).regular(DeviceBatch.synthetic(B, seed=0))
    with_term = coord_criterion(0.1, 1.0)

    def mse_only(outs, d):            # the criterion of coord_criterion without its coordinate term (no soft-arg-max launch at all)
        from pose_adv_aug_amd.pylib import HumanPts
        t = HumanPts.pts2heatmap_batch(d['pts'], res // 4, res // 4).permute(0, 2, 3, 1).contiguous()
        return sum(Criterion.weighted_L2(o, t, 1) for o in outs)

    def step(crit):
        return lambda: crit(net.forward_autograd(img4=data['img4'], pts=data['pts'], layout='nhwc'), data).backward()
    return [('net B 24, 2 stacks, chan 256: forward + MSE + backward (nhwc)', step(mse_only), 0),
            ('net B 24, ...: the same + 0.1 coord_L1(soft_argmax)', step(with_term), 0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'soft_argmax.txt'))
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--note', action='append', default=[], help='a line appended to the file')
    ap.add_argument('--exp-error', action='store_true', help='only measure the device exp and print')
    ap.add_argument('--no-net', action='store_true', help='leave the two whole-step rows out')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.exp_error:
        print('\n'.join(exp_lines()))
        return
    from pose_adv_aug_amd import _lib
    lines = ['soft-arg-max over heat maps: %s build, %s' % (_lib.DTYPE, torch.cuda.get_device_name(0)), ''] + exp_lines() + [''] + accuracy_lines() + ['']
    lines += list(REGISTERS) + ['']
    variants = [v for B, H, W in SHAPES for v in operator_variants(B, H, W)] + ([] if args.no_net else step_variants())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = dict((name, []) for name, _, _ in variants)
    for r in range(args.rounds + 1):            # round 0 warms up and is not counted
        for name, step, _ in variants:
            step()
            e0.record()
            for _ in range(args.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[name].append(e0.elapsed_time(e1) / args.steps)
    lines += ['HIP events around %d back-to-back calls, %d interleaved rounds after one warm-up round, one process (the torch rows include their allocations)' % (args.steps, args.rounds),
              'design bytes per launch: forward 4 B HW J read; backward the same read and written; GB/s = design bytes / median time',
              '%-66s %9s %20s %9s' % ('call', 'us/call', '(min .. max)', 'GB/s')]
    med = {}
    for name, _, nbytes in variants:
        t = np.array(times[name]) * 1e3
        med[name] = float(np.median(t))
        lines.append('%-66s %9.1f %20s %9s' % (name, med[name], '(%.1f .. %.1f)' % (t.min(), t.max()), '%.0f' % (nbytes / med[name] / 1e3) if nbytes else ''))
    lines.append('')
    for B, H, W in SHAPES:
        tag = 'B %d, %d x %d: ' % (B, H, W)
        pair, tor = med[tag + 'pa_soft_argmax'] + med[tag + 'pa_soft_argmax_bwd'], med[tag + 'torch forward + autograd backward']
        lines.append('%sHIP forward + backward %.1f us; torch composition %.1f us (+ %.1f us per stack for the NCHW copy it reads): the HIP pair is %s'
                     % (tag, pair, tor, med[tag + 'torch NHWC -> NCHW copy (per stack)'], 'FASTER, %.1f x' % (tor / pair) if pair < tor else 'NOT faster, %.2f x the time' % (pair / tor)))
        lines.append('%sbackward reaches %.0f %% of pa_copy_probe on the same bytes' % (tag, 100 * med[tag + 'pa_copy_probe, the same bytes as bwd'] / med[tag + 'pa_soft_argmax_bwd']))
    lines += ([''] + args.note) if args.note else []
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fd:
        fd.write(text)


if __name__ == '__main__':
    main()
