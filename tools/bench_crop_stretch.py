"""The staged crop with and without the stretch mode, on the benchmark's batch and with the warm and cold loops of
tools/bench_crop.py, alternated in ONE process so that all figures see the same machine state:

    python tools/bench_crop_stretch.py [--parent LIB] [--rounds N] [--out FILE]

  parent pa_crop   LIB = a libposeadv_hip.so built from the commit to compare against (left out without --parent)
  pa_crop          this tree's default path
  pa_crop_stretch  this tree's stretch mode

A round times each of them once, warm (50 back-to-back calls, wall clock) and cold (20 calls, 640 MB of other traffic in
front of each, event pairs); the spread of one variant against itself over the rounds is what a difference between two
variants has to be read against."""
import argparse, ctypes, os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pose_adv_aug_amd._lib import lib, ptr, stream
from pose_adv_aug_amd.data import Augmenter, DeviceBatch

ap = argparse.ArgumentParser()
ap.add_argument('--parent', default='')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--out', default='')
args = ap.parse_args()

batch = DeviceBatch.synthetic(24, seed=0)
Augmenter(seed=1).regular(batch)
p = batch.params
B, Hs, Ws, res = batch.B, batch.Hs, batch.Ws, 256
lines = ['pre-downscale samples: %d of 24, rotated: %d' % (int((p[:, 2] * 200 / 256 >= 2).sum()), int((p[:, 3] != 0).sum()))]
out4 = torch.empty((B, res, res, 4), dtype=torch.bfloat16, device='cuda')
need = int(lib().pa_crop_stretch_workspace_bytes(B, Hs, Ws, res))
lines.append('workspace: pa_crop %d bytes, pa_crop_stretch %d bytes' % (int(lib().pa_crop_workspace_bytes(B, Hs, Ws, res)), need))
ws = torch.empty(need, dtype=torch.uint8, device='cuda')


def caller(fn):
    fn.restype = ctypes.c_int
    return lambda: fn(ptr(batch.frames), Hs, Ws, None, ptr(p), B, res, ptr(ws), ptr(out4), None, None, stream())


variants = []
if args.parent:
    parent = ctypes.CDLL(os.path.abspath(args.parent), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    variants.append(('parent pa_crop', caller(parent.pa_crop)))
variants += [('pa_crop', caller(lib().pa_crop)), ('pa_crop_stretch', caller(lib().pa_crop_stretch))]
scratch = torch.empty(640 << 20, dtype=torch.uint8, device='cuda')


def warm(call):
    for _ in range(5):
        assert call() == 0
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(50):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / 50 * 1e6


def cold(call):
    tot = 0.0
    for i in range(20):
        scratch.fill_(i & 1)
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        tot += e0.elapsed_time(e1)
    return tot / 20 * 1e3


got = {name: ([], []) for name, _ in variants}
for r in range(args.rounds):
    for name, call in variants:
        w, c = warm(call), cold(call)
        got[name][0].append(w); got[name][1].append(c)
        lines.append('round %d  %-16s warm %7.1f us   cold %7.1f us   per batch of 24' % (r, name, w, c))
for name, (w, c) in got.items():
    lines.append('%-16s warm min %.1f max %.1f   cold min %.1f max %.1f us' % (name, min(w), max(w), min(c), max(c)))
print('\n'.join(lines))
if args.out:
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
