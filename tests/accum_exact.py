"""Exact check of gradient accumulation (pa_grad_accumulate, csrc/grad_accum.hip; utils.optim accumulate() / step()).

Reference.  One IEEE fp32 addition per element, and a group's sum is ((g1 + g2) + g3) + ... in the order of the calls: numpy float32
addition, sequential.  An fp32 addition is correctly rounded on both sides, so there is no bound: the check is equality of the int32
views, element by element.  The one exception IEEE leaves open is the payload of a NaN: where the reference holds a NaN the result must
hold a NaN, any NaN.  The build has no flush-to-zero flag, so denormal operands and denormal sums are ordinary values, and the inputs
carry them, beside +-0, +-inf, inf + -inf (= NaN), NaN and a sum that overflows (SPECIALS).

tests/test_accum_cpu.py shows on the host that the check rejects the pairwise order, a scale applied before the sum, a dropped tail,
written guard elements and a copy treated as an addition onto a stale sum.  tests/test_gpu_accum.py runs the cases below; the IEEE-half
build runs this file as a child process (one storage type per process)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.optim_exact import GRID_ELEMS, GUARD

FILL_DST, FILL_A, FILL_B = 3.0, 5.0, 7.0          # sentinels of the guard elements (and of a destination before the launch)
_TINY = float(np.float32(2.0 ** -126))            # the smallest normal number
_DEN = float(np.float32(2.0 ** -149))             # the smallest denormal
_BIG = float(np.float32(3.0e38))
_INF, _NAN = float('inf'), float('nan')
# (a, b): the operand pairs every input carries
SPECIALS = ((0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (1.5, -1.5),
            (_INF, 1.0), (-_INF, 1.0), (_INF, _INF), (_INF, -_INF), (-_INF, _INF),
            (_NAN, 1.0), (2.0, _NAN), (_NAN, _INF),
            (_DEN, 0.0), (_DEN, _DEN), (-3 * _DEN, 1.0), (5 * _DEN, -2 * _DEN),      # denormal operands
            (1.5 * _TINY, -_TINY), (_TINY, -_DEN), (-1.25 * _TINY, _TINY),           # normal operands, a denormal sum
            (_BIG, _BIG), (-_BIG, -_BIG), (_BIG, 1.0e38))                            # a sum that overflows to +-inf


def make_inputs(n, seed, count=2):
    """`count` numpy fp32 arrays of n elements: magnitudes log-uniform over 1e-3 .. 1e3 with random signs (near enough for the order of a
    sum to matter in most elements), SPECIALS planted at the front, at the end (the element-wise tail) and at random places; for an n below their number
    the specials alone, rotated by the seed.  Arrays beyond the second repeat the pattern with the operands swapped."""
    r = np.random.Generator(np.random.PCG64([seed, n]))
    K = len(SPECIALS)
    out = []
    where = np.concatenate([np.arange(min(n, K)), n - 1 - np.arange(min(n, K)), r.integers(0, n, 4 * K)]) if n >= 2 * K else np.arange(n)
    for c in range(count):
        x = (10.0 ** r.uniform(-3, 3, n) * np.where(r.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)
        with np.errstate(all='ignore'):
            for j, pos in enumerate(where):
                x[pos] = np.float32(SPECIALS[(j + seed) % K][c % 2])
        out.append(x)
    return out


def reference(a, b=None):
    """numpy fp32: a + b, or a copy of a (b is None)"""
    if b is None:
        return a.copy()
    with np.errstate(all='ignore'):
        return (a.astype(np.float32) + b.astype(np.float32)).astype(np.float32)


def reference_sum(gs):
    """((g1 + g2) + g3) + ... in fp32, the order of accumulate() ... step()"""
    acc = reference(gs[0])
    for g in gs[1:]:
        acc = reference(acc, g)
    return acc


def _as_tensor(x):
    return torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x


def mismatches(got, want):
    """number of elements of `got` that are not `want` bit for bit; a NaN of the reference is matched by any NaN.  numpy fp32 arrays or
    torch fp32 tensors (the GPU cases compare on the device)."""
    got, want = _as_tensor(got), _as_tensor(want)
    if got.shape != want.shape:
        return max(got.numel(), want.numel())
    same = (got.contiguous().view(torch.int32) == want.contiguous().view(torch.int32)) | (torch.isnan(got) & torch.isnan(want))
    return int((~same).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU cases
class Buf(object):
    """n floats with GUARD sentinel floats on both sides, the whole shifted by `shift` floats from a 16-byte boundary; .x is the view the
    engine gets"""
    def __init__(self, values, fill, shift=0):
        n = values.numel()
        self.buf = torch.full((n + 2 * GUARD + 4,), float(fill), dtype=torch.float32, device='cuda')
        self.lo = GUARD + shift
        self.x = self.buf[self.lo:self.lo + n]
        self.x.copy_(values)
        assert self.x.data_ptr() % 16 == 4 * shift

    def expect(self, values):
        """mismatches of the WHOLE buffer, guards included, against `values` inside and the sentinel outside"""
        want = torch.full_like(self.buf, float(self.buf[0]))
        want[self.lo:self.lo + values.numel()] = values
        return mismatches(self.buf, want)


FORMS = ('distinct', 'dst==a', 'dst==b', 'copy')
# which of (dst, a, b) is moved one float off the 16-byte boundary: the element-wise path of the kernel
SHIFTS = {'distinct': ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)), 'dst==a': ((0, 0, 0), (1, 1, 0), (0, 0, 1)),
          'dst==b': ((0, 0, 0), (1, 0, 1), (0, 1, 0)), 'copy': ((0, 0, 0), (1, 0, 0), (0, 1, 0))}


def run_case(n, log=print):
    """Every pointer form and every shift at size n: the destination bit for bit, the guards of all three buffers and the inputs that
    are not the destination unchanged.  Returns the failures [(what, count)]."""
    from pose_adv_aug_amd._lib import lib, ptr, stream
    L = lib()
    a, b = make_inputs(n, 40)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    want = {'add': torch.from_numpy(reference(a, b)).cuda(), 'copy': ta}
    fails = []
    for form in FORMS:
        for sd, sa, sb in SHIFTS[form]:
            what = 'n %d %s shifts %d%d%d' % (n, form, sd, sa, sb)
            A = Buf(ta, FILL_A, sa)
            Bb = Buf(tb, FILL_B, sb) if form != 'copy' else None
            D = A if form == 'dst==a' else Bb if form == 'dst==b' else Buf(torch.full_like(ta, FILL_DST), FILL_DST, sd)
            rc = L.pa_grad_accumulate(ptr(D.x), ptr(A.x), ptr(Bb.x) if Bb is not None else None, n, stream())
            torch.cuda.synchronize()
            if rc != 0:
                fails.append((what + ': refused: %s' % L.pa_last_error(), rc))
                continue
            bad = D.expect(want['copy' if form == 'copy' else 'add'])
            if bad:
                fails.append((what + ': destination or its guards', bad))
            for name, X, t in (('a', A, ta), ('b', Bb, tb)):
                if X is not None and X is not D and X.expect(t):
                    fails.append((what + ': input %s was written' % name, X.expect(t)))
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('accum_exact n %d: %d launches, %d failures' % (n, sum(len(v) for v in SHIFTS.values()), len(fails)))
    return fails


def run_error_cases():
    """NULL dst, NULL a, n == 0 and ranges that overlap in part: non-zero, a message that names the entry, the buffers untouched.
    dst == a with b == NULL: 0, and nothing written."""
    from pose_adv_aug_amd._lib import lib, ptr, stream
    L = lib()
    n = 1024
    buf = torch.full((4 * n,), 9.0, dtype=torch.float32, device='cuda')
    keep = buf.clone()
    d, a, b = buf[0:n], buf[n:2 * n], buf[2 * n:3 * n]
    at = lambda k: C.c_void_p(buf.data_ptr() + 4 * k)
    fails = []
    cases = (('NULL dst', (None, ptr(a), ptr(b), n)), ('NULL a', (ptr(d), None, ptr(b), n)), ('NULL a, copy form', (ptr(d), None, None, n)),
             ('n == 0', (ptr(d), ptr(a), ptr(b), 0)), ('n == 0, copy form', (ptr(d), ptr(a), None, 0)),
             ('dst overlaps a by one float', (at(1), at(0), at(2 * n), n)), ('dst overlaps a from below', (at(0), at(n - 1), at(2 * n), n)),
             ('dst overlaps b', (at(0), at(2 * n), at(n // 2), n)), ('a overlaps b', (at(0), at(n), at(n + 4), n)),
             ('dst overlaps a, copy form', (at(4), at(0), None, n)), ('dst == b, a overlaps both', (at(0), at(8), at(0), n)))
    for what, args in cases:
        rc = L.pa_grad_accumulate(*(args + (stream(),)))
        msg = L.pa_last_error() or b''
        if rc == 0 or b'pa_grad_accumulate' not in msg:
            fails.append((what, rc, msg))
    rc = L.pa_grad_accumulate(ptr(d), ptr(d), None, n, stream())
    if rc != 0:
        fails.append(('dst == a with b NULL must return 0', rc, L.pa_last_error()))
    torch.cuda.synchronize()
    if not torch.equal(buf.view(torch.int32), keep.view(torch.int32)):
        fails.append(('a refused call wrote to a buffer', 0, b''))
    return fails


# 1-stack chan-128 pose net, 64 x 64 input, batch 2: the smallest net the engine builds
STACKS, CHAN, RES, B = 1, 128, 64, 2


def small_net(seed=11):
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    net = create_hg(STACKS, 1, 16, CHAN, res=RES, default_batch=B)
    net.reset_parameters(seed=seed)
    net.train()
    return net


def small_batch(k):
    from tests import inputs
    return (torch.from_numpy(inputs.images(300 + k, B, RES)).cuda(), torch.from_numpy(inputs.heat_pts(400 + k, B, res=RES // 4)).cuda())


def _bits(x):
    return x.view(torch.int32)


def run_skip_group(log=print):
    """fp16 build.  A group of 2 whose FIRST micro-batch gradient has one inf written into flat_grads before accumulate(): the inf
    survives the fold, the step's finite check skips the whole group's step once.  Parameters and optimizer state bit-unchanged,
    skipped_steps() == 1, the EMA holds once, pending == 0; the next group steps normally."""
    from pose_adv_aug_amd.utils.optim import Adam, ModelEma, RMSprop
    fails = []
    for make in (lambda net: RMSprop(net), lambda net: Adam(net, max_grad_norm=1.0)):
        net = small_net()
        opt = make(net)
        ema = ModelEma(net, decay=0.9)
        name = type(opt).__name__
        state = lambda: [net.flat_params.clone()] + [getattr(opt, k).clone() for k in ('square_avg', 'exp_avg', 'exp_avg_sq') if hasattr(opt, k)]
        before, twin_before = state(), ema.module.flat_params.clone()
        net.loss_and_backward(*small_batch(0))
        net.flat_grads[12345] = float('inf')
        opt.accumulate()
        net.loss_and_backward(*small_batch(1))
        opt.step()
        ema.update(opt)
        torch.cuda.synchronize()
        if not bool(torch.isinf(net.flat_grads[12345])):
            fails.append((name + ': the inf did not reach the folded gradient', float(net.flat_grads[12345])))
        if not all(torch.equal(_bits(x), _bits(y)) for x, y in zip(before, state())):
            fails.append((name + ': parameters or state moved on the skipped group', 0))
        if not torch.equal(_bits(twin_before), _bits(ema.module.flat_params)):
            fails.append((name + ': the EMA moved on the skipped group', 0))
        got = (opt.skipped_steps(), ema.held(), ema.updates(), opt.pending)
        if got != (1, 1, 0, 0):
            fails.append((name + ': (skipped, held, updates, pending) after the skipped group', got))
        if name == 'Adam' and opt.steps_taken() != 0:
            fails.append(('Adam: the step count advanced on the skipped group', opt.steps_taken()))
        for k in (2, 3):                                    # the next group: finite, taken
            net.loss_and_backward(*small_batch(k))
            opt.accumulate() if k == 2 else opt.step()
        ema.update(opt)
        torch.cuda.synchronize()
        got = (opt.skipped_steps(), ema.held(), ema.updates(), opt.pending)
        if got != (1, 1, 1, 0):
            fails.append((name + ': (skipped, held, updates, pending) after the next group', got))
        if torch.equal(_bits(before[0]), _bits(net.flat_params)) or not bool(torch.isfinite(net.flat_params).all()):
            fails.append((name + ': the next group did not step, or stepped to a non-finite value', 0))
        if os.environ.get('POSEADV_TEST_VERBOSE'):
            log('accum_exact skipped group %s: %d failures so far' % (name, len(fails)))
    return fails


FP16_SIZES = (1023, GRID_ELEMS + 5)

if __name__ == '__main__':          # the fp16 build: tests/test_gpu_accum.py runs this with POSEADV_DTYPE=fp16
    from pose_adv_aug_amd._lib import lib as _l
    assert _l().pa_dtype() == 1, 'run with POSEADV_DTYPE=fp16'
    torch.cuda.set_device(0)
    out = lambda s: print(s, flush=True)
    fails = []
    for n in FP16_SIZES:
        fails += run_case(n, log=out)
    fails += run_error_cases()
    fails += run_skip_group(log=out)
    print('FAILURES %d %s' % (len(fails), fails[:20]))
    print('FP16 ACCUM EXACT ' + ('PASSED' if not fails else 'FAILED'), flush=True)
    sys.exit(1 if fails else 0)
