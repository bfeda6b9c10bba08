"""Exact check of the fused RMSprop step (rmsprop_kernel / rmsprop_checked_kernel and the rmsprop_v / rmsprop_p both share, csrc/elementwise.hip; pa_rmsprop_step and
pa_rmsprop_step_state): every element of p AND of square_avg after a step, against a float64 evaluation of

    v' = alpha32 v + c32 (g s)^2,      p' = p - lr32 (g s) / (sqrt(v') + eps32)

from the (p, g, v) the engine itself held before that step, with the engine's own fp32 constants (alpha32 = (float)alpha,
c32 = 1.f - alpha32, lr32, eps32, s = (float)gscale: the values the C ABI receives).  Over several steps the reference restarts from
the engine's previous output, so every step is a local check.

Bound.  Class E of tests/bn_exact.py (u = 2^-24, first-order propagation), every operation of the kernel charged on its own --
g s; c32 (g s); that times (g s); alpha32 v; their sum; sqrtf; + eps32; the division; the product with lr32; the subtraction from p --
which admits any FMA contraction the compiler picks (a contracted pair rounds once where the bound pays twice).  sqrtf follows the
rule of rsqrtf there (E.sqrt: the exact interval of its argument, widened by 2u); the division is correctly rounded (E.div: hipcc's
default, csrc/build.sh passes no fast-math flag).  Nothing is fitted: tests/test_optim_exact_cpu.py shows on an fp32 emulation of the
kernel that the bound holds (worst error / bound just below 1) and that eps inside the root, no eps, a dropped or doubled gscale
and four elements skipped or updated twice are each far outside it.  The relative rounding model needs normal numbers: the inputs
keep |g s| >= 1e-15 or exactly 0, so that no square is subnormal (DOMAIN).

tests/test_gpu_optim_exact.py runs the cases below; the IEEE-half build (whose step first scans the gradient for inf / NaN and skips
the update: grad_check_kernel) runs this file as a child process, one storage type per process."""
import os
import sys

import numpy as np
import torch

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.bn_exact import E, _ratio

LR, ALPHA, EPS = 2.5e-4, 0.99, 1e-8
GSCALES = (1.0, 0.5, 1.0 / 3.0, 1.0 / 32768.0)
GRID_ELEMS = 2048 * 256 * 4                 # what one pass of the capped launch covers (pa_launch_rmsprop)
SIZES = (1, 2, 3, 4, 5, 7, 1023, 100003) + tuple(GRID_ELEMS + k for k in (0, 1, 3, 5))
GUARD = 64                                  # floats on either side of [0, n): a multiple of 4, the 16-byte loads stay aligned
DOMAIN = 1e-15                              # smallest nonzero |g s| the bound is stated for


def _f32(x):
    return float(np.float32(x))


def reference(p, g, v, lr=LR, alpha=ALPHA, eps=EPS, gscale=1.0):
    """(p', v') as E terms (float64 value, bound of the fp32 evaluation) from float64 tensors that hold fp32 values."""
    c32 = float(np.float32(1.0) - np.float32(alpha))
    gr = E(g) * E(_f32(gscale))
    v1 = E(_f32(alpha)) * E(v) + (E(c32) * gr) * gr
    q = gr.div(v1.sqrt() + E(_f32(eps)))
    p1 = E(p) - E(_f32(lr)) * q
    return p1, v1


def check(p0, g, v0, p1, v1, gscale, lr=LR, alpha=ALPHA, eps=EPS):
    """worst error / bound of p and of v after one step from (p0, g, v0); NaN if the step produced one"""
    rp, rv = reference(p0.double(), g.double(), v0.double(), lr, alpha, eps, gscale)
    return _ratio(p1, rp.v, rp.e), _ratio(v1, rv.v, rv.e)


def make_inputs(n, seed, gscale, v_zero):
    """numpy fp32 (p, g, v): |g s| log-uniform in 1e-12 .. 1e3 with random signs and exact zeros, v zero or -- half of it -- log-uniform
    in 1e-24 .. 1e6, p standard normal."""
    r = np.random.Generator(np.random.PCG64([seed, n]))
    gs = 10.0 ** r.uniform(-12, 3, n) * np.where(r.random(n) < 0.5, -1.0, 1.0)
    gs[r.random(n) < 0.05] = 0.0
    g = (gs / _f32(gscale)).astype(np.float32)
    p = r.standard_normal(n).astype(np.float32)
    v = np.zeros(n, dtype=np.float32)
    if not v_zero:
        v = np.where(r.random(n) < 0.5, 10.0 ** r.uniform(-24, 6, n), 0.0).astype(np.float32)
    return p, g, v


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU cases
class Guarded(object):
    """n floats with GUARD sentinel floats on both sides; .x is the view the engine gets"""
    def __init__(self, values, fill):
        n = values.numel()
        self.buf = torch.full((n + 2 * GUARD,), float(fill), dtype=torch.float32, device='cuda')
        self.x = self.buf[GUARD:GUARD + n]
        self.x.copy_(values)
        self.fill = torch.full((GUARD,), float(fill), dtype=torch.float32, device='cuda').view(torch.int32)

    def guards_intact(self):
        b = self.buf.view(torch.int32)
        return bool(torch.equal(b[:GUARD], self.fill)) and bool(torch.equal(b[-GUARD:], self.fill))


def _t(a):
    return torch.from_numpy(a).cuda()


class Stepper(object):
    """one optimizer state (p, v, its skip counter) behind either entry point"""
    def __init__(self, entry, p, v):
        from pose_adv_aug_amd._lib import lib
        self.L, self.entry = lib(), entry
        self.p, self.v = Guarded(p, 3.0), Guarded(v, 5.0)
        self.state = torch.zeros(2, dtype=torch.int32, device='cuda') if entry == 'state' else None

    def step(self, g, gscale):
        """g: a Guarded gradient (its guards hold NaN: the fp16 build's scan must not read them)"""
        from pose_adv_aug_amd._lib import check as ok, ptr, stream
        n = self.p.x.numel()
        if self.entry == 'state':
            ok(self.L.pa_rmsprop_step_state(ptr(self.p.x), ptr(g.x), ptr(self.v.x), n, LR, ALPHA, EPS, float(gscale), ptr(self.state), stream()))
        else:
            ok(self.L.pa_rmsprop_step(ptr(self.p.x), ptr(g.x), ptr(self.v.x), n, LR, ALPHA, EPS, float(gscale), stream()))

    def skipped(self):
        import ctypes as C
        from pose_adv_aug_amd._lib import check as ok, ptr, stream
        c = C.c_longlong(-1)
        if self.entry == 'state':
            ok(self.L.pa_rmsprop_skipped_steps_state(ptr(self.state), C.byref(c), stream()))
        else:
            ok(self.L.pa_rmsprop_skipped_steps(C.byref(c), stream()))
        return int(c.value)


def run_case(n, entry, log=print, steps=3):
    """Every gscale, from v = 0 and from a non-zero v: `steps` consecutive steps with fresh gradients, each checked from the engine's
    own state before it; guards bit-identical; the skip counter unchanged.  Returns the failures [(what, figure)]."""
    fails = []
    worst = [0.0, 0.0]
    for gi, gscale in enumerate(GSCALES):
        for v_zero in (True, False):
            p, _, v = make_inputs(n, 900 + gi, gscale, v_zero)
            S = Stepper(entry, _t(p), _t(v))
            skipped0 = S.skipped()
            for k in range(steps):
                _, g, _ = make_inputs(n, 1000 + 10 * gi + k, gscale, True)
                G = Guarded(_t(g), float('nan'))
                p0, v0 = S.p.x.clone(), S.v.x.clone()
                S.step(G, gscale)
                torch.cuda.synchronize()
                rp, rv = check(p0, G.x, v0, S.p.x, S.v.x, gscale)
                worst = [max(worst[0], rp) if rp == rp else rp, max(worst[1], rv) if rv == rv else rv]
                what = 'n %d %s gscale %g v0 %s step %d' % (n, entry, gscale, 'zero' if v_zero else 'nonzero', k)
                if not (rp <= 1.0):
                    fails.append(('p ' + what, rp))
                if not (rv <= 1.0):
                    fails.append(('square_avg ' + what, rv))
                if not (S.p.guards_intact() and S.v.guards_intact()):
                    fails.append(('guard elements changed ' + what, 0))
            if S.skipped() != skipped0:
                fails.append(('skip counter moved on finite gradients n %d %s' % (n, entry), S.skipped() - skipped0))
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('optim_exact n %d %s: worst error / bound p %.3g square_avg %.3g' % (n, entry, worst[0], worst[1]))
    return fails


def _check_flat(module, opt, what, fails, log):
    """Two steps of `opt` on the whole flat array of `module`, whose flat_grads hold a backward pass: every element whose gradient is in
    the stated domain within the bound, the alignment padding between the tensors (g = 0, v = 0, p = 0) exactly 0 before and after.
    Returns the number of padding elements."""
    from pose_adv_aug_amd._lib import grad_scale
    n = module.flat_params.numel()
    used = torch.zeros(n, dtype=torch.bool, device='cuda')
    for _, _, off, numel, kind in module._table:
        if kind == 0:
            used[off:off + numel] = True
    pad = ~used
    for name, a in (('p', module.flat_params), ('g', module.flat_grads), ('square_avg', opt.square_avg)):
        if bool((a[pad] != 0).any()):
            fails.append(('%s: padding of %s not zero before the step' % (what, name), float(a[pad].abs().max())))
    worst = [0.0, 0.0]
    gscale = 1.0 / grad_scale()
    for k in range(2):          # from v = 0, then from the v that step left (the same gradient: a local check either way)
        p0, g, v0 = module.flat_params.clone(), module.flat_grads.clone(), opt.square_avg.clone()
        opt.step()
        torch.cuda.synchronize()
        gs = (g.double() * _f32(gscale)).abs()
        dom = (gs == 0) | (gs >= DOMAIN)
        if float(dom.float().mean()) < 0.9:
            fails.append(('%s: less than 90 %% of the real gradient is in the bound\'s domain' % what, float(dom.float().mean())))
        if not bool((g != 0).any()):
            fails.append(('%s: the gradient is all zero, no backward pass reached it' % what, 0))
        rp, rv = check(p0[dom], g[dom], v0[dom], module.flat_params[dom], opt.square_avg[dom], gscale)
        worst = [max(worst[0], rp) if rp == rp else rp, max(worst[1], rv) if rv == rv else rv]
        if not (rp <= 1.0):
            fails.append(('p of the flat array of %s, step %d' % (what, k), rp))
        if not (rv <= 1.0):
            fails.append(('square_avg of the flat array of %s, step %d' % (what, k), rv))
        if not bool(torch.isfinite(module.flat_params).all() and torch.isfinite(opt.square_avg).all()):
            fails.append(('non-finite value in the flat array of %s after step %d' % (what, k), 0))
        for name, a in (('p', module.flat_params), ('square_avg', opt.square_avg)):
            if bool((a[pad] != 0).any()):
                fails.append(('%s: padding of %s not zero after step %d' % (what, name, k), float(a[pad].abs().max())))
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('optim_exact flat array of %s n %d (%d padding elements): worst error / bound p %.3g square_avg %.3g'
            % (what, n, int(pad.sum()), worst[0], worst[1]))
    return int(pad.sum())


def run_flat_array(log=print):
    """The optimizers of a real pose net (2 stacks, chan 128, B 2, 256 x 256) and of the scale / rotation agent on it, each on its flat
    array after a backward pass (_check_flat).  Every tensor of the pose net has a multiple of 4 elements, so its flat array has no
    alignment padding (Net::add_param rounds every offset up to 4 floats); the agent's has, behind the 7-element biases of fc_scale and
    fc_rotation, which is why the agent is here (256 is the smallest size it accepts).  No padding anywhere is a failure: nothing would
    have been tested."""
    from pose_adv_aug_amd.models.asn_stacked_hg import create_asn
    from pose_adv_aug_amd.utils.optim import RMSprop
    from tests import inputs
    from tests.asn_exact import _targets
    from tests.test_gpu_net import t, _hg_pair
    chan, B, res = 128, 2, 256
    ref, net = _hg_pair(2, chan, B, res, seed=61)
    del ref
    agent = create_asn(chan, chan, 7, 7, is_aug=True, res=res, default_batch=B)
    agent.reset_parameters(seed=62)
    img = t(inputs.images(161, B, res)).cuda()
    net.train(); agent.train()
    ls, lr = net(img, asn=agent, is_half_hg=True, is_aug=True)          # before the pose net's step: the agent reads its weights
    gs_t, gr_t = _targets(163, ls, lr, B)
    agent.zero_grad()
    agent.loss_and_backward(gs_t, gr_t)
    net.loss_and_backward(img, t(inputs.heat_pts(162, B, res=res // 4)).cuda())
    fails = []
    pads = _check_flat(net, RMSprop(net), 'the pose net', fails, log)
    pads += _check_flat(agent, RMSprop(agent), 'the agent', fails, log)
    if pads == 0:
        fails.append(('neither flat array has alignment padding: nothing was tested', 0))
    return fails


# the fp16 build's skip: a non-finite gradient at these positions of an n with n % 4 == 3 that needs a second grid pass
SKIP_N = GRID_ELEMS + 7
SKIP_POSITIONS = (('index 0', 0), ('vector body', 4097), ('last tail element', SKIP_N - 1), ('beyond the first grid pass', GRID_ELEMS + 1))


def run_skip_case(entry, log=print):
    """fp16 build.  For each position and inf / NaN in turn: optimizer A steps on the poisoned gradient, optimizer B (its own state
    pair) on a finite one, then A on a finite one.  A's p and v bit-unchanged and its counter + 1 after the first; B applied within the
    bound, its counter unmoved; A's next step applied within the bound, its counter unmoved."""
    n, gscale = SKIP_N, 1.0 / 32768.0
    assert n % 4 == 3
    fails = []
    p, g, v = make_inputs(n, 950, gscale, False)
    A = Stepper(entry, _t(p), _t(v))
    p2, _, v2 = make_inputs(n, 951, gscale, False)
    Bo = Stepper('state', _t(p2), _t(v2))
    G = Guarded(_t(g), float('nan'))
    bi = lambda x: x.view(torch.int32)
    for i, (where, pos) in enumerate(SKIP_POSITIONS):
        for bad in (float('inf'), float('nan'), float('-inf')):
            what = '%s %s at %s' % (entry, bad, where)
            Gb = Guarded(G.x, float('nan'))
            Gb.x[pos] = bad
            pa, va, ca, cb = A.p.x.clone(), A.v.x.clone(), A.skipped(), Bo.skipped()
            A.step(Gb, gscale)
            pb, vb = Bo.p.x.clone(), Bo.v.x.clone()
            Bo.step(G, gscale)
            torch.cuda.synchronize()
            if not (torch.equal(bi(A.p.x), bi(pa)) and torch.equal(bi(A.v.x), bi(va))):
                fails.append(('p or square_avg changed on a skipped step: ' + what, int((bi(A.p.x) != bi(pa)).sum() + (bi(A.v.x) != bi(va)).sum())))
            if A.skipped() != ca + 1:
                fails.append(('skip counter not + 1: ' + what, A.skipped() - ca))
            if Bo.skipped() != cb:
                fails.append(('the other optimizer\'s counter moved: ' + what, Bo.skipped() - cb))
            r = check(pb, G.x, vb, Bo.p.x, Bo.v.x, gscale)
            if not (r[0] <= 1.0 and r[1] <= 1.0):
                fails.append(('the other optimizer\'s finite step: ' + what, r))
            A.step(G, gscale)
            torch.cuda.synchronize()
            r = check(pa, G.x, va, A.p.x, A.v.x, gscale)
            if not (r[0] <= 1.0 and r[1] <= 1.0):
                fails.append(('the next finite step: ' + what, r))
            if A.skipped() != ca + 1:
                fails.append(('skip counter moved on the next finite step: ' + what, A.skipped() - ca - 1))
            if not (A.p.guards_intact() and A.v.guards_intact() and Bo.p.guards_intact() and Bo.v.guards_intact()):
                fails.append(('guard elements changed: ' + what, 0))
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('optim_exact skip %s: %d positions x 3 values, %d failures' % (entry, len(SKIP_POSITIONS), len(fails)))
    return fails


if __name__ == '__main__':          # the fp16 build: tests/test_gpu_optim_exact.py runs this with POSEADV_DTYPE=fp16
    from pose_adv_aug_amd._lib import lib as _l
    assert _l().pa_dtype() == 1, 'run with POSEADV_DTYPE=fp16'
    torch.cuda.set_device(0)
    out = lambda s: print(s, flush=True)
    fails = []
    for entry in ('plain', 'state'):
        for n in SIZES:
            fails += run_case(n, entry, log=out)
        fails += run_skip_case(entry, log=out)
    fails += run_flat_array(log=out)
    print('FAILURES %d %s' % (len(fails), fails[:20]))
    print('FP16 OPTIM EXACT ' + ('PASSED' if not fails else 'FAILED'), flush=True)
    sys.exit(1 if fails else 0)
