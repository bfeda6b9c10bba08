"""Oracles and cases for the layer-wise optimizers (csrc/opt_layerwise.hip; pa_opt_segments_host, pa_tensor_norms, pa_lamb_step, pa_lars_step;
utils.optim.SGD / LARS / LAMB).

Formulas (include/poseadv.h has them with the order of operations):

    LAMB  gr = (g s) coef;  m' = m + (gr - m)(1 - b1);  v' = b2 v + ((1 - b2) gr) gr;  u = (m' / bc1) / (sqrt(v') / bc2s + eps) [+ wd p]
          r_t = (adapt_t and W > 0 and U > 0) ? W / U : 1, capped at max_trust > 0;  p' = p - (lr r_t) u
    LARS  gr = (g s) coef;  r_t = (tc > 0 and adapt_t and W > 0 and G > 0) ? tc W / (G + wd W + eps) : 1
          d = gr [+ wd p];  d = r_t d (tc > 0);  buf' = mom buf + d;  d = nesterov ? d + mom buf' : buf';  p' = p - lr d
    adapt_t = always_adapt or the tensor's weight decay != 0;  W = ||p||, U = ||u||, G = ||gr|| per tensor.

lars_oracle / lamb_oracle evaluate them in float64 on a list of tensors (tests/test_layerwise_cpu.py compares them with torch.optim.SGD
and torch.optim.AdamW).  lamb_reference / lars_reference evaluate ONE step per element with the error bound of the fp32 evaluation (class
E of tests/bn_exact.py: every fp32 operation charged on its own, which admits any FMA contraction; sqrtf within 2u; divisions correctly
rounded: the rules of tests/adam_exact.py), from the arrays the engine held before the step and the engine's own coef, bc1, bc2s and r_t.
The norms and ratios are checked on their own (check_norms): W and G within 2u + 1e-12 relative of the float64 value (one rounding to
fp32 and the order of the double additions), U within ||e||_2 of ||u_ref||_2 plus the same slack (e: the per-element bound of u), and r_t
inside the interval that follows from those, widened by 2u.

The synthetic table (table()): tensors of 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, 2 S + 5 and 7 S floats (S =
PA_OPT_SEGMENT_FLOATS) with 0, 4 and 12 floats of padding between them, ending at an n with n % 4 == 3.  Tensor ZERO_P is all zero and
tensor ZERO_G has a zero gradient.

tests/test_gpu_layerwise.py runs the cases; the IEEE-half build runs this file as a child process, one storage type per process."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import torch

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.bn_exact import E, U, _ratio
from tests.optim_exact import DOMAIN, Guarded, make_inputs, _f32, _t
from tests.adam_exact import make_state, one_minus, read_state, check_consts

S = 1024                                    # PA_OPT_SEGMENT_FLOATS (test_layerwise_cpu.py checks it against the header and _lib)
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, 2 * S + 5, 7 * S)
GAPS = (0, 4, 12)
ZERO_P, ZERO_G = 5, 7                       # the all-zero tensor (64 floats) and the tensor with a zero gradient (255 floats)
LR, BETA1, BETA2, EPS = 1e-3, 0.9, 0.999, 1e-6
GSCALES = (1.0, 1.0 / 3.0, 1.0 / 32768.0)
SLACK = 1e-12


def table(order=None, gaps=GAPS):
    """(offsets, numels, n) of the synthetic table; order: a permutation of the tensors (None: as listed)"""
    sizes = [SIZES[i] for i in (order if order is not None else range(len(SIZES)))]
    offsets, off = [], 0
    for i, numel in enumerate(sizes):
        offsets.append(off)
        off = (off + numel + 3) // 4 * 4 + gaps[i % len(gaps)]
    return offsets, sizes, off + 3


def segments(L, offsets, numels, groups, n, cap=None):
    """(count, ctypes array of OptSegment) from pa_opt_segments_host; count 0 on an error"""
    from pose_adv_aug_amd._lib import OptSegment
    nt = len(offsets)
    a = ((C.c_size_t * nt)(*offsets), (C.c_size_t * nt)(*numels), (C.c_int32 * nt)(*groups))
    count = int(L.pa_opt_segments_host(a[0], a[1], a[2], nt, n, None, 0))
    if count == 0:
        return 0, None
    host = (OptSegment * count)()
    got = int(L.pa_opt_segments_host(a[0], a[1], a[2], nt, n, host, count if cap is None else cap))
    return got, host


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 oracles on lists of tensors
def _norm(x):
    return float(x.double().pow(2).sum().sqrt())


def lars_oracle(ps, gs, bufs, lr, momentum=0.0, weight_decay=0.0, nesterov=False, trust_coefficient=0.0, eps=1e-8, always_adapt=False,
                wds=None, force_ratio=None):
    """one step in float64, in place on ps and bufs; wds: per-tensor weight decay (None: weight_decay everywhere).  Returns the ratios."""
    ratios = []
    for i, (p, g, buf) in enumerate(zip(ps, gs, bufs)):
        wd = weight_decay if wds is None else wds[i]
        W, G = _norm(p), _norm(g)
        r = 1.0
        if trust_coefficient > 0 and (always_adapt or wd != 0) and W > 0 and G > 0:
            r = trust_coefficient * W / (G + wd * W + eps)
        if force_ratio is not None:
            r = force_ratio
        d = g + wd * p if wd != 0 else g.clone()
        if trust_coefficient > 0:
            d = r * d
        if momentum != 0:
            buf.mul_(momentum).add_(d)
            d = d + momentum * buf if nesterov else buf
        p.sub_(lr * d)
        ratios.append(r)
    return ratios


def lamb_oracle(ps, gs, ms, vs, t, lr=LR, betas=(BETA1, BETA2), eps=EPS, weight_decay=0.01, max_trust=0.0, always_adapt=False, wds=None,
                force_ratio=None):
    """step t (1-based) in float64, in place on ps, ms and vs.  Returns the ratios."""
    b1, b2 = betas
    bc1, bc2s = 1.0 - b1 ** t, (1.0 - b2 ** t) ** 0.5
    ratios = []
    for i, (p, g, m, v) in enumerate(zip(ps, gs, ms, vs)):
        wd = weight_decay if wds is None else wds[i]
        m.add_((g - m) * (1.0 - b1))
        v.mul_(b2).add_((1.0 - b2) * g * g)
        u = (m / bc1) / (v.sqrt() / bc2s + eps)
        if wd != 0:
            u = u + wd * p
        W, Un = _norm(p), _norm(u)
        r = W / Un if (always_adapt or wd != 0) and W > 0 and Un > 0 else 1.0
        if max_trust > 0:
            r = min(r, max_trust)
        if force_ratio is not None:
            r = force_ratio
        p.sub_((lr * r) * u)
        ratios.append(r)
    return ratios


# ---------------------------------------------------------------------------------------------------------------------------------
# per-element references with bounds.  wd, lr, r: float64 tensors, one value per element (the tensor's)
def _sel(mask, a, b):
    return E(torch.where(mask, a.v, b.v), torch.where(mask, a.e, b.e))


def _gr(g, gscale, coef):
    gr = E(g) * E(_f32(gscale))
    return gr * E(float(coef)) if coef is not None else gr


def lamb_reference(p, g, m, v, gscale, coef, bc1, bc2s, wd, lr, r, eps=EPS, beta1=BETA1, beta2=BETA2):
    """{p, exp_avg, exp_avg_sq, u: E terms}"""
    gr = _gr(g, gscale, coef)
    m1 = E(m) + (gr - E(m)) * E(one_minus(beta1))
    v1 = E(_f32(beta2)) * E(v) + (E(one_minus(beta2)) * gr) * gr
    den = v1.sqrt().div(E(float(bc2s))) + E(_f32(eps))
    u = m1.div(E(float(bc1))).div(den)
    u = _sel(wd != 0, u + E(wd) * E(p), u)
    return {'p': E(p) - (E(lr) * E(r)) * u, 'exp_avg': m1, 'exp_avg_sq': v1, 'u': u}


def lars_reference(p, g, buf, gscale, coef, wd, lr, r, momentum, nesterov, trust):
    """{p, momentum_buffer (momentum != 0): E terms}; r is applied iff trust"""
    gr = _gr(g, gscale, coef)
    d = _sel(wd != 0, gr + E(wd) * E(p), gr)
    if trust:
        d = E(r) * d
    out = {}
    if momentum != 0:
        b1 = E(_f32(momentum)) * E(buf) + d
        out['momentum_buffer'] = b1
        d = d + E(_f32(momentum)) * b1 if nesterov else b1
    out['p'] = E(p) - E(lr) * d
    return out


def tensor_sums(x, offsets, numels):
    """float64 [sum of x^2 over tensor t]"""
    return [float(x[o:o + k].double().pow(2).sum()) for o, k in zip(offsets, numels)]


def check_norms(kind, lay, norms, trust, p, gr64, u_ref, opts, wd_t, live):
    """norms: the engine's [2][nt] floats, trust: its nt ratios, p: before the step, gr64: float64 g s coef (LARS), u_ref: the E term of u
    (LAMB); wd_t: the weight decay of every tensor, live: which tensors are not frozen.  Returns failures [(what, figure)]."""
    fails = []
    offsets, numels, nt = lay.offsets, lay.numels, len(lay.offsets)
    W2 = tensor_sums(p, offsets, numels)
    rel = 2 * U + SLACK
    for t in range(nt):
        if not live[t]:
            continue
        W = W2[t] ** 0.5
        if abs(float(norms[t]) - W) > rel * W:
            fails.append(('W of tensor %d' % t, (float(norms[t]), W)))
        o, k = offsets[t], numels[t]
        adapt = (opts['always_adapt'] or wd_t[t] != 0)
        got_r = float(trust[t])
        if kind == 'lamb':
            Uv = float(u_ref.v[o:o + k].pow(2).sum().sqrt())
            Ue = float(u_ref.e[o:o + k].pow(2).sum().sqrt())
            if abs(float(norms[nt + t]) - Uv) > Ue + rel * Uv:
                fails.append(('U of tensor %d' % t, (float(norms[nt + t]), Uv, Ue)))
            if adapt and W > 0 and Uv > 0:
                lo, hi = W / (Uv + Ue), W / max(Uv - Ue, 1e-300)
            else:
                lo = hi = 1.0
            if opts['max_trust'] > 0:
                lo, hi = min(lo, _f32(opts['max_trust'])), min(hi, _f32(opts['max_trust']))
        else:
            G = float(gr64[o:o + k].pow(2).sum().sqrt())
            if abs(float(norms[nt + t]) - G) > rel * G:
                fails.append(('G of tensor %d' % t, (float(norms[nt + t]), G)))
            tc = _f32(opts['trust_coefficient'])
            r = tc * W / (G + _f32(wd_t[t]) * W + _f32(opts['eps'])) if tc > 0 and adapt and W > 0 and G > 0 else 1.0
            lo = hi = r
        if not (lo * (1 - rel) <= got_r <= hi * (1 + rel)):
            fails.append(('r of tensor %d' % t, (got_r, lo, hi)))
    return fails


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU cases
class Layout(object):
    """a table, its group of every tensor, the uploaded segment list, and per-element views of per-tensor values"""
    def __init__(self, order=None, gaps=GAPS, groups=None, single=None):
        from pose_adv_aug_amd._lib import lib
        if single is not None:
            self.offsets, self.numels, self.n = [0], [single], single
        else:
            self.offsets, self.numels, self.n = table(order, gaps)
        self.order = list(order) if order is not None else list(range(len(self.offsets)))
        nt = len(self.offsets)
        self.groups = list(groups) if groups is not None else [0] * nt
        self.nsegs, host = segments(lib(), self.offsets, self.numels, self.groups, self.n)
        assert self.nsegs > 0, lib().pa_last_error()
        self.segs = torch.frombuffer(host, dtype=torch.int32).clone().cuda()
        self.tensor_of = torch.full((self.n,), -1, dtype=torch.long)
        for t, (o, k) in enumerate(zip(self.offsets, self.numels)):
            self.tensor_of[o:o + k] = t
        self.used = (self.tensor_of >= 0).cuda()
        self.tensor_of = self.tensor_of.cuda()

    def per_elem(self, per_tensor):
        """float64 device tensor: per_tensor[t] at the elements of tensor t, 0 in the padding"""
        v = torch.as_tensor(per_tensor, dtype=torch.float64).cuda()
        return torch.where(self.used, v[self.tensor_of.clamp_min(0)], torch.zeros((), dtype=torch.float64, device='cuda'))

    def where(self, canonical):
        """the position in this layout of the tensor that is number `canonical` in SIZES"""
        return self.order.index(canonical)

    def scatter(self, values_by_canonical):
        """a flat fp32 array of this layout from {canonical tensor: 1-D fp32 tensor} (padding 0)"""
        x = torch.zeros(self.n, dtype=torch.float32)
        for t, c in enumerate(self.order):
            x[self.offsets[t]:self.offsets[t] + self.numels[t]] = values_by_canonical[c]
        return x.cuda()


def canonical_inputs(seed, gscale, zero_state):
    """{name: {canonical tensor: fp32 values}} for p, g, v, m: optim_exact.make_inputs / adam_exact.make_state per tensor, tensor ZERO_P all
    zero (p and its state), tensor ZERO_G with a zero gradient"""
    out = {'p': {}, 'g': {}, 'v': {}, 'm': {}}
    for c, k in enumerate(SIZES):
        p, g, v = make_inputs(k, seed + c, gscale, zero_state)
        m, _ = make_state(k, seed + c, v, zero_state)
        if c == ZERO_P:
            p, v, m = np.zeros_like(p), np.zeros_like(v), np.zeros_like(m)
        if c == ZERO_G:
            g = np.zeros_like(g)
        for name, a in (('p', p), ('g', g), ('v', v), ('m', m)):
            out[name][c] = torch.from_numpy(a)
    return out


def group_table(groups):
    """groups: [(lr, wd, frozen)] -> a ctypes array of OptGroup"""
    from pose_adv_aug_amd._lib import OptGroup
    tab = (OptGroup * len(groups))()
    for k, (lr, wd, frozen) in enumerate(groups):
        tab[k].lr, tab[k].weight_decay, tab[k].frozen = lr, wd, int(frozen)
    return tab


class Stepper(object):
    """the arrays of one optimizer on a Layout behind pa_lamb_step / pa_lars_step; groups: [(lr, wd, frozen)]"""
    def __init__(self, kind, lay, inputs, groups, **opts):
        from pose_adv_aug_amd._lib import lib
        self.L, self.kind, self.lay, self.groups, self.opts = lib(), kind, lay, groups, opts
        nt = len(lay.offsets)
        self.a = {'p': Guarded(lay.scatter(inputs['p']), 3.0)}
        if kind == 'lamb':
            self.a['exp_avg'] = Guarded(lay.scatter(inputs['m']), 5.0)
            self.a['exp_avg_sq'] = Guarded(lay.scatter(inputs['v']), 7.0)
            self.state = torch.zeros(8, dtype=torch.int32, device='cuda')
        else:
            if opts.get('momentum', 0) != 0:
                self.a['momentum_buffer'] = Guarded(lay.scatter(inputs['m']), 5.0)
            self.state = torch.zeros(2, dtype=torch.int32, device='cuda')
        self.ws = torch.zeros(int(self.L.pa_opt_layer_workspace_bytes(lay.nsegs, nt)) // 8, dtype=torch.float64, device='cuda')
        self.norms = torch.zeros(2 * nt, dtype=torch.float32, device='cuda')
        self.trust = torch.ones(nt, dtype=torch.float32, device='cuda')

    def arrays(self):
        return dict((k, a.x.clone()) for k, a in self.a.items())

    def everything(self):
        return dict(self.arrays(), norms=self.norms.clone(), trust=self.trust.clone(), state=self.state.clone())

    def step(self, g, gscale, coef=None):
        from pose_adv_aug_amd._lib import check as ok, ptr, stream, LambOpts, LarsOpts
        lay, o = self.lay, self.opts
        x = lambda k: ptr(self.a[k].x) if k in self.a else None
        tab = group_table(self.groups)
        cp = None if coef is None else ptr(coef)
        nt = len(lay.offsets)
        if self.kind == 'lamb':
            lo = LambOpts(BETA1, BETA2, EPS, o.get('max_trust', 0.0), int(o.get('always_adapt', False)), 0)
            ok(self.L.pa_lamb_step(C.byref(lo), tab, len(self.groups), ptr(lay.segs), lay.nsegs, nt, x('p'), ptr(g.x), x('exp_avg'), x('exp_avg_sq'),
                                   lay.n, float(gscale), cp, ptr(self.ws), ptr(self.norms), ptr(self.trust), ptr(self.state), stream()), 'pa_lamb_step')
        else:
            trust = o.get('trust_coefficient', 0.0) > 0
            lo = LarsOpts(o.get('momentum', 0.0), o.get('trust_coefficient', 0.0), o.get('eps', 1e-8), int(o.get('nesterov', False)),
                          int(o.get('always_adapt', False)))
            ok(self.L.pa_lars_step(C.byref(lo), tab, len(self.groups), ptr(lay.segs), lay.nsegs, nt, x('p'), ptr(g.x), x('momentum_buffer'), lay.n,
                                   float(gscale), cp, ptr(self.ws) if trust else None, ptr(self.norms) if trust else None,
                                   ptr(self.trust) if trust else None, ptr(self.state), stream()), 'pa_lars_step')

    def guards_intact(self):
        return all(a.guards_intact() for a in self.a.values())

    def check(self, before, g, gscale, coef, fails, what):
        """one step against the references (check_step), and the guards"""
        st = read_state(self.state) if self.kind == 'lamb' else None
        check_step(self.kind, self.lay, self.groups, self.opts, before, self.arrays(), g, gscale, coef, st, self.norms, self.trust, fails, what)
        if not self.guards_intact():
            fails.append(('guard elements changed ' + what, 0))


def check_step(kind, lay, groups, opts, before, after, g, gscale, coef, st, norms, trust, fails, what, dom=None):
    """One step against the references: every element of the live tensors (and of `dom`, the domain of the bound, when given) within the
    bound, frozen tensors and padding bit for bit, norms and ratios (check_norms).  groups: [(lr, wd, frozen)]; lay: offsets, numels,
    groups (per tensor), used, per_elem(); st: the engine's pa_adam_state as a dict (LAMB)."""
    o = opts
    wd_t = [groups[k][1] for k in lay.groups]
    live_t = [not groups[k][2] for k in lay.groups]
    wd = lay.per_elem([_f32(w) for w in wd_t])
    lr = lay.per_elem([_f32(groups[k][0]) for k in lay.groups])
    r = lay.per_elem(trust.double().cpu().tolist())
    live = lay.per_elem([float(x) for x in live_t]) != 0
    d = lambda k: before[k].double()
    c = float(coef) if coef is not None else None
    trust_on = True
    if kind == 'lamb':
        ref = lamb_reference(d('p'), g.double(), d('exp_avg'), d('exp_avg_sq'), gscale, c, st['bc1'], st['bc2s'], wd, lr, r,
                             eps=o.get('eps', EPS), beta1=o.get('betas', (BETA1, BETA2))[0], beta2=o.get('betas', (BETA1, BETA2))[1])
        u_ref = ref.pop('u')
    else:
        trust_on = o.get('trust_coefficient', 0.0) > 0
        ref = lars_reference(d('p'), g.double(), d('momentum_buffer') if 'momentum_buffer' in before else None, gscale, c, wd, lr, r,
                             o.get('momentum', 0.0), o.get('nesterov', False), trust_on)
        u_ref = None
    sel = live if dom is None else live & dom
    for k, e in ref.items():
        x = _ratio(after[k][sel], e.v[sel], e.e[sel]) if bool(sel.any()) else 0.0
        if not (x <= 1.0):
            fails.append(('%s %s' % (k, what), x))
    for k in after:
        rest = ~live
        if not torch.equal(after[k][rest].view(torch.int32), before[k][rest].view(torch.int32)):
            fails.append(('%s changed in the padding or in a frozen tensor %s' % (k, what), 0))
        if bool((after[k][~lay.used] != 0).any()):
            fails.append(('%s: padding not zero %s' % (k, what), 0))
        if not bool(torch.isfinite(after[k][live]).all()):
            fails.append(('%s: a non-finite value %s' % (k, what), 0))
    if trust_on:
        gr64 = torch.where(live, g.double(), torch.zeros((), dtype=torch.float64, device=g.device)) * _f32(gscale) * (c if c is not None else 1.0)
        copts = dict(always_adapt=o.get('always_adapt', False), max_trust=o.get('max_trust', 0.0),
                     trust_coefficient=o.get('trust_coefficient', 0.0), eps=o.get('lars_eps', o.get('eps', 1e-8)))
        fails += [('%s %s' % (w, what), x) for w, x in check_norms(kind, lay, norms.cpu(), trust.cpu(), before['p'], gr64, u_ref, copts, wd_t, live_t)]


class NetLayout(object):
    """the Layout interface over the parameter table of a real net and the groups of an utils.optim optimizer on it"""
    def __init__(self, opt):
        params = opt._params()
        self.offsets, self.numels, self.n = [t[2] for t in params], [t[3] for t in params], opt.net.flat_params.numel()
        self.names, self.shapes = [t[0] for t in params], [tuple(t[1]) for t in params]
        self.groups = [0] * len(params)
        for k, g in enumerate(opt.param_groups):
            for i in g.get('params', ()):
                self.groups[i] = k
        self.tensor_of = torch.full((self.n,), -1, dtype=torch.long)
        for t, (o, k) in enumerate(zip(self.offsets, self.numels)):
            self.tensor_of[o:o + k] = t
        self.used = (self.tensor_of >= 0).cuda()
        self.tensor_of = self.tensor_of.cuda()

    per_elem = Layout.per_elem


def optimizer_arrays(opt):
    """{name: the live flat array} of an utils.optim SGD / LARS / LAMB"""
    a = {'p': opt.net.flat_params}
    if hasattr(opt, 'exp_avg'):
        a.update(exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq)
    elif opt.momentum_buffer is not None:
        a['momentum_buffer'] = opt.momentum_buffer
    return a


def check_optimizer_step(opt, g, gscale, fails, what, step=None):
    """opt.step() (or `step`, which must end in it) on the flat arrays of a real net, checked per element by check_step on the domain of
    the bound: |g s| and |g s coef| at least DOMAIN or 0 (tests/optim_exact.py), moments that are normal numbers or 0 before and after
    (tests/test_gpu_groups.py says why); at least 90 % of the elements must lie in it.  g: the gradient the step applies."""
    from tests.groups_exact import normal_or_zero
    kind = 'lamb' if hasattr(opt, 'exp_avg') else 'lars'
    lay = NetLayout(opt)
    groups = [(float(g_['lr']), float(g_.get('weight_decay', 0)), bool(g_.get('frozen', False))) for g_ in opt.param_groups]
    g0 = opt.param_groups[0]
    opts = dict((k, g0[k]) for k in ('momentum', 'nesterov', 'trust_coefficient', 'lars_eps', 'always_adapt', 'max_trust', 'betas', 'eps') if k in g0)
    before = dict((k, a.clone()) for k, a in optimizer_arrays(opt).items())
    (step or opt.step)()
    torch.cuda.synchronize()
    after = optimizer_arrays(opt)
    coef = float(opt._norm_out[1]) if opt.max_grad_norm is not None else None
    gs = g.double() * _f32(gscale)
    dom = ((gs == 0) | (gs.abs() >= DOMAIN)) & ((gs * (coef or 1.0) == 0) | ((gs * (coef or 1.0)).abs() >= DOMAIN))
    state = [a for k, a in before.items() if k != 'p'] + [a for k, a in after.items() if k != 'p']
    if state:
        dom = dom & normal_or_zero(*state)
    if float(dom[lay.used].float().mean()) < 0.9:
        fails.append(('%s: less than 90 %% of the elements are in the bound\'s domain' % what, float(dom[lay.used].float().mean())))
    if not bool((g[lay.used] != 0).any()):
        fails.append(('%s: the gradient is all zero' % what, 0))
    st = read_state(opt._state) if kind == 'lamb' else None
    trust = opt._trust if opt.last_trust() is not None else torch.ones(len(lay.offsets), device='cuda')
    check_step(kind, lay, groups, opts, before, after, g, gscale, coef, st, opt._norms, trust, fails, what, dom=dom)
    return lay


def clip_of(g, lay, gscale):
    """out2 of pa_grad_norm with max_norm = half the norm (a coefficient around 0.5)"""
    from tests.optim_opts_exact import grad_norm
    norm = float(((g.double() * _f32(gscale)) ** 2).sum().sqrt())
    return grad_norm(g, lay.n, gscale, 0.5 * norm if norm > 0 else 1.0)


def grads_for(lay, seed, gscale, steps=3):
    return [Guarded(lay.scatter(canonical_inputs(seed + 100 * k, gscale, True)['g']), float('nan')) for k in range(steps)]


LAMB_COMBOS = tuple(itertools.product((0.0, 0.01), (0.0, 1.0), (False, True)))          # (wd, max_trust, clip)
LARS_COMBOS = tuple(itertools.product((0.0, 0.9), (False, True), (0.0, 1e-4), (0.0, 1e-3)))   # (momentum, nesterov, wd, trust_coefficient)


def run_lamb(log=print, steps=3):
    """three consecutive steps per (gscale, zero / non-zero state, wd, max_trust, clip); wd 0 also with always_adapt (else no ratio is formed)"""
    fails, lay = [], Layout()
    for gi, gscale in enumerate(GSCALES):
        grads = grads_for(lay, 5000 + gi, gscale, steps)
        coefs = [clip_of(G.x, lay, gscale) for G in grads]
        for zero in (True, False):
            inputs = canonical_inputs(4000 + gi, gscale, zero)
            for wd, max_trust, clip in LAMB_COMBOS:
                for always in ((False, True) if wd == 0 else (False,)):
                    S_ = Stepper('lamb', lay, inputs, [(LR, wd, False)], max_trust=max_trust, always_adapt=always)
                    what0 = 'lamb gscale %g state %s wd %g max_trust %g clip %d always %d' % (gscale, 'zero' if zero else 'nonzero', wd, max_trust, clip, always)
                    for k, (G, out2) in enumerate(zip(grads, coefs)):
                        before = S_.arrays()
                        S_.step(G, gscale, out2[1:] if clip else None)
                        torch.cuda.synchronize()
                        st = read_state(S_.state)
                        for name, x in check_consts(st, k + 1, lr=LR).items():
                            if not (x <= 1.0):
                                fails.append(('%s of the state %s step %d' % (name, what0, k), x))
                        S_.check(before, G.x, gscale, float(out2[1]) if clip else None, fails, '%s step %d' % (what0, k))
                        t = S_.trust.cpu()
                        zp, zg = lay.where(ZERO_P), lay.where(ZERO_G)
                        # (first step only: afterwards the zero tensor has moved and the other has moments)
                        if k == 0 and (float(t[zp]) != 1.0 or (zero and wd == 0 and float(t[zg]) != 1.0)):
                            fails.append(('r of the all-zero tensor / the zero-gradient tensor %s step %d' % (what0, k), (float(t[zp]), float(t[zg]))))
                        if wd == 0 and not always and not bool((t == 1.0).all()):
                            fails.append(('a tensor without decay was adapted ' + what0, 0))
                        if (wd != 0 or always) and max_trust == 0 and k == 0 and bool((t == 1.0).all()):
                            fails.append(('no ratio differs from 1: nothing was tested ' + what0, 0))
    return fails


def run_lars(log=print, steps=3):
    """momentum 0 / 0.9, Nesterov, wd 0 / 1e-4, trust_coefficient 0 / 1e-3 (always_adapt with wd 0); gscale 1 and 1/32768; with
    trust_coefficient 0 also torch.optim.SGD on a twin within the same bound"""
    fails, lay = [], Layout()
    for gi, gscale in enumerate((1.0, 1.0 / 32768.0)):
        grads = grads_for(lay, 7000 + gi, gscale, steps)
        inputs = canonical_inputs(6000 + gi, gscale, True)              # torch's momentum buffer starts at zero
        for (mom, nesterov, wd, tc), clip in itertools.product(LARS_COMBOS, (False, True)):
            if nesterov and mom == 0:
                continue
            if clip and not (mom != 0 and wd != 0):
                continue                                                 # the coefficient: with the full formula, trust on and off
            S_ = Stepper('lars', lay, inputs, [(LR, wd, False)], momentum=mom, nesterov=nesterov, trust_coefficient=tc, always_adapt=wd == 0)
            what0 = 'lars gscale %g momentum %g nesterov %d wd %g tc %g clip %d' % (gscale, mom, nesterov, wd, tc, clip)
            twin = None
            if tc == 0 and not clip:
                tp = torch.nn.Parameter(S_.a['p'].x.clone())
                twin = (torch.optim.SGD([tp], lr=_f32(LR), momentum=_f32(mom), weight_decay=_f32(wd), nesterov=nesterov), tp)
            for k, G in enumerate(grads):
                out2 = clip_of(G.x, lay, gscale) if clip else None
                before = S_.arrays()
                S_.step(G, gscale, out2[1:] if clip else None)
                torch.cuda.synchronize()
                S_.check(before, G.x, gscale, float(out2[1]) if clip else None, fails, '%s step %d' % (what0, k))
                if twin is not None:
                    # torch from the ENGINE's state before the step (a local check, like every other): p and the buffer are set, then one step
                    topt, tp = twin
                    with torch.no_grad():
                        tp.copy_(before['p'])
                    if mom != 0:
                        topt.state[tp]['momentum_buffer'] = before['momentum_buffer'].clone()
                    tp.grad = G.x * torch.tensor(_f32(gscale), dtype=torch.float32, device='cuda')
                    topt.step()
                    wdv, lrv = lay.per_elem([_f32(wd)] * len(lay.offsets)), lay.per_elem([_f32(LR)] * len(lay.offsets))
                    ref = lars_reference(before['p'].double(), G.x.double(), before['momentum_buffer'].double() if mom != 0 else None, gscale, None,
                                         wdv, lrv, None, mom, nesterov, False)
                    x = _ratio(tp.detach()[lay.used], ref['p'].v[lay.used], ref['p'].e[lay.used])
                    if not (x <= 1.0):
                        fails.append(('torch.optim.SGD itself against the reference %s step %d' % (what0, k), x))
    return fails


def run_tensor_norms():
    """pa_tensor_norms on the table and on an array with one tensor (sizes 1, 1023 and 5 S + 3), scale 1 and 1/3"""
    from pose_adv_aug_amd._lib import lib, check as ok, ptr, stream
    L, fails = lib(), []
    for lay in (Layout(), Layout(single=1), Layout(single=1023), Layout(single=5 * S + 3)):
        nt = len(lay.offsets)
        x = Guarded(lay.scatter(dict((c, torch.from_numpy(make_inputs(k, 8000 + c, 1.0, True)[1])) for c, k in enumerate(lay.numels)))
                    if nt == 1 else lay.scatter(canonical_inputs(8000, 1.0, True)['g']), float('nan'))
        ws = torch.zeros(int(L.pa_opt_layer_workspace_bytes(lay.nsegs, nt)) // 8, dtype=torch.float64, device='cuda')
        for scale in (1.0, 1.0 / 3.0):
            norms = torch.full((nt,), -1.0, dtype=torch.float32, device='cuda')
            ok(L.pa_tensor_norms(ptr(x.x), ptr(lay.segs), lay.nsegs, nt, scale, ptr(ws), ptr(norms), stream()), 'pa_tensor_norms')
            torch.cuda.synchronize()
            ref = [s ** 0.5 for s in tensor_sums(x.x.double() * _f32(scale), lay.offsets, lay.numels)]
            for t in range(nt):
                if abs(float(norms[t]) - ref[t]) > (2 * U + SLACK) * ref[t]:
                    fails.append(('pa_tensor_norms n %d tensor %d scale %g' % (lay.n, t, scale), (float(norms[t]), ref[t])))
        if not x.guards_intact():
            fails.append(('pa_tensor_norms changed a guard', 0))
    return fails


def run_groups():
    """16 interleaved groups with different lr / wd (tensor t in group t % 16; group 3 has wd 0), LAMB and LARS, two steps"""
    fails = []
    lay = Layout(groups=[t % 16 for t in range(len(SIZES))])
    groups = [(LR * (1 + 0.25 * k), 0.0 if k == 3 else 0.01 / (1 + k), False) for k in range(16)]
    grads = grads_for(lay, 9100, 1.0, 2)
    for kind, opts in (('lamb', dict()), ('lars', dict(momentum=0.9, nesterov=True, trust_coefficient=1e-3))):
        S_ = Stepper(kind, lay, canonical_inputs(9000, 1.0, False), groups, **opts)
        for k, G in enumerate(grads):
            before = S_.arrays()
            S_.step(G, 1.0)
            torch.cuda.synchronize()
            S_.check(before, G.x, 1.0, None, fails, '%s with 16 groups step %d' % (kind, k))
        if float(S_.trust[lay.where(3)]) != 1.0:
            fails.append(('%s: the tensor of the group without decay was adapted' % kind, float(S_.trust[3])))
    return fails


def run_frozen(plant=True):
    """group 1 (every third tensor) frozen: bit for bit untouched with inf / NaN planted in its gradient (bf16 build), its ratio stays at
    the sentinel it had; the other tensors' results are bit for bit those of a run without the planted values"""
    fails = []
    lay = Layout(groups=[1 if t % 3 == 1 else 0 for t in range(len(SIZES))])
    groups = [(LR, 0.01, False), (LR, 0.01, True)]
    frozen_t = [t for t in range(len(SIZES)) if t % 3 == 1]
    for kind, opts in (('lamb', dict()), ('lars', dict(momentum=0.9, trust_coefficient=1e-3))):
        runs = []
        for planted in ((False, True) if plant else (False,)):
            S_ = Stepper(kind, lay, canonical_inputs(9200, 1.0, False), groups, **opts)
            S_.trust[frozen_t] = 0.375                     # a sentinel: a frozen tensor's ratio is left as it was
            G = grads_for(lay, 9300, 1.0, 1)[0]
            if planted:
                for i, t in enumerate(frozen_t):
                    G.x[lay.offsets[t] + lay.numels[t] // 2] = (float('inf'), float('nan'), float('-inf'))[i % 3]
            before = S_.arrays()
            S_.step(G, 1.0)
            torch.cuda.synchronize()
            S_.check(before, torch.where(lay.per_elem([float(t in frozen_t) for t in range(len(SIZES))]) != 0, torch.zeros_like(G.x), G.x),
                     1.0, None, fails, '%s with a frozen group planted %d' % (kind, planted))
            if not bool((S_.trust[frozen_t] == 0.375).all()):
                fails.append(('%s: the ratio of a frozen tensor changed' % kind, S_.trust[frozen_t].tolist()))
            runs.append(S_.everything())
        if plant:
            for k in runs[0]:
                if not torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)):
                    fails.append(('%s: %s differs with inf / NaN planted in the frozen gradient' % (kind, k), 0))
    return fails


def run_determinism_and_packing():
    """the same step twice from the same bits: the same bits everywhere; the same tensors in another order with other gaps: the same
    per-tensor norms and ratios, and the same values in every tensor, bit for bit"""
    fails = []
    order = list(reversed(range(len(SIZES))))
    lays = (Layout(), Layout(), Layout(order=order, gaps=(12, 0, 4)))
    for kind, opts in (('lamb', dict(always_adapt=True)), ('lars', dict(momentum=0.9, trust_coefficient=1e-3, always_adapt=True))):
        runs = []
        for lay in lays:
            S_ = Stepper(kind, lay, canonical_inputs(9400, 1.0, False), [(LR, 0.01, False)], **opts)
            for G in grads_for(lay, 9500, 1.0, 2):
                S_.step(G, 1.0)
            torch.cuda.synchronize()
            runs.append(S_.everything())
        for k in runs[0]:
            if not torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)):
                fails.append(('%s: %s differs between two runs from the same bits' % (kind, k), 0))
        nt = len(SIZES)
        perm = torch.tensor([lays[2].where(c) for c in range(nt)], device='cuda')
        a, b = runs[0], runs[2]
        if not torch.equal(a['trust'].view(torch.int32), b['trust'][perm].view(torch.int32)):
            fails.append(('%s: the ratios depend on the layout' % kind, 0))
        for half in (0, 1):
            if not torch.equal(a['norms'][half * nt:(half + 1) * nt].view(torch.int32), b['norms'][half * nt + perm].view(torch.int32)):
                fails.append(('%s: the norms (%d) depend on the layout' % (kind, half), 0))
        for k in a:
            if k in ('trust', 'norms', 'state'):
                continue
            for c in range(nt):
                t = lays[2].where(c)
                x = a[k][lays[0].offsets[c]:lays[0].offsets[c] + SIZES[c]]
                y = b[k][lays[2].offsets[t]:lays[2].offsets[t] + SIZES[c]]
                if not torch.equal(x.view(torch.int32), y.view(torch.int32)):
                    fails.append(('%s: %s of tensor %d depends on the layout' % (kind, k, c), 0))
    return fails


def run_error_cases():
    """every listed argument error of the three device entry points: non-zero, the function's name in the message, nothing written"""
    from pose_adv_aug_amd._lib import lib, ptr, stream, LambOpts, LarsOpts
    L, fails = lib(), []
    lay = Layout()
    nt = len(lay.offsets)
    inputs = canonical_inputs(9600, 1.0, False)
    A_ = Stepper('lamb', lay, inputs, [(LR, 0.01, False)])
    B_ = Stepper('lars', lay, inputs, [(LR, 0.01, False)], momentum=0.9)
    G = grads_for(lay, 9700, 1.0, 1)[0]
    keepA, keepB = A_.everything(), B_.everything()
    odd = torch.zeros(12, dtype=torch.int32, device='cuda')
    nan, inf = float('nan'), float('inf')

    def lamb(what, o=None, tab=None, ng=1, segs=lay.segs, nsegs=lay.nsegs, nt_=nt, null=(), state=None, n=lay.n):
        o = o or LambOpts(BETA1, BETA2, EPS, 0.0, 0, 0)
        arg = dict(p=A_.a['p'].x, g=G.x, m=A_.a['exp_avg'].x, v=A_.a['exp_avg_sq'].x, ws=A_.ws, norms=A_.norms, trust=A_.trust)
        a = dict((k, None if k in null else ptr(t)) for k, t in arg.items())
        rc = L.pa_lamb_step(None if 'o' in null else C.byref(o), None if 'tab' in null else (tab or group_table([(LR, 0.01, False)])), ng,
                            None if 'segs' in null else ptr(segs), nsegs, nt_, a['p'], a['g'], a['m'], a['v'], n, 1.0, None, a['ws'], a['norms'],
                            a['trust'], None if 'state' in null else ptr(A_.state if state is None else state), stream())
        if rc == 0 or b'pa_lamb_step' not in (L.pa_last_error() or b''):
            fails.append(('pa_lamb_step accepted ' + what, rc))

    for k in ('o', 'p', 'g', 'm', 'v', 'ws', 'norms', 'trust', 'state', 'segs', 'tab'):
        lamb('NULL ' + k, null=(k,))
    for what, o in (('beta1 = 1', LambOpts(1.0, BETA2, EPS, 0.0, 0, 0)), ('beta2 < 0', LambOpts(BETA1, -0.1, EPS, 0.0, 0, 0)), ('beta1 NaN', LambOpts(nan, BETA2, EPS, 0.0, 0, 0)),
                    ('eps 0', LambOpts(BETA1, BETA2, 0.0, 0.0, 0, 0)), ('eps < 0', LambOpts(BETA1, BETA2, -1e-6, 0.0, 0, 0)),
                    ('max_trust < 0', LambOpts(BETA1, BETA2, EPS, -1.0, 0, 0)), ('max_trust inf', LambOpts(BETA1, BETA2, EPS, inf, 0, 0)),
                    ('amsgrad', LambOpts(BETA1, BETA2, EPS, 0.0, 0, 1))):
        lamb(what, o=o)
    for what, g_ in (('lr < 0', (-LR, 0.0, False)), ('lr NaN', (nan, 0.0, False)), ('wd < 0', (LR, -0.01, False)), ('wd inf', (LR, inf, False))):
        lamb(what, tab=group_table([g_]))
    lamb('ngroups 0', ng=0)
    lamb('ngroups 17', ng=17, tab=group_table([(LR, 0.0, False)] * 17))
    lamb('a misaligned state', state=odd[1:9])
    lamb('nsegs 0 with n > 0', nsegs=0)

    def lars(what, o=None, tab=None, ng=1, nsegs=lay.nsegs, null=(), buf=True):
        o = o or LarsOpts(0.9, 1e-3, 1e-8, 0, 0)
        arg = dict(p=B_.a['p'].x, g=G.x, ws=B_.ws, norms=B_.norms, trust=B_.trust, state=B_.state, segs=lay.segs)
        a = dict((k, None if k in null else ptr(t)) for k, t in arg.items())
        rc = L.pa_lars_step(None if 'o' in null else C.byref(o), None if 'tab' in null else (tab or group_table([(LR, 0.01, False)])), ng, a['segs'], nsegs,
                            nt, a['p'], a['g'], ptr(B_.a['momentum_buffer'].x) if buf else None, lay.n, 1.0, None, a['ws'], a['norms'], a['trust'],
                            a['state'], stream())
        if rc == 0 or b'pa_lars_step' not in (L.pa_last_error() or b''):
            fails.append(('pa_lars_step accepted ' + what, rc))

    for k in ('o', 'p', 'g', 'ws', 'norms', 'trust', 'state', 'segs', 'tab'):
        lars('NULL ' + k, null=(k,))
    lars('a missing momentum_buf', buf=False)
    lars('a superfluous momentum_buf', o=LarsOpts(0.0, 1e-3, 1e-8, 0, 0))
    lars('nesterov without momentum', o=LarsOpts(0.0, 1e-3, 1e-8, 1, 0), buf=False)
    for what, o in (('momentum < 0', LarsOpts(-0.9, 1e-3, 1e-8, 0, 0)), ('momentum NaN', LarsOpts(nan, 1e-3, 1e-8, 0, 0)), ('trust_coef < 0', LarsOpts(0.9, -1e-3, 1e-8, 0, 0)),
                    ('trust_coef inf', LarsOpts(0.9, inf, 1e-8, 0, 0)), ('lars_eps < 0', LarsOpts(0.9, 1e-3, -1e-8, 0, 0)), ('lars_eps NaN', LarsOpts(0.9, 1e-3, nan, 0, 0))):
        lars(what, o=o)
    lars('lr inf', tab=group_table([(inf, 0.0, False)]))
    lars('wd < 0', tab=group_table([(LR, -1.0, False)]))
    lars('ngroups 0', ng=0)
    lars('ngroups 17', ng=17, tab=group_table([(LR, 0.0, False)] * 17))
    lars('nsegs 0 with n > 0', nsegs=0)
    norms = torch.zeros(nt, device='cuda')
    for what, args in (('NULL x', (None, ptr(lay.segs), lay.nsegs, nt, 1.0, ptr(A_.ws), ptr(norms))), ('NULL segs', (ptr(G.x), None, lay.nsegs, nt, 1.0, ptr(A_.ws), ptr(norms))),
                       ('NULL workspace', (ptr(G.x), ptr(lay.segs), lay.nsegs, nt, 1.0, None, ptr(norms))), ('NULL norms', (ptr(G.x), ptr(lay.segs), lay.nsegs, nt, 1.0, ptr(A_.ws), None)),
                       ('nsegs 0', (ptr(G.x), ptr(lay.segs), 0, nt, 1.0, ptr(A_.ws), ptr(norms))), ('ntensors 0', (ptr(G.x), ptr(lay.segs), lay.nsegs, 0, 1.0, ptr(A_.ws), ptr(norms))),
                       ('scale NaN', (ptr(G.x), ptr(lay.segs), lay.nsegs, nt, nan, ptr(A_.ws), ptr(norms)))):
        rc = L.pa_tensor_norms(*(args + (stream(),)))
        if rc == 0 or b'pa_tensor_norms' not in (L.pa_last_error() or b''):
            fails.append(('pa_tensor_norms accepted ' + what, rc))
    torch.cuda.synchronize()
    for keep, now in ((keepA, A_.everything()), (keepB, B_.everything())):
        for k in keep:
            if not torch.equal(keep[k].view(torch.int32), now[k].view(torch.int32)):
                fails.append(('a refused call changed ' + k, 0))
    if bool(norms.any()) or not (A_.guards_intact() and B_.guards_intact()):
        fails.append(('a refused call wrote norms or a guard', 0))
    return fails


def run_skip_case():
    """fp16 build: one inf in the gradient (in a live tensor, in the padding-free tail, in a frozen tensor): p, every state array, the step
    count and constants, the norms and the ratios bit for bit what they were, the skip counted once; the next finite step is taken"""
    from pose_adv_aug_amd._lib import lib, check as ok, ptr, stream
    fails = []
    lay = Layout(groups=[1 if t == 2 else 0 for t in range(len(SIZES))])
    groups = [(LR, 0.01, False), (LR, 0.01, True)]
    gscale = 1.0 / 32768.0
    for kind, opts in (('lamb', dict()), ('lars', dict(momentum=0.9, trust_coefficient=1e-3)), ('lars', dict(momentum=0.9))):
        S_ = Stepper(kind, lay, canonical_inputs(9800, gscale, False), groups, **opts)
        G = grads_for(lay, 9900, gscale, 1)[0]
        S_.step(G, gscale)                                # one taken step first: norms, ratios and constants are in place

        def skipped():
            c = C.c_longlong(-1)
            if kind == 'lamb':
                t = C.c_longlong(-1)
                ok(S_.L.pa_adam_steps(ptr(S_.state), C.byref(t), C.byref(c), stream()))
            else:
                ok(S_.L.pa_rmsprop_skipped_steps_state(ptr(S_.state), C.byref(c), stream()))
            return int(c.value)

        for where, pos in (('the first tensor', 0), ('the last element of the last tensor', lay.offsets[-1] + lay.numels[-1] - 1), ('a frozen tensor', lay.offsets[2] + 1)):
            Gb = Guarded(G.x, float('nan'))
            Gb.x[pos] = float('inf')
            before, k0 = S_.everything(), skipped()
            S_.step(Gb, gscale)
            torch.cuda.synchronize()
            now = S_.everything()
            for k in before:
                a, b = before[k].view(torch.int32), now[k].view(torch.int32)
                if k == 'state':
                    a, b = a[2:], b[2:]                    # (words 0 and 1 are the flag and the skip count)
                if not torch.equal(a, b):
                    fails.append(('%s %s: %s changed on a skipped step (inf in %s)' % (kind, opts, k, where), 0))
            if skipped() != k0 + 1:
                fails.append(('%s %s: skips counted for one inf in %s' % (kind, opts, where), skipped() - k0))
            before = S_.arrays()
            S_.step(G, gscale)
            torch.cuda.synchronize()
            S_.check(before, torch.where(lay.tensor_of == 2, torch.zeros_like(G.x), G.x), gscale, None, fails, '%s %s: the finite step after a skip' % (kind, opts))
            if skipped() != k0 + 1:
                fails.append(('%s %s: a finite step was counted as skipped' % (kind, opts), 0))
    return fails


# ---------------------------------------------------------------------------------------------------------------------------------
# two ranks (tests/dist_optim_exact.py drives and records; the ratios and norms join the arrays it snapshots)
def record_trust():
    """make the snapshots of dist_optim_exact (test_gpu_accum._state) carry the trust ratios and the per-tensor norms too"""
    from tests import test_gpu_accum as TA
    if getattr(TA._state, 'with_trust', False):
        return
    plain = TA._state

    def _state(net, opt):
        return plain(net, opt) + [(k, getattr(opt, k)) for k in ('_trust', '_norms') if getattr(opt, k, None) is not None]
    _state.with_trust = True
    TA._state = _state


def dist_worker(rank, world, init, out, cases):
    """dist_optim_exact.worker with record_trust() in the spawned rank"""
    from tests import dist_optim_exact as D
    record_trust()
    getattr(D, 'plain_worker', D.worker)(rank, world, init, out, cases)          # (a spawned rank imports the module afresh)


def run_all(fp16=False):
    fails = run_lamb() + run_lars() + run_tensor_norms() + run_groups() + run_frozen(plant=not fp16) + run_determinism_and_packing() + run_error_cases()
    if fp16:
        fails += run_skip_case()
    return fails


if __name__ == '__main__':          # the fp16 build: tests/test_gpu_layerwise.py runs this with POSEADV_DTYPE=fp16
    from pose_adv_aug_amd._lib import lib as _l
    assert _l().pa_dtype() == 1, 'run with POSEADV_DTYPE=fp16'
    torch.cuda.set_device(0)
    fails = run_all(fp16=True)
    print('FAILURES %d %s' % (len(fails), fails[:20]))
    print('FP16 LAYERWISE EXACT ' + ('PASSED' if not fails else 'FAILED'), flush=True)
    sys.exit(1 if fails else 0)
