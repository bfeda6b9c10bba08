"""Parameter groups in the fused optimizer steps (rmsprop_groups_kernel, adam_groups_kernel, adam_prologue_groups_kernel,
grad_sqsum_groups_kernel, csrc/elementwise.hip; pa_rmsprop_step_groups, pa_adam_step_groups, pa_grad_norm_groups): cases and helpers.

A group is a property of a 16-byte chunk: chunk_map[i // 4] is the group of element i.  The checks are the project's own, unchanged:
for every group, the elements of that group go through optim_opts_exact.reference / adam_exact.check with THAT group's lr and
weight_decay, the engine's own clip coefficient and (Adam) the engine's own group_consts[k] as step_size; error / bound <= 1 in p and
in every state array.  The elements of a frozen group are compared bit for bit with what they held before.  With one group the whole
call is compared bit for bit with the ungrouped entry point on a copy.

Layouts (chunk -> group):  'one': a single group;  'mod16': chunk c in group c % 16;  'runs': contiguous runs with boundaries at chunks
1, 63, 64, 65, 255, 256, 257 (the wave and workgroup edges of the first workgroup) and the last chunk -- the tail, when n % 4 != 0 --
a group of its own.  Group values: lr from {0, 1e-5, 2.5e-4, 1e-3, 1e-2}, weight_decay alternating between 0 and {1e-4, 1e-2} from one
group to the next, two frozen groups in 'mod16' and 'runs' (in 'runs' the last chunk is one of them, so the tail is frozen there and
live in 'mod16').

tests/test_gpu_groups.py runs the cases; the IEEE-half build runs this file as a child process, one storage type per process.
tests/test_groups_cpu.py shows on the numpy emulations below that the per-group check is not vacuous."""
import ctypes as C
import os
import sys

import numpy as np
import torch

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.bn_exact import E, _ratio
from tests import optim_exact as X
from tests import optim_opts_exact as Y
from tests import adam_exact as A
from tests.optim_exact import Guarded, make_inputs, _f32, _t

GROUPS_MAX = 16
LRS = (0.0, 1e-5, 2.5e-4, 1e-3, 1e-2)
WDS = (1e-4, 1e-2)
RUN_BOUNDS = (1, 63, 64, 65, 255, 256, 257)
LAYOUTS = ('one', 'mod16', 'runs')
GSCALES = (1.0, 1.0 / 3.0, 1.0 / 32768.0)
# the options every group shares.  RMSprop: (momentum, centered); Adam: (decoupled, amsgrad)
RMS_COMBOS = ((0.0, False), (Y.MOM, True))
ADAM_COMBOS = ((False, True), (True, False))


def n_chunks(n):
    return (n + 3) // 4


def group_values(ngroups, frozen=()):
    """[(lr, weight_decay, frozen)]: group 0 has lr 2.5e-4 and no decay; zero and non-zero decay alternate between neighbours"""
    return [(LRS[(k + 2) % len(LRS)], 0.0 if k % 2 == 0 else WDS[(k // 2) % 2], k in frozen) for k in range(ngroups)]


def layout(name, n):
    """(chunk map as numpy uint8, [(lr, wd, frozen)] of its groups)"""
    c = np.arange(n_chunks(n))
    if name == 'one':
        return np.zeros(len(c), dtype=np.uint8), group_values(1)
    if name == 'mod16':
        return (c % 16).astype(np.uint8), group_values(16, frozen=(5, 10))
    assert name == 'runs'
    m = np.searchsorted(np.array(RUN_BOUNDS), c, side='right').astype(np.uint8)
    if len(c) > 1:
        m[-1] = len(RUN_BOUNDS) + 1
    return m, group_values(len(RUN_BOUNDS) + 2, frozen=(1, len(RUN_BOUNDS) + 1))


def numpy_chunk_map(table, n, ngroups_unused=None):
    """what pa_opt_chunk_map_host builds, from [(offset, numel, group)]: every chunk a tensor touches gets its group, a chunk no tensor
    touches the group of the tensor in front of it (0 in front of the first)"""
    m = np.zeros(n_chunks(n), dtype=np.uint8)
    filled = np.zeros(n_chunks(n), dtype=bool)
    for off, numel, grp in table:
        if numel:
            m[off // 4:(off + numel - 1) // 4 + 1] = grp
            filled[off // 4:(off + numel - 1) // 4 + 1] = True
    cur = 0
    for i in range(len(m)):
        if filled[i]:
            cur = m[i]
        else:
            m[i] = cur
    return m


def elem_groups(cmap, n):
    """group of every element, from a chunk map (numpy or torch)"""
    if torch.is_tensor(cmap):
        return cmap.repeat_interleave(4)[:n]
    return np.repeat(cmap, 4)[:n]


def group_table(groups):
    from pose_adv_aug_amd._lib import OptGroup
    tab = (OptGroup * len(groups))()
    for k, (lr, wd, frozen) in enumerate(groups):
        tab[k].lr, tab[k].weight_decay, tab[k].frozen = lr, wd, int(frozen)
    return tab


def frozen_mask(groups):
    return sum(1 << k for k, g in enumerate(groups) if g[2])


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy fp32 emulations of the grouped kernels (the formulas of tests/test_optim_opts_cpu.py and tests/test_adam_cpu.py with per-element
# lr / wd / frozen from the chunk map), and the defects a per-group check has to catch
f = np.float32
DEFECTS_BOTH = ('map indexed by element', 'weight_decay of group 0', 'lr of group 0', 'frozen second moment moves')
DEFECTS_ADAM = ('decoupled factor of the next group', 'step size of the group in front')


def _per_element(cmap, n, groups, defect):
    eg = elem_groups(cmap, n)
    if defect == 'map indexed by element':
        eg = cmap[np.minimum(np.arange(n), len(cmap) - 1)]
    lr = np.array([g[0] for g in groups], dtype=f)
    wd = np.array([g[1] for g in groups], dtype=f)
    fr = np.array([g[2] for g in groups], dtype=bool)
    lr_e = np.full(n, lr[0], dtype=f) if defect == 'lr of group 0' else lr[eg]
    wd_e = np.full(n, wd[0], dtype=f) if defect == 'weight_decay of group 0' else wd[eg]
    return eg, lr_e, wd_e, fr[eg]


def emulate_rmsprop(s, g, gscale, coef, mom, centered, cmap, groups, defect=None):
    n = len(g)
    eg, lr, w, frozen = _per_element(cmap, n, groups, defect)
    alpha, eps, m = f(X.ALPHA), f(X.EPS), f(mom)
    c = f(1) - alpha
    p, v, buf, ga = s['p'], s['square_avg'], s['momentum_buffer'], s['grad_avg']
    gr = g * f(gscale)
    if coef is not None:
        gr = gr * f(coef)
    gr = np.where(w != 0, gr + w * p, gr)
    vv = alpha * v + c * gr * gr
    out = {'square_avg': vv}
    var = vv
    if centered:
        out['grad_avg'] = alpha * ga + c * gr
        var = np.maximum(f(0), vv - out['grad_avg'] * out['grad_avg'])
    q = gr / (np.sqrt(var) + eps)
    if mom > 0:
        out['momentum_buffer'] = m * buf + q
        out['p'] = p - lr * out['momentum_buffer']
    else:
        out['p'] = p - lr * q
    for k in out:
        moves = defect == 'frozen second moment moves' and k == 'square_avg'
        out[k] = np.where(frozen & (not moves), s[k], out[k]).astype(f)
    return out


def adam_consts(t, groups, defect=None):
    """(the state's constants as adam_prologue_groups_kernel forms them, group_consts)"""
    bc1 = f(1.0 - float(f(A.BETA1)) ** t)
    bc2 = f(1.0 - float(f(A.BETA2)) ** t)
    lr = [f(g[0]) for g in groups]
    if defect == 'step size of the group in front':
        lr = [lr[k - 1] for k in range(len(lr))]
    gc = np.array([x / bc1 for x in lr], dtype=f)
    return {'step': t, 'bc1': float(bc1), 'bc2': float(bc2), 'step_size': float(gc[0]), 'bc2s': float(np.sqrt(bc2))}, gc


def emulate_adam(s, g, gscale, coef, decoupled, amsgrad, cmap, groups, c, gc, defect=None):
    n = len(g)
    eg, lr, w, frozen = _per_element(cmap, n, groups, defect)
    b2, eps = f(A.BETA2), f(A.EPS)
    o1, o2 = f(1) - f(A.BETA1), f(1) - b2
    cd = np.array([A.c_dec(gr_[0], gr_[1]) for gr_ in groups], dtype=f)
    if defect == 'lr of group 0':
        cd = np.array([A.c_dec(groups[0][0], gr_[1]) for gr_ in groups], dtype=f)
    cd_e = cd[eg] if defect != 'weight_decay of group 0' else np.array([A.c_dec(gr_[0], groups[0][1]) for gr_ in groups], dtype=f)[eg]
    step_e = gc[eg] if defect != 'lr of group 0' else np.full(n, gc[0], dtype=f)
    p, m, v, vmax = s['p'], s['exp_avg'], s['exp_avg_sq'], s['max_exp_avg_sq']
    gr = g * f(gscale)
    if coef is not None:
        gr = gr * f(coef)
    decays = w != 0
    if decoupled:
        p = np.where(decays, p * cd_e, p)
        if defect == 'decoupled factor of the next group':
            p = np.where(decays, p, p * cd[(eg + 1) % len(groups)])
    else:
        gr = np.where(decays, gr + w * p, gr)
    mm = m + (gr - m) * o1
    vv = b2 * v + (o2 * gr) * gr
    out = {'exp_avg': mm, 'exp_avg_sq': vv}
    vhat = vv
    if amsgrad:
        out['max_exp_avg_sq'] = vhat = np.maximum(vmax, vv)
    out['p'] = p - step_e * (mm / (np.sqrt(vhat) / f(c['bc2s']) + eps))
    for k in out:
        moves = defect == 'frozen second moment moves' and k == 'exp_avg_sq'
        out[k] = np.where(frozen & (not moves), s[k], out[k]).astype(f)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the per-group checks (numpy or device tensors)
def _tt(a):
    return None if a is None else (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)))


def _bits_equal(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def check_groups(kind, before, g, after, gscale, coef, opts, eg, groups, consts=None, group_consts=None):
    """kind 'rmsprop': opts = (momentum, centered); 'adam': opts = (decoupled, amsgrad), consts the engine's state, group_consts its
    per-group step sizes.  Returns {(group, array name): error / bound; for a frozen group 0.0 when bit-identical, inf otherwise}."""
    before, after, g, eg = dict((k, _tt(a)) for k, a in before.items()), dict((k, _tt(a)) for k, a in after.items()), _tt(g), _tt(eg)
    out = {}
    for k, (lr, wd, frozen) in enumerate(groups):
        sel = eg == k
        if not bool(sel.any()):
            continue
        pick = lambda d: dict((name, None if a is None else a[sel]) for name, a in d.items())
        b, a_ = pick(before), pick(after)
        if frozen:
            for name in b:
                if b[name] is not None and a_.get(name) is not None:
                    out[(k, name)] = 0.0 if _bits_equal(a_[name], b[name]) else float('inf')
            continue
        d = lambda t: None if t is None else t.double()
        if kind == 'rmsprop':
            mom, centered = opts
            ref, reach = Y.reference(d(b['p']), g[sel].double(), d(b['square_avg']), d(b['momentum_buffer']) if mom > 0 else None,
                                     d(b['grad_avg']) if centered else None, gscale, coef, mom, wd, centered, lr=lr)
            r = dict((name, _ratio(a_[name], e.v, e.e)) for name, e in ref.items())
            if reach:
                r['interval of v - ga^2 reaches 0'] = float('inf')
        else:
            decoupled, amsgrad = opts
            if not amsgrad:
                b, a_ = dict(b, max_exp_avg_sq=None), dict(a_, max_exp_avg_sq=None)
            r, _ = A.check(b, g[sel], a_, gscale, coef, {'bc2s': consts['bc2s'], 'step_size': float(group_consts[k])}, wd, decoupled,
                           amsgrad, lr=lr)
        for name, x in r.items():
            out[(k, name)] = x if x == x else float('nan')
    return out


def normal_or_zero(*arrays):
    """elements at which every array holds a normal fp32 number or 0: the bounds' rounding model is relative (optim_exact.DOMAIN keeps the
    gradient there; on a real net the moments need the same, see test_gpu_groups' real-net test)"""
    ok = None
    for a in arrays:
        if a is not None:
            here = (a == 0) | (a.abs() >= 2.0 ** -126)
            ok = here if ok is None else ok & here
    return ok


def check_group_consts(c, group_consts, groups, t):
    """the state's constants (adam_exact.check_consts with group 0's lr), every group_consts[k] as ONE fp32 division of lr_k by the
    engine's bc1 (E.div), and step_size == group_consts[0] bit for bit.  Returns {name: error / bound}."""
    r = A.check_consts(c, t, lr=groups[0][0])
    for k, (lr, _, _) in enumerate(groups):
        q = E(_f32(lr)).div(E(c['bc1']))
        r['group_consts[%d]' % k] = abs(float(group_consts[k]) - float(q.v)) / max(float(q.e), 1e-300) if lr != 0 else (0.0 if float(group_consts[k]) == 0 else float('inf'))
    r['step_size is group_consts[0]'] = 0.0 if np.float32(c['step_size']).tobytes() == np.float32(float(group_consts[0])).tobytes() else float('inf')
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU cases
class RmsGroups(Y.OptStepper):
    """optim_opts_exact.OptStepper behind pa_rmsprop_step_groups; o->lr and o->weight_decay hold values the call must ignore"""
    def __init__(self, mom, centered, groups, cmap, p, v, buf, ga):
        Y.OptStepper.__init__(self, mom, 0.0, centered, p, v, buf, ga)
        self.groups, self.cmap = groups, cmap

    def step(self, g, gscale, coef=None):
        from pose_adv_aug_amd._lib import check as ok, ptr, stream, RmspropOpts
        x = lambda k: None if self.a[k] is None else ptr(self.a[k].x)
        o = RmspropOpts(77.0, X.ALPHA, X.EPS, self.mom, 55.0, int(self.centered))
        ok(self.L.pa_rmsprop_step_groups(C.byref(o), group_table(self.groups), len(self.groups), None if self.cmap is None else ptr(self.cmap),
                                         x('p'), ptr(g.x), x('square_avg'), x('momentum_buffer'), x('grad_avg'), g.x.numel(), float(gscale),
                                         None if coef is None else ptr(coef), ptr(self.state), stream()), 'pa_rmsprop_step_groups')


class AdamGroups(A.AdamStepper):
    """adam_exact.AdamStepper behind pa_adam_step_groups, with its group_consts array (guarded: 16 floats)"""
    def __init__(self, decoupled, amsgrad, groups, cmap, p, m, v, vmax, consts=True):
        A.AdamStepper.__init__(self, 0.0, decoupled, amsgrad, p, m, v, vmax)
        self.groups, self.cmap = groups, cmap
        self.consts = Guarded(torch.full((GROUPS_MAX,), -1.0), 11.0) if consts else None

    def step(self, g, gscale, coef=None):
        from pose_adv_aug_amd._lib import check as ok, ptr, stream, AdamOpts
        x = lambda k: None if self.a[k] is None else ptr(self.a[k].x)
        o = AdamOpts(77.0, A.BETA1, A.BETA2, A.EPS, 55.0, int(self.amsgrad), int(self.decoupled))
        ok(self.L.pa_adam_step_groups(C.byref(o), group_table(self.groups), len(self.groups), None if self.cmap is None else ptr(self.cmap),
                                      None if self.consts is None else ptr(self.consts.x), x('p'), ptr(g.x), x('exp_avg'), x('exp_avg_sq'),
                                      x('max_exp_avg_sq'), g.x.numel(), float(gscale), None if coef is None else ptr(coef), ptr(self.state),
                                      stream()), 'pa_adam_step_groups')

    def guards_intact(self):
        return A.AdamStepper.guards_intact(self) and (self.consts is None or self.consts.guards_intact())


def norm_groups(g, n, cmap, excluded, gscale, max_norm):
    """pa_grad_norm_groups over the n floats of tensor g -> the engine's out2"""
    from pose_adv_aug_amd._lib import lib, check as ok, ptr, stream
    L = lib()
    ws = torch.empty(int(L.pa_grad_norm_workspace_bytes(n)) // 8, dtype=torch.float64, device='cuda')
    out2 = torch.zeros(2, dtype=torch.float32, device='cuda')
    ok(L.pa_grad_norm_groups(ptr(g), n, None if cmap is None else ptr(cmap), int(excluded), float(gscale), float(max_norm), ptr(ws), ptr(out2),
                             stream()), 'pa_grad_norm_groups')
    return out2


def is_bf16():
    from pose_adv_aug_amd._lib import lib
    return lib().pa_dtype() == 0


def make_grads(n, seed, gscale, frozen_e, steps=3):
    """[(Guarded gradient, its copy with the frozen elements zeroed, max_norm = half the norm of the live part)].  bf16 build: inf and
    NaN planted in the FROZEN elements only (the half-precision build scans the whole gradient and would skip the step)."""
    out = []
    for k in range(steps):
        g = _t(make_inputs(n, seed + k, gscale, True)[1])
        if is_bf16() and bool(frozen_e.any()):
            idx = frozen_e.nonzero().flatten()
            g[idx[0]] = float('inf')
            g[idx[-1]] = float('nan')
            g[idx[len(idx) // 2]] = float('-inf')
        live = torch.where(frozen_e, torch.zeros_like(g), g)
        norm = float(((live.double() * _f32(gscale)) ** 2).sum().sqrt())
        out.append((Guarded(g, float('nan')), live, 0.5 * norm if norm > 0 else 1.0))
    return out


def run_norm(n, name):
    """pa_grad_norm_groups with the layout's frozen groups excluded is bit for bit pa_grad_norm on the gradient with those chunks zeroed
    (inf / NaN planted in them in the bf16 build); with nothing excluded it is bit for bit pa_grad_norm, with and without a map"""
    fails = []
    cmap_h, groups = layout(name, n)
    cmap = _t(cmap_h)
    frozen_e = _t(np.array([g[2] for g in groups]))[elem_groups(cmap, n).long()]
    for gscale in (1.0, 1.0 / 32768.0):
        G, live, max_norm = make_grads(n, 4100, gscale, frozen_e, steps=1)[0]
        got = norm_groups(G.x, n, cmap, frozen_mask(groups), gscale, max_norm)
        want = Y.grad_norm(live, n, gscale, max_norm)
        torch.cuda.synchronize()
        if not _bits_equal(got, want):
            fails.append(('norm with excluded groups, n %d %s gscale %g' % (n, name, gscale), (got.tolist(), want.tolist())))
        if not torch.isfinite(got).all():
            fails.append(('norm not finite, n %d %s gscale %g' % (n, name, gscale), got.tolist()))
        for m in (cmap, None):
            got = norm_groups(live, n, m, 0, gscale, max_norm)
            if not _bits_equal(got, want):
                fails.append(('norm with nothing excluded, n %d %s gscale %g' % (n, name, gscale), (got.tolist(), want.tolist())))
        if not G.guards_intact():
            fails.append(('guard elements changed', 0))
    return fails


def _states(kind, n, seed, gscale, zero):
    p, _, v = make_inputs(n, seed, gscale, zero)
    a, b = (Y.make_state if kind == 'rmsprop' else A.make_state)(n, seed, v, zero)
    return _t(p), _t(v), _t(a), _t(b)


def run_one_group(kind, n, log=print, steps=3):
    """Layout 'one': every array, the state words and the norm output bit for bit those of the ungrouped call on a copy; with a chunk
    map and without one; Adam with and without a group_consts array, whose [0] is the state's step_size"""
    fails = []
    cmap = _t(layout('one', n)[0])
    groups = [(1e-3, 1e-2, False)]
    lr, wd, _ = groups[0]
    none = torch.zeros(n, dtype=torch.bool, device='cuda')
    for gi, gscale in enumerate(GSCALES):
        grads = make_grads(n, 5000 + 10 * gi, gscale, none, steps)
        for zero in (True, False):
            p, v, s1, s2 = _states(kind, n, 4900 + gi, gscale, zero)
            for opts in (RMS_COMBOS if kind == 'rmsprop' else ADAM_COMBOS):
                for clip in (False, True):
                    for m in (cmap, None):
                        if kind == 'rmsprop':
                            S, R = RmsGroups(opts[0], opts[1], groups, m, p, v, s1, s2), Y.OptStepper(opts[0], wd, opts[1], p, v, s1, s2)
                        else:
                            S = AdamGroups(opts[0], opts[1], groups, m, p, s1, v, s2, consts=m is not None)
                            R = A.AdamStepper(wd, opts[0], opts[1], p, s1, v, s2)
                        what = '%s one group n %d opts %s clip %d map %d gscale %g state %s' % (kind, n, opts, clip, m is not None, gscale, 'zero' if zero else 'nonzero')
                        for k, (G, live, max_norm) in enumerate(grads):
                            c1 = norm_groups(G.x, n, m, 0, gscale, max_norm)
                            c2 = Y.grad_norm(G.x, n, gscale, max_norm)
                            S.step(G, gscale, c1[1:] if clip else None)
                            if kind == 'rmsprop':           # the ungrouped call with the group's lr
                                from pose_adv_aug_amd._lib import check as ok, ptr, stream, RmspropOpts
                                x = lambda key: None if R.a[key] is None else ptr(R.a[key].x)
                                o = RmspropOpts(lr, X.ALPHA, X.EPS, R.mom, wd, int(R.centered))
                                ok(R.L.pa_rmsprop_step_opts(C.byref(o), x('p'), ptr(G.x), x('square_avg'), x('momentum_buffer'), x('grad_avg'), n,
                                                            float(gscale), ptr(c2[1:]) if clip else None, ptr(R.state), stream()), 'pa_rmsprop_step_opts')
                            else:
                                from pose_adv_aug_amd._lib import check as ok, ptr, stream
                                x = lambda key: None if R.a[key] is None else ptr(R.a[key].x)
                                o = A._opts(wd, R.decoupled, R.amsgrad, lr=lr)
                                ok(R.L.pa_adam_step(C.byref(o), x('p'), ptr(G.x), x('exp_avg'), x('exp_avg_sq'), x('max_exp_avg_sq'), n, float(gscale),
                                                    ptr(c2[1:]) if clip else None, ptr(R.state), stream()), 'pa_adam_step')
                            torch.cuda.synchronize()
                            a, b = S.arrays(), R.arrays()
                            for name in a:
                                if a[name] is not None and not _bits_equal(a[name], b[name]):
                                    fails.append(('%s differs from the ungrouped call: %s step %d' % (name, what, k), int((a[name] != b[name]).sum())))
                            if not torch.equal(S.state, R.state):
                                fails.append(('the state words differ from the ungrouped call: %s step %d' % (what, k), (S.state.tolist(), R.state.tolist())))
                            if not _bits_equal(c1, c2):
                                fails.append(('the norm output differs: %s step %d' % (what, k), 0))
                            if kind == 'adam' and S.consts is not None and not _bits_equal(S.consts.x[:1], S.state[6:7].view(torch.float32)):
                                fails.append(('group_consts[0] is not the state\'s step_size: %s step %d' % (what, k), float(S.consts.x[0])))
                            if not (S.guards_intact() and G.guards_intact()):
                                fails.append(('guard elements changed %s step %d' % (what, k), 0))
    return fails


# optim_opts_exact.SEED_BUMP's input artefact, met here too: with weight decay, g s coef + wd p can cancel to within its own rounding error
# (a few in 1e9 of the drawn elements), and E, which treats v' and ga'^2 as independent, then cannot keep the interval of their
# difference away from 0.  The check reports that count as a failure of its own; the seeds are fixed per case, to draws for which it is 0
# on the engine.  A count that turns nonzero after a change of the kernel's arithmetic asks for another draw here, not for a wider check.
SEED_BUMP = {('rmsprop', 'mod16', X.GRID_ELEMS + 3): 1}


def run_groups(kind, n, name, log=print, steps=3):
    """Layouts 'mod16' and 'runs': every gscale, from zero and from non-zero state, both option pairs, with and without a clip coefficient
    (pa_grad_norm_groups over the live groups, max_norm = half that norm): `steps` consecutive steps, each checked per group from the
    engine's own arrays before it (check_groups); Adam's constants after every step (check_group_consts); guards intact; the skip
    counter unmoved.  bf16 build: inf / NaN in the gradient of the frozen chunks."""
    fails = []
    cmap_h, groups = layout(name, n)
    cmap = _t(cmap_h)
    eg = elem_groups(cmap, n).long()
    frozen_e = _t(np.array([g[2] for g in groups]))[eg]
    worst = {}
    seed = 100 * SEED_BUMP.get((kind, name, n), 0)
    for gi, gscale in enumerate(GSCALES):
        grads = make_grads(n, 5100 + seed + 10 * gi, gscale, frozen_e, steps)
        coefs = [norm_groups(G.x, n, cmap, frozen_mask(groups), gscale, max_norm) for G, _, max_norm in grads]
        for zero in (True, False):
            p, v, s1, s2 = _states(kind, n, 4950 + seed + gi, gscale, zero)
            for opts in (RMS_COMBOS if kind == 'rmsprop' else ADAM_COMBOS):
                for clip in (False, True):
                    S = RmsGroups(opts[0], opts[1], groups, cmap, p, v, s1, s2) if kind == 'rmsprop' else AdamGroups(opts[0], opts[1], groups, cmap, p, s1, v, s2)
                    what = '%s %s n %d opts %s clip %d gscale %g state %s' % (kind, name, n, opts, clip, gscale, 'zero' if zero else 'nonzero')
                    for k, ((G, live, _), out2) in enumerate(zip(grads, coefs)):
                        before = S.arrays()
                        S.step(G, gscale, out2[1:] if clip else None)
                        torch.cuda.synchronize()
                        c = gc = None
                        if kind == 'adam':
                            c, gc = A.read_state(S.state), S.consts.x[:len(groups)].cpu()
                            for key, x in check_group_consts(c, gc, groups, k + 1).items():
                                if not (x <= 1.0):
                                    fails.append(('%s of the constants %s step %d' % (key, what, k), x))
                            if not bool((S.consts.x[len(groups):] == -1.0).all()):
                                fails.append(('group_consts written at or above ngroups %s step %d' % (what, k), 0))
                        after = S.arrays()
                        # the live elements: the gradient the kernel read there is `live`'s (the frozen ones hold inf / NaN)
                        r = check_groups(kind, before, live, after, gscale, float(out2[1]) if clip else None, opts, eg, groups, c, gc)
                        for key, x in r.items():
                            worst[key[1]] = max(worst.get(key[1], 0.0), x) if x == x else x
                            if not (x <= 1.0):
                                fails.append(('group %d %s %s step %d' % (key[0], key[1], what, k), x))
                        for key, a in after.items():
                            if a is not None and not bool(torch.isfinite(a).all()):
                                fails.append(('non-finite value in %s %s step %d' % (key, what, k), 0))
                        if not (S.guards_intact() and G.guards_intact()):
                            fails.append(('guard elements changed %s step %d' % (what, k), 0))
                    counts = (S.skipped(),) if kind == 'rmsprop' else S.counts()
                    if counts != ((0,) if kind == 'rmsprop' else (steps, 0)):
                        fails.append(('step / skip counters after finite live gradients ' + what, counts))
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('groups_exact %s %s n %d: worst error / bound %s' % (kind, name, n, worst))
    return fails


def run_set_steps(name='runs', n=1023):
    """from pa_adam_set_steps(1000) the next grouped step writes the constants of t = 1001 for every group"""
    fails = []
    cmap_h, groups = layout(name, n)
    cmap = _t(cmap_h)
    eg = elem_groups(cmap, n).long()
    frozen_e = _t(np.array([g[2] for g in groups]))[eg]
    p, v, m, vmax = _states('adam', n, 4990, 1.0, False)
    S = AdamGroups(True, True, groups, cmap, p, m, v, vmax)
    G, live, _ = make_grads(n, 5200, 1.0, frozen_e, 1)[0]
    S.set_steps(1000)
    before = S.arrays()
    S.step(G, 1.0)
    torch.cuda.synchronize()
    c, gc = A.read_state(S.state), S.consts.x[:len(groups)].cpu()
    rc = check_group_consts(c, gc, groups, 1001)
    if not all(x <= 1.0 for x in rc.values()):
        fails.append(('constants at t = 1001', rc))
    if all(x <= 1.0 for x in check_group_consts(c, gc, groups, 1).values()):
        fails.append(('the constants of t = 1 pass as well: the check says nothing', c))
    r = check_groups('adam', before, live, S.arrays(), 1.0, None, (True, True), eg, groups, c, gc)
    if not all(x <= 1.0 for x in r.values()):
        fails.append(('the step from t = 1000', dict((k, x) for k, x in r.items() if not x <= 1.0)))
    return fails


def run_frozen_skip(kind, log=print):
    """fp16 build.  A non-finite value in a FROZEN chunk skips the whole step: every array bit-unchanged, skipped + 1, Adam's step, its
    constants and group_consts unchanged; a pa_ema_advance behind it holds.  Then a finite step is taken and within the bound."""
    import ctypes
    from pose_adv_aug_amd._lib import lib, check as ok, ptr, stream
    n, gscale, name = X.GRID_ELEMS + 7, 1.0 / 32768.0, 'mod16'
    fails = []
    cmap_h, groups = layout(name, n)
    cmap = _t(cmap_h)
    eg = elem_groups(cmap, n).long()
    frozen_e = _t(np.array([g[2] for g in groups]))[eg]
    p, v, s1, s2 = _states(kind, n, 4995, gscale, False)
    opts = RMS_COMBOS[1] if kind == 'rmsprop' else ADAM_COMBOS[0]
    S = RmsGroups(opts[0], opts[1], groups, cmap, p, v, s1, s2) if kind == 'rmsprop' else AdamGroups(opts[0], opts[1], groups, cmap, p, s1, v, s2)
    G, live, max_norm = make_grads(n, 5300, gscale, frozen_e, 1)[0]
    out2 = norm_groups(G.x, n, cmap, frozen_mask(groups), gscale, max_norm)
    S.step(G, gscale, out2[1:])                     # one taken step first: Adam's constants of t = 1 are in the state
    ema = torch.zeros(8, dtype=torch.int32, device='cuda')
    idx = frozen_e.nonzero().flatten()
    for where, pos in (('first frozen element', int(idx[0])), ('last frozen element', int(idx[-1]))):
        for bad in (float('inf'), float('nan')):
            what = '%s %s at the %s' % (kind, bad, where)
            Gb = Guarded(G.x, float('nan'))
            Gb.x[pos] = bad
            before, s0 = S.arrays(), S.state.clone()
            gc0 = None if kind == 'rmsprop' else S.consts.x.clone()
            e0 = ema.clone()
            S.step(Gb, gscale, out2[1:])
            ok(lib().pa_ema_advance(ptr(ema), 0.99, 0, ptr(S.state), stream()), 'pa_ema_advance')
            torch.cuda.synchronize()
            after = S.arrays()
            changed = sum(int((after[k].view(torch.int32) != before[k].view(torch.int32)).sum()) for k in after if after[k] is not None)
            if changed:
                fails.append(('an array changed on a skipped step: ' + what, changed))
            if int(S.state[1]) != int(s0[1]) + 1 or int(S.state[0]) != 1:
                fails.append(('flag / skipped after the poisoned step: ' + what, S.state.tolist()))
            if kind == 'adam' and not (torch.equal(S.state[2:], s0[2:]) and _bits_equal(S.consts.x, gc0)):
                fails.append(('step, a constant or group_consts changed on a skipped step: ' + what, 0))
            if int(ema[0]) != int(e0[0]) or int(ema[1]) != int(e0[1]) + 1:
                fails.append(('the EMA behind a skipped step did not hold: ' + what, ema.tolist()))
            S.step(G, gscale, out2[1:])
            torch.cuda.synchronize()
            c = gc = None
            if kind == 'adam':
                c, gc = A.read_state(S.state), S.consts.x[:len(groups)].cpu()
            r = check_groups(kind, before, live, S.arrays(), gscale, float(out2[1]), opts, eg, groups, c, gc)
            if not all(x <= 1.0 for x in r.values()):
                fails.append(('the next finite step: ' + what, dict((k, x) for k, x in r.items() if not x <= 1.0)))
            if not S.guards_intact():
                fails.append(('guard elements changed: ' + what, 0))
    return fails


if __name__ == '__main__':          # the fp16 build: tests/test_gpu_groups.py runs this with POSEADV_DTYPE=fp16
    from pose_adv_aug_amd._lib import lib as _l
    assert _l().pa_dtype() == 1, 'run with POSEADV_DTYPE=fp16'
    torch.cuda.set_device(0)
    out = lambda s: print(s, flush=True)
    # arguments: `rmsprop|adam n [n ...]` = the exact cases of one optimizer at these sizes; `rest` = the frozen overflow, the norm, set_steps
    fails = []
    if sys.argv[1] == 'rest':
        for kind in ('rmsprop', 'adam'):
            fails += run_frozen_skip(kind, log=out)
        for n in Y.NORM_SIZES:
            for name in LAYOUTS:
                fails += run_norm(n, name)
        fails += run_set_steps()
    else:
        kind = sys.argv[1]
        for n in (int(a) for a in sys.argv[2:]):
            fails += run_one_group(kind, n, log=out)
            for name in ('mod16', 'runs'):
                fails += run_groups(kind, n, name, log=out)
            out('%s n %d done, %d failures so far' % (kind, n, len(fails)))
    print('FAILURES %d %s' % (len(fails), fails[:20]))
    print('FP16 GROUPS EXACT ' + ('PASSED' if not fails else 'FAILED'), flush=True)
    sys.exit(1 if fails else 0)
