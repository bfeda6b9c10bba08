"""Exact checks of the ASN agent (csrc/asn.hip) after ONE agent step -- the pose net in eval mode, the agent in train mode, the modes
of train_agent_sr; the first agent step after the bind ('fresh') or one behind pose and agent optimizer steps or eval-mode and
unfinished agent forwards (tests/exact_history.py) -- recomputed in float64 from the tensors the engine itself stored (pa_asn_debug_tensor / pa_hg_debug_tensor views
0-4, include/poseadv.h):
  * the 12 residual blocks (in0..4 = residual_skip1-4 / residual_neck, merge0..3 = merge1-4, deep0..2 = deep_merge.0-2) with the per-block
    checks of tests/conv_exact.py (Checker.block) and the per-BatchNorm checks of tests/bn_exact.py (check_bn_site): one definition of
    every bound.  The five input blocks read the pose net's hg0.skip1-4 / hg0.neck in place: their conv1 operand is rnd(view 0) of the
    POSE net's tensor (its eval-mode constants), they give no input gradient (Residual::bwd with need_dx = false, asn.hip:336-338) and
    the pose net's flat_grads must stay zero;
  * pool+add forward (pooladd_fwd_kernel asn.hip:26-38: one fp32 max chain, one add, one rounding) bit for bit, and its backward
    (asn.hip:332-335): the plain gradient of pa<k> through the ReLU mask of in<k+1> (pa_launch_ep_apply) and routed to the first maximum
    of hi under hi's ReLU mask (pa_launch_maxpool_bwd with a BatchNorm-backward epilogue, no addend), both bit for bit
    (bn_exact.check_pool_bwd).  The sums these launches feed to the BatchNorm backward of lo / hi are the BatchNorm checks' (sum_depth
    models the streaming kernels);
  * the scale/rotation head (asn_head_fwd_kernel asn.hip:54-88, asn_head_bwd_kernel :94-123, asn_fc_wgrad_kernel :126-142), for
    log_eps 1e-7 and 0, by the class E of tests/bn_exact.py.  Depths read from the kernels: feat = 16 adds from 0 (15 roundings) and a
    division (:59-65): the mean of the TOP-LEFT 4 x 4 window of the top map (AvgPool2d(4) + view + Linear of the reference); a logit = C
    fmas from the bias (:74-75); the softmax = a subtraction, expf, a chain of K <= 7 adds, a division (:82-86); the loss = per sample
    and head a chain of K terms t (logf t - logf(p + eps)) over t > 0 only, a division by B and 2 B atomic adds in any order (:104,
    :113); dlogits = gs p (g - sum g p), g = -t / (B (p + eps)) (:105-109); fc weight / bias gradients = chains of B fmas / adds
    (:133, :138); d act = a chain of K = 14 fmas, the division by 16 and one rounding to the storage type inside the window, 0 outside
    (:118-121), then the ReLU mask of deep2 (pa_launch_ep_apply, :323).  probs and dlogits are not exposed: they are propagated as E
    terms from the OBSERVED logits (exact fp32 inputs of the softmax), feat from view 0 of deep2;
  * the occlusion head (asn_mask_head_fwd_kernel :147-157: C / 64 fmas per lane, 6 shuffle adds, the bias; asn_mask_head_bwd_kernel
    :160-177: chains over the B 16 rows);
  * eval mode (bn_exact.check_eval on every BatchNorm'd tensor) and update_running=False (running estimates unchanged bit for bit,
    logits equal to those of the updating pass).

expf / logf: no document of the ROCm installation this was written against states their error (its HIP documentation holds the runtime
API only; the math headers give no figure), so each is charged 2 ulp = 4u of its result.  That is an ASSUMPTION, not a measurement of
the code under test; the published HIP math tables list both at 1 ulp.

Conditioning of the legs.  The BatchNorm bounds degenerate when |mean| / sigma of a channel exceeds about 10 (tests/bn_exact.py).  The
fp32 oracle agent on the fp32 oracle pose features with the legs' seeds and sizes (CPU, train-mode agent) gives a largest |mean| / sigma
over all 36 BatchNorms of 2.4 - 3.3 (LARGEST_MEAN_OVER_SIGMA below, per leg; the largest at chan 512) once the pose net's running
estimates are calibrated (oracle_pair); with the deterministic fill's arbitrary estimates it is 140 - 500 in bn1 of the five input blocks.  A leg asserts
nothing about these figures: a degenerate bound on the GPU is reported as a failure of its own."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import bn_exact as BX
from tests import conv_exact as CX
from tests.bn_exact import E, U

# largest |mean| / sigma over the agent's BatchNorm inputs, fp32 oracle on the CPU (oracle_conditioning below;
# tests/test_asn_exact_cpu.py::test_oracle_conditioning recomputes the small entries): {(chan, B, res, seed, occlusion agent): value}
LARGEST_MEAN_OVER_SIGMA = {(256, 24, 256, 51, False): 2.38, (256, 3, 384, 52, False): 2.70, (128, 4, 256, 53, False): 2.70,
                           (256, 24, 256, 54, True): 2.50, (128, 2, 256, 55, True): 2.37, (256, 3, 384, 56, False): 2.60,
                           (512, 2, 256, 60, False): 3.07, (512, 2, 256, 61, True): 2.83, (512, 2, 256, 62, False): 3.25,
                           (256, 3, 320, 91, False): 2.55, (128, 2, 448, 92, False): 2.76, (128, 2, 448, 93, False): 2.70}

IN_PREFIX = ['residual_skip1.', 'residual_skip2.', 'residual_skip3.', 'residual_skip4.', 'residual_neck.']
POSE_FEATS = ['hg0.skip1', 'hg0.skip2', 'hg0.skip3', 'hg0.skip4', 'hg0.neck']


def block_sites():
    """(parameter prefix, hook name of the output, input in the pose net?, hook name of the input) of the agent's 12 residual blocks, wired
    as Net::asn_forward_trunk (asn.hip:243-262)."""
    s = [(IN_PREFIX[k], 'in%d' % k, True, POSE_FEATS[k]) for k in range(5)]
    s += [('merge%d.' % (k + 1), 'merge%d' % k, False, 'pa%d' % k) for k in range(4)]
    s += [('deep_merge.%d.' % k, 'deep%d' % k, False, 'merge3' if k == 0 else 'deep%d' % (k - 1)) for k in range(3)]
    return s


def bn_sites():
    s = []
    for p, t, _, _ in block_sites():
        s += [(p + 'bn1', t + '.x1'), (p + 'bn2', t + '.x2'), (p + 'bn3', t)]
    return s


def conv_names():
    return [p + c for p, _, _, _ in block_sites() for c in ('conv1', 'conv2', 'conv3')]


# ---------------------------------------------------------------------------------------------------------------------------------
# the heads as E terms (float64 value, bound of the fp32 evaluation)
def chain_sum(x, dim):
    """a chain of n adds starting from 0 (the first is exact): every partial sum is at most sum |x| + sum e"""
    n = x.v.shape[dim]
    ev = x.e.sum(dim)
    return E(x.v.sum(dim), ev + (n - 1) * U * (x.v.abs().sum(dim) + ev))


def window_mean(val, whole_map=False):
    """feat [B][C]: the mean of the top-left 4 x 4 window of val (view 0 of the top map, >= 0), 16 adds and a division in fp32."""
    w = val.double() if whole_map else val.double()[:, :, :4, :4]
    n = w.shape[2] * w.shape[3]
    s = w.sum(dim=(2, 3))
    return E(s, (n - 1) * U * s) / n


def dot_chain(a, w, start=None):
    """sum_j a[i][j] w[j][k] (+ start[k]) as a chain of fmas over j: a an E [I][J], w exact [J][K].  Returns a conv_exact.Term."""
    v = a.v.matmul(w)
    mag = a.v.abs().matmul(w.abs())
    ein = a.e.matmul(w.abs())
    if start is not None:
        v, mag = v + start, mag + start.abs()
    return CX.Term(v, ein + w.shape[0] * U * (mag + ein), mag)


def check_e(got, t):
    """(worst |got - value| / e, degenerate fraction) of an fp32 result against a Term whose e already holds every rounding"""
    return CX.ratio(got, t.v, t.e), CX.degenerate(t.mag, t.e)


def softmax_kl(lg, t, B, eps, gs):
    """One head from its OBSERVED logits lg [B][K] and targets t [B][K] (fp32 values as float64): probs, the per-sample loss terms l / B
    and dlogits as E terms (module docstring).  eps: the fp32 value of log_eps."""
    mx = lg.max(1, keepdim=True).values.expand_as(lg)
    ex = (E(lg) - E(mx)).exp()
    s = chain_sum(ex, 1)
    p = ex.div(E(s.v.unsqueeze(1).expand_as(lg), s.e.unsqueeze(1).expand_as(lg)))
    pe = p if eps == 0 else p + E(torch.full_like(lg, eps))
    pos = t > 0
    tl = E(torch.where(pos, t, torch.ones_like(t))).log()
    term = E(t) * (tl - pe.log())
    term = E(torch.where(pos, term.v, torch.zeros_like(t)), torch.where(pos, term.e, torch.zeros_like(t)))
    l = chain_sum(term, 1) / B
    g = -(E(t).div(E(torch.full_like(lg, float(B))) * pe))
    gp = chain_sum(g * p, 1)
    dz = p * (g - E(gp.v.unsqueeze(1).expand_as(lg), gp.e.unsqueeze(1).expand_as(lg)))
    if gs != 1.0:
        dz = dz * E(torch.full_like(lg, gs))
    return dict(p=p, l=l, dz=dz)


def loss_term(ls):
    """the loss: the 2 B values l / B of both heads added atomically in any order (a chain of at most 2 B adds)"""
    v = torch.cat([l.v for l in ls])
    e = torch.cat([l.e for l in ls])
    n = v.numel()
    es = e.sum()
    return CX.Term(v.sum().reshape(1), (es + (n - 1) * U * (v.abs().sum() + es)).reshape(1), v.abs().sum().reshape(1))


def fc_grad_terms(dz, feat):
    """dW[k][c] = sum_b dz[b][k] feat[b][c] (B fmas), db[k] = sum_b dz[b][k] (B adds)"""
    B = dz.v.shape[0]
    v = dz.v.t().matmul(feat.v)
    mag = dz.v.abs().t().matmul(feat.v.abs())
    ein = dz.v.abs().t().matmul(feat.e) + dz.e.t().matmul(feat.v.abs()) + dz.e.t().matmul(feat.e)
    dw = CX.Term(v, ein + B * U * (mag + ein), mag)
    ab = dz.v.abs().sum(0)
    eb = dz.e.sum(0)
    db = CX.Term(dz.v.sum(0), eb + (B - 1) * U * (ab + eb), ab)
    return dw, db


def dact_term(dz, w, shape, whole_map=False):
    """the head's gradient of the top map before its ReLU mask: df = chain of K fmas of dz[b][k] w[k][c], divided by 16 (exact) inside the
    top-left 4 x 4 window, 0 outside; shape = (B, C, H, W).  Returns (Term over the map, window mask)."""
    t = dot_chain(dz, w)
    Bn, C, H, W = shape
    win = torch.zeros(shape, dtype=torch.float64, device=t.v.device)
    n = 16.0
    if whole_map:
        win[:] = 1.0
        n = float(H * W)
    else:
        win[:, :, :4, :4] = 1.0
    ex = lambda a: (a / n).view(Bn, C, 1, 1) * win
    return CX.Term(ex(t.v), ex(t.e), ex(t.mag)), win


def mask_head_terms(val, w, b):
    """mask logits [B][16] (cell = 4 y + x): C / 64 fmas per lane, 6 shuffle adds, the bias"""
    Bn, C = val.shape[:2]
    x = val.double().permute(0, 2, 3, 1).reshape(-1, C)
    v = x.matmul(w) + b
    mag = x.abs().matmul(w.abs()) + b.abs()
    return CX.Term(v.view(Bn, 16), ((C // 64 + 6 + 1) * U * mag).view(Bn, 16), mag.view(Bn, 16))


def mask_head_bwd_terms(val, dl, w, gs):
    """out_conv.weight / bias gradients (chains over the B 16 rows, then the product with gs) and gs dl w per element"""
    Bn, C = val.shape[:2]
    rows = Bn * 16
    x = val.double().permute(0, 2, 3, 1).reshape(rows, C)
    d = dl.double().reshape(rows)
    mag = gs * d.abs().matmul(x.abs())
    dw = CX.Term(gs * d.matmul(x), (rows + 1) * U * mag, mag)
    db = CX.Term(gs * d.sum().reshape(1), rows * U * gs * d.abs().sum().reshape(1), gs * d.abs().sum().reshape(1))
    v = (gs * d).view(rows, 1) * w.view(1, C)
    da = CX.Term(v.view(Bn, 4, 4, C).permute(0, 3, 1, 2), (2 * U * v.abs()).view(Bn, 4, 4, C).permute(0, 3, 1, 2))
    return dw, db, da


# ---------------------------------------------------------------------------------------------------------------------------------
# bit-exact pool+add
def check_pooladd_fwd(val_hi, val_lo, pa_raw, dtype):
    """pa = round(maxpool2x2(hi) + lo), the max and the add in fp32"""
    return BX._mismatch(pa_raw, BX.rnd(F.max_pool2d(val_hi.float(), 2, 2) + val_lo.float(), dtype))


def check_pooladd_bwd(dpa, val_hi, val_lo, dhi, dlo, dtype):
    """d lo = d pa [lo > 0]; d hi = [hi > 0] route(d pa) to the first maximum.  Returns (differing elements, tied windows)."""
    r, ties = BX.check_pool_bwd(dpa, val_hi, dhi, dtype, masked=True)
    return r + BX._mismatch(dlo, dpa.float() * (val_lo > 0).float()), ties


def outside_window(dtop):
    """elements of the top map's gradient [B][C][H][W] outside the top-left 4 x 4 window that are not exactly zero (NaN counts): the head
    averages that window only (AvgPool2d(4) on a 5 x 5, 6 x 6 or 7 x 7 map has one window) and nothing else reads the top map"""
    out = dtop.clone()
    out[:, :, :4, :4] = 0
    return int((out != 0).sum())


KINDS = ('pool+add forward', 'pool+add backward', 'head logits', 'head loss', 'head fc gradients', 'head data gradient',
         'head gradient outside the window', 'mode 2 running stats', 'mode 2 logits')


def oracle_pair(chan, res, seed, dropout=False):
    """The oracle pose net and agent of a leg (CPU, tests/test_gpu_agent._pair's deterministic fill), the pose net CALIBRATED: its running
    BatchNorm estimates are the batch statistics of two seeded images (one train-mode pass with momentum 1), as a trained net's are of
    its data.  With the fill's arbitrary estimates (mean U(+-0.1), variance U(0.5, 1.5)) the eval-mode features drift so far that bn1 of
    the agent's five input blocks sees |mean| / sigma of 140 - 500 per channel and every bound of those BatchNorms is degenerate;
    calibrated, the largest is below 4 (LARGEST_MEAN_OVER_SIGMA)."""
    from oracle import model as om
    from tests import inputs
    from tests.test_gpu_net import t
    ref = om.create_hg(2, 1, 16, chan); om.deterministic_fill_(ref, seed=seed)
    bns = [m for m in ref.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    mom = [m.momentum for m in bns]
    for m in bns:
        m.momentum = 1.0
    ref.train()
    with torch.no_grad():
        ref(t(inputs.images(seed + 200, 2, res)))
    for m, v in zip(bns, mom):
        m.momentum = v
    ref.eval()
    if dropout:
        ragent = om.create_asn(chan, chan, is_dropout=True)
    else:
        ragent = om.create_asn(chan, chan, 7, 7, is_aug=True)
    om.deterministic_fill_(ragent, seed=seed + 1)
    return ref, ragent


def oracle_conditioning(chan, B, res, seed, dropout=False):
    """largest |mean| / sigma over the inputs of the agent's 36 BatchNorms: fp32 oracle agent (train mode) on the oracle pose features"""
    from tests import inputs
    from tests.test_gpu_net import t
    ref, ragent = oracle_pair(chan, res, seed, dropout)
    ragent.train()
    worst = [0.0]

    def hook(m, inp):
        x = inp[0]
        worst[0] = max(worst[0], float((x.mean(dim=(0, 2, 3)).abs() / x.var(dim=(0, 2, 3), unbiased=False).sqrt()).max()))
    hs = [m.register_forward_pre_hook(hook) for m in ragent.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(hs) == 36
    with torch.no_grad():
        f, _, _ = ref.hg[0].agent_features(ref.stem(t(inputs.images(seed + 100, B, res))))
        ragent(f, is_aug=not dropout, is_dropout=dropout)
    return worst[0]


def _pair(chan, B, res, seed, dropout=False):
    """the engine's pose net and agent with the parameters of oracle_pair"""
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg, create_asn
    ref, ragent = oracle_pair(chan, res, seed, dropout)
    net = create_hg(2, 1, 16, chan, res=res, default_batch=B); net.load_state_dict(ref.state_dict())
    if dropout:
        agent = create_asn(chan, chan, is_dropout=True, res=res, default_batch=B)
    else:
        agent = create_asn(chan, chan, 7, 7, is_aug=True, res=res, default_batch=B)
    assert list(agent.state_dict().keys()) == list(ragent.state_dict().keys())
    agent.load_state_dict(ragent.state_dict())
    return net, agent


def _targets(seed, ls, lr, B):
    """reward-shaped targets from seeded draws, as tests/test_gpu_agent.test_agent_graph_matches_locally.  The nearly uniform softmax of
    an untrained agent never drives gen_groundtruth's clamp to 0, so every third sample gets one seeded bin set to exactly 0 and its row
    renormalised: the loss's t > 0 branch (0 log 0 = 0) and a zero gradient weight must be met."""
    from oracle import pylib as opl
    from tests import inputs
    from tests.test_gpu_net import t
    g = inputs.rng(seed)
    ps, pr = torch.softmax(ls.cpu(), 1), torch.softmax(lr.cpu(), 1)
    f = lambda: t(g.random(B).astype(np.float32))
    gs = opl.gen_groundtruth(ps, t(g.integers(0, 7, (B, 1))), f(), f())
    gr = opl.gen_groundtruth(pr, t(g.integers(0, 7, (B, 1))), f(), f())
    gs, gr = gs.float(), gr.float()
    for tg in (gs, gr):
        for b_ in range(0, B, 3):
            tg[b_, int(g.integers(0, 7))] = 0.0
            tg[b_] /= tg[b_].sum()
    return gs, gr


class Leg(object):
    """the shared part of a leg: the bookkeeping of all three files' kinds, the trunk checks"""
    def __init__(self, net, agent, sd0, dtype, B):
        self.net, self.agent, self.dtype, self.B = net, agent, dtype, B
        self.sd0 = sd0
        self.Pp, self.Pa = BX.Probe(net), BX.AsnProbe(agent)
        self.worst = dict((k, 0.0) for k in KINDS)
        self.bworst = dict((k, 0.0) for k in BX.KINDS)
        self.fails = []
        self.bnote = BX.make_note(self.bworst, self.fails)
        self.stored = {'.x2': 0, '': 0}
        self.ties = 0
        self.params = set()         # every parameter some check compared its gradient for

    def note(self, kind, what, r, bit=False):
        self.worst[kind] = max(self.worst[kind], r)
        if (r != 0) if bit else not (r <= 1.0):
            self.fails.append((kind, what, r))

    def note_t(self, kind, what, r_deg):
        r, deg = r_deg
        self.note(kind, what, r)
        if deg > CX.DEGENERATE:
            self.fails.append(('degenerate bound', '%s %s' % (kind, what), deg))

    def trunk(self, grads, before, expect=(), stored_expected=('.x2',)):
        """after a backward pass: the 12 blocks, the 36 BatchNorms, the four pool+add merges"""
        net, agent, dtype, Pp, Pa = self.net, self.agent, self.dtype, self.Pp, self.Pa
        sd = agent.state_dict()
        self.ck = ck = CX.Checker(self.sd0, grads, dtype, self.B)
        for p, out, from_pose, inp in block_sites():
            # merge<k> reads the plain pa<k> (no pending BatchNorm); deep<k> a block output
            ck.block(p, out, Pa, Pp if from_pose else Pa, inp, input_grad=not from_pose, in_masked=not inp.startswith('pa'))
        for pre, name in bn_sites():
            BX.check_bn_site(Pa, pre, name, sd, before, grads, dtype, self.bnote, self.stored)
            self.params |= {pre + '.weight', pre + '.bias'}
        for suf, cnt in self.stored.items():
            if cnt == 0 and suf in stored_expected:
                self.fails.append(('stored bn backward', 'no block stored its dz%s' % ('2' if suf else '3'), 0))
        for k in range(4):
            hi, lo, pa = ('in0' if k == 0 else 'merge%d' % (k - 1)), 'in%d' % (k + 1), 'pa%d' % k
            vh, vl = Pa.get(hi, 0), Pa.get(lo, 0)
            self.note('pool+add forward', pa, check_pooladd_fwd(vh, vl, Pa.get(pa, 2), dtype), bit=True)
            r, n = check_pooladd_bwd(Pa.get(pa, 1), vh, vl, Pa.get(hi, 1), Pa.get(lo, 1), dtype)
            self.note('pool+add backward', pa, r, bit=True)
            self.ties += n
        if self.ties == 0:
            self.fails.append(('pool+add backward', 'no 2 x 2 window had tied maxima: first-maximum routing was not tested', 0))
        self.fails += ck.fails
        for c, kind in ck.checked:
            if kind == 'weight gradient':
                self.params.add(c + '.weight')
            if kind == 'bias':
                self.params.add(c + '.bias')
        want = set((c, k) for c in conv_names() for k in ('conv forward', 'weight gradient', 'bias'))
        want |= set((p + c, 'conv data gradient') for p, _, _, _ in block_sites() for c in ('conv2', 'conv3'))
        want |= set((p + 'conv1', 'conv data gradient') for p, _, fp, _ in block_sites() if not fp)
        if want - ck.checked:
            self.fails.append(('coverage', 'checks missing: %s' % sorted(want - ck.checked)[:20], 0))
        for kind in expect:
            if not ck.met[kind]:
                self.fails.append(('coverage', 'no layer of this leg has a shape of the %s weight-gradient split' % kind, 0))
        # the features are detached: nothing reaches the pose net
        if float(net.flat_grads.abs().max()) != 0.0:
            self.fails.append(('pose net gradients', 'the agent step wrote into the pose net\'s flat_grads', float(net.flat_grads.abs().max())))

    def coverage(self, grads):
        missing = sorted(set(grads) - self.params)
        if missing:
            self.fails.append(('coverage', 'parameters without a gradient check: %s' % missing[:20], 0))

    def eval_mode(self, forward):
        agent = self.agent
        agent.eval()
        forward()
        torch.cuda.synchronize()
        sd = agent.state_dict()
        for pre, name in bn_sites():
            BX.check_bn_eval_site(self.Pa, pre, name, sd, self.bnote)
        agent.train()

    def report(self, log, title):
        if os.environ.get('POSEADV_TEST_VERBOSE'):
            both = list(self.worst.items()) + [(k, v) for k, v in self.bworst.items() if k not in ('pool forward', 'merge forward', 'merge backward', 'pool backward')] + \
                list(self.ck.worst.items())
            log('asn_exact %s %s: worst error / bound (bit-exact kinds: differing elements): %s; stored dz2 / dz3 checked in %d / %d blocks; '
                '%d tied pool windows; %d layers with grouped splits'
                % ('fp16' if self.dtype == torch.float16 else 'bf16', title, ', '.join('%s %.3g' % kv for kv in both),
                   self.stored['.x2'], self.stored[''], self.ties, self.ck.met['group']))


def _guards(agent):
    sd = agent.state_dict()
    assert sorted(conv_names()) == sorted(k[:-len('.weight')] for k in sd if k.endswith('.weight') and sd[k].dim() == 4 and
                                          not k.startswith('out_conv')), 'conv_names must name every conv of the agent\'s trunk'
    assert sorted(p for p, _ in bn_sites()) == sorted(k[:-len('.running_mean')] for k in sd if k.endswith('.running_mean')), \
        'bn_sites must name every BatchNorm of the agent'


def run_leg(chan, B, res, seed, log=print, expect=(), history='fresh', stored_expected=('.x2',)):
    """The scale/rotation agent: half hourglass (eval) + agent (train) behind `history` (tests/exact_history.py: 'fresh' = the first agent
    step after the bind), one loss_and_backward per log_eps, then every check.  Returns ({kind: worst}, failures).  stored_expected: as
    bn_exact.run_leg -- () at chan 512, where no block of the agent has a data gradient that a tile kernel takes (512 gradient channels,
    a 3 x 3 layer with 256)."""
    from pose_adv_aug_amd._lib import act_dtype, grad_scale
    from tests import exact_history
    dtype = act_dtype()
    gsc = grad_scale()
    torch.cuda.set_device(0)
    net, agent = _pair(chan, B, res, seed)
    _guards(agent)

    def backward(out, k):
        gs_h, gr_h = _targets(seed + 10 + k, out[0], out[1], B)
        net.zero_grad(); agent.zero_grad()
        agent.loss_and_backward(gs_h, gr_h)
    fwd = exact_history.agent_history(net, agent, B, res, seed, history,
                                      lambda **im: net(im.get('x'), asn=agent, is_half_hg=True, is_aug=True, img4=im.get('img4')), backward)
    sd0 = {k: v.clone() for k, v in agent.state_dict().items()}          # immediately before the checked step
    ls, lr = fwd()
    gs_t, gr_t = _targets(seed + 2, ls, lr, B)
    assert bool((gs_t == 0).any()) or bool((gr_t == 0).any()), 'the targets of a leg must hold zeros (the t > 0 branch of the loss)'
    L = Leg(net, agent, sd0, dtype, B)
    Pa = L.Pa
    Ws, Wr = sd0['fc_scale.weight'].double(), sd0['fc_rotation.weight'].double()
    Wall = torch.cat([Ws, Wr], 0)
    for eps in (0.0, 1e-7):       # one forward + backward each; the last one (the joint loop's) leaves the trunk's tensors for the checks below
        before = {k: v.clone() for k, v in agent.state_dict().items() if k.endswith('running_mean') or k.endswith('running_var')}
        ls, lr = fwd()
        net.zero_grad(); agent.zero_grad()
        loss = agent.loss_and_backward(gs_t, gr_t, log_eps=eps).clone()
        torch.cuda.synchronize()
        grads = {n: g.clone() for n, g in agent.named_grads()}
        tag = 'log_eps %g' % eps
        top = Pa.get('deep2', 0)
        feat = window_mean(top)
        lg_s = dot_chain(feat, Ws.t(), sd0['fc_scale.bias'].double())
        lg_r = dot_chain(feat, Wr.t(), sd0['fc_rotation.bias'].double())
        L.note_t('head logits', 'scale', check_e(ls, lg_s))
        L.note_t('head logits', 'rotation', check_e(lr, lg_r))
        e32 = float(np.float32(eps))
        hs = softmax_kl(ls.double(), gs_t.cuda().double(), B, e32, gsc)
        hr = softmax_kl(lr.double(), gr_t.cuda().double(), B, e32, gsc)
        L.note_t('head loss', tag, check_e(loss.reshape(1), loss_term([hs['l'], hr['l']])))
        for h, nm in ((hs, 'fc_scale'), (hr, 'fc_rotation')):
            dw, db = fc_grad_terms(h['dz'], feat)
            L.note_t('head fc gradients', '%s.weight %s' % (nm, tag), check_e(grads[nm + '.weight'], dw))
            L.note_t('head fc gradients', '%s.bias %s' % (nm, tag), check_e(grads[nm + '.bias'], db))
            L.params |= {nm + '.weight', nm + '.bias'}
        dz = E(torch.cat([hs['dz'].v, hr['dz'].v], 1), torch.cat([hs['dz'].e, hr['dz'].e], 1))
        da, win = dact_term(dz, Wall, tuple(top.shape))
        dtop = Pa.get('deep2', 1)
        L.note_t('head data gradient', 'deep2 ' + tag, CX.check16(dtop, da, dtype, (top > 0).double() * win))
        # (check16's bound is 0 outside the window, which already admits nothing there; said once more on its own, per element)
        assert top.shape[2] == top.shape[3] == res // 64 and int(win[0, 0].sum()) == 16
        L.note('head gradient outside the window', 'deep2 ' + tag, outside_window(dtop), bit=True)
    L.trunk(grads, before, expect, stored_expected)
    L.coverage(grads)
    # update_running=False: the same batch statistics, the running estimates left alone
    sd1 = {k: v.clone() for k, v in agent.state_dict().items()}
    ls2, lr2 = agent.forward_features(net, update_running=False)
    torch.cuda.synchronize()
    sd2 = agent.state_dict()
    L.note('mode 2 running stats', 'all', sum(BX._mismatch(sd2[k], sd1[k]) for k in before), bit=True)
    L.note('mode 2 logits', 'both', BX._mismatch(ls2, ls) + BX._mismatch(lr2, lr), bit=True)
    L.eval_mode(lambda: agent.forward_features(net))
    L.report(log, '%s chan %d B %d res %d' % (history, chan, B, res))
    worst = dict(L.worst); worst.update(L.bworst); worst.update(L.ck.worst)
    return worst, L.fails


def run_mask_leg(chan, B, seed, log=print, expect=(), history='fresh', stored_expected=('.x2',)):
    """The occlusion agent (res 256) behind `history`: forward, backward_masks with a seeded gradient, then the trunk checks and the mask
    head's.  stored_expected: as run_leg."""
    from pose_adv_aug_amd._lib import act_dtype, grad_scale
    from tests import exact_history, inputs
    from tests.test_gpu_net import t
    dtype = act_dtype()
    gsc = grad_scale()
    torch.cuda.set_device(0)
    net, agent = _pair(chan, B, 256, seed, dropout=True)
    _guards(agent)
    seeded = lambda k: t(inputs.rng(seed + k).standard_normal((B, 1, 4, 4)).astype(np.float32)).cuda()

    def backward(out, k):
        net.zero_grad(); agent.zero_grad()
        agent.backward_masks(seeded(10 + k))
    fwd = exact_history.agent_history(net, agent, B, 256, seed, history,
                                      lambda **im: net(im.get('x'), asn=agent, is_half_hg=True, is_dropout=True, img4=im.get('img4')), backward)
    sd0 = {k: v.clone() for k, v in agent.state_dict().items()}          # immediately before the checked step
    before = {k: v for k, v in sd0.items() if k.endswith('running_mean') or k.endswith('running_var')}
    pm = fwd()
    gy = seeded(2)
    net.zero_grad(); agent.zero_grad()
    agent.backward_masks(gy)
    torch.cuda.synchronize()
    grads = {n: g.clone() for n, g in agent.named_grads()}
    L = Leg(net, agent, sd0, dtype, B)
    top = L.Pa.get('deep2', 0)
    w, b = sd0['out_conv.weight'].double().reshape(-1), sd0['out_conv.bias'].double()
    L.note_t('head logits', 'mask', check_e(pm.reshape(B, 16), mask_head_terms(top, w, b)))
    dw, db, da = mask_head_bwd_terms(top, gy, w, gsc)
    L.note_t('head fc gradients', 'out_conv.weight', check_e(grads['out_conv.weight'].reshape(-1), dw))
    L.note_t('head fc gradients', 'out_conv.bias', check_e(grads['out_conv.bias'], db))
    L.params |= {'out_conv.weight', 'out_conv.bias'}
    L.note_t('head data gradient', 'deep2', CX.check16(L.Pa.get('deep2', 1), da, dtype, (top > 0).double()))
    L.trunk(grads, before, expect, stored_expected)
    L.coverage(grads)
    L.eval_mode(lambda: agent.forward_masks(net))
    L.report(log, 'occlusion %s chan %d B %d' % (history, chan, B))
    worst = dict(L.worst); worst.update(L.bworst); worst.update(L.ck.worst)
    return worst, L.fails


if __name__ == '__main__':          # the fp16 legs: tests/test_gpu_asn_exact.py runs this with POSEADV_DTYPE=fp16
    from pose_adv_aug_amd._lib import lib as _l
    assert _l().pa_dtype() == 1, 'run with POSEADV_DTYPE=fp16'
    _rest, _stored = BX._child_stored(sys.argv[5:])
    _kw = BX._child_kw(_rest)
    if _stored is not None:
        _kw['stored_expected'] = _stored
    worst, fails = run_leg(*[int(a) for a in sys.argv[1:5]], log=lambda s: print(s, flush=True), **_kw)
    print('FAILURES %d %s' % (len(fails), fails[:20]))
    print('FP16 ASN EXACT ' + ('PASSED' if not fails else 'FAILED'), flush=True)
    sys.exit(1 if fails else 0)
