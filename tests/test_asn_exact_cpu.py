"""The new bounds of tests/asn_exact.py, tests/bn_exact.py (pool backward) and tests/conv_exact.py (heat gradient, loss) are not vacuous:
an fp32 emulation of each operation passes its check on synthetic tensors, and each planted defect is reported -- or, where a check
cannot see it, that is asserted instead of claimed:
  * pool backward: routed to the last maximum instead of the first, on a tensor with ReLU zeros: caught; the addend dropped: caught;
    the addend rounded to the storage type before the add: NOT visible -- the addend (d xin<i+1>) is a stored storage-type tensor
    already, rounding it again changes no bit; asserted as such;
  * the ReLU mask of a pool+add input taken from the raw tensor instead of the value: caught;
  * the head on a 6 x 6 top map: the whole-map mean instead of the 4 x 4 window: caught (logits); 1 / HW with HW = 36 spread over
    the whole map in the backward: caught (data gradient);
  * the KL gradient without its 1 / B: caught (fc gradients and data gradient); log_eps added outside the log: caught by the loss
    check on a peaked softmax, where eps / p is far above the fp32 resolution; a target of 0 contributing 0 log 0: caught (the loss
    is not finite);
  * the heat gradient without the in_conv addend, with gscale off by the factor 16, with the Gaussian patch shifted by one pixel:
    caught;
  * the loss with one workgroup's partial sum missing: caught.
The oracle's conditioning of the small legs is recomputed here (tests/asn_exact.LARGEST_MEAN_OVER_SIGMA)."""
import numpy as np
import pytest
import torch

from tests import asn_exact as A
from tests import bn_exact as BX
from tests import conv_exact as CX
from tests import inputs

torch.set_num_threads(min(16, torch.get_num_threads()))
BF = torch.bfloat16
f32 = lambda x: x.to(torch.float32)


def _fma(a, b, c):
    """fmaf on fp32 tensors: the exact product and sum (float64 holds it for these magnitudes), rounded once"""
    return (a.double() * b.double() + c.double()).float()


# ---------------------------------------------------------------------------------------------------------------------------------
def _route_scan(g, val, last=False):
    """the kernels' scan: m = v[0]; for k in 1..3: if v[k] > m (>= for the planted defect) take k"""
    v = BX._win(val.float())
    m, a = v[0].clone(), torch.zeros_like(v[0], dtype=torch.long)
    for k in (1, 2, 3):
        upd = (v[k] >= m) if last else (v[k] > m)
        m = torch.where(upd, v[k], m)
        a = torch.where(upd, torch.full_like(a, k), a)
    return BX._unwin(torch.stack([(a == k).float() * g.float() for k in range(4)], 0))


@pytest.mark.parametrize('B,C,H', [(2, 16, 8), (3, 8, 12)])
def test_pool_backward_routing(B, C, H):
    g = torch.Generator().manual_seed(H)
    val = torch.relu(torch.randn(B, C, H, H, generator=g)).to(BF).float()            # ReLU zeros: tied windows
    dp = torch.randn(B, C, H // 2, H // 2, generator=g).to(BF).float()
    add = torch.randn(B, C, H, H, generator=g).to(BF).float()
    good = BX.rnd(_route_scan(dp, val) + add, BF)
    r, ties = BX.check_pool_bwd(dp, val, good, BF, addend=add)
    assert r == 0 and ties > 0
    assert BX.check_pool_bwd(dp, val, BX.rnd(_route_scan(dp, val, last=True) + add, BF), BF, addend=add)[0] > 0      # last maximum
    assert BX.check_pool_bwd(dp, val, _route_scan(dp, val), BF, addend=add)[0] > 0                                  # addend dropped
    # the addend rounded before the add: it is a storage-type tensor already -- the defect changes nothing and the check cannot see it
    assert BX.check_pool_bwd(dp, val, BX.rnd(_route_scan(dp, val) + BX.rnd(add, BF), BF), BF, addend=add)[0] == 0
    # under a BatchNorm-backward epilogue: the ReLU-masked routed gradient
    masked = _route_scan(dp, val) * (val > 0).float()
    assert BX.check_pool_bwd(dp, val, masked, BF, masked=True)[0] == 0
    # (under the mask a tie at 0 receives nothing either way: there only ties of positive values tell first from last)
    # a window whose four values are equal and positive: only the first pixel may receive the gradient
    flat = torch.ones(1, 1, 2, 2)
    one = torch.full((1, 1, 1, 1), 3.0)
    assert BX.check_pool_bwd(one, flat, _route_scan(one, flat), BF, masked=True) == (0, 1)
    assert BX.check_pool_bwd(one, flat, _route_scan(one, flat, last=True), BF, masked=True)[0] == 2


def test_pooladd_forward_and_masks():
    g = torch.Generator().manual_seed(5)
    B, C, H = 2, 16, 6
    raw_lo = torch.randn(B, C, H, H, generator=g).to(BF).float()
    lo = torch.relu(raw_lo + 0.4)                                                   # the value: relu(k0 raw + k1), k1 moves the sign
    hi = torch.relu(torch.randn(B, C, 2 * H, 2 * H, generator=g)).to(BF).float()
    pa = BX.rnd(torch.nn.functional.max_pool2d(hi, 2, 2) + lo, BF)
    assert A.check_pooladd_fwd(hi, lo, pa, BF) == 0
    bad = pa.clone(); bad[1, 3, 2, 2] += 2.0 ** -6
    assert A.check_pooladd_fwd(hi, lo, bad, BF) == 1
    dpa = torch.randn(B, C, H, H, generator=g).to(BF).float()
    dhi = _route_scan(dpa, hi) * (hi > 0).float()
    r, ties = A.check_pooladd_bwd(dpa, hi, lo, dhi, dpa * (lo > 0).float(), BF)
    assert r == 0 and ties > 0
    assert A.check_pooladd_bwd(dpa, hi, lo, dhi, dpa * (raw_lo > 0).float(), BF)[0] > 0      # mask from the raw tensor


# ---------------------------------------------------------------------------------------------------------------------------------
def emulate_head(top, Ws, bs, Wr, br, ts, tr, eps, whole_map=False, hw36=False, no_inv_b=False, eps_outside=False, zero_log_zero=False):
    """asn_head_fwd_kernel / asn_head_bwd_kernel / asn_fc_wgrad_kernel in fp32 (torch's fp32 exp / log stand in for expf / logf)"""
    B, C, H, W = top.shape
    win = top if whole_map else top[:, :, :4, :4]
    acc = torch.zeros(B, C)
    for y in range(win.shape[2]):
        for x in range(win.shape[3]):
            acc = acc + f32(win[:, :, y, x])
    feat = acc / np.float32(win.shape[2] * win.shape[3])
    out = {}
    dzs = []
    loss = torch.zeros(())
    for name, Wt, b, t in (('s', Ws, bs, ts), ('r', Wr, br, tr)):
        lg = f32(b).unsqueeze(0).repeat(B, 1)
        for c in range(C):
            lg = _fma(feat[:, c:c + 1], f32(Wt[:, c]).unsqueeze(0), lg)
        out['logits_' + name] = lg
        K = lg.shape[1]
        ex = torch.exp(lg - lg.max(1, keepdim=True).values)
        s = torch.zeros(B)
        for k in range(K):
            s = s + ex[:, k]
        p = ex / s.unsqueeze(1)
        e32 = np.float32(eps)
        l, gp = torch.zeros(B), torch.zeros(B)
        Bf = np.float32(1.0 if no_inv_b else B)
        for k in range(K):
            lp = (torch.log(p[:, k]) + e32) if eps_outside else torch.log(p[:, k] + e32)
            term = t[:, k] * (torch.log(t[:, k]) - lp)
            l = l + (term if zero_log_zero else torch.where(t[:, k] > 0, term, torch.zeros(B)))
            gp = gp + (-t[:, k] / (Bf * (p[:, k] + e32))) * p[:, k]
        gk = -t / (Bf * (p + e32))
        dzs.append(p * (gk - gp.unsqueeze(1)))
        for b_ in range(B):
            loss = loss + l[b_] / np.float32(B)
    out['loss'] = loss
    dz = torch.cat(dzs, 1)
    Wall = torch.cat([f32(Ws), f32(Wr)], 0)
    dW = torch.zeros(dz.shape[1], C)
    db = torch.zeros(dz.shape[1])
    for b_ in range(B):
        dW = _fma(dz[b_].unsqueeze(1), feat[b_].unsqueeze(0), dW)
        db = db + dz[b_]
    out['dW'], out['db'] = dW, db
    df = torch.zeros(B, C)
    for k in range(dz.shape[1]):
        df = _fma(dz[:, k:k + 1], Wall[k].unsqueeze(0), df)
    d = torch.zeros(B, C, H, W)
    if hw36:
        d[:] = (df / np.float32(H * W)).to(BF).float().view(B, C, 1, 1)
    else:
        d[:, :, :4, :4] = (df / np.float32(16)).to(BF).float().view(B, C, 1, 1)
    out['dact'] = d * (top > 0).float()
    return out


def _head_checks(top, Ws, bs, Wr, br, ts, tr, eps, got):
    B = top.shape[0]
    feat = A.window_mean(top)
    r = {}
    r['logits'] = max(A.check_e(got['logits_s'], A.dot_chain(feat, Ws.double().t(), bs.double()))[0],
                      A.check_e(got['logits_r'], A.dot_chain(feat, Wr.double().t(), br.double()))[0])
    e32 = float(np.float32(eps))
    hs = A.softmax_kl(got['logits_s'].double(), ts.double(), B, e32, 1.0)
    hr = A.softmax_kl(got['logits_r'].double(), tr.double(), B, e32, 1.0)
    r['loss'] = A.check_e(got['loss'].reshape(1), A.loss_term([hs['l'], hr['l']]))[0]
    dz = BX.E(torch.cat([hs['dz'].v, hr['dz'].v], 1), torch.cat([hs['dz'].e, hr['dz'].e], 1))
    dw, db = A.fc_grad_terms(dz, feat)
    r['fc'] = max(A.check_e(got['dW'], dw)[0], A.check_e(got['db'], db)[0])
    da, win = A.dact_term(dz, torch.cat([Ws, Wr], 0).double(), tuple(top.shape))
    r['dact'], r['degenerate'] = CX.check16(got['dact'], da, BF, (top > 0).double() * win)
    return r


def _head_data(B, C, H, seed, spread=1.0):
    g = torch.Generator().manual_seed(seed)
    top = torch.relu(torch.randn(B, C, H, H, generator=g) + 0.3)                    # fp32 values (view 0), some zeros
    Ws = (torch.rand(7, C, generator=g) * 2 - 1) * spread / C ** 0.5
    Wr = (torch.rand(7, C, generator=g) * 2 - 1) * spread / C ** 0.5
    bs, br = torch.randn(7, generator=g) * 0.05 * spread, torch.randn(7, generator=g) * 0.05 * spread
    ts, tr = torch.softmax(torch.randn(B, 7, generator=g), 1), torch.softmax(torch.randn(B, 7, generator=g), 1)
    for t in (ts, tr):
        t[0, 2] = 0.0                                                               # a zero target
        t[0] /= t[0].sum()
    return top, Ws, bs, Wr, br, ts, tr


@pytest.mark.parametrize('eps', [1e-7, 0.0])
@pytest.mark.parametrize('B,C,H', [(3, 128, 6), (4, 128, 4)])
def test_head_bounds_hold_and_catch_the_defects(B, C, H, eps):
    d = _head_data(B, C, H, seed=B * 10 + H)
    ok = _head_checks(*d, eps, emulate_head(*d, eps))
    assert max(ok['logits'], ok['loss'], ok['fc'], ok['dact']) <= 1.0 and ok['degenerate'] <= CX.DEGENERATE, ok
    if H == 6:
        assert _head_checks(*d, eps, emulate_head(*d, eps, whole_map=True))['logits'] > 1.0
        assert _head_checks(*d, eps, emulate_head(*d, eps, hw36=True))['dact'] > 1.0
    else:       # on the 4 x 4 map of a 256 input both forms are the same computation
        assert _head_checks(*d, eps, emulate_head(*d, eps, whole_map=True, hw36=True)) == ok
    bad = _head_checks(*d, eps, emulate_head(*d, eps, no_inv_b=True))
    assert bad['fc'] > 1.0 and bad['dact'] > 1.0
    assert _head_checks(*d, eps, emulate_head(*d, eps, zero_log_zero=True))['loss'] > 1.0           # nan: not finite


def test_eps_outside_the_log_is_caught_on_a_peaked_softmax():
    """log(p) + eps instead of log(p + eps): the difference t eps (1 / p - 1) needs a small p to exceed the fp32 resolution of the loss"""
    d = _head_data(4, 128, 4, seed=9, spread=40.0)
    eps = 1e-7
    ok = _head_checks(*d, eps, emulate_head(*d, eps))
    assert max(ok['logits'], ok['loss'], ok['fc'], ok['dact']) <= 1.0, ok
    assert float(torch.softmax(emulate_head(*d, eps)['logits_s'], 1).min()) < 1e-4
    assert _head_checks(*d, eps, emulate_head(*d, eps, eps_outside=True))['loss'] > 1.0


def test_mask_head_bounds():
    g = torch.Generator().manual_seed(4)
    B, C = 2, 128
    top = torch.relu(torch.randn(B, C, 4, 4, generator=g))
    w = (torch.rand(C, generator=g) * 2 - 1) / C ** 0.5
    b = torch.tensor([0.03])
    x = top.permute(0, 2, 3, 1).reshape(-1, C)
    lanes = torch.zeros(B * 16, 64)
    for j in range(C // 64):
        lanes = _fma(x[:, j * 64:(j + 1) * 64], w[j * 64:(j + 1) * 64].unsqueeze(0), lanes)
    o = 32
    while o:                                                                        # the xor butterfly
        lanes = lanes + lanes[:, torch.arange(64) ^ o]
        o >>= 1
    logits = (lanes[:, 0] + b).view(B, 16)
    t = A.mask_head_terms(top, w.double(), b.double())
    assert A.check_e(logits, t)[0] <= 1.0
    assert A.check_e(logits - b, t)[0] > 1.0                                        # the bias left out
    dl = torch.randn(B * 16, generator=g)
    dw = torch.zeros(C)
    s = torch.zeros(())
    for r in range(B * 16):
        dw = _fma(dl[r].expand(C), x[r], dw)
        s = s + dl[r]
    da = (dl.view(-1, 1) * w.view(1, -1)).to(BF).float().view(B, 4, 4, C).permute(0, 3, 1, 2) * (top > 0).float()
    tw, tb, ta = A.mask_head_bwd_terms(top, dl.view(B, 1, 4, 4), w.double(), 1.0)
    assert A.check_e(dw, tw)[0] <= 1.0 and A.check_e(s.reshape(1), tb)[0] <= 1.0
    assert CX.check16(da, ta, BF, (top > 0).double())[0] <= 1.0
    dw_bad = dw - _fma(dl[5].expand(C), x[5], torch.zeros(C))                       # one row missing
    assert A.check_e(dw_bad, tw)[0] > 1.0
    assert CX.check16(da * 0 + (dl.view(-1, 1) * w.view(1, -1)).to(BF).float().view(B, 4, 4, C).permute(0, 3, 1, 2), ta, BF,
                      (top > 0).double())[0] > 1.0                                  # the ReLU mask left out


# ---------------------------------------------------------------------------------------------------------------------------------
def _heat_data(B, H, seed):
    g = torch.Generator().manual_seed(seed)
    pts = inputs.heat_pts(seed, B, res=H)
    target = torch.from_numpy(inputs.heatmaps_from_pts(pts, res=H))
    heat = (target + 0.15 * torch.randn(B, 16, H, H, generator=g)).float()
    add = (torch.randn(B, 16, H, H, generator=g) * 1e-5).to(BF).float()
    return pts, target, heat, add


def _emulate_heat_grad(heat, target, gscale, add):
    g = (np.float32(2.0) * (heat - target)) * np.float32(gscale)
    if add is not None:
        g = g + add
    return g.to(BF).float()


@pytest.mark.parametrize('B,H', [(2, 32), (3, 96)])
def test_heat_gradient_bound_holds_and_catches_the_defects(B, H):
    pts, target, heat, add = _heat_data(B, H, seed=H)
    gs = 1.0 / (B * 16.0 * H * H)
    ck = lambda got, a=add: CX.heat_grad_check(got, heat, target, gs, a, BF)
    r, deg = ck(_emulate_heat_grad(heat, target, gs, add))
    assert r <= 1.0 and deg <= CX.DEGENERATE
    # the contracted form: fma(2 (heat - target), gscale, add), one rounding fewer
    fused = _fma(np.float32(2.0) * (heat - target), torch.full_like(heat, np.float32(gs)), add).to(BF).float()
    assert ck(fused)[0] <= 1.0
    assert ck(_emulate_heat_grad(heat, target, gs, None))[0] > 1.0                                  # the addend dropped
    assert ck(_emulate_heat_grad(heat, target, gs * 16, add))[0] > 1.0                              # gscale off by 16
    assert ck(_emulate_heat_grad(heat, target, gs, None), None)[0] <= 1.0                           # the last stack: no addend
    shifted = torch.roll(target, 1, dims=3)
    assert float((shifted != target).sum()) > 0
    assert ck(_emulate_heat_grad(heat, shifted, gs, add))[0] > 1.0                                  # the patch one pixel to the right


@pytest.mark.parametrize('B,H', [(2, 32), (3, 96)])
def test_loss_bound_holds_and_catches_a_missing_workgroup(B, H):
    pts, target, heat, _ = _heat_data(B, H, seed=H + 1)
    M = B * H * H
    groups = -(-M // 16)
    blocks = min(768, -(-groups // 4))
    d2 = ((heat - target) * (heat - target)).permute(0, 2, 3, 1).reshape(M, 16)      # fp32, NHWC16 rows
    inv = np.float32(1.0) / np.float32(M * 16.0)
    part = torch.zeros(blocks)
    for g0 in range(groups):                                                         # group g0 belongs to workgroup (g0 / 4) % blocks
        blk = (g0 // 4) % blocks
        part[blk] = part[blk] + d2[g0 * 16:(g0 + 1) * 16].sum()
    part = part * inv
    total = torch.zeros(())
    for v in part:
        total = total + v
    _, r = CX.loss_check(total, heat, target)
    assert r <= 1.0
    _, r = CX.loss_check(total - part[blocks // 2], heat, target)
    assert r > 1.0
    assert CX.loss_depth(24 * 64 * 64) == 4 * 2 + 9 + 767 and CX.loss_depth(2 * 32 * 32) == 4 + 9 + 31


def test_oracle_conditioning():
    """the oracle alone stays far inside the degenerate threshold (|mean| / sigma about 10) on the small legs; the figures of all legs
    are recorded in tests/asn_exact.py"""
    for key in ((128, 4, 256, 53, False), (128, 2, 256, 55, True), (512, 2, 256, 60, False), (512, 2, 256, 61, True)):
        v = A.oracle_conditioning(*key)
        assert abs(v - A.LARGEST_MEAN_OVER_SIGMA[key]) < 0.05 and v < 5.0, (key, v)
    assert max(A.LARGEST_MEAN_OVER_SIGMA.values()) < 5.0
