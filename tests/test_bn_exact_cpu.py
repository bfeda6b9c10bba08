"""The bounds of tests/bn_exact.py are not vacuous: on synthetic tensors with the legs' per-level shapes, an fp32 emulation of the engine's
BatchNorm arithmetic (bn_fin.h, the epilogues' sums) passes every check, and each of these defects is reported:
  * one partial row's worth of pixels (the smallest row any kernel writes at that level) dropped from a channel's forward sums (reported
    by the forward or the running-statistics check) or backward sums (the beta / gamma gradients), with the backward sum of dz * xhat in
    either of its two forms;
  * one element one ulp off in each bit-exact check (pool forward, merge forward, merge backward);
  * the biased variance in the running-variance update (where it differs from the unbiased one by more than the fp32 sums can:
    the small maps; at n = 98304 the two are 1e-5 apart, below what any fp32 statistics pass resolves);
  * the 2 x 2 sum of the merge backward in another order.
A bound that has degenerated (a nearly constant channel with a large mean) is reported as such."""
import numpy as np
import pytest
import torch

from tests import bn_exact as X

# (B, H, W, pixels of the smallest partial row at that level, channels of the layers there, capacity factor of the backward rows)
SHAPES = [
    (24, 128, 128, 64, 128, 1),  # configs[1] 128 x 128 (stem bn1, residual1): 64-pixel rows of the tile kernels
    (24, 64, 64, 64, 256, 1),    # configs[1] 64 x 64: 64-pixel rows of the 1 x 1 / 3 x 3 tile kernels (1536 rows)
    (24, 32, 32, 16, 256, 4),    # configs[1] 32 x 32 (up1.x3): the fused epilogue's 2 x 32-pixel tiles of the 64 x 64 map = 16 low-resolution pixels
    (24, 4, 4, 16, 256, 1),      # configs[1] neck
    (3, 96, 96, 64, 256, 1),     # configs[4] geometry, B 3
    (3, 6, 6, 36, 256, 1),       # its masked 6 x 6 neck: one tile per image
    (2, 2, 2, 4, 128, 1),        # tiny maps: the 2 x 2 neck, one image per row
    (8, 64, 64, 64, 512, 1),     # chan 512, B 8 at 64 x 64: the 64-pixel rows of the row-tile 1 x 1 forward (256 -> 512), beside the generic kernel's 128-pixel rows
    (2, 32, 32, 16, 512, 4),     # chan 512 tiny maps, up1.x3: 32 rows of 64 pixels in a four-fold capacity; a quarter row dropped
    (2, 2, 2, 4, 512, 1),        # chan 512 neck of the tiny maps
]
C = 6


def _f(x):
    return x.float()


def _emulate(raw, gamma, beta, dz, rm0, rv0, drop_fwd=None, drop_bwd=None, biased=False, shifted=0):
    """The engine's fp32 arithmetic on NCHW float64 tensors (bf16-exact values).  drop_*: (first pixel, pixels) of a partial row
    (NHWC pixel order) left out of the forward / backward sums.  shifted = P: the backward sum of dz * xhat in the epilogues' row form
    invstd * (sum dz x - mean sum dz) over rows of P pixels (pa_conv_epilogue_lds_bwd / _lds_up); 0: per term."""
    B, Cc, H, W = raw.shape
    n = B * H * W
    keep_f = torch.ones(n, dtype=torch.bool)
    keep_b = torch.ones(n, dtype=torch.bool)
    if drop_fwd:
        keep_f[drop_fwd[0]:drop_fwd[0] + drop_fwd[1]] = False
    if drop_bwd:
        keep_b[drop_bwd[0]:drop_bwd[0] + drop_bwd[1]] = False
    x = _f(raw).permute(0, 2, 3, 1).reshape(n, Cc)
    S1 = x[keep_f].sum(0)
    S2 = (x * x)[keep_f].sum(0)
    cnt = np.float32(n)
    mu = S1 / cnt
    var = torch.clamp(S2 / cnt - mu * mu, min=0)
    inv = torch.rsqrt(var + np.float32(X.EPS))
    scale = _f(gamma) * inv
    shift = _f(beta) - mu * scale
    bc = lambda v: v.view(1, -1, 1, 1)
    val = (bc(scale).double() * raw + bc(shift).double()).float().clamp_min(0)         # fmaf: one rounding
    m = np.float32(X.MOMENTUM)
    unb = var if biased else var * cnt / (cnt - np.float32(1))
    rm = (np.float32(1) - m) * _f(rm0) + m * mu
    rv = (np.float32(1) - m) * _f(rv0) + m * unb
    d = _f(dz).permute(0, 2, 3, 1).reshape(n, Cc)
    T1 = d[keep_b].sum(0)
    if shifted:
        dk, xk = d * keep_b[:, None], x
        r1 = dk.view(-1, shifted, Cc).sum(1)
        r2 = (dk * xk).view(-1, shifted, Cc).sum(1)
        T2 = (inv * (r2 - mu * r1)).sum(0)
    else:
        T2 = ((d * (x - mu)) * inv)[keep_b].sum(0)
    kA = scale
    b = -scale * inv * T2 / cnt
    kC = -scale * T1 / cnt - b * mu
    inner = (bc(b).double() * raw + bc(kC).double()).float()
    dx = (bc(kA).double() * dz + inner.double()).float()
    return dict(val=val, rm=rm, rv=rv, dgamma=T2, dbeta=T1, dx=dx)


def _data(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    mean = torch.linspace(-1.5, 2.0, C).view(1, -1, 1, 1)
    raw = (torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 0.7 + mean).bfloat16().double()
    val_mask = torch.rand(B, C, H, W, generator=g) > 0.4
    dz = (torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 1e-3 * val_mask).bfloat16().double()
    gamma = torch.rand(C, generator=g, dtype=torch.float64).float().double() + 0.1
    beta = (torch.randn(C, generator=g, dtype=torch.float64) * 0.3).float().double()
    rm0 = (torch.randn(C, generator=g) * 0.2).float()
    rv0 = (torch.rand(C, generator=g) + 0.5).float()
    return raw, dz, gamma, beta, rm0, rv0


def _checks(raw, dz, gamma, beta, rm0, rv0, e, chan, rows_scale):
    k = X.fwd_consts(raw, gamma, beta, rows_scale=rows_scale, chan=chan)
    assert k['degenerate'] < X.DEGENERATE
    T1, T2 = X.bwd_sums(raw, dz, k)
    return dict(fwd=X.check_forward(raw, e['val'], k), run=X.check_running(k, rm0, rv0, e['rm'], e['rv']),
                grads=X.check_param_grads(T1, T2, e['dgamma'], e['dbeta']), bwd=X.check_backward(raw, dz, e['dx'], k, T1, T2))


@pytest.mark.parametrize('shifted', [False, True])
@pytest.mark.parametrize('B,H,W,P,chan,rs', SHAPES)
def test_bn_bounds_hold_for_the_engine_arithmetic_and_catch_a_dropped_row(B, H, W, P, chan, rs, shifted):
    raw, dz, gamma, beta, rm0, rv0 = _data(B, H, W, seed=H * 7 + B)
    sh = P if shifted else 0
    ck = lambda e: _checks(raw, dz, gamma, beta, rm0, rv0, e, chan, rs)
    ok = ck(_emulate(raw, gamma, beta, dz, rm0, rv0, shifted=sh))
    assert all(r <= 1.0 for r in ok.values()), ok
    n = B * H * W
    row = (n // 2 // P) * P                                    # a row in the middle of the map
    bad_f = ck(_emulate(raw, gamma, beta, dz, rm0, rv0, drop_fwd=(row, P), shifted=sh))
    assert bad_f['fwd'] > 1.0 or bad_f['run'] > 1.0, bad_f
    bad_b = ck(_emulate(raw, gamma, beta, dz, rm0, rv0, drop_bwd=(row, P), shifted=sh))
    assert bad_b['grads'] > 1.0, bad_b


@pytest.mark.parametrize('B,H,W,P,chan,rs', [s for s in SHAPES if s[0] * s[1] * s[2] <= 400])
def test_running_var_bound_catches_the_biased_variance(B, H, W, P, chan, rs):
    raw, dz, gamma, beta, rm0, rv0 = _data(B, H, W, seed=5 + H)
    e = _emulate(raw, gamma, beta, dz, rm0, rv0, biased=True)
    assert _checks(raw, dz, gamma, beta, rm0, rv0, e, chan, rs)['run'] > 1.0


def test_a_degenerate_bound_is_reported():
    """A nearly constant channel with a large mean: the one-pass variance bound covers var + eps, and fwd_consts says so."""
    raw = torch.full((24, 2, 64, 64), 300.0, dtype=torch.float64)
    raw[:, :, ::7, ::5] = 301.0
    k = X.fwd_consts(raw, torch.ones(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64))
    assert k['degenerate'] > X.DEGENERATE


def test_eval_bound_holds_for_the_engine_arithmetic_and_catches_a_wrong_running_var():
    raw, _, gamma, beta, rm0, rv0 = _data(24, 16, 16, seed=3)
    s = _f(gamma) * torch.rsqrt(rv0 + np.float32(X.EPS))
    sh = _f(beta) - rm0 * s
    val = (s.view(1, -1, 1, 1).double() * raw + sh.view(1, -1, 1, 1).double()).float().clamp_min(0)
    assert X.check_eval(raw, val, _f(gamma), _f(beta), rm0, rv0) <= 1.0
    # the running variance one update off (biased instead of unbiased at n = 8: 14 %): far outside
    assert X.check_eval(raw, val, _f(gamma), _f(beta), rm0, rv0 * (1 + 0.1 / 7)) > 1.0


def _next_ulp(v, dtype):
    """v (a storage-type value held in fp32) moved up by one ulp of the storage type."""
    bits = torch.tensor([v], dtype=dtype).view(torch.int16)
    return float((bits + (1 if v >= 0 else -1)).view(dtype).float())


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('B,H,W', [(24, 64, 64), (3, 12, 12), (2, 4, 4)])
def test_bit_exact_checks_catch_one_ulp_and_another_summation_order(dtype, B, H, W):
    g = torch.Generator().manual_seed(B * H)
    vin = torch.relu(torch.randn(B, 4, H, W, generator=g))                    # BatchNorm+ReLU-applied fp32 values
    pooled = X.rnd(torch.nn.functional.max_pool2d(vin, 2, 2), dtype)
    assert X.check_pool(vin, pooled, dtype) == 0
    bad = pooled.clone()
    bad.view(-1)[bad.numel() // 3] = _next_ulp(float(bad.view(-1)[bad.numel() // 3]), dtype)
    assert X.check_pool(vin, bad, dtype) == 1
    vu = torch.relu(torch.randn(B, 4, H // 2, W // 2, generator=g))
    vs = torch.relu(torch.randn(B, 4, H, W, generator=g))
    merged = X.rnd(X.up2(vu) + vs, dtype)
    assert X.check_merge_fwd(vu, vs, merged, dtype) == 0
    bad = merged.clone()
    bad.view(-1)[7] = _next_ulp(float(bad.view(-1)[7]), dtype)
    assert X.check_merge_fwd(vu, vs, bad, dtype) == 1
    dm = X.rnd(torch.randn(B, 4, H, W, generator=g), dtype)
    # four values of a storage type add up exactly in fp32 unless their magnitudes are far apart: plant 2 x 2 blocks {A, 0.75 ulp_fp32(A);
    # -A, 0} in which (tl + tr) rounds, so that ((tl + tr) + bl) + br = ulp_fp32(A) and (tl + bl) + (tr + br) = 0.75 ulp_fp32(A)
    A = 1.0 if dtype == torch.bfloat16 else 2048.0
    for blk in range(0, vu.numel() // 4, 5):
        b_, c_, y_, x_ = np.unravel_index(blk, vu.shape)
        dm[b_, c_, 2 * y_:2 * y_ + 2, 2 * x_:2 * x_ + 2] = torch.tensor([[A, 0.75 * A * 2.0 ** -23], [-A, 0.0]])
    dup = X.rnd(X.sum2x2(dm), dtype) * (vu > 0).float()
    dsk = dm * (vs > 0).float()
    assert X.check_merge_bwd(dm, vu, vs, dup, dsk, dtype) == 0
    i = int((vu.view(-1) > 0).nonzero()[0])
    bad = dup.clone()
    bad.view(-1)[i] = _next_ulp(float(bad.view(-1)[i]), dtype)
    assert X.check_merge_bwd(dm, vu, vs, bad, dsk, dtype) == 1
    bad = dsk.clone()
    j = int((bad.view(-1) != 0).nonzero()[0])
    bad.view(-1)[j] = _next_ulp(float(bad.view(-1)[j]), dtype)
    assert X.check_merge_bwd(dm, vu, vs, dup, bad, dtype) == 1
    # another order of the 2 x 2 sum: (tl + bl) + (tr + br)
    d = dm.float()
    other = X.rnd((d[:, :, 0::2, 0::2] + d[:, :, 1::2, 0::2]) + (d[:, :, 0::2, 1::2] + d[:, :, 1::2, 1::2]), dtype) * (vu > 0).float()
    differs = int((other != dup).sum())
    assert differs > 0
    assert X.check_merge_bwd(dm, vu, vs, other, dsk, dtype) == differs


# ---- the occlusion branch: masked copies of the skip / neck tensors (check_mask_fwd, check_merge_bwd_masked, check_mask_bwd)
def _masks(B):
    """two zero cells per sample: the map corners, then an interior pair sharing an edge (tests/exact_history.FORCED_CELLS)"""
    M = torch.ones(B, 1, 4, 4)
    for b, cells in enumerate(((0, 15), (5, 6))[:B]):
        for c in cells:
            M[b, 0, c // 4, c % 4] = 0
    return M


def _emulate_masked(vs, vu, dm, M, dtype, shift=None, fwd_only=False, mask_up=False, no_relu=False):
    """Hourglass::encode / decode / bwd under Net::drop_mask on storage-type tensors: the masked copy of the skip tensor, the merge
    over it, and the two gradients.  shift: (dim, cells) the engine's mask is displaced by; fwd_only: the backward launch forgets the
    mask; mask_up: the mask lands on the upsampled tensor, not on the skip; no_relu: d skip without the ReLU factor of skip."""
    H = vs.shape[2]
    m = X.up4(M if shift is None else torch.roll(M, shift[1], dims=shift[0]), H)
    if mask_up:
        masked = X.rnd(vs, dtype)
        merged = X.rnd(X.up2(vu) * m + masked, dtype)
    else:
        masked = X.rnd(vs, dtype) * m
        merged = X.rnd(X.up2(vu) + masked, dtype)
    dup = X.rnd(X.sum2x2(dm), dtype) * (vu > 0).float()
    dmasked = dm.clone()
    dsk = dmasked * (torch.ones_like(m) if (fwd_only or mask_up) else m) * (torch.ones_like(vs) if no_relu else (vs > 0).float())
    return dict(masked=masked, merged=merged, dup=dup, dmasked=dmasked, dsk=dsk)


def _masked_checks(vs, vu, dm, M, dtype, e):
    return {'mask forward': X.check_mask_fwd(vs, M, e['masked'], dtype),
            'merge forward': X.check_merge_fwd(vu, e['masked'], e['merged'], dtype),
            'merge backward': X.check_merge_bwd_masked(dm, vu, e['dup'], e['dmasked'], dtype),
            'mask backward': X.check_mask_bwd(e['dmasked'], M, vs, e['dsk'])}


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('H', [64, 8, 4])
def test_masked_merge_checks_pass_the_emulation_and_report_each_defect(dtype, H):
    B, Cc = 2, 4
    g = torch.Generator().manual_seed(H)
    vs = torch.relu(torch.randn(B, Cc, H, H, generator=g))                   # BatchNorm+ReLU-applied fp32 values: zeros and positives everywhere
    vu = torch.relu(torch.randn(B, Cc, H // 2, H // 2, generator=g))
    dm = X.rnd(torch.randn(B, Cc, H, H, generator=g), dtype)
    M = _masks(B)
    ck = lambda **kw: _masked_checks(vs, vu, dm, M, dtype, _emulate_masked(vs, vu, dm, M, dtype, **kw))
    assert ck() == {'mask forward': 0, 'merge forward': 0, 'merge backward': 0, 'mask backward': 0}
    for dim in (2, 3):                                                        # the mask one cell off in y, in x
        bad = ck(shift=(dim, 1))
        assert bad['mask forward'] > 0 and bad['mask backward'] > 0, bad
    bad = ck(fwd_only=True)
    assert bad['mask backward'] > 0 and bad['mask forward'] == 0 and bad['merge forward'] == 0, bad
    bad = ck(mask_up=True)
    assert bad['mask forward'] > 0 and bad['merge forward'] > 0, bad
    bad = ck(no_relu=True)
    assert bad['mask backward'] > 0 and bad['mask forward'] == 0 and bad['merge backward'] == 0, bad
    # one element one ulp off, in each tensor the masked step adds (a kept cell: the last pixel of sample 1 is cell 15, kept there)
    e = _emulate_masked(vs, vu, dm, M, dtype)
    for key, kind in (('masked', 'mask forward'), ('dmasked', 'merge backward'), ('dsk', 'mask backward')):
        t = e[key].clone()
        j = int((t.view(-1) != 0).nonzero()[-1])
        t.view(-1)[j] = _next_ulp(float(t.view(-1)[j]), dtype)
        r = _masked_checks(vs, vu, dm, M, dtype, dict(e, **{key: t}))
        assert r[kind] == 1, (key, r)
    # the gradient of the masked copy is d merged itself: a ReLU mask there is reported
    r = _masked_checks(vs, vu, dm, M, dtype, dict(e, dmasked=e['dmasked'] * (vs > 0).float()))
    assert r['merge backward'] > 0


def test_sum_depth_at_chan_512_and_the_child_arguments():
    """D of the chan-512 legs is the formula's own (tests/bn_exact.py re-derives its parts for 64 channel groups): the 127-deep row tree
    dominates the streaming chain at every leg's size, and the finalize part is 8 + 20 up to 32768 pixels.  The optional 'stored='
    argument of the child-process entry points (which dz kinds a leg expects stored) parses to run_leg's stored_expected."""
    for n in (2 * 32 * 32, 4 * 64 * 64, 8 * 64 * 64):
        assert X.sum_depth(n, 512) == 127 + 8 + 20 and X.sum_depth(n, 512, 4) == 127 + 32 + 20
    assert -(-8 * 64 * 64 * 512 // (8 * 65536)) + 26 == 58 < 127          # the streaming chain of the largest chan-512 map
    assert X._child_stored(['warm', '370']) == (['warm', '370'], None)
    assert X._child_stored(['stored=x2']) == ([], ('.x2',))
    assert X._child_stored(['fresh', 'stored=x2,x3']) == (['fresh'], ('.x2', ''))
    assert X._child_stored(['fresh', 'stored=']) == (['fresh'], ())
    assert X._child_kw(X._child_stored(['fresh', '740', 'stored=x2'])[0]) == {'history': 'fresh', 'masks': 740}
