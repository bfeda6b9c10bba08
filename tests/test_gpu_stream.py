"""The engine's random stream and the three samplers that draw from it, draw for draw, against the host restatement of the stream
(tests/stream_exact.py): with every uniform the device will draw known on the host, every sampler output is an exact expectation.

  1  pa_sample_aug with its own stream: gains, flip, the forced-zero rotation and the mirrored centre bit for bit.
  2  its two normals, bracketed: pa_sample_aug_given with z_ref - delta and z_ref + delta must enclose the own-stream scale and
     rotation (both laws are monotone in z), and the two ends may differ by one fp32 ulp in s / 4 delta 30 in r at the most.
  3  pa_sample_categorical: every pick == categorical_pick(the device's probs, the restated uniform); probs against the float64 softmax.
  4  a class of probability zero is never picked (the fp32 probabilities sum to less than 1: a raw u can fall in the gap), and the
     mirror case (sum above 1, u between the normalised and the raw edge).
  5  both sides of every interior cdf edge, with uniforms found within 1e-7 of it.
  6  pa_sample_dropout_masks with its own stream == the same call with uniforms = the restated stream.
  7  refusals: slot 256 (it would be slot 0 of the next sample), K = 0, K = 65, B = 0.
  8  sample_bins and a train_hg_step-style sequence: bins and jitter recomputed from the restatement with the slot map.

delta = 32 * 2^-53 * max(1, R), R = sqrt(-2 ln u1).  The device evaluates R cos(fl(2 pi) u2) in float64: log, sqrt, the product and cos
within a few ulp each (the published HIP math tables list double log and sqrt at 1 ulp and cos at 2; no document of the ROCm
installation this was written against states a figure, so there is no documented sum to compare with a quarter of delta), and the
rounded argument fl(fl(2 pi) u2) moves the cosine by at most ~3.5 * 2^-53: together about 8 * 2^-53 * R, a quarter of delta, and twelve
orders of magnitude below the effect of a wrong draw.

probs bound (as tests/asn_exact.py::softmax_kl derives its softmax terms, u = 2^-24): x = l - max is one fp32 subtraction (u |x|), expf
is charged 2 ulp = 4 u of its result on top of exp(x) expm1(u |x|), the sum is a chain of K adds from 0 ((K - 1) u of the running
magnitude), the division is correctly rounded (u); one subnormal step 2^-149 is added for results below the normal range."""
import numpy as np
import pytest
import torch

from tests import stream_exact as S

pytestmark = pytest.mark.gpu

BS = (1, 63, 64, 65, 257, 4096)             # 64 threads per block, one row per thread
KEYS = ((0, 0), (1, 1), (2 ** 32 + 5, 1), (2 ** 63 + 11, 2 ** 32 + 5), (7, 2 ** 63 + 11), (0, 2 ** 32 + 5))      # (seed, step)
U32 = 2.0 ** -24
D_ULP = 2.0 ** -53


def _api():
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    return lib(), check, ptr, stream


def _last_error():
    msg = _api()[0].pa_last_error()
    return msg.decode() if msg else ''


def _meta(B, seed=3):
    g = np.random.default_rng(seed)
    m = np.stack([640 + g.uniform(-300, 300, B), 360 + g.uniform(-100, 100, B), 1.5 + 2.5 * g.random(B), np.full(B, 1280.0)], 1)
    m[::5, 3] = 1279.0
    return m.astype(np.float32)


def _aug(meta, mode, seed, step, si=None, ri=None, draws=None):
    L, check, ptr, stream = _api()
    B = meta.shape[0]
    dm = torch.from_numpy(meta).cuda()
    params = torch.full((B, 8), float('nan'), dtype=torch.float64, device='cuda')
    dsi = torch.from_numpy(si).cuda() if si is not None else None
    dri = torch.from_numpy(ri).cuda() if ri is not None else None
    if draws is None:
        check(L.pa_sample_aug(ptr(dm), ptr(dsi), ptr(dri), mode, seed, step, B, ptr(params), stream()), 'pa_sample_aug')
    else:
        dd = torch.from_numpy(np.ascontiguousarray(draws)).cuda()
        check(L.pa_sample_aug_given(ptr(dm), ptr(dsi), ptr(dri), mode, ptr(dd), B, ptr(params), stream()), 'pa_sample_aug_given')
    return params.cpu().numpy()


def _bins(B, shift=0):
    b = np.arange(B)
    return ((b + shift) % 7).astype(np.int32), ((3 * b + 1 + shift) % 7).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_aug_uniforms_bit_for_bit():
    for seed, step in KEYS:
        for B in BS:
            meta = _meta(B)
            p = _aug(meta, 0, seed, step)
            d, _, _ = S.aug_draws(seed, step, B)
            for c in range(3):
                assert np.array_equal(p[:, 5 + c], 0.6 + (1.4 - 0.6) * d[:, 4 + c]), (seed, step, B, c)
            flip = d[:, 3] <= 0.5
            assert np.array_equal(p[:, 4], flip.astype(np.float64))
            assert np.array_equal(p[:, 3] == 0.0, d[:, 2] <= 0.6)
            cx = np.where(flip, meta[:, 3].astype(np.float64) - meta[:, 0].astype(np.float64), meta[:, 0].astype(np.float64))
            assert np.array_equal(p[:, 0], cx.astype(np.float32).astype(np.float64))
            assert np.array_equal(p[:, 1], meta[:, 1].astype(np.float64))
    B = 257
    meta = _meta(B)
    si, ri = _bins(B)
    for mode in (2, 3):
        p = _aug(meta, mode, 7, 3, si, ri)
        assert np.all(p[:, 4] == 0.0) and np.all(p[:, 5:8] == 1.0) and np.array_equal(p[:, 0], meta[:, 0].astype(np.float64))
        if mode == 2:
            assert np.all(p[:, 3] == 0.0)
        else:
            assert np.array_equal(p[:, 2], meta[:, 2].astype(np.float64))


def _bracket(meta, mode, seed, step, si, ri):
    """(own, lo, hi, delta_s, delta_r): the own-stream parameters and the given-draws parameters at z_ref -+ delta"""
    B = meta.shape[0]
    d, (zs, Rs), (zr, Rr) = S.aug_draws(seed, step, B)
    ds = (32 * D_ULP * np.maximum(1, Rs)).astype(np.longdouble)
    dr = (32 * D_ULP * np.maximum(1, Rr)).astype(np.longdouble)
    lo, hi = d.copy(), d.copy()
    lo[:, 0], hi[:, 0] = (zs - ds).astype(np.float64), (zs + ds).astype(np.float64)
    lo[:, 1], hi[:, 1] = (zr - dr).astype(np.float64), (zr + dr).astype(np.float64)
    own = _aug(meta, mode, seed, step, si, ri)
    return own, _aug(meta, mode, 0, 0, si, ri, lo), _aug(meta, mode, 0, 0, si, ri, hi), ds.astype(np.float64), dr.astype(np.float64)


def _check_bracket(own, lo, hi, dr, tag):
    """own inside [lo, hi] in s and r, everything else identical; the ends at most one fp32 ulp / 4 delta 30 apart.  Returns the
    number of samples whose ends differ."""
    for c in (0, 1, 4, 5, 6, 7):
        assert np.array_equal(own[:, c], lo[:, c]) and np.array_equal(own[:, c], hi[:, c]), (tag, c)
    assert np.all(lo[:, 2] <= own[:, 2]) and np.all(own[:, 2] <= hi[:, 2]), (tag, 's', np.abs(own[:, 2] - lo[:, 2]).max())
    assert np.all(lo[:, 3] <= own[:, 3]) and np.all(own[:, 3] <= hi[:, 3]), (tag, 'r', np.abs(own[:, 3] - lo[:, 3]).max())
    ulp = np.spacing(hi[:, 2].astype(np.float32)).astype(np.float64)
    assert np.all(hi[:, 2] - lo[:, 2] <= ulp), (tag, 's ends')
    assert np.all(hi[:, 3] - lo[:, 3] <= 4 * dr * 30), (tag, 'r ends')
    return int((hi[:, 2] != lo[:, 2]).sum()), int((hi[:, 3] != lo[:, 3]).sum())


def test_aug_normals_bracketed():
    n = ns = nr = 0
    worst_delta = 0.0
    for mode in (0, 1, 2, 3):
        for (seed, step), B in zip(KEYS, BS):
            meta = _meta(B, seed=4 + mode)
            si, ri = _bins(B, shift=mode) if mode else (None, None)
            own, lo, hi, ds, dr = _bracket(meta, mode, seed, step, si, ri)
            a, b = _check_bracket(own, lo, hi, dr, (mode, seed, step, B))
            n += B; ns += a; nr += b
            worst_delta = max(worst_delta, float(ds.max()), float(dr.max()))
            if mode:                                   # the bins really took effect: the jittered exponent / angle sits in its bin
                if mode != 3:
                    f = np.log2(own[:, 2] / meta[:, 2].astype(np.float64))
                    mu = -0.6 + 0.2 * si
                    assert np.all(f >= mu - 0.05 + 1e-3 - 1e-6) and np.all(f <= mu + 0.05 + 1e-6)
                if mode != 2:
                    mu = -60 + 20.0 * ri
                    assert np.all(own[:, 3] >= mu - 5 + 1e-3 - 1e-9) and np.all(own[:, 3] <= mu + 5 + 1e-9)
    print('normals: %d samples; bracket ends differ in s for %d (%.2e), in r for %d (%.2e); largest delta %.3e'
          % (n, ns, ns / n, nr, nr / n, worst_delta))


# ---------------------------------------------------------------------------------------------------------------------------------
def _logit_rows(B, K, seed=0):
    """rows cycling through: Gaussian; all equal; one logit 30 above the rest; first logit -200; last logit -200; a -inf logit (K >= 2:
    a row of K = 1 whose only logit is -inf has no distribution)"""
    g = np.random.default_rng(100 + K + seed)
    l = g.standard_normal((B, K)).astype(np.float32)
    for b in range(B):
        kind = b % 6
        if kind == 1:
            l[b] = np.float32(g.standard_normal())
        elif kind == 2:
            l[b, (b // 6) % K] += np.float32(30.0)
        elif kind == 3:
            l[b, 0] = -200.0
        elif kind == 4:
            l[b, K - 1] = -200.0
        elif kind == 5 and K >= 2:
            l[b, (b // 6) % K] = -np.inf
    return l


def _categorical(logits, seed, step, slot, want_probs=True, want_idx=True):
    L, check, ptr, stream = _api()
    B, K = logits.shape
    dl = torch.from_numpy(np.ascontiguousarray(logits)).cuda()
    probs = torch.full((B, K), float('nan'), device='cuda') if want_probs else None
    idx = torch.full((B,), -1, dtype=torch.int32, device='cuda') if want_idx else None
    check(L.pa_sample_categorical(ptr(dl), B, K, seed, step, slot, ptr(probs), ptr(idx), stream()), 'pa_sample_categorical')
    return (probs.cpu().numpy() if want_probs else None), (idx.cpu().numpy() if want_idx else None)


def softmax_bound(logits):
    """(float64 softmax of the fp32 logits, bound of the kernel's fp32 evaluation): module docstring"""
    l = logits.astype(np.float64)
    x = l - l.max(1, keepdims=True)
    fin = np.isfinite(x)
    ex_in = np.where(fin, U32 * np.abs(np.where(fin, x, 0.0)), 0.0)
    v = np.exp(x)
    e = v * np.expm1(ex_in)
    e = e + 4 * U32 * (v + e)
    K = l.shape[1]
    sv, se = v.sum(1, keepdims=True), e.sum(1, keepdims=True)
    se = se + (K - 1) * U32 * (sv + se)
    p = v / sv
    pe = (e + p * se) / (sv - se)
    return p, pe + U32 * (p + pe) + 2.0 ** -149


@pytest.mark.parametrize('K', [1, 2, 7, 64])
def test_categorical_picks_exact(K):
    worst = 0.0
    for B in BS:
        logits = _logit_rows(B, K)
        ref, bound = softmax_bound(logits)
        b = np.arange(B, dtype=np.uint64)
        first = None
        for seed, step in KEYS:
            for slot in (0, 1, 255):
                probs, idx = _categorical(logits, seed, step, slot)
                if first is None:
                    first = probs
                    assert np.all(np.isfinite(probs)) and np.all(np.abs(probs - ref) <= bound), (K, B, (np.abs(probs - ref) / bound).max())
                    worst = max(worst, float((np.abs(probs - ref) / bound).max()))
                    assert np.all(probs[logits - logits.max(1, keepdims=True) < -150] == 0.0)
                else:
                    assert np.array_equal(probs, first)
                want = S.categorical_pick(probs, S.uniform(seed, step, b, slot))
                assert np.array_equal(idx, want.astype(np.int32)), (K, B, seed, step, slot, int((idx != want).sum()))
                assert np.all(probs[np.arange(B), idx] > 0)
        # probs = NULL and idx = NULL each accepted
        seed, step = KEYS[3]
        _, idx_only = _categorical(logits, seed, step, 1, want_probs=False)
        probs_only, _ = _categorical(logits, seed, step, 1, want_idx=False)
        assert np.array_equal(probs_only, first)
        assert np.array_equal(idx_only, S.categorical_pick(first, S.uniform(seed, step, b, 1)).astype(np.int32))
    print('K = %d: worst |probs - softmax| / bound %.3f' % (K, worst))


def test_categorical_never_picks_a_zero_class():
    g = np.random.default_rng(41)
    logits = (1.5 * g.standard_normal((1024, 7))).astype(np.float32)
    logits[:, 6] = -200.0
    probs, _ = _categorical(logits, 11, 0, 0)
    assert np.all(probs[:, 6] == 0.0)
    sums = np.cumsum(probs.astype(np.float64), 1)[:, -1]
    row = int(sums.argmin())
    gap = 1.0 - sums[row]
    hi_row = int(sums.argmax())
    cdf_hi = np.cumsum(probs[hi_row].astype(np.float64))
    k = int(np.argmax(cdf_hi[:5] * (1 - 1 / cdf_hi[-1])))             # the widest interval between a normalised and a raw interior edge
    found = S.find_keys(11, 0, [sums[row], cdf_hi[k] / cdf_hi[-1]], [1.0, cdf_hi[k]], 1 << 27)
    print('zero class: %d of 1024 sums below 1, widest gap %.3e (row %d), %d of 2^27 keys inside it; mirror: largest sum 1 + %.3e, '
          'edge %d, %d keys between the normalised and the raw edge'
          % (int((sums < 1).sum()), gap, row, found[0][0].size, sums[hi_row] - 1, k, found[1][0].size))
    assert gap >= 1e-7, gap
    steps, us = found[0]
    assert steps.size >= 1
    for step, u in list(zip(steps, us))[:8]:
        p1, i1 = _categorical(logits[row:row + 1], 11, int(step), 0)
        assert np.array_equal(p1[0], probs[row])
        assert sums[row] <= u < 1.0
        assert int(i1[0]) != 6 and int(i1[0]) == int(S.categorical_pick(p1, [u])[0]) == 5
    # the mirror: the sum exceeds 1, and u in [cdf[k] / total, cdf[k]) belongs to cell k + 1 by the normalised rule, to k by the raw one
    assert sums[hi_row] > 1.0
    steps, us = found[1]
    assert steps.size >= 1
    for step, u in list(zip(steps, us))[:8]:
        p1, i1 = _categorical(logits[hi_row:hi_row + 1], 11, int(step), 0)
        assert int(i1[0]) == int(S.categorical_pick(p1, [u])[0]) == k + 1, (step, u, int(i1[0]), k)


def test_categorical_cdf_edges():
    g = np.random.default_rng(43)
    logits = g.standard_normal((1, 7)).astype(np.float32)
    probs, _ = _categorical(logits, 5, 0, 1)
    cdf = np.cumsum(probs[0].astype(np.float64))
    edges = cdf[:6] / cdf[-1]
    near = S.nearest_keys(5, 1, edges, 1 << 26)
    dist = []
    for k, (e, (below, above)) in enumerate(zip(edges, near)):
        assert below[0] is not None and above[0] is not None
        dist += [e - below[1], above[1] - e]
        assert 0 < e - below[1] < 1e-7 and 0 <= above[1] - e < 1e-7, (k, e, below, above)
        picks = []
        for step, u in (below, above):
            p1, i1 = _categorical(logits, 5, step, 1)
            assert int(i1[0]) == int(S.categorical_pick(p1, [u])[0])
            picks.append(int(i1[0]))
        assert picks == [k, k + 1], (k, picks)
    print('edges: nearest uniforms %.2e .. %.2e from their edge' % (min(dist), max(dist)))


# ---------------------------------------------------------------------------------------------------------------------------------
def _masks(logits, k, seed, step, uniforms=None):
    L, check, ptr, stream = _api()
    B, cells = logits.shape
    dl = torch.from_numpy(np.ascontiguousarray(logits)).cuda()
    masks = torch.full((B, cells), float('nan'), device='cuda')
    idx = torch.full((B, max(k, 1)), -1, dtype=torch.int32, device='cuda')
    du = torch.from_numpy(np.ascontiguousarray(uniforms)).cuda() if uniforms is not None else None
    check(L.pa_sample_dropout_masks(ptr(dl), B, cells, k, seed, step, ptr(du), None, ptr(masks), ptr(idx), stream()), 'pa_sample_dropout_masks')
    return masks.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize('cells,k', [(16, 1), (16, 2), (16, 3), (64, 2), (2, 1), (16, 0)])
def test_masks_own_stream_exact(cells, k):
    from pose_adv_aug_amd.models.asn_stacked_hg import sample_mask
    for (seed, step), B in zip(KEYS, BS):
        g = np.random.default_rng(7 + cells + k)
        logits = (2 * g.standard_normal((B, cells))).astype(np.float32)
        b = np.arange(B)
        logits[b % 4 == 1, 0] = -200.0                       # cells of probability zero at either end, and at both
        logits[b % 4 == 2, -1] = -200.0
        if cells > 2:
            logits[b % 4 == 3, 0] = -200.0; logits[b % 4 == 3, -1] = -200.0
        u = S.uniform(seed, step, b.astype(np.uint64)[:, None], S.MASK_SLOT0 + np.arange(max(k, 1), dtype=np.uint64)[None, :])
        m_own, i_own = _masks(logits, k, seed, step)
        m_giv, i_giv = _masks(logits, k, 99, 99, uniforms=u)
        assert np.array_equal(m_own, m_giv) and np.array_equal(i_own, i_giv), (cells, k, B, seed, step)
        if k == 0:
            assert np.all(m_own == 1.0)
            continue
        assert np.all((m_own == 0).sum(1) == k) and np.all(logits[b[:, None], i_own] > -150)
        if cells in (16, 64):
            side = int(round(cells ** 0.5))
            m_py, i_py = sample_mask(torch.from_numpy(logits).view(B, 1, side, side).cuda(), dropout_num=k, seed=seed, step=step)
            assert np.array_equal(m_py.cpu().numpy().reshape(B, cells), m_own) and np.array_equal(i_py.cpu().numpy(), i_own)


def test_refusals():
    L, check, ptr, stream = _api()
    logits = torch.zeros(4, 65, device='cuda')
    probs = torch.zeros(4, 65, device='cuda'); idx = torch.full((4,), -1, dtype=torch.int32, device='cuda')
    for B, K, slot, text in ((4, 7, 256, 'slot <= 255'), (4, 0, 0, '1 <= K <= 64'), (4, 65, 0, '1 <= K <= 64'), (0, 7, 0, 'B >= 1')):
        rc = L.pa_sample_categorical(ptr(logits), B, K, 1, 2, slot, ptr(probs), ptr(idx), stream())
        assert rc != 0 and 'pa_sample_categorical' in _last_error() and text in _last_error(), (B, K, slot, rc, _last_error())
    torch.cuda.synchronize()
    assert np.all(idx.cpu().numpy() == -1) and float(probs.abs().sum()) == 0.0              # nothing was launched
    meta = torch.zeros(4, 4, device='cuda'); params = torch.zeros(4, 8, dtype=torch.float64, device='cuda')
    assert L.pa_sample_aug(ptr(meta), None, None, 0, 1, 2, 0, ptr(params), stream()) != 0 and 'pa_sample_aug: B >= 1' in _last_error()
    masks = torch.zeros(4, 16, device='cuda')
    assert L.pa_sample_dropout_masks(ptr(logits), 0, 16, 2, 1, 2, None, None, ptr(masks), None, stream()) != 0
    assert 'pa_sample_dropout_masks: B >= 1' in _last_error()
    assert L.pa_sample_categorical(ptr(logits), 4, 7, 1, 2, 255, ptr(probs), ptr(idx), stream()) == 0                 # the last slot is fine


def test_loops_draw_what_the_restatement_says():
    from pose_adv_aug_amd import joint_train_pose_s_r_agent as J
    from pose_adv_aug_amd.data import Augmenter, DeviceBatch
    B = 24
    b = np.arange(B, dtype=np.uint64)
    g = np.random.default_rng(17)
    ls = torch.from_numpy(g.standard_normal((B, 7)).astype(np.float32)).cuda()
    lr = torch.from_numpy(g.standard_normal((B, 7)).astype(np.float32)).cuda()
    for seed, step, slot in ((5, 9, 0), (2 ** 62 + 3, 2 ** 33, 255), (0, 0, 96)):
        probs, idx = J.sample_bins(ls, seed, step, slot)
        assert np.array_equal(idx.cpu().numpy(), S.categorical_pick(probs.cpu().numpy(), S.uniform(seed, step, b, slot)).astype(np.int32))
    # train_hg_step's sequence on a fresh augmenter with the default seed = 0: iteration 0 regular, iteration 1 the agent's bins and law
    aug = Augmenter(seed=4242)
    batch = DeviceBatch.synthetic(B, seed=2)
    aug.regular(batch)
    i = 1
    assert aug.step == i and J._bin_seed(0, aug) == aug.seed           # the coincidence the slot map has to survive
    ps, si = J.sample_bins(ls, J._bin_seed(0, aug), i, J.BIN_SLOTS_TRAIN_HG[0])
    pr, ri = J.sample_bins(lr, J._bin_seed(0, aug), i, J.BIN_SLOTS_TRAIN_HG[1])
    meta = batch.meta.cpu().numpy()
    aug.agent(batch, si, ri, mode=1)
    own = batch.params.cpu().numpy().copy()
    u_s, u_r = S.uniform(aug.seed, i, b, S.BIN_SLOTS_TRAIN_HG[0]), S.uniform(aug.seed, i, b, S.BIN_SLOTS_TRAIN_HG[1])
    want_s, want_r = S.categorical_pick(ps.cpu().numpy(), u_s).astype(np.int32), S.categorical_pick(pr.cpu().numpy(), u_r).astype(np.int32)
    assert np.array_equal(si.cpu().numpy(), want_s) and np.array_equal(ri.cpu().numpy(), want_r)
    d, (zs, Rs), (zr, Rr) = S.aug_draws(aug.seed, i, B)
    ds, dr = 32 * D_ULP * np.maximum(1, Rs), 32 * D_ULP * np.maximum(1, Rr)
    lo, hi = d.copy(), d.copy()
    lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1] = (zs - ds).astype(np.float64), (zs + ds).astype(np.float64), (zr - dr).astype(np.float64), (zr + dr).astype(np.float64)
    _check_bracket(own, _aug(meta, 1, 0, 0, want_s, want_r, lo), _aug(meta, 1, 0, 0, want_s, want_r, hi), dr.astype(np.float64), 'train_hg_step')
    # distinct keys: the uniforms that picked the bins are not the two uniforms of the scale jitter (slots 0 / 1 of the same seed and step)
    j1, j2 = S.uniform(aug.seed, i, b, S.AUG_SLOTS['scale_normal'][0]), S.uniform(aug.seed, i, b, S.AUG_SLOTS['scale_normal'][1])
    assert not np.any(u_s == j1) and not np.any(u_r == j2)
    keys = np.concatenate([S.key(i, b, s) for s in S.AUG_SLOT_LIST + S.BIN_SLOTS_TRAIN_HG])
    assert np.unique(keys).size == keys.size
