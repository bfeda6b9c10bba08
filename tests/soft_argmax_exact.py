"""The soft-arg-max over heat maps and its backward pass (csrc/soft_argmax.hip; pa_soft_argmax, pa_soft_argmax_bwd), element by element
against float64: the reference, the cases, the bound and the legs that tests/test_gpu_soft_argmax.py and tests/test_soft_argmax_cpu.py
assert on (tools/bench_soft_argmax.py prints the same legs' worst ratios into profiles/soft_argmax.txt).

u64 = 2^-53, u32 = 2^-24 (the unit roundoffs of double and float).  Per map, m its maximum, x_p = p % W + 1, y_p = p / W + 1:
  e_p = exp(beta (h_p - m)),  Z = sum e_p,  p_p = e_p / Z,  ex = sum x_p p_p,  ey = sum y_p p_p
  dmaps_p = beta p_p t_p,  t_p = (x_p - ex) gx + (y_p - ey) gy

Forward:   |coords - ref| <= u32 |ref| + d          (state's Z, ex, ey: the d term alone; m: equal)
Backward:  |dmaps - ref|  <= u32 |ref| + d + 2^-126 (whether the final conversion keeps subnormals is the compiler's business)

d is counted from the kernel's double operations, never fitted to what the device returned:
  * a term e_p carries a relative error eps_p = EXP_REL + 2 u64 + 2 u64 |a_p| : the device's exp (EXP_REL, below), the host exp of this
    reference (1 ulp = 2 u64), and the two roundings of the argument a_p = beta (h_p - m) (difference, product; kernel and reference
    round them alike, the term covers the distance of both to the exact value); where e_p is subnormal an absolute EXP_SUB 2^-1074.
  * every sum has terms >= 0 only, so its relative error is at most (additions on its longest path) u64.  The kernel's order: a thread
    adds its ceil(HW / T) terms in increasing p, 6 butterfly steps over the lanes of a wave, T / 64 - 1 additions over the waves:
    n = ceil(HW / T) + 6 + T / 64 - 1, with T = 1024 on the joint-minor path and 256 on the strided one (csrc/soft_argmax.h).
  * Z:  dZ = Z (sum p_p eps_p + (n + 1) u64)                       (+ 1: the reference's own sum, accumulated in extended precision)
  * ex: to first order ex^ - ex = sum (x_p - ex) e_p delta_p / Z, so |..| <= sum |x_p - ex| p_p eps_p; the products x_p e_p (1 rounding),
    the two sums (n each), the quotient (1) and the reference's three roundings add ex (2 n + 6) u64.
  * dmaps: c = beta / Z^ carries Z's relative error + 1, c e_p t one rounding per product, e_p its eps_p, the float64 conversions of
    beta and the reference's operations 3 more: |ref| (dZ / Z + eps_p + 6 u64); t_p is formed from the STATE's ex, ey (the forward's
    error dx, dy) with two differences, two products and one sum: beta p_p (|gx| dx + |gy| dy + 3 u64 (|(x_p - ex) gx| + |(y_p - ey) gy|)).
  * 1 % on top for the second-order terms (every first-order term is below 1e-10).
d is about 1e-13 |ref| where u32 |ref| is 6e-8 |ref|: the fp32 rounding of the result is the bound, d keeps it honest.

EXP_REL, EXP_SUB: the one constant that cannot be counted.  Measured once on an MI355X by tools/bench_soft_argmax.py (pa_exp_probe, the
function the kernels call; 2^21 arguments over [-745, 0] against numpy.longdouble; profiles/soft_argmax.txt) and DOUBLED here."""
import ctypes as C
import math

import numpy as np

U64, U32, FLOOR32 = 2.0 ** -53, 2.0 ** -24, 2.0 ** -126
# csrc/soft_argmax.h (tests/test_soft_argmax_cpu.py holds these against the header)
THREADS, INFLIGHT, GENERIC_THREADS, BWD_THREADS, BWD_CHUNKS = 1024, 4, 256, 256, 4
EXP_MEASURED_REL, EXP_MEASURED_SUB = 1.3905e-16, 0.877           # profiles/soft_argmax.txt: relative (normal results), units of 2^-1074 (subnormal)
EXP_REL, EXP_SUB = 2 * EXP_MEASURED_REL, 2 * EXP_MEASURED_SUB
SUB = 2.0 ** -1074
GUARD, SENTINEL = 64, 12345.0


def xy(H, W):
    p = np.arange(H * W)
    return (p % W + 1).astype(np.float64), (p // W + 1).astype(np.float64)


def _sum(a):
    """sum over the last axis of float64 terms, rounded once: extended precision where numpy has it, else math.fsum"""
    if np.finfo(np.longdouble).nmant > 52:
        return a.astype(np.longdouble).sum(-1).astype(np.float64)
    return np.array([math.fsum(r) for r in a.reshape(-1, a.shape[-1])]).reshape(a.shape[:-1])


def forward64(maps, W, beta):
    """maps [B][J][H*W] float32 -> dict of float64 arrays: m, Z, ex, ey [B][J]; a, e [B][J][HW]"""
    HW = maps.shape[-1]
    x, y = xy(HW // W, W)
    h = maps.astype(np.float64)
    m = h.max(-1, keepdims=True)
    with np.errstate(under='ignore'):
        a = np.float64(np.float32(beta)) * (h - m)
        e = np.exp(a)
        Z = _sum(e)
        return dict(m=m[..., 0], Z=Z, ex=_sum(x * e) / Z, ey=_sum(y * e) / Z, a=a, e=e, x=x, y=y, beta=np.float64(np.float32(beta)))


def backward64(ref, dco):
    """d loss / d maps [B][J][HW] float64 from dco [B][J][2] float32, and t"""
    gx, gy = dco[..., 0:1].astype(np.float64), dco[..., 1:2].astype(np.float64)
    with np.errstate(under='ignore'):
        t = (ref['x'] - ref['ex'][..., None]) * gx + (ref['y'] - ref['ey'][..., None]) * gy
        return ref['beta'] * ref['e'] / ref['Z'][..., None] * t, t


def longdouble_eval(maps, W, beta, dco):
    """the same formulas in numpy.longdouble throughout (the argument included) -> ex, ey, Z, dmaps as longdouble"""
    ld = np.longdouble
    HW = maps.shape[-1]
    p = np.arange(HW)
    x, y = (p % W + 1).astype(ld), (p // W + 1).astype(ld)
    h = maps.astype(ld)
    with np.errstate(under='ignore'):
        e = np.exp(ld(np.float32(beta)) * (h - h.max(-1, keepdims=True)))
        Z = e.sum(-1)
        ex, ey = (x * e).sum(-1) / Z, (y * e).sum(-1) / Z
        t = (x - ex[..., None]) * dco[..., 0:1].astype(ld) + (y - ey[..., None]) * dco[..., 1:2].astype(ld)
        return ex, ey, Z, ld(np.float32(beta)) * e / Z[..., None] * t


def n_add(HW, fast):
    T = THREADS if fast else GENERIC_THREADS
    return -(-HW // T) + 6 + T // 64 - 1


def forward_bound(ref, fast):
    """the d terms: dict dZ, dx, dy [B][J] and eps [B][J][HW], relZ [B][J]"""
    HW = ref['e'].shape[-1]
    n = n_add(HW, fast)
    Z = ref['Z']
    with np.errstate(under='ignore'):
        p = ref['e'] / Z[..., None]
        eps = EXP_REL + 2 * U64 + 2 * U64 * np.abs(ref['a'])
        relZ = (p * eps).sum(-1) + HW * EXP_SUB * SUB / Z
        out = dict(eps=eps, relZ=relZ, dZ=1.01 * Z * (relZ + (n + 1) * U64), n=n)
        for k, c in (('dx', 'x'), ('dy', 'y')):
            dist = np.abs(ref[c] - ref['e' + c][..., None])
            out[k] = 1.01 * ((dist * p * eps).sum(-1) + dist.sum(-1) * EXP_SUB * SUB / Z + ref['e' + c] * (2 * n + 6) * U64)
    return out


def backward_bound(ref, fb, dco, want, t):
    """(bound [B][J][HW] including the fp32 rounding and the 2^-126 floor, d alone)"""
    gx, gy = np.abs(dco[..., 0:1].astype(np.float64)), np.abs(dco[..., 1:2].astype(np.float64))
    Z = ref['Z'][..., None]
    with np.errstate(under='ignore'):
        p = ref['e'] / Z
        T = gx * fb['dx'][..., None] + gy * fb['dy'][..., None] + 3 * U64 * (np.abs(ref['x'] - ref['ex'][..., None]) * gx + np.abs(ref['y'] - ref['ey'][..., None]) * gy)
        rel = fb['relZ'][..., None] + (fb['n'] + 1) * U64 + fb['eps'] + 6 * U64
        d = 1.01 * (np.abs(want) * rel + ref['beta'] * p * T + ref['beta'] * EXP_SUB * SUB / Z * np.abs(t))
    return U32 * np.abs(want) + d + FLOOR32, d


def ratio(got, want, bound):
    """worst |got - want| / bound; inf where got is not finite"""
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return float('inf')
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ cases
def peak_positions(H, W):
    """pixel indices on each side of every boundary of the kernels' split: first and last pixel, lanes / waves (64), the forward's thread
    stride (T) and trip (INFLIGHT T), the backward's workgroup (64 pixels) and grid stride, a row of the map"""
    HW = H * W
    stride = -(-HW * 4 // (BWD_THREADS * BWD_CHUNKS)) * BWD_THREADS // 4
    trip = INFLIGHT * THREADS
    cand = [0, HW - 1, 63, 64, THREADS - 1, THREADS, trip - 1, trip, 2 * trip - 1, 2 * trip, stride - 1, stride, 127, 128, W - 1, W,
            GENERIC_THREADS - 1, GENERIC_THREADS, 2 * stride - 1, 2 * stride]
    out = []
    for c in cand:
        if 0 <= c < HW and c not in out:
            out.append(c)
    return out


def _peaked(seed, B, J, H, W):
    gen = np.random.Generator(np.random.PCG64(seed))
    maps = (gen.standard_normal((B, J, H * W)) * 1.5).astype(np.float32)
    pos = peak_positions(H, W)
    peaks = np.array([pos[k % len(pos)] for k in range(B * J)]).reshape(B, J)
    np.put_along_axis(maps, peaks[..., None], np.float32(8.0), axis=-1)
    return maps, peaks


def _dco(seed, B, J):
    d = np.random.Generator(np.random.PCG64(seed + 1000)).standard_normal((B, J, 2)).astype(np.float32)
    if J > 2:
        d[0, 2] = 0.0                         # a joint without gradient: its dmaps are exactly zero
    return d


FAST_SHAPES = ((1, 1), (16, 16), (64, 64), (96, 96), (8, 24))
CASES = ['fast_%dx%d_B%d' % (h, w, b) for h, w in FAST_SHAPES for b in (1, 3)] + ['fast_ramp_64x64', 'fast_ramp_8x24', 'range_3e4', 'range_3e38'] + \
        ['generic_J%d_l%d' % (j, l) for j in (1, 5, 17) for l in (0, 1)] + ['generic_offset']
FP16_CASES = ['fast_96x96_B3', 'fast_8x24_B1', 'generic_J5_l0', 'generic_offset']
_CASE_CACHE = {}


def case(name):
    """dict: maps [B][J][HW] float32, dco [B][J][2] float32, H, W, J, B, beta, layout, offset (floats the pointer is moved by), fast"""
    if name in _CASE_CACHE:
        return _CASE_CACHE[name]
    seed = CASES.index(name)
    c = dict(layout=1, offset=0, beta=1.0, J=16)
    if name.startswith('fast_ramp'):
        H, W = (64, 64) if name.endswith('64x64') else (8, 24)
        p = np.arange(H * W, dtype=np.float64)
        slope = (np.arange(16) // 2 + 1) * (8.0 / (H * W)) * np.where(np.arange(16) % 2 == 0, 1.0, -1.0)   # even joints rise, odd ones fall
        c.update(H=H, W=W, B=1, maps=(slope[:, None] * p[None, :]).astype(np.float32)[None])
    elif name.startswith('fast_'):
        shape, b = name.split('_')[1:]
        H, W = (int(v) for v in shape.split('x'))
        B = int(b[1:])
        c.update(H=H, W=W, B=B, beta=1.0 if B == 1 else 0.75, maps=_peaked(seed, B, 16, H, W)[0])
    elif name.startswith('range'):
        gen = np.random.Generator(np.random.PCG64(seed))
        if name == 'range_3e4':
            maps = gen.uniform(-3e4, 3e4, (2, 16, 256)).astype(np.float32)
        else:
            maps = np.where(gen.uniform(size=(2, 16, 256)) < 0.5, np.float32(3e38), np.float32(-3e38)).astype(np.float32)
            c['beta'] = 1e-3
        c.update(H=16, W=16, B=2, maps=maps)
    elif name == 'generic_offset':
        c.update(H=8, W=24, B=2, offset=1, maps=_peaked(seed, 2, 16, 8, 24)[0])
    else:
        J, layout = int(name.split('_')[1][1:]), int(name[-1])
        c.update(H=13, W=20, B=2, J=J, layout=layout, maps=_peaked(seed, 2, J, 13, 20)[0])
    c['dco'] = _dco(seed, c['B'], c['J'])
    c['fast'] = c['J'] == 16 and c['layout'] == 1 and c['offset'] == 0
    c['maps'].setflags(write=False)
    _CASE_CACHE[name] = c
    return c


_REF_CACHE = {}


def reference(name):
    """(case, forward reference, forward bound, dmaps reference, dmaps bound): computed once per case and shared"""
    if name not in _REF_CACHE:
        cs = case(name)
        ref = forward64(cs['maps'], cs['W'], cs['beta'])
        fb = forward_bound(ref, cs['fast'])
        want, t = backward64(ref, cs['dco'])
        bound, _ = backward_bound(ref, fb, cs['dco'], want, t)
        _REF_CACHE[name] = (cs, ref, fb, want, bound)
    return _REF_CACHE[name]


def to_storage(planar, layout):
    """[B][J][HW] -> the flat array of layout 0 ([B][J][H][W]) or 1 ([B][HW][J])"""
    return np.ascontiguousarray(planar if layout == 0 else planar.transpose(0, 2, 1)).reshape(-1)


def from_storage(flat, layout, B, J, HW):
    return flat.reshape(B, J, HW) if layout == 0 else flat.reshape(B, HW, J).transpose(0, 2, 1)


# ------------------------------------------------------------------------------------------------ the kernel, restated in numpy
def _kernel_sum(terms, T):
    """sum over the last axis in the kernel's order: thread tid adds p = tid, tid + T, ... in turn; xor butterfly over 64 lanes; waves in order"""
    B, J, HW = terms.shape
    trips = -(-HW // T)
    pad = np.zeros((B, J, trips * T))
    pad[..., :HW] = terms
    pad = pad.reshape(B, J, trips, T)
    acc = np.zeros((B, J, T))
    for k in range(trips):
        acc = acc + pad[:, :, k]
    v = acc.reshape(B, J, T // 64, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    out = v[:, :, 0, 0]
    for w in range(1, T // 64):
        out = out + v[:, :, w, 0]
    return out


def kernel_restatement(maps, H, W, beta, dco, fast, defect=None):
    """what the kernels compute, in float64 numpy with their order of additions -> (coords float32, state [B][J][4], dmaps float32).
    defect: one planted mistake (tests/test_soft_argmax_cpu.py shows that the bound tells each)"""
    T = THREADS if fast else GENERIC_THREADS
    B, J, HW = maps.shape
    p = np.arange(HW)
    row = p // (H if defect == 'row_div_H' else W)
    one = 0 if defect == 'zero_based' else 1
    x, y = (p % W + one).astype(np.float64), (row + one).astype(np.float64)
    if defect == 'swap_xy':
        x, y = y, x
    b64 = np.float64(np.float32(beta))
    h = maps.astype(np.float64)
    m = h.max(-1, keepdims=True)
    if defect == 'no_max':
        m = np.zeros_like(m)
    with np.errstate(all='ignore'):
        if defect == 'merge_no_rescale':
            # one pass with a running maximum per thread; neither the thread's sums nor the merge of the threads are rescaled
            trips = -(-HW // T)
            pad = np.full((B, J, trips * T), -np.inf)
            pad[..., :HW] = h
            run = np.maximum.accumulate(pad.reshape(B, J, trips, T), axis=2).reshape(B, J, trips * T)[..., :HW]
            e = np.exp(b64 * (h - run))
        else:
            e = np.exp(b64 * (h - m))
        if defect == 'drop_last_trip':
            e_sum = e.copy()
            e_sum[..., (HW // (INFLIGHT * T)) * (INFLIGHT * T):] = 0.0
        else:
            e_sum = e
        Z, Sx, Sy = _kernel_sum(e_sum, T), _kernel_sum(x * e_sum, T), _kernel_sum(y * e_sum, T)
        ex, ey = Sx / Z, Sy / Z
        state = np.stack([m[..., 0], Z, ex, ey], axis=-1)
        coords = np.stack([ex, ey], axis=-1).astype(np.float32)
        gx, gy = dco[..., 0:1].astype(np.float64), dco[..., 1:2].astype(np.float64)
        cx, cy = ex[..., None], ey[..., None]
        if defect == 'grad_at_argmax':
            am = h.argmax(-1)
            cx, cy = x[am][..., None], y[am][..., None]
        c = (1.0 if defect == 'no_beta_bwd' else b64) / Z[..., None]
        dmaps = ((c * e) * ((x - cx) * gx + (y - cy) * gy)).astype(np.float32)
    return coords, state, dmaps


DEFECTS = {              # planted defect -> the case that tells it
    'swap_xy': 'fast_8x24_B1', 'row_div_H': 'fast_8x24_B1', 'zero_based': 'fast_16x16_B1', 'no_beta_bwd': 'fast_16x16_B3', 'no_max': 'range_3e4',
    'merge_no_rescale': 'fast_ramp_64x64', 'grad_at_argmax': 'fast_64x64_B1', 'drop_last_trip': 'fast_96x96_B1'}


def judge(name, coords, state, dmaps):
    """worst ratios of one result against the case's reference: dict coords, state, dmaps, dsum; and the list of findings"""
    cs, ref, fb, want, bound = reference(name)
    fails = []
    state = np.asarray(state, dtype=np.float64)
    worst = dict(coords=max(ratio(coords[..., 0], ref['ex'], U32 * np.abs(ref['ex']) + fb['dx']), ratio(coords[..., 1], ref['ey'], U32 * np.abs(ref['ey']) + fb['dy'])),
                 state=max(ratio(state[..., 1], ref['Z'], fb['dZ']), ratio(state[..., 2], ref['ex'], fb['dx']), ratio(state[..., 3], ref['ey'], fb['dy'])),
                 dmaps=ratio(dmaps, want, bound))
    if not np.array_equal(state[..., 0], ref['m']):
        fails.append(('the maximum in state differs', float(np.abs(state[..., 0] - ref['m']).max())))
    if np.all(np.isfinite(state)) and not (np.array_equal(coords[..., 0], state[..., 2].astype(np.float32)) and np.array_equal(coords[..., 1], state[..., 3].astype(np.float32))):
        fails.append(('coords is not state rounded to float', 0))
    dsum = np.abs(np.asarray(dmaps, dtype=np.float64).sum(-1))
    worst['dsum'] = ratio(dsum, 0.0, bound.sum(-1))
    for k, v in worst.items():
        if not v <= 1.0:
            fails.append(('%s leaves its bound' % k, v))
    zero = (cs['dco'] == 0).all(-1)
    if zero.any() and not np.all(np.asarray(dmaps)[zero] == 0):
        fails.append(('a joint with dcoords == 0 has a non-zero gradient', 0))
    return worst, fails


# ------------------------------------------------------------------------------------------------ the device
def _guarded(n, dtype, fill, shift=0):
    """a device buffer of GUARD + shift + n + GUARD elements: sentinel outside, `fill` inside; returns (buffer, first element, pointer)"""
    import torch
    buf = torch.full((2 * GUARD + shift + n,), SENTINEL, dtype=dtype, device='cuda')
    buf[GUARD + shift:GUARD + shift + n] = fill
    return buf, GUARD + shift, C.c_void_p(buf.data_ptr() + (GUARD + shift) * buf.element_size())


def _guards_ok(buf, first, n):
    return bool((buf[:first] == SENTINEL).all()) and bool((buf[first + n:] == SENTINEL).all())


def device_call(cs, lib=None):
    """pa_soft_argmax and pa_soft_argmax_bwd on a case, outputs pre-filled with NaN inside guard regions ->
    (coords [B][J][2], state [B][J][4], dmaps [B][J][HW] as numpy, the three device buffers' payloads as tensors, findings)"""
    import torch
    from pose_adv_aug_amd._lib import lib as _lib, check, stream
    L = lib or _lib()
    B, J, H, W, lay, off = cs['B'], cs['J'], cs['H'], cs['W'], cs['layout'], cs['offset']
    n = B * J * H * W
    flat = to_storage(cs['maps'], lay).copy()
    mbuf, mfirst, mptr = _guarded(n, torch.float32, 0.0, off)
    mbuf[mfirst:mfirst + n] = torch.from_numpy(flat).cuda()
    dco = torch.from_numpy(cs['dco']).cuda()
    cbuf, cfirst, cptr = _guarded(B * J * 2, torch.float32, float('nan'))
    sbuf, sfirst, sptr = _guarded(B * J * 4, torch.float64, float('nan'))
    dbuf, dfirst, dptr = _guarded(n, torch.float32, float('nan'), off)
    check(L.pa_soft_argmax(mptr, lay, B, J, H, W, cs['beta'], cptr, sptr, stream()), 'pa_soft_argmax')
    check(L.pa_soft_argmax_bwd(mptr, lay, B, J, H, W, cs['beta'], sptr, C.c_void_p(dco.data_ptr()), dptr, stream()), 'pa_soft_argmax_bwd')
    torch.cuda.synchronize()
    fails = []
    for what, buf, first, cnt in (('coords', cbuf, cfirst, B * J * 2), ('state', sbuf, sfirst, B * J * 4), ('dmaps', dbuf, dfirst, n), ('maps', mbuf, mfirst, n)):
        if not _guards_ok(buf, first, cnt):
            fails.append(('the guard region around %s was written' % what, 0))
    if not torch.equal(mbuf[mfirst:mfirst + n].cpu(), torch.from_numpy(flat)):
        fails.append(('maps was changed', 0))
    pay = (cbuf[cfirst:cfirst + B * J * 2], sbuf[sfirst:sfirst + B * J * 4], dbuf[dfirst:dfirst + n])
    for what, t in zip(('coords', 'state', 'dmaps'), pay):
        if bool(torch.isnan(t).any()):
            fails.append(('%s is not fully overwritten (NaN left)' % what, int(torch.isnan(t).sum())))
    coords = pay[0].cpu().numpy().reshape(B, J, 2)
    state = pay[1].cpu().numpy().reshape(B, J, 4)
    dmaps = from_storage(pay[2].cpu().numpy(), lay, B, J, H * W)
    return coords, state, dmaps, pay, fails


def operator_leg(name, verbose=False):
    """a case through the C ABI: every element of coords, state and dmaps within its bound, sum_p dmaps within the summed bound of 0,
    outputs fully overwritten, guards untouched, a second run bit-identical -> (findings, worst ratios)"""
    import torch
    cs = case(name)
    coords, state, dmaps, pay, fails = device_call(cs)
    worst, f2 = judge(name, coords, state, dmaps)
    fails += f2
    _, _, _, pay2, _ = device_call(cs)
    if not all(torch.equal(a, b) for a, b in zip(pay, pay2)):
        fails.append(('two runs differ', 0))
    if verbose:
        print('%-20s %s' % (name, ' '.join('%s %.4f' % kv for kv in sorted(worst.items()))), flush=True)
    return fails, worst


def main():
    """the fp16 build's subset (the operator is fp32 in both builds): run as a child process with POSEADV_DTYPE=fp16"""
    import torch
    from pose_adv_aug_amd import _lib
    torch.cuda.set_device(0)
    bad = []
    for name in FP16_CASES:
        fails, _ = operator_leg(name, verbose=True)
        bad += [(name, f) for f in fails]
    if bad or _lib.DTYPE != 'fp16':
        print('FAILED', _lib.DTYPE, bad)
        raise SystemExit(1)
    print('FP16 SOFT ARGMAX PASSED')


if __name__ == '__main__':
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
