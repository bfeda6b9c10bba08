"""The stand-alone pose-library operators of csrc/pose_ops.hip and the layout converters, element by element: pa_affine_warp_bilinear(_sized)
(forward), pa_affine_params, pa_transform_pts(_sized), pa_gaussian_heatmap, pa_weighted_l2, pa_flip_lr_nhwc4, pa_flip_tta_merge,
pa_nchw_to_nhwc / pa_nhwc_to_nchw.  Every comparison is bit equality or a bound whose constants are counted from the kernel's operations;
u64 = 2^-53, u32 = 2^-24 (the unit roundoffs of double and float).

1. Warp forward.  warp64 restates the sampler per output pixel in numpy float64 on the per-pixel quantities of warp_grad_exact._sample
(sx = ti0 u + ti1 v + ti2, sy likewise, the four taps around the floor, 0 outside the sample's own frame, mirrored when flip):
S_c = sum w_k p_k / 255, ref = clip(g_c S_c, 0, 1).  tinv is an OPERAND (the GPU legs pass the device's own pa_affine_params output).
  |outf - ref| <= d + u32 (|ref| + d),   d = u64 (c mag + c_xy mag_xy)
  mag = |g_c| sum |w_k| p_k / 255 (the weights are >= 0, so this is |g_c| S_c).
  c = 9 + 9.  One value of the kernel takes 9 double roundings along its longest path: 1 - ax (1), 1 - ay (1), the tap weight (1), p / 255 (1),
  their product (1), three additions of S (3; the first addend meets an exact 0), the product with the gain (1); the clamp is exact and
  1-Lipschitz.  warp64 forms the same value with its own 9.  With multiply-add contraction (pose_ops.hip is compiled with it) a product
  and the addition behind it round once instead of twice: fewer roundings, never more.  The cast to float is the u32 (|ref| + d) term.
  mag_xy: a fraction ax = sx - floor(sx) inherits the absolute rounding error of sx, at most u64 Mx per operation with
  Mx = |ti0 u| + |ti1 v| + |ti2| + |floor sx| (warp_grad_exact._sample), five operations in the kernel and five in the reference:
  c_xy = 5 + 5.  Every tap weight that holds ax moves by that error times its other factor, so the value moves by at most
  |g_c| (Mx ((1 - ay)(q00 + q01) + ay (q10 + q11)) + My ((1 - ax)(q00 + q10) + ax (q01 + q11))), q = p / 255: warp_grad_exact's S_xy.
  The zero-padded bilinear sampler followed by a clamp is continuous in (sx, sy): no condition on the distance from an integer or from
  the clamp is needed, integer coordinates and saturated pixels are legal inputs.
  Condition (warp_conditions, asserted on the CPU for every case from the reference alone): every d < 2^-30, so the bound can never
  pass a wrong tap (one byte step of one tap at weight 1/4 is 1e-3).
  out4: channels 0..2 are outf rounded to the storage type, round to nearest even (outf.to(act_dtype())), bit for bit; channel 3 is +0.

2. pa_affine_params.  The reference of t_out is oracle.pylib.get_transform in numpy float64; of tinv_in the cofactor inverse of that
transform.  The bound is a running first-order error analysis (class E): every quantity carries |error| <= e u64, every operation adds
2 |result| (ONE rounding in the kernel and ONE in the reference) to the propagated errors of its operands, i.e. per coefficient
u64 * c * (the sum of the absolute values of the terms that form it) with c counted operation by operation instead of once for the
longest path.  The paths: make_transform h (1), res / h (1), c / h (1), + 0.5 (1), * res (1), - hr (1), * cs / sn (1), the difference
(1), + hr (1) = at most 9 roundings; invert_affine two products and a difference for det (3), a quotient (1), two products, a sum (3).
sin / cos: TRIG = 6 units of |sin| (|cos|): the device's double sin / cos are good to 2 ulp = 4 u64, the host's to 1 ulp = 2 u64; their
argument -rot pi / 180 carries two roundings on each side, which move sin by |rr| 4 u64 |cos| and cos by |rr| 4 u64 |sin| (so an exact
zero of the cosine at 90 degrees is not required of either side).  t(res) o tinv(res) = identity within
sum_k |t_ik| e(tinv_kj) + e(t_ik) |tinv_kj| (the product itself is formed exactly, in rationals).

3. pa_transform_pts(_sized).  The device's own t is the operand.  x' = width - x in fp32 when flip (pts_img: bit-exact), the joints of a
flipped sample read from their left / right partner when J == 16 and from themselves otherwise; x' <= 0 or y <= 0 gives exactly (0, 0);
else |out - (t0 x' + t1 y + t2)| <= u64 * 4 * (|t0 x'| + |t1 y| + |t2|): two products and two additions, the kernel's and the
reference's (contraction: fewer).

4. pa_gaussian_heatmap: bit-equal with oracle.pylib.pts2heatmap(...).astype(float32).

5. pa_weighted_l2.  Reference: math.fsum of the float64 terms (p - g)^2 w, divided by n (plus the start value of *loss).
  |loss - ref| <= u32 D sum |term| / n (+ u32 * 1.5 when *loss starts at 1.5)
  D = 3 + L + 6 + 3 + 1 + blocks: the difference, the square and the product with the weight (3), the per-thread chain of
  L = ceil(n / (256 blocks)) additions, 6 shuffle levels of the wave sum, 3 additions of the four waves' partials, the product with
  1 / n, and blocks = min(ceil(n / 256), 1024) atomic additions in any order, each charged at the full sum.  (The one rounding of
  1 / n and the reference's three double roundings per term disappear in that last charge: the partial sums the atomics round are on
  average half the full sum.)  The atomics make two runs differ in the last bits: no bit equality here.
  The sentinel leg is exact instead: pred - gt = 0 except 1 at ONE index e with w[e] = 3; the loss must be fl32(3 fl32(1 / fl32(n))).

6. pa_flip_lr_nhwc4, pa_flip_tta_merge, pa_nchw_to_nhwc, pa_nhwc_to_nchw: bit-equal with torch on the host.

Run as a script (POSEADV_DTYPE=fp16) this executes every GPU leg in the loaded build and prints PYLIB EXACT PASSED."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))        # (run as a script by the fp16 leg)
from tests import inputs  # noqa: E402
from tests import warp_grad_exact as W  # noqa: E402

U64 = 2.0 ** -53
U32 = 2.0 ** -24
C_WARP = 9 + 9
C_XY = 5 + 5
D_CAP = 2.0 ** -30
TRIG = 6.0
PAD = 8                     # guard elements on each side of every output
GRID_WARP = 8192 * 256      # pa_launch_warp's grid cap in pixels
WORST = {}                  # leg -> worst error / bound of the run (report())


def _note(leg, ratio):
    WORST[leg] = max(WORST.get(leg, 0.0), float(ratio))


def report(log=print):
    for leg in sorted(WORST):
        log('pylib_exact %s: worst error / bound %.3g' % (leg, WORST[leg]))


def ratio(got, ref, bound):
    """max |got - ref| / bound; an element with bound 0 must be equal"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.max(r)) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. warp forward
WARP_CASES = ('a', 'b', 'c', 'd', 'int', 'sat', 'out', 'tiny_r1_1x1', 'tiny_r3_1x1', 'tiny_r1_2x3', 'tiny_r3_2x3', 'stride')


def _params(c, s, r, flip, gain):
    p = np.zeros((len(s), 8))
    p[:, 0:2], p[:, 2], p[:, 3], p[:, 4], p[:, 5:8] = np.asarray(c), s, r, flip, gain
    return p


def warp_case(name):
    """dict(name, frames uint8 [B][Hs][Ws][3], sizes int32 [B][2] or None, params float64 [B][8], res)"""
    if name in W.CASES:
        cs = W.case(name)
        return dict(name=name, frames=cs['frames'], sizes=cs['sizes'], params=cs['params'], res=cs['res'])
    sizes = None
    if name == 'int':           # the original forward test: the centre of the output maps onto an integer source pixel
        frames = inputs.rng(90).integers(0, 256, size=(3, 90, 120, 3), dtype=np.uint8)
        p = _params([[60.0, 45.0], [50.0, 40.0], [70.0, 30.0]], [0.35, 0.5, 0.28], [0.0, 25.0, -40.0], [0, 1, 0],
                    np.array([[1, 1, 1], [0.7, 1.3, 1.0], [1.4, 0.6, 1.2]], dtype=np.float32).astype(np.float64))
        res = 64
    elif name == 'sat':         # bright frames under gain 1.4: many pixels clamp to exactly 1.0
        frames = inputs.rng(94).integers(180, 256, size=(2, 40, 50, 3), dtype=np.uint8)
        p = _params([[25.3, 20.2], [24.1, 19.7]], [0.15, 0.12], [0.0, 20.0], [0, 1], np.full((2, 3), 1.4))
        res = 32
    elif name == 'out':         # one window wholly outside its frame; one hanging over the top-left corner (negative coordinates)
        frames = inputs.rng(95).integers(1, 256, size=(2, 30, 40, 3), dtype=np.uint8)
        p = _params([[-500.5, -400.25], [3.3, 2.6]], [0.2, 0.2], [15.0, -10.0], [0, 0], [[1.0, 1.1, 0.9], [1.2, 1.0, 0.8]])
        res = 16
    elif name.startswith('tiny'):
        res = int(name[6])
        hs, ws = (1, 1) if name.endswith('1x1') else (2, 3)
        frames = inputs.rng(96, res, hs).integers(100, 256, size=(1, hs, ws, 3), dtype=np.uint8)
        # a window of two source pixels around the frame: centre near the frame's, scale 0.01 (h = 2), some rotation at res 3
        p = _params([[0.4 * ws, 0.3 * hs]], [0.01], [0.0 if res == 1 else 30.0], [0 if res == 1 else 1], [[1.0, 0.9, 1.1]])
    elif name == 'stride':      # the smallest round shape past the grid cap: the grid-stride loop runs
        g = inputs.rng(97)
        B, res = 9, 512
        sizes = np.array([[32, 24]] * B, dtype=np.int32)
        sizes[2], sizes[6] = (20, 24), (27, 19)
        frames = np.full((B, 24, 32, 3), 200, dtype=np.uint8)
        for i, (w, h) in enumerate(sizes):
            frames[i, :h, :w] = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        c = np.stack([sizes[:, 0] * g.uniform(0.4, 0.6, B), sizes[:, 1] * g.uniform(0.4, 0.6, B)], axis=1)
        p = _params(c, g.uniform(0.1, 0.2, B), g.uniform(-45, 45, B), (np.arange(B) % 3 == 2).astype(np.float64), g.uniform(0.7, 1.3, size=(B, 3)))
    else:
        raise KeyError(name)
    return dict(name=name, frames=frames, sizes=sizes, params=p, res=res)


def warp64(frames, sizes, tinv, params, res):
    """-> (ref [B][3][res][res] float64, d [B][3][res][res]: the double part of the bound)"""
    frames, tinv, params = np.asarray(frames), np.asarray(tinv, dtype=np.float64), np.asarray(params, dtype=np.float64)
    B = params.shape[0]
    ref, d = np.zeros((B, 3, res, res)), np.zeros((B, 3, res, res))
    for b in range(B):
        wb, hb = (int(sizes[b][0]), int(sizes[b][1])) if sizes is not None else (frames.shape[2], frames.shape[1])
        u, v, sx, sy, ax, ay, taps, oks, Mx, My = W._sample(frames[b], wb, hb, tinv[b], params[b], res)
        g = params[b, 5:8]
        axc, ayc = ax[..., None], ay[..., None]
        wx0, wy0 = 1.0 - axc, 1.0 - ayc
        q = taps / 255.0
        S = (wx0 * wy0) * q[0]
        S = S + (axc * wy0) * q[1]
        S = S + (wx0 * ayc) * q[2]
        S = S + (axc * ayc) * q[3]
        ref[b] = np.clip(S * g, 0.0, 1.0).transpose(2, 0, 1)
        S_xy = Mx[..., None] * (wy0 * (q[0] + q[1]) + ayc * (q[2] + q[3])) + My[..., None] * (wx0 * (q[0] + q[2]) + axc * (q[1] + q[3]))
        d[b] = (U64 * (C_WARP * np.abs(g) * S + C_XY * np.abs(g) * S_xy)).transpose(2, 0, 1)
    return ref, d


def warp_bound(ref, d):
    return d + U32 * (np.abs(ref) + d)


def warp_conditions(cs, ref, d):
    """the list of violated case conditions, from the reference alone"""
    bad = []
    if not float(d.max()) < D_CAP:
        bad.append('d reaches %.3g, not below 2^-30' % float(d.max()))
    B, res = cs['params'].shape[0], cs['res']
    if cs['name'] == 'sat' and not float((ref == 1.0).mean()) > 0.1:
        bad.append('the saturated share is %.3g' % float((ref == 1.0).mean()))
    if cs['name'] == 'out' and not (bool((ref[0] == 0).all()) and float(ref[1].max()) > 0 and bool((ref[1][:, 0, 0] == 0).all())):
        bad.append('sample 0 is not all zero, or sample 1 does not hang over the corner')
    if cs['name'] == 'stride' and not B * res * res > GRID_WARP:
        bad.append('B * res * res does not exceed the grid cap')
    if cs['name'] != 'out' and not all(float(ref[b].max()) > 0 for b in range(B)):
        bad.append('a sample with an all-zero reference')
    if cs['name'] == 'b' and int((cs['frames'] == 200).sum()) == 0:
        bad.append('no padding bytes')
    return bad


def out4_mismatches(out4, outf, dtype):
    """number of elements of out4 [B][res][res][4] (storage type) that are not outf [B][3][res][res] (fp32) rounded to nearest even
    (channels 0..2) / not +0 (channel 3), compared as bits"""
    want = outf.permute(0, 2, 3, 1).to(dtype).contiguous().view(torch.int16)
    got = out4.contiguous().view(torch.int16)
    return int((got[..., :3] != want).sum()) + int((got[..., 3] != 0).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. pa_affine_params: running error analysis
class E(object):
    """a float64 value v with |error| <= e u64 on either side (kernel and reference)"""
    __slots__ = ('v', 'e')

    def __init__(self, v, e=0.0):
        self.v, self.e = float(v), float(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    @staticmethod
    def _op(v, e):
        return E(v, e + 2.0 * abs(v))               # one rounding in the kernel, one in the reference

    def __neg__(self):
        return E(-self.v, self.e)

    def __add__(self, o):
        o = E.of(o)
        return E._op(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = E.of(o)
        return E._op(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = E.of(o)
        return E._op(self.v * o.v, abs(self.v) * o.e + abs(o.v) * self.e)

    def __truediv__(self, o):
        o = E.of(o)
        return E._op(self.v / o.v, self.e / abs(o.v) + abs(self.v / o.v) * o.e / abs(o.v))


def transform_E(cx, cy, scale, rot, res, size=200.0):
    """make_transform of csrc/pose_ops.hip, operation by operation -> [6] E"""
    h = E(size) * scale
    a = E(res) / h
    tx = E(res) * ((-E(cx)) / h + 0.5)
    ty = E(res) * ((-E(cy)) / h + 0.5)
    t = [a, E(0.0), tx, E(0.0), a, ty]
    if rot != 0.0:
        rr = (-E(rot)) * 3.14159265358979323846 / 180.0
        sn = E(math.sin(rr.v), rr.e * abs(math.cos(rr.v)) + TRIG * abs(math.sin(rr.v)))
        cs = E(math.cos(rr.v), rr.e * abs(math.sin(rr.v)) + TRIG * abs(math.cos(rr.v)))
        hr = res / 2.0
        t = [cs * t[0], (-sn) * t[4], cs * (t[2] - hr) - sn * (t[5] - hr) + hr,
             sn * t[0], cs * t[4], sn * (t[2] - hr) + cs * (t[5] - hr) + hr]
    return t


def invert_E(t):
    """invert_affine of csrc/pose_ops.hip -> [6] E"""
    det = t[0] * t[4] - t[1] * t[3]
    i0, i1, i3, i4 = t[4] / det, (-t[1]) / det, (-t[3]) / det, t[0] / det
    return [i0, i1, -(i0 * t[2] + i1 * t[5]), i3, i4, -(i3 * t[2] + i4 * t[5])]


AFFINE_RES = ((256, 64), (384, 96), (64, 64), (1, 1))
AFFINE_ROTS = (0.0, -0.0, 90.0, 180.0, 360.0, 1e-9, 37.5, -37.5)


def affine_case(B=65):
    """params [B][8]: every rotation of AFFINE_ROTS, scales 0.05 .. 10 (both ends included), centres in a 1280 x 720 frame"""
    g = inputs.rng(98)
    s = np.exp(np.linspace(np.log(0.05), np.log(10.0), B))
    s[0], s[-1] = 0.05, 10.0
    g.shuffle(s)
    c = np.stack([g.uniform(0, 1280, B), g.uniform(0, 720, B)], axis=1)
    c[:4] = [[0.0, 0.0], [640.0, 360.0], [1280.0, 720.0], [100.0, 200.0]]
    r = np.array([AFFINE_ROTS[i % len(AFFINE_ROTS)] for i in range(B)])
    return _params(c, s, r, (np.arange(B) % 2).astype(np.float64), g.uniform(0.6, 1.4, size=(B, 3)))


def affine_reference(params, res_in, res_out):
    """-> (t [B][6], bound of t, tinv [B][6], bound of tinv): t from oracle.pylib.get_transform at res_out, tinv the cofactor inverse of
    get_transform at res_in (float64, invert_affine's formula); the bounds from the running analysis"""
    from oracle import pylib as opl
    B = params.shape[0]
    t, bt, ti, bi = (np.zeros((B, 6)) for _ in range(4))
    for b, p in enumerate(params):
        te = transform_E(p[0], p[1], p[2], p[3], float(res_out))
        t[b] = opl.get_transform(p[0:2], p[2], p[3], res_out)[:2].reshape(6)
        bt[b] = [U64 * x.e for x in te]
        tin = transform_E(p[0], p[1], p[2], p[3], float(res_in))
        oin = opl.get_transform(p[0:2], p[2], p[3], res_in)[:2].reshape(6)
        ie = invert_E([E(v, x.e) for v, x in zip(oin, tin)])
        ti[b] = [x.v for x in ie]
        bi[b] = [U64 * x.e for x in ie]
    return t, bt, ti, bi


def compose_exact(t, ti):
    """t o ti of two [6] double rows, formed exactly -> [6] floats (the deviation from the identity is what is looked at)"""
    a = [Fraction(float(x)) for x in t]
    b = [Fraction(float(x)) for x in ti]
    m = [a[0] * b[0] + a[1] * b[3], a[0] * b[1] + a[1] * b[4], a[0] * b[2] + a[1] * b[5] + a[2],
         a[3] * b[0] + a[4] * b[3], a[3] * b[1] + a[4] * b[4], a[3] * b[2] + a[4] * b[5] + a[5]]
    ident = (1, 0, 0, 0, 1, 0)
    return np.array([float(x - i) for x, i in zip(m, ident)])


def compose_bound(t, bt, ti, bi):
    """|t o ti - identity| per coefficient, first order: sum_k |t_ik| e(ti_kj) + e(t_ik) |ti_kj| (+ e(t_i2) in the last column)"""
    at, ai = np.abs(t), np.abs(ti)
    out = np.zeros(6)
    for i in (0, 1):
        r = 3 * i
        for j in range(3):
            out[r + j] = at[r] * bi[j] + bt[r] * ai[j] + at[r + 1] * bi[3 + j] + bt[r + 1] * ai[3 + j]
        out[r + 2] += bt[r + 2]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. pa_transform_pts
PERM16 = np.array([5, 4, 3, 2, 1, 0, 6, 7, 8, 9, 15, 14, 13, 12, 11, 10])
F32_DENORM = np.float32(1e-45)                  # the least positive float
F32_MINNORM = np.float32(2.0 ** -126)


def pts_case(J, sized, B=65):
    """dict(pts fp32 [B][J][2], params [B][8], width (float) or sizes int32 [B][2]).  Samples alternate unflipped / flipped.  Sample 0
    (unflipped) holds y == 0, x == 0, and y, x just inside (the least denormal and the least normal float); sample 1 (flipped) holds
    x == width (mirrors onto 0: invalid), the float below width (valid), y == 0 and x > width; sample 2 and 3 repeat them at other joints"""
    assert J >= 5
    g = inputs.rng(99, J, int(sized))
    widths = g.integers(600, 1281, size=B).astype(np.int32) if sized else np.full(B, 1280, dtype=np.int32)
    pts = np.stack([g.uniform(1.0, widths[:, None] - 1.0, size=(B, J)), g.uniform(1.0, 700.0, size=(B, J))], axis=2).astype(np.float32)
    flip = (np.arange(B) % 2).astype(np.float64)
    for b, j0 in ((0, 0), (2, J - 5)):
        pts[b, j0 + 0, 1] = 0.0
        pts[b, j0 + 1, 0] = 0.0
        pts[b, j0 + 2, 1] = F32_DENORM
        pts[b, j0 + 3, 0] = F32_DENORM
        pts[b, j0 + 4] = [F32_MINNORM, F32_MINNORM]
    for b, j0 in ((1, 0), (3, J - 4)):
        w = np.float32(widths[b])
        pts[b, j0 + 0, 0] = w
        pts[b, j0 + 1, 0] = np.nextafter(w, np.float32(0))
        pts[b, j0 + 2, 1] = 0.0
        pts[b, j0 + 3, 0] = w + np.float32(3.5)
    c = np.stack([g.uniform(100, 500, B), g.uniform(100, 600, B)], axis=1)
    r = np.array([(0.0, 25.0, -40.0, 90.0)[i % 4] for i in range(B)])
    p = _params(c, g.uniform(0.5, 3.0, B), r, flip, np.ones((B, 3)))
    sizes = np.stack([widths, np.full(B, 720, dtype=np.int32)], axis=1).astype(np.int32) if sized else None
    return dict(pts=pts, params=p, width=1280.0, sizes=sizes, J=J, B=B)


def pts_reference(cs, t):
    """-> (out [B][J][2] float64, bound, pts_img fp32 [B][J][2], invalid [B][J]) with the operand t [B][6]"""
    pts, p, J, B = cs['pts'], cs['params'], cs['J'], cs['B']
    out, bound, invalid = np.zeros((B, J, 2)), np.zeros((B, J, 2)), np.zeros((B, J), dtype=bool)
    img = np.zeros((B, J, 2), dtype=np.float32)
    for b in range(B):
        flip = p[b, 4] != 0
        src = PERM16 if (flip and J == 16) else np.arange(J)
        x, y = pts[b, src, 0], pts[b, src, 1]
        w = np.float32(cs['sizes'][b, 0]) if cs['sizes'] is not None else np.float32(cs['width'])
        xp = (w - x).astype(np.float32) if flip else x
        img[b, :, 0], img[b, :, 1] = xp, y
        ok = ~((xp <= 0) | (y <= 0))
        invalid[b] = ~ok
        x64, y64 = xp.astype(np.float64), y.astype(np.float64)
        for k in (0, 1):
            a, bb, c = t[b, 3 * k] * x64, t[b, 3 * k + 1] * y64, t[b, 3 * k + 2]
            out[b, :, k] = np.where(ok, a + bb + c, 0.0)
            bound[b, :, k] = np.where(ok, U64 * 4 * (np.abs(a) + np.abs(bb) + abs(c)), 0.0)
    return out, bound, img, invalid


def pts_planted_ok(cs, invalid):
    """the planted joints of pts_case are invalid / valid as planned (a flipped 16-joint sample shows joint k at its partner's place)"""
    J = cs['J']
    at = (lambda k: PERM16[k]) if J == 16 else (lambda k: k)
    return (invalid[0, :5].tolist() == [True, True, False, False, False] and invalid[2, J - 5:].tolist() == [True, True, False, False, False]
            and [bool(invalid[1, at(k)]) for k in range(4)] == [True, False, True, True]
            and [bool(invalid[3, at(J - 4 + k)]) for k in range(4)] == [True, False, True, True] and int(invalid.sum()) == 10)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. pa_gaussian_heatmap
HEAT_SHAPES = ((48, 80), (80, 48), (5, 9), (3, 3), (1, 1))
HEAT_JOINTS = (1, 7, 16)


def heat_points(H, Wd):
    """the hand-placed points of one map shape, [n][2] (x, y)"""
    up = lambda v: float(np.nextafter(float(v), np.inf))
    lx, ly = min(1.5, 0.75 * Wd), min(1.5, 0.75 * H)                                                  # a valid coordinate on every map
    P = [(0.5, 0.5), (Wd - 0.5, 0.5), (0.5, H - 0.5), (Wd - 0.5, H - 0.5),                          # the patch across each corner
         (Wd / 2.0, 0.7), (Wd / 2.0, H - 0.2), (0.3, H / 2.0), (Wd - 0.1, H / 2.0),                  # ... and each edge
         (2.5, 2.25), (2.5, H / 2.0 + 0.5), (Wd / 2.0 + 0.5, 2.9), (2.001, 2.999),                   # pt - 3 in (-1, 0): truncation toward zero
         (3.0, 3.0), (3.5, 3.5), (Wd / 2.0 + 0.25, H / 2.0 + 0.75),
         (float(Wd), float(H)), (float(Wd), ly), (lx, float(H)),                                      # x == W, y == H: valid
         (up(Wd), ly), (lx, up(H)), (up(Wd), up(H)),                                                  # the next double above: invalid
         (H + 0.5, ly), (lx, Wd + 0.5), (Wd + 0.5, ly), (lx, H + 0.5),                                # one coordinate valid, the other past ITS limit
         (Wd - 0.25, H + 2.5), (Wd + 2.5, H - 0.25), (min(H, Wd) + 1.5, min(H, Wd) + 1.5),
         (0.0, 5.0), (5.0, 0.0), (0.0, 0.0), (-1.0, -1.0), (-0.5, 2.0), (1e-9, 1e-9), (1e6, 1e6), (Wd + 3.0, H + 3.0), (Wd + 2.999, 1.0)]
    return np.array(P, dtype=np.float64)


def heat_batches(H, Wd, J, B=3):
    """the points of heat_points(H, W) laid out as as many [B][J][2] batches as it takes to hold them all (the rest: (0, 0))"""
    P = heat_points(H, Wd)
    per = B * J
    out = []
    for i in range(0, len(P), per):
        chunk = np.zeros((per, 2))
        chunk[:len(P[i:i + per])] = P[i:i + per]
        out.append(chunk.reshape(B, J, 2))
    return out


def heat_reference(pts, H, Wd):
    from oracle import pylib as opl
    return np.stack([opl.pts2heatmap(pts[b].copy(), [H, Wd])[0] for b in range(pts.shape[0])]).astype(np.float32)


def heat_mismatches(got, pts, H, Wd):
    """number of elements of got [B][J][H][W] fp32 that differ in bits from the oracle's map"""
    ref = heat_reference(pts, H, Wd)
    return int((np.asarray(got, dtype=np.float32).view(np.int32) != ref.view(np.int32)).sum())


def heat_model(pts, H, Wd, swap=False):
    """gauss_patch / gauss_value of csrc/pose_ops.hip restated in numpy (the CPU test holds it against the oracle on every case);
    swap=True transposes H and W in gauss_patch: the planted error a non-square map must expose"""
    B, J = pts.shape[:2]
    out = np.zeros((B, J, H, Wd), dtype=np.float32)
    hh, ww = (Wd, H) if swap else (H, Wd)
    tab = np.exp(-np.arange(19) / 9.0).astype(np.float32)
    for b in range(B):
        for j in range(J):
            px, py = float(pts[b, j, 0]), float(pts[b, j, 1])
            if px <= 0.0 or py <= 0.0 or px > ww or py > hh:
                continue
            ulx, uly, brx, bry = int(px - 3.0), int(py - 3.0), int(px + 3.0), int(py + 3.0)
            if ulx >= ww or uly >= hh or brx < 0 or bry < 0:
                continue
            for y in range(max(uly, 0), min(uly + 6, bry, H - 1) + 1):
                for x in range(max(ulx, 0), min(ulx + 6, brx, Wd - 1) + 1):
                    out[b, j, y, x] = tab[(x - ulx - 3) ** 2 + (y - uly - 3) ** 2]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. pa_weighted_l2
L2_SIZES = (1, 63, 64, 255, 256, 257, 1000, 262144, 262145, 600001)
L2_CAP = 1024


def l2_blocks(n):
    return min((n + 255) // 256, L2_CAP)


def l2_case(n, weighted):
    g = inputs.rng(100, n, int(weighted))
    pred, gt = g.standard_normal(n).astype(np.float32), g.standard_normal(n).astype(np.float32)
    w = g.uniform(0.5, 1.5, n).astype(np.float32) if weighted else None
    return pred, gt, w


def l2_reference(pred, gt, w, start=0.0):
    """-> (ref, bound)"""
    n = pred.size
    d = pred.astype(np.float64) - gt.astype(np.float64)
    terms = d * d * (w.astype(np.float64) if w is not None else 1.0)
    blocks = l2_blocks(n)
    D = 3 + (n + 256 * blocks - 1) // (256 * blocks) + 6 + 3 + 1 + blocks
    mag = math.fsum(np.abs(terms).tolist()) / n
    return start + math.fsum(terms.tolist()) / n, U32 * D * mag + (U32 * 1.5 if start != 0.0 else 0.0)


def l2_sentinels(n):
    """the sentinel positions of one n: the first and last element of the first block, the first of the second, the last element of
    the first grid pass, the first of the grid-stride pass, the last element"""
    b = l2_blocks(n)
    return sorted({e for e in (0, 255, 256, 256 * b - 1, 256 * b, n - 1) if 0 <= e < n})


def l2_sentinel_value(n):
    return np.float32(3.0) * (np.float32(1.0) / np.float32(n))


def l2_sentinel_ok(got, n):
    return np.float32(got).view(np.int32) == l2_sentinel_value(n).view(np.int32)


def l2_model(pred, gt, w, passes=None):
    """the kernel's sum in fp32 without its tree (exact on a sentinel input, where one term is non-zero); passes = 1 drops the
    grid-stride increment (only the first 256 * blocks elements are read): the planted error of the CPU test"""
    n = pred.size
    m = n if passes is None else min(n, 256 * l2_blocks(n) * passes)
    d = pred[:m] - gt[:m]
    return np.float32(np.sum(d * d * (w[:m] if w is not None else np.float32(1)), dtype=np.float32) * (np.float32(1.0) / np.float32(n)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. flips and converters: shapes
FLIP_LR_SHAPES = ((1, 1, 1), (2, 3, 5), (5, 512, 512))                       # the last: 1 310 720 pixels, past 4096 x 256
TTA_SHAPES = ((1, 16, 1, 1), (2, 16, 5, 7), (5, 16, 128, 128))
CONVERT_SHAPES = ((2, 1, 5, 7), (2, 3, 5, 7), (2, 64, 5, 7), (2, 100, 5, 7), (2, 64, 96, 96))


def wide_floats(seed, shape):
    """fp32 values over eight decades (inside the range of both storage types), both signs, with exact zeros"""
    g = inputs.rng(101, seed)
    x = (g.standard_normal(shape) * 10.0 ** g.uniform(-5, 3, shape)).astype(np.float32)
    x[g.random(shape) < 0.02] = 0.0
    return x


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU legs (shared by tests/test_gpu_pylib_exact.py and the half-precision child below).  Each returns a list of failures.
def _dev():
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd._lib import check, lib, ptr, stream
    return _lib, lib(), check, ptr, stream


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


class Guarded(object):
    """n elements of dtype with PAD guard elements on each side, everything filled with `fill`"""

    def __init__(self, shape, dtype, fill):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * PAD,), fill, dtype=dtype, device='cuda')
        self.fill = self.buf[0].clone()
        self.t = self.buf[PAD:PAD + self.n].view(*shape)

    def intact(self):
        g = torch.cat([self.buf[:PAD], self.buf[PAD + self.n:]])
        return bool((g == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


_WREF = {}


def warp_reference(name, tinv):
    key = (name, np.asarray(tinv).tobytes())
    if key not in _WREF:
        cs = warp_case(name)
        _WREF[key] = warp64(cs['frames'], cs['sizes'], tinv, cs['params'], cs['res'])
    return _WREF[key]


def warp_leg(name, log=print):
    """pa_affine_warp_bilinear(_sized) on a case: every element of outf within its bound, out4 = outf rounded to the storage type bit for
    bit with a +0 fourth channel, one output alone and a second call give the bits of the full call, the guards stay"""
    _lib, L, check, ptr, stream = _dev()
    from pose_adv_aug_amd.pylib import HumanAug
    fails, what = [], 'warp ' + name
    cs = warp_case(name)
    B, res = cs['params'].shape[0], cs['res']
    Hs, Ws = cs['frames'].shape[1:3]
    frames = torch.from_numpy(cs['frames']).cuda()
    sizes = torch.from_numpy(cs['sizes']).cuda() if cs['sizes'] is not None else None
    params = torch.from_numpy(cs['params']).cuda()
    _, tinv = HumanAug.affine_params(params, res, res)
    ref, d = warp_reference(name, tinv.cpu().numpy())
    bad = warp_conditions(cs, ref, d)
    if bad:
        fails.append((what, 'case conditions', bad))
    dt = _lib.act_dtype()

    def run(want4, wantf):
        o4 = Guarded((B, res, res, 4), dt, -3.0) if want4 else None
        of = Guarded((B, 3, res, res), torch.float32, -3.0) if wantf else None
        p4, pf = (ptr(o4.t) if o4 else None), (ptr(of.t) if of else None)
        if sizes is None:
            check(L.pa_affine_warp_bilinear(ptr(frames), Hs, Ws, ptr(tinv), ptr(params), B, res, p4, pf, stream()), 'pa_affine_warp_bilinear')
        else:
            check(L.pa_affine_warp_bilinear_sized(ptr(frames), Hs, Ws, ptr(sizes), ptr(tinv), ptr(params), B, res, p4, pf, stream()),
                  'pa_affine_warp_bilinear_sized')
        torch.cuda.synchronize()
        for o in (o4, of):
            if o is not None and not o.intact():
                fails.append((what, 'wrote outside an output', 0))
        return (o4.t.clone() if o4 else None), (of.t.clone() if of else None)

    out4, outf = run(True, True)
    only4, _ = run(True, False)
    _, onlyf = run(False, True)
    again4, againf = run(True, True)
    bits = lambda a, b: torch.equal(_bits(a), _bits(b))
    if not (bits(only4, out4) and bits(onlyf, outf)):
        fails.append((what, 'one output alone differs from the full call', 0))
    if not (bits(again4, out4) and bits(againf, outf)):
        fails.append((what, 'two calls on the same input differ', 0))
    got = outf.cpu().numpy()
    r = ratio(got, ref, warp_bound(ref, d))
    _note('warp outf ' + name, r)
    if not r <= 1.0:
        fails.append((what, 'outf outside the bound', r))
    n4 = out4_mismatches(out4, outf, dt)
    if n4:
        fails.append((what, 'out4 is not outf rounded to the storage type / a +0 fourth channel', n4))
    if name == 'sat' and not float((got == 1.0).mean()) > 0.1:
        fails.append((what, 'share of outputs that are exactly 1.0', float((got == 1.0).mean())))
    if name == 'out' and not bool((got[0] == 0).all()):
        fails.append((what, 'a window wholly outside its frame is not all zero', float(np.abs(got[0]).max())))
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('pylib_exact %s: B %d res %d, worst error / bound outf %.3g, max d %.3g, out4 mismatches %d' % (what, B, res, r, float(d.max()), n4))
    return fails


def affine_leg(log=print):
    """pa_affine_params at B 65 and four resolution pairs: t_out and tinv_in within the running bound, t(res) o tinv(res) the identity"""
    _lib, L, check, ptr, stream = _dev()
    fails = []
    p = affine_case()
    B = p.shape[0]
    params = torch.from_numpy(p).cuda()
    for res_in, res_out in AFFINE_RES:
        what = 'affine_params res_in %d res_out %d' % (res_in, res_out)
        t, ti = Guarded((B, 6), torch.float64, -777.25), Guarded((B, 6), torch.float64, -777.25)
        check(L.pa_affine_params(ptr(params), B, res_in, res_out, ptr(t.t), ptr(ti.t), stream()), 'pa_affine_params')
        torch.cuda.synchronize()
        if not (t.intact() and ti.intact()):
            fails.append((what, 'wrote outside an output', 0))
        rt, bt, ri, bi = affine_reference(p, res_in, res_out)
        r1, r2 = ratio(t.t.cpu().numpy(), rt, bt), ratio(ti.t.cpu().numpy(), ri, bi)
        _note('affine_params t_out', r1)
        _note('affine_params tinv_in', r2)
        if not (r1 <= 1.0 and r2 <= 1.0):
            fails.append((what, 't_out / tinv_in outside the bound', (r1, r2)))
        # the identity: both at ONE resolution
        t2, ti2 = torch.empty((B, 6), dtype=torch.float64, device='cuda'), torch.empty((B, 6), dtype=torch.float64, device='cuda')
        check(L.pa_affine_params(ptr(params), B, res_in, res_in, ptr(t2), ptr(ti2), stream()), 'pa_affine_params')
        th, tih = t2.cpu().numpy(), ti2.cpu().numpy()
        qt, qbt, qi, qbi = affine_reference(p, res_in, res_in)
        r3 = max(ratio(compose_exact(th[b], tih[b]), np.zeros(6), compose_bound(qt[b], qbt[b], qi[b], qbi[b])) for b in range(B))
        _note('affine_params t o tinv', r3)
        if not r3 <= 1.0:
            fails.append((what, 't o tinv is not the identity within the bound', r3))
        if os.environ.get('POSEADV_TEST_VERBOSE'):
            log('pylib_exact %s: worst error / bound t_out %.3g tinv_in %.3g identity %.3g' % (what, r1, r2, r3))
    return fails


def pts_leg(J, sized, log=print):
    """pa_transform_pts(_sized) at B 65: out within 4 u64 of the terms, exact zeros for invalid joints, pts_img bit-exact"""
    _lib, L, check, ptr, stream = _dev()
    from pose_adv_aug_amd.pylib import HumanAug
    fails, what = [], 'transform_pts J %d %s' % (J, 'sized' if sized else 'one width')
    cs = pts_case(J, sized)
    B = cs['B']
    params = torch.from_numpy(cs['params']).cuda()
    pts = torch.from_numpy(cs['pts']).cuda()
    t, _ = HumanAug.affine_params(params, 256, 64)
    out, img = Guarded((B, J, 2), torch.float64, -777.25), Guarded((B, J, 2), torch.float32, -777.25)
    if sized:
        sizes = torch.from_numpy(cs['sizes']).cuda()
        check(L.pa_transform_pts_sized(ptr(pts), ptr(params), ptr(t), B, J, ptr(sizes), ptr(out.t), ptr(img.t), stream()), 'pa_transform_pts_sized')
    else:
        check(L.pa_transform_pts(ptr(pts), ptr(params), ptr(t), B, J, cs['width'], ptr(out.t), ptr(img.t), stream()), 'pa_transform_pts')
    torch.cuda.synchronize()
    if not (out.intact() and img.intact()):
        fails.append((what, 'wrote outside an output', 0))
    ref, bound, rimg, invalid = pts_reference(cs, t.cpu().numpy())
    got = out.t.cpu().numpy()
    r = ratio(got, ref, bound)
    _note('transform_pts out', r)
    if not r <= 1.0:
        fails.append((what, 'out outside the bound', r))
    if not np.array_equal(img.t.cpu().numpy().view(np.int32), rimg.view(np.int32)):
        fails.append((what, 'pts_img differs in bits', 0))
    if not pts_planted_ok(cs, invalid):
        fails.append((what, 'the planted invalid joints are not the invalid ones of the reference', int(invalid.sum())))
    if not bool((got[invalid] == 0).all()):
        fails.append((what, 'an invalid joint is not exactly (0, 0)', 0))
    # without pts_img: the same bits
    out2 = torch.empty((B, J, 2), dtype=torch.float64, device='cuda')
    if sized:
        check(L.pa_transform_pts_sized(ptr(pts), ptr(params), ptr(t), B, J, ptr(sizes), ptr(out2), None, stream()), 'pa_transform_pts_sized')
    else:
        check(L.pa_transform_pts(ptr(pts), ptr(params), ptr(t), B, J, cs['width'], ptr(out2), None, stream()), 'pa_transform_pts')
    torch.cuda.synchronize()
    if not torch.equal(out2, out.t):
        fails.append((what, 'pts_img == NULL changes out', 0))
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('pylib_exact %s: worst error / bound %.3g, %d invalid joints' % (what, r, int(invalid.sum())))
    return fails


def heat_leg(H, Wd, J, log=print):
    _lib, L, check, ptr, stream = _dev()
    fails, what = [], 'gaussian_heatmap H %d W %d J %d' % (H, Wd, J)
    for k, p in enumerate(heat_batches(H, Wd, J)):
        B = p.shape[0]
        pts = torch.from_numpy(p).cuda()
        out = Guarded((B, J, H, Wd), torch.float32, -3.0)
        check(L.pa_gaussian_heatmap(ptr(pts), ptr(out.t), B, J, H, Wd, stream()), 'pa_gaussian_heatmap')
        torch.cuda.synchronize()
        if not out.intact():
            fails.append((what, 'wrote outside the output', k))
        bad = heat_mismatches(out.t.cpu().numpy(), p, H, Wd)
        if bad:
            fails.append((what, 'elements that differ from the oracle, batch %d' % k, bad))
    return fails


def l2_leg(n, log=print):
    """pa_weighted_l2 at one n: weight NULL / given, *loss from 0 / 1.5, within the bound; the sentinels exact"""
    _lib, L, check, ptr, stream = _dev()
    fails = []
    for weighted in (False, True):
        pred, gt, w = l2_case(n, weighted)
        dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
        dw = torch.from_numpy(w).cuda() if weighted else None
        for start in (0.0, 1.5):
            what = 'weighted_l2 n %d %s start %.1f' % (n, 'weighted' if weighted else 'unit', start)
            loss = Guarded((1,), torch.float32, start)
            check(L.pa_weighted_l2(ptr(dp), ptr(dg), ptr(dw), n, ptr(loss.t), stream()), 'pa_weighted_l2')
            torch.cuda.synchronize()
            if not loss.intact():
                fails.append((what, 'wrote outside the loss', 0))
            ref, bound = l2_reference(pred, gt, w, start)
            r = ratio(np.array([float(loss.t[0])]), np.array([ref]), np.array([bound]))
            _note('weighted_l2', r)
            if not r <= 1.0:
                fails.append((what, 'outside the bound', r))
            if os.environ.get('POSEADV_TEST_VERBOSE'):
                log('pylib_exact %s: error / bound %.3g (bound %.3g relative)' % (what, r, bound / abs(ref)))
    want = l2_sentinel_value(n)
    gt0 = torch.zeros(n, device='cuda')
    for e in l2_sentinels(n):
        pred = torch.zeros(n, device='cuda')
        pred[e] = 1.0
        w = torch.ones(n, device='cuda')
        w[e] = 3.0
        loss = torch.zeros(1, device='cuda')
        check(L.pa_weighted_l2(ptr(pred), ptr(gt0), ptr(w), n, ptr(loss), stream()), 'pa_weighted_l2')
        got = np.float32(loss.cpu().numpy()[0])
        if not l2_sentinel_ok(got, n):
            fails.append(('weighted_l2 n %d sentinel at %d' % (n, e), 'is not fl32(3 / n)', (float(got), float(want))))
    return fails


def flip_lr_leg(shape, log=print):
    _lib, L, check, ptr, stream = _dev()
    B, H, Wd = shape
    dt = _lib.act_dtype()
    x = torch.from_numpy(wide_floats(B * 1000 + H, (B, H, Wd, 4))).to(dt)
    src = x.cuda()
    dst = Guarded((B, H, Wd, 4), dt, -3.0)
    check(L.pa_flip_lr_nhwc4(ptr(src), ptr(dst.t), B, H, Wd, stream()), 'pa_flip_lr_nhwc4')
    torch.cuda.synchronize()
    fails = []
    if not dst.intact():
        fails.append(('flip_lr %s' % (shape,), 'wrote outside the output', 0))
    if not torch.equal(_bits(dst.t.cpu()), _bits(x.flip(2))):
        fails.append(('flip_lr %s' % (shape,), 'differs from x.flip(2) in bits', 0))
    if not torch.equal(_bits(src.cpu()), _bits(x)):
        fails.append(('flip_lr %s' % (shape,), 'the source changed', 0))
    return fails


def tta_leg(shape, log=print):
    _lib, L, check, ptr, stream = _dev()
    from oracle import pylib as opl
    B, J, H, Wd = shape
    a, b = torch.from_numpy(wide_floats(B * 7 + H, shape)), torch.from_numpy(wide_floats(B * 11 + H, shape))
    out, da, db = Guarded(shape, torch.float32, -3.0), a.cuda(), b.cuda()
    check(L.pa_flip_tta_merge(ptr(da), ptr(db), ptr(out.t), B, J, H, Wd, stream()), 'pa_flip_tta_merge')
    torch.cuda.synchronize()
    fails = []
    if not out.intact():
        fails.append(('flip_tta_merge %s' % (shape,), 'wrote outside the output', 0))
    want = (a + opl.flip_heatmaps(b)) / 2
    if not torch.equal(out.t.cpu().view(torch.int32), want.view(torch.int32)):
        fails.append(('flip_tta_merge %s' % (shape,), 'differs from (a + flip_heatmaps(b)) / 2 in bits', float((out.t.cpu() - want).abs().max())))
    return fails


def convert_leg(shape, log=print):
    """pa_nchw_to_nhwc == x.to(storage) permuted; pa_nhwc_to_nchw == storage -> float, permuted: both bit for bit"""
    _lib, L, check, ptr, stream = _dev()
    B, Cc, H, Wd = shape
    dt = _lib.act_dtype()
    fails, what = [], 'convert %s' % (shape,)
    x = torch.from_numpy(wide_floats(Cc * 13 + H, shape))
    dst, dx = Guarded((B, H, Wd, Cc), dt, -3.0), x.cuda()
    check(L.pa_nchw_to_nhwc(ptr(dx), ptr(dst.t), B, Cc, H, Wd, stream()), 'pa_nchw_to_nhwc')
    torch.cuda.synchronize()
    if not dst.intact():
        fails.append((what, 'pa_nchw_to_nhwc wrote outside the output', 0))
    want = x.to(dt).permute(0, 2, 3, 1).contiguous()
    if not torch.equal(_bits(dst.t.cpu()), _bits(want)):
        fails.append((what, 'pa_nchw_to_nhwc differs from x.to(storage) permuted', int((_bits(dst.t.cpu()) != _bits(want)).sum())))
    back, dwant = Guarded(shape, torch.float32, -3.0), want.cuda()
    check(L.pa_nhwc_to_nchw(ptr(dwant), ptr(back.t), B, Cc, H, Wd, stream()), 'pa_nhwc_to_nchw')
    torch.cuda.synchronize()
    if not back.intact():
        fails.append((what, 'pa_nhwc_to_nchw wrote outside the output', 0))
    wantf = want.float().permute(0, 3, 1, 2).contiguous()
    if not torch.equal(back.t.cpu().view(torch.int32), wantf.view(torch.int32)):
        fails.append((what, 'pa_nhwc_to_nchw differs from storage -> float permuted', 0))
    return fails


def refusal_leg(log=print):
    """refusals the CPU test has shown to return before any launch: the pre-filled outputs stay untouched"""
    _lib, L, check, ptr, stream = _dev()
    fails = []
    dt = _lib.act_dtype()
    cs = warp_case('b')
    B, res = 3, cs['res']
    frames, sizes, params = torch.from_numpy(cs['frames']).cuda(), torch.from_numpy(cs['sizes']).cuda(), torch.from_numpy(cs['params']).cuda()
    tinv = torch.zeros((B, 6), dtype=torch.float64, device='cuda')
    o4, of = Guarded((B, res, res, 4), dt, -3.0), Guarded((B, 3, res, res), torch.float32, -3.0)
    o64 = Guarded((B, 16, 2), torch.float64, -777.25)
    o32 = Guarded((B, 16, 2), torch.float32, -777.25)
    f = torch.zeros(B * 16 * 2, device='cuda')
    calls = (
        ('res must', lambda: L.pa_affine_warp_bilinear(ptr(frames), 48, 64, ptr(tinv), ptr(params), B, 0, ptr(o4.t), ptr(of.t), stream())),
        ('tinv is NULL', lambda: L.pa_affine_warp_bilinear(ptr(frames), 48, 64, None, ptr(params), B, res, ptr(o4.t), ptr(of.t), stream())),
        ('B must', lambda: L.pa_affine_warp_bilinear_sized(ptr(frames), 48, 64, ptr(sizes), ptr(tinv), ptr(params), 0, res, ptr(o4.t), ptr(of.t), stream())),
        ('sizes is NULL', lambda: L.pa_affine_warp_bilinear_sized(ptr(frames), 48, 64, None, ptr(tinv), ptr(params), B, res, ptr(o4.t), ptr(of.t), stream())),
        ('both NULL', lambda: L.pa_affine_warp_bilinear(ptr(frames), 48, 64, ptr(tinv), ptr(params), B, res, None, None, stream())),
        ('params is NULL', lambda: L.pa_affine_params(None, B, 64, 64, ptr(o64.t), ptr(o64.t), stream())),
        ('res_in must', lambda: L.pa_affine_params(ptr(params), B, 0, 64, ptr(o64.t), ptr(o64.t), stream())),
        ('J must', lambda: L.pa_transform_pts(ptr(f), ptr(params), ptr(tinv), B, 0, 1280.0, ptr(o64.t), ptr(o32.t), stream())),
        ('sizes is NULL', lambda: L.pa_transform_pts_sized(ptr(f), ptr(params), ptr(tinv), B, 16, None, ptr(o64.t), ptr(o32.t), stream())),
        ('pts is NULL', lambda: L.pa_gaussian_heatmap(None, ptr(of.t), B, 1, 4, 4, stream())),
        ('W must', lambda: L.pa_gaussian_heatmap(ptr(tinv), ptr(of.t), 1, 1, 4, 0, stream())),
        ('n must', lambda: L.pa_weighted_l2(ptr(f), ptr(f), None, 0, ptr(o32.t), stream())),
        ('gt is NULL', lambda: L.pa_weighted_l2(ptr(f), None, None, 4, ptr(o32.t), stream())),
        ('H must', lambda: L.pa_flip_lr_nhwc4(ptr(o4.t), ptr(o4.t), 1, 0, 4, stream())),
        ('J must be 16', lambda: L.pa_flip_tta_merge(ptr(f), ptr(f), ptr(of.t), 1, 5, 2, 2, stream())),
        ('out_flipped is NULL', lambda: L.pa_flip_tta_merge(ptr(f), None, ptr(of.t), 1, 16, 1, 1, stream())),
        ('C must', lambda: L.pa_nchw_to_nhwc(ptr(f), ptr(o4.t), 1, 0, 2, 2, stream())),
        ('src is NULL', lambda: L.pa_nhwc_to_nchw(None, ptr(of.t), 1, 4, 2, 2, stream())),
    )
    for word, call in calls:
        if call() == 0 or word.encode() not in L.pa_last_error():
            fails.append(('refusal', word, L.pa_last_error()))
    torch.cuda.synchronize()
    for nm, o in (('out4', o4), ('outf', of), ('float64 output', o64), ('fp32 output', o32)):
        if not o.untouched():
            fails.append(('refusal', 'a refused call wrote to ' + nm, 0))
    return fails


def all_legs(log=print):
    fails = []
    for name in WARP_CASES:
        fails += warp_leg(name, log)
    fails += affine_leg(log)
    for J, sized in ((16, False), (16, True), (5, False), (5, True)):
        fails += pts_leg(J, sized, log)
    for H, Wd in HEAT_SHAPES:
        for J in HEAT_JOINTS:
            fails += heat_leg(H, Wd, J, log)
    for n in L2_SIZES:
        fails += l2_leg(n, log)
    for s in FLIP_LR_SHAPES:
        fails += flip_lr_leg(s, log)
    for s in TTA_SHAPES:
        fails += tta_leg(s, log)
    for s in CONVERT_SHAPES:
        fails += convert_leg(s, log)
    fails += refusal_leg(log)
    return fails


if __name__ == '__main__':          # the half-precision leg: tests/test_gpu_pylib_exact.py runs this with POSEADV_DTYPE=fp16
    _log = lambda s: print(s, flush=True)
    from pose_adv_aug_amd._lib import lib as _l, DTYPE as _D
    _log('pylib_exact: the %s build (pa_dtype %d)' % (_D, _l().pa_dtype()))
    _fails = all_legs(_log)
    report(_log)
    print('FAILURES %d %s' % (len(_fails), _fails[:20]))
    print('PYLIB EXACT ' + ('PASSED' if not _fails else 'FAILED'), flush=True)
    sys.exit(1 if _fails else 0)
