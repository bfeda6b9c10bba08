"""The backward pass of the bilinear warp (csrc/warp_bwd.hip; pa_affine_warp_bilinear_bwd, pa_affine_params_bwd_host,
HumanAug.warp_batch_backward / warp_autograd, Augmenter.bilinear) against float64, element by element.

Reference.  warp_grad64(frames, sizes, tinv, params, dimg) restates the sampler per output pixel in numpy float64 -- sx = ti0 u + ti1 v + ti2,
sy likewise, the four taps around (floor sx, floor sy) (0 outside the sample's own frame, the frame mirrored when flip), S_c = sum w_k p_k,c / 255,
m_c = [0 <= g_c S_c <= 1] -- and forms, per pixel and channel, the terms
    dtinv: dimg_c m_c (g_c / 255) dS_c/dsx {u, v, 1},  dimg_c m_c (g_c / 255) dS_c/dsy {u, v, 1},      dgain_c: dimg_c m_c S_c
with dS_c/dsx = (1 - ay)(p01 - p00) + ay (p11 - p10) and dS_c/dsy = (1 - ax)(p10 - p00) + ax (p11 - p01) on the bytes.  Each output is the
exactly rounded sum (math.fsum) of its N = 3 res^2 terms.  tinv is an OPERAND: the GPU legs pass the device's own tinv, copied back, so
that only the kernel's arithmetic is judged and a last-bit difference in sin / cos cannot move a pixel into another cell.

Bound.  |got - ref| <= u64 (N + c) mag + u64 c_xy mag_xy + u64 |ref|, u64 = 2^-53.
  mag = the sum over the N terms of |term|, every factor by its absolute value, the fractions ax, ay taken as given:
  |dimg m k| ((1 - ay) |p01 - p00| + ay |p11 - p10|) {|u|, |v|, 1} and its mirror image for dtinv, |dimg m| S for dgain.
  N: the kernel adds the N terms of an output in some order in double: (N - 1) u64 mag.
  c = 8 + 8.  With the fractions given, one term of the kernel takes 8 double operations: a dgain term wx0 or wy0 (1), the tap weight
  (1), p / 255 (1), their product (1), the three additions of S (3), dimg m S (1); a dtinv term g / 255 (1), dimg m k (1), 1 - ay (1),
  two products and one addition of the slope (3), the product with it (1), the product with u or v (1).  The float64 reference forms
  the same term with its own 8 roundings; its sum is exactly rounded (the u64 |ref| term).  dimg (fp32) and the bytes enter exactly;
  byte differences are exact.
  The coordinates, apart from the sum: a fraction ay = sy - floor(sy) inherits the ABSOLUTE rounding error of sy -- two products, two
  additions and the subtraction, each at most u64 My with My = |ti3 u| + |ti4 v| + |ti5| + |floor sy| (Mx likewise) -- and a term moves
  by its absolute slope in the fraction times that.  mag_xy = the sum over the terms of that slope times Mx or My:
  |dimg m k| (|p01 - p00| + |p11 - p10|) My {|u|, |v|, 1} for the sx-derivative terms (they depend on ay only), the mirror image for the
  sy-derivative terms, |dimg m| (Mx ((1 - ay)(q00 + q01) + ay (q10 + q11)) + My ((1 - ax)(q00 + q10) + ax (q01 + q11))) for dgain
  (q = p / 255).  c_xy = 5 + 5: the five coordinate operations of the kernel and of the reference.  This is a per-term effect and is
  NOT multiplied by N.  (The kernel, compiled without multiply-add fusion, and numpy form sx, sy with the same operations in the same
  order, so on matching operands this part is not used up at all; it is there so that the bound does not rest on that.)  Products of
  two roundings (u64^2) are ignored.
  The mask is not a rounding matter: conditions() asserts that no pre-clamp value other than an exact 0 lies within 1e-9 of 0 or 1, and
  (outside the integer leg) that no coordinate lies within 1e-9 of an integer, so kernel and reference decide every cell and every
  mask alike.

dparams.  chain64 is the Jacobian of tinv(params) = [k cos th, k sin th, cx - k hr (cos th + sin th); -k sin th, k cos th,
cy - k hr (cos th - sin th)], k = 200 s / res, th = -rot pi / 180, hr = res / 2, written as a matrix J [8][9] on (dtinv, dgain).  The
bound of dparams_i is sum_j |J_ij| bound_j + 16 u64 sum_j |J_ij| |ref_j|: the device's sin / cos (a few u64 each), k, hr (cos +- sin) and
the six products and five additions of one row.

Cases.  (a) the forward test's case of tests/test_gpu_pylib.py (B 3, 90 x 120 frames, res 64, rotations 0 / 25 / -40, one flipped
sample, gains up to 1.4), with ONE change: its centres are integers, (60, 45), (50, 40), (70, 30), and the centre of the output,
pixel (32, 32), maps onto the centre of the crop for every scale and rotation (and, with rot 0 and scale 0.35, sx = 1.09375 u + 25 is
an integer at every u = 32 k): coordinates that are integers up to rounding, which conditions() forbids outside the integer leg.  The
centres are moved by a fraction of a pixel to (60.3, 45.2), (50.4, 40.3), (70.2, 30.6); frames, scales, rotations, flip and gains are
the forward test's.  (b) sized: padded [3][48][64] frames (padding bytes 200, which must never be read as pixels) with sizes (64, 48),
(40, 48), (64, 30), the narrow one flipped, res 20, one window reaching outside its frame.  (c) the integer leg: res 32, 40 x 40 frame,
centre (20, 20), scale 0.16, rot 0: tinv is exactly [1, 0, 4; 0, 1, 4], every fraction is 0 and the one-sided derivative convention
(the right-hand cell, the one the forward sampled) is what is under test.  (d) res 256, B 2: the workload's strip count."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))        # (run as a script by the fp16 leg)
from tests import inputs  # noqa: E402

U64 = 2.0 ** -53
C_OPS = 8 + 8
C_XY = 5 + 5
EDGE = 1e-9
CASES = ('a', 'b', 'c', 'd')


def case(name):
    """dict(frames uint8 [B][Hs][Ws][3], sizes int32 [B][2] or None, params float64 [B][8], res, dimg fp32 [B][3][res][res], integer)"""
    if name == 'a':
        g = inputs.rng(90)
        frames = g.integers(0, 256, size=(3, 90, 120, 3), dtype=np.uint8)
        c = [[60.3, 45.2], [50.4, 40.3], [70.2, 30.6]]
        s, r, flip = [0.35, 0.5, 0.28], [0.0, 25.0, -40.0], [0, 1, 0]
        gain = np.array([[1, 1, 1], [0.7, 1.3, 1.0], [1.4, 0.6, 1.2]], dtype=np.float32).astype(np.float64)
        sizes, res, seed = None, 64, 901
    elif name == 'b':
        g = inputs.rng(91)
        sizes = np.array([[64, 48], [40, 48], [64, 30]], dtype=np.int32)
        frames = np.full((3, 48, 64, 3), 200, dtype=np.uint8)
        for i, (w, h) in enumerate(sizes):
            frames[i, :h, :w] = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        c = [[31.7, 24.3], [19.4, 25.6], [50.2, 20.1]]
        s, r, flip = [0.21, 0.17, 0.3], [10.0, -15.0, 33.0], [0, 1, 0]
        gain = g.uniform(0.8, 1.2, size=(3, 3))
        res, seed = 20, 911
    elif name == 'c':
        g = inputs.rng(92)
        frames = g.integers(0, 255, size=(1, 40, 40, 3), dtype=np.uint8)        # (no byte 255: 1.0 * 255 / 255 would sit ON the clamp's bound)
        c, s, r, flip = [[20.0, 20.0]], [0.16], [0.0], [0]
        gain = np.array([[0.9, 1.0, 1.1]])
        sizes, res, seed = None, 32, 921
    elif name == 'd':
        g = inputs.rng(93)
        frames = g.integers(0, 256, size=(2, 90, 120, 3), dtype=np.uint8)
        c = [[60.3, 45.2], [55.1, 40.7]]
        s, r, flip = [0.4, 0.33], [17.0, -8.0], [0, 1]
        gain = g.uniform(0.7, 1.3, size=(2, 3))
        sizes, res, seed = None, 256, 931
    else:
        raise KeyError(name)
    B = frames.shape[0]
    p = np.zeros((B, 8))
    p[:, 0:2], p[:, 2], p[:, 3], p[:, 4], p[:, 5:8] = np.asarray(c), s, r, flip, gain
    dimg = inputs.rng(seed).standard_normal((B, 3, res, res)).astype(np.float32)
    return dict(name=name, frames=frames, sizes=sizes, params=p, res=res, dimg=dimg, integer=(name == 'c'))


def tinv64(params, res):
    """invert(get_transform) per sample with the CPU oracle: the operand of the CPU tests (the GPU legs use the device's own)"""
    from oracle import pylib as opl
    return np.stack([np.linalg.inv(opl.get_transform(p[0:2], p[2], p[3], res))[:2].reshape(6) for p in params])


def _sample(frames_b, wb, hb, ti, p, res):
    """the sampler's per-pixel quantities for one sample, [res][res] (v rows, u columns) and [4][res][res][3] taps (p00, p01, p10, p11)"""
    v, u = np.meshgrid(np.arange(res, dtype=np.float64), np.arange(res, dtype=np.float64), indexing='ij')
    sx = ti[0] * u + ti[1] * v + ti[2]
    sy = ti[3] * u + ti[4] * v + ti[5]
    fx0, fy0 = np.floor(sx), np.floor(sy)
    ax, ay = sx - fx0, sy - fy0
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    taps, oks = [], []
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < wb) & (yy >= 0) & (yy < hb)
            xs = (wb - 1 - xx) if p[4] != 0 else xx
            px = frames_b[np.clip(yy, 0, hb - 1), np.clip(xs, 0, wb - 1)].astype(np.float64)
            taps.append(np.where(ok[..., None], px, 0.0))
            oks.append(ok)
    Mx = np.abs(ti[0] * u) + np.abs(ti[1] * v) + abs(ti[2]) + np.abs(fx0)
    My = np.abs(ti[3] * u) + np.abs(ti[4] * v) + abs(ti[5]) + np.abs(fy0)
    return u, v, sx, sy, ax, ay, np.stack(taps), np.stack(oks), Mx, My


def _fsum(a):
    return math.fsum(a.reshape(-1).tolist())


def warp_grad64(frames, sizes, tinv, params, dimg):
    """-> dict: dtinv [B][6], dgain [B][3], mag_tinv [B][6], mag_gain [B][3] (the sums of absolute terms), xy_tinv, xy_gain (mag_xy of the
    module docstring: what a rounding of the coordinates moves), and the
    case statistics conditions() asserts: frac_dist (least distance of a coordinate from an integer), clamp_dist (least distance of a
    non-zero pre-clamp value from 0 and from 1), clamped (share of clamped channels), outside (share of taps outside the frame)"""
    frames, tinv, params = np.asarray(frames), np.asarray(tinv, dtype=np.float64), np.asarray(params, dtype=np.float64)
    dimg = np.asarray(dimg).astype(np.float64)
    B, res = dimg.shape[0], dimg.shape[2]
    out = dict(dtinv=np.zeros((B, 6)), dgain=np.zeros((B, 3)), mag_tinv=np.zeros((B, 6)), mag_gain=np.zeros((B, 3)),
               xy_tinv=np.zeros((B, 6)), xy_gain=np.zeros((B, 3)))
    frac_dist, clamp_dist, n_clamped, n_out, n_taps = np.inf, np.inf, 0, 0, 0
    for b in range(B):
        wb, hb = (int(sizes[b][0]), int(sizes[b][1])) if sizes is not None else (frames.shape[2], frames.shape[1])
        u, v, sx, sy, ax, ay, taps, oks, Mx, My = _sample(frames[b], wb, hb, tinv[b], params[b], res)
        p00, p01, p10, p11 = taps                                    # [res][res][3]
        g = params[b, 5:8]
        axc, ayc = ax[..., None], ay[..., None]
        wx0, wy0 = 1.0 - axc, 1.0 - ayc
        q = taps / 255.0
        S = (wx0 * wy0) * q[0]
        S = S + (axc * wy0) * q[1]
        S = S + (wx0 * ayc) * q[2]
        S = S + (axc * ayc) * q[3]
        pre = S * g
        m = ((pre >= 0.0) & (pre <= 1.0)).astype(np.float64)
        d = dimg[b].transpose(1, 2, 0) * m                          # [res][res][3], masked
        D = d * (g / 255.0)
        dxs = wy0 * (p01 - p00) + ayc * (p11 - p10)
        dys = wx0 * (p10 - p00) + axc * (p11 - p01)
        dxs_abs = wy0 * np.abs(p01 - p00) + ayc * np.abs(p11 - p10)
        dys_abs = wx0 * np.abs(p10 - p00) + axc * np.abs(p11 - p01)
        dxs_xy = My[..., None] * (np.abs(p01 - p00) + np.abs(p11 - p10))
        dys_xy = Mx[..., None] * (np.abs(p10 - p00) + np.abs(p11 - p01))
        for j, (slope, slope_abs, slope_xy, f) in enumerate(((dxs, dxs_abs, dxs_xy, u), (dxs, dxs_abs, dxs_xy, v), (dxs, dxs_abs, dxs_xy, None),
                                                             (dys, dys_abs, dys_xy, u), (dys, dys_abs, dys_xy, v), (dys, dys_abs, dys_xy, None))):
            fac = 1.0 if f is None else f[..., None]
            out['dtinv'][b, j] = _fsum(D * slope * fac)
            out['mag_tinv'][b, j] = float(np.sum(np.abs(D) * slope_abs * np.abs(fac)))
            out['xy_tinv'][b, j] = float(np.sum(np.abs(D) * slope_xy * np.abs(fac)))
        S_xy = Mx[..., None] * (wy0 * (q[0] + q[1]) + ayc * (q[2] + q[3])) + My[..., None] * (wx0 * (q[0] + q[2]) + axc * (q[1] + q[3]))
        for c in range(3):
            out['dgain'][b, c] = _fsum(d[..., c] * S[..., c])
            out['mag_gain'][b, c] = float(np.sum(np.abs(d[..., c]) * S[..., c]))
            out['xy_gain'][b, c] = float(np.sum(np.abs(d[..., c]) * S_xy[..., c]))
        for s_ in (sx, sy):
            frac_dist = min(frac_dist, float(np.min(np.abs(s_ - np.round(s_)))))
        nz = pre[pre != 0.0]
        if nz.size:
            clamp_dist = min(clamp_dist, float(np.min(np.abs(nz))), float(np.min(np.abs(nz - 1.0))))
        n_clamped += int((m == 0).sum())
        n_out += int((~oks).sum())
        n_taps += oks.size
    out.update(frac_dist=frac_dist, clamp_dist=clamp_dist, clamped=n_clamped / float(B * res * res * 3), outside=n_out / float(n_taps))
    return out


def bounds(ref, res):
    """(bound of dtinv [B][6], bound of dgain [B][3])"""
    n = 3 * res * res
    return (U64 * (n + C_OPS) * ref['mag_tinv'] + U64 * C_XY * ref['xy_tinv'] + U64 * np.abs(ref['dtinv']),
            U64 * (n + C_OPS) * ref['mag_gain'] + U64 * C_XY * ref['xy_gain'] + U64 * np.abs(ref['dgain']))


def jacobian(p, res):
    """J [8][9]: dparams = J (dtinv, dgain) for one sample's params"""
    k, hr, th = 200.0 * p[2] / res, res / 2.0, -p[3] * math.pi / 180.0
    sn, cs = math.sin(th), math.cos(th)
    dk = np.array([cs, sn, -hr * (cs + sn), -sn, cs, -hr * (cs - sn)])
    dth = k * np.array([-sn, cs, -hr * (cs - sn), -cs, -sn, hr * (cs + sn)])
    J = np.zeros((8, 9))
    J[0, 2] = 1.0
    J[1, 5] = 1.0
    J[2, :6] = dk * (200.0 / res)
    J[3, :6] = dth * (-math.pi / 180.0)
    J[5, 6] = J[6, 7] = J[7, 8] = 1.0
    return J


def chain64(params, dtinv, dgain, res):
    g9 = np.concatenate([dtinv, dgain], axis=1)
    return np.stack([jacobian(params[b], res).dot(g9[b]) for b in range(len(params))])


def dparams_bound(params, ref, res):
    bt, bg = bounds(ref, res)
    b9 = np.concatenate([bt, bg], axis=1)
    r9 = np.abs(np.concatenate([ref['dtinv'], ref['dgain']], axis=1))
    return np.stack([np.abs(jacobian(params[b], res)).dot(b9[b] + 16 * U64 * r9[b]) for b in range(len(params))])


def conditions(cs, ref):
    """the list of violated case conditions (empty = the case sits on no discontinuity and exercises what it is for)"""
    bad = []
    if cs['integer']:
        if ref['frac_dist'] != 0.0:
            bad.append('the integer leg has a non-integer coordinate')
    elif not ref['frac_dist'] > EDGE:
        bad.append('a coordinate within 1e-9 of an integer (%.3g)' % ref['frac_dist'])
    if not ref['clamp_dist'] > EDGE:
        bad.append('a pre-clamp value within 1e-9 of 0 or 1 (%.3g)' % ref['clamp_dist'])
    if cs['name'] == 'a' and not ref['clamped'] > 0:
        bad.append('the gain leg clamps nothing')
    if cs['name'] == 'b' and not ref['outside'] > 0:
        bad.append('the sized leg has no tap outside its frame')
    return bad


def sampler_torch(frames, sizes, tinv, gain, flip, res):
    """An independent torch float64 restatement of the sampler for autograd (gather with detached indices): tinv [B][6] and gain [B][3]
    may require grad.  -> [B][3][res][res]"""
    B = tinv.shape[0]
    fr = torch.from_numpy(np.asarray(frames).astype(np.int64)).double() / 255.0
    ar = torch.arange(res, dtype=torch.float64)
    v, u = torch.meshgrid(ar, ar, indexing='ij')
    outs = []
    for b in range(B):
        wb, hb = (int(sizes[b][0]), int(sizes[b][1])) if sizes is not None else (fr.shape[2], fr.shape[1])
        src = fr[b, :hb, :wb]
        if flip[b]:
            src = src.flip(1)
        src = torch.nn.functional.pad(src.permute(2, 0, 1), (1, 1, 1, 1))          # a zero border: index + 1
        sx = tinv[b, 0] * u + tinv[b, 1] * v + tinv[b, 2]
        sy = tinv[b, 3] * u + tinv[b, 4] * v + tinv[b, 5]
        x0, y0 = torch.floor(sx).detach(), torch.floor(sy).detach()
        ax, ay = sx - x0, sy - y0
        acc = 0
        for dy, wy in ((0, 1 - ay), (1, ay)):
            for dx, wx in ((0, 1 - ax), (1, ax)):
                xi = (x0.long() + dx + 1).clamp(0, wb + 1)
                yi = (y0.long() + dy + 1).clamp(0, hb + 1)
                acc = acc + (wx * wy) * src[:, yi, xi]
        outs.append(torch.clamp(acc * gain[b].view(3, 1, 1), 0.0, 1.0))
    return torch.stack(outs)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU legs (shared by tests/test_gpu_warp_grad.py and the fp16 child below)
SENTINEL = -777.25
PAD = 8                    # guard doubles around every output
WS_PAD = 64                # guard bytes around the workspace
_REF = {}


def reference(name, tinv):
    """warp_grad64 of a case with the device's tinv, computed once per (case, tinv bits) and shared"""
    key = (name, np.asarray(tinv).tobytes())
    if key not in _REF:
        cs = case(name)
        _REF[key] = warp_grad64(cs['frames'], cs['sizes'], tinv, cs['params'], cs['dimg'])
    return _REF[key]


def device_case(name):
    """the case's tensors on the device + the device's own tinv"""
    from pose_adv_aug_amd.pylib import HumanAug
    cs = case(name)
    frames = torch.from_numpy(cs['frames']).cuda()
    sizes = torch.from_numpy(cs['sizes']).cuda() if cs['sizes'] is not None else None
    params = torch.from_numpy(cs['params']).cuda()
    _, tinv = HumanAug.affine_params(params, cs['res'], cs['res'])
    return cs, frames, sizes, params, tinv


def dimg_layout(dimg, layout):
    """fp32 [B][3][res][res] on the device -> the buffer of `layout` (1: NHWC4 with a 4th float that must be ignored)"""
    if layout == 0:
        return dimg.contiguous()
    d4 = torch.full(dimg.shape[:1] + dimg.shape[2:] + (4,), 3.5e4, dtype=torch.float32, device=dimg.device)
    d4[..., :3] = dimg.permute(0, 2, 3, 1)
    return d4


def _ratio(got, ref, bound):
    return float(np.max(np.abs(got - ref) / np.maximum(bound, 1e-300)))


def operator_leg(name, layout, log=print):
    """pa_affine_warp_bilinear_bwd on a case: every element of dtinv, dgain and dparams within its bound; the guard doubles around the
    outputs and the guard bytes around the workspace untouched; a second call gives the same bits"""
    import ctypes as C
    from pose_adv_aug_amd._lib import check, lib, ptr, stream
    L, fails = lib(), []
    cs, frames, sizes, params, tinv = device_case(name)
    B, res = cs['params'].shape[0], cs['res']
    what = 'case %s layout %d' % (name, layout)
    tinv_host = tinv.cpu().numpy()
    if cs['integer'] and not np.array_equal(tinv_host, np.array([[1.0, 0.0, 4.0, 0.0, 1.0, 4.0]])):
        fails.append((what, 'tinv of the integer leg is not exactly [1, 0, 4; 0, 1, 4]', tinv_host.tolist()))
    ref = reference(name, tinv_host)
    bad = conditions(cs, ref)
    if bad:
        fails.append((what, 'case conditions', bad))
    dimg = dimg_layout(torch.from_numpy(cs['dimg']).cuda(), layout)
    nws = int(L.pa_affine_warp_bwd_workspace_bytes(B, res))
    Hs, Ws = cs['frames'].shape[1:3]

    def run():
        ws = torch.full((nws + 2 * WS_PAD,), 0xA5, dtype=torch.uint8, device='cuda')
        buf = torch.full((B * 17 + 4 * PAD,), SENTINEL, dtype=torch.float64, device='cuda')
        o_t, o_g, o_p = PAD, 2 * PAD + 6 * B, 3 * PAD + 9 * B
        at = lambda o: C.c_void_p(buf.data_ptr() + 8 * o)
        check(L.pa_affine_warp_bilinear_bwd(ptr(frames), Hs, Ws, ptr(sizes), ptr(tinv), ptr(params), B, res, ptr(dimg), layout,
                                            C.c_void_p(ws.data_ptr() + WS_PAD), at(o_t), at(o_g), at(o_p), stream()),
              'pa_affine_warp_bilinear_bwd')
        torch.cuda.synchronize()
        guards = torch.cat([buf[:o_t], buf[o_t + 6 * B:o_g], buf[o_g + 3 * B:o_p], buf[o_p + 8 * B:]])
        if guards.numel() != 4 * PAD or not bool((guards == SENTINEL).all()):
            fails.append((what, 'wrote outside an output', 0))
        if not (bool((ws[:WS_PAD] == 0xA5).all()) and bool((ws[WS_PAD + nws:] == 0xA5).all())):
            fails.append((what, 'wrote outside the workspace', 0))
        return buf[o_t:o_t + 6 * B].view(B, 6).clone(), buf[o_g:o_g + 3 * B].view(B, 3).clone(), buf[o_p:o_p + 8 * B].view(B, 8).clone()

    dt, dg, dp = run()
    dt2, dg2, dp2 = run()
    if not (torch.equal(dt, dt2) and torch.equal(dg, dg2) and torch.equal(dp, dp2)):
        fails.append((what, 'two calls on the same input differ', 0))
    bt, bg = bounds(ref, res)
    rt, rg = _ratio(dt.cpu().numpy(), ref['dtinv'], bt), _ratio(dg.cpu().numpy(), ref['dgain'], bg)
    rp = _ratio(dp.cpu().numpy(), chain64(cs['params'], ref['dtinv'], ref['dgain'], res), dparams_bound(cs['params'], ref, res))
    log('warp_grad %s: worst error / bound dtinv %.3g dgain %.3g dparams %.3g; clamped %.3g outside %.3g'
        % (what, rt, rg, rp, ref['clamped'], ref['outside']))
    for nm, r in (('dtinv', rt), ('dgain', rg), ('dparams', rp)):
        if not (r <= 1.0):
            fails.append((what, nm + ' outside the bound', r))
    if not (np.abs(ref['dtinv']).min() > 0 and np.abs(ref['dgain']).min() > 0):
        fails.append((what, 'a zero reference', 0))
    if bool((dp[:, 4] != 0).any()):
        fails.append((what, 'the flip column is not 0', 0))
    # the Python operator: the same bits
    from pose_adv_aug_amd.pylib import HumanAug
    pt, pg, pp = HumanAug.warp_batch_backward(frames, tinv, params, dimg, 'nhwc4' if layout else 'nchw', sizes=sizes)
    if not (torch.equal(pt, dt) and torch.equal(pg, dg) and torch.equal(pp, dp)):
        fails.append((what, 'warp_batch_backward differs from the C call', 0))
    return fails


def chain_leg(res=64, B=2, seed=95, log=print):
    """params.grad of loss(net(warp_autograd(frames, params))) == warp_batch_backward fed with a twin net's backward(input_grad=True), bit
    for bit; flat_grads of the two nets equal; the flip column 0; without requires_grad no backward launch"""
    from pose_adv_aug_amd.pylib import Criterion, HumanAug, HumanPts
    from tests.heat_grads_exact import make_net
    fails = []
    cs = case('d')
    frames = torch.from_numpy(cs['frames'][:B]).cuda()
    params = torch.from_numpy(cs['params'][:B]).cuda()
    pts = torch.from_numpy(inputs.heat_pts(seed + 1, B, res=res // 4)).cuda()
    T = HumanPts.pts2heatmap_batch(pts, res // 4, res // 4)
    net, twin = make_net(1, B, res, seed), make_net(1, B, res, seed)
    calls = []
    orig = HumanAug.warp_batch_backward
    HumanAug.warp_batch_backward = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        p = params.clone().requires_grad_()
        img = HumanAug.warp_autograd(frames, p, res=res)
        if img.grad_fn is None or img.dtype != torch.float32 or tuple(img.shape) != (B, 3, res, res):
            fails.append(('chain', 'warp_autograd output', (img.dtype, tuple(img.shape))))
        loss = sum(Criterion.weighted_L2(o, T, 1) for o in net.forward_autograd(x=img))
        loss.backward()
        torch.cuda.synchronize()
        if calls != [1]:
            fails.append(('chain', 'backward launches with requires_grad', len(calls)))
        # the twin: the same pixels, the heat gradients autograd delivers, the image gradient by hand, the operator by hand
        _, tinv = HumanAug.affine_params(params, res, res)
        _, outf = HumanAug.warp_batch(frames, tinv, params, res=res, want_nchw=True, want_nhwc4=False)
        if not torch.equal(outf, img.detach()):
            fails.append(('chain', 'warp_autograd pixels differ from warp_batch', 0))
        o2 = [o.detach().requires_grad_() for o in twin(outf)]
        gs = torch.autograd.grad(sum(Criterion.weighted_L2(o, T, 1) for o in o2), o2)
        d = twin.backward(list(gs), input_grad=True)
        _, _, dp = orig(frames, tinv, params, d, 'nchw')
        torch.cuda.synchronize()
        if p.grad is None or p.grad.dtype != torch.float64 or tuple(p.grad.shape) != (B, 8):
            fails.append(('chain', 'params.grad', None))
        else:
            if not (torch.equal(p.grad, dp) and float(dp[:, :4].abs().min()) > 0 and bool(torch.isfinite(dp).all())):
                fails.append(('chain', 'params.grad differs from the hand-made chain', float((p.grad - dp).abs().max())))
            if bool((p.grad[:, 4] != 0).any()):
                fails.append(('chain', 'the flip column is not 0', 0))
        if not torch.equal(net.flat_grads, twin.flat_grads):
            fails.append(('chain', 'flat_grads of the twins differ', 0))
        log('warp_grad chain: d loss / d (scale, rot) = %s' % p.grad[:, 2:4].tolist())
        # without requires_grad: warp_batch and nothing else
        del calls[:]
        img2 = HumanAug.warp_autograd(frames, params.clone(), res=res)
        if img2.grad_fn is not None or not torch.equal(img2, outf):
            fails.append(('chain', 'warp_autograd without requires_grad', 0))
        sum(Criterion.weighted_L2(o, T, 1) for o in net.forward_autograd(x=img2)).backward()
        torch.cuda.synchronize()
        if calls:
            fails.append(('chain', 'a backward launch without requires_grad', len(calls)))
        if not torch.equal(net.flat_grads, twin.flat_grads):
            fails.append(('chain', 'flat_grads without requires_grad', 0))
    finally:
        HumanAug.warp_batch_backward = orig
    return fails


if __name__ == '__main__':          # the fp16 legs: tests/test_gpu_warp_grad.py runs this with POSEADV_DTYPE=fp16
    from pose_adv_aug_amd._lib import lib as _l
    assert _l().pa_dtype() == 1, 'run with POSEADV_DTYPE=fp16'
    _log = lambda s: print(s, flush=True)
    fails = []
    for _lay in (0, 1):
        fails += operator_leg('a', _lay, _log)
    fails += chain_leg(log=_log)
    print('FAILURES %d %s' % (len(fails), fails[:20]))
    print('FP16 WARP GRAD ' + ('PASSED' if not fails else 'FAILED'), flush=True)
    sys.exit(1 if fails else 0)
