"""The device half of the JPEG decode (pa_jpeg_decode: dequantise + inverse DCT + range limit, then chroma upsampling + colour
conversion + padding) and the feed built on it (MPII.batches(decoder='device')).  Every expected pixel is Pillow's
Image.open(f).convert('RGB') of a file written at test time; the second reference, tests/jpeg_exact.py on the same coefficients,
tells a kernel fault from an entropy-stage fault."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import jpeg_exact
from tests.jpeg_files import encode, picture, pillow_rgb, host_decode

pytestmark = pytest.mark.gpu


def _pack(files):
    """host stage of a batch: -> (coef int16 [n], descs uint8 [B * DESC_BYTES], coef_base int64 [B], [desc], [coef view])"""
    from pose_adv_aug_amd.pylib import Jpeg
    decoded = []
    for data in files:
        if data is None:                                     # an entry the device is to leave alone (ncomp == 0)
            decoded.append((Jpeg.JpegDesc(), np.zeros(0, dtype=np.int16)))
            continue
        rc, desc, coef = host_decode(data)
        assert rc == 0, Jpeg.last_error()
        decoded.append((desc, coef))
    base = np.concatenate([[0], np.cumsum([c.size for _, c in decoded])]).astype(np.int64)
    coef = np.concatenate([c for _, c in decoded] + [np.zeros(64, dtype=np.int16)])
    descs = np.frombuffer(b''.join(bytes(d) for d, _ in decoded), dtype=np.uint8).copy()
    return coef, descs, base[:-1].copy(), [d for d, _ in decoded], [c for _, c in decoded]


def _decode_and_check(files, Hs=None, Ws=None):
    from pose_adv_aug_amd.pylib import Jpeg
    coef, descs, base, dl, cl = _pack(files)
    want = [pillow_rgb(f) for f in files]
    Hs = Hs or max(a.shape[0] for a in want)
    Ws = Ws or max(a.shape[1] for a in want)
    frames, sizes = Jpeg.jpeg_decode_batch(torch.from_numpy(coef).cuda(), torch.from_numpy(descs).cuda(), torch.from_numpy(base).cuda(), Hs, Ws)
    torch.cuda.synchronize()
    frames, sizes = frames.cpu().numpy(), sizes.cpu().numpy()
    assert frames.shape == (len(files), Hs, Ws, 3)
    for b, a in enumerate(want):
        h, w = a.shape[:2]
        assert tuple(sizes[b]) == (w, h), b
        restated = jpeg_exact.decode_rgb(cl[b], dl[b])
        assert np.array_equal(frames[b, :h, :w], restated), ('kernels differ from the restated arithmetic', b, w, h)
        assert np.array_equal(frames[b, :h, :w], a), ('differs from Pillow', b, w, h)
        assert not frames[b, h:].any() and not frames[b, :, w:].any(), ('padding is not zero', b)
    return frames, sizes


def test_mixed_batch_equals_pillow_byte_for_byte():
    """B = 12: the seven sizes and the four samplings mixed, a restart-interval file, a quality-100 noise file; Hs, Ws = the maxima"""
    specs = [((83, 61), 'smooth', 2, 90, False, 0), ((17, 33), 'noise', 1, 75, False, 0), ((33, 18), 'checker', 0, 90, False, 0),
             ((130, 95), 'smooth', 'gray', 80, True, 0), ((16, 16), 'noise', 2, 100, False, 0), ((9, 7), 'smooth', 2, 90, False, 0),
             ((64, 48), 'checker', 1, 35, True, 0), ((130, 95), 'noise', 2, 75, False, 3), ((83, 61), 'checker', 0, 95, False, 1),
             ((17, 33), 'smooth', 'gray', 60, False, 2), ((33, 18), 'noise', 1, 100, False, 0), ((9, 7), 'checker', 0, 50, False, 0)]
    files = [encode(picture(content, w, h, seed=k), sampling, q, opt, rst) for k, ((w, h), content, sampling, q, opt, rst) in enumerate(specs)]
    assert len(files) == 12
    _decode_and_check(files)


def test_frames_wider_and_taller_than_one_workgroup_tile():
    """Stage (b) gives a workgroup 128 threads x 4 pixels = 512 pixels of one frame row: 520 x 40 puts pixels 512 .. 519 (and the
    chroma samples 255 / 256 on either side of that boundary) into a second workgroup, and Ws = 520 is not a multiple of that span.
    Stage (a) gives a workgroup 32 consecutive blocks of the image's block list (luma, then Cb, then Cr, each in raster order):
    520 x 40 at 4:2:0 has 66 x 6 luma blocks and 33 x 3 per chroma plane, so workgroup boundaries fall inside block rows (32 does
    not divide 66 or 33) and both component boundaries (block 396 and 495) fall inside a workgroup; 40 x 264 has 6 x 34 luma blocks,
    so one workgroup spans more than five block rows, and its 264 frame rows are 264 workgroups of stage (b) (grid.y = row)."""
    files = [encode(picture('noise', 520, 40, seed=5), 2, 85), encode(picture('smooth', 40, 264, seed=6), 2, 92)]
    _decode_and_check(files)


def test_decode_stays_inside_workspace_frames_and_sizes():
    """Guard regions in front of and behind the workspace, the frames and the sizes stay intact with Hs, Ws larger than every image;
    an ncomp == 0 entry gets an all-zero frame (the decode writes the padding itself: the frames start out as 0xCD) and its sizes
    row is not touched."""
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    files = [encode(picture('noise', 83, 61, seed=1), 2, 90), None, encode(picture('smooth', 130, 95, seed=2), 1, 80),
             encode(picture('checker', 33, 18, seed=3), 'gray', 70)]
    coef, descs, base, dl, cl = _pack(files)
    B, Hs, Ws = len(files), 101, 141
    L = lib()
    G = 4 << 20

    def guarded(nbytes, fill):
        big = torch.full((nbytes + 2 * G,), 0x5A, dtype=torch.uint8, device='cuda')
        big[G:G + nbytes] = fill
        return big
    nws = L.pa_jpeg_workspace_bytes(B, Hs, Ws)
    assert nws > 0
    ws, fr, sz = guarded(nws, 0xEE), guarded(B * Hs * Ws * 3, 0xCD), guarded(B * 8, 0xF9)
    dcoef, ddesc, dbase = torch.from_numpy(coef).cuda(), torch.from_numpy(descs).cuda(), torch.from_numpy(base).cuda()
    check(L.pa_jpeg_decode(ptr(dcoef), ptr(ddesc), ptr(dbase), B, Hs, Ws, C.c_void_p(ws.data_ptr() + G), C.c_void_p(fr.data_ptr() + G),
                           C.c_void_p(sz.data_ptr() + G), stream()), 'pa_jpeg_decode')
    torch.cuda.synchronize()
    for big, n in ((ws, nws), (fr, B * Hs * Ws * 3), (sz, B * 8)):
        assert bool((big[:G] == 0x5A).all()) and bool((big[G + n:] == 0x5A).all())
    frames = fr[G:G + B * Hs * Ws * 3].cpu().numpy().reshape(B, Hs, Ws, 3)
    sizes = sz[G:G + B * 8].cpu().numpy().view(np.int32).reshape(B, 2)
    for b, data in enumerate(files):
        if data is None:
            assert not frames[b].any() and sizes[b].tobytes() == b'\xf9' * 8
            continue
        a = pillow_rgb(data)
        h, w = a.shape[:2]
        assert tuple(sizes[b]) == (w, h) and np.array_equal(frames[b, :h, :w], a)
        assert not frames[b, h:].any() and not frames[b, :, w:].any()
    # the host side of the call refuses what it can see
    for bad in ((0, Hs, Ws), (B, 0, Ws), (B, Hs, -1)):
        assert L.pa_jpeg_decode(ptr(dcoef), ptr(ddesc), ptr(dbase), bad[0], bad[1], bad[2], C.c_void_p(ws.data_ptr() + G),
                                C.c_void_p(fr.data_ptr() + G), C.c_void_p(sz.data_ptr() + G), stream()) != 0
    assert L.pa_jpeg_decode(ptr(dcoef), ptr(ddesc), ptr(dbase), B, Hs, Ws, None, C.c_void_p(fr.data_ptr() + G),
                            C.c_void_p(sz.data_ptr() + G), stream()) != 0


def _jpeg_dataset(tmp_path):
    g = np.random.default_rng(41)
    sizes = [(320, 240), (200, 260), (256, 256)]
    anno = []
    for i in range(12):
        w, h = sizes[i % 3]
        arr = picture(('smooth', 'noise', 'checker')[i % 3], w, h, seed=i)
        kw = dict(progressive=True) if i == 5 else {}
        (tmp_path / ('im%d.jpg' % i)).write_bytes(encode(arr, (2, 1, 0, 'gray')[i % 4], 70 + 2 * i, i % 2 == 1, 4 if i == 7 else 0, **kw))
        joints = np.concatenate([g.uniform(5, [w - 5, h - 5], (16, 2)), np.ones((16, 1))], 1)
        anno.append({'dataset': 'MPII', 'isValidation': 0.0, 'img_paths': 'im%d.jpg' % i, 'joint_self': joints.tolist(),
                     'objpos': [w / 2.0 + float(g.uniform(-10, 10)), h / 2.0 + float(g.uniform(-10, 10))],
                     'scale_provided': float(g.uniform(0.8, 1.4)), 'normalizer': float(g.uniform(40, 90))})
    path = tmp_path / 'anno.json'
    path.write_text(json.dumps(anno))
    return str(path)


def test_device_feed_equals_thread_feed_and_trains_to_the_same_losses(tmp_path):
    """12 JPEG files of three sizes, one of them progressive (the per-image PIL fallback): decoder='device' yields the batches of
    decoder='thread' exactly -- whole padded frames, sizes, meta, joints, normalizer -- names itself (an unknown decoder value
    selects the thread path, so equality alone would prove nothing), counts one fallback, and two stack_hg training steps driven by
    either feed give the same losses and the same parameters, bit for bit.

    The loss compared bit for bit is the heat-map MSE of stack-hg.py:156-159 evaluated from the step's own heat maps and target in
    float64 on the host.  The engine's loss SCALAR cannot serve: head_fwd_kernel (csrc/pose_ops.hip) adds one partial sum per
    workgroup into it with a float atomicAdd, n = ceil(B * 64 * 64 / 64) = 384 of them here, in arrival order, so that two runs over
    the SAME feed differ in its last bits (measured: 0.054371533915 against 0.054371528327 for the mean of the two steps, 1e-7
    relative).  Any two orders of n non-negative fp32 additions lie within 2 (n - 1) 2^-24 of each other relatively; the scalar
    is held to that, 4.6e-5."""
    from pose_adv_aug_amd.mpii_for_mpii import MPII
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    from pose_adv_aug_amd.utils.optim import RMSprop
    from pose_adv_aug_amd.data import Augmenter
    from pose_adv_aug_amd.pylib import HumanPts
    from pose_adv_aug_amd import stack_hg
    path = _jpeg_dataset(tmp_path)
    ds = MPII(path, str(tmp_path), is_train=True, log=lambda *_: None)
    ft = ds.batches(4, shuffle=False, decoder='thread')
    fd = ds.batches(4, shuffle=False, decoder='device', workers=3, prefetch=2)
    assert fd.decoder == 'device' and ft.decoder == 'thread' and len(fd) == len(ft) == 3 and fd.num_samples == 12
    n = 0
    for a, b in zip(ft, fd):
        assert a.index == b.index and torch.equal(a.sizes, b.sizes) and torch.equal(a.meta, b.meta)
        assert torch.equal(a.joints, b.joints) and torch.equal(a.normalizer, b.normalizer)
        assert a.frames.shape == b.frames.shape and torch.equal(a.frames, b.frames), a.index
        n += 1
    assert n == 3 and fd.fallbacks == 1

    def two_steps(decoder):
        net = create_hg(1, 1, 16, 128, default_batch=6)
        net.reset_parameters(seed=0)
        net.train()
        opt = RMSprop(net, lr=2.5e-4)
        aug = Augmenter(seed=1)
        feed = ds.batches(6, shuffle=False, decoder=decoder, workers=3, prefetch=2)
        assert len(feed) == 2 and feed.decoder == decoder
        scalars, exact = [], []
        for batch in feed:
            if batch.ready is not None:
                torch.cuda.current_stream().wait_event(batch.ready)
            data = aug.regular(batch)
            loss, _, _ = stack_hg.train_step(net, opt, aug, batch, data=data)
            heat = net.heatmaps(batch.B)[-1].double().cpu().numpy()
            target = HumanPts.pts2heatmap_batch(data['pts'], 64, 64).double().cpu().numpy()
            scalars.append(float(loss))
            exact.append(float(np.mean((heat - target) ** 2)))
        torch.cuda.synchronize()
        return scalars, exact, net.flat_params.clone()
    st, et, wt = two_steps('thread')
    sd, ed, wd = two_steps('device')
    print('loss scalars', st, sd, 'float64 losses', et, ed)
    assert len(et) == 2 and all(np.isfinite(et)) and et == ed
    assert torch.equal(wt, wd)
    bound = 2 * (384 - 1) * 2.0 ** -24
    for a, b in zip(st, sd):
        assert abs(a - b) <= bound * max(a, b)


def test_device_feed_with_six_assemblers_sharing_the_decode_stream(tmp_path):
    """Six assembler threads enqueue their decodes on the one copy stream; each call owns the workspace between its two launches,
    so a launch of another thread landing between them cannot swap the planes.  36 single-image batches of three geometries,
    two passes: every frame equals Pillow."""
    from pose_adv_aug_amd.mpii_for_mpii import MPII
    path = _jpeg_dataset(tmp_path)
    ds = MPII(path, str(tmp_path), is_train=True, log=lambda *_: None)
    want = [pillow_rgb((tmp_path / ('im%d.jpg' % i)).read_bytes()) for i in range(12)]
    feed = ds.batches(1, shuffle=False, decoder='device', workers=4, prefetch=6)
    for _ in range(2):
        got = [(b.index[0], b.frames[0].cpu().numpy(), tuple(b.sizes[0].tolist())) for b in feed]
        assert [i for i, _, _ in got] == list(range(12))
        for i, fr, (w, h) in got:
            assert (h, w) == want[i].shape[:2] and np.array_equal(fr[:h, :w], want[i]), i
