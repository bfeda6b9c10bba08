"""The arg-max / final_preds kernels and the in-engine PCK / PCKh (pa_hg_accuracy, pa_hg_pckh) against oracle.pylib, coordinate by
coordinate, on the inputs of tests/metrics_cases.py (whose properties tests/test_metrics_cases_cpu.py asserts without a GPU).

A coordinate is an integer: `preds`, `maxval` and the back-projected final predictions are compared with np.array_equal; PCK
values are ratios of integers below 100 and are compared to 1e-6 (float32 division on both sides; the tolerance
tests/test_gpu_pylib.py::test_metric_edge_cases_against_oracle uses for the same quantities).

pa_get_preds_nhwc / pa_final_preds_nhwc read joint-minor maps [B][H*W][J] with the strides the engine uses on its own heat maps:
J = 16 at a 16-byte-aligned pointer is argmax_nhwc16_kernel (one 1024-thread workgroup per sample), anything else the generic
argmax_kernel (256 threads per map) with a stride of J floats."""
import numpy as np
import pytest
import torch

from oracle import pylib as opl
from tests import inputs
from tests import metrics_cases as mc

pytestmark = pytest.mark.gpu


def _run(maps_dev, B, J, H, W, meta, joint_minor):
    """(preds, maxval, final_preds) of the library on device maps in either layout"""
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    c, s, r = meta
    L = lib()
    get, fin = (L.pa_get_preds_nhwc, L.pa_final_preds_nhwc) if joint_minor else (L.pa_get_preds, L.pa_final_preds)
    preds = torch.full((B, J, 2), -7.0, device='cuda')
    maxval = torch.full((B, J), -7.0, device='cuda')
    out = torch.full((B, J, 2), -7.0, device='cuda')
    tmp = torch.empty((B, J, 2), device='cuda')
    check(get(ptr(maps_dev), B, J, H, W, ptr(preds), ptr(maxval), stream()), 'get_preds')
    check(fin(ptr(maps_dev), ptr(c[:B].contiguous()), ptr(s[:B].contiguous()), ptr(r[:B].contiguous()), B, J, H, W, ptr(out), ptr(tmp),
              stream()), 'final_preds')
    return preds.cpu().numpy(), maxval.cpu().numpy(), out.cpu().numpy(), tmp.cpu().numpy()


def _check_sets(H, W, J, split, joint_minor, offset=0):
    """every case of the three sets at one size, B = 5 and B = 1 (the first sample), against the oracle.  offset: the maps start
    that many floats into a larger allocation."""
    (c, s, _, r), _ = mc.meta_tensors(H, W, J)
    meta = (c.cuda(), s.reshape(-1).cuda(), r.reshape(-1).cuda())
    failed = []
    for name, maps in mc.case_sets(H, W, J, split).items():
        want = mc.oracle_points(H, W, J, split, name)
        for B in (mc.B, 1):
            host = mc.nhwc(maps[:B]) if joint_minor else np.ascontiguousarray(maps[:B])
            buf = torch.full((host.size + 8,), float('nan'), device='cuda')
            dev = buf[offset:offset + host.size]
            dev.copy_(mc.t(host).reshape(-1))
            assert (dev.data_ptr() % 16 == 0) == (offset % 4 == 0)
            preds, maxval, final, tmp = _run(dev, B, J, H, W, meta, joint_minor)
            for what, got, ref in (('preds', preds, want[0][:B]), ('maxval', maxval, want[1][:B]), ('final_preds', final, want[2][:B]),
                                   ('final_preds scratch', tmp, want[0][:B])):
                if not np.array_equal(got, ref):
                    bad = np.argwhere((got != ref).reshape(B, J, -1).any(-1))
                    failed.append('%s B=%d %s: %d of %d maps differ, first (b, j) = %s: got %s, oracle %s'
                                  % (name, B, what, len(bad), B * J, bad[0].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])]))
    assert not failed, '\n'.join(['%d x %d, J = %d:' % (H, W, J)] + failed)


@pytest.mark.parametrize('H,W', mc.NHWC_SIZES)
def test_joint_minor_argmax_and_final_preds_are_exact(H, W):
    """argmax_nhwc16_kernel + the strided final_preds_kernel, standalone: 16 x 16 (whole waves without a pixel), 32 x 32 (one pixel
    per thread), 48 x 48 (a partly filled slot), 64 x 64 (the workload), 80 x 80 (a second, partly filled trip), 96 x 96 (three
    trips) and two non-square maps, where the expectation is the reference's y = floor(p / H) + 1."""
    _check_sets(H, W, 16, mc.NHWC_SPLIT, True)


@pytest.mark.parametrize('H,W', mc.NHWC_SIZES)
def test_joint_minor_maps_four_floats_into_an_allocation(H, W):
    """the same kernel at a base that is 16-byte aligned but not an allocation's start (a stack's heat maps inside the workspace)"""
    _check_sets(H, W, 16, mc.NHWC_SPLIT, True, offset=4)


@pytest.mark.parametrize('H,W', mc.NHWC_SIZES)
def test_unaligned_joint_minor_maps_take_the_generic_kernel(H, W):
    """one float into an allocation the 16-byte loads are not possible: pa_launch_argmax falls back to the generic kernel with a
    stride of 16 floats (the tie cases are laid out for its 256 threads x 8 loads)"""
    _check_sets(H, W, 16, mc.NCHW_SPLIT, True, offset=1)


@pytest.mark.parametrize('J', [1, 3, 17])
@pytest.mark.parametrize('H,W', mc.NHWC_SIZES)
def test_joint_minor_maps_of_other_joint_counts(H, W, J):
    _check_sets(H, W, J, mc.NCHW_SPLIT, True)


@pytest.mark.parametrize('J', [1, 16, 17])
@pytest.mark.parametrize('H,W', mc.NCHW_SIZES)
def test_joint_major_argmax_and_final_preds_are_exact(H, W, J):
    """pa_get_preds / pa_final_preds (argmax_kernel, one 256-thread workgroup per map) below one pixel per thread (5 x 7, 8 x 8),
    at exactly one (16 x 16), with a ragged second trip (48 x 64 = 1.5 trips of 2048), with more than two (96 x 96) and on
    non-square maps: the oracle's y = floor(p / H) + 1 and its guard 1 < px < W, 1 < py < H are the expectation."""
    _check_sets(H, W, J, mc.NCHW_SPLIT, False)


# ------------------------------------------------------------------------------------------------ in the net
IDX = list(range(16))


def _net(res):
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    net = create_hg(1, 1, 16, 128, res=res, default_batch=mc.B)
    net.reset_parameters(seed=res)
    return net


def _write_heat(net, maps):
    """overwrite the last stack's heat maps [B][H*W][16] in place: pa_hg_heatmap_nhwc points into the workspace tensor the
    Python layer owns, so a view of that tensor at the pointer's offset is the engine's buffer"""
    from pose_adv_aug_amd._lib import lib
    h, ws = net._nets[mc.B]
    p = lib().pa_hg_heatmap_nhwc(h, net.num_stacks - 1)
    off, n = p - ws.data_ptr(), maps.size * 4
    assert off >= 0 and off % 16 == 0 and off + n <= ws.numel()
    ws[off:off + n].view(torch.float32).copy_(mc.t(mc.nhwc(maps)).reshape(-1))


def _metrics(net, H, seed):
    (c, s, _, r), (gpts, norm) = mc.meta_tensors(H, H, 16, seed)
    acc = net.accuracy(IDX)
    pckh, person = net.pckh_origin_res(c.cuda(), s.reshape(-1).cuda(), r.reshape(-1).cuda(), gpts.cuda(), norm.cuda(), per_person=True)
    return acc, pckh, person


def _oracle(H, variant):
    seed = None if variant == 0 else 500 + H + 1000 * variant
    maps, tgt, tp = mc.realistic(H, variant=variant)
    (c, s, res, r), (gpts, norm) = mc.meta_tensors(H, H, 16, seed)
    o = mc.t(maps)
    return (maps, tp, seed, opl.accuracy(o, mc.t(tgt), IDX).numpy(), opl.accuracy_origin_res(o, c, s, res, gpts, norm, r).numpy(),
            opl.per_person_pckh(o, mc.t(tgt), c, s, res, gpts, norm, r).numpy())


def _assert_metrics(got, want, what):
    acc, pckh, person = (g.cpu().numpy() for g in got)
    print('%s: heat-map accuracy %s (oracle mean %.4f), PCKh mean %.4f (oracle %.4f), per person %s' %
          (what, acc[0], want[3][0], pckh[0], want[4][0], person))
    assert np.allclose(acc, want[3], rtol=0, atol=1e-6), (what, acc, want[3])
    assert np.allclose(pckh, want[4], rtol=0, atol=1e-6), (what, pckh, want[4])
    assert np.allclose(person, want[5], rtol=0, atol=1e-6), (what, person, want[5])
    assert acc[0] > 0.5, (what, acc)              # never again 0 == 0


@pytest.mark.parametrize('res', [128, 192, 256, 320, 384])
def test_in_engine_metrics_on_chosen_heat_maps(res):
    """pa_hg_accuracy / pa_hg_pckh on heat maps written over the engine's own after an eval-mode forward pass: the values of the
    oracle on those maps; the same bits from the meter stream (pa_net_meters_async, joined by the next forward pass); and after
    a further forward pass with other joints and other maps the oracle's values on THOSE (the arg-max cached per forward pass,
    heat_peak_valid, must not survive a forward pass)."""
    from pose_adv_aug_amd._lib import lib, check
    H = res // 4
    net = _net(res)
    net.eval()
    img = mc.t(inputs.images(res, mc.B, res)).cuda()
    first, second = _oracle(H, 0), _oracle(H, 1)
    assert not np.array_equal(first[3], second[3]) and not np.array_equal(first[4], second[4])

    def forward(o):
        net(img, pts=mc.t(o[1]).cuda())
        _write_heat(net, o[0])

    forward(first)
    plain = _metrics(net, H, first[2])
    _assert_metrics(plain, first, 'res %d' % res)
    again = _metrics(net, H, first[2])              # the cached peaks
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    # on the meter stream, beside whatever the net's stream is given next; the next forward pass joins them
    forward(first)
    h = net._net(mc.B)
    net._meter_keep = []                            # (what loss_and_backward(after_forward=...) does: the meters' buffers stay alive until the join)
    check(lib().pa_net_meters_async(h, 1), 'pa_net_meters_async')
    try:
        beside = _metrics(net, H, first[2])
    finally:
        check(lib().pa_net_meters_async(h, 0), 'pa_net_meters_async')
    forward(second)
    net._meter_keep = None
    assert all(torch.equal(a, b) for a, b in zip(plain, beside)), (plain, beside)
    _assert_metrics(_metrics(net, H, second[2]), second, 'res %d, second forward pass' % res)


def test_in_engine_metrics_across_graph_replays():
    """the same across pa_hg_train_step(use_graph=1): the capture at step 0 and the replays at steps 1 and 2 each invalidate the
    cached arg-max (the replay path clears the flag in Net::train_step_graph, not in the forward pass)"""
    from pose_adv_aug_amd import _lib
    res, H = 128, 32
    net = _net(res)
    net.train()
    net.use_graph = True
    img4 = torch.zeros((mc.B, res, res, 4), dtype=_lib.act_dtype(), device='cuda')
    img4[..., :3] = mc.t(inputs.images(res, mc.B, res)).permute(0, 2, 3, 1).to(_lib.act_dtype())
    sets = (_oracle(H, 0), _oracle(H, 1), _oracle(H, 0))
    for step, o in enumerate(sets):
        loss, _ = net.loss_and_backward(img4=img4, pts=mc.t(o[1]).cuda())
        _write_heat(net, o[0])
        _assert_metrics(_metrics(net, H, o[2]), o, 'graph step %d' % step)
        assert np.isfinite(float(loss))
