"""GPU parity of the MFMA implicit-GEMM convolution kernels (forward, data gradient, weight gradient)
against torch.nn.functional.conv2d in fp32 on bf16-rounded operands.  Tolerance: the kernels multiply
bf16 operands exactly and accumulate in fp32, outputs are rounded to bf16 once: rel-rms <= 4e-3
(= bf16 half-ulp 2^-9 ~ 2e-3 plus accumulation-order noise); weight gradients stay fp32: <= 1e-4."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import inputs

pytestmark = pytest.mark.gpu


def rel_rms(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def run_conv(mode, a, b, w, bias, B, Cin, Cout, H, W, k, want_db=True):
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    L = lib()
    ws = torch.zeros(L.pa_conv2d_workspace_bytes(B, Cin, Cout, H, W, k), dtype=torch.uint8, device='cuda')
    if mode == 0:
        out = torch.empty((B, Cout, H, W), device='cuda'); out2 = None
    elif mode == 1:
        out = torch.empty((B, Cin, H, W), device='cuda'); out2 = None
    else:
        out = torch.empty((Cout, Cin, k, k), device='cuda'); out2 = torch.empty(Cout, device='cuda') if want_db else None
    # keep the device copies alive across the call (a temporary's block would be recycled by the allocator)
    ad = a.cuda().contiguous(); bd = b.cuda().contiguous() if b is not None else None
    wd = w.cuda().contiguous(); biasd = bias.cuda() if bias is not None else None
    check(L.pa_conv2d(mode, ptr(ad), ptr(bd), ptr(wd), ptr(biasd), ptr(out), ptr(out2),
                      B, Cin, Cout, H, W, k, ptr(ws), stream()), 'pa_conv2d')
    return out.cpu(), (out2.cpu() if out2 is not None else None)


SHAPES = [
    # B, Cin, Cout, H, W, k     (M = B*H*W)
    (2, 64, 64, 8, 8, 1),        # single 64x64 tile, K = 64
    (2, 128, 64, 16, 16, 1),     # two K steps
    (1, 64, 128, 5, 7, 1),       # ragged M = 35
    (2, 256, 128, 32, 32, 1),    # the bottleneck reduce conv
    (2, 128, 128, 16, 16, 3),    # the 3x3 conv, borders everywhere
    (3, 64, 64, 6, 10, 3),       # ragged M, non-square
    (24, 128, 256, 64, 64, 1),   # full-size expand conv: M = 98304 -> 128x128 tiles
    (24, 128, 128, 64, 64, 3),   # full-size 3x3 (BASELINE config 2 shape)
    # round 6: the persistent kernel with LDS-resident weights (conv1x1_ws.hip: >= 4 row tiles of 64 per CU) -- with the shape above
    # (128 -> 256 forward, 256 -> 128 data gradient) every instance: 256 -> 128 / 128 -> 256 / 128 -> 128, ragged tile count per workgroup
    (24, 256, 128, 64, 64, 1),
    (24, 128, 128, 64, 64, 1),
    (17, 256, 128, 64, 64, 1),   # 1088 tiles on 256 workgroups: 4.25 tiles each
    # shapes that select the tile kernels (conv3x3_tile.hip: H % 8 == 0, W % 16 == 0; conv_wgrad_tile.hip: >= 48 / 96 tiles)
    (6, 128, 128, 32, 32, 3),    # 48 halo tiles, 128 channels
    (8, 64, 128, 32, 48, 3),     # non-square, Cin != Cout, 96 tiles
    (3, 128, 64, 16, 32, 3),     # 12 tiles: tile forward/dgrad, generic wgrad
    (3, 256, 128, 64, 64, 1),    # 96 row tiles of 128 pixels
    (3, 64, 128, 65, 63, 1),     # ragged M = 12285 -> last row tile partly empty
    (4, 64, 64, 64, 64, 1),      # 64-channel blocks on both sides
    # shapes that reach the GENERIC kernel with 128-channel tiles (weight-row permutation of conv_igemm.hip)
    (4, 64, 128, 64, 64, 1),     # 128 row tiles of 128 < 192 -> generic <64,128>
    (8, 192, 128, 64, 64, 1),    # 192 input channels: not a tile-kernel shape, generic <128,128>
    (8, 192, 128, 64, 64, 3),
    # remaining template instances of the tile kernels (row tiles >= 192, channel blocks of 64 on either side)
    (3, 128, 64, 64, 64, 1),
    (3, 256, 64, 64, 64, 1),
    (6, 64, 128, 64, 64, 1),
    (6, 64, 64, 64, 64, 1),
    (24, 64, 64, 64, 64, 3),     # 64-channel 3x3 at 768 tiles (16 x 8 tiles, both channel blocks 64)
    # low-resolution levels: one workgroup = 2 images of 8x8 / 8 images of 4x4 (ragged image counts)
    (3, 128, 128, 8, 8, 3),
    (5, 64, 128, 4, 4, 3),
    (24, 128, 128, 4, 4, 3),
    # round 6: maps TILED by the 8 x 8 / 4 x 4 variants (sides multiples of 8 or 4 that the 16 x 8 tiles do not take): the 24 x 24 and 12 x 12
    # levels of BASELINE configs[4] (384 x 384 input); sub-tiles of one workgroup in two images, ragged last workgroup
    (5, 128, 128, 24, 24, 3),
    (16, 128, 128, 24, 24, 3),
    (3, 64, 128, 12, 12, 3),
    (16, 128, 128, 12, 12, 3),
    (2, 128, 64, 8, 24, 3),
    # ... and maps up to 8 x 8 that are neither 8 x 8 nor 4 x 4 (the 6 x 6 necks of configs[4]): one masked 8 x 8 tile per image
    (16, 128, 128, 6, 6, 3),
    (3, 64, 64, 5, 7, 3),
    # the layers of a chan-512 net: 512 input channels (the most pa_launch_conv admits: 8 K steps of the generic kernel, no tile or one-shot
    # instance), 512 output channels, the 3 x 3 layer with 256 input channels (K = 2304, no tile instance), weight-gradient plans of 8 / 16
    # channel blocks.  M < 16384: <64,64> tiles (the 256 -> 512 forward and the 512 -> 256 data gradient take the one-shot kernel)
    (2, 512, 256, 16, 16, 1),
    (2, 256, 512, 16, 16, 1),
    (2, 256, 256, 16, 16, 3),
    (1, 512, 512, 5, 7, 1),      # ragged M = 35
    (2, 512, 512, 32, 32, 1),
    (4, 512, 256, 64, 64, 1),    # M = 16384: <64,128>
    (8, 512, 256, 64, 64, 1),    # M = 32768: <128,128>
    (8, 256, 512, 64, 64, 1),    # forward: the row-tile kernel (256 input channels, 512 row tiles); data gradient <128,128>
    (8, 256, 256, 64, 64, 3),    # <128,128>, nine taps
    # the tilings no shape above reaches (tests/test_conv_plan_cpu.py asks the planner): the generic <128,64> tier with one and nine taps,
    # <64,128> with nine taps, and the 16 x 8 halo tiles of 128 input channels with a 64-channel output block (512 tiles: B 16 at 64 x 64)
    (8, 512, 64, 64, 64, 1),
    (8, 256, 64, 64, 64, 3),
    (4, 256, 128, 64, 64, 3),
    (16, 128, 64, 64, 64, 3),
]


@pytest.mark.parametrize('B,Cin,Cout,H,W,k', SHAPES)
def test_conv_forward(B, Cin, Cout, H, W, k):
    g = inputs.rng(100, B, Cin, Cout, H, k)
    x = torch.from_numpy(g.standard_normal((B, Cin, H, W)).astype(np.float32))
    w = torch.from_numpy((g.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32))
    bias = torch.from_numpy(g.standard_normal(Cout).astype(np.float32))
    y, _ = run_conv(0, x, None, w, bias, B, Cin, Cout, H, W, k)
    ref = F.conv2d(x.bfloat16().float(), w.bfloat16().float(), bias, padding=k // 2)
    assert rel_rms(y, ref) < 4e-3


@pytest.mark.parametrize('B,Cin,Cout,H,W,k', SHAPES)
def test_conv_dgrad(B, Cin, Cout, H, W, k):
    g = inputs.rng(101, B, Cin, Cout, H, k)
    dy = torch.from_numpy(g.standard_normal((B, Cout, H, W)).astype(np.float32))
    w = torch.from_numpy((g.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32))
    dx, _ = run_conv(1, dy, None, w, None, B, Cin, Cout, H, W, k)
    ref = F.conv_transpose2d(dy.bfloat16().float(), w.bfloat16().float(), padding=k // 2)
    assert rel_rms(dx, ref) < 4e-3


@pytest.mark.parametrize('B,Cin,Cout,H,W,k', SHAPES)
def test_conv_wgrad(B, Cin, Cout, H, W, k):
    g = inputs.rng(102, B, Cin, Cout, H, k)
    dy = torch.from_numpy(g.standard_normal((B, Cout, H, W)).astype(np.float32))
    x = torch.from_numpy(g.standard_normal((B, Cin, H, W)).astype(np.float32))
    w = torch.zeros((Cout, Cin, k, k))
    dw, db = run_conv(2, dy, x, w, None, B, Cin, Cout, H, W, k)
    xr = x.bfloat16().float(); dyr = dy.bfloat16().float()
    wr = torch.zeros((Cout, Cin, k, k), requires_grad=True)
    br = torch.zeros(Cout, requires_grad=True)
    torch.set_num_threads(8)
    F.conv2d(xr, wr, br, padding=k // 2).backward(dyr)
    assert rel_rms(dw, wr.grad) < 1e-4
    assert rel_rms(db, br.grad) < 1e-4
    # without the bias gradient (every conv in front of a BatchNorm): the 3x3 tile kernel takes this path
    dw2, _ = run_conv(2, dy, x, w, None, B, Cin, Cout, H, W, k, want_db=False)
    assert rel_rms(dw2, wr.grad) < 1e-4


@pytest.mark.parametrize('B,H', [(24, 64), (24, 32), (24, 16), (24, 8)])
def test_conv3x3_tile_has_no_sporadic_elements(B, H):
    """Race screen for the LDS-DMA weight ring of conv3x3_tile.hip (counted s_waitcnt vmcnt + raw s_barrier): a missing
    `s_waitcnt lgkmcnt(0)` in front of the barrier once gave 0.3-0.5 % wrong elements (whole 8-channel groups off by
    O(1)) at some launches only, which a relative-RMS bound does not see reliably.  Here every element of five
    repeated launches per shape is checked against fp32 conv2d with an ABSOLUTE bound (bf16 output rounding at |y| < 8
    is <= 0.03)."""
    torch.set_num_threads(8)
    Cin = Cout = 128
    g = inputs.rng(300, B, H)
    x = torch.from_numpy(g.standard_normal((B, Cin, H, H)).astype(np.float32))
    w = torch.from_numpy((g.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32))
    ref = F.conv2d(x.bfloat16().float(), w.bfloat16().float(), None, padding=1)
    for rep in range(5):
        y, _ = run_conv(0, x, None, w, None, B, Cin, Cout, H, H, 3)
        err = (y - ref).abs()
        assert float(err.max()) < 0.05, (rep, float(err.max()), float((err > 0.05).float().mean()))


# ---------------------------------------------------------------------------------------------------------------------
# The grouped weight-gradient launch (wgrad_group_kernel, conv_wgrad_tile.hip): the training step's dominant kernel by time.  It is
# reached here through pa_wgrad_group (mode 0: the same layers launched alone, 1: ONE group launch ordered longest-first like
# Net::flush_wgrads does, 2: one group launch in the given order) and checked against autograd of F.conv2d on the bf16-rounded EFFECTIVE
# operands (x through BatchNorm + ReLU, dy through the BatchNorm backward, exactly as the kernel forms them before its MFMAs).
def _wg_job(g, B, Cin, Cout, H, W, k, lin2, bnrelu, want_db):
    """one layer: host tensors + the fp32 reference gradient"""
    dy = torch.from_numpy(g.standard_normal((B, Cout, H, W)).astype(np.float32)).bfloat16().float()
    x = torch.from_numpy(g.standard_normal((B, Cin, H, W)).astype(np.float32)).bfloat16().float()
    job = dict(B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=k, dy=dy, x=x, dy_q=None, dy_k=None, x_k=None, want_db=want_db)
    dye, xe = dy, x
    if lin2:
        q = torch.from_numpy(g.standard_normal((B, Cout, H, W)).astype(np.float32)).bfloat16().float()
        kk = torch.from_numpy(np.stack([g.uniform(0.5, 1.5, Cout), g.uniform(-0.5, 0.5, Cout), g.uniform(-0.1, 0.1, Cout)]).astype(np.float32))
        job['dy_q'] = q; job['dy_k'] = kk
        # fmaf(k0, p, fmaf(k1, q, k2)) rounded to the 16-bit storage type once (conv_wgrad_tile.hip staging)
        dye = (kk[0].view(1, -1, 1, 1).double() * dy.double() + (kk[1].view(1, -1, 1, 1).double() * q.double() + kk[2].view(1, -1, 1, 1).double())).float().bfloat16().float()
    if bnrelu:
        kx = torch.from_numpy(np.stack([g.uniform(0.5, 1.5, Cin), g.uniform(-0.3, 0.3, Cin)]).astype(np.float32))
        job['x_k'] = kx
        xe = torch.clamp(kx[0].view(1, -1, 1, 1).double() * x.double() + kx[1].view(1, -1, 1, 1).double(), min=0).float().bfloat16().float()
    wr = torch.zeros((Cout, Cin, k, k), requires_grad=True)
    br = torch.zeros(Cout, requires_grad=True)
    F.conv2d(xe, wr, br, padding=k // 2).backward(dye)
    job['ref_dw'] = wr.grad; job['ref_db'] = br.grad
    return job


def _run_wgrad_group(jobs, mode):
    import ctypes as C
    from pose_adv_aug_amd._lib import lib, check, ptr, stream

    class Job(C.Structure):
        _fields_ = [(n, C.c_int) for n in ('B', 'Cin', 'Cout', 'H', 'W', 'k')] + [(n, C.c_void_p) for n in ('dy', 'dy_q', 'dy_k', 'x', 'x_k', 'dw', 'db')]

    L = lib()
    arr = (Job * len(jobs))()
    keep = []
    outs = []
    for i, j in enumerate(jobs):
        dev = {n: (j[n].cuda().contiguous() if j[n] is not None else None) for n in ('dy', 'dy_q', 'dy_k', 'x', 'x_k')}
        dw = torch.full((j['Cout'], j['Cin'], j['k'], j['k']), float('nan'), device='cuda')
        db = torch.full((j['Cout'],), float('nan'), device='cuda') if j['want_db'] else None
        keep.append((dev, dw, db)); outs.append((dw, db))
        for n in ('B', 'Cin', 'Cout', 'H', 'W', 'k'):
            setattr(arr[i], n, j[n])
        for n in ('dy', 'dy_q', 'dy_k', 'x', 'x_k'):
            setattr(arr[i], n, dev[n].data_ptr() if dev[n] is not None else None)
        arr[i].dw = dw.data_ptr(); arr[i].db = db.data_ptr() if db is not None else None
    nbytes = L.pa_wgrad_group_workspace_bytes(C.addressof(arr), len(jobs))
    assert nbytes > 0
    ws = torch.zeros(nbytes + 4096, dtype=torch.uint8, device='cuda')
    ws[nbytes:] = 0xA5                                      # guard region behind the workspace
    check(L.pa_wgrad_group(C.addressof(arr), len(jobs), mode, ptr(ws), stream()), 'pa_wgrad_group')
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all()), 'pa_wgrad_group wrote behind its workspace'
    return [(dw.cpu(), db.cpu() if db is not None else None) for dw, db in outs]


# (B, Cin, Cout, H, W, k, dy through BatchNorm backward, x through BatchNorm + ReLU, bias gradient)
_R64 = [  # one residual block of the 64 x 64 level at a small batch: conv3 / conv2 (dz stored: plain dy) / conv1 (LIN2 dy)
    (3, 128, 256, 64, 64, 1, False, True, False), (3, 128, 128, 64, 64, 3, False, True, False), (3, 256, 128, 64, 64, 1, True, False, False)]
WG_GROUPS = {
    'two_1x1_128x128_and_3x3_lin2': [(3, 128, 128, 64, 64, 3, True, True, False), (3, 128, 128, 32, 32, 1, False, True, True)],
    'residual_block_64': _R64,
    # ragged: tile counts that the jobs' split counts do not divide (56 halo tiles; 40 and 38 row tiles of 128 pixels, the last one partly empty)
    'ragged_splits': [(7, 128, 128, 32, 32, 3, True, True, False), (5, 64, 128, 32, 32, 1, False, False, True), (5, 128, 64, 24, 40, 1, True, True, True)],
    # eight jobs, every tile shape of the kernel (3x3 64x64 plain and LIN2; 1x1 128x128, 128x64, 64x128, 64x64), mixed operand modes
    'eight_mixed': [(2, 128, 128, 64, 64, 3, False, True, False), (2, 64, 64, 64, 64, 3, True, True, False),
                    (2, 128, 128, 64, 64, 1, True, True, True), (2, 64, 128, 64, 64, 1, False, False, True),
                    (2, 128, 64, 64, 64, 1, True, False, False), (2, 64, 64, 64, 64, 1, False, True, True),
                    (2, 256, 128, 32, 32, 1, True, True, False), (2, 128, 256, 32, 32, 1, False, True, True)],
}


@pytest.mark.parametrize('name', sorted(WG_GROUPS))
def test_wgrad_group_kernel_matches_conv2d_and_the_single_launches(name):
    torch.set_num_threads(8)
    g = inputs.rng(400, len(name))
    jobs = [_wg_job(g, *spec) for spec in WG_GROUPS[name]]
    alone = _run_wgrad_group(jobs, 0)
    group = _run_wgrad_group(jobs, 1)
    # the step's order is longest-first; here: the caller's order reversed (begin[] of the kernel not sorted by work)
    rev = _run_wgrad_group(jobs[::-1], 2)[::-1]
    for j, (dw0, db0), (dw1, db1), (dw2, db2) in zip(jobs, alone, group, rev):
        tag = (name, j['Cin'], j['Cout'], j['H'], j['k'])
        assert torch.isfinite(dw1).all() and torch.isfinite(dw2).all(), tag
        assert rel_rms(dw1, j['ref_dw']) < 1e-4, tag            # the single-layer tolerance of test_conv_wgrad
        assert rel_rms(dw0, j['ref_dw']) < 1e-4, tag
        assert rel_rms(dw1, dw0) < 1e-6, tag                    # group == the same layers launched alone (same tiles, same split order)
        assert rel_rms(dw2, dw0) < 1e-6, tag                    # ... in any job order
        if j['want_db']:
            assert rel_rms(db1, j['ref_db']) < 1e-4 and rel_rms(db1, db0) < 1e-6 and rel_rms(db2, db0) < 1e-6, tag


def test_wgrad_group_refuses_shapes_the_grouped_kernel_does_not_take():
    from pose_adv_aug_amd._lib import PoseAdvError
    g = inputs.rng(401)
    jobs = [_wg_job(g, 2, 64, 64, 8, 8, 3, False, True, False)]            # 8 x 8 map: no 8 x 16 tiles
    assert rel_rms(_run_wgrad_group(jobs, 0)[0][0], jobs[0]['ref_dw']) < 1e-4      # alone: the generic kernel takes it
    with pytest.raises(PoseAdvError):
        _run_wgrad_group(jobs, 1)
