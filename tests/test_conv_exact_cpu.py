"""The bounds of tests/conv_exact.py are not vacuous: on synthetic tensors with the net's level shapes (small batches), an fp32 emulation
of the conv kernels (bf16 operands, fp32 accumulation in chunks of the MFMA's K = 32 along the tap-major reduction, the chain of chunks,
the epilogue adds, one rounding to nearest even) passes every check, and each of these defects is reported -- or, where the bound cannot
see it, that is asserted instead of claimed:
  * one halo tap dropped on a tile border (one column of one image, the tap that reads the neighbouring tile): caught;
  * one 8 x 16 tile of the output shifted by one pixel: caught;
  * the output rounded toward zero instead of to nearest even: caught (half of the elements are up to one ulp off);
  * the bias omitted or doubled: caught;
  * one 8-channel group of the input transformed (BatchNorm+ReLU) with its neighbouring group's constants: caught;
  * the data gradient's ReLU mask taken from the raw tensor instead of the value: caught;
  * a shortcut addend rounded to bf16 before the add: caught (per element about a quarter ulp of the addend, many elements);
  * weight gradient: one split's slab dropped or doubled: caught at the split counts of the net's layers; one image's contribution
    missing: caught at B 2 / 3; one image row missing from a B 24 64 x 64 gradient (1 / 1536 of the pixels): caught, and so is one
    missing pixel there -- the bound is per element and, at the grouped split count, about 2u * 250 of sum |dy x|;
  * a nonzero value where every term of the sum is zero (the ulp of zero is the storage type's floor): caught."""
import pytest
import torch

from tests import conv_exact as X

torch.set_num_threads(min(16, torch.get_num_threads()))
BF = torch.bfloat16


def _f32(x):
    return x.float()


def emulate_conv(x, w, bias=None, add=(), stride=1, pad=None, drop_tap=None, shift_tile=None, rtz=False, bias_mult=1.0):
    """the kernel's arithmetic: bf16 operands (exact in float64), per-tap 32-channel chunks summed exactly then rounded to fp32 (one
    MFMA: within its 2u-per-addition allowance), chained in fp32; + bias, + each addend in fp32; rounded to bf16 (RNE or toward zero)."""
    k = w.shape[2]
    pad = k // 2 if pad is None else pad
    B, C, H, W_ = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W_ + 2 * pad - k) // stride + 1
    acc = torch.zeros(B, Ho, Wo, w.shape[0], dtype=torch.float32)
    for ky, kx, xs in X._taps(x.double(), k, stride, pad, Ho, Wo):
        for c0 in range(0, C, 32):
            part = xs[..., c0:c0 + 32].matmul(w[:, c0:c0 + 32, ky, kx].double().t())
            if drop_tap is not None and (ky, kx) == drop_tap[0]:
                b_, col = drop_tap[1]
                part[b_, :, col, :] = 0
            acc = acc + part.float()
    if bias is not None:
        acc = acc + _f32(bias) * bias_mult
    out = acc.permute(0, 3, 1, 2)
    for a in add:
        out = out + _f32(a)
    if shift_tile is not None:
        b_, y0, x0 = shift_tile
        out = out.clone()
        out[b_, :, y0:y0 + 8, x0:x0 + 16] = out[b_, :, y0:y0 + 8, x0 + 1:x0 + 17].clone()
    if rtz:
        bits = out.contiguous().view(torch.int32) & ~0xFFFF
        return bits.view(torch.float32).to(BF).double()
    return out.to(BF).double()


def _data(B, C, N, H, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(B, C, H, H, generator=g, dtype=torch.float64)).to(BF).double()
    w = (torch.randn(N, C, k, k, generator=g, dtype=torch.float64) / (C * k * k) ** 0.5).to(BF).double()
    b = torch.randn(N, generator=g, dtype=torch.float64).float().double() * 0.3
    return g, x, w, b


# (B, Cin, Cout, H, k): the residual blocks' convs at the net's levels, small batches
LEVELS = [(2, 128, 128, 32, 3), (2, 256, 128, 16, 1), (2, 128, 256, 16, 1), (3, 128, 128, 24, 3), (2, 128, 128, 4, 3), (3, 128, 128, 6, 3),
          # the layers of a chan-512 block: K = 512 (16 chunks of the MFMA's 32), 512 outputs, the 3 x 3 layer at K = 2304 (72 chunks)
          # (32 wide: the dropped halo tap below sits on column 16)
          (2, 512, 256, 8, 1), (2, 256, 512, 8, 1), (1, 256, 256, 32, 3)]


def _fwd(x, w, b, **kw):
    return X.check16(emulate_conv(x, w, b, **kw), X.conv_term(x, w, x.shape[1] * w.shape[2] ** 2, b), BF)


@pytest.mark.parametrize('B,C,N,H,k', LEVELS)
def test_forward_bound_holds_and_catches_the_defects(B, C, N, H, k):
    g, x, w, b = _data(B, C, N, H, k, seed=H * 11 + k)
    ok = _fwd(x, w, b)
    assert ok[0] <= 1.0 and ok[0] > 0.3, ok                      # tight: the half ulp is reached
    assert _fwd(x, w, b, rtz=True)[0] > 1.0
    assert X.check16(emulate_conv(x, w, None), X.conv_term(x, w, C * k * k, b), BF)[0] > 1.0          # bias omitted
    assert _fwd(x, w, b, bias_mult=2.0)[0] > 1.0                                                      # bias doubled
    if k == 3 and H >= 16:
        assert _fwd(x, w, b, drop_tap=((1, 0), (B - 1, 16 % H)))[0] > 1.0      # the left tap of column 16 (left halo of a 16-wide tile)
        assert _fwd(x, w, b, shift_tile=(0, 8, 0))[0] > 1.0
    # one 8-channel group through BatchNorm+ReLU with its neighbour's constants (the prologue); the check uses the true values
    raw = torch.randn(B, C, H, H, generator=g, dtype=torch.float64).to(BF).double()
    k0 = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).float().double()
    k1 = (torch.randn(C, generator=g, dtype=torch.float64) * 0.5).float().double()
    val = lambda a, c: torch.relu((a.view(1, -1, 1, 1) * raw + c.view(1, -1, 1, 1)).float().double())     # fmaf: one rounding
    good = val(k0, k1)
    k0b, k1b = k0.clone(), k1.clone()
    k0b[8:16], k1b[8:16] = k0[16:24], k1[16:24]
    ref = X.conv_term(X.rnd(good, BF), w, C * k * k, b)
    assert X.check16(emulate_conv(X.rnd(good, BF), w, b), ref, BF)[0] <= 1.0
    assert X.check16(emulate_conv(X.rnd(val(k0b, k1b), BF), w, b), ref, BF)[0] > 1.0


@pytest.mark.parametrize('B,C,N,H', [(2, 128, 256, 16), (3, 128, 256, 24)])
def test_shortcut_addend_and_data_gradient_mask(B, C, N, H):
    g, x, w, b = _data(B, C, N, H, 1, seed=B * H)
    short = torch.relu(torch.randn(B, N, H, H, generator=g, dtype=torch.float64) * 3).float().double()   # the fp32 value view 0
    ref = X.conv_term(x, w, C, b, (short,))
    assert X.check16(emulate_conv(x, w, b, add=(short,)), ref, BF)[0] <= 1.0
    assert X.check16(emulate_conv(x, w, b, add=(X.rnd(short, BF),)), ref, BF)[0] > 1.0        # rounded before the add
    # data gradient of a 1 x 1 conv, masked by the ReLU of the value relu(k0 raw + k1); a mask from raw > 0 differs where k1 moves the sign
    dy = torch.randn(B, N, H, H, generator=g, dtype=torch.float64).to(BF).double()
    raw = torch.randn(B, C, H, H, generator=g, dtype=torch.float64).to(BF).double()
    value = torch.relu(raw + 0.4)
    t = X.dgrad_term(dy, w, N)
    wt = w.flip(2, 3).transpose(0, 1)
    dx = emulate_conv(dy, wt)
    assert X.check16(dx * (value > 0).double(), t, BF, (value > 0).double())[0] <= 1.0
    assert X.check16(dx * (raw > 0).double(), t, BF, (value > 0).double())[0] > 1.0


def emulate_wgrad(x, dy, k, S, drop_split=None, double_split=None, drop_image=None, drop_row=None):
    """fp32 slabs of S contiguous pixel ranges (32-pixel MFMA chunks chained in fp32), summed in split order."""
    B, C, H, W_ = x.shape
    pad = k // 2
    xs_all = [(ky, kx, xs.reshape(-1, C)) for ky, kx, xs in X._taps(x.double(), k, 1, pad, H, W_)]
    g = dy.double().permute(0, 2, 3, 1).reshape(-1, dy.shape[1])
    keep = torch.ones(g.shape[0], dtype=torch.float64)
    if drop_image is not None:
        keep.view(B, H * W_)[drop_image] = 0
    if drop_row is not None:
        keep.view(B, H, W_)[drop_row[0], drop_row[1]] = 0
    g = g * keep[:, None]
    M = g.shape[0]
    per = -(-M // S)
    out = torch.zeros(dy.shape[1], C, k, k, dtype=torch.float32)
    for s in range(S):
        if s == drop_split:
            continue
        slab = torch.zeros(dy.shape[1], C, k, k, dtype=torch.float32)
        end = min(M, (s + 1) * per)
        for m0 in range(s * per, end, 32):
            m1 = min(m0 + 32, end)
            for ky, kx, xs in xs_all:
                slab[:, :, ky, kx] += g[m0:m1].t().matmul(xs[m0:m1]).float()
        out = out + slab * (2 if s == double_split else 1)
    return out


@pytest.mark.parametrize('B,C,N,H,k', [(2, 128, 128, 16, 3), (3, 128, 256, 24, 1), (2, 64, 64, 32, 1), (2, 512, 256, 16, 1), (2, 256, 256, 16, 3)])
def test_wgrad_bound_holds_and_catches_a_split_and_an_image(B, C, N, H, k):
    g, x, _, _ = _data(B, C, N, H, k, seed=7 * H + k)
    dy = (torch.randn(B, N, H, H, generator=g, dtype=torch.float64) * 1e-2).to(BF).double()
    S = X.layer_splits(B, H, H, C, N, k)
    ck = lambda dw: X.wgrad_check(dw, x, dy, k, S)[0]
    assert ck(emulate_wgrad(x, dy, k, S)) <= 1.0
    if S > 1:
        assert ck(emulate_wgrad(x, dy, k, S, drop_split=S // 2)) > 1.0
        assert ck(emulate_wgrad(x, dy, k, S, double_split=0)) > 1.0
    assert ck(emulate_wgrad(x, dy, k, S, drop_image=B - 1)) > 1.0
    db = dy.sum(dim=(0, 2, 3)).float()
    assert X.bgrad_check(db, dy, S)[0] <= 1.0
    assert X.bgrad_check(db - dy[B - 1].sum(dim=(1, 2)).float(), dy, S)[0] > 1.0      # one image missing from the bias gradient


def test_one_missing_image_row_is_caught_at_benchmark_size():
    """B 24, 64 x 64, 1 x 1, 128 -> 128 at its grouped split count (S 64): the accumulation bound is per element, and one image row
    (1 / 1536 of the pixels) is far outside it -- here even one missing pixel is."""
    g = torch.Generator().manual_seed(3)
    B, C, H = 24, 128, 64
    x = torch.relu(torch.randn(B, C, H, H, generator=g, dtype=torch.float64)).to(BF).double()
    dy = (torch.randn(B, C, H, H, generator=g, dtype=torch.float64) * 1e-2).to(BF).double()
    S = X.layer_splits(B, H, H, C, C, 1)
    assert X.wgrad_check(X.wgrad64(x, dy, 1).float(), x, dy, 1, S)[0] <= 1.0
    for sl in ((5, slice(None), 17, slice(None)), (5, slice(None), 17, 30)):
        d = dy.clone()
        d[sl] = 0
        assert X.wgrad_check(X.wgrad64(x, d, 1).float(), x, dy, 1, S)[0] > 1.0


@pytest.mark.parametrize('dtype,floor', [(torch.bfloat16, 2.0 ** -133), (torch.float16, 2.0 ** -24)])
def test_an_element_whose_terms_are_all_zero_must_be_zero(dtype, floor):
    """ulp(0) is the storage type's floor, so an output whose every term is exactly zero has a bound of half its smallest subnormal:
    any nonzero value there fails."""
    assert float(X.ulp(torch.zeros(1, dtype=torch.float64), dtype)) == floor
    x = torch.zeros(1, 64, 4, 4, dtype=torch.float64)
    x[:, :, 1:, 1:] = 1.0
    w = torch.ones(8, 64, 1, 1, dtype=torch.float64)
    t = X.conv_term(x, w, 64)
    got = X.conv64(x, w)
    assert X.check16(got, t, dtype)[0] <= 1.0
    bad = got.clone()
    bad[0, 0, 0, 0] = torch.tensor(floor, dtype=dtype).double()           # the smallest positive value of the type, where all terms are 0
    assert X.check16(bad, t, dtype)[0] > 1.0


def test_split_mirror_knows_the_net_layers_and_refuses_unknown_shapes():
    assert X.layer_splits(24, 128, 128, 3, 64, 7) == 512              # the stem at benchmark size (pa_wgrad_plan's stem override)
    assert X.layer_splits(2, 64, 64, 3, 64, 7) == 128                 # tiny maps: the generic count
    assert X.group_splits(24, 64, 64, 128, 128, 9) > 0                # the grouped kernel takes the 64 x 64 3 x 3 layers
    assert X.group_splits(2, 8, 8, 128, 128, 9) == 0
    with pytest.raises(ValueError):
        X.wgrad_splits(100, 10, 10, 96, 64, 1)
    with pytest.raises(ValueError):
        X.wgrad_splits(100, 10, 10, 64, 64, 4)


@pytest.mark.parametrize('chan', (128, 512))
def test_site_lists_name_every_conv_and_batchnorm_of_the_oracle(chan):
    """What run_leg asserts on the GPU against the engine's state_dict (whose keys are the oracle's: tests/test_modules_cpu.py), here
    against the oracle's own: conv_names / bn_sites name every conv and BatchNorm of a 2-stack net, at chan 512 as at 128; and the
    shapes the chan-512 legs are there for -- 512 input channels, the 3 x 3 layer with 256, the inner head's 512 -> 512 and 16 -> 512."""
    from oracle import model as om
    from tests import bn_exact
    sd = om.create_hg(2, 1, 16, chan).state_dict()
    assert sorted(X.conv_names(2)) == sorted(k[:-len('.weight')] for k in sd if k.endswith('.weight') and sd[k].dim() == 4)
    assert sorted(p for p, _ in bn_exact.bn_sites(2)) == sorted(k[:-len('.running_mean')] for k in sd if k.endswith('.running_mean'))
    shape = lambda n: tuple(sd[n + '.weight'].shape)
    assert shape('hg.0.skip1.0.conv1') == (chan // 2, chan, 1, 1) and shape('hg.1.neck.0.conv2') == (chan // 2, chan // 2, 3, 3)
    assert shape('hg.0.up4.0.conv3') == (chan, chan // 2, 1, 1) and shape('residual3.adapter') == (chan, 128, 1, 1)
    assert shape('forth_conv.0') == (chan, chan, 1, 1) and shape('in_conv.0') == (chan, 16, 1, 1) and shape('out_conv.1') == (16, chan, 1, 1)


def test_the_chan_512_legs_meet_grouped_splits_and_the_plans_of_8_and_16_blocks():
    """expect=('group',) of the chan-512 legs (tests/test_gpu_conv_exact.py) from the mirror alone, and the plans those legs are there
    for: 8 channel blocks for the 1 x 1 layers of a block (128-channel blocks on both sides) and 16 for the head's 512 -> 512; for the
    3 x 3 layer 16 blocks of 64 x 64 channels where the tile kernel takes the map (>= 48 tiles of 8 x 16) and 36 (2 x 18 blocks of 128
    over taps * Cin) in the generic plan below that."""
    assert X.wgrad_plan(2, 32, 32, 512, 256, 1).blocks == 8 and X.wgrad_plan(2, 32, 32, 256, 512, 1).blocks == 8
    assert X.wgrad_plan(2, 32, 32, 512, 512, 1).blocks == 16
    assert X.wgrad_plan(4, 64, 64, 256, 256, 9)[:1] + X.wgrad_plan(4, 64, 64, 256, 256, 9)[-1:] == ('tile', 16)
    assert X.wgrad_plan(2, 32, 32, 256, 256, 9)[:1] + X.wgrad_plan(2, 32, 32, 256, 256, 9)[-1:] == ('generic', 36)
    for B, H in ((2, 32), (4, 64), (8, 64), (2, 64)):           # the largest hourglass map of each leg
        assert X.group_splits(B, H, H, 512, 256, 1) > 0 and X.group_splits(B, H, H, 256, 512, 1) > 0, (B, H)
    assert X.group_splits(2, 32, 32, 256, 256, 9) == 0 and X.group_splits(4, 64, 64, 256, 256, 9) > 0
    assert X.group_splits(2, 8, 8, 512, 256, 1) == 0            # below three 128-pixel tiles: the generic count


def test_the_grouped_split_count_never_exceeds_the_count_of_the_layer_alone():
    """pa_conv2d_workspace_bytes lays its layer out without the batch (PaWgradPlan::splits), pa_conv2d with it (group_splits where the
    grouped kernel takes the shape): the size query covers the run only while group_splits <= splits.  Release values, every shape of the
    sweep."""
    n = 0
    for taps in (1, 9):
        for Cin in (64, 128, 192, 256, 384, 512):
            for Cout in (64, 128, 192, 256, 384, 512):
                for B in (1, 2, 3, 5, 8, 16, 24, 32):
                    for H in (4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128):
                        for W in sorted(set((H, 2 * H, 16, 32))):
                            p = X.wgrad_plan(B, H, W, Cin, Cout, taps)
                            assert p.group_splits <= p.splits, ((B, H, W, Cin, Cout, taps), p)
                            n += 1
    assert n == 23040


# The workspace queries make no HIP call, so the mirror test of the GPU selection also runs here (same body, collected a second time
# under this module): it pins every layer's slab count without a GPU.
from tests.test_gpu_conv_exact import test_split_mirror_matches_the_library  # noqa: E402,F401


def test_data_gradient_of_a_plain_input_catches_a_relu_mask():
    """up4 in a step with occlusion masks reads maskedneck, a plain tensor (no pending BatchNorm): its gradient conv1^T(g1) + dz3 goes
    through a plain epilogue and is checked without a mask (Checker.block(in_masked=False)).  A gradient that was masked by the ReLU of
    the tensor's value -- which is zero inside the dropped cells and wherever the neck's ReLU cut -- is outside the bound."""
    B, C, N, H = 2, 128, 64, 4
    g, _, w, _ = _data(B, C, N, H, 1, seed=21)
    dy = torch.randn(B, N, H, H, generator=g, dtype=torch.float64).to(BF).double()              # g1, the gradient of up4.x1
    dz3 = torch.randn(B, C, H, H, generator=g, dtype=torch.float64).to(BF).double()             # the shortcut's addend
    value = torch.relu(torch.randn(B, C, H, H, generator=g, dtype=torch.float64)).to(BF).double()
    value[0, :, 0, 0] = 0                                                                       # a dropped cell
    t = X.dgrad_term(dy, w, N, (dz3,))
    dx = emulate_conv(dy, w.flip(2, 3).transpose(0, 1), add=(dz3,))
    assert X.check16(dx, t, BF, None)[0] <= 1.0
    assert X.check16(dx * (value > 0).double(), t, BF, None)[0] > 1.0
    # (and the converse stays caught: a plain gradient where the check expects the mask)
    assert X.check16(dx, t, BF, (value > 0).double())[0] > 1.0
