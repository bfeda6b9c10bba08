"""num_modules > 1 (chains of residual blocks per hourglass site and in post_res) without a GPU: the oracle against the reference's own
2-module golden (tests/golden/make_modules_goldens.py), the engine's tensor table against the oracle's state_dict, the two creation
entries of the C ABI against each other, and the Python constructor.  Creating a net only declares tensors and lays the workspace
out: no device is touched."""
import ctypes as C
import multiprocessing as mp

import numpy as np
import pytest
import torch

from oracle import model as om
from oracle import step as ostep
from tests import inputs
from tests.test_oracle_golden import digest, load, t


def test_oracle_reproduces_the_reference_two_module_golden():
    """hg_s1m2c128.npz: the reference's create_hg(1, 2, 16, 128) through one training step.  The bars are those of
    tests/test_oracle_golden.py::test_hourglass_train_step for the outputs, the loss and the gradients."""
    g = load('hg_s1m2c128.npz')
    torch.set_num_threads(8)
    seed = 72
    net = om.create_hg(1, 2, 16, 128)
    assert sum(p.numel() for p in net.parameters()) == int(g['nparams']) and len(net.state_dict()) == int(g['nkeys']) == 671
    om.deterministic_fill_(net, seed=seed)
    net.train()
    img = t(inputs.images(seed + 100, 2, 128))
    heat = t(inputs.heatmaps_from_pts(inputs.heat_pts(seed + 200, 2, res=32), res=32))
    opt = ostep.make_optimizer(net)
    out, loss = ostep.pose_loss_and_grads(net, img, heat)
    grads = [p.grad.clone() for p in net.parameters()]
    opt.step()
    assert np.allclose(np.stack([o.detach().numpy() for o in out]), g['out'], atol=2e-5)
    assert abs(float(loss) - float(g['loss'])) < 1e-6
    assert np.allclose(digest(grads), g['grad_digest'], rtol=1e-3, atol=1e-6)
    names = [n for n, _ in net.named_parameters()]
    head = [n for n in names if n.startswith('out_conv.0.') or n.startswith('linear.0.1.')]
    assert head == list(g['head_names'])
    mine = np.concatenate([x.flatten().numpy() for n, x in zip(names, grads) if n in head])
    assert np.allclose(mine, g['head_grads'], rtol=1e-3, atol=1e-7)
    net.eval()
    with torch.no_grad():
        oe = np.stack([o.numpy() for o in net(img)])
    assert np.allclose(oe, g['out_eval'], rtol=1e-3, atol=2e-3)


def _table(L, h):
    name = C.create_string_buffer(256)
    shape = (C.c_int * 4)(); nd = C.c_int(); off = C.c_size_t(); numel = C.c_size_t(); kind = C.c_int()
    rows = []
    for i in range(L.pa_net_num_tensors(h)):
        assert L.pa_net_tensor_info(h, i, name, 256, shape, C.byref(nd), C.byref(off), C.byref(numel), C.byref(kind)) == 0
        rows.append((name.value.decode(), tuple(shape[k] for k in range(nd.value)), off.value, numel.value, kind.value))
    return rows


@pytest.mark.parametrize('stacks,modules,chan,entries', [(1, 2, 128, 671), (2, 3, 128, 1860), (2, 2, 256, 1272), (1, 2, 512, 671),
                                                        (2, 1, 512, 684)])
def test_tensor_table_is_the_oracles_state_dict(stacks, modules, chan, entries):
    """names, shapes and order of pa_net_tensor_info == the oracle's state_dict (the reference's registration order: the blocks
    <site>.0 .. <site>.<modules-1> of a site one after the other); the parameter count is the oracle's, rounded up to 4."""
    from pose_adv_aug_amd._lib import lib
    L = lib()
    h = L.pa_hg_create_modules(stacks, modules, 16, chan, 2, 256)
    assert h, L.pa_last_error()
    try:
        ref = om.create_hg(stacks, modules, 16, chan)
        sd = ref.state_dict()
        rows = _table(L, h)
        assert len(rows) == len(sd) == entries
        assert [r[0] for r in rows] == list(sd.keys())
        assert [r[1] for r in rows] == [tuple(v.shape) for v in sd.values()]
        nparams = sum(p.numel() for p in ref.parameters())
        assert L.pa_net_param_floats(h) == (nparams + 3) // 4 * 4
        assert L.pa_net_num_modules(h) == modules
        # parameters do not overlap and every tensor is 16-byte aligned
        par = sorted((r[2], r[3]) for r in rows if r[4] == 0)
        assert all(o % 4 == 0 for o, _ in par) and all(a[0] + a[1] <= b[0] for a, b in zip(par, par[1:]))
        # hg.<i>. stays one contiguous range of the flat parameter array
        lo, hi = C.c_size_t(), C.c_size_t()
        for i in range(stacks):
            assert L.pa_hg_bucket_range(h, i, C.byref(lo), C.byref(hi)) == 0, L.pa_last_error()
            inside = [r for r in rows if r[4] == 0 and r[0].startswith('hg.%d.' % i)]
            assert lo.value == min(r[2] for r in inside) and hi.value == max(r[2] + r[3] for r in inside)
    finally:
        L.pa_net_destroy(h)


def test_the_two_creation_entries_agree_at_one_module():
    from pose_adv_aug_amd._lib import lib
    L = lib()
    a = L.pa_hg_create(2, 16, 256, 24, 256)
    b = L.pa_hg_create_modules(2, 1, 16, 256, 24, 256)
    assert a and b
    try:
        assert _table(L, a) == _table(L, b)
        for f in (L.pa_net_param_floats, L.pa_net_buffer_floats, L.pa_net_workspace_bytes, L.pa_net_num_tensors, L.pa_net_num_modules):
            assert f(a) == f(b)
        assert L.pa_net_num_modules(a) == 1
    finally:
        L.pa_net_destroy(a); L.pa_net_destroy(b)


def test_agents_report_one_module():
    from pose_adv_aug_amd._lib import lib
    L = lib()
    h = L.pa_asn_create(128, 7, 7, 2, 256)
    assert h and L.pa_net_num_modules(h) == 1
    L.pa_net_destroy(h)


@pytest.mark.parametrize('modules', (0, 9, -1))
def test_module_counts_outside_1_to_8_are_refused_with_a_message(modules):
    from pose_adv_aug_amd._lib import lib
    L = lib()
    assert not L.pa_hg_create_modules(2, modules, 16, 256, 2, 256)
    assert b'num_modules' in L.pa_last_error(), L.pa_last_error()
    # the other conditions are pa_hg_create's
    assert not L.pa_hg_create_modules(2, 2, 16, 384, 2, 256) and not L.pa_hg_create_modules(2, 2, 15, 256, 2, 256)


def test_python_constructor_takes_num_modules():
    """(raised ValueError for anything but 1 before chains existed)"""
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    net = create_hg(2, 2, 16, 256)
    assert net.num_modules == 2
    assert create_hg(2, 1, 16, 256).num_modules == 1
    for bad in (0, 9):
        with pytest.raises(ValueError):
            create_hg(2, bad, 16, 256)


def test_option_num_modules_defaults_to_one(tmp_path):
    from pose_adv_aug_amd.options.train_options import TrainOptions
    base = ['--exp_dir', str(tmp_path), '--exp_id', 'x']
    assert TrainOptions().parse(base).num_modules == 1
    assert TrainOptions().parse(base + ['--num_modules', '3']).num_modules == 3


def _stub_worker(out):
    from tests import abi_stub
    fake = abi_stub.install(0)
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    net = create_hg(2, 1, 16, 256, default_batch=2)
    net._net(2)
    out['one'] = fake.names()
    del fake.log[:]
    net2 = create_hg(2, 2, 16, 256, default_batch=2)
    try:
        net2._net(2)
    except Exception:          # (the stub answers the unknown entry with 0 = NULL: creation fails, which is all this needs)
        pass
    out['two'] = [(n, tuple(a)) for n, a in fake.log if n.startswith('pa_hg_create')]


def test_one_module_net_goes_through_pa_hg_create():
    """tests/abi_stub.py stubs pa_hg_create by name: a num_modules = 1 net must keep using that entry, a 2-module net the new one."""
    out = mp.Manager().dict()
    p = mp.get_context('spawn').Process(target=_stub_worker, args=(out,))
    p.start(); p.join(120)
    assert p.exitcode == 0
    assert 'pa_hg_create' in out['one'] and 'pa_hg_create_modules' not in out['one']
    assert out['two'] == [('pa_hg_create_modules', (2, 2, 16, 256, 2, 256))]
