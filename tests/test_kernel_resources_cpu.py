"""Registers, scratch and LDS of the tile convolution kernels, from the compiler (tools/kernel_resources.py; no GPU): the instances that
are meant to run four workgroups per CU (csrc/conv1x1_tile.hip pa_conv1_occ, csrc/conv3x3_tile.hip pa_conv3_occ) must compile to four
waves per SIMD without scratch and with an LDS footprint that fits a CU four times; no other instance of the two files may use more
scratch than it did before these instances were moved (tests/golden/kernel_resources.json: the tool's output on the commit before)."""
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_resources as KR  # noqa: E402

FILES = ('conv1x1_tile.hip', 'conv3x3_tile.hip')
# <CIN,BM,BN,LD,KS,UP,POOL,PIN> / <CIN,BN,LD,TW,TH,SPS,PF,NT,FIN>; LD: 0 plain, 1 BatchNorm + ReLU, 2 BatchNorm backward
FOUR = {
    'conv1x1_tile.hip': ['conv1x1_tile_kernel<128,64,64,0,64,false,0,false>', 'conv1x1_tile_kernel<128,64,64,2,64,false,0,true>',
                         'conv1x1_tile_kernel<64,128,64,1,64,false,0,false>',
                         'conv1x1_tile_kernel<64,64,128,0,32,false,0,false>', 'conv1x1_tile_kernel<64,64,128,2,32,false,0,false>'],
    'conv3x3_tile.hip': ['conv3x3_tile_kernel<64,64,1,16,8,1,true,256,false>', 'conv3x3_tile_kernel<64,64,2,16,8,1,true,256,false>'],
}


@pytest.fixture(scope='module')
def resources():
    if KR._tool('hipcc') is None:
        pytest.fail('hipcc not found: the resource check needs the compiler the build uses')
    src = os.path.join(ROOT, 'pose_adv_aug_amd', 'csrc')
    with ThreadPoolExecutor(len(FILES)) as ex:
        return dict(zip(FILES, ex.map(lambda f: KR.kernel_resources(os.path.join(src, f)), FILES)))


@pytest.fixture(scope='module')
def before():
    return json.load(open(os.path.join(ROOT, 'tests', 'golden', 'kernel_resources.json')))


@pytest.mark.parametrize('f', FILES)
def test_four_workgroup_instances_fit_four_times(resources, f):
    for k in FOUR[f]:
        assert k in resources[f], (k, sorted(resources[f]))
        r = resources[f][k]
        assert r['waves_per_simd'] >= 4 and r['scratch'] == 0 and 4 * r['lds'] <= KR.LDS_PER_CU, (k, r)
        assert KR.blocks_per_cu(r) >= (4, 4), (k, r)


@pytest.mark.parametrize('f', FILES)
def test_no_other_instance_gained_scratch(resources, before, f):
    others = sorted(set(resources[f]) - set(FOUR[f]))
    assert others
    for k in others:
        assert k in before[f], '%s: an instance tests/golden/kernel_resources.json does not know' % k
        assert resources[f][k]['scratch'] <= before[f][k]['scratch'], (k, resources[f][k], before[f][k])
