"""The planner's read-only query (pa_conv_plan_describe) and the engine's launch log for the tests: tests/test_conv_plan_cpu.py and the GPU
legs that assert the tier they exist to reach."""
import contextlib
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('path', 'inst', 'gx', 'gy', 'threads', 'nbw', 'rows', 'rows2', 'xcd', 'takes_fin', 'stores_dz', 'pool_route', 'pool_in', 'bwd_lds',
          'cannot_trap', 'kernel_lds')
REFUSED, GENERIC, ONESHOT, ROW, ROW_UP, TILE3 = range(6)
NONE, PLAIN, BNRELU, LIN2, POOL = -1, 0, 1, 2, 3                 # operand load modes
OUT_PLAIN, OUT_STATS, OUT_BWD = 0, 1, 2                          # epilogue modes
BIAS, OUT2, DZ, IN_MAP, IN_Q, EP2_AFFINE, ADD2_MAP = 1, 2, 4, 8, 16, 32, 64
VARIANTS = 8


def _tilings():
    """names of enum PaConvTiling, in order (the instance id is tiling * 8 + variant)"""
    hdr = open(os.path.join(ROOT, 'pose_adv_aug_amd', 'csrc', 'conv_plan.h')).read()
    body = re.search(r'enum PaConvTiling \{(.*?)PA_CT_N', hdr, re.S).group(1)
    return re.findall(r'PA_CT_(\w+)', body)


TILINGS = _tilings()


def lib():
    import pose_adv_aug_amd as P
    if not os.path.isfile(P.LIB_PATH):
        P.build()
    return P.lib()


def describe(L, B, H, W, Cin, Cout, taps, in_=PLAIN, a1=NONE, a2=NONE, ep=OUT_PLAIN, ep2=OUT_PLAIN, fin=0, flags=0, cus=256):
    out = (C.c_int * 16)()
    assert L.pa_conv_plan_describe(B, H, W, Cin, Cout, taps, in_, a1, a2, ep, ep2, fin, flags, cus, out, 16) == 16
    d = dict(zip(FIELDS, out))
    d['tiling'] = TILINGS[d['inst'] // VARIANTS] if d['path'] != REFUSED else None
    d['variant'] = d['inst'] % VARIANTS if d['path'] != REFUSED else None
    return d


def device_cus():
    """compute units of the device a GPU leg runs on (what the launchers pass to the planner)"""
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def plan(*shape, **modes):
    """the plan of one launch ON THIS DEVICE, for the GPU legs that exist to reach a tier: they assert it instead of re-deriving the dispatch"""
    modes.setdefault('cus', device_cus())
    return describe(lib(), *shape, **modes)


LAUNCHES = os.path.join(ROOT, 'tests', 'golden', 'conv_launches.json')


def recorded_launches():
    """{leg: [launch, ...]}: convolution launches of the numerical GPU legs, each the 14 arguments of pa_conv_plan_describe, as the engine's launch
    log gave them on the MI355X.  Every leg asserts that it still makes the launches listed for it (launches()), so the list cannot go stale
    unseen; POSEADV_WRITE_CONV_LAUNCHES=<file> makes the legs write a new list instead."""
    import json
    return {k: [tuple(x) for x in v] for k, v in json.load(open(LAUNCHES)).items()}


@contextlib.contextmanager
def launches(leg):
    """around the body of a GPU leg: the engine's launch log; afterwards every launch recorded for the leg must have been made"""
    import json
    L = lib()
    L.pa_conv_launch_log(None, 0)
    try:
        yield
    except BaseException:
        L.pa_conv_launch_log((C.c_int * 14)(), 1)
        raise
    buf = (C.c_int * (14 * 1024))()
    n = L.pa_conv_launch_log(buf, 1024)
    got = {tuple(buf[14 * i:14 * i + 14]) for i in range(n)}
    assert 0 < n < 1024, (leg, n)
    out = os.environ.get('POSEADV_WRITE_CONV_LAUNCHES')
    if out:
        d = json.load(open(out)) if os.path.isfile(out) else {}
        d[leg] = sorted(set(map(tuple, d.get(leg, []))) | got)
        json.dump(d, open(out, 'w'), indent=0, sort_keys=True)
        return
    want = recorded_launches().get(leg)
    assert want is not None, 'no recorded launches for %r' % leg
    assert set(want) <= got, (leg, sorted(set(want) - got)[:5])
