"""Registers, scratch, LDS and occupancy of every kernel instance of a .hip file, from the compiler (no GPU needed):

    python tools/kernel_resources.py pose_adv_aug_amd/csrc/conv1x1_tile.hip [more.hip ...] [--json] [-D...]

Compiles the device side for gfx950 with the flags of csrc/build.sh plus -Rpass-analysis=kernel-resource-usage and prints one line per
__global__ instance: allocated VGPRs (arch + accumulation registers as the hardware counts them), scratch bytes per lane, LDS bytes per
workgroup, waves per SIMD, and the workgroups per CU that follow for a 256-thread workgroup (one wave per SIMD each) from registers and from
the 160 KB of LDS.  --json: {file: {instance: {...}}} for tests/test_kernel_resources_cpu.py and tests/golden/kernel_resources.json.
Further arguments that start with -D go to the compiler (e.g. -DPA_FP16, '-DPA_CONV1_OCC4(cin,bm,bn,ld)=3')."""
import json
import os
import re
import shutil
import subprocess
import sys

ARCH = 'gfx950'
LDS_PER_CU = 163840
FIELDS = (('VGPRs', 'vgprs'), ('AGPRs', 'agprs'), ('ScratchSize [bytes/lane]', 'scratch'), ('Occupancy [waves/SIMD]', 'waves_per_simd'),
          ('LDS Size [bytes/block]', 'lds'), ('SGPRs Spill', 'sgpr_spill'), ('VGPRs Spill', 'vgpr_spill'))


def _tool(name):
    for cand in (shutil.which(name), os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'bin', name),
                 os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin', name)):
        if cand and os.path.exists(cand):
            return cand
    return None


def _demangle(names):
    filt = _tool('llvm-cxxfilt') or _tool('c++filt')
    if not filt or not names:
        return list(names)
    out = subprocess.run([filt], input='\n'.join(names) + '\n', capture_output=True, text=True, check=True).stdout.splitlines()
    return out if len(out) == len(names) else list(names)


def _short(demangled):
    """'void conv1x1_tile_kernel<128, 64, ...>(PaConvArgs, int)' -> 'conv1x1_tile_kernel<128,64,...>'"""
    s = re.sub(r'^void\s+', '', demangled)
    depth = 0
    for i, ch in enumerate(s):                  # cut the argument list: the first '(' outside the template brackets
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif ch == '(' and depth == 0 and i > 0:
            s = s[:i]
            break
    s = re.sub(r'\((?:int|bool|unsigned int)\)', '', s)
    return s.replace(', ', ',')


def kernel_resources(path, defines=()):
    """{instance: {vgprs, agprs, scratch, lds, waves_per_simd, ...}} of one .hip file."""
    hipcc = _tool('hipcc')
    if not hipcc:
        raise RuntimeError('hipcc not found')
    cmd = [hipcc, '--offload-arch=' + ARCH, '-O3', '-std=c++17', '-fPIC', '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage',
           *defines, '-c', path, '-o', os.devnull]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode:
        raise RuntimeError('%s failed:\n%s' % (' '.join(cmd), p.stderr[-4000:]))
    recs, cur = [], None
    for line in p.stderr.splitlines():
        m = re.search(r'remark: .*Function Name: (\S+)', line)
        if m:
            cur = {'mangled': m.group(1)}
            recs.append(cur)
            continue
        if cur is None:
            continue
        for label, key in FIELDS:
            m = re.search(r'remark: .*\s' + re.escape(label) + r': (\d+)', line)
            if m:
                cur[key] = int(m.group(1))
    names = _demangle([r['mangled'] for r in recs])
    out = {}
    for r, n in zip(recs, names):
        if 'lds' not in r or 'vgprs' not in r:
            continue                            # (device functions that were not inlined carry no kernel record)
        del r['mangled']
        out[_short(n)] = r
    return out


def blocks_per_cu(r, waves_per_block=4):
    """workgroups of waves_per_block waves that fit a CU (4 SIMDs): by registers, by LDS"""
    by_regs = r['waves_per_simd'] * 4 // waves_per_block
    by_lds = LDS_PER_CU // r['lds'] if r['lds'] else 99
    return by_regs, by_lds


def main(argv):
    defines = [a for a in argv if a.startswith('-D')]
    files = [a for a in argv if not a.startswith('-')]
    res = {os.path.basename(f): kernel_resources(f, defines) for f in files}
    if '--json' in argv:
        json.dump(res, sys.stdout, indent=1, sort_keys=True)
        print()
        return
    for f, ks in res.items():
        print('# %s %s' % (f, ' '.join(defines)))
        print('%-92s %5s %5s %7s %7s %10s %12s' % ('instance', 'VGPR', 'AGPR', 'scratch', 'LDS B', 'waves/SIMD', 'wg/CU by LDS'))
        for k in sorted(ks):
            r = ks[k]
            print('%-92s %5d %5d %7d %7d %10d %12d' % (k, r['vgprs'], r['agprs'], r['scratch'], r['lds'], r['waves_per_simd'], blocks_per_cu(r)[1]))


if __name__ == '__main__':
    main(sys.argv[1:])
