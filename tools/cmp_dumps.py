"""Compare two `bench.py --dump-outputs` directories array by array, bit for bit:  python tools/cmp_dumps.py DIR_A DIR_B"""
import glob, os, sys
import numpy as np
a, b = sys.argv[1], sys.argv[2]
names = sorted(os.path.basename(f) for f in glob.glob(a + '/*.npy'))
assert names and names == sorted(os.path.basename(f) for f in glob.glob(b + '/*.npy')), (names, os.listdir(b))
bad = 0
for n in names:
    x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
    same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
    print('%-22s %-18s %-8s %s' % (n, x.shape, x.dtype, 'bitwise equal' if same else 'DIFFERS (max abs %.3e)' % float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max())))
    bad += not same
print('ALL EQUAL' if not bad else '%d arrays differ' % bad)
