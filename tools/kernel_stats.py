"""Kernel statistics of the TIMED region of a rocprofv3 kernel trace of `bench.py --steps 20 --warmup 5` (rocpd database), every kernel listed:
    rocprofv3 --kernel-trace --stats --output-format rocpd -d DIR -o bench -- python bench.py --steps 20 --warmup 5
    python tools/kernel_stats.py DIR "title line" out.txt
The region is found by the optimizer launches (one per step): behind the 5th, up to the 25th."""
import collections, glob, sqlite3, sys
d, title, path = sys.argv[1], sys.argv[2], sys.argv[3]
db = glob.glob('%s/**/*results.db' % d, recursive=True)[0]
rows = list(sqlite3.connect(db).execute('select name, start, end, queue_id from kernels order by start'))
idx = [i for i, r in enumerate(rows) if 'rmsprop' in r[0]]
lo, hi, steps = idx[4] + 1, idx[24] + 1, 20
agg = collections.defaultdict(lambda: [0, 0.0])
for name, s, e, q in rows[lo:hi]:
    a = agg[name.split('(')[0][:110]]; a[0] += 1; a[1] += (e - s) / 1e3
tot = sum(v[1] for v in agg.values())
with open(path, 'w') as f:
    f.write('# %s\n# timed region (20 steps): kernel time %.3f ms/step, %d launches/step\n' % (title, tot / 1e3 / steps, (hi - lo) // steps))
    f.write('# wall time of the region in this (profiled) run: %.3f ms/step\n' % ((rows[idx[24]][2] - rows[idx[4]][2]) / 1e6 / 20))
    f.write('%10s %8s %9s %6s  %s\n' % ('us/step', 'calls/st', 'avg us', '%', 'kernel'))
    for k, (c, us) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        f.write('%10.1f %8.2f %9.2f %6.2f  %s\n' % (us / steps, c / steps, us / c, 100 * us / tot, k))
print('wrote', path)
