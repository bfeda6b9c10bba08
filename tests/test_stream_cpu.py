"""The restated random stream (tests/stream_exact.py) on the host: the published splitmix64 vectors, its statistical quality at sizes only a
CPU affords, the distinctness of every key one training process uses, and the aliasing that makes slots above 255 refusable.

Everything runs on fixed seeds, so each outcome is deterministic.  The thresholds are the statistic's own p = 1e-9 quantile under the
null hypothesis (independent uniforms / standard normals), by the formulas written beside each:
  * z(p): the two-sided normal quantile, erfc(z / sqrt 2) = p (6.109 at 1e-9), found by bisection on math.erfc;
  * chi-square with k = 255 degrees of freedom: Wilson-Hilferty, k (1 - 2/(9k) +- z sqrt(2/(9k)))^3, both tails;
  * a sample correlation of n pairs: |r| sqrt(n) is standard normal to O(1/n), so |r| < z / sqrt(n);
  * the mean of n normals: |m| < z / sqrt(n); their variance: |v - 1| < z sqrt(2 / (n - 1));
  * Kolmogorov-Smirnov: P(D_n > d) <= 2 exp(-2 n d^2) (Dvoretzky-Kiefer-Wolfowitz with Massart's constant), so d = sqrt(ln(2 / p) / (2 n))."""
import math

import numpy as np

from tests import stream_exact as S

P = 1e-9
N = 1 << 20


def z_two_sided(p):
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if math.erfc(mid / math.sqrt(2.0)) > p else (lo, mid)
    return hi


Z = z_two_sided(P)


def chi2_bounds(k, z):
    a = 2.0 / (9.0 * k)
    return k * (1 - a - z * math.sqrt(a)) ** 3, k * (1 - a + z * math.sqrt(a)) ** 3


def corr(a, b):
    a = a - a.mean(); b = b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def axis_uniforms(axis, n=N):
    """n uniforms along one axis of the key with the other three held (at values that are neither 0 nor small)"""
    held = dict(seed=0x1234567, step=77, sample=5, slot=3)
    held[axis] = np.arange(n, dtype=np.uint64)
    return S.uniform(held['seed'], held['step'], held['sample'], held['slot'])


def test_published_splitmix64_vectors():
    """the first two outputs of splitmix64 from state 0: mix64 adds the golden gamma itself, so they are mix64(0) and mix64(gamma)"""
    assert int(S.mix64(0)) == 0xE220A8397B1DCDAF
    assert int(S.mix64(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4
    # wrapping arithmetic on arrays and the top half of both 64-bit arguments
    assert int(S.mix64(np.array([0xFFFFFFFFFFFFFFFF], dtype=np.uint64))[0]) == int(S.mix64(0xFFFFFFFFFFFFFFFF))
    u = S.uniform(2 ** 63 + 11, 2 ** 32 + 5, 3, 7)
    assert u.dtype == np.float64 and 0.0 < float(u) <= 1.0
    assert float(u) != float(S.uniform(11, 2 ** 32 + 5, 3, 7)) and float(u) != float(S.uniform(2 ** 63 + 11, 5, 3, 7))


def test_uniform_rounds_like_the_kernel():
    """((k >> 11) + 0.5) 2^-53: exact below 2^52, ties to even above, 1.0 at the top"""
    def u_of_bits(n):
        return float((np.array([n], dtype=np.uint64).astype(np.float64) + 0.5)[0] * S.TWO_M53)
    assert u_of_bits(0) == 2.0 ** -54
    assert u_of_bits(2 ** 52 - 1) == (2 ** 53 - 1) * 2.0 ** -54
    assert u_of_bits(2 ** 52 + 1) == (2 ** 52 + 2) * 2.0 ** -53          # odd: the tie goes up to the even neighbour
    assert u_of_bits(2 ** 52 + 2) == (2 ** 52 + 2) * 2.0 ** -53          # even: the tie goes down
    assert u_of_bits(2 ** 53 - 1) == 1.0


def test_uniform_quality_along_every_key_axis():
    lo, hi = chi2_bounds(255, Z)
    for axis in ('seed', 'step', 'sample', 'slot'):
        u = axis_uniforms(axis)
        assert u.min() > 0.0 and u.max() <= 1.0
        counts = np.bincount(np.minimum((u * 256).astype(np.int64), 255), minlength=256)
        chi2 = float(((counts - N / 256.0) ** 2).sum() / (N / 256.0))
        r1 = corr(u[:-1], u[1:])
        print('%-6s chi2 %.1f in (%.1f, %.1f)   lag-1 r %.2e, bound %.2e' % (axis, chi2, lo, hi, r1, Z / math.sqrt(N - 1)))
        assert lo < chi2 < hi, (axis, chi2)
        assert abs(r1) < Z / math.sqrt(N - 1), (axis, r1)


def test_normal_quality():
    b = np.arange(N, dtype=np.uint64)
    z, R = S.normal(0x1234567, 77, b, 0)
    u2 = S.uniform(0x1234567, 77, b, 1)
    z = z.astype(np.float64)
    c = np.cos(2 * np.pi * u2)
    bound = Z / math.sqrt(N)
    # the two halves of Box-Muller (the radius from slot 0, the angle from slot 1) and the two normals of one sample (slots 0-1, 2-3)
    z2, _ = S.normal(0x1234567, 77, b, 2)
    r_halves, r_pair = corr(R.astype(np.float64), c), corr(z, z2.astype(np.float64))
    mean, var = float(z.mean()), float(z.var(ddof=1))
    zs = np.sort(z)
    cdf = 0.5 * _erfc(-zs / math.sqrt(2.0))
    i = np.arange(1, N + 1, dtype=np.float64)
    ks = float(max((i / N - cdf).max(), (cdf - (i - 1) / N).max()))
    ks_bound = math.sqrt(math.log(2.0 / P) / (2.0 * N))
    print('halves r %.2e pair r %.2e (bound %.2e)  mean %.2e (bound %.2e)  var-1 %.2e (bound %.2e)  KS %.2e (bound %.2e)'
          % (r_halves, r_pair, bound, mean, bound, var - 1, Z * math.sqrt(2.0 / (N - 1)), ks, ks_bound))
    assert abs(r_halves) < bound and abs(r_pair) < bound
    assert abs(mean) < bound
    assert abs(var - 1.0) < Z * math.sqrt(2.0 / (N - 1))
    assert ks < ks_bound


def _erfc(x):
    """erfc on an array: math.erfc on the float64 values (NumPy has none of its own)"""
    return np.frompyfunc(math.erfc, 1, 1)(x).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# every key of one training process
RANKS = range(8)
AUG_SEEDS = [1234 + r for r in RANKS] + [4242 + r for r in RANKS] + [4321]      # stack_hg, joint_train_pose_s_r_agent, pretrain_s_r_agent
JOINT_SEEDS = [4242 + r for r in RANKS]
EPOCHS = range(256)
MASK_SEEDS = [0] + AUG_SEEDS       # sample_mask's default seed, and a caller that hands over its augmenter's


def consumers(bins_hg, bins_agent, epochs=EPOCHS):
    """(name, seed, slot) of every consumer of the stream; each draws at every (step, sample)"""
    out = [('aug', s, sl) for s in AUG_SEEDS for sl in S.AUG_SLOT_LIST]
    out += [('mask', s, sl) for s in MASK_SEEDS for sl in S.MASK_SLOTS]
    for e in epochs:
        for a in JOINT_SEEDS:
            out += [('train_hg bins e%d' % e, S.bin_seed(e, a), sl) for sl in bins_hg]
            out += [('train_agent bins e%d' % e, S.bin_seed(e, a), sl) for sl in bins_agent]
    return out


def duplicate_seed_slots(cons):
    pairs = np.array([(s, sl) for _, s, sl in cons], dtype=np.uint64)
    packed = np.zeros(len(pairs), dtype=[('seed', 'u8'), ('slot', 'u8')])
    packed['seed'], packed['slot'] = pairs[:, 0], pairs[:, 1]
    uniq, first, counts = np.unique(packed, return_index=True, return_counts=True)
    dup = uniq[counts > 1]
    return [[c[0] for c in cons if c[1] == int(d['seed']) and c[2] == int(d['slot'])] for d in dup[:4]], int((counts > 1).sum())


def test_slot_map_is_the_loops():
    from pose_adv_aug_amd import joint_train_pose_s_r_agent as J

    class A(object):
        seed = 4245
    assert tuple(J.BIN_SLOTS_TRAIN_HG) == S.BIN_SLOTS_TRAIN_HG and tuple(J.BIN_SLOTS_TRAIN_AGENT) == S.BIN_SLOTS_TRAIN_AGENT
    for e in (0, 1, 255, 2 ** 40):
        assert J._bin_seed(e, A()) == S.bin_seed(e, 4245)
    used = set(S.AUG_SLOT_LIST) | set(S.MASK_SLOTS)
    bins = S.BIN_SLOTS_TRAIN_HG + S.BIN_SLOTS_TRAIN_AGENT
    assert len(set(bins)) == 4 and not (set(bins) & used) and max(bins) <= 255


def test_every_key_of_a_training_process_is_distinct():
    """No two (consumer, step, sample, slot) tuples map to one (seed, key) pair, over steps 0-4095, samples 0-63, every slot of the map,
    the augmenter seeds of ranks 0-7 and _bin_seed of epochs 0-255.  The key does not depend on the seed and every consumer ranges over
    the same steps and samples, so the full set of pairs (4.5e9) factors: (a) the key is injective over steps x samples x the map's
    slots (np.unique over all 2.0e7 keys), and then two pairs coincide exactly when two consumers share (seed, slot) -- (b) np.unique
    over those pairs.  (c) the pairs themselves, literally, on a sub-grid (steps 0-255, samples 0-7, epochs 0-7).
    With the bin draws on slots 0 / 1 (where they were) (b) fails at epoch 0: _bin_seed(0, a) is the augmenter's seed."""
    slots = np.array(sorted(set(S.AUG_SLOT_LIST) | set(S.MASK_SLOTS) | set(S.BIN_SLOTS_TRAIN_HG) | set(S.BIN_SLOTS_TRAIN_AGENT)), dtype=np.uint64)
    steps = np.arange(4096, dtype=np.uint64)
    samples = np.arange(64, dtype=np.uint64)
    keys = S.key(steps[:, None, None], samples[None, :, None], slots[None, None, :]).ravel()
    assert np.unique(keys).size == keys.size == 4096 * 64 * slots.size                       # (a)
    cons = consumers(S.BIN_SLOTS_TRAIN_HG, S.BIN_SLOTS_TRAIN_AGENT)
    names, n_dup = duplicate_seed_slots(cons)
    assert n_dup == 0, names                                                                 # (b)
    # the negative control: the slots the bin draws had before
    names, n_dup = duplicate_seed_slots(consumers((0, 1), (0, 1), epochs=range(1)))
    assert n_dup > 0 and any('aug' in n and 'train_hg bins e0' in n for n in names), names
    # (c) literal (seed, key) pairs on a sub-grid
    sub = S.key(np.arange(256, dtype=np.uint64)[:, None], np.arange(8, dtype=np.uint64)[None, :], 0).ravel()
    cons = consumers(S.BIN_SLOTS_TRAIN_HG, S.BIN_SLOTS_TRAIN_AGENT, epochs=range(8))
    packed = np.zeros(len(cons) * sub.size, dtype=[('seed', 'u8'), ('key', 'u8')])
    packed['seed'] = np.repeat(np.array([c[1] for c in cons], dtype=np.uint64), sub.size)
    packed['key'] = (sub[None, :] + np.array([c[2] for c in cons], dtype=np.uint64)[:, None]).ravel()
    assert np.unique(packed).size == packed.size


def test_slot_256_aliases_the_next_sample():
    """the reason pa_sample_categorical refuses slot > 255: the key holds the slot in 8 bits"""
    b = np.arange(64, dtype=np.uint64)
    for seed, step in ((0, 0), (7, 3), (2 ** 63 + 11, 2 ** 32 + 5)):
        for j in (0, 1, 17, 255):
            assert np.array_equal(S.uniform(seed, step, b, 256 + j), S.uniform(seed, step, b + np.uint64(1), j))
            assert not np.array_equal(S.uniform(seed, step, b, j), S.uniform(seed, step, b + np.uint64(1), j))


def test_categorical_pick_is_the_normalised_rule():
    """first cell whose running sum exceeds u * total; never a cell of probability 0; edges belong to the upper cell"""
    p = np.array([[0.25, 0.0, 0.5, 0.25 - 1e-7, 0.0]])
    total = float(np.cumsum(p[0])[-1])
    for u, want in ((0.0, 0), (0.2499, 0), (0.25 / total, 2), (0.5, 2), (0.74, 2), (0.76, 3), (1.0 - 1e-12, 3), (1.0, 3)):
        assert int(S.categorical_pick(p, [u])[0]) == want, (u, want)
    st, us = S.find_keys(11, 0, 0.5, 0.5 + 1e-6, 1 << 22)
    assert st.size > 0 and np.all((us >= 0.5) & (us < 0.5 + 1e-6)) and np.array_equal(us, S.uniform(11, st, 0, 0))
    (below, above), = S.nearest_keys(11, 0, [0.5], 1 << 22)
    assert below[1] < 0.5 <= above[1] and float(S.uniform(11, below[0], 0, 0)) == below[1] and above[1] == us.min()
