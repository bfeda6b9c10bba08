"""The engine's counter-based random stream (pa_mix64 / pa_uniform / pa_normal, csrc/pose_ops.hip) restated on the host, bit for bit.

The stream is integer arithmetic (splitmix64's output function, wrapping modulo 2^64) and one exact float64 product, so NumPy computes
the very uniform the device draws for any key (seed, step, sample, slot):

    key     = step * 0x100000001B3 + (sample << 8) + slot                 (uint64, wrapping)
    k       = mix64(seed ^ mix64(key))
    uniform = (float64(k >> 11) + 0.5) * 2^-53

k >> 11 < 2^53 converts exactly.  The + 0.5 is exact below 2^52 and ties to even from there on (the spacing of float64 is 1), so the
result lies in (0, 1] and is exactly 1.0 for the one value k >> 11 == 2^53 - 1 (probability 2^-53): NumPy's float64 add rounds the same
way.  The normal is Box-Muller of the uniforms of (slot, slot + 1); a device evaluates log, sqrt and cos in float64 to a few ulp, so the
restatement gives it in np.longdouble (64-bit mantissa on x86) together with R = sqrt(-2 ln u1), the scale of that error
(tests/test_gpu_stream.py brackets the device's value with it).

Host only: NumPy and oracle.model (its inverse-CDF rule); neither a GPU nor the library is imported."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MUL1 = np.uint64(0xBF58476D1CE4E5B9)
MUL2 = np.uint64(0x94D049BB133111EB)
STEP_MUL = np.uint64(0x100000001B3)
TWO_M53 = 2.0 ** -53

# ---------------------------------------------------------------------------------------------------------------------------------
# the slot map: which slot of a (seed, step, sample) key each consumer draws from.  A slot is 8 bits wide (0..255).
AUG_SLOTS = {
    'scale_normal': (0, 1),        # pa_normal(slot 0): u1 = slot 0, u2 = slot 1
    'rot_normal': (2, 3),
    'rot_zero': 4,                 # regular law: rotation forced to 0 when u <= 0.6
    'flip': 5,                     # u <= 0.5
    'gain': (6, 7, 8),             # 0.6 + (1.4 - 0.6) u per channel
}
MASK_SLOT0 = 16                    # pa_sample_dropout_masks: draw j of a sample is slot 16 + j, j < dropout_num < cells <= 64
MASK_SLOTS = tuple(range(16, 80))
BIN_SLOTS_TRAIN_HG = (96, 97)      # joint_train_pose_s_r_agent.train_hg_step: scale bin, rotation bin
BIN_SLOTS_TRAIN_AGENT = (98, 99)   # joint_train_pose_s_r_agent.train_agent_sr: scale bin, rotation bin
AUG_SLOT_LIST = tuple(range(9))


def bin_seed(epoch, augmenter_seed):
    """joint_train_pose_s_r_agent._bin_seed"""
    return (int(epoch) * 1000003 + int(augmenter_seed)) & 0x7fffffffffffffff


def _u64(x):
    """x (Python ints of any size below 2^64, or an integer array) as a uint64 array"""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    if isinstance(x, (list, tuple, range)):
        return np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in x], dtype=np.uint64)
    return np.array(int(x) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)


def mix64(z):
    """splitmix64's output function of the state z + golden gamma (pa_mix64), wrapping modulo 2^64"""
    with np.errstate(over='ignore'):
        z = _u64(z) + GOLDEN
        z = (z ^ (z >> np.uint64(30))) * MUL1
        z = (z ^ (z >> np.uint64(27))) * MUL2
        return z ^ (z >> np.uint64(31))


def key(step, sample, slot):
    """the 64-bit counter of a draw; sample and slot are the kernel's 32-bit unsigned arguments widened to 64 bits"""
    with np.errstate(over='ignore'):
        return _u64(step) * STEP_MUL + (_u64(sample) << np.uint64(8)) + _u64(slot)


def uniform_of_key(seed, k):
    bits = mix64(_u64(seed) ^ mix64(k))
    return ((bits >> np.uint64(11)).astype(np.float64) + 0.5) * TWO_M53


def uniform(seed, step, sample, slot):
    """pa_uniform: float64, the device's value bit for bit.  The arguments broadcast."""
    return uniform_of_key(seed, key(step, sample, slot))


def normal(seed, step, sample, slot):
    """pa_normal in np.longdouble: (z, R) with z = R cos(2 pi u2), R = sqrt(-2 ln u1), u1 / u2 the uniforms of slot / slot + 1"""
    u1 = uniform(seed, step, sample, slot).astype(np.longdouble)
    u2 = uniform(seed, step, sample, _u64(slot) + np.uint64(1)).astype(np.longdouble)
    R = np.sqrt(np.longdouble(-2) * np.log(u1))
    two_pi = np.longdouble(8) * np.arctan(np.longdouble(1))
    return R * np.cos(two_pi * u2), R


def aug_draws(seed, step, B):
    """the [B][7] float64 block pa_sample_aug_given takes ({N scale, N rotation, U rotation-forced-to-0, U flip, U gain x 3}) from the
    restated stream; the two normals rounded to float64 from the longdouble value.  Also returns (z, R) of both normals in longdouble."""
    b = np.arange(B, dtype=np.uint64)
    zs, Rs = normal(seed, step, b, AUG_SLOTS['scale_normal'][0])
    zr, Rr = normal(seed, step, b, AUG_SLOTS['rot_normal'][0])
    d = np.empty((B, 7), dtype=np.float64)
    d[:, 0], d[:, 1] = zs.astype(np.float64), zr.astype(np.float64)
    d[:, 2] = uniform(seed, step, b, AUG_SLOTS['rot_zero'])
    d[:, 3] = uniform(seed, step, b, AUG_SLOTS['flip'])
    for c, s in enumerate(AUG_SLOTS['gain']):
        d[:, 4 + c] = uniform(seed, step, b, s)
    return d, (zs, Rs), (zr, Rr)


def categorical_pick(probs, u):
    """np.random.choice(K, p=probs) as the inverse CDF of the float64 running sum NORMALISED by its last entry: the first cell whose
    cdf exceeds u * total, else the last cell of positive probability (oracle.model.sample_cells_inverse_cdf with one draw)."""
    from oracle.model import sample_cells_inverse_cdf
    probs = np.asarray(probs, dtype=np.float64)
    return sample_cells_inverse_cdf(probs, np.asarray(u, dtype=np.float64).reshape(-1, 1))[:, 0]


def find_keys(seed, slot, lo, hi, n_keys, chunk=1 << 16):
    """the steps in [0, n_keys), at sample 0, whose uniform lies in [lo, hi): (steps uint64, uniforms float64), ascending in step.
    With sequences lo, hi: a list of such pairs, one per interval, from one pass over the keys.  Searched in cache-sized chunks."""
    many = np.ndim(lo) > 0
    los, his = (list(lo), list(hi)) if many else ([lo], [hi])
    steps, us = [[] for _ in los], [[] for _ in los]
    for s0 in range(0, int(n_keys), chunk):
        st = np.arange(s0, min(s0 + chunk, int(n_keys)), dtype=np.uint64)
        u = uniform(seed, st, 0, slot)
        for n, (a, b) in enumerate(zip(los, his)):
            hit = np.nonzero((u >= a) & (u < b))[0]
            if hit.size:
                steps[n].append(st[hit]); us[n].append(u[hit])
    out = [(np.concatenate(a), np.concatenate(b)) if a else (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.float64))
           for a, b in zip(steps, us)]
    return out if many else out[0]


def nearest_keys(seed, slot, edges, n_keys, window=1e-6, chunk=1 << 16):
    """over the steps in [0, n_keys) at sample 0, for every edge: ((step, u) of the largest uniform < edge, (step, u) of the smallest
    uniform >= edge), looked for within `window` of the edge ((None, -inf) / (None, inf) when there is none).  One pass over the keys
    for all edges."""
    edges = [float(e) for e in edges]
    below = [(None, -np.inf)] * len(edges)
    above = [(None, np.inf)] * len(edges)
    for s0 in range(0, int(n_keys), chunk):
        st = np.arange(s0, min(s0 + chunk, int(n_keys)), dtype=np.uint64)
        u = uniform(seed, st, 0, slot)
        for n, e in enumerate(edges):
            for i in np.nonzero(np.abs(u - e) < window)[0]:
                if u[i] < e and u[i] > below[n][1]:
                    below[n] = (int(st[i]), float(u[i]))
                if u[i] >= e and u[i] < above[n][1]:
                    above[n] = (int(st[i]), float(u[i]))
    return list(zip(below, above))
