"""CPU model of the per-tile bucket sort's bin arithmetic (binning.hip bucket_sort_list / bucket_sort_long).

The kernels cut a tile's key range [min, max] into at most NBMAX equal bins (about two keys per bin), count the
keys per bin and give the list to a bitonic network instead -- their fallback -- when the bins are badly skewed:
sum(bin size^2) > kSkew * n.  This module restates that arithmetic (``bin_shift``, ``bin_counts``,
``skew_rejected``) on keys formed as the kernels form them (``make_keys``: float32 depth bits << 32 |
Gaussian << 4), so a test can prove from the oracle's lists alone which tiles of a scene take a fallback, and
keeps the windowed long-list model (``bucket_sort_long_model``, tests/test_bucket_long_model.py).

Bins per kernel (NBMAX) and the list lengths each takes:
    tile_sort_kernel                  512     129..1024 keys
    prefix and window kernels         2048    over 1024 keys, any length
    tile_sort_full_kernel (the redo)  4096    up to 8192 keys (longer lists: the global-memory network at once)
"""
import random

import numpy as np

K_BIN_SHIFT = 1
K_SKEW = 48
K_SKEW_BIN_MAX = 1 << 15  # bucket_sort_long counts a bin as this many keys at most (kSkewBinMax)

NB_WAVE = 512    # tile_sort_kernel: BucketLds<kSortT, kSortWaveMax, kSortWaveMax / 2>
NB_LONG = 2048   # tile_sort_prefix_kernel, tile_sort_window_kernel: kPrefixBins
NB_FULL = 4096   # tile_sort_full_kernel: kBucketMax / 2
WAVE_MIN, WAVE_MAX = 129, 1024  # tile_sort_kernel bucket-sorts lists of kBucketMinN < n <= kSortWaveMax keys
FULL_MAX = 8192                 # kBucketMax


def make_keys(depths, gaussians) -> np.ndarray:
    """uint64 keys of (float32 depth, Gaussian index) pairs as K3 writes them."""
    bits = np.ascontiguousarray(depths, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | (np.asarray(gaussians).astype(np.uint64) << np.uint64(4))


def tile_keys(depths, point_list, ranges):
    """The key list of every tile, from the oracle's geom()["depths"] and binning()."""
    keys = make_keys(np.asarray(depths)[point_list], point_list)
    return [keys[int(a):int(b)] for a, b in ranges]


def bin_shift(n, mn, mx, nbmax):
    """(sh, nb) of a list of n keys in [mn, mx]: a key's bin is (key - mn) >> sh, nb <= 2^lg bins in all,
    2^lg = the power of two >= n >> kBinShift, at most nbmax."""
    lg = 0
    while (1 << lg) < (n >> K_BIN_SHIFT) and (1 << lg) < nbmax:
        lg += 1
    span = int(mx) - int(mn)
    bits = span.bit_length() if span else 0
    sh = bits - lg if bits > lg else 0
    return sh, (span >> sh) + 1


def bin_counts(keys, nbmax) -> np.ndarray:
    """The bin sizes (int64 [nb]) the kernels count for this list."""
    keys = np.asarray(keys, dtype=np.uint64)
    mn, mx = keys.min(), keys.max()
    sh, nb = bin_shift(len(keys), mn, mx, nbmax)
    b = ((keys - mn) >> np.uint64(sh)).astype(np.int64)
    return np.bincount(b, minlength=nb)


def skew_rejected(keys, nbmax, wrap32=False, bin_max=None) -> bool:
    """sum(bin size^2) > kSkew * n: the list goes to the fallback network.  wrap32: the squares and their sum
    taken mod 2^32, as a kernel that accumulates them in uint32 computes them (a bin of 65536 keys adds 0);
    bin_max: a bin counts as at most this many keys.  wrap32 with bin_max = K_SKEW_BIN_MAX is bucket_sort_long's
    arithmetic; wrap32 alone is what it computed before it clamped the bins."""
    v = [int(x) if bin_max is None else min(int(x), bin_max) for x in bin_counts(keys, nbmax)]
    if wrap32:
        total = 0
        for x in v:
            total = (total + ((x * x) & 0xFFFFFFFF)) & 0xFFFFFFFF
    else:
        total = sum(x * x for x in v)
    return total > K_SKEW * len(keys)


def bucket_sort_long_model(keys, nmax=2048, nbmax=2048, threads=256, rng=None, lim=None):
    """Returns the sorted list -- in prefix mode (lim) (its first `sorted` entries, sorted) -- or None where the
    kernel reports failure (skew, or one bin over the buffer)."""
    rng = rng or random.Random(0)
    n = len(keys)
    mn, mx = min(keys), max(keys)
    sh, nb = bin_shift(n, mn, mx, nbmax)
    per = (nb + threads - 1) // threads
    start = [0] * (per * threads + 2)
    for k in keys:
        start[(k - mn) >> sh] += 1
    if sum(v * v for v in start[:nb]) > K_SKEW * n:
        return None
    at = 0
    for b in range(per * threads):
        v = start[b]
        start[b] = at
        at += v
    start[nb] = n
    out = [None] * n
    bw0 = w0 = 0
    lim = n if lim is None else lim
    while w0 < n and w0 < lim:
        cut = w0 + nmax
        w1 = cut if cut < n else n
        if cut < n:
            for b in range(bw0, nb):
                if start[b] < cut < start[b + 1]:
                    w1 = min(w1, start[b])
        if w1 <= w0:
            return None
        bw1 = min([b for b in range(bw0, nb) if start[b] >= w1], default=nb)
        buf = [None] * nmax
        order = list(range(n))
        rng.shuffle(order)  # the atomics' arrival order is arbitrary
        for i in order:
            k = keys[i]
            b = (k - mn) >> sh
            if bw0 <= b < bw1:
                buf[start[b] - w0] = k
                start[b] += 1
        for j in range(w1 - w0):
            kj = buf[j]
            b = (kj - mn) >> sh
            st = (start[b - 1] if b else 0) - w0
            en = start[b] - w0
            c = sum(1 for q in range(st, en) if buf[q] < kj)
            out[w0 + st + c] = kj
        w0, bw0 = w1, bw1
    return out if lim >= n else (out[:w0], w0)
