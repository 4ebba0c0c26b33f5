"""What the depth-layer scenes (tests/common.py DEPTH_CASES) reach, proved from the references alone.

tests/test_gpu_depth_skew.py holds the GPU to the oracle on scenes whose depths cluster, tie or span the whole
key range.  A right result there says something about the bucket sort's fallbacks (binning.hip: sort_list<64, E>,
sort_list<256, 16>, sort_list_global) only if the scene sends lists to them, so this module asserts, from the f32
oracle's tile lists and depths and the bin model (tests/sort_model.py) and without a GPU, that
  * every list-length class a scene names has tiles the model rejects for skew (all of its lists lie in that class,
    so a rejected tile takes that class's network);
  * moderate_pass is rejected nowhere and ranks a bin of at least 256 keys;
  * hot_bin_65536 has one bin of exactly 2^16 keys, which the skew test sees only when it does not wrap at 2^32;
  * the fg_wall scenes' near-first cut (a float64 restatement of the depth-mass histogram) falls between the
    foreground and the wall and leaves every tile a near list shorter than its walk;
  * depth_extremes has visible Gaussians in the first and the last depth bin;
  * the f32 oracle agrees with the f64 oracle at every pixel (no rounding flip), so the GPU tests' exact bars hold
    without a flip rule.
Measured (tiles rejected of tiles, list lengths): wall_129_256 11 of 16, 129..204; wall_257_512 16 of 16, 399..498;
wall_513_1024 16 of 16, 829..962; wall_class0_1k 4 of 4, 1027..1230; wall_class0_3k 4 of 4, 2858..3205;
wall_class1 1 of 1, 10000; wall_equal 4 of 4; moderate_pass 0 of 4, largest bin 319; hot_bin_65536 1 of 1, 65544;
fg_wall_4k 4 of 4, 2585..2918; fg_wall_8k 4 of 4, 4593..5232; depth_extremes 0 of 4, 2446..2647."""
import numpy as np
import pytest

from tests import common as C
from tests import sort_model as M

# name -> (shortest list, longest list, bins of the kernel that takes such lists first, tiles rejected there)
CLASSES = {
    "wall_129_256": (129, 256, M.NB_WAVE, 1),     # rejected: sort_list<64, 4>
    "wall_257_512": (257, 512, M.NB_WAVE, 16),    # sort_list<64, 8>
    "wall_513_1024": (513, 1024, M.NB_WAVE, 16),  # sort_list<64, 16>
    "wall_class0_1k": (1025, 2048, M.NB_LONG, 4),  # sort_list_global behind bucket_sort_list (prefix / window mode)
    "wall_class0_3k": (2049, 4096, M.NB_LONG, 4),
    "wall_class1": (8193, 1 << 30, M.NB_LONG, 1),  # sort_list_global behind bucket_sort_long
    "wall_equal": (2049, 4096, M.NB_LONG, 4),
    "moderate_pass": (2049, 4096, M.NB_LONG, 0),
    "hot_bin_65536": (65544, 65544, M.NB_LONG, 1),
    "fg_wall_4k": (2049, 4096, M.NB_FULL, 4),     # the redo: sort_list<256, 16>
    "fg_wall_8k": (4097, 8192, M.NB_FULL, 4),     # the redo: sort_list_global
    "depth_extremes": (2049, 4096, M.NB_LONG, 0),
}


def rejected_tiles(keys, nbmax):
    return np.array([len(k) > 1 and M.skew_rejected(k, nbmax) for k in keys])


def test_every_case_is_classified():
    assert sorted(CLASSES) == sorted(c.name for c in C.DEPTH_CASES)


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_case_reaches_its_path(name):
    case, inp, ref, keys = C.depth_reference(name)
    lo, hi, nbmax, min_rejected = CLASSES[name]
    n = np.array([len(k) for k in keys])
    assert lo <= n.min() and n.max() <= hi, (n.min(), n.max())
    rej = rejected_tiles(keys, nbmax)
    largest = max(int(M.bin_counts(k, nbmax).max()) for k in keys)
    print(f"[{name}] {len(n)} tiles of {n.min()}..{n.max()} keys, {int(rej.sum())} rejected at {nbmax} bins, "
          f"largest bin {largest}")
    if min_rejected:
        assert rej.sum() >= min_rejected, int(rej.sum())
    else:
        assert not rej.any()
    # the image and n_contrib of the f32 oracle are those of the f64 oracle: exact bars need no flip rule
    assert C.rounding_flip_caps(inp, ref)[2] == (0, 0)
    # depth is world z exactly under the identity camera
    vis = ref.radii > 0
    np.testing.assert_array_equal(ref.handle.geom()["depths"][vis], inp["means3D"][:, 2].numpy()[vis])


def test_long_walls_are_rejected_in_every_sort_mode():
    """A long list meets the bucket sort with 2048 bins in the prefix and window kernels and with 4096 in the redo
    and inspection kernel: the wall scenes are rejected by both."""
    for name in ("wall_class0_1k", "wall_class0_3k", "wall_equal", "fg_wall_4k", "fg_wall_8k"):
        keys = C.depth_reference(name)[3]
        assert rejected_tiles(keys, M.NB_LONG).all() and rejected_tiles(keys, M.NB_FULL).all(), name


def test_clamped_skew_sum_decides_as_the_exact_sum():
    """bucket_sort_long's sum (32 bits, bins counted as 2^15 keys at most) against the exact one on every long list
    of these scenes, and on lists of under 2^17 keys with a bin of 2^15 .. 2^16 keys, where it cannot wrap."""
    for c in C.DEPTH_CASES:
        for k in C.depth_reference(c.name)[3]:
            if len(k) > 1024:
                assert (M.skew_rejected(k, M.NB_LONG, wrap32=True, bin_max=M.K_SKEW_BIN_MAX)
                        == M.skew_rejected(k, M.NB_LONG)), c.name
    rng = np.random.default_rng(0)
    for hot in (1 << 15, 40000, (1 << 16) - 1, 1 << 16, (1 << 16) + 1):
        n = min(hot + int(rng.integers(8, 60000)), (1 << 17) - 1)
        depths = np.concatenate([np.full(hot, 5.0), rng.uniform(2.0, 50.0, n - hot)]).astype(np.float32)
        keys = M.make_keys(depths, rng.permutation(n))
        assert M.bin_counts(keys, M.NB_LONG).max() >= hot
        assert M.skew_rejected(keys, M.NB_LONG) and M.skew_rejected(keys, M.NB_LONG, wrap32=True,
                                                                    bin_max=M.K_SKEW_BIN_MAX)


def test_moderate_pass_ranks_a_long_bin():
    keys = C.depth_reference("moderate_pass")[3]
    for nbmax in (M.NB_LONG, M.NB_FULL):
        assert not rejected_tiles(keys, nbmax).any()
    assert max(int(M.bin_counts(k, M.NB_LONG).max()) for k in keys) >= 256


def test_wall_equal_is_ordered_by_index():
    """9 distinct depths among the visible Gaussians: inside a run of equal depth the oracle's list is in index
    order, which only the low key bits carry."""
    case, inp, ref, keys = C.depth_reference("wall_equal")
    depths = ref.handle.geom()["depths"]
    assert len(np.unique(depths[ref.radii > 0])) <= 16
    for k in keys:
        assert (np.diff(k.astype(np.uint64)) > 0).all()  # the oracle's order is the keys' order
        d = k >> np.uint64(32)
        runs = np.diff(np.flatnonzero(np.concatenate([[True], d[1:] != d[:-1], [True]])))
        assert runs.max() >= 2048, int(runs.max())


def test_hot_bin_wraps_the_32_bit_skew_sum():
    case, inp, ref, keys = C.depth_reference("hot_bin_65536")
    assert len(keys) == 1 and len(keys[0]) == 65536 + 8
    counts = M.bin_counts(keys[0], M.NB_LONG)
    assert counts.max() == 65536 and np.count_nonzero(counts) >= 3
    # its square is 0 mod 2^32: a sum kept in uint32 passes the skew test, the exact sum rejects the list
    assert not M.skew_rejected(keys[0], M.NB_LONG, wrap32=True)
    assert M.skew_rejected(keys[0], M.NB_LONG)
    # ... and so does the kernel's 32-bit sum over bins counted as 2^15 keys at most
    assert M.skew_rejected(keys[0], M.NB_LONG, wrap32=True, bin_max=M.K_SKEW_BIN_MAX)
    # keys lie in front of the hot bin, so a windowed sort writes them before it meets the bin that fits no window
    assert 0 < counts[:int(counts.argmax())].sum() < 2048


@pytest.mark.parametrize("name", ["fg_wall_4k", "fg_wall_8k"])
def test_fg_wall_cut_falls_in_front_of_the_wall(name):
    """The near-first cut at near_mass = 1, restated in float64 (the library sums a fixed-point mass; the GPU test
    asserts the cut it made): the depth bin at which the screen-averaged opacity mass reaches 1."""
    case, inp, ref, keys = C.depth_reference(name)
    g = ref.handle.geom()
    conic, op = g["conic_opacity"][:, :3].astype(np.float64), g["conic_opacity"][:, 3].astype(np.float64)
    det_inv = conic[:, 0] * conic[:, 2] - conic[:, 1] ** 2
    vis = (ref.radii > 0) & (det_inv > 0)
    mass = np.where(vis, op * 2 * np.pi / np.sqrt(np.maximum(det_inv, 1e-30)), 0.0)
    zb = C.zbin_of(g["depths"])
    hist = np.bincount(zb[vis], weights=mass[vis], minlength=256)
    cut = int(np.argmax(np.cumsum(hist) >= 1.0 * case.W * case.H))
    wall = int(C.zbin_of(np.array([5.0], np.float32))[0])
    assert np.cumsum(hist)[-1] >= case.W * case.H and cut < wall, (cut, wall)
    assert hist[wall] > 0.9 * hist.sum()  # nearly all of the histogram's mass in one bin
    nc = ref.handle.image()["n_contrib"].astype(np.int64)
    rb = ref.handle.binning()
    gx = (case.W + 15) // 16
    n = np.array([len(k) for k in keys])
    assert n.mean() >= 2048  # api.hip kNearMinMeanList: the cut applies
    for t, (a, b) in enumerate(rb["ranges"]):
        near = int((zb[rb["point_list"][int(a):int(b)]] <= cut).sum())
        ty, tx = divmod(t, gx)
        walk = int(nc[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].max())
        print(f"[{name}] tile {t}: cut bin {cut} (wall {wall}), near list {near} of {b - a}, longest walk {walk}")
        assert 0 < near < walk


def test_depth_extremes_reaches_both_zbin_clamps():
    case, inp, ref, keys = C.depth_reference("depth_extremes")
    d = ref.handle.geom()["depths"][ref.radii > 0]
    zb = C.zbin_of(d)
    assert zb.min() == 0 and zb.max() == 255
    assert d.max() > 0.2 * 2.0 ** 16  # beyond the last bin's own range: the upper clamp acts
    span = max(int(k.max()) - int(k.min()) for k in keys)
    assert span.bit_length() >= 32 + 27  # depths over more than 16 octaves: the widest key range the sort shifts
