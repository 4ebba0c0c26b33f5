"""The tile sort on skewed, tied and extreme depth distributions (tests/common.py DEPTH_CASES) against the oracle.

Every other scene of the suite draws depth uniformly, which the per-tile bucket sort (binning.hip) is tuned for:
its fallbacks -- the one-wave register networks sort_list<64, 4 | 8 | 16>, sort_list<256, 16> with its LDS
exchange, and the global-memory network sort_list_global, which one call site runs after bucket_sort_long has
written part of the list -- take over only when a tile's depths cluster in a sliver of their range.  These scenes
do that: a wall seen head-on with a few floaters in front and behind, at every list-length class; the same wall at
one exact depth, ordered by the Gaussian index alone; a bin of exactly 2^16 keys, whose square is 0 in 32 bits;
a moderately clustered scene that stays in the bucket sort and ranks a long bin; a thin foreground before a wall,
where the near-first cut's histogram has nearly all its mass in one bin and every tile is redone; and depths over
the whole range of the cut's depth bins.  tests/test_depth_skew_ref.py proves without a GPU that each scene
reaches what it is meant to reach (the skew rejections by tests/sort_model.py, no rounding flip between the f32
and f64 oracles); here the GPU is held to the bars of test_gpu_parity.py / test_gpu_options.py:
  * num_rendered, radii, ranges, point_list and n_contrib identical to the f32 oracle;
  * colour and inverse depth within 1e-5; gradients within 1e-5 absolute with the L1 upstream gradient and 2e-4
    of max |ref| with a unit one;
  * on the record path, image and gradients bitwise those of whole-list sorting without a near-first cut;
and debug_sort_state / debug_near_state show that the path was taken, not only that the result is right.
"""
import numpy as np
import pytest
import torch

from tests import common as C
from tests import sort_model as M

pytestmark = pytest.mark.gpu

_rec = pytest.mark.record_path
# (options, capacity hint).  The near-first cut and the fused binning apply to the capacity-hinted forward only.
VARIANTS = [
    pytest.param({}, False, id="default"),
    pytest.param({}, True, id="default-hint"),
    pytest.param(dict(sort_prefix=0), False, id="sort_prefix=0", marks=_rec),
    pytest.param(dict(sort_prefix=64), False, id="sort_prefix=64", marks=_rec),
    pytest.param(dict(sort_prefix=64), True, id="sort_prefix=64-hint", marks=_rec),
    pytest.param(dict(fused_bin=0), True, id="fused_bin=0", marks=_rec),
    pytest.param(dict(near_mass=0), True, id="near_mass=0", marks=_rec),
    pytest.param(dict(near_mass=1), True, id="near_mass=1", marks=_rec),
    pytest.param(dict(bwd_atomic=0), True, id="bwd_atomic=0"),
    pytest.param(dict(bwd_atomic=1), True, id="bwd_atomic=1"),
]
# Every case under every variant: hot_bin_65536, whose 65544 keys go through the one-workgroup global-memory
# network (153 passes), takes 0.05-0.14 s per test on an MI355X, the others 0.01-0.02 s (the file: 128 tests, 4.5 s).
CASES =[c.name for c in C.DEPTH_CASES]

_SHARED: dict = {}


def _np(t):
    return t.detach().float().cpu().numpy()


def _run(case, inp, ref, grads, hint):
    """Forward (synchronising, or with a capacity hint of the exact count) + one backward per upstream gradient."""
    from gaussian_splatting_amd import _C as CM

    key = (torch.cuda.current_device(), case.W, case.H)
    CM._capacity.pop(key, None)
    if hint:
        CM._capacity[key] = (case.P, ref.num_rendered)
    try:
        fwd = C.run_gpu_forward(inp)
        outs = [C.run_gpu_backward(inp, fwd, *g) for g in grads]
        torch.cuda.synchronize()
    finally:
        CM._capacity.pop(key, None)
    return fwd, outs


def _shared(name):
    """Per case, once: the upstream gradients, the oracle's gradients for them, and the record path's image and
    gradients with whole lists sorted and no near-first cut (numpy, read only)."""
    if name not in _SHARED:
        from gaussian_splatting_amd import _lib

        case, inp, ref, _ = C.depth_reference(name)
        grads = (C.unit_grads(case.H, case.W), C.l1_grads(case.H, case.W))
        ref_grads = [ref.handle.backward(gc, gd) for gc, gd in grads]
        with _lib.options(sort_prefix=0, near_mass=0, bwd_atomic=0):
            fwd, outs = _run(case, inp, ref, grads, hint=False)
        base = dict(color=_np(fwd[1]), invdepth=_np(fwd[6]), outs=[[_np(o) for o in out] for out in outs])
        _SHARED[name] = (grads, ref_grads, base)
    return _SHARED[name]


def _check_against_oracle(name, fwd, outs, tag):
    from gaussian_splatting_amd import _C as CM

    case, inp, ref, _ = C.depth_reference(name)
    grads, ref_grads, _ = _shared(name)
    nr, color, radii, *_rest, invd = fwd
    assert nr == ref.num_rendered
    np.testing.assert_array_equal(_np(radii).astype(np.int32), ref.radii)
    st = CM.debug_forward_state(fwd, case.P)
    rb = ref.handle.binning()
    np.testing.assert_array_equal(st["ranges"].numpy(), rb["ranges"].astype(np.int64))
    np.testing.assert_array_equal(st["point_list"].numpy(), rb["point_list"].astype(np.int64))
    np.testing.assert_array_equal(st["n_contrib"].numpy(), ref.handle.image()["n_contrib"].astype(np.int64))
    np.testing.assert_allclose(_np(color), ref.color, atol=1e-5, rtol=0)
    np.testing.assert_allclose(_np(invd), ref.invdepth, atol=1e-5, rtol=0)
    for r, out, mode in zip(ref_grads, outs, ("unit", "l1")):
        for k, got in zip(C.GRAD_NAMES, out):
            if mode == "l1":
                np.testing.assert_allclose(_np(got), r[k], atol=1e-5, rtol=0, err_msg=f"{tag} {k}")
            else:
                assert C.rel_err(_np(got), r[k]) <= 2e-4, (tag, k, C.rel_err(_np(got), r[k]))
    return st


def _check_bitwise(name, fwd, outs, grads_too):
    base = _shared(name)[2]
    np.testing.assert_array_equal(_np(fwd[1]), base["color"])
    np.testing.assert_array_equal(_np(fwd[6]), base["invdepth"])
    if grads_too:
        for out, b in zip(outs, base["outs"]):
            for k, got, want in zip(C.GRAD_NAMES, out, b):
                np.testing.assert_array_equal(_np(got), want, err_msg=k)


@pytest.mark.parametrize("opts,hint", VARIANTS)
@pytest.mark.parametrize("name", CASES)
def test_depth_case_matches_oracle(name, opts, hint):
    from gaussian_splatting_amd import _lib

    case, inp, ref, _ = C.depth_reference(name)
    grads = _shared(name)[0]
    with _lib.options(**opts):
        record = _lib.option_get("bwd_atomic") == 0
        fwd, outs = _run(case, inp, ref, grads, hint)
        _check_against_oracle(name, fwd, outs, str(opts))
    # the image is the same sum in the same order whatever sorted the lists; so are the record path's gradients
    _check_bitwise(name, fwd, outs, grads_too=record)


LONG_WALLS = ["wall_class0_1k", "wall_class0_3k", "wall_class1", "wall_equal", "hot_bin_65536"]


@pytest.mark.parametrize("name", LONG_WALLS + ["moderate_pass"])
@pytest.mark.record_path
def test_prefix_mode_fallback_sorts_whole_lists(name):
    """Prefix mode (sort_prefix=64, no near-first cut): a long list the bin model rejects at 2048 bins goes to the
    fallback network, which sorts it whole -- sorted_len is the list's length and, every long tile of these walls
    being rejected, no tile is rendered again (a bucket-sorted prefix of 64 would be passed by every tile's walk).
    moderate_pass is rejected nowhere: its long lists stay prefix-sorted where the walk allows (sort_prefix=1024,
    longer than its longest walk) and are redone where it does not (sort_prefix=64)."""
    from gaussian_splatting_amd import _C as CM
    from gaussian_splatting_amd import _lib

    case, inp, ref, keys = C.depth_reference(name)
    grads = _shared(name)[0]
    n = np.array([len(k) for k in keys])
    long = n > 1024
    rejected = np.array([M.skew_rejected(k, M.NB_LONG) for k in keys])
    assert long.all()
    for prefix in (64, 1024):
        with _lib.options(sort_prefix=prefix, near_mass=0):
            fwd, outs = _run(case, inp, ref, grads, hint=False)
            st = CM.debug_sort_state(fwd, case.P)
            _check_against_oracle(name, fwd, outs, f"prefix {prefix}")
        _check_bitwise(name, fwd, outs, grads_too=True)
        sl = st["sorted_len"].numpy()
        walk = int(ref.handle.image()["n_contrib"].max())
        print(f"[{name} prefix {prefix}] lists {n.tolist()}, rejected {int(rejected.sum())}, sorted_len {sl.tolist()}, "
              f"redone tiles {st['redo_count']}, longest walk {walk}")
        assert (sl[rejected] == n[rejected]).all()
        if name == "moderate_pass":
            assert not rejected.any()
            if prefix == 64:
                assert st["redo_count"] > 0  # the walks (up to 281 entries) pass a prefix of 64 + its bin's rest
            else:
                assert walk < prefix and st["redo_count"] == 0 and (sl < n).any() and (sl >= prefix).all()
        else:
            assert rejected.all() and st["redo_count"] == 0


@pytest.mark.parametrize("name", ["fg_wall_4k", "fg_wall_8k"])
@pytest.mark.record_path
def test_near_first_redo_sorts_rejected_lists(name):
    """near_mass=1 with a capacity hint: the cut falls between the thin foreground and the wall, every tile's walk
    passes its near entries, and the redo (tile_far_fill + tile_sort_full_kernel) sorts whole lists the model
    rejects at that kernel's 4096 bins: sort_list<256, 16> up to 4096 keys (fg_wall_4k), sort_list_global
    above (fg_wall_8k)."""
    from gaussian_splatting_amd import _C as CM
    from gaussian_splatting_amd import _lib

    case, inp, ref, keys = C.depth_reference(name)
    grads = _shared(name)[0]
    n = np.array([len(k) for k in keys])
    with _lib.options(near_mass=1):
        fwd, outs = _run(case, inp, ref, grads, hint=True)
        nst = CM.debug_near_state(fwd, case.P)
        st = CM.debug_sort_state(fwd, case.P)
        _check_against_oracle(name, fwd, outs, "near_mass=1")
    _check_bitwise(name, fwd, outs, grads_too=True)
    near = nst["near_len"].numpy()
    nc = ref.handle.image()["n_contrib"].astype(np.int64)
    gx, gy = (case.W + 15) // 16, (case.H + 15) // 16
    walk = nc[:gy * 16, :gx * 16].reshape(gy, 16, gx, 16).max(axis=(1, 3)).reshape(-1)
    wall = int(C.zbin_of(np.array([5.0], np.float32))[0])
    redone = near < walk  # a pixel of the tile blends an entry behind the near ones
    rejected = np.array([M.skew_rejected(k, M.NB_FULL) for k in keys])
    print(f"[{name}] cut bin {nst['zcut']} (wall {wall}), near lists {near.tolist()} of {n.tolist()}, longest walks "
          f"{walk.tolist()}, redone tiles {st['redo_count']}, sorted_len {st['sorted_len'].tolist()}")
    assert nst["zcut"] is not None and nst["zcut"] < wall
    assert (near <= n).all() and redone.any() and st["redo_count"] > 0
    assert st["redo_count"] >= int(redone.sum())
    assert rejected[redone].all()
    assert (st["sorted_len"].numpy()[redone] == n[redone]).all()
    if name == "fg_wall_4k":
        assert (n[redone] <= 4096).all()
    else:
        assert (n[redone] > 4096).all() and (n[redone] <= M.FULL_MAX).all()
