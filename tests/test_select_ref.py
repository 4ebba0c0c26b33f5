"""CPU checks of the selection reference (tests/select_ref.py) that tests/test_gpu_select.py holds the kernels to, of
the new C ABI symbols and of the Python argument checks of ``median=`` and ``topk=``.

On ``ragged_37x23`` the reference (``T_i = 1 - sum_{j<i} w_j`` in float64, vectorised selection) against a brute-force
per-pixel Python loop that carries ``T`` as a running product of ``1 - alpha_i`` and keeps the selections by the rule's
own wording; hand-built pixels with known answers; the scatter backward against torch autograd of ``t[ids]``.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import common as C
from tests import contrib_ref as CR
from tests import distortion_ref as DR
from tests import select_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _ragged():
    case = next(c for c in C.SMALL_CASES if c.name == "ragged_37x23")
    inp = C.build(case)
    ref = C.run_oracle(inp)
    return inp, ref, CR.per_pixel_weights(ref, inp["H"], inp["W"])


def test_reference_matches_a_brute_force_loop():
    """Pixel by pixel over the oracle's list: T carried as a running product, the median overwritten while T > 0.5
    before T is multiplied (2DGS's loop), the top-K kept by insertion with displacement on strict > only."""
    inp, ref, w = _ragged()
    H, W, K = inp["H"], inp["W"], 4
    t = DR.view_depth(inp)
    got = SR.oracle_select(inp, K, t, ref=ref, w=w)
    lists = SR.pixel_lists(ref, H, W)
    tn = t.numpy()
    crossing = never = 0
    for pix in range(H * W):
        T = 1.0
        mid, mval = -1, 0.0
        top = []  # (weight, id), descending
        for g in lists[pix]:
            wg = float(w[pix, g])
            if wg <= 0:
                continue
            if T > 0.5:
                mid, mval = int(g), float(tn[g])
            pos = len(top)
            while pos > 0 and wg > top[pos - 1][0]:
                pos -= 1
            top.insert(pos, (wg, int(g)))
            del top[K:]
            T *= 1.0 - wg / T
        y, x = divmod(pix, W)
        if not got["decided_median"][y, x]:
            continue
        assert got["median_ids"][y, x] == mid and got["median"][y, x] == mval, pix
        ids = [g for _, g in top] + [-1] * (K - len(top))
        wts = [v for v, _ in top] + [0.0] * (K - len(top))
        assert list(got["topk_ids"][:, y, x]) == ids and list(got["topk_weights"][:, y, x]) == wts, pix
        if mid >= 0:
            crossing += T <= 0.5
            never += T > 0.5
    print(f"ragged_37x23: {crossing} pixels cross one half, {never} never do; undecided median "
          f"{int((~got['decided_median']).sum())}, top-{K} {int((~got['decided_topk']).sum())}; most contributors "
          f"{int(got['count'].max())}")
    assert crossing > 50 and never > 50  # both branches of the median rule
    assert int(got["crosses"].sum()) == crossing
    assert int(got["count"].max()) <= 8  # (tests/test_gpu_select.py's K = 8 then holds every contributor)


def test_known_answers():
    t = np.array([5.0, 6.0, 7.0, 8.0], np.float32)
    # no contributor
    r = SR.select_pixel([], [], 2, t)
    assert r["median_id"] == -1 and r["median"] == 0.0 and list(r["topk_ids"]) == [-1, -1]
    assert not r["topk_weights"].any() and r["decided_median"] and r["decided_topk"]
    # one Gaussian: it is the median whatever its weight, and K beyond the count is padded with (-1, 0.0)
    r = SR.select_pixel([0.3], [2], 3, t)
    assert r["median_id"] == 2 and r["median"] == 7.0
    assert list(r["topk_ids"]) == [2, -1, -1] and list(r["topk_weights"]) == [0.3, 0.0, 0.0]
    # an opaque stack: alpha 0.99 each, T = 1, 0.01, 1e-4: only the first is blended while T > 0.5
    r = SR.select_pixel([0.99, 0.0099, 0.000099], [3, 1, 0], 2, t)
    assert r["median_id"] == 3 and r["median"] == 8.0 and list(r["topk_ids"]) == [3, 1]
    # T never reaches one half (1, 0.9, 0.8, 0.7 before the entries): the median is the last contributor
    r = SR.select_pixel([0.1, 0.1, 0.1, 0.1], [0, 1, 2, 3], 1, t)
    assert r["median_id"] == 3 and r["median"] == 8.0
    # the crossing entry itself: T = 1, 0.7, 0.4 before the entries -- the second takes T to 0.4 and is the median
    r = SR.select_pixel([0.3, 0.3, 0.2], [0, 1, 2], 3, t)
    assert r["median_id"] == 1 and r["decided_median"]
    # an exact weight tie: the earlier one in list order ranks first, at either end of the kept ranks; undecided
    r = SR.select_pixel([0.25, 0.125, 0.25, 0.125], [3, 2, 1, 0], 3, t)
    assert list(r["topk_ids"]) == [3, 1, 2] and list(r["topk_weights"]) == [0.25, 0.25, 0.125]
    assert not r["decided_topk"]
    # T exactly one half before an entry: by the rule that entry is NOT in front (T > 0.5 fails), and it is undecided
    r = SR.select_pixel([0.5, 0.25], [0, 1], 1, t)
    assert r["median_id"] == 0 and not r["decided_median"]
    # the tie behind rank K + 1 does not matter
    r = SR.select_pixel([0.4, 0.2, 0.05, 0.05], [0, 1, 2, 3], 1, t)
    assert r["decided_topk"] and list(r["topk_ids"]) == [0]


def test_scatter_backward_matches_autograd():
    inp, ref, w = _ragged()
    H, W, P = inp["H"], inp["W"], inp["means3D"].shape[0]
    sel = SR.oracle_select(inp, 1, DR.view_depth(inp), ref=ref, w=w)
    ids = torch.from_numpy(np.array(sel["median_ids"])).reshape(-1)
    U = DR.make_upstream(H, W).double().reshape(-1)
    t = DR.view_depth(inp).double().requires_grad_(True)
    hit = ids >= 0
    (t[ids[hit]] * U[hit]).sum().backward()
    got = SR.scatter_backward(sel["median_ids"], U.numpy(), P)
    assert got.shape == (P,) and np.abs(got).max() > 0
    assert np.abs(got - t.grad.numpy()).max() <= 1e-12 * np.abs(got).max()
    assert (~hit).any()  # (pixels without a contributor take no part)


def test_symbols_are_declared_bound_and_exported():
    from gaussian_splatting_amd import _lib

    names = _lib.header_symbols(os.path.join(ROOT, "include", "gsr.h"))
    for sym in ("gsr_render_select", "gsr_render_select_max_k", "gsr_render_median_backward"):
        assert sym in names, sym
        assert sym in _lib.SIGNATURES, sym
    assert len(_lib.SIGNATURES["gsr_render_select"][1]) == 16
    assert len(_lib.SIGNATURES["gsr_render_select_max_k"][1]) == 0
    assert len(_lib.SIGNATURES["gsr_render_median_backward"][1]) == 7


def test_the_built_library_exports_the_entry_points():
    from gaussian_splatting_amd import _C, _lib

    lib = _lib.load()
    for sym in ("gsr_render_select", "gsr_render_select_max_k", "gsr_render_median_backward"):
        assert getattr(lib, sym) is not None, sym
    assert _C.select_max_k() == 8


def _call(over=None, **kw):
    """rasterize_gaussians(median=..., topk=...) on host tensors: every check below must raise before any device
    work."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, rasterize_gaussians

    P = 5
    z = torch.zeros
    eye = torch.eye(4)
    s = GaussianRasterizationSettings(8, 8, 1.0, 1.0, z(3), 1.0, eye, eye, 0, z(3), False, False, False)
    a = dict(means3D=z(P, 3), means2D=z(P, 3), sh=torch.Tensor([]), colors=z(P, 3), opac=z(P, 1), scales=z(P, 3),
             rot=z(P, 4), cov=torch.Tensor([]))
    a.update(over or {})
    return rasterize_gaussians(a["means3D"], a["means2D"], a["sh"], a["colors"], a["opac"], a["scales"], a["rot"],
                               a["cov"], s, **kw)


def test_median_argument_checks_raise():
    from gaussian_splatting_amd import _C

    for call in (lambda t: _call(median=t), lambda t: _C.check_median(t, 5)):
        with pytest.raises(RuntimeError, match=r"\(num_points,\)"):
            call(torch.zeros(5, 1))
        with pytest.raises(RuntimeError, match=r"\(num_points,\)"):
            call(torch.zeros(4))  # another point count
        with pytest.raises(RuntimeError, match="float32"):
            call(torch.zeros(5, dtype=torch.float64))
        with pytest.raises(TypeError, match="tensor"):
            call([0.0] * 5)
        with pytest.raises(RuntimeError, match="HIP device"):
            call(torch.zeros(5))  # a host tensor: there is no CPU path
    keep = _C._require_device
    _C._require_device = lambda t, name: None  # (contiguity is checked on device tensors, after the device check)
    try:
        with pytest.raises(RuntimeError, match="contiguous"):
            _C.check_median(torch.zeros(5, 2)[:, 0], 5)
        _C.check_median(torch.zeros(5), 5)
    finally:
        _C._require_device = keep


def test_topk_argument_checks_raise():
    from gaussian_splatting_amd import _C

    for call in (lambda k: _call(topk=k), _C.check_topk):
        for bad in (0, -1, 9, 1 << 40):
            with pytest.raises(ValueError, match="1 <= K <= 8"):
                call(bad)
        for bad in (True, False, 2.0, "4", torch.tensor(3)):
            with pytest.raises(TypeError, match="expected an int"):
                call(bad)
    assert [_C.check_topk(k) for k in range(1, 9)] == list(range(1, 9))
    with pytest.raises(RuntimeError, match="HIP device"):  # a valid K goes on to the device check
        _call(topk=4)
    with pytest.raises(ValueError, match="nothing to select"):
        _C.render_select(torch.zeros(0), torch.zeros(0), torch.zeros(0), 0, 5, 8, 8)


def test_cov3d_precomp_with_a_geometry_gradient_is_not_refused():
    """median= and topk= form no geometry gradient: the refusal that features= and distortion= keep does not apply,
    and the call goes on to the device check."""
    cov = dict(scales=torch.Tensor([]), rot=torch.Tensor([]), cov=torch.zeros(5, 6),
               means3D=torch.zeros(5, 3, requires_grad=True))
    with pytest.raises(RuntimeError, match="HIP device"):
        _call(cov, median=torch.zeros(5))
    with pytest.raises(RuntimeError, match="HIP device"):
        _call(cov, topk=2)
    with pytest.raises(RuntimeError, match="distortion= with cov3D_precomp"):  # (the refusal stays where it was)
        _call(cov, median=torch.zeros(5), distortion=torch.zeros(5))
