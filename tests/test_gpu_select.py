"""The per-pixel selections on the GPU: ``_C.render_select`` / ``_C.render_median_backward`` (include/gsr.h
gsr_render_select / gsr_render_median_backward; csrc/select.hip) and ``median=`` / ``topk=`` through the autograd nodes.

Reference: tests/select_ref.py -- the median contributor and the top-K in float64 from the per-pixel weights and the
tile lists of the unchanged oracle, which tests/test_select_ref.py pins on the CPU.  ``t`` is the view depth
``(means3D, 1) @ viewmatrix[:, 2]`` in float32.  A selection is discrete, so parity is EXACT on every pixel that is not
excused; excused are the pixels within the project's margins of a threshold of the reference's blend
(contrib_ref.flagged_pixels), those that end their walk at another contributor than the oracle's, and those whose
selection the reference itself calls undecided (within ATOL_FWD = 1e-5 of a tie).  Their number is capped from the
references alone.  Each reference is computed once per case and shared read-only.
"""
import functools

import numpy as np
import pytest
import torch

from tests import common as C
from tests import contrib_ref as CR
from tests import distortion_ref as DR
from tests import select_ref as SR
from tests.test_gpu_alpha import _backward, _forward
from tests.test_gpu_distortion import _built, _caps, _oracle, _threads

pytestmark = pytest.mark.gpu

ATOL_FWD = 1e-5
RTOL_BWD = 2e-4
DEV = "cuda"
NAMES = ["ragged_37x23", "background", "lists_1k_2k", "lists_over_8k", "pose_clamped"]
K_REF = 4


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _t(name):
    return DR.view_depth(_built(name))


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The reference selections (K = 4) of a named case with the reference's flagged pixels, computed once."""
    inp = _built(name)
    nt = _threads(name)
    ref = SR.oracle_select(inp, K_REF, _t(name), nthreads=nt, ref=_oracle(name))
    ref["flagged"] = CR.flagged_pixels(_oracle(name), nt)
    return ref


def _select(inp, fwd, t=None, topk=0):
    from gaussian_splatting_amd import _C

    nr, _c, _r, geom, binning, img = fwd[:6]
    return _C.render_select(geom, binning, img, nr, inp["means3D"].shape[0], inp["H"], inp["W"],
                            t=None if t is None else t.to(DEV), topk=topk, device=geom.device)


def _render(inp, geom_grad=True, cam=None, means3D=None, **kw):
    """GaussianRasterizer on ``inp`` with the per-Gaussian inputs as leaves; returns (outputs, leaves)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from tests.test_gpu_camera import _settings

    per_gaussian = ("means3D", "opacities", "shs", "scales", "rotations", "colors_precomp", "cov3D_precomp")
    L = {k: inp[k].to(DEV).requires_grad_(geom_grad) for k in per_gaussian if inp.get(k) is not None}
    if means3D is not None:
        L["means3D"] = means3D
    L["means2D"] = torch.zeros_like(L["means3D"], requires_grad=geom_grad)
    cam = cam or tuple(inp[k].to(DEV) for k in ("viewmatrix", "projmatrix", "campos"))
    args = dict(means3D=L["means3D"], means2D=L["means2D"], opacities=L["opacities"],
                colors_precomp=L.get("colors_precomp"), scales=L.get("scales"), rotations=L.get("rotations"),
                cov3D_precomp=L.get("cov3D_precomp"), shs=L.get("shs"))
    return GaussianRasterizer(_settings(inp, *cam))(**args, **kw), L


# ---- 1. parity with the reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_selections_match_reference(name):
    """Exact ids, ``median_map == t[median_ids]`` bitwise and weights within 1e-5 on every pixel not excused; an
    excused pixel still selects from its own tile's list and copies that Gaussian's t; excused pixels are at most the
    reference's own flagged + undecided ones plus C.rounding_flip_caps' n_contrib cap.  ``background`` renders over a
    non-zero background, which the maps must ignore."""
    from gaussian_splatting_amd import _C as CM

    inp = _built(name)
    H, W = inp["H"], inp["W"]
    t = _t(name)
    tn = t.numpy()
    ref = _ref(name)
    fwd = _forward(inp)
    med, mid, ids, wts = (_np(x) for x in _select(inp, fwd, t, K_REF))
    assert med.shape == (1, H, W) and mid.shape == (1, H, W) and ids.shape == (K_REF, H, W) and wts.shape == ids.shape
    assert med.dtype == np.float32 and mid.dtype == np.int32 and ids.dtype == np.int32 and wts.dtype == np.float32
    med, mid = med[0], mid[0]
    st = CM.debug_forward_state(fwd[:7], inp["means3D"].shape[0])
    nc_differs = st["n_contrib"].numpy() != ref["n_contrib"]
    undecided = ~(ref["decided_median"] & ref["decided_topk"])
    ref_excused = int(ref["flagged"].sum()) + int(undecided.sum())
    excused = ref["flagged"] | nc_differs | undecided
    _, cap_nc, oracle_counts = _caps(name)
    ok = ~excused
    d = np.abs(wts.astype(np.float64) - ref["topk_weights"])[:, ok]
    wrong_m = int((mid[ok] != ref["median_ids"][ok]).sum())
    wrong_k = int((ids[:, ok] != ref["topk_ids"][:, ok]).sum())
    crossing = int((ref["crosses"] & (ref["count"] > 0)).sum())
    print(f"[{name}] {H * W} pixels: flagged {int(ref['flagged'].sum())}, undecided median "
          f"{int((~ref['decided_median']).sum())} top-{K_REF} {int((~ref['decided_topk']).sum())}, n_contrib differs "
          f"{int(nc_differs.sum())} (cap {cap_nc}; f32 oracle vs f64 oracle {oracle_counts}); excused "
          f"{int(excused.sum())}; wrong median ids {wrong_m}, wrong top-k ids {wrong_k}, max |w - ref| "
          f"{d.max():.2e}; {crossing} pixels reach one half, {int((~ref['crosses'] & (ref['count'] > 0)).sum())} "
          f"never do")
    assert ref_excused <= 0.01 * H * W
    assert int(excused.sum()) <= ref_excused + cap_nc
    assert wrong_m == 0 and wrong_k == 0
    assert d.max() <= ATOL_FWD
    # every pixel, excused or not: the map is a copy of t at the id (0.0 at -1)
    want = np.where(mid >= 0, tn[np.maximum(mid, 0)], np.float32(0.0))
    assert np.array_equal(med.view(np.int32), want.view(np.int32))
    for y, x in zip(*np.nonzero(excused)):
        lst = set(ref["lists"][y * W + x].tolist()) | {-1}
        assert int(mid[y, x]) in lst and all(int(g) in lst for g in ids[:, y, x]), (y, x)
    # a pixel without a contributor
    empty = st["n_contrib"].numpy() == 0
    assert (mid[empty] == -1).all() and (ids[:, empty] == -1).all() and not wts[:, empty].any()
    # both branches of the median rule
    assert crossing > 0
    if name in ("ragged_37x23", "background", "pose_clamped"):
        assert int((~ref["crosses"] & (ref["count"] > 0)).sum()) > 100
    if name == "background":
        assert float(inp["bg"].abs().max()) > 0 and empty.any()


# ---- 2. exact self-consistency on the GPU --------------------------------------------------------------------
def test_selections_agree_with_the_contribution_statistics():
    """K = 8 holds every contributor of every pixel of ragged_37x23 (at most 7), so the top-K planes are the pixel's
    whole weight set: bitwise the one contrib.hip forms, both kernels recomputing the forward's alpha identically."""
    from gaussian_splatting_amd import _C as CM

    name = "ragged_37x23"
    inp = _built(name)
    P, H, W = inp["means3D"].shape[0], inp["H"], inp["W"]
    fwd = _forward(inp, return_alpha=True)
    nr, _c, _r, geom, binning, img = fwd[:6]
    alpha = fwd[7]
    st = CM.debug_forward_state(fwd[:7], P)
    assert int(_ref(name)["count"].max()) <= 7
    med8, mid8, ids8, w8 = _select(inp, fwd, _t(name), 8)
    stats = CM.contribution_stats(geom, binning, img, nr, P, H, W)
    ids, w = _np(ids8).reshape(-1), _np(w8).reshape(-1)
    on = ids >= 0
    assert (w[on] > 0).all() and not w[~on].any()
    count = np.bincount(ids[on], minlength=P)
    assert np.array_equal(count, _np(stats[:, 2].contiguous().view(torch.int32)).astype(np.int64))
    wmax = np.zeros(P, np.float32)
    np.maximum.at(wmax, ids[on], w[on])
    assert np.array_equal(wmax.view(np.int32), _np(stats[:, 1].contiguous()).view(np.int32))
    # the number of filled ranks is the pixel's contributor count: never more than its n_contrib
    assert (_np(ids8 >= 0).sum(0) <= st["n_contrib"].numpy()).all()
    s = float((w8.sum(0) - alpha[0]).abs().max())
    print(f"max |sum_k topk_weights - alpha| = {s:.2e}")
    assert s <= 1e-6
    # descending, ties apart
    assert bool((w8[:-1] >= w8[1:]).all())
    # fewer planes are the first planes; the median does not depend on the top-K beside it
    _, _, ids2, w2 = _select(inp, fwd, None, 2)
    assert torch.equal(ids8[:2], ids2) and torch.equal(w8[:2], w2)
    for k in (1, 3, 4, 5):
        m, i, idk, wk = _select(inp, fwd, _t(name), k)
        assert torch.equal(idk, ids8[:k]) and torch.equal(wk, w8[:k]), k
        assert torch.equal(i, mid8) and torch.equal(m, med8), k
    m, i, none_ids, none_w = _select(inp, fwd, _t(name), 0)
    assert none_ids is None and none_w is None and torch.equal(i, mid8) and torch.equal(m, med8)


# ---- 3. invariance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_37x23", "lists_over_8k", "pose_clamped"])
def test_selections_are_bitwise_reproducible_under_every_forward(name):
    """The weights depend on the forward's discrete state alone: the same bits from a second call, from copies of the
    buffers, after a whole-tile forward ("fwd_quads" 4), a half-tile one (2) and a no_backward forward."""
    from gaussian_splatting_amd import _lib

    inp = _built(name)
    t = _t(name)
    base = _select(inp, _forward(inp), t, 8)
    assert int((base[1] >= 0).sum()) > 0 and float(base[3].max()) > 0

    def same(fwd):
        return all(torch.equal(a, b) for a, b in zip(_select(inp, fwd, t, 8), base))

    fwd = _forward(inp)
    assert same(fwd) and same(fwd)
    assert same(fwd[:3] + tuple(b.clone() for b in fwd[3:6]))
    for q in (2, 4):
        with _lib.options(fwd_quads=q):
            assert same(_forward(inp)), q
    assert same(_forward(inp, no_backward=True))


@pytest.mark.parametrize("path", ["atomic", "record"])
def test_colour_backward_is_unaffected_by_the_select_calls(path):
    """The select forward and the median backward read the buffers only: a colour backward after them equals a fresh
    one (bitwise on the record path, within the backward's bar under float atomics)."""
    from gaussian_splatting_amd import _C, _lib

    name = "lists_1k_2k"
    inp = _built(name)
    P, H, W = inp["means3D"].shape[0], inp["H"], inp["W"]
    g_c, g_d = C.unit_grads(H, W)
    U = DR.make_upstream(H, W).to(DEV)
    with _lib.options(bwd_atomic=1 if path == "atomic" else 0):
        fwd = _forward(inp)
        before = _select(inp, fwd, _t(name), 4)
        _C.render_median_backward(before[1], U, P)
        after = _backward(inp, fwd, g_c, g_d)
        again = _select(inp, fwd, _t(name), 4)  # (and the backward leaves the selections alone)
        fresh = _backward(inp, _forward(inp), g_c, g_d)
        torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, again))
    for k, a, b in zip(C.GRAD_NAMES, after, fresh):
        if path == "record":
            assert torch.equal(a, b), k
        else:  # (float atomics: the hardware's order)
            assert C.rel_err(_np(a), _np(b)) <= RTOL_BWD, k


# ---- 4. backward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_37x23", "lists_1k_2k", "pose_clamped"])
def test_median_backward_is_the_scatter_of_the_upstream(name):
    """dL_dt against np.bincount in float64 over the GPU's own ids: sums of at most H W float32 terms in the
    hardware's order, within 1e-6 of max |ref|."""
    from gaussian_splatting_amd import _C

    inp = _built(name)
    P, H, W = inp["means3D"].shape[0], inp["H"], inp["W"]
    U = DR.make_upstream(H, W)
    _m, mid, _i, _w = _select(inp, _forward(inp), _t(name), 0)
    got = _np(_C.render_median_backward(mid, U.to(DEV), P))
    want = SR.scatter_backward(_np(mid), U.numpy(), P)
    e = C.rel_err(got, want)
    print(f"[{name}] dL_dt vs bincount: {e:.1e} (max |ref| {np.abs(want).max():.3g}, {int((want != 0).sum())} rows "
          f"hit)")
    assert np.abs(want).max() > 0 and got.shape == (P,)
    assert e <= 1e-6
    assert not got[want == 0].any()


@pytest.mark.parametrize("cam_grad", [False, True], ids=["means3D", "means3D+camera"])
def test_gradients_reach_what_t_was_built_from(cam_grad):
    """t built in torch from the means3D leaf (and a viewmatrix leaf) with a joint colour + median loss: means3D.grad
    is the colour-only gradient plus the scatter chained through the view depth -- the kernel forms no geometry
    gradient of the median -- and the viewmatrix leaf receives the chain through t."""
    name = "ragged_37x23"
    inp = _built(name)
    H, W = inp["H"], inp["W"]
    g_c, _ = C.unit_grads(H, W)
    U = DR.make_upstream(H, W)
    outs_c, Lc = _render(inp)
    (outs_c[0] * g_c.to(DEV)).sum().backward()
    m = inp["means3D"].to(DEV).requires_grad_(True)
    V = inp["viewmatrix"].to(DEV).requires_grad_(cam_grad)
    t = (torch.cat([m, torch.ones_like(m[:, :1])], 1) @ V[:, 2]).contiguous()
    outs, L = _render(inp, means3D=m, median=t)
    assert len(outs) == 5 and outs[3].requires_grad and not outs[4].requires_grad and outs[4].dtype == torch.int32
    ((outs[0] * g_c.to(DEV)).sum() + (outs[3] * U.to(DEV)).sum()).backward()
    dL_dt = SR.scatter_backward(_np(outs[4]), U.numpy(), m.shape[0])
    col = inp["viewmatrix"].double().numpy()[:, 2]
    want_m = _np(Lc["means3D"].grad).astype(np.float64) + np.outer(dL_dt, col[:3])
    e_m = C.rel_err(_np(m.grad), want_m)
    print(f"means3D {e_m:.1e}")
    assert np.abs(np.outer(dL_dt, col[:3])).max() > 10 * RTOL_BWD * np.abs(want_m).max()  # (the t part shows)
    assert e_m <= RTOL_BWD
    for k in ("opacities", "scales", "rotations", "shs", "means2D"):  # the colour loss alone
        assert C.rel_err(_np(L[k].grad), _np(Lc[k].grad)) <= RTOL_BWD, k
    if cam_grad:
        want_V = np.concatenate([inp["means3D"].double().numpy(), np.ones((m.shape[0], 1))], 1).T @ dL_dt
        e_V = C.rel_err(_np(V.grad)[:, 2], want_V)
        print(f"viewmatrix[:, 2] {e_V:.1e}")
        assert e_V <= RTOL_BWD and not _np(V.grad)[:, [0, 1, 3]].any()


# ---- 5. surface ----------------------------------------------------------------------------------------------
@pytest.mark.record_path
def test_output_order_with_every_keyword_combination():
    from tests import features_ref as FR

    name = "background"
    inp = _built(name)
    P, H, W = inp["means3D"].shape[0], inp["H"], inp["W"]
    t = _t(name).to(DEV)
    F = FR.make_features(P, 3).to(DEV)
    plain = _render(inp)[0]
    assert len(plain) == 3
    full, _ = _render(inp, return_alpha=True, features=F, distortion=t, median=t, topk=3, return_contrib=True)
    assert len(full) == 11
    color, radii, invd, alpha, fmap, dmap, med, mid, tids, tw, stats = full
    shapes = [(3, H, W), (P,), (1, H, W), (1, H, W), (3, H, W), (1, H, W), (1, H, W), (1, H, W), (3, H, W), (3, H, W),
              (P, 4)]
    assert [tuple(o.shape) for o in full] == shapes
    assert mid.dtype == torch.int32 and tids.dtype == torch.int32 and tw.dtype == torch.float32
    assert med.requires_grad is False  # (t is no leaf that requires grad here)
    assert not (mid.requires_grad or tids.requires_grad or tw.requires_grad or stats.requires_grad)
    for a, b in zip((color, radii, invd), plain):
        assert torch.equal(a, b)
    for flags in range(32):
        kw = {}
        want = [color, radii, invd]
        if flags & 1:
            kw["return_alpha"] = True
            want.append(alpha)
        if flags & 2:
            kw["features"] = F
            want.append(fmap)
        if flags & 4:
            kw["median"] = t
            want += [med, mid]
        if flags & 8:
            kw["topk"] = 3
            want += [tids, tw]
        if flags & 16:
            kw["return_contrib"] = True
            want.append(stats)
        if not flags & 12:
            continue  # (the tuples without the two keywords are the existing tests')
        with torch.no_grad():
            got = _render(inp, **kw)[0]
        assert len(got) == len(want), flags
        for a, b in zip(got, want):
            if a is got[-1] and flags & 16:  # (the statistics' two sums are added atomically)
                assert torch.equal(a[:, 1:3].view(torch.int32), b[:, 1:3].view(torch.int32)), flags
            else:
                assert a.dtype == b.dtype and torch.equal(a, b), flags
    with_d = _render(inp, distortion=t, median=t)[0]
    assert len(with_d) == 6 and torch.equal(with_d[3], dmap) and torch.equal(with_d[5], mid)
    # a leaf t: the map is differentiable, nothing else of the pair or of topk is
    tl = t.clone().requires_grad_(True)
    outs = _render(inp, geom_grad=False, median=tl, topk=2)[0]
    assert outs[3].requires_grad and not any(o.requires_grad for o in outs[4:])
    outs[3].sum().backward()
    assert float(tl.grad.sum()) == float((outs[4] >= 0).sum())


def test_the_keywords_change_nothing_else():
    """The colour node's backward gives the same bits with the keywords as without (record path)."""
    from gaussian_splatting_amd import _lib

    name = "lists_1k_2k"
    inp = _built(name)
    g_c, g_d = C.unit_grads(inp["H"], inp["W"])
    with _lib.options(bwd_atomic=0):
        plain, Lp = _render(inp)
        with_kw, Lw = _render(inp, median=_t(name).to(DEV), topk=4)
        for outs in (plain, with_kw):
            torch.autograd.backward([outs[0], outs[2]], [g_c.to(DEV), g_d.to(DEV)])
    for a, b in zip(plain, with_kw[:3]):
        assert torch.equal(a, b)
    for k in ("means2D", "means3D", "opacities", "shs", "scales", "rotations"):
        assert torch.equal(Lp[k].grad, Lw[k].grad), k


def test_empty_and_culled_scenes():
    inp = dict(C.build(C.Case("tmp", P=10, W=37, H=23)))
    for k in ("means3D", "opacities", "shs", "scales", "rotations"):
        inp[k] = inp[k][:0]
    t0 = torch.zeros(0, device=DEV, requires_grad=True)
    outs, _ = _render(inp, median=t0, topk=2)
    assert len(outs) == 7
    _c, _r, _i, med, mid, tids, tw = outs
    assert tuple(med.shape) == (1, 23, 37) and tuple(tids.shape) == (2, 23, 37)
    assert not _np(med).any() and (mid == -1).all() and (tids == -1).all() and not _np(tw).any()
    med.sum().backward()
    assert tuple(t0.grad.shape) == (0,)
    # every Gaussian behind the camera: num_rendered == 0
    inp = dict(C.build(C.Case("behind", P=50, W=37, H=23, bg=(0.1, 0.2, 0.3))))
    inp["means3D"] = inp["means3D"].clone()
    inp["means3D"][:, 2] = -5.0
    t = torch.linspace(1.0, 2.0, 50, device=DEV).requires_grad_(True)
    fwd = _forward(inp)
    assert fwd[0] == 0
    med, mid, tids, tw = _select(inp, fwd, t.detach(), 8)
    assert not _np(med).any() and (mid == -1).all() and (tids == -1).all() and not _np(tw).any()
    assert tids.dtype == torch.int32 and tuple(tw.shape) == (8, 23, 37)
    outs, _ = _render(inp, median=t)
    (outs[3] * DR.make_upstream(23, 37).to(DEV)).sum().backward()
    assert tuple(t.grad.shape) == (50,) and not _np(t.grad).any()
    outs, _ = _render(inp, topk=1)
    assert len(outs) == 5 and (outs[3] == -1).all() and not _np(outs[4]).any()


def test_cov3d_precomp_with_a_geometry_gradient_is_accepted():
    inp = _built("cov3d_precomp")
    t = DR.view_depth(inp).to(DEV).requires_grad_(True)
    U = DR.make_upstream(inp["H"], inp["W"]).to(DEV)
    outs, L = _render(inp, median=t, topk=2)  # (geometry leaves require grad)
    assert len(outs) == 7 and L["cov3D_precomp"].requires_grad
    ((outs[3] * U).sum() + outs[0].sum()).backward()
    assert float(t.grad.abs().max()) > 0 and float(L["cov3D_precomp"].grad.abs().max()) > 0
    want = SR.scatter_backward(_np(outs[4]), _np(U), t.shape[0])
    assert C.rel_err(_np(t.grad), want) <= 1e-6


def test_bad_arguments_are_refused_and_the_library_stays_usable():
    from gaussian_splatting_amd import _C, _lib

    name = "ragged_37x23"
    inp = _built(name)
    P, H, W = inp["means3D"].shape[0], inp["H"], inp["W"]
    fwd = _forward(inp)
    nr, _c, _r, geom, binning, img = fwd[:6]
    td = _t(name).to(DEV)
    med, mid = torch.zeros(H, W, device=DEV), torch.zeros(H, W, dtype=torch.int32, device=DEV)
    ids, wts = torch.zeros(8, H, W, dtype=torch.int32, device=DEV), torch.zeros(8, H, W, device=DEV)
    lib = _lib.load()
    bufs = (geom.data_ptr(), binning.data_ptr(), img.data_ptr(), 0, binning.numel())
    tp, m, i, k, w = td.data_ptr(), med.data_ptr(), mid.data_ptr(), ids.data_ptr(), wts.data_ptr()
    bad = [((P, nr, 0, H, *bufs, tp, 4, m, i, k, w, None), b"invalid sizes"),
           ((P, nr, W, H, *bufs, None, 4, m, i, k, w, None), b"go together"),
           ((P, nr, W, H, *bufs, tp, 4, None, i, k, w, None), b"go together"),
           ((P, nr, W, H, *bufs, tp, 4, m, None, k, w, None), b"go together"),
           ((P, nr, W, H, *bufs, tp, 0, None, None, k, w, None), b"go together"),
           ((P, nr, W, H, *bufs, tp, 9, m, i, k, w, None), b"K=9"),
           ((P, nr, W, H, *bufs, tp, -1, m, i, k, w, None), b"K=-1"),
           ((P, nr, W, H, *bufs, tp, 0, m, i, k, w, None), b"exactly when K > 0"),
           ((P, nr, W, H, *bufs, tp, 4, m, i, None, w, None), b"exactly when K > 0"),
           ((P, nr, W, H, *bufs, tp, 4, m, i, k, None, None), b"exactly when K > 0"),
           ((P, nr, W, H, *bufs, None, 0, None, None, None, None, None), b"nothing to select"),
           ((P, nr, W, H, *bufs[:4], binning.numel() + 8, tp, 4, m, i, k, w, None), b"no layout"),
           ((P, nr, W, H, None, None, None, 0, 0, tp, 4, m, i, k, w, None), b"missing")]
    for args, msg in bad:
        assert lib.gsr_render_select(*args) == 1, msg  # GSR_ERR_ARGUMENT
        assert msg in lib.gsr_last_error(), (msg, lib.gsr_last_error())
    assert not _np(med).any() and not _np(mid).any() and not _np(ids).any() and not _np(wts).any()
    dt = torch.zeros(P, device=DEV)
    for args, msg in [((P, 0, H, i, m, dt.data_ptr(), None), b"invalid sizes"),
                      ((P, W, H, None, m, dt.data_ptr(), None), b"null"),
                      ((P, W, H, i, None, dt.data_ptr(), None), b"null"),
                      ((P, W, H, i, m, None, None), b"null")]:
        assert lib.gsr_render_median_backward(*args) == 1, msg
        assert msg in lib.gsr_last_error(), (msg, lib.gsr_last_error())
    assert not _np(dt).any()
    with pytest.raises(RuntimeError, match="int32"):
        _C.render_median_backward(mid.view(1, H, W).float(), med.view(1, H, W), P)
    with pytest.raises(RuntimeError, match="dL_dmedian_map"):
        _C.render_median_backward(mid.view(1, H, W), med, P)
    # ids outside 0 .. P-1 are skipped, not followed
    wild = torch.full((1, H, W), P, dtype=torch.int32, device=DEV)
    wild[0, 0, 0] = -7
    wild[0, 0, 1] = 3
    got = _C.render_median_backward(wild, torch.ones(1, H, W, device=DEV), P)
    assert float(got[3]) == 1.0 and float(got.sum()) == 1.0
    base = _select(inp, fwd, _t(name), K_REF)  # (still usable)
    ref = _ref(name)
    assert (_np(base[1])[0] != ref["median_ids"]).sum() <= 5
