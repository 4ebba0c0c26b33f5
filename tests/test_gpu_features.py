"""N-channel feature rendering on the GPU: ``_C.render_features`` / ``_C.render_features_backward`` (include/gsr.h
gsr_render_features / gsr_render_features_backward; csrc/features.hip) and ``features=`` through the autograd nodes.

Reference: tests/features_ref.py -- ceil(C/3) runs of the unchanged oracle with the features as precomputed colours
over a zero background, which tests/test_features_ref.py pins on the CPU -- and the project's own colour path.
Bars: the project's, 1e-5 max(1, max |F|) per pixel of the map and RTOL_BWD = 2e-4 of max |ref| per gradient tensor.
"""
import functools

import numpy as np
import pytest
import torch

from tests import alpha_ref as AR
from tests import common as C
from tests import features_ref as FR
from tests.test_gpu_alpha import _backward, _forward

pytestmark = pytest.mark.gpu

ATOL_FWD = 1e-5
RTOL_BWD = 2e-4
DEV = "cuda"
CHANNELS = [1, 3, 7, 16, 35]
NAMES = ["sh3_scalerot", "ragged_37x23", "antialiasing", "background", "dense_opaque", "lists_1k_2k", "lists_over_8k",
         "pose_general", "pose_clamped"]
PATHS = [pytest.param("atomic", id="atomic"), pytest.param("record", marks=pytest.mark.record_path, id="record")]
LEAF_OF = {"dL_dmeans3D": "means3D", "dL_dmeans2D": "means2D", "dL_dopacity": "opacities", "dL_dscales": "scales",
           "dL_drotations": "rotations"}


def _case(name):
    return next(c for c in C.SMALL_CASES + C.POSE_CASES if c.name == name)


def _np(t):
    return t.detach().float().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _built(name):
    return C.build(_case(name))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return C.run_oracle(_built(name))


@functools.lru_cache(maxsize=None)
def _caps(name):
    return C.rounding_flip_caps(_built(name), _oracle(name))


@functools.lru_cache(maxsize=None)
def _FU(name, Cn):
    inp = _built(name)
    return FR.make_features(inp["means3D"].shape[0], Cn), FR.make_upstream(Cn, inp["H"], inp["W"])


@functools.lru_cache(maxsize=None)
def _ref(name, Cn):
    """The oracle's feature map and gradients for a named case and channel count, computed once, read-only."""
    return FR.oracle_features(_built(name), *_FU(name, Cn))


def _fmap(inp, fwd, F):
    from gaussian_splatting_amd import _C

    nr, _c, _r, geom, binning, img = fwd[:6]
    return _C.render_features(geom, binning, img, nr, inp["means3D"].shape[0], inp["H"], inp["W"], F.to(DEV))


def _render(inp, F=None, geom_grad=True, feat_grad=True, cam_grad=False, **kw):
    """GaussianRasterizer on ``inp`` with the per-Gaussian inputs as leaves; returns (outputs, leaves)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from tests.test_gpu_camera import _settings

    per_gaussian = ("means3D", "opacities", "shs", "scales", "rotations", "colors_precomp", "cov3D_precomp")
    L = {k: inp[k].to(DEV).requires_grad_(geom_grad) for k in per_gaussian if inp.get(k) is not None}
    L["means2D"] = torch.zeros_like(L["means3D"], requires_grad=geom_grad)
    cam = tuple(inp[k].to(DEV).requires_grad_(cam_grad) for k in ("viewmatrix", "projmatrix", "campos"))
    L.update(zip(("viewmatrix", "projmatrix", "campos"), cam))
    if F is not None:
        L["features"] = F.to(DEV).requires_grad_(feat_grad)
        kw["features"] = L["features"]
    args = dict(means3D=L["means3D"], means2D=L["means2D"], opacities=L["opacities"],
                colors_precomp=L.get("colors_precomp"), scales=L.get("scales"), rotations=L.get("rotations"),
                cov3D_precomp=L.get("cov3D_precomp"), shs=L.get("shs"))
    return GaussianRasterizer(_settings(inp, *cam))(**args, **kw), L


def _as_colours(inp, F):
    """``inp`` rendering ``F`` [P,3] as precomputed colours over a zero background."""
    a = dict(inp)
    a.update(colors_precomp=F, shs=None, bg=torch.zeros(3))
    return a


def test_channel_counts_cross_a_chunk():
    from gaussian_splatting_amd import _C

    ch = _C.feature_chunk()
    assert ch >= 1
    assert any(c > ch and c % ch != 0 for c in CHANNELS), (ch, CHANNELS)  # several chunks, the last one partial
    assert any(c < ch for c in CHANNELS) and 1 in CHANNELS


# ---- 1. the forward against the oracle --------------------------------------------------------------------
@pytest.mark.parametrize("Cn", CHANNELS)
@pytest.mark.parametrize("name", NAMES)
def test_feature_map_matches_oracle(name, Cn):
    """|Fmap - ref| <= 1e-5 max(1, max |F|) on every pixel that ends its walk at the oracle's contributor; the pixels
    that do not are at most C.rounding_flip_caps' cap (f32 against f64 of the oracle alone).  ``background`` renders
    its colour over a non-zero background, which the feature map must ignore (the reference has none)."""
    from gaussian_splatting_amd import _C as CM

    inp = _built(name)
    F, _ = _FU(name, Cn)
    ref = _ref(name, Cn)
    fwd = _forward(inp)
    got = _np(_fmap(inp, fwd, F)).astype(np.float64)
    assert got.shape == (Cn, inp["H"], inp["W"]) and np.isfinite(got).all()
    st = CM.debug_forward_state(fwd[:7], inp["means3D"].shape[0])
    same = st["n_contrib"].numpy() == ref["n_contrib"]
    _, cap_nc, oracle_counts = _caps(name)
    d = np.abs(got - ref["Fmap"]).max(0)
    bar = ATOL_FWD * max(1.0, float(F.abs().max()))
    print(f"[{name} C={Cn}] max |Fmap - ref| = {d[same].max():.2e} (bar {bar:.2e}) over {int(same.sum())} pixels; "
          f"left out {int((~same).sum())} (cap {cap_nc}; f32 oracle vs f64 oracle {oracle_counts})")
    assert int((~same).sum()) <= cap_nc
    assert d[same].max() <= bar
    untouched = st["n_contrib"].numpy() == 0
    assert (got[:, untouched] == 0.0).all()
    if name == "background":
        assert float(inp["bg"].abs().max()) > 0 and untouched.any()


# ---- 2. the forward against the project's own colour ------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_feature_map_of_the_colours_is_the_colour(name):
    """F = colors_precomp (C = 3, bg = 0): the same forward's colour within 1e-5 on EVERY pixel (one discrete state)."""
    inp = _built(name)
    F = torch.rand(inp["means3D"].shape[0], 3, generator=torch.Generator().manual_seed(5))
    a = _as_colours(inp, F)
    fwd = _forward(a)
    d = (_fmap(a, fwd, F) - fwd[1]).abs().max().item()
    print(f"[{name}] max |Fmap - colour| = {d:.2e}")
    assert d <= ATOL_FWD


# ---- 3. the backward against the oracle, on both paths ------------------------------------------------------
def _check_grads(tag, L, ref, with_F=True):
    errs = {}
    if with_F:
        errs["dL_dF"] = C.rel_err(_np(L["features"].grad), ref["dL_dF"])
    for k, leaf in LEAF_OF.items():
        got = _np(L[leaf].grad)
        assert got.shape == ref[k].shape, (k, got.shape, ref[k].shape)
        assert np.isfinite(got).all(), k
        assert np.abs(ref[k]).max() > 0, k
        errs[k] = C.rel_err(got, ref[k])
    print(f"[{tag}] " + " ".join(f"{k[3:]}={e:.1e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= RTOL_BWD, (k, e)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("Cn", CHANNELS)
@pytest.mark.parametrize("name", NAMES)
def test_feature_backward_matches_oracle(name, Cn, path):
    """A loss on the feature map alone: dL_dF and the five geometry gradients against the chunked oracle."""
    inp = _built(name)
    if name == "pose_clamped":
        C.assert_clamp_preconditions(inp, _oracle(name))
    F, U = _FU(name, Cn)
    outs, L = _render(inp, F)
    assert len(outs) == 4 and outs[3].requires_grad
    (outs[3] * U.to(DEV)).sum().backward()
    _check_grads(f"{name} C={Cn} {path}", L, _ref(name, Cn))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", NAMES)
def test_joint_loss_matches_the_sum_of_the_references(name, path):
    """Colour + inverse depth + alpha + features in one backward: every leaf's gradient is the sum of the two nodes'."""
    Cn = 7
    inp = _built(name)
    F, U = _FU(name, Cn)
    g_c, g_d = C.unit_grads(inp["H"], inp["W"])
    g_a = AR.alpha_grad(inp["H"], inp["W"])
    (color, _radii, invd, alpha, fmap), L = _render(inp, F, return_alpha=True)
    loss = (color * g_c.to(DEV)).sum() + (invd * g_d.to(DEV)).sum() + (alpha * g_a.to(DEV)).sum() \
        + (fmap * U.to(DEV)).sum()
    loss.backward()
    first = AR.oracle_joint_grads(inp, g_c, g_d, g_a, ref=_oracle(name))
    feat = _ref(name, Cn)
    ref = {k: first[k] + feat[k] for k in LEAF_OF}
    ref["dL_dF"] = feat["dL_dF"]
    _check_grads(f"{name} joint {path}", L, ref)
    assert C.rel_err(_np(L["shs"].grad), first["dL_dsh"]) <= RTOL_BWD  # the colours see the colour loss alone


# ---- 4. the backward against the project's own colour backward ----------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_feature_backward_of_the_colours_is_the_colour_backward(name):
    inp = _built(name)
    P, H, W = inp["means3D"].shape[0], inp["H"], inp["W"]
    F = torch.rand(P, 3, generator=torch.Generator().manual_seed(5))
    U = FR.make_upstream(3, H, W)
    a = _as_colours(inp, F)
    fwd = _forward(a)
    col = dict(zip(C.GRAD_NAMES, _backward(a, fwd, U, torch.zeros(1, H, W))))
    outs, L = _render(a, F)
    (outs[3] * U.to(DEV)).sum().backward()
    ref = {k: _np(col[k]) for k in LEAF_OF}
    ref["dL_dF"] = _np(col["dL_dcolors"])
    _check_grads(f"{name} vs colour", L, ref)


# ---- 5. frozen geometry -------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [3, 35])
@pytest.mark.parametrize("name", ["ragged_37x23", "dense_opaque", "lists_over_8k"])
def test_frozen_geometry_gives_the_same_feature_gradient(name, Cn):
    """Only ``features`` requires grad: the kernel variant without the geometry part.  dL_dF is added with float
    atomics in the hardware's order, so it equals the full variant's within 1e-6 of max |ref|, not bit for bit."""
    inp = _built(name)
    F, U = _FU(name, Cn)
    outs, L = _render(inp, F)
    (outs[3] * U.to(DEV)).sum().backward()
    outs_f, Lf = _render(inp, F, geom_grad=False)
    assert outs_f[3].requires_grad and torch.equal(outs_f[3], outs[3])
    (outs_f[3] * U.to(DEV)).sum().backward()
    e = C.rel_err(_np(Lf["features"].grad), _np(L["features"].grad))
    print(f"[{name} C={Cn}] frozen vs full dL_dF: {e:.1e}")
    assert e <= 1e-6
    assert C.rel_err(_np(Lf["features"].grad), _ref(name, Cn)["dL_dF"]) <= RTOL_BWD
    for k in ("means3D", "means2D", "opacities", "scales", "rotations", "shs"):
        assert Lf[k].grad is None, k


# ---- 6. nothing else moved ------------------------------------------------------------------------------------
@pytest.mark.record_path
@pytest.mark.parametrize("name", ["background", "lists_1k_2k"])
def test_the_keyword_changes_nothing_else(name):
    inp = _built(name)
    F, _ = _FU(name, 7)
    g_c, g_d = C.unit_grads(inp["H"], inp["W"])
    kw = dict(return_alpha=True, return_contrib=True)
    plain, Lp = _render(inp, **kw)
    with_f, Lw = _render(inp, F, **kw)
    assert len(plain) == 5 and len(with_f) == 6
    color, radii, invd, alpha, fmap, stats = with_f
    assert tuple(fmap.shape) == (7, inp["H"], inp["W"]) and not stats.requires_grad
    for a, b in zip((color, radii, invd, alpha), plain[:4]):
        assert torch.equal(a, b)
    assert torch.equal(stats[:, 1:3].view(torch.int32), plain[4][:, 1:3].view(torch.int32))
    for col in (0, 3):  # (the statistics' two sums are added atomically)
        assert C.rel_err(_np(stats[:, col]), _np(plain[4][:, col])) <= RTOL_BWD
    # a loss that does not use the feature map: the colour node's backward gives the same bits
    for outs in (plain, with_f):
        torch.autograd.backward([outs[0], outs[2]], [g_c.to(DEV), g_d.to(DEV)])
    for k in ("means2D", "means3D", "opacities", "shs", "scales", "rotations"):
        assert torch.equal(Lp[k].grad, Lw[k].grad), k
    assert Lw["features"].grad is None
    # without the keyword the tuple is the one before the feature
    assert len(_render(inp)[0]) == 3 and len(_render(inp, F)[0]) == 4


@pytest.mark.parametrize("name", ["dense_opaque", "lists_over_8k", "pose_clamped"])
def test_feature_map_is_bitwise_reproducible_under_every_forward(name):
    """The weights depend on the forward's discrete state alone: the same bits from a second call, from copies of the
    buffers, after a whole-tile forward ("fwd_quads" 4), a half-tile one (2) and a no_backward forward."""
    from gaussian_splatting_amd import _lib

    inp = _built(name)
    F, _ = _FU(name, 35)
    fwd = _forward(inp)
    base = _fmap(inp, fwd, F)
    assert float(base.abs().max()) > 0
    assert torch.equal(_fmap(inp, fwd, F), base)
    assert torch.equal(_fmap(inp, fwd[:3] + tuple(t.clone() for t in fwd[3:6]), F), base)
    for q in (2, 4):
        with _lib.options(fwd_quads=q):
            assert torch.equal(_fmap(inp, _forward(inp), F), base), q
    assert torch.equal(_fmap(inp, _forward(inp, no_backward=True), F), base)


@pytest.mark.parametrize("path", ["atomic", "record"])
def test_colour_backward_is_unaffected_by_the_feature_calls(path):
    """The feature forward and backward read the buffers only: a colour backward after them equals a fresh one."""
    from gaussian_splatting_amd import _C, _lib

    name = "lists_1k_2k"
    inp = _built(name)
    P, H, W = inp["means3D"].shape[0], inp["H"], inp["W"]
    F, U = _FU(name, 16)
    g_c, g_d = C.unit_grads(H, W)
    with _lib.options(bwd_atomic=1 if path == "atomic" else 0):
        fwd = _forward(inp)
        fmap = _fmap(inp, fwd, F)
        nr, _c, radii, geom, binning, img = fwd[:6]
        geometry = dict(viewmatrix=inp["viewmatrix"].to(DEV), projmatrix=inp["projmatrix"].to(DEV),
                        campos=inp["campos"].to(DEV), tanfovx=inp["tanfovx"], tanfovy=inp["tanfovy"],
                        antialiasing=inp["antialiasing"], radii=radii)
        dF, block = _C.render_features_backward(geom, binning, img, nr, P, H, W, F.to(DEV), fmap, U.to(DEV),
                                                geometry=geometry)
        after = _backward(inp, fwd, g_c, g_d)
        fresh = _backward(inp, _forward(inp), g_c, g_d)
        torch.cuda.synchronize()
    assert block.numel() == _C.view_block_floats(P)
    assert C.rel_err(_np(dF), _ref(name, 16)["dL_dF"]) <= RTOL_BWD
    for k, a, b in zip(C.GRAD_NAMES, after, fresh):
        if path == "record":
            assert torch.equal(a, b), k
        else:  # (float atomics: the hardware's order)
            assert C.rel_err(_np(a), _np(b)) <= RTOL_BWD, k


# ---- 7. edges ---------------------------------------------------------------------------------------------------
def test_empty_and_culled_scenes():
    from gaussian_splatting_amd import _C

    inp = dict(C.build(C.Case("tmp", P=10, W=37, H=23)))
    for k in ("means3D", "opacities", "shs", "scales", "rotations"):
        inp[k] = inp[k][:0]
    outs, L = _render(inp, torch.zeros(0, 5))
    assert len(outs) == 4 and tuple(outs[3].shape) == (5, 23, 37) and not _np(outs[3]).any()
    outs[3].sum().backward()
    assert tuple(L["features"].grad.shape) == (0, 5)
    # every Gaussian behind the camera: num_rendered == 0, a zero map, zero gradients
    inp = dict(C.build(C.Case("behind", P=50, W=37, H=23, bg=(0.1, 0.2, 0.3))))
    inp["means3D"] = inp["means3D"].clone()
    inp["means3D"][:, 2] = -5.0
    F = FR.make_features(50, 5)
    fwd = _forward(inp)
    assert fwd[0] == 0 and not _np(_fmap(inp, fwd, F)).any()
    outs, L = _render(inp, F)
    assert not _np(outs[3]).any()
    (outs[3] * FR.make_upstream(5, 23, 37).to(DEV)).sum().backward()
    for k in ("features", "means3D", "means2D", "opacities", "scales", "rotations"):
        assert tuple(L[k].grad.shape) == tuple(L[k].shape) and not _np(L[k].grad).any(), k
    with pytest.raises(RuntimeError, match="C >= 1"):
        _C.render_features(*fwd[3:6], fwd[0], 50, 23, 37, torch.zeros(50, 0, device=DEV))


def test_bad_arguments_are_refused_and_the_library_stays_usable():
    from gaussian_splatting_amd import _lib

    name = "ragged_37x23"
    inp = _built(name)
    P, H, W = inp["means3D"].shape[0], inp["H"], inp["W"]
    F, _ = _FU(name, 3)
    fwd = _forward(inp)
    nr, _c, _r, geom, binning, img = fwd[:6]
    Fd, out = F.to(DEV), torch.zeros(3, H, W, device=DEV)
    lib = _lib.load()
    bufs = (geom.data_ptr(), binning.data_ptr(), img.data_ptr(), 0, binning.numel())
    bad = [((P, 0, nr, W, H, *bufs, Fd.data_ptr(), out.data_ptr(), None), b"C=0"),
           ((P, 3, nr, W, H, *bufs, None, out.data_ptr(), None), b"null"),
           ((P, 3, nr, W, H, *bufs, Fd.data_ptr(), None, None), b"null"),
           ((P, 3, nr, W, H, *bufs[:4], binning.numel() + 8, Fd.data_ptr(), out.data_ptr(), None), b"no layout"),
           ((P, 3, nr, W, H, None, None, None, 0, 0, Fd.data_ptr(), out.data_ptr(), None), b"missing")]
    for args, msg in bad:
        assert lib.gsr_render_features(*args) == 1, msg  # GSR_ERR_ARGUMENT
        assert msg in lib.gsr_last_error(), (msg, lib.gsr_last_error())
    assert not _np(out).any()
    assert np.abs(_np(_fmap(inp, fwd, F)) - _ref(name, 3)["Fmap"]).max() <= 1e-4  # (still usable)


def test_no_grad_render():
    name = "ragged_37x23"
    inp = _built(name)
    F, _ = _FU(name, 7)
    outs, _ = _render(inp, F)
    with torch.no_grad():
        outs_n, _ = _render(inp, F, return_alpha=True)
    assert len(outs_n) == 5 and not outs_n[4].requires_grad
    assert torch.equal(outs_n[4], outs[3]) and torch.equal(outs_n[0], outs[0])


@pytest.mark.record_path
def test_camera_node_with_features():
    """The camera node hands its buffers over like the plain one; the feature loss does not reach the camera tensors,
    whose gradients are those of the colour loss alone."""
    name = "pose_general"
    inp = _built(name)
    F, U = _FU(name, 7)
    g_c, g_d = C.unit_grads(inp["H"], inp["W"])
    outs_p, Lp = _render(inp, cam_grad=True)
    ((outs_p[0] * g_c.to(DEV)).sum() + (outs_p[2] * g_d.to(DEV)).sum()).backward()
    outs, L = _render(inp, F, cam_grad=True)
    ((outs[0] * g_c.to(DEV)).sum() + (outs[2] * g_d.to(DEV)).sum() + (outs[3] * U.to(DEV)).sum()).backward()
    for k in ("viewmatrix", "projmatrix", "campos"):
        assert float(Lp[k].grad.abs().max()) > 0 and torch.equal(L[k].grad, Lp[k].grad), k
    assert C.rel_err(_np(L["features"].grad), _ref(name, 7)["dL_dF"]) <= RTOL_BWD
    assert not torch.equal(L["means3D"].grad, Lp["means3D"].grad)  # the geometry does see the feature loss


def test_cov3d_precomp():
    name = "cov3d_precomp"
    inp = _built(name)
    F, U = _FU(name, 7)
    with pytest.raises(RuntimeError, match="cov3D_precomp"):
        _render(inp, F)
    outs, L = _render(inp, F, geom_grad=False)  # no geometry gradient required: accepted
    (outs[3] * U.to(DEV)).sum().backward()
    assert C.rel_err(_np(L["features"].grad), _ref(name, 7)["dL_dF"]) <= RTOL_BWD
    with torch.no_grad():
        assert torch.equal(_render(inp, F)[0][3], outs[3])
