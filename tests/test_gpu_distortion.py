"""The depth-distortion map on the GPU: ``_C.render_distortion`` / ``_C.render_distortion_backward`` (include/gsr.h
gsr_render_distortion / gsr_render_distortion_backward; csrc/distortion.hip) and ``distortion=`` through the autograd
nodes.

Reference: tests/distortion_ref.py -- the symmetric form ``sum_{i,j} w_i w_j |t_i - t_j|`` in float64 from the per-pixel
weights of the unchanged oracle, and the oracle's colour backward for the geometry, which tests/test_distortion_ref.py
pins on the CPU.  ``t`` is the view depth ``(means3D, 1) @ viewmatrix[:, 2]`` in float32: monotone along every list up
to one ulp of the sort key, which moves D by about 1e-6 at most.  Bars: the project's ATOL_FWD = 1e-5 times the map's
sensitivity to a weight, ``|dD/dw| <= 2 (max t - min t)``, i.e. ``1e-5 max(1, 2 spread)`` per pixel, and RTOL_BWD = 2e-4
of max |ref| per gradient tensor.  Each reference is computed once per case and shared read-only.
"""
import functools

import numpy as np
import pytest
import torch

from tests import alpha_ref as AR
from tests import common as C
from tests import contrib_ref as CR
from tests import distortion_ref as DR
from tests import features_ref as FR
from tests.test_gpu_alpha import _backward, _forward

pytestmark = pytest.mark.gpu

ATOL_FWD = 1e-5
RTOL_BWD = 2e-4
DEV = "cuda"
NAMES = ["ragged_37x23", "background", "antialiasing", "lists_1k_2k", "lists_over_8k", "pose_clamped"]
PATHS = [pytest.param("atomic", id="atomic"), pytest.param("record", marks=pytest.mark.record_path, id="record")]
LEAF_OF = {"dL_dmeans3D": "means3D", "dL_dmeans2D": "means2D", "dL_dopacity": "opacities", "dL_dscales": "scales",
           "dL_drotations": "rotations"}


def _case(name):
    return next(c for c in C.SMALL_CASES + C.POSE_CASES if c.name == name)


def _np(t):
    return t.detach().float().cpu().numpy()


def _threads(name):
    return 4 if name.startswith("lists_") else 1


@functools.lru_cache(maxsize=None)
def _built(name):
    return C.build(_case(name))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return C.run_oracle(_built(name), nthreads=_threads(name))


@functools.lru_cache(maxsize=None)
def _caps(name):
    return C.rounding_flip_caps(_built(name), _oracle(name), nthreads=_threads(name))


@functools.lru_cache(maxsize=None)
def _tU(name):
    inp = _built(name)
    return DR.view_depth(inp), DR.make_upstream(inp["H"], inp["W"])


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The reference map and gradients of a named case, computed once, read-only."""
    inp = _built(name)
    nt = _threads(name)
    w = CR.per_pixel_weights(_oracle(name), inp["H"], inp["W"], nt)
    return DR.oracle_distortion(inp, *_tU(name), nthreads=nt, ref=_oracle(name), w=w)


@functools.lru_cache(maxsize=None)
def _feat(name):
    """The 7-channel feature reference of the joint loss: (F, U, oracle result)."""
    inp = _built(name)
    F, U = FR.make_features(inp["means3D"].shape[0], 7), FR.make_upstream(7, inp["H"], inp["W"])
    return F, U, FR.oracle_features(inp, F, U, nthreads=_threads(name))


def _bar(t):
    return ATOL_FWD * max(1.0, 2.0 * float(t.max() - t.min()))


def _dmap(inp, fwd, t):
    from gaussian_splatting_amd import _C

    nr, _c, _r, geom, binning, img = fwd[:6]
    return _C.render_distortion(geom, binning, img, nr, inp["means3D"].shape[0], inp["H"], inp["W"], t.to(DEV))[0]


def _render(inp, t=None, F=None, geom_grad=True, t_grad=True, cam_grad=False, **kw):
    """GaussianRasterizer on ``inp`` with the per-Gaussian inputs as leaves; returns (outputs, leaves)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from tests.test_gpu_camera import _settings

    per_gaussian = ("means3D", "opacities", "shs", "scales", "rotations", "colors_precomp", "cov3D_precomp")
    L = {k: inp[k].to(DEV).requires_grad_(geom_grad) for k in per_gaussian if inp.get(k) is not None}
    L["means2D"] = torch.zeros_like(L["means3D"], requires_grad=geom_grad)
    cam = tuple(inp[k].to(DEV).requires_grad_(cam_grad) for k in ("viewmatrix", "projmatrix", "campos"))
    L.update(zip(("viewmatrix", "projmatrix", "campos"), cam))
    if F is not None:
        L["features"] = F.to(DEV).requires_grad_(True)
        kw["features"] = L["features"]
    if t is not None:
        L["t"] = t.to(DEV).requires_grad_(t_grad)
        kw["distortion"] = L["t"]
    args = dict(means3D=L["means3D"], means2D=L["means2D"], opacities=L["opacities"],
                colors_precomp=L.get("colors_precomp"), scales=L.get("scales"), rotations=L.get("rotations"),
                cov3D_precomp=L.get("cov3D_precomp"), shs=L.get("shs"))
    return GaussianRasterizer(_settings(inp, *cam))(**args, **kw), L


# ---- 1. the forward against the reference -------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_distortion_map_matches_reference(name):
    """|D - D_ref| <= 1e-5 max(1, 2 spread) on every pixel that ends its walk at the oracle's contributor; the pixels
    that do not are at most C.rounding_flip_caps' cap.  ``background`` renders over a non-zero background, which the
    map must ignore."""
    from gaussian_splatting_amd import _C as CM

    inp = _built(name)
    t, _ = _tU(name)
    ref = _ref(name)
    fwd = _forward(inp)
    got = _np(_dmap(inp, fwd, t)).astype(np.float64)
    assert got.shape == (1, inp["H"], inp["W"]) and np.isfinite(got).all()
    st = CM.debug_forward_state(fwd[:7], inp["means3D"].shape[0])
    same = st["n_contrib"].numpy() == ref["n_contrib"]
    _, cap_nc, oracle_counts = _caps(name)
    d = np.abs(got[0] - ref["D"])
    bar = _bar(t)
    print(f"[{name}] max |D - ref| = {d[same].max():.2e} (bar {bar:.2e}, max D {ref['D'].max():.3g}) over "
          f"{int(same.sum())} pixels; left out {int((~same).sum())} (cap {cap_nc}; f32 oracle vs f64 oracle "
          f"{oracle_counts})")
    assert ref["D"].max() > 10 * bar  # (the map is not small against its bar)
    assert int((~same).sum()) <= cap_nc
    assert d[same].max() <= bar
    untouched = st["n_contrib"].numpy() == 0
    assert (got[0][untouched] == 0.0).all()
    if name == "background":
        assert float(inp["bg"].abs().max()) > 0 and untouched.any()


# ---- 2. the backward against the reference, on both paths ----------------------------------------------------
def _check_grads(tag, L, ref):
    errs = {"dL_dt": C.rel_err(_np(L["t"].grad), ref["dL_dt"])}
    assert np.abs(ref["dL_dt"]).max() > 0
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
@pytest.mark.parametrize("name", NAMES)
def test_distortion_backward_matches_reference(name, path):
    """A loss on the distortion map alone: dL_dt and the five geometry gradients."""
    inp = _built(name)
    if name == "pose_clamped":
        C.assert_clamp_preconditions(inp, _oracle(name))
    t, U = _tU(name)
    outs, L = _render(inp, t)
    assert len(outs) == 4 and outs[3].requires_grad and tuple(outs[3].shape) == (1, inp["H"], inp["W"])
    (outs[3] * U.to(DEV)).sum().backward()
    _check_grads(f"{name} {path}", L, _ref(name))


def test_gradients_reach_what_t_was_built_from():
    """t built in torch from the means3D leaf and a camera leaf: means3D.grad is the kernel's geometry gradient plus
    dL_dt chained through the view depth, and the camera tensor receives dL_dt's chain alone."""
    name = "ragged_37x23"
    inp = _built(name)
    _, U = _tU(name)
    ref = _ref(name)
    m = inp["means3D"].to(DEV).requires_grad_(True)
    V = inp["viewmatrix"].to(DEV).requires_grad_(True)
    t = (torch.cat([m, torch.ones_like(m[:, :1])], 1) @ V[:, 2]).contiguous()
    from diff_gaussian_rasterization import GaussianRasterizer
    from tests.test_gpu_camera import _settings

    s = _settings(inp, inp["viewmatrix"].to(DEV), inp["projmatrix"].to(DEV), inp["campos"].to(DEV))
    outs = GaussianRasterizer(s)(means3D=m, means2D=torch.zeros_like(m), opacities=inp["opacities"].to(DEV),
                                 shs=inp["shs"].to(DEV), scales=inp["scales"].to(DEV),
                                 rotations=inp["rotations"].to(DEV), distortion=t)
    (outs[3] * U.to(DEV)).sum().backward()
    col = inp["viewmatrix"].double().numpy()[:, 2]
    want_m = ref["dL_dmeans3D"] + np.outer(ref["dL_dt"], col[:3])
    want_V = np.concatenate([inp["means3D"].double().numpy(), np.ones((m.shape[0], 1))], 1).T @ ref["dL_dt"]
    e_m, e_V = C.rel_err(_np(m.grad), want_m), C.rel_err(_np(V.grad)[:, 2], want_V)
    print(f"means3D {e_m:.1e} viewmatrix[:, 2] {e_V:.1e}")
    assert e_m <= RTOL_BWD and e_V <= RTOL_BWD
    assert not _np(V.grad)[:, [0, 1, 3]].any()


# ---- 3. the joint loss ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", NAMES)
def test_joint_loss_matches_the_sum_of_the_references(name, path):
    """Colour + inverse depth + alpha + a 7-channel feature map + distortion in one backward: every leaf's gradient
    is the sum of the three nodes'."""
    inp = _built(name)
    H, W = inp["H"], inp["W"]
    t, U = _tU(name)
    F, UF, feat = _feat(name)
    g_c, g_d = C.unit_grads(H, W)
    g_a = AR.alpha_grad(H, W)
    (color, _radii, invd, alpha, fmap, dmap), L = _render(inp, t, F, return_alpha=True)
    assert tuple(fmap.shape) == (7, H, W) and tuple(dmap.shape) == (1, H, W)
    loss = (color * g_c.to(DEV)).sum() + (invd * g_d.to(DEV)).sum() + (alpha * g_a.to(DEV)).sum() \
        + (fmap * UF.to(DEV)).sum() + (dmap * U.to(DEV)).sum()
    loss.backward()
    first = AR.oracle_joint_grads(inp, g_c, g_d, g_a, ref=_oracle(name))
    dist = _ref(name)
    ref = {k: first[k] + feat[k] + dist[k] for k in LEAF_OF}
    ref["dL_dt"] = dist["dL_dt"]
    _check_grads(f"{name} joint {path}", L, ref)
    assert C.rel_err(_np(L["features"].grad), feat["dL_dF"]) <= RTOL_BWD
    assert C.rel_err(_np(L["shs"].grad), first["dL_dsh"]) <= RTOL_BWD  # the colours see the colour loss alone


# ---- 4. frozen geometry --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_37x23", "lists_1k_2k", "lists_over_8k"])
def test_frozen_geometry_gives_the_same_t_gradient(name):
    """Only ``t`` requires grad: the kernel variant without the geometry part.  dL_dt is added with float atomics in
    the hardware's order, so it equals the full variant's within 1e-6 of max |ref|, not bit for bit."""
    inp = _built(name)
    t, U = _tU(name)
    outs, L = _render(inp, t)
    (outs[3] * U.to(DEV)).sum().backward()
    outs_f, Lf = _render(inp, t, geom_grad=False)
    assert outs_f[3].requires_grad and torch.equal(outs_f[3], outs[3])
    (outs_f[3] * U.to(DEV)).sum().backward()
    e = C.rel_err(_np(Lf["t"].grad), _np(L["t"].grad))
    print(f"[{name}] frozen vs full dL_dt: {e:.1e}")
    assert e <= 1e-6
    assert C.rel_err(_np(Lf["t"].grad), _ref(name)["dL_dt"]) <= RTOL_BWD
    for k in ("means3D", "means2D", "opacities", "scales", "rotations", "shs"):
        assert Lf[k].grad is None, k


# ---- 5. invariances ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_37x23", "lists_1k_2k", "pose_clamped"])
def test_invariances(name):
    """D is a function of the differences of t, homogeneous of degree 1 in t: a constant t gives zero, a shift changes
    nothing and a factor of two doubles the map, each within the forward's bar."""
    inp = _built(name)
    t, _ = _tU(name)
    fwd = _forward(inp)
    bar = _bar(t)
    base = _dmap(inp, fwd, t)
    const = _dmap(inp, fwd, torch.full_like(t, float(t.mean())))
    shifted = _dmap(inp, fwd, t + 2.5)
    doubled = _dmap(inp, fwd, 2 * t)
    e = [float(const.abs().max()), float((shifted - base).abs().max()), float((doubled - 2 * base).abs().max())]
    print(f"[{name}] constant {e[0]:.2e} shift {e[1]:.2e} scale {e[2]:.2e} (bar {bar:.2e}, max D {float(base.max()):.3g})")
    assert float(base.max()) > 100 * bar
    assert e[0] <= ATOL_FWD  # (the bar of a constant t: its spread is zero)
    assert e[1] <= bar and e[2] <= bar


# ---- 6. reproducibility, read-only behaviour -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_37x23", "lists_over_8k", "pose_clamped"])
def test_distortion_map_is_bitwise_reproducible_under_every_forward(name):
    """The weights depend on the forward's discrete state alone: the same bits from a second call, from copies of the
    buffers, after a whole-tile forward ("fwd_quads" 4), a half-tile one (2) and a no_backward forward."""
    from gaussian_splatting_amd import _lib

    inp = _built(name)
    t, _ = _tU(name)
    fwd = _forward(inp)
    base = _dmap(inp, fwd, t)
    assert float(base.abs().max()) > 0
    assert torch.equal(_dmap(inp, fwd, t), base)
    assert torch.equal(_dmap(inp, fwd[:3] + tuple(b.clone() for b in fwd[3:6]), t), base)
    for q in (2, 4):
        with _lib.options(fwd_quads=q):
            assert torch.equal(_dmap(inp, _forward(inp), t), base), q
    assert torch.equal(_dmap(inp, _forward(inp, no_backward=True), t), base)


@pytest.mark.parametrize("path", ["atomic", "record"])
def test_colour_backward_is_unaffected_by_the_distortion_calls(path):
    """The distortion forward and backward read the buffers only: a colour backward after them equals a fresh one."""
    from gaussian_splatting_amd import _C, _lib

    name = "lists_1k_2k"
    inp = _built(name)
    P, H, W = inp["means3D"].shape[0], inp["H"], inp["W"]
    t, U = _tU(name)
    g_c, g_d = C.unit_grads(H, W)
    with _lib.options(bwd_atomic=1 if path == "atomic" else 0):
        fwd = _forward(inp)
        nr, _c, radii, geom, binning, img = fwd[:6]
        dmap, moments = _C.render_distortion(geom, binning, img, nr, P, H, W, t.to(DEV))
        geometry = dict(viewmatrix=inp["viewmatrix"].to(DEV), projmatrix=inp["projmatrix"].to(DEV),
                        campos=inp["campos"].to(DEV), tanfovx=inp["tanfovx"], tanfovy=inp["tanfovy"],
                        antialiasing=inp["antialiasing"], radii=radii)
        dt, block = _C.render_distortion_backward(geom, binning, img, nr, P, H, W, t.to(DEV), dmap, moments, U.to(DEV),
                                                  geometry=geometry)
        after = _backward(inp, fwd, g_c, g_d)
        fresh = _backward(inp, _forward(inp), g_c, g_d)
        torch.cuda.synchronize()
    assert block.numel() == _C.view_block_floats(P) and tuple(moments.shape) == (2, H, W)
    assert C.rel_err(_np(dt), _ref(name)["dL_dt"]) <= RTOL_BWD
    for k, a, b in zip(C.GRAD_NAMES, after, fresh):
        if path == "record":
            assert torch.equal(a, b), k
        else:  # (float atomics: the hardware's order)
            assert C.rel_err(_np(a), _np(b)) <= RTOL_BWD, k


# ---- 7. nothing else moved -----------------------------------------------------------------------------------
@pytest.mark.record_path
@pytest.mark.parametrize("name", ["background", "lists_1k_2k"])
def test_the_keyword_changes_nothing_else(name):
    inp = _built(name)
    t, _ = _tU(name)
    g_c, g_d = C.unit_grads(inp["H"], inp["W"])
    kw = dict(return_alpha=True, return_contrib=True)
    plain, Lp = _render(inp, **kw)
    with_t, Lw = _render(inp, t, **kw)
    assert len(plain) == 5 and len(with_t) == 6
    color, radii, invd, alpha, dmap, stats = with_t
    assert tuple(dmap.shape) == (1, inp["H"], inp["W"]) and dmap.requires_grad and not stats.requires_grad
    for a, b in zip((color, radii, invd, alpha), plain[:4]):
        assert torch.equal(a, b)
    assert torch.equal(stats[:, 1:3].view(torch.int32), plain[4][:, 1:3].view(torch.int32))
    # a loss that does not use the map: the colour node's backward gives the same bits
    for outs in (plain, with_t):
        torch.autograd.backward([outs[0], outs[2]], [g_c.to(DEV), g_d.to(DEV)])
    for k in ("means2D", "means3D", "opacities", "shs", "scales", "rotations"):
        assert torch.equal(Lp[k].grad, Lw[k].grad), k
    assert Lw["t"].grad is None
    # without the keyword the tuple is the one before the feature; with features= the map follows the feature map
    assert len(_render(inp)[0]) == 3 and len(_render(inp, t)[0]) == 4
    both = _render(inp, t, FR.make_features(inp["means3D"].shape[0], 3), **kw)[0]
    assert len(both) == 7 and tuple(both[4].shape) == (3, inp["H"], inp["W"])
    assert torch.equal(both[5], dmap) and torch.equal(both[3], alpha)


# ---- 8. edges ------------------------------------------------------------------------------------------------
def test_empty_and_culled_scenes():
    inp = dict(C.build(C.Case("tmp", P=10, W=37, H=23)))
    for k in ("means3D", "opacities", "shs", "scales", "rotations"):
        inp[k] = inp[k][:0]
    outs, L = _render(inp, torch.zeros(0))
    assert len(outs) == 4 and tuple(outs[3].shape) == (1, 23, 37) and not _np(outs[3]).any()
    outs[3].sum().backward()
    assert tuple(L["t"].grad.shape) == (0,)
    # every Gaussian behind the camera: num_rendered == 0, a zero map, zero gradients
    inp = dict(C.build(C.Case("behind", P=50, W=37, H=23, bg=(0.1, 0.2, 0.3))))
    inp["means3D"] = inp["means3D"].clone()
    inp["means3D"][:, 2] = -5.0
    t = torch.linspace(1.0, 2.0, 50)
    fwd = _forward(inp)
    assert fwd[0] == 0 and not _np(_dmap(inp, fwd, t)).any()
    outs, L = _render(inp, t)
    assert not _np(outs[3]).any()
    (outs[3] * DR.make_upstream(23, 37).to(DEV)).sum().backward()
    for k in ("t", "means3D", "means2D", "opacities", "scales", "rotations"):
        assert tuple(L[k].grad.shape) == tuple(L[k].shape) and not _np(L[k].grad).any(), k


def test_bad_arguments_are_refused_and_the_library_stays_usable():
    from gaussian_splatting_amd import _C, _lib

    name = "ragged_37x23"
    inp = _built(name)
    P, H, W = inp["means3D"].shape[0], inp["H"], inp["W"]
    t, U = _tU(name)
    fwd = _forward(inp)
    nr, _c, _r, geom, binning, img = fwd[:6]
    td, out, mom = t.to(DEV), torch.zeros(1, H, W, device=DEV), torch.zeros(2, H, W, device=DEV)
    lib = _lib.load()
    bufs = (geom.data_ptr(), binning.data_ptr(), img.data_ptr(), 0, binning.numel())
    o, m = out.data_ptr(), mom.data_ptr()
    bad = [((P, nr, 0, H, *bufs, td.data_ptr(), o, m, None), b"invalid sizes"),
           ((P, nr, W, H, *bufs, None, o, m, None), b"null"),
           ((P, nr, W, H, *bufs, td.data_ptr(), None, m, None), b"null"),
           ((P, nr, W, H, *bufs, td.data_ptr(), o, None, None), b"null"),
           ((P, nr, W, H, *bufs[:4], binning.numel() + 8, td.data_ptr(), o, m, None), b"no layout"),
           ((P, nr, W, H, None, None, None, 0, 0, td.data_ptr(), o, m, None), b"missing")]
    for args, msg in bad:
        assert lib.gsr_render_distortion(*args) == 1, msg  # GSR_ERR_ARGUMENT
        assert msg in lib.gsr_last_error(), (msg, lib.gsr_last_error())
    assert not _np(out).any() and not _np(mom).any()
    dmap, moments = _C.render_distortion(geom, binning, img, nr, P, H, W, td)
    ud, dt = U.to(DEV), torch.zeros(P, device=DEV)
    block = torch.zeros(_C.view_block_floats(P) + 4, device=DEV)
    cam = (None, None, None, 0.0, 0.0, 0, None, _lib.ALLOC_FN(), None, None)
    head = (P, nr, W, H, *bufs, td.data_ptr(), dmap.data_ptr(), moments.data_ptr())
    bad = [((*head, ud.data_ptr(), None, None, *cam), b"null"),
           ((*head, None, dt.data_ptr(), None, *cam), b"null"),
           ((*head, ud.data_ptr(), dt.data_ptr(), block.data_ptr() + 4, *cam), b"16-byte aligned"),
           ((*head, ud.data_ptr(), dt.data_ptr(), block.data_ptr(), *cam), b"needs the camera")]
    for args, msg in bad:
        assert lib.gsr_render_distortion_backward(*args) == 1, msg
        assert msg in lib.gsr_last_error(), (msg, lib.gsr_last_error())
    assert not _np(dt).any()
    assert np.abs(_np(_dmap(inp, fwd, t))[0] - _ref(name)["D"]).max() <= 10 * _bar(t)  # (still usable)


def test_no_grad_render():
    name = "ragged_37x23"
    inp = _built(name)
    t, _ = _tU(name)
    outs, _ = _render(inp, t)
    with torch.no_grad():
        outs_n, _ = _render(inp, t, return_alpha=True)
    assert len(outs_n) == 5 and not outs_n[4].requires_grad
    assert torch.equal(outs_n[4], outs[3]) and torch.equal(outs_n[0], outs[0])


@pytest.mark.record_path
def test_camera_node_with_distortion():
    """The camera node hands its buffers over like the plain one; the kernel's geometry part does not reach the camera
    tensors, whose gradients are those of the colour loss alone."""
    name = "pose_clamped"
    inp = _built(name)
    t, U = _tU(name)
    g_c, g_d = C.unit_grads(inp["H"], inp["W"])
    outs_p, Lp = _render(inp, cam_grad=True)
    ((outs_p[0] * g_c.to(DEV)).sum() + (outs_p[2] * g_d.to(DEV)).sum()).backward()
    outs, L = _render(inp, t, cam_grad=True)
    ((outs[0] * g_c.to(DEV)).sum() + (outs[2] * g_d.to(DEV)).sum() + (outs[3] * U.to(DEV)).sum()).backward()
    for k in ("viewmatrix", "projmatrix", "campos"):
        assert float(Lp[k].grad.abs().max()) > 0 and torch.equal(L[k].grad, Lp[k].grad), k
    assert C.rel_err(_np(L["t"].grad), _ref(name)["dL_dt"]) <= RTOL_BWD
    assert not torch.equal(L["means3D"].grad, Lp["means3D"].grad)  # the geometry does see the distortion loss


def test_cov3d_precomp():
    inp = _built("cov3d_precomp")
    t, U = DR.view_depth(inp), DR.make_upstream(inp["H"], inp["W"])
    with pytest.raises(RuntimeError, match="distortion= with cov3D_precomp"):
        _render(inp, t)
    outs, L = _render(inp, t, geom_grad=False)  # no geometry gradient required: accepted
    (outs[3] * U.to(DEV)).sum().backward()
    assert float(L["t"].grad.abs().max()) > 0
    with torch.no_grad():
        assert torch.equal(_render(inp, t)[0][3], outs[3])
