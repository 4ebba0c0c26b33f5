"""The accumulated-alpha output on the GPU: ``alpha = 1 - final_T`` [1,H,W] from
``rasterize_gaussians(..., return_alpha=True)`` (include/gsr.h gsr_render_alpha; csrc/alpha.hip) and its gradient
through ``rasterize_gaussians_backward(..., dL_dout_alpha=...)`` (gsr_backward_args.dL_dalphas; the seed of the
per-pixel scalar gB in csrc/render.hip render_bwd).

References: the product's own per-pixel state for the forward's bits, and the unchanged oracle -- the forward's
``final_T`` and, for gradients, the two-pass construction of tests/alpha_ref.py, which tests/test_alpha_ref.py
pins on the CPU.  Bars: the project's, ATOL_FWD = 1e-5 per pixel and RTOL_BWD = 2e-4 of max |ref| per tensor.
"""
import functools

import numpy as np
import pytest
import torch

from tests import alpha_ref as AR
from tests import common as C

pytestmark = pytest.mark.gpu

ATOL_FWD = 1e-5
RTOL_BWD = 2e-4
DEV = "cuda"
PATHS = [pytest.param("atomic", id="atomic"), pytest.param("record", marks=pytest.mark.record_path, id="record")]
BWD_NAMES = ["sh3_scalerot", "ragged_37x23", "background", "antialiasing", "cov3d_precomp", "colors_precomp",
             "dense_opaque", "lists_1k_2k", "pose_general", "pose_clamped"]


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


def _upstream(inp, loss):
    """(g_c, g_d, g_a): ``joint`` = C.unit_grads plus the seeded alpha gradient; ``alpha`` = that alone."""
    g_c, g_d = C.unit_grads(inp["H"], inp["W"])
    if loss == "alpha":
        g_c, g_d = torch.zeros_like(g_c), torch.zeros_like(g_d)
    return g_c, g_d, AR.alpha_grad(inp["H"], inp["W"])


@functools.lru_cache(maxsize=None)
def _ref_grads(name, loss):
    """The oracle's gradients of the loss for a named case (tests/alpha_ref.py), computed once, read-only."""
    inp = _built(name)
    return AR.oracle_joint_grads(inp, *_upstream(inp, loss), ref=_oracle(name))


def _forward(inp, sh=None, **kw):
    """_C.rasterize_gaussians on ``inp`` (C.run_gpu_forward's arguments; ``sh`` = (dc, rest) for the split form)."""
    from gaussian_splatting_amd import _C

    d = lambda k: C._dev(inp[k], DEV)  # noqa: E731
    sh = (d("shs"),) if sh is None else sh
    return _C.rasterize_gaussians(
        d("bg"), d("means3D"), d("colors_precomp"), d("opacities"), d("scales"), d("rotations"),
        inp["scale_modifier"], d("cov3D_precomp"), d("viewmatrix"), d("projmatrix"), inp["tanfovx"],
        inp["tanfovy"], inp["H"], inp["W"], *sh, inp["sh_degree"], d("campos"), False, inp["antialiasing"], False, **kw)


def _backward(inp, fwd, g_c, g_d, sh=None, **kw):
    from gaussian_splatting_amd import _C

    d = lambda k: C._dev(inp[k], DEV)  # noqa: E731
    nr, _color, radii, geom, binning, img, _invd = fwd[:7]
    sh = (d("shs"),) if sh is None else sh
    kw = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    return _C.rasterize_gaussians_backward(
        d("bg"), d("means3D"), radii, d("colors_precomp"), d("opacities"), d("scales"), d("rotations"),
        inp["scale_modifier"], d("cov3D_precomp"), d("viewmatrix"), d("projmatrix"), inp["tanfovx"], inp["tanfovy"],
        g_c.to(DEV), g_d.to(DEV), *sh, inp["sh_degree"], d("campos"), geom, nr, binning, img, inp["antialiasing"],
        False, **kw)


# ---- 1. the forward against the product's own state ------------------------------------------------------
@pytest.mark.parametrize("name,opts", [("ragged_37x23", {}), ("background", {}), ("dense_opaque", {}),
                                       ("lists_4k_8k", {"sort_prefix": 256, "near_mass": 0}),
                                       ("lists_4k_8k", {"near_mass": 1}),
                                       # (the two above redo no tile -- their walks end inside the prefix / the near
                                       # entries; these two do, as tests/test_gpu_parity.py asserts of them)
                                       ("lists_1k_2k", {"sort_prefix": 64, "near_mass": 0}),
                                       ("lists_2k_4k", {"near_mass": 1})],
                         ids=["ragged_37x23", "background", "dense_opaque", "sort_prefix_256", "near_mass_1",
                              "sort_prefix_64_redo", "near_mass_1_redo"])
def test_alpha_is_one_minus_final_T_bitwise(name, opts):
    """alpha == 1 - final_T of the forward's own per-pixel state, bit for bit: partial edge tiles, terminated
    pixels, tiles rendered again after the reachable-prefix sort and after a near-first cut."""
    from gaussian_splatting_amd import _C as CM
    from gaussian_splatting_amd import _lib

    inp = _built(name)
    key = (torch.cuda.current_device(), inp["W"], inp["H"])
    if "near_mass" in opts and opts["near_mass"]:
        CM._capacity[key] = (inp["means3D"].shape[0], _oracle(name).num_rendered)  # the hinted forward takes the cut
    try:
        with _lib.options(**opts):
            fwd = _forward(inp, return_alpha=True)
            plain = _forward(inp)
            st = CM.debug_forward_state(fwd[:7], inp["means3D"].shape[0])
            sort = CM.debug_sort_state(fwd[:7], inp["means3D"].shape[0])
    finally:
        CM._capacity.pop(key, None)
    assert len(fwd) == 8 and len(plain) == 7
    alpha = fwd[7]
    assert tuple(alpha.shape) == (1, inp["H"], inp["W"]) and alpha.dtype == torch.float32
    a = _np(alpha)[0]
    fT = st["final_T"].numpy()
    np.testing.assert_array_equal(a, np.float32(1) - fT)
    untouched = st["n_contrib"].numpy() == 0
    print(f"[{name} {opts}] pixels no Gaussian reaches: {int(untouched.sum())}, redone tiles {sort['redo_count']}, "
          f"alpha in [{a.min():.3g}, {a.max():.3g}]")
    assert (a[untouched] == 0.0).all()
    if name in ("ragged_37x23", "background"):
        assert untouched.any()
    if name == "dense_opaque":
        assert fT.min() < 2e-4  # pixels ended by the T < 1e-4 rule (final_T is T before the entry that ended them)
    if name in ("lists_1k_2k", "lists_2k_4k"):
        assert sort["redo_count"] > 0
    # asking for alpha changes nothing else
    for i in (1, 2, 6):
        assert torch.equal(fwd[i], plain[i])


def test_alpha_of_empty_and_culled_scenes():
    inp = dict(C.build(C.Case("tmp", P=10, W=37, H=23)))
    for k in ("means3D", "opacities", "shs", "scales", "rotations"):
        inp[k] = inp[k][:0]
    fwd = _forward(inp, return_alpha=True)
    assert fwd[0] == 0 and tuple(fwd[7].shape) == (1, 23, 37) and float(fwd[7].abs().max()) == 0.0
    g_c, g_d = C.unit_grads(23, 37)
    for t in _backward(inp, fwd, g_c, g_d, dL_dout_alpha=AR.alpha_grad(23, 37)):
        assert t.numel() == 0 or float(t.abs().max()) == 0.0
    # every Gaussian behind the camera: num_rendered == 0, alpha == 0 everywhere, all gradients zero
    inp = dict(C.build(C.Case("behind", P=50, W=37, H=23, bg=(0.1, 0.2, 0.3))))
    inp["means3D"] = inp["means3D"].clone()
    inp["means3D"][:, 2] = -5.0
    fwd = _forward(inp, return_alpha=True)
    assert fwd[0] == 0
    assert (_np(fwd[7]) == 0.0).all()
    for t in _backward(inp, fwd, g_c, g_d, dL_dout_alpha=AR.alpha_grad(23, 37)):
        assert float(t.abs().max()) == 0.0


# ---- 2. the forward against the oracle --------------------------------------------------------------------
@pytest.mark.parametrize("case", C.SMALL_CASES + C.POSE_CASES, ids=lambda c: c.name)
def test_alpha_matches_oracle(case):
    """|alpha - (1 - final_T of the f32 oracle)| <= 1e-5 on every pixel that ends its walk at the oracle's
    contributor; the pixels that do not are at most C.rounding_flip_caps' cap (f32 against f64 of the oracle alone)."""
    from gaussian_splatting_amd import _C as CM

    inp = _built(case.name)
    ref = _oracle(case.name)
    fwd = _forward(inp, return_alpha=True)
    st = CM.debug_forward_state(fwd[:7], case.P)
    same = st["n_contrib"].numpy() == ref.handle.image()["n_contrib"].astype(np.int64)
    _, cap_nc, oracle_counts = C.rounding_flip_caps(inp, ref)
    d = np.abs(_np(fwd[7])[0].astype(np.float64) - AR.oracle_alpha(ref))
    print(f"[{case.name}] max |alpha - ref| = {d[same].max():.2e} over {int(same.sum())} pixels; left out "
          f"{int((~same).sum())} (cap {cap_nc}; f32 oracle vs f64 oracle {oracle_counts})")
    assert int((~same).sum()) <= cap_nc
    assert d[same].max() <= ATOL_FWD


# ---- 3. backward parity on both paths ---------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("loss", ["alpha", "joint"])
@pytest.mark.parametrize("name", BWD_NAMES)
def test_alpha_backward_matches_oracle(name, loss, path):
    inp = _built(name)
    if name == "pose_clamped":
        C.assert_clamp_preconditions(inp, _oracle(name))
    g_c, g_d, g_a = _upstream(inp, loss)
    fwd = _forward(inp, return_alpha=True)
    out = dict(zip(C.GRAD_NAMES, _backward(inp, fwd, g_c, g_d, dL_dout_alpha=g_a)))
    torch.cuda.synchronize()
    ref = _ref_grads(name, loss)
    errs = {}
    for k in C.GRAD_NAMES:
        got, exp = _np(out[k]), ref[k]
        if k in ("dL_dscales", "dL_drotations") and inp["scales"] is None:
            exp = np.zeros_like(got)
        assert got.shape == exp.shape, (k, got.shape, exp.shape)
        assert np.isfinite(got).all(), k
        errs[k] = C.rel_err(got, exp)
    print(f"[{name}/{loss}/{path}] " + " ".join(f"{k[3:]}={e:.1e}" for k, e in errs.items()))
    if loss == "alpha":  # the alpha map does not depend on the colours
        assert not _np(out["dL_dcolors"]).any() and not _np(out["dL_dsh"]).any()
        assert np.abs(ref["dL_dopacity"]).max() > 0
    for k, e in errs.items():
        assert e <= RTOL_BWD, (k, e)


# ---- 4. nothing else moved --------------------------------------------------------------------------------
@pytest.mark.record_path
def test_no_alpha_gradient_is_the_plain_backward_bitwise():
    inp = _built("background")
    g_c, g_d, g_a = _upstream(inp, "joint")
    fwd = _forward(inp, return_alpha=True)
    plain = _backward(inp, fwd, g_c, g_d)
    for kw in ({"dL_dout_alpha": None}, {"dL_dout_alpha": torch.Tensor([])}):
        for a, b in zip(plain, _backward(inp, fwd, g_c, g_d, **kw)):
            assert torch.equal(a, b)
    # a zero alpha gradient adds nothing either (x - 0 is x), and the alpha loss is reproducible
    for a, b in zip(plain, _backward(inp, fwd, g_c, g_d, dL_dout_alpha=torch.zeros_like(g_a))):
        assert torch.equal(a, b)
    one = _backward(inp, fwd, g_c, g_d, dL_dout_alpha=g_a)
    two = _backward(inp, _forward(inp, return_alpha=True), g_c, g_d, dL_dout_alpha=g_a)
    assert not torch.equal(one[2], plain[2])
    for a, b in zip(one, two):
        assert torch.equal(a, b)


# ---- 5. autograd ------------------------------------------------------------------------------------------
def _module_render(inp, split=False, cam_grad=False, **kw):
    """GaussianRasterizer on ``inp`` with every per-Gaussian input a leaf; returns (outputs, leaves)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from tests.test_gpu_camera import _settings

    per_gaussian = ("means3D", "opacities", "shs", "scales", "rotations", "colors_precomp", "cov3D_precomp")
    L = {k: inp[k].to(DEV).requires_grad_(True) for k in per_gaussian if inp.get(k) is not None}
    L["means2D"] = torch.zeros_like(L["means3D"], requires_grad=True)
    cam = tuple(inp[k].to(DEV).requires_grad_(cam_grad) for k in ("viewmatrix", "projmatrix", "campos"))
    L.update(zip(("viewmatrix", "projmatrix", "campos"), cam))
    args = dict(means3D=L["means3D"], means2D=L["means2D"], opacities=L["opacities"],
                colors_precomp=L.get("colors_precomp"), scales=L.get("scales"), rotations=L.get("rotations"),
                cov3D_precomp=L.get("cov3D_precomp"), shs=L.get("shs"))
    if split:
        L["dc"] = L["shs"].detach()[:, :1].contiguous().requires_grad_(True)
        L["rest"] = L["shs"].detach()[:, 1:].contiguous().requires_grad_(True)
        args.update(dc=L["dc"], shs=L["rest"])
    return GaussianRasterizer(_settings(inp, *cam))(**args, **kw), L


@pytest.mark.record_path
@pytest.mark.parametrize("split", [False, True], ids=["combined", "dc"])
@pytest.mark.parametrize("name", ["sh3_scalerot", "pose_general"])
def test_autograd_alpha_matches_direct_calls_bitwise(name, split):
    inp = _built(name)
    g_c, g_d, g_a = _upstream(inp, "joint")
    (color, radii, invd, alpha), L = _module_render(inp, split=split, return_alpha=True)
    assert alpha.requires_grad and tuple(alpha.shape) == (1, inp["H"], inp["W"])
    loss = (color * g_c.to(DEV)).sum() + (invd * g_d.to(DEV)).sum() + (alpha * g_a.to(DEV)).sum()
    loss.backward()
    sh = (L["dc"].detach(), L["rest"].detach()) if split else None
    fwd = _forward(inp, sh=sh, return_alpha=True)
    out = _backward(inp, fwd, g_c, g_d, sh=sh, dL_dout_alpha=g_a)
    names = C.GRAD_NAMES[:5] + ["dL_ddc"] + C.GRAD_NAMES[5:] if split else C.GRAD_NAMES
    d = dict(zip(names, out))
    assert torch.equal(alpha, fwd[7]) and torch.equal(color, fwd[1]) and torch.equal(invd, fwd[6])
    pairs = [("means2D", "dL_dmeans2D"), ("means3D", "dL_dmeans3D"), ("opacities", "dL_dopacity"),
             ("scales", "dL_dscales"), ("rotations", "dL_drotations")]
    pairs += [("dc", "dL_ddc"), ("rest", "dL_dsh")] if split else [("shs", "dL_dsh")]
    for leaf, k in pairs:
        assert torch.equal(L[leaf].grad, d[k]), k
    # the alpha loss did reach the leaves: the same node without it gives other opacity gradients
    assert not torch.equal(d["dL_dopacity"], dict(zip(names, _backward(inp, fwd, g_c, g_d, sh=sh)))["dL_dopacity"])


@pytest.mark.record_path
def test_autograd_without_the_keyword_and_with_an_unused_alpha():
    inp = _built("sh3_scalerot")
    g_c, g_d, _ = _upstream(inp, "joint")
    out, L = _module_render(inp)
    assert len(out) == 3
    torch.autograd.backward([out[0], out[2]], [g_c.to(DEV), g_d.to(DEV)])
    # an alpha map the loss does not use gets no gradient (None -> NULL): the leaves' gradients are the same bits
    out_a, La = _module_render(inp, return_alpha=True)
    assert len(out_a) == 4
    torch.autograd.backward([out_a[0], out_a[2]], [g_c.to(DEV), g_d.to(DEV)])
    for k in ("means2D", "means3D", "opacities", "shs", "scales", "rotations"):
        assert torch.equal(L[k].grad, La[k].grad), k
    # and a loss on the alpha map alone runs (colour and inverse depth get zero gradients)
    out_b, Lb = _module_render(inp, return_alpha=True)
    out_b[3].sum().backward()
    assert float(Lb["opacities"].grad.abs().max()) > 0 and not Lb["shs"].grad.any()
    with torch.no_grad():
        out_c, _ = _module_render(inp, return_alpha=True)
    assert len(out_c) == 4 and torch.equal(out_c[3], out_a[3])


# ---- 6. camera gradients of an alpha loss -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["pose_general", "pose_principal"])
def test_camera_gradients_of_an_alpha_loss(name):
    inp = _built(name)
    g_a = AR.alpha_grad(inp["H"], inp["W"])
    (_color, _radii, _invd, alpha), L = _module_render(inp, cam_grad=True, return_alpha=True)
    (alpha * g_a.to(DEV)).sum().backward()
    ref = AR.camera_alpha_grads(inp, g_a)
    got = {"dL_dviewmatrix": L["viewmatrix"].grad, "dL_dprojmatrix": L["projmatrix"].grad,
           "dL_dcampos": L["campos"].grad}
    got = {k: v.detach().cpu().numpy() for k, v in got.items()}
    errs = {k: C.rel_err(got[k], ref[k]) for k in ("dL_dviewmatrix", "dL_dprojmatrix")}
    print(f"[{name}] " + " ".join(f"{k}={e:.1e}" for k, e in errs.items()))
    assert not ref["dL_dcampos"].any() and (got["dL_dcampos"] == 0).all()
    for k, e in errs.items():
        assert np.abs(ref[k]).max() > 0 and np.isfinite(got[k]).all(), k
        assert e <= RTOL_BWD, (k, e)
