"""Camera-pose gradients on the GPU: dL/dviewmatrix, dL/dprojmatrix, dL/dcampos (include/gsr.h
gsr_camera_backward; csrc/camera.hip) against the float64 reference tests/torch_ref_camera.py, which
tests/test_camera_ref.py checks on the CPU.

Bar: the project's gradient bar, max |gpu - ref| <= RTOL_BWD (2e-4) x max |ref| per tensor.  A float32 evaluation
of the reference's own autograd differs from the float64 one by at most 5e-6 of max |ref| on these cases.
Under antialiasing the reference differentiates its own forward and the product follows the original
rasterizer's formula (torch_ref's docstring), so dL/dviewmatrix is held to the rigid-motion identity there and
only dL/dprojmatrix and dL/dcampos, which do not pass through that chain, to the reference.
"""
import functools

import numpy as np
import pytest
import torch

from tests import common as C
from tests import torch_ref_camera as TRC
from tests.test_pose_equivariance import _grad_full

pytestmark = pytest.mark.gpu

RTOL_BWD = 2e-4
DEV = "cuda"
CAM = TRC.CAMERA_NAMES
POSE_NAMES = ["pose_general", "pose_back", "pose_principal", "pose_clamped", "pose_general_sh1",
              "pose_general_precomp", "pose_general_cov3d"]
SMALL_NAMES = ["sh3_scalerot", "ragged_37x23", "sh0_M1", "scale_modifier", "background"]
PER_GAUSSIAN = ("means3D", "opacities", "shs", "scales", "rotations", "colors_precomp", "cov3D_precomp")


def _case(name):
    for c in C.POSE_CASES + C.SMALL_CASES:
        if c.name == name:
            return c
    raise KeyError(name)


def _upstream(kind, H, W):
    return C.unit_grads(H, W) if kind == "unit" else C.l1_grads(H, W)


@functools.lru_cache(maxsize=None)
def _built(name):
    return C.build(_case(name))


@functools.lru_cache(maxsize=None)
def _ref(name, kind):
    """The float64 reference's gradients for a named case, computed once and never modified."""
    inp = _built(name)
    g = TRC.camera_grads(inp, *_upstream(kind, inp["H"], inp["W"]))
    for v in g.values():
        v.setflags(write=False)
    return g


def _settings(inp, view, proj, campos):
    from gaussian_splatting_amd import GaussianRasterizationSettings

    return GaussianRasterizationSettings(
        image_height=inp["H"], image_width=inp["W"], tanfovx=inp["tanfovx"], tanfovy=inp["tanfovy"],
        bg=inp["bg"].to(DEV), scale_modifier=inp["scale_modifier"], viewmatrix=view, projmatrix=proj,
        sh_degree=inp["sh_degree"], campos=campos, prefiltered=False, debug=False, antialiasing=inp["antialiasing"])


def _render(inp, cam=None, cam_grad=True, gauss_grad=True, split=False):
    """The product's render of ``inp`` through GaussianRasterizer.  ``cam``: the three camera tensors to use
    (default: leaves made from inp's).  Returns (color, radii, invdepth, leaves: dict)."""
    from gaussian_splatting_amd import GaussianRasterizer

    L = {k: inp[k].to(DEV).requires_grad_(gauss_grad) for k in PER_GAUSSIAN if inp.get(k) is not None}
    if cam is None:
        cam = tuple(inp[k].to(DEV).requires_grad_(cam_grad) for k in ("viewmatrix", "projmatrix", "campos"))
        L.update(zip(("viewmatrix", "projmatrix", "campos"), cam))
    L["means2D"] = torch.zeros_like(L["means3D"], requires_grad=gauss_grad)
    kw = dict(means3D=L["means3D"], means2D=L["means2D"], opacities=L["opacities"], colors_precomp=L.get("colors_precomp"),
              scales=L.get("scales"), rotations=L.get("rotations"), cov3D_precomp=L.get("cov3D_precomp"))
    if split and "shs" in L:
        L["dc"] = L["shs"].detach()[:, :1].contiguous().requires_grad_(gauss_grad)
        L["rest"] = L["shs"].detach()[:, 1:].contiguous().requires_grad_(gauss_grad)
        kw.update(dc=L["dc"], shs=L["rest"])
    else:
        kw.update(shs=L.get("shs"))
    color, radii, invd = GaussianRasterizer(_settings(inp, *cam))(**kw)
    return color, radii, invd, L


def _gpu_camera_grads(inp, kind="unit", **kw):
    """Camera gradients (and the leaves) of the product for the upstream gradients ``kind``."""
    color, radii, invd, L = _render(inp, **kw)
    gc, gd = _upstream(kind, inp["H"], inp["W"])
    torch.autograd.backward([color, invd], [gc.to(DEV), gd.to(DEV)])
    g = {"dL_dviewmatrix": L["viewmatrix"].grad, "dL_dprojmatrix": L["projmatrix"].grad, "dL_dcampos": L["campos"].grad}
    return {k: v.detach().cpu().numpy() for k, v in g.items()}, L, radii


def _assert_camera_close(got, ref, names=CAM, rtol=RTOL_BWD, tag=""):
    errs = {k: C.rel_err(got[k], ref[k]) for k in names}
    print(f"[{tag}] " + " ".join(f"{k}={e:.1e}" for k, e in errs.items()))
    for k in names:
        assert np.isfinite(got[k]).all(), k
        if np.abs(ref[k]).max() == 0:  # (campos with precomputed colours)
            assert (got[k] == 0).all(), k
        else:
            assert errs[k] <= rtol, (k, errs[k])
    # entries the forward never reads: exact zeros
    assert (got["dL_dviewmatrix"][:, 3] == 0).all() and (got["dL_dprojmatrix"][:, 2] == 0).all()


# ---- 3. parity with the float64 reference --------------------------------------------------------------
@pytest.mark.parametrize("kind", ["unit", "l1"])
@pytest.mark.parametrize("name", POSE_NAMES + SMALL_NAMES)
def test_camera_parity(name, kind):
    inp = _built(name)
    got, _, radii = _gpu_camera_grads(inp, kind)
    ref = _ref(name, kind)
    np.testing.assert_array_equal(radii.cpu().numpy() > 0, ref["radii"] > 0)
    _assert_camera_close(got, ref, tag=f"{name}/{kind}")


@pytest.mark.parametrize("kind", ["unit", "l1"])
def test_camera_parity_antialiasing(kind):
    inp = _built("pose_general_aa")
    got, _, _ = _gpu_camera_grads(inp, kind)
    _assert_camera_close(got, _ref("pose_general_aa", kind), names=["dL_dprojmatrix", "dL_dcampos"], tag=f"aa/{kind}")
    assert np.abs(got["dL_dviewmatrix"]).max() > 0


# ---- 4. the rigid-motion identity on the GPU's own outputs ----------------------------------------------
def _identity_residuals(inp):
    gc, gd = C.unit_grads(inp["H"], inp["W"])
    fwd = C.run_gpu_forward(inp, device=DEV)
    out = _backward(inp, fwd, gc, gd, camera=True)
    g = dict(zip(C.GRAD_NAMES + CAM, (t.detach().cpu().numpy() for t in out)))
    sides = np.array([TRC.twist_sides(tw, g, inp, _grad_full(g["dL_dcov3D"].astype(np.float64)), TRC.world_cov(inp))
                      for tw in TRC.TWISTS])
    scale = np.abs(sides).max()
    assert scale > 0
    return np.abs(sides[:, 0] - sides[:, 1]) / scale


def _backward(inp, fwd, gc, gd, camera, dc_rest=None):
    from gaussian_splatting_amd import _C

    d = lambda k: C._dev(inp[k], DEV)  # noqa: E731
    nr, _color, radii, geom, binning, img, _invd = fwd
    sh = (d("shs"),) if dc_rest is None else dc_rest
    kw = dict(camera=True) if camera else {}
    return _C.rasterize_gaussians_backward(
        d("bg"), d("means3D"), radii, d("colors_precomp"), d("opacities"), d("scales"), d("rotations"),
        inp["scale_modifier"], d("cov3D_precomp"), d("viewmatrix"), d("projmatrix"), inp["tanfovx"], inp["tanfovy"],
        gc.to(DEV), gd.to(DEV), *sh, inp["sh_degree"], d("campos"), geom, nr, binning, img, inp["antialiasing"],
        False, **kw)


def test_rigid_motion_identity_precomputed_colours():
    r = _identity_residuals(_built("pose_general_precomp"))
    print("precomp:", " ".join(f"{x:.1e}" for x in r))
    assert (r <= RTOL_BWD).all(), r


def test_rigid_motion_identity_sh3_translations():
    r = _identity_residuals(_built("pose_general"))
    print("sh3:", " ".join(f"{x:.1e}" for x in r))
    assert (r[3:] <= RTOL_BWD).all(), r


def test_rigid_motion_identity_antialiasing_clamped():
    """Antialiasing follows the original rasterizer's dL/dcov2D formula; the identity only needs the camera and
    the Gaussian gradients to use the SAME dL/dcov2D, which is what it checks."""
    inp = C.build(C.Case("aa_clamped_precomp", mode_color="precomp", antialiasing=True, xy_spread=1.6, **C._GENERAL))
    r = _identity_residuals(inp)
    print("aa+clamped:", " ".join(f"{x:.1e}" for x in r))
    assert (r <= RTOL_BWD).all(), r


# ---- 5. the ordinary gradients are unchanged ------------------------------------------------------------
@pytest.mark.record_path
@pytest.mark.parametrize("split", [False, True], ids=["combined", "dc"])
def test_ordinary_gradients_bit_equal(split):
    inp = _built("pose_general")
    gc, gd = C.unit_grads(inp["H"], inp["W"])
    if split:
        from tests.test_separate_sh import _accel_forward, _split

        dc_rest = _split(inp, DEV)
        fwd = _accel_forward(inp, *dc_rest, DEV)
    else:
        dc_rest, fwd = None, C.run_gpu_forward(inp, device=DEV)
    plain = _backward(inp, fwd, gc, gd, camera=False, dc_rest=dc_rest)
    with_cam = _backward(inp, fwd, gc, gd, camera=True, dc_rest=dc_rest)
    assert len(plain) == (9 if split else 8) and len(with_cam) == len(plain) + 3
    for a, b in zip(plain, with_cam):
        assert torch.equal(a, b)


def test_ordinary_gradients_default_path():
    inp = _built("pose_general")
    gc, gd = C.unit_grads(inp["H"], inp["W"])
    fwd = C.run_gpu_forward(inp, device=DEV)
    plain = _backward(inp, fwd, gc, gd, camera=False)
    fwd = C.run_gpu_forward(inp, device=DEV)
    with_cam = _backward(inp, fwd, gc, gd, camera=True)
    for k, a, b in zip(C.GRAD_NAMES, plain, with_cam):
        assert C.rel_err(b.cpu().numpy(), a.cpu().numpy()) <= RTOL_BWD, k


# ---- 6. shapes that break a reduction -------------------------------------------------------------------
def _slice(inp, n):
    return {k: (v[:n].contiguous() if k in PER_GAUSSIAN and v is not None else v) for k, v in inp.items()}


def test_single_gaussian_at_the_image_centre():
    case = C.pose_case("pose_general")
    R, center = C.case_pose(case)
    inp = _slice(_built("pose_general"), 1)
    inp["means3D"] = torch.from_numpy((center + R @ np.array([0.0, 0.0, 5.0])).astype(np.float32))[None]
    inp["scales"] = torch.tensor([[0.3, 0.2, 0.25]])
    inp["opacities"] = torch.tensor([[0.8]])
    gc, gd = C.unit_grads(inp["H"], inp["W"])
    ref = TRC.camera_grads(inp, gc, gd)
    assert ref["radii"][0] > 0
    got, _, _ = _gpu_camera_grads(inp)
    _assert_camera_close(got, ref, tag="P=1")


@pytest.mark.parametrize("n", [63, 64, 65])
def test_wave_boundaries(n):
    inp = _slice(_built("sh3_scalerot"), n)
    gc, gd = C.unit_grads(inp["H"], inp["W"])
    got, _, _ = _gpu_camera_grads(inp)
    _assert_camera_close(got, TRC.camera_grads(inp, gc, gd), tag=f"P={n}")


def test_many_workgroups_ragged_last_wave():
    inp = _built("lists_2k_4k")
    assert inp["means3D"].shape[0] == 5000
    got, _, _ = _gpu_camera_grads(inp)
    _assert_camera_close(got, _ref("lists_2k_4k", "unit"), tag="P=5000")


def _with_degenerates():
    """pose_general plus 64 Gaussians the forward culls: view-space z negative, z in (0, 0.2), mean == campos."""
    case = C.pose_case("pose_general")
    base = _built("pose_general")
    R, center = C.case_pose(case)
    g = torch.Generator().manual_seed(11)
    cam_pts = torch.zeros(64, 3)
    cam_pts[:, :2] = torch.empty(64, 2).uniform_(-1.0, 1.0, generator=g)
    cam_pts[:24, 2] = -torch.empty(24).uniform_(0.5, 6.0, generator=g)
    cam_pts[24:48, 2] = torch.empty(24).uniform_(0.01, 0.19, generator=g)
    cam_pts[24:48, :2] *= 0.05
    extra = C.to_world(cam_pts, R, center)
    extra[48:] = base["campos"]
    inp = dict(base)
    inp["means3D"] = torch.cat([base["means3D"], extra])
    for k in ("opacities", "shs", "scales", "rotations"):
        inp[k] = torch.cat([base[k], base[k][:64]])
    return inp


@pytest.mark.record_path
def test_culled_and_degenerate_gaussians():
    inp = _with_degenerates()
    got, _, radii = _gpu_camera_grads(inp)
    assert (radii[300:] == 0).all() and radii.numel() == 364
    base, _, _ = _gpu_camera_grads(_built("pose_general"))
    ref = _ref("pose_general", "unit")
    for k in CAM:
        assert np.isfinite(got[k]).all(), k
        assert np.abs(got[k] - base[k]).max() <= 1e-6 * np.abs(ref[k]).max(), k


@pytest.mark.record_path
def test_camera_gradients_are_deterministic():
    inp = _built("lists_2k_4k")
    gc, gd = C.unit_grads(inp["H"], inp["W"])
    fwd = C.run_gpu_forward(inp, device=DEV)
    a = _backward(inp, fwd, gc, gd, camera=True)[-3:]
    b = _backward(inp, fwd, gc, gd, camera=True)[-3:]
    c = _backward(inp, C.run_gpu_forward(inp, device=DEV), gc, gd, camera=True)[-3:]
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
        assert x.abs().max() > 0 or x.numel() == 3


@pytest.mark.record_path
@pytest.mark.parametrize("name", ["pose_general", "pose_general_sh1"])
def test_separate_sh_inputs_bitwise(name):
    inp = _built(name)
    comb, _, _ = _gpu_camera_grads(inp)
    sep, L, _ = _gpu_camera_grads(inp, split=True)
    assert L["dc"].grad is not None and L["rest"].grad is not None
    for k in CAM:
        np.testing.assert_array_equal(comb[k], sep[k])
    assert np.abs(comb["dL_dcampos"]).max() > 0


def test_poisoned_buffers_leave_no_nan(monkeypatch):
    monkeypatch.setenv("GSR_POISON", "1")
    got, _, radii = _gpu_camera_grads(_with_degenerates())
    assert (radii == 0).sum() >= 64
    for k in CAM:
        assert np.isfinite(got[k]).all(), k


# ---- 7. surface -----------------------------------------------------------------------------------------
def _hat4(xi):
    """se(3) generator [[omega]x, v; 0, 0] of the twist xi = (omega, v), differentiable."""
    z = torch.zeros((), dtype=xi.dtype)
    return torch.stack([torch.stack([z, -xi[2], xi[1], xi[3]]), torch.stack([xi[2], z, -xi[0], xi[4]]),
                        torch.stack([-xi[1], xi[0], z, xi[5]]), torch.stack([z, z, z, z])])


def _pose_from_twist(xi, V_true, Pt):
    """The camera tensors of the pose reached from ``V_true`` by moving the world by exp(xi): the stored view
    matrix exp(hat(xi))^T V_true, proj = view @ Pt, campos = inverse(view)[3, :3]."""
    view = torch.linalg.matrix_exp(_hat4(xi)).t() @ V_true
    return view, view @ Pt, view.inverse()[3, :3]


def _projection_part(inp, dtype=torch.float32):
    return (inp["viewmatrix"].double().inverse() @ inp["projmatrix"].double()).to(dtype)


def test_gradients_reach_the_leaves_of_the_camera_tensors():
    inp = _built("pose_general")
    xi0 = [0.02, -0.015, 0.01, 0.04, -0.03, 0.05]
    xi = torch.tensor(xi0, requires_grad=True)
    view, proj, campos = _pose_from_twist(xi, inp["viewmatrix"], _projection_part(inp))
    color, _, invd, _ = _render(inp, cam=(view.to(DEV), proj.to(DEV), campos.to(DEV)), gauss_grad=False)
    gc, gd = C.unit_grads(inp["H"], inp["W"])
    torch.autograd.backward([color, invd], [gc.to(DEV), gd.to(DEV)])
    # reference: its camera gradients at the same float32 camera tensors, chained through the same graph in float64
    ref = TRC.camera_grads(dict(inp, viewmatrix=view.detach(), projmatrix=proj.detach(), campos=campos.detach()), gc, gd)
    x64 = torch.tensor(xi0, dtype=torch.float64, requires_grad=True)
    cam64 = _pose_from_twist(x64, inp["viewmatrix"].double(), _projection_part(inp, torch.float64))
    torch.autograd.backward(list(cam64), [torch.from_numpy(np.array(ref[k])) for k in CAM])
    err = C.rel_err(xi.grad.numpy(), x64.grad.numpy())
    print(f"twist gradient rel err {err:.1e}")
    assert err <= RTOL_BWD


def test_transposed_viewmatrix_gets_its_own_layout():
    inp = _built("pose_general")
    vt = inp["viewmatrix"].t().contiguous().to(DEV).requires_grad_(True)  # the leaf holds the transpose
    proj = inp["projmatrix"].to(DEV)
    campos = inp["campos"].to(DEV)
    view = vt.t()
    assert not view.is_contiguous()
    color, _, invd, _ = _render(inp, cam=(view, proj, campos), gauss_grad=False)
    gc, gd = C.unit_grads(inp["H"], inp["W"])
    torch.autograd.backward([color, invd], [gc.to(DEV), gd.to(DEV)])
    ref = _ref("pose_general", "unit")["dL_dviewmatrix"]
    assert proj.grad is None and campos.grad is None
    assert C.rel_err(vt.grad.cpu().numpy(), ref.T) <= RTOL_BWD


def test_camera_only_render_backpropagates():
    inp = _built("pose_general")
    color, _, invd, L = _render(inp, gauss_grad=False)
    assert type(color.grad_fn).__name__.startswith("_RasterizeGaussiansCamera")
    gc, gd = C.unit_grads(inp["H"], inp["W"])
    torch.autograd.backward([color, invd], [gc.to(DEV), gd.to(DEV)])
    got = {"dL_dviewmatrix": L["viewmatrix"].grad, "dL_dprojmatrix": L["projmatrix"].grad, "dL_dcampos": L["campos"].grad}
    _assert_camera_close({k: v.cpu().numpy() for k, v in got.items()}, _ref("pose_general", "unit"), tag="camera only")
    assert L["means3D"].grad is None


def test_without_camera_grad_the_existing_path_is_used():
    from gaussian_splatting_amd import rasterizer

    inp = _built("pose_general")
    color, radii, invd, L = _render(inp, cam_grad=False)
    assert type(color.grad_fn).__name__ == "_RasterizeGaussiansBackward"
    fwd = C.run_gpu_forward(inp, device=DEV)
    assert torch.equal(color, fwd[1]) and torch.equal(radii, fwd[2]) and torch.equal(invd, fwd[6])
    gc, gd = C.unit_grads(inp["H"], inp["W"])
    torch.autograd.backward([color, invd], [gc.to(DEV), gd.to(DEV)])
    assert L["viewmatrix"].grad is None and L["means3D"].grad is not None
    with torch.no_grad():  # grad mode off: the existing path even when a camera tensor requires grad
        color2, _, _, _ = _render(inp)
    assert color2.grad_fn is None and torch.equal(color2, fwd[1])
    assert rasterizer._RasterizeGaussiansCamera is not rasterizer._RasterizeGaussians


def test_backward_arity_without_the_keyword():
    from tests.test_separate_sh import _accel_forward, _split

    inp = _built("pose_general")
    gc, gd = C.unit_grads(inp["H"], inp["W"])
    assert len(_backward(inp, C.run_gpu_forward(inp, device=DEV), gc, gd, camera=False)) == 8
    dc_rest = _split(inp, DEV)
    assert len(_backward(inp, _accel_forward(inp, *dc_rest, DEV), gc, gd, camera=False, dc_rest=dc_rest)) == 9


# ---- 8. pose refinement end to end ----------------------------------------------------------------------
def test_pose_refinement_converges():
    """40 Adam steps (lr 3e-3) on the twist of a pose started 1.5 degrees and 7 cm off, against the product's own
    render at the true pose, mean squared colour error.  On the float64 reference the loss falls from 1.37e-2 to
    2.5e-5 (/ 540) and max |V - V_true| from 4.3e-2 to 1.2e-2; asked here: loss / 20, pose error / 2."""
    inp = _built("pose_general")
    V_true, Pt = inp["viewmatrix"], _projection_part(inp)
    with torch.no_grad():
        target = _render(inp, cam_grad=False, gauss_grad=False)[0]
    xi = torch.tensor([0.02, -0.015, 0.01, 0.04, -0.03, 0.05], requires_grad=True)
    opt = torch.optim.Adam([xi], lr=3e-3)
    losses, pose_err = [], []
    for _ in range(41):
        view, proj, campos = _pose_from_twist(xi, V_true, Pt)
        color = _render(inp, cam=(view.to(DEV), proj.to(DEV), campos.to(DEV)), gauss_grad=False)[0]
        loss = ((color - target) ** 2).mean()
        losses.append(float(loss.detach()))
        pose_err.append(float((view.detach() - V_true).abs().max()))
        if len(losses) == 41:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    print(f"loss {losses[0]:.3e} -> {losses[-1]:.3e}, max|V - V_true| {pose_err[0]:.3e} -> {pose_err[-1]:.3e}")
    assert losses[-1] <= losses[0] / 20
    assert pose_err[-1] <= pose_err[0] / 2
