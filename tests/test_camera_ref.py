"""The float64 camera-gradient reference (tests/torch_ref_camera.py) checked on the CPU, before anything on
the GPU is held to it.

1. With the camera tensors as leaves it still gives torch_ref's eight ordinary gradients, and the entries the
   forward never reads (viewmatrix[:, 3], projmatrix[:, 2], campos with precomputed colours) are exact zeros.
2. The rigid-motion identity (torch_ref_camera.twist_sides), which uses no second implementation: the loss's
   derivative along a rigid motion of all Gaussians equals its derivative along the camera change that has the
   same effect.  With precomputed colours it holds for all six basis twists; with SH colours for the three
   translations only, a world rotation turning the view directions the camera change leaves alone -- and the
   test asserts that the rotational twists then differ, so it is seen to detect an error.

Residuals are relative to the largest magnitude among the six twists' values.  Measured (float64):
    precomputed colours + cov3D, six twists                               <= 1.1e-16
    scales/rotations, AA, xy_spread 1.6, scale_modifier 0.7, six twists   <= 6.7e-16
    pose_general (SH3): translations <= 7.6e-17, rotations 8.8e-4 .. 4.6e-3
Bars: 1e-12 where only float64 rounding is left; 1e-6 for the scales/rotations rotational twists (the Gaussian
side takes the covariance built from float32-normalised quaternions as it is, so nothing but rounding is left
there either, and the bar has room); > 1e-4 for the SH rotational twists.
"""
import numpy as np

from tests import common as C
from tests import torch_ref as TR
from tests import torch_ref_camera as TRC
from tests.test_pose_equivariance import _grad_full


def _residuals(inp, g):
    S = TRC.world_cov(inp)
    sides = np.array([TRC.twist_sides(tw, g, inp, _grad_full(g["dL_dcov3D"]), S) for tw in TRC.TWISTS])
    scale = np.abs(sides).max()
    assert scale > 0
    return np.abs(sides[:, 0] - sides[:, 1]) / scale


def _grads(case):
    inp = C.build(case)
    gc, gd = C.unit_grads(case.H, case.W)
    return inp, TRC.camera_grads(inp, gc, gd)


def test_ordinary_gradients_equal_torch_ref():
    case = C.pose_case("pose_general")
    inp, g = _grads(case)
    gc, gd = C.unit_grads(case.H, case.W)
    ref = TR.grads(TR.render(inp), gc, gd)
    for k in C.GRAD_NAMES:
        assert np.abs(ref[k]).max() > 0, k
        assert C.rel_err(g[k], ref[k]) <= 1e-12, k
    assert (g["dL_dviewmatrix"][:, 3] == 0).all() and (g["dL_dprojmatrix"][:, 2] == 0).all()
    for k, zero in (("dL_dviewmatrix", [3]), ("dL_dprojmatrix", [2])):
        rest = np.delete(g[k], zero, axis=1)
        assert (rest != 0).all(), k  # ... and every other entry is read
    assert (g["dL_dcampos"] != 0).all()
    _, gp = _grads(C.pose_case("pose_general_precomp"))
    assert (gp["dL_dcampos"] == 0).all()


def test_rigid_motion_identity_precomputed():
    """Precomputed colours and covariance: nothing but the camera chain, all six twists."""
    inp, g = _grads(C.Case("precomp_both", mode_color="precomp", mode_cov="precomp", **C._GENERAL))
    r = _residuals(inp, g)
    print("precomp:", " ".join(f"{x:.1e}" for x in r))
    assert (r <= 1e-12).all(), r


def test_rigid_motion_identity_scalerot_aa_clamped():
    """Scales / rotations, antialiasing, clamped view-space coordinates and scale_modifier != 1 (the reference
    differentiates its own antialiased forward, so the identity holds for it as it stands)."""
    case = C.Case("scalerot_aa", mode_color="precomp", antialiasing=True, xy_spread=1.6, scale_modifier=0.7,
                  **C._GENERAL)
    inp, g = _grads(case)
    pv = np.concatenate([inp["means3D"].double().numpy(), np.ones((case.P, 1))], 1) @ inp["viewmatrix"].double().numpy()
    vis = g["radii"] > 0
    assert (vis & (np.abs(pv[:, 0] / pv[:, 2]) > 1.3 * inp["tanfovx"])).any()
    assert (vis & (np.abs(pv[:, 1] / pv[:, 2]) > 1.3 * inp["tanfovy"])).any()
    r = _residuals(inp, g)
    print("scalerot+aa:", " ".join(f"{x:.1e}" for x in r))
    assert (r[3:] <= 1e-12).all(), r
    assert (r[:3] <= 1e-6).all(), r


def test_rigid_motion_identity_sh_translations_only():
    inp, g = _grads(C.pose_case("pose_general"))
    r = _residuals(inp, g)
    print("sh3:", " ".join(f"{x:.1e}" for x in r))
    assert (r[3:] <= 1e-12).all(), r
    assert (r[:3] > 1e-4).all(), r  # the view directions turn: the identity does not hold, and the test sees it
