"""Rigid-motion equivariance of the float64 oracle (oracle/gsr_oracle.c).  CPU only.

A camera with pose (R, c) that renders a world-space scene must give what the identity camera with the same
fx, fy and principal point gives for the same scene expressed in the camera's frame:

    m_w = R m_c + c,    Sigma_w = R Sigma_c R^T,    colours and opacities unchanged

(precomputed colours and precomputed cov3D, so nothing but the camera chain is involved).  The property uses
no second implementation: it is the check that the oracle and tests/torch_ref.py, which agree with each other
under general poses (tests/test_oracle_autograd.py), do not share a convention error -- a transposed view
rotation, a view row read as a column, focal_x where focal_y belongs -- in the terms that the yaw cameras of
the other tests multiply by 0 or 1.

Bars: num_rendered, radii and n_contrib identical; colour and inverse depth within 1e-5 (the project's forward
bar); gradients within 2e-4 of max |ref| (the project's RTOL_BWD) after mapping dL/dmeans3D by R^T and
dL/dcov3D by the congruence G_c = R^T G_w R.  The residual comes from the float32 storage of the matrices, the
world-space means and cov3D.
"""
import numpy as np
import pytest
import torch

from tests import common as C

ATOL_FWD = 1e-5
RTOL_BWD = 2e-4
NAMES = ["pose_general", "pose_roll90", "pose_pitch", "pose_back", "pose_principal", "pose_clamped",
         "pose_general_aa"]
TRI = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def _full(c6):
    """[P,6] stored upper triangle -> [P,3,3] symmetric matrices."""
    S = np.zeros((c6.shape[0], 3, 3))
    for k, (i, j) in enumerate(TRI):
        S[:, i, j] = S[:, j, i] = c6[:, k]
    return S


def _tri(S):
    return np.stack([S[:, i, j] for i, j in TRI], 1)


def _grad_full(g6):
    """dL/d(stored entry) -> dL/d(matrix element) of the symmetric matrix: a stored off-diagonal entry stands
    for two elements, so each gets half."""
    G = _full(g6)
    off = ~np.eye(3, dtype=bool)
    G[:, off] *= 0.5
    return G


def _grad_tri(G):
    g6 = _tri(G)
    g6[:, [1, 2, 4]] *= 2.0
    return g6


def _pair(case):
    """(inputs under the case's camera in world space, inputs under the identity camera in the camera frame, R)."""
    R, center = C.case_pose(case)
    cam = C.case_camera(case)
    fy = case.focal_y if case.focal_y is not None else case.focal
    ident = C.make_pose_camera(case.W, case.H, case.focal, fy, 0.0, 0.0, 0.0, (0.0, 0.0, 0.0), case.principal)
    sc = C.camera_frame_scene(case, cam)
    cov_c = C.cov3d_reference(sc.scales, sc.rotations)
    cov_w = torch.from_numpy(_tri(R @ _full(cov_c.double().numpy()) @ R.T).astype(np.float32))
    g = torch.Generator().manual_seed(case.seed + 7)
    colors = torch.rand(case.P, 3, generator=g)

    def inputs(camera, means, cov):
        return dict(bg=torch.tensor(case.bg, dtype=torch.float32), means3D=means, opacities=sc.opacities, shs=None,
                    sh_degree=0, scales=None, rotations=None, colors_precomp=colors, cov3D_precomp=cov,
                    viewmatrix=camera.viewmatrix, projmatrix=camera.projmatrix, campos=camera.campos,
                    tanfovx=camera.tanfovx, tanfovy=camera.tanfovy, H=case.H, W=case.W, scale_modifier=1.0,
                    antialiasing=case.antialiasing)

    return inputs(cam, C.to_world(sc.means3D, R, center), cov_w), inputs(ident, sc.means3D, cov_c), R


@pytest.mark.parametrize("name", NAMES)
def test_pose_camera_equals_identity_camera_in_camera_frame(name):
    """Measured maxima (float64 oracle, float32 inputs), colour / inverse depth absolute, gradients relative to
    max |ref|:
        case              colour   invdepth  means2D  colors   opacity  means3D  cov3D
        pose_general      1.5e-06  3.5e-07   4.1e-06  4.6e-07  8.1e-07  2.5e-06  2.8e-06
        pose_roll90       2.6e-15  7.8e-16   4.7e-15  1.3e-15  9.6e-16  2.6e-15  3.3e-15
        pose_pitch        1.2e-06  4.7e-07   2.3e-06  6.4e-07  1.0e-06  2.4e-06  1.5e-06
        pose_back         1.1e-06  6.7e-07   2.0e-06  6.5e-07  6.1e-07  2.9e-06  8.6e-07
        pose_principal    9.9e-07  4.4e-07   2.4e-06  6.0e-07  1.0e-06  2.9e-06  9.1e-07
        pose_clamped      9.7e-07  2.7e-07   1.6e-06  5.2e-07  6.7e-07  7.9e-07  2.1e-06
        pose_general_aa   6.3e-07  3.0e-07   2.1e-06  4.2e-07  6.6e-07  2.2e-06  1.3e-06
    (pose_roll90's rotation is a signed permutation: exact in float32, so only float64 rounding is left.)
    """
    case = C.pose_case(name)
    inp_w, inp_c, R = _pair(case)
    a, b = C.run_oracle(inp_w, precision="f64"), C.run_oracle(inp_c, precision="f64")
    assert (b.radii > 0).sum() >= case.P // 3  # the scene fills the frame
    assert a.num_rendered == b.num_rendered
    np.testing.assert_array_equal(a.radii, b.radii)
    np.testing.assert_array_equal(a.handle.image()["n_contrib"], b.handle.image()["n_contrib"])
    errs = [float(np.abs(a.color - b.color).max()), float(np.abs(a.invdepth - b.invdepth).max())]
    gc, gd = C.unit_grads(case.H, case.W)
    ga = a.handle.backward(gc.double().numpy(), gd.double().numpy())
    gb = b.handle.backward(gc.double().numpy(), gd.double().numpy())
    mapped = dict(dL_dmeans2D=ga["dL_dmeans2D"], dL_dcolors=ga["dL_dcolors"], dL_dopacity=ga["dL_dopacity"],
                  dL_dmeans3D=ga["dL_dmeans3D"] @ R,  # rows g_w^T R = (R^T g_w)^T
                  dL_dcov3D=_grad_tri(R.T @ _grad_full(ga["dL_dcov3D"]) @ R))
    errs += [C.rel_err(mapped[k], gb[k]) for k in mapped]
    print(f"[{name}] " + " ".join(f"{e:.1e}" for e in errs))
    assert errs[0] <= ATOL_FWD and errs[1] <= ATOL_FWD, errs
    for k, e in zip(mapped, errs[2:]):
        assert np.abs(gb[k]).max() > 0, k
        assert e <= RTOL_BWD, (k, e)


def test_cases_are_general():
    """What the property is for: the compared cameras have a y row in the view rotation and the camera-frame
    scene is not the world-space one."""
    for name in NAMES:
        case = C.pose_case(name)
        inp_w, inp_c, R = _pair(case)
        assert np.abs(R - np.eye(3)).max() > 0.1
        assert float((inp_w["means3D"] - inp_c["means3D"]).abs().max()) > 0.5
        assert float((inp_w["cov3D_precomp"] - inp_c["cov3D_precomp"]).abs().max()) > 1e-3
