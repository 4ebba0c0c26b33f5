"""tests/torch_ref.py with the camera as a differentiable input.  TEST INFRASTRUCTURE ONLY.

``torch_ref.render`` detaches ``viewmatrix``, ``projmatrix`` and ``campos``; here the same float64 forward runs
with the three as autograd leaves, so ``loss.backward()`` gives dL/dviewmatrix [4,4], dL/dprojmatrix [4,4] and
dL/dcampos [3] beside the eight ordinary gradients.  The per-Gaussian math (``_preprocess``, ``_rect``,
``eval_sh``, ``cov3d_from_scale_rot``) is torch_ref's own, imported; only the forward's body is restated, because
that is where the detach sits.  The three tensors are independent inputs, exactly as the forward reads them:

  viewmatrix  the view-space point t (cov2D's Jacobian, the inverse depth) and the rotation W of T = W J
  projmatrix  the screen position
  campos      the SH view direction

and the conventions are torch_ref's (no gradient through culling / radius / tile rectangle / skip / termination,
a clamped t.x, t.y a constant in J, the 0.99 clamp straight-through).  Entries the forward never reads --
viewmatrix[:, 3], projmatrix[:, 2], all of campos with precomputed colours -- get exact zeros.
Antialiasing: autograd differentiates the forward's h, which the reference's hand backward does not
(torch_ref's docstring), so dL/dviewmatrix under antialiasing is not the product's convention; dL/dprojmatrix
and dL/dcampos do not pass through that chain.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import torch_ref as TR
from tests.torch_ref import BLOCK, F64, _leaf, _preprocess, _rect

CAMERA_NAMES = ["dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"]


def render(inp, antialiasing=None):
    """torch_ref.render with ``res["cam"]`` = the (viewmatrix, projmatrix, campos) float64 leaves."""
    aa = inp["antialiasing"] if antialiasing is None else antialiasing
    W, H = inp["W"], inp["H"]
    P = inp["means3D"].shape[0]
    V, Pm, campos = _leaf(inp["viewmatrix"]), _leaf(inp["projmatrix"]), _leaf(inp["campos"])
    bg = inp["bg"].detach().to(F64)
    L = {k: _leaf(inp.get(k)) for k in ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations",
                                        "cov3D_precomp")}
    L["means2D"] = torch.zeros(P, 3, dtype=F64, requires_grad=True)
    gx, gy = (W + BLOCK - 1) // BLOCK, (H + BLOCK - 1) // BLOCK
    mod = float(inp["scale_modifier"])
    tanfovx, tanfovy = float(inp["tanfovx"]), float(inp["tanfovy"])

    with torch.no_grad():  # pass 1: which Gaussians survive preprocess
        ph = torch.cat([L["means3D"], torch.ones(P, 1, dtype=F64)], 1)
        idx = torch.arange(P)[(ph @ V[:, :3])[:, 2] > 0.2]
        pre = _preprocess(L, V, Pm, campos, tanfovx, tanfovy, W, H, inp["sh_degree"], mod, aa, idx)
        ok = pre["det"] != 0
        xmin, ymin, xmax, ymax = _rect(pre["xy"], pre["radius"], gx, gy)
        ok &= (xmax - xmin) * (ymax - ymin) != 0
        idx = idx[ok]
    pre = _preprocess(L, V, Pm, campos, tanfovx, tanfovy, W, H, inp["sh_degree"], mod, aa, idx)
    if L["colors_precomp"] is None:
        pre["rgb"].retain_grad()
    if L["cov3D_precomp"] is None:
        pre["cov3D"].retain_grad()
    depth = pre["p_view"][:, 2]
    radii = torch.zeros(P, dtype=torch.int64)
    radii[idx] = pre["radius"].to(torch.int64)
    xmin, ymin, xmax, ymax = _rect(pre["xy"].detach(), pre["radius"], gx, gy)

    order = torch.sort(depth.detach(), stable=True).indices
    xy, conic, opac, rgb = pre["xy"][order], pre["conic"][order], pre["opac"][order], pre["rgb"][order]
    invd = 1.0 / depth[order]
    xmin, ymin, xmax, ymax = xmin[order], ymin[order], xmax[order], ymax[order]

    py, px = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    px, py = px.reshape(-1), py.reshape(-1)
    tx, ty = px // BLOCK, py // BLOCK
    member = ((tx[:, None] >= xmin[None]) & (tx[:, None] < xmax[None]) & (ty[:, None] >= ymin[None]) &
              (ty[:, None] < ymax[None]))
    dx = xy[None, :, 0] - px[:, None].to(F64)
    dy = xy[None, :, 1] - py[:, None].to(F64)
    power = -0.5 * (conic[None, :, 0] * dx * dx + conic[None, :, 2] * dy * dy) - conic[None, :, 1] * dx * dy
    raw = opac[None] * torch.exp(power)
    val = torch.clamp_max(raw, 0.99)
    a_st = raw + (val - raw).detach()
    with torch.no_grad():
        use = member & (power <= 0) & (val >= 1.0 / 255.0)
        a_d = torch.where(use, val, torch.zeros_like(val))
        Tin = torch.cumprod(torch.cat([torch.ones_like(a_d[:, :1]), 1.0 - a_d[:, :-1]], 1), 1)
        term = use & (Tin * (1.0 - a_d) < 0.0001)
        keep = use & (torch.cumsum(term.to(torch.int64), 1) == 0)
    a = torch.where(keep, a_st, torch.zeros_like(a_st))
    T_incl = torch.cumprod(1.0 - a, 1)
    T_excl = torch.cat([torch.ones_like(a[:, :1]), T_incl[:, :-1]], 1)
    w = a * T_excl
    final_T = T_incl[:, -1] if a.shape[1] else torch.ones(H * W, dtype=F64)
    out = w @ rgb + final_T[:, None] * bg[None]
    return dict(color=out.t().reshape(3, H, W), invdepth=(w @ invd).reshape(1, H, W), radii=radii, leaves=L,
                pre=pre, idx=idx, mod=mod, cam=(V, Pm, campos))


def grads(res, dL_dcolor, dL_dinvdepth=None):
    """torch_ref.grads' eight gradients plus dL_dviewmatrix [4,4], dL_dprojmatrix [4,4], dL_dcampos [3]
    (float64 numpy; a tensor the loss does not depend on gets zeros)."""
    out = TR.grads(res, dL_dcolor, dL_dinvdepth)
    for name, t in zip(CAMERA_NAMES, res["cam"]):
        out[name] = (torch.zeros_like(t) if t.grad is None else t.grad).detach().numpy()
    return out


def camera_grads(inp, dL_dcolor, dL_dinvdepth=None):
    """Forward + backward in one call: the dict of ``grads`` and the forward's radii."""
    res = render(inp)
    g = grads(res, dL_dcolor, dL_dinvdepth)
    g["radii"] = res["radii"].numpy()
    return g


# ---- rigid-motion identity -------------------------------------------------------------------------------
# Move every Gaussian by the rigid motion exp(eps G), G = [[omega]x, v; 0, 0]: m -> m + eps (omega x m + v),
# Sigma -> Sigma + eps ([omega]x Sigma + Sigma [omega]x^T).  The forward reads the means only through the rows
# (m, 1) @ Vt, (m, 1) @ Pt (Vt, Pt: the matrices as stored) and m - c, so the same change of every quantity the
# forward forms comes from leaving the Gaussians alone and changing the camera tensors by
#   dVt = eps G^T Vt,   dPt = eps G^T Pt,   dc = -eps (omega x c + v)
# except that m - c is then not turned by omega: with SH colours the two sides agree for translations only.
TWISTS = np.eye(6)  # (omega, v): three rotations, three translations


def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def twist_sides(twist, g, inp, G_full, S_full):
    """(camera side, Gaussian side) of the identity for ``twist`` = (omega, v), both dL/d(eps).
    ``g``: gradients by name (dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, dL_dmeans3D); ``G_full`` [P,3,3]:
    dL/d(matrix element) of the world-space covariance ``S_full`` [P,3,3].  Summed in float64."""
    om, v = np.asarray(twist[:3], np.float64), np.asarray(twist[3:], np.float64)
    G = np.zeros((4, 4))
    G[:3, :3], G[:3, 3] = _hat(om), v
    Vt = inp["viewmatrix"].detach().double().cpu().numpy()
    Pt = inp["projmatrix"].detach().double().cpu().numpy()
    c = inp["campos"].detach().double().cpu().numpy()
    cam = ((np.asarray(g["dL_dviewmatrix"], np.float64).reshape(4, 4) * (G.T @ Vt)).sum()
           + (np.asarray(g["dL_dprojmatrix"], np.float64).reshape(4, 4) * (G.T @ Pt)).sum()
           + np.asarray(g["dL_dcampos"], np.float64).reshape(3) @ (-np.cross(om, c) - v))
    m = inp["means3D"].detach().double().cpu().numpy()
    gauss = (np.asarray(g["dL_dmeans3D"], np.float64) * (np.cross(om, m) + v)).sum()
    gauss += (np.asarray(G_full, np.float64) * (_hat(om) @ S_full + S_full @ _hat(om).T)).sum()
    return float(cam), float(gauss)


def world_cov(inp):
    """The world-space covariances the forward uses, [P,3,3] float64 (scale_modifier applied)."""
    if inp.get("cov3D_precomp") is not None:
        c6 = inp["cov3D_precomp"].detach().double().cpu()
    else:
        c6 = TR.cov3d_from_scale_rot(inp["scales"].detach().double().cpu(), float(inp["scale_modifier"]),
                                     inp["rotations"].detach().double().cpu())
    c6 = c6.numpy()
    S = np.zeros((c6.shape[0], 3, 3))
    for k, (i, j) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        S[:, i, j] = S[:, j, i] = c6[:, k]
    return S
