"""Reference for the depth-distortion map (include/gsr.h gsr_render_distortion / gsr_render_distortion_backward), built
on the unchanged oracle.  TEST INFRASTRUCTURE ONLY (shared by tests/test_distortion_ref.py and
tests/test_gpu_distortion.py).

From the per-pixel blend weights ``w[pix, g]`` of tests/contrib_ref.py (one one-hot oracle backward per pixel), in
float64 and in the SYMMETRIC form, which needs no list order:

    D(pix)      = sum_{i,j} w_i w_j |t_i - t_j|
    dL/dt_g     = sum_pix U(pix) 2 w_g sum_j w_j sign(t_g - t_j)
    G[pix, g]   = U(pix) dD/dw_g = U(pix) 2 sum_j w_j |t_g - t_j|

each evaluated by sorting on ``t`` with prefix sums (no P x P matrix).  The geometry gradients follow by linearity in
the colours: ``dL/dalpha_i = T_i G_i - sum_{h behind i} w_h G_h / (1 - alpha_i)`` is what the oracle's colour backward
forms for the colours ``G[pix, :]`` over a zero background and a one-hot upstream at ``pix``.  Three pixels share one
oracle run (one per colour channel); summing the oracle's ``GEOM`` gradients over the groups is the chain rule exactly.
``ordered_pass`` restates the kernels' single front-to-back pass in float64, for tests/test_distortion_ref.py to hold
against torch autograd.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import common as C
from tests import contrib_ref as CR

GEOM = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dscales", "dL_drotations")


def view_depth(inp) -> torch.Tensor:
    """``t`` of the GPU tests: view-space depth ``(means3D, 1) @ viewmatrix[:, 2]``, float32 [P]."""
    m = inp["means3D"]
    return (torch.cat([m, torch.ones(m.shape[0], 1)], 1) @ inp["viewmatrix"][:, 2]).contiguous()


def make_upstream(H, W, seed=29) -> torch.Tensor:
    """Seeded upstream gradient of the distortion map, [1,H,W] float32."""
    return torch.randn(1, H, W, generator=torch.Generator().manual_seed(seed)).contiguous()


def pixel_weights(ref, H, W, pixels, nthreads=1) -> np.ndarray:
    """Rows of contrib_ref.per_pixel_weights for the flat pixel indices ``pixels`` only: [len(pixels), P] float32."""
    w = np.zeros((len(pixels), ref.radii.shape[0]), np.float32)
    g = torch.zeros(3, H, W)
    for k, pix in enumerate(pixels):
        y, x = divmod(int(pix), W)
        g[0, y, x] = 1.0
        w[k] = ref.handle.backward(g, None, nthreads=nthreads)["dL_dcolors"][:, 0]
        g[0, y, x] = 0.0
    return w


def symmetric(w, t):
    """``(D [N], S [N,P], sgn [N,P])`` in float64 for weights ``w`` [N,P] and ``t`` [P]: ``S[n, g] = sum_j w_j |t_g -
    t_j|`` and ``sgn[n, g] = sum_j w_j sign(t_g - t_j)`` (ties count zero), ``D = sum_g w_g S_g``."""
    w = np.asarray(w, np.float64)
    t = np.asarray(t, np.float64)
    order = np.argsort(t, kind="stable")
    ws, ts = w[:, order], t[order]
    zero = np.zeros((w.shape[0], 1))
    cA = np.concatenate([zero, np.cumsum(ws, 1)], 1)       # cA[:, k] = sum of the first k sorted weights
    cB = np.concatenate([zero, np.cumsum(ws * ts, 1)], 1)
    lo, hi = np.searchsorted(ts, ts, "left"), np.searchsorted(ts, ts, "right")
    A_less, B_less = cA[:, lo], cB[:, lo]
    A_more, B_more = cA[:, -1:] - cA[:, hi], cB[:, -1:] - cB[:, hi]
    S = np.empty_like(w)
    sgn = np.empty_like(w)
    S[:, order] = ts * A_less - B_less + B_more - ts * A_more
    sgn[:, order] = A_less - A_more
    return (w * S).sum(1), S, sgn


def ordered_pass(w, t):
    """The kernels' single pass in float64 over ONE pixel's contributors in list order (``w``, ``t`` [n]): returns
    ``(D, g [n], dD_dt [n], dD_dalpha [n])`` by include/gsr.h's formulas, with ``alpha_i = w_i / T_i`` and ``T_{i+1} =
    T_i - w_i``."""
    w = np.asarray(w, np.float64)
    t = np.asarray(t, np.float64)
    A_prev = np.concatenate([[0.0], np.cumsum(w)[:-1]])
    B_prev = np.concatenate([[0.0], np.cumsum(w * t)[:-1]])
    A_n, B_n = w.sum(), (w * t).sum()
    D = 2.0 * (w * (t * A_prev - B_prev)).sum()
    g = 2.0 * (t * (2.0 * A_prev - A_n) + B_n - 2.0 * B_prev)
    dD_dt = 2.0 * w * (2.0 * A_prev + w - A_n)
    T = 1.0 - A_prev
    alpha = w / T
    suffix = 2.0 * D - np.cumsum(w * g)
    return D, g, dD_dt, T * g - suffix / (1.0 - alpha)


def geometry_grads(inp, G, pixels, nthreads=1) -> dict:
    """The oracle's ``GEOM`` gradients (float64) of the loss whose per-pixel colour-form is ``G`` [len(pixels), P]: one
    oracle forward and backward per group of three pixels, ``colors_precomp[:, c] = G[pix_c]`` over ``bg = 0`` with a
    one-hot upstream at ``(c, pix_c)``."""
    H, W = inp["H"], inp["W"]
    P = inp["means3D"].shape[0]
    out = None
    a = dict(inp)
    a["shs"] = None
    a["bg"] = torch.zeros(3, dtype=torch.float32)
    for k0 in range(0, len(pixels), 3):
        col = torch.zeros(P, 3, dtype=torch.float32)
        g = torch.zeros(3, H, W)
        for c, k in enumerate(range(k0, min(k0 + 3, len(pixels)))):
            col[:, c] = torch.from_numpy(np.asarray(G[k], np.float32))
            y, x = divmod(int(pixels[k]), W)
            g[c, y, x] = 1.0
        a["colors_precomp"] = col.contiguous()
        b = C.run_oracle(a, nthreads=nthreads).handle.backward(g, None, nthreads=nthreads)
        if out is None:
            out = {name: np.zeros(b[name].shape, np.float64) for name in GEOM}
        for name in GEOM:
            out[name] += b[name]
    if out is None:
        z = C.run_oracle(inp, nthreads=nthreads).handle.backward(torch.zeros(3, H, W), None)
        out = {name: np.zeros(z[name].shape, np.float64) for name in GEOM}
    return out


def oracle_distortion(inp, t, U=None, nthreads=1, ref=None, w=None) -> dict:
    """``D`` [H,W] (float64) and ``n_contrib`` [H,W] of the oracle's blend for ``t`` [P]; with ``U`` [1,H,W] also
    ``dL_dt`` [P] and the geometry gradients ``GEOM`` of ``sum(U * D)``.  ``ref`` / ``w``: the oracle forward of
    ``inp`` and its per-pixel weights, if the caller has them.  Arrays read-only."""
    ref = C.run_oracle(inp, nthreads=nthreads) if ref is None else ref
    H, W = inp["H"], inp["W"]
    w = CR.per_pixel_weights(ref, H, W, nthreads) if w is None else w
    t64 = t.double().numpy()
    D, S, sgn = symmetric(w, t64)
    out = dict(D=D.reshape(H, W), n_contrib=ref.handle.image()["n_contrib"].astype(np.int64), w=w)
    if U is not None:
        u = U.double().numpy().reshape(-1, 1)
        w64 = np.asarray(w, np.float64)
        out["dL_dt"] = (u * 2.0 * w64 * sgn).sum(0)
        pixels = np.flatnonzero((w64 > 0).any(1) & (u[:, 0] != 0))  # (no contributor or no upstream: no gradient)
        out.update(geometry_grads(inp, (u * 2.0 * S)[pixels], pixels, nthreads))
    for v in out.values():
        v.setflags(write=False)
    return out
