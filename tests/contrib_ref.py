"""Reference for the per-Gaussian contribution statistics (include/gsr.h gsr_contrib_stats), built on the unchanged
oracle.  TEST INFRASTRUCTURE ONLY (shared by tests/test_contrib_ref.py and tests/test_gpu_contrib.py).

The blend weight w(g, pix) = alpha(g, pix) T(g, pix) is the factor of Gaussian g's colour in the pixel, so whatever
the colour source is

    dL_dcolors[g, c] = sum_pix w(g, pix) dL_dpix[c, pix]        (CR/backward.cu:553-569)

and column 0 of the oracle backward's ``dL_dcolors`` for ``dL_dpix = (m, 0, 0)`` is ``sum_pix w m``: ``weight_sum``
for m = 1, ``weighted_sum`` for a weight map.  For a one-hot ``dL_dpix`` the same column is the pixel's weights
themselves (one term, no rounding of a sum) -- one oracle backward per pixel, the method of tests/absgrad_ref.py --
and from those come ``weight_max``, ``pixel_count = #(w > 0)`` and, in float64, the two sums again.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import common as C

# the project's threshold margins (tests/test_gpu_fullsize.py): a pixel within these of a discrete decision of the
# reference's blend may legitimately take the other branch under another rounding
MARGIN_POWER, MARGIN_ALPHA, MARGIN_T = 1e-5, 1e-4, 1e-4


def weight_map(H, W, seed=11) -> torch.Tensor:
    """A seeded, strictly positive per-pixel weight map [H,W] float32 in [0.25, 1.75)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(H, W, generator=g) * 1.5 + 0.25).contiguous()


def one_call_sum(ref, H, W, m=None, nthreads=1) -> np.ndarray:
    """[P] float64: column 0 of the oracle backward's dL_dcolors for dL_dpix = (m or 1, 0, 0)."""
    g = torch.zeros(3, H, W)
    g[0] = 1.0 if m is None else m
    return ref.handle.backward(g, None, nthreads=nthreads)["dL_dcolors"][:, 0].astype(np.float64)


def per_pixel_weights(ref, H, W, nthreads=1) -> np.ndarray:
    """[H*W, P] float32, read-only: row y*W+x holds w(g, (x, y)) for every Gaussian (0 where g does not contribute)."""
    P = ref.radii.shape[0]
    w = np.zeros((H * W, P), np.float32)
    g = torch.zeros(3, H, W)
    for y in range(H):
        for x in range(W):
            g[0, y, x] = 1.0
            w[y * W + x] = ref.handle.backward(g, None, nthreads=nthreads)["dL_dcolors"][:, 0]
            g[0, y, x] = 0.0
    w.setflags(write=False)
    return w


def flagged_pixels(ref, nthreads=1) -> np.ndarray:
    """bool [H,W]: pixels whose blend comes within the project's margins of a discrete threshold of the reference."""
    m = ref.handle.pixel_margins(nthreads=nthreads)
    return (m["power"] < MARGIN_POWER) | (m["alpha"] < MARGIN_ALPHA) | (m["T"] < MARGIN_T)


def oracle_contrib(inp, m=None, nthreads=1, ref=None) -> dict:
    """The reference statistics of ``inp`` (float64 / int64 [P], read-only) with the per-pixel weights they come from:
    ``weight_sum``, ``weight_max``, ``pixel_count``, ``weighted_sum`` (zeros without ``m``), ``w`` [H*W, P],
    ``one_call_sum`` / ``one_call_weighted`` (the single-backward columns), ``flagged`` [H,W] and ``final_T`` [H,W]."""
    ref = C.run_oracle(inp, nthreads=nthreads) if ref is None else ref
    H, W = inp["H"], inp["W"]
    w = per_pixel_weights(ref, H, W, nthreads)
    w64 = w.astype(np.float64)
    out = dict(
        w=w,
        weight_sum=w64.sum(0),
        weight_max=w64.max(0) if w.shape[0] else np.zeros(w.shape[1]),
        pixel_count=(w > 0).sum(0).astype(np.int64),
        weighted_sum=(w64 * m.double().numpy().reshape(-1, 1)).sum(0) if m is not None else np.zeros(w.shape[1]),
        one_call_sum=one_call_sum(ref, H, W, None, nthreads),
        one_call_weighted=one_call_sum(ref, H, W, m, nthreads) if m is not None else None,
        flagged=flagged_pixels(ref, nthreads),
        final_T=ref.handle.image()["final_T"].astype(np.float64),
    )
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
