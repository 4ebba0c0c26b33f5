"""Reference for N-channel feature rendering (include/gsr.h gsr_render_features / gsr_render_features_backward), built
on the unchanged oracle.  TEST INFRASTRUCTURE ONLY (shared by tests/test_features_ref.py and tests/test_gpu_features.py).

The blend is linear in the channels, so an N-channel render is ceil(C/3) oracle runs with ``colors_precomp =
F[:, 3k:3k+3]`` (the last chunk zero-padded) over ``bg = 0``: ``Fmap`` is the concatenated colour outputs, ``dL_dF``
the concatenated ``dL_dcolors`` for the upstream chunk ``U[3k:3k+3]`` (no inverse-depth gradient), and each geometry
gradient the SUM over the chunks of the oracle backward's -- the chain rule, exact by linearity.  The blend walk
(alphas, skips, termination) does not depend on the colours, so every chunk's walk is the scene's own.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import common as C

GEOM = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dscales", "dL_drotations")


def make_features(P, Cn, seed=21) -> torch.Tensor:
    """Seeded features [P,Cn] float32, normal with unit spread (both signs: a feature map is not a colour)."""
    return torch.randn(P, Cn, generator=torch.Generator().manual_seed(seed)).contiguous()


def make_upstream(Cn, H, W, seed=23) -> torch.Tensor:
    """Seeded upstream gradient of the feature map, [Cn,H,W] float32."""
    return torch.randn(Cn, H, W, generator=torch.Generator().manual_seed(seed)).contiguous()


def chunk_inputs(inp, F, k):
    """``inp`` rendering channels [3k, 3k+3) of ``F`` as precomputed colours (zero-padded) over a zero background."""
    P, Cn = F.shape
    col = torch.zeros(P, 3, dtype=torch.float32)
    n = min(3, Cn - 3 * k)
    col[:, :n] = F[:, 3 * k:3 * k + n]
    a = dict(inp)
    a["colors_precomp"] = col.contiguous()
    a["shs"] = None
    a["bg"] = torch.zeros(3, dtype=torch.float32)
    return a


def oracle_features(inp, F, U=None, precision="f32", nthreads=1) -> dict:
    """``Fmap`` [Cn,H,W] and ``n_contrib`` [H,W] of the oracle; with ``U`` also ``dL_dF`` [P,Cn] and the geometry
    gradients ``GEOM`` summed over the chunks.  Arrays in the oracle's precision, read-only."""
    P, Cn = F.shape
    H, W = inp["H"], inp["W"]
    fmap = np.zeros((Cn, H, W), np.float64 if precision == "f64" else np.float32)
    out = {}
    for k in range((Cn + 2) // 3):
        n = min(3, Cn - 3 * k)
        ref = C.run_oracle(chunk_inputs(inp, F, k), precision=precision, nthreads=nthreads)
        fmap[3 * k:3 * k + n] = ref.color[:n]
        out.setdefault("n_contrib", ref.handle.image()["n_contrib"].astype(np.int64))
        if U is None:
            continue
        g = torch.zeros(3, H, W, dtype=torch.float32)
        g[:n] = U[3 * k:3 * k + n]
        b = ref.handle.backward(g, None, nthreads=nthreads)
        if "dL_dF" not in out:
            out["dL_dF"] = np.zeros((P, Cn), b["dL_dcolors"].dtype)
            for name in GEOM:
                out[name] = np.zeros_like(b[name])
        out["dL_dF"][:, 3 * k:3 * k + n] = b["dL_dcolors"][:, :n]
        for name in GEOM:
            out[name] = out[name] + b[name]
    out["Fmap"] = fmap
    for v in out.values():
        v.setflags(write=False)
    return out
