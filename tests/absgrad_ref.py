"""Reference for the absolute screen-space gradient (AbsGS; include/gsr.h gsr_backward_args.dL_dmean2D_abs), built on
the unchanged oracle.  TEST INFRASTRUCTURE ONLY (shared by tests/test_absgrad_ref.py and tests/test_gpu_absgrad.py).

    absgrad[g] = (sum_pix |t_x(g, pix)|, sum_pix |t_y(g, pix)|, 0)

with t_x, t_y the terms the reference adds per pixel into dL_dmean2D (CR/backward.cu:600-601).  The oracle's
backward only returns the sum over pixels, but it is linear in the upstream gradient: the backward of ONE forward
with every upstream map zeroed except at pixel p returns exactly pixel p's terms (the blend walk, the skips and
the termination belong to the forward and do not depend on the upstream values).  So the reference is one
backward per pixel, the absolute value of its ``dL_dmeans2D[:, :2]``, accumulated in float64.  With an alpha
gradient, pixel p's term is the total over all upstream maps: the second pass of tests/alpha_ref.py (zero
colours over the background (-1, 0, 0)), masked at the same pixel, is added before the absolute value.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import alpha_ref as AR
from tests import common as C


def per_pixel_terms(inp, g_c, g_d, g_a=None, precision="f32", nthreads=1, ref=None):
    """Generator over the image's pixels in row-major order: ``(y, x, t)`` with ``t`` [P,2] float64, pixel (x, y)'s
    terms of ``dL_dmeans2D[:, :2]`` for the loss ``sum(g_c color) + sum(g_d invdepth) [+ sum(g_a alpha)]``."""
    ref = C.run_oracle(inp, precision=precision, nthreads=nthreads) if ref is None else ref
    second = None
    if g_a is not None:
        second = C.run_oracle(AR.alpha_pass_inputs(inp), precision=precision, nthreads=nthreads)
    H, W = inp["H"], inp["W"]
    mc, md = torch.zeros_like(g_c), torch.zeros_like(g_d)
    ma = None if g_a is None else torch.zeros(3, H, W, dtype=g_c.dtype)
    for y in range(H):
        for x in range(W):
            mc[:, y, x] = g_c[:, y, x]
            md[:, y, x] = g_d[:, y, x]
            t = ref.handle.backward(mc, md, nthreads=nthreads)["dL_dmeans2D"][:, :2].astype(np.float64)
            if second is not None:
                ma[0, y, x] = g_a[0, y, x]
                t = t + second.handle.backward(ma, None, nthreads=nthreads)["dL_dmeans2D"][:, :2].astype(np.float64)
                ma[0, y, x] = 0
            mc[:, y, x] = 0
            md[:, y, x] = 0
            yield y, x, t


def oracle_absgrad(inp, g_c, g_d, g_a=None, precision="f32", nthreads=1, ref=None):
    """``(absgrad [P,3], signed [P,3])`` float64, read-only: the absolute screen-space gradient and, from the same
    per-pixel terms, their signed sum (what one backward call returns in ``dL_dmeans2D``)."""
    P = inp["means3D"].shape[0]
    ab, sg = np.zeros((P, 3)), np.zeros((P, 3))
    for _y, _x, t in per_pixel_terms(inp, g_c, g_d, g_a, precision, nthreads, ref):
        ab[:, :2] += np.abs(t)
        sg[:, :2] += t
    ab.setflags(write=False)
    sg.setflags(write=False)
    return ab, sg
