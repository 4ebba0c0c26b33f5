"""References for the accumulated-alpha output ``A = 1 - final_T``, built on the unchanged oracle.
TEST INFRASTRUCTURE ONLY (shared by tests/test_alpha_ref.py and tests/test_gpu_alpha.py).

The oracle's backward has no alpha input, but the background term of its colour has the form needed:
dC/dalpha_i contains -T_final / (1 - alpha_i) . bg, and dA/dalpha_i = +T_final / (1 - alpha_i).  So a second
pass over the same scene with every colour zero (``colors_precomp = 0``, no ``shs``) and ``bg = (-1, 0, 0)``
renders colour channel 0 = -T_final = A - 1 -- the blend walk is the first pass's, colours never steer it --
and its backward with ``dL_dpix = (g_a, 0, 0)`` is the gradient of ``sum(g_a * A)``.  The gradient of a joint
loss is the first pass's backward with ``(g_c, g_d)`` plus the second pass's, over the tensors in ``SUMMED``;
``dL_dcolors`` and ``dL_dsh`` come from the first pass alone (A does not depend on the colours).
tests/test_alpha_ref.py pins the construction against an independent one (unit colours, zero background).
"""
from __future__ import annotations

import numpy as np
import torch

from tests import common as C

SUMMED = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")
FIRST_PASS_ONLY = ("dL_dcolors", "dL_dsh")


def alpha_pass_inputs(inp, colour=0.0, bg=(-1.0, 0.0, 0.0)):
    """``inp`` with every Gaussian's colour the constant ``colour`` (precomputed, no SH) over background ``bg``."""
    a = dict(inp)
    a["colors_precomp"] = torch.full((inp["means3D"].shape[0], 3), float(colour), dtype=torch.float32)
    a["shs"] = None
    a["bg"] = torch.tensor(bg, dtype=torch.float32)
    return a


def alpha_pix_grad(g_a):
    """``g_a`` [1,H,W] as the upstream gradient of colour channel 0: [3,H,W] with zeros elsewhere."""
    return torch.cat([g_a, torch.zeros(2, *g_a.shape[1:], dtype=g_a.dtype)], 0)


def alpha_grad(H, W, seed=11):
    """The seeded upstream gradient of the alpha map, [1,H,W]."""
    return torch.randn(1, H, W, generator=torch.Generator().manual_seed(seed))


def oracle_alpha(ref):
    """``1 - final_T`` [H,W] of an oracle forward, in the oracle's precision."""
    return 1 - ref.handle.image()["final_T"]


def oracle_joint_grads(inp, g_c, g_d, g_a, precision="f32", ref=None):
    """The oracle's gradients of ``sum(g_c * color) + sum(g_d * invdepth) + sum(g_a * A)`` by the two-pass
    construction above (``ref``: the first pass's forward, if the caller has it already)."""
    ref = C.run_oracle(inp, precision=precision) if ref is None else ref
    first = ref.handle.backward(g_c, g_d)
    second = C.run_oracle(alpha_pass_inputs(inp), precision=precision).handle.backward(alpha_pix_grad(g_a), None)
    out = {k: first[k] + second[k] for k in SUMMED}
    out.update({k: first[k] for k in FIRST_PASS_ONLY})
    for v in out.values():
        v.setflags(write=False)
    return out


def camera_alpha_grads(inp, g_a):
    """dL/dviewmatrix, dL/dprojmatrix, dL/dcampos of ``sum(g_a * A)`` from the float64 camera reference
    (tests/torch_ref_camera.py) by the same substitution."""
    from tests import torch_ref_camera as TRC

    g = TRC.camera_grads(alpha_pass_inputs(inp), alpha_pix_grad(g_a), None)
    return {k: np.asarray(g[k]) for k in TRC.CAMERA_NAMES}
