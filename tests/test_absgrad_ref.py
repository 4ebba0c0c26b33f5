"""The yardstick of the absolute screen-space gradient, on the oracle alone (no GPU): tests/absgrad_ref.py sums
|per-pixel term| over one oracle backward per pixel.  Here the construction is pinned -- its signed sum is the
one-call backward, the absolute sum dominates it, a single-pixel loss has abs == |grad|, column 2 is zero -- and
the C ABI and the Python surface of the feature are checked where no device is needed.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import absgrad_ref as ABR
from tests import alpha_ref as AR
from tests import common as C


def _case(name):
    return next(c for c in C.SMALL_CASES + C.POSE_CASES if c.name == name)


@pytest.mark.parametrize("loss", ["colour_depth", "joint"])
def test_reference_is_consistent_with_the_one_call_backward(loss):
    """ragged_37x23, f32 oracle: signed per-pixel sum == one backward within 1e-5 of max |ref|;
    abs >= |signed| - 1e-5 max; column 2 zero; and the effect is not a rounding-level one."""
    inp = C.build(_case("ragged_37x23"))
    g_c, g_d = C.unit_grads(inp["H"], inp["W"])
    g_a = AR.alpha_grad(inp["H"], inp["W"]) if loss == "joint" else None
    ref = C.run_oracle(inp)
    ab, sg = ABR.oracle_absgrad(inp, g_c, g_d, g_a, ref=ref)
    one = (AR.oracle_joint_grads(inp, g_c, g_d, g_a, ref=ref) if g_a is not None else
           ref.handle.backward(g_c, g_d))["dL_dmeans2D"].astype(np.float64)
    mx = np.abs(one).max()
    err = np.abs(sg - one).max() / mx
    big = ab[:, :2].sum(1) > 1.5 * np.abs(sg[:, :2]).sum(1)
    nz = ab[:, :2].sum(1) > 0
    print(f"[ragged_37x23/{loss}] signed sum vs one call {err:.2e} of max; max abs / max |grad| = "
          f"{ab.max() / mx:.2f}; rows with abs > 1.5 |signed|: {int(big.sum())} of {int(nz.sum())} non-zero")
    assert mx > 0 and err <= 1e-5
    assert (ab[:, :2] >= np.abs(sg[:, :2]) - 1e-5 * mx).all()
    assert not ab[:, 2].any() and not sg[:, 2].any()
    assert (ab[ref.radii == 0] == 0).all()
    assert big.sum() >= 0.5 * nz.sum()  # cancellation across a Gaussian's centre is the rule, not the exception


def test_single_pixel_upstream_has_abs_equal_grad():
    inp = C.build(_case("ragged_37x23"))
    H, W = inp["H"], inp["W"]
    g_c, g_d = C.unit_grads(H, W)
    keep = torch.zeros(1, H, W)
    keep[0, 11, 17] = 1
    g_c, g_d = g_c * keep, g_d * keep
    ref = C.run_oracle(inp)
    ab, _ = ABR.oracle_absgrad(inp, g_c, g_d, ref=ref)
    one = ref.handle.backward(g_c, g_d)["dL_dmeans2D"].astype(np.float64)
    assert np.abs(one).max() > 0
    np.testing.assert_array_equal(ab, np.abs(one))


def test_abi_declares_and_exports_the_absgrad_entry_point():
    """include/gsr.h declares the absolute gradient as the output field dL_dmean2D_abs of gsr_rasterize_backward's
    argument struct, _lib.BackwardArgs mirrors it (tests/test_abi_layout.py compares every field's offset and size
    with the C compiler's), and a built library exports the function."""
    import re

    from gaussian_splatting_amd import _lib

    new = {"gsr_rasterize_backward"}
    assert new <= set(_lib.header_symbols(_lib.HEADER_PATH))
    assert new <= set(_lib.SIGNATURES)
    text = open(_lib.HEADER_PATH).read()
    struct = re.search(r"typedef struct gsr_backward_args \{(.*?)\} gsr_backward_args;", text, flags=re.S).group(1)
    assert re.search(r"^\s*float\* dL_dmean2D_abs;", struct, flags=re.M)
    assert "int gsr_rasterize_backward(const gsr_backward_args* args);" in text
    assert "dL_dmean2D_abs" in dict(_lib.BackwardArgs._fields_)
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert new <= exported


def test_python_surface_takes_the_keyword():
    """The keyword exists on every layer, the shim forwards it, and the densification helper refuses a tensor
    without the attribute before it touches the device."""
    import inspect

    import diff_gaussian_rasterization as shim
    from gaussian_splatting_amd import _C, densify, rasterizer

    assert inspect.signature(_C.rasterize_gaussians_backward).parameters["absgrad"].default is False
    assert inspect.signature(rasterizer.rasterize_gaussians).parameters["absgrad"].default is False
    assert inspect.signature(rasterizer.GaussianRasterizer.forward).parameters["absgrad"].default is False
    assert inspect.signature(densify.add_densification_stats).parameters["absgrad"].default is False
    assert shim.rasterize_gaussians is rasterizer.rasterize_gaussians
    assert shim.GaussianRasterizer is rasterizer.GaussianRasterizer

    class Model:
        xyz_gradient_accum = torch.zeros(4, 1)
        denom = torch.zeros(4, 1)

    with pytest.raises(RuntimeError, match="absgrad"):
        densify.add_densification_stats(Model(), torch.zeros(4, 3), torch.ones(4, dtype=torch.bool), absgrad=True)
