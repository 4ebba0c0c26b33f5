"""The yardstick of the accumulated-alpha output, on the oracle alone (no GPU): tests/alpha_ref.py builds the
alpha map and the gradient of an alpha loss from the unchanged oracle by rendering the scene a second time with
zero colours over the background (-1, 0, 0).  Here that construction is held against an independent one -- unit
colours over a zero background, whose colour channel 0 is sum_i alpha_i T_i = 1 - final_T -- and the C ABI of the
feature is checked in the header and, where the library is built, in its symbol table.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import alpha_ref as AR
from tests import common as C

NAMES = ["sh3_scalerot", "background", "pose_general"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(name):
    return next(c for c in C.SMALL_CASES + C.POSE_CASES if c.name == name)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("precision,atol", [("f64", 1e-12), ("f32", 1e-6)])
def test_alpha_is_unit_colour_channel(name, precision, atol):
    """(a) 1 - final_T == colour channel 0 of a render with unit colours and zero background."""
    inp = C.build(_case(name))
    alpha = AR.oracle_alpha(C.run_oracle(inp, precision=precision))
    unit = C.run_oracle(AR.alpha_pass_inputs(inp, colour=1.0, bg=(0.0, 0.0, 0.0)), precision=precision)
    assert alpha.min() >= 0 and alpha.max() <= 1 and alpha.max() > 0.5
    err = float(np.abs(alpha - unit.color[0]).max())
    print(f"[{name}/{precision}] max |(1 - final_T) - unit colour| = {err:.2e}")
    assert err <= atol
    # ... and the zero-colour / bg = -1 pass renders alpha - 1 in channel 0, nothing in the others
    sub = C.run_oracle(AR.alpha_pass_inputs(inp), precision=precision)
    np.testing.assert_array_equal(sub.color[0], -C.run_oracle(inp, precision=precision).handle.image()["final_T"])
    assert not sub.color[1:].any()


@pytest.mark.parametrize("name", NAMES)
def test_alpha_gradient_constructions_agree(name):
    """(b) float64: the gradients of sum(g_a * alpha) from the zero-colour / bg = -1 pass equal those from the
    unit-colour / bg = 0 pass, to 1e-9 of max |ref| per tensor."""
    inp = C.build(_case(name))
    g_pix = AR.alpha_pix_grad(AR.alpha_grad(inp["H"], inp["W"]))
    sub = C.run_oracle(AR.alpha_pass_inputs(inp), precision="f64").handle.backward(g_pix, None)
    unit = C.run_oracle(AR.alpha_pass_inputs(inp, colour=1.0, bg=(0.0, 0.0, 0.0)), precision="f64").handle.backward(
        g_pix, None)
    for k in AR.SUMMED:
        assert np.abs(unit[k]).max() > 0, k
        err = C.rel_err(sub[k], unit[k])
        print(f"[{name}] {k}: {err:.2e}")
        assert err <= 1e-9, (k, err)


def test_abi_declares_and_exports_the_alpha_entry_points():
    """(c) include/gsr.h declares gsr_render_alpha, and the alpha gradient as the field dL_dalphas of
    gsr_rasterize_backward's argument struct (mirrored by _lib.BackwardArgs; tests/test_abi_layout.py holds the
    two layouts together); a built library exports both functions."""
    import re

    from gaussian_splatting_amd import _lib

    new = {"gsr_render_alpha", "gsr_rasterize_backward"}
    assert new <= set(_lib.header_symbols(_lib.HEADER_PATH))
    assert new <= set(_lib.SIGNATURES)
    text = open(_lib.HEADER_PATH).read()
    assert "int gsr_render_alpha(int width, int height, const void* image_buffer, float* out_alpha, void* stream);" in text
    struct = re.search(r"typedef struct gsr_backward_args \{(.*?)\} gsr_backward_args;", text, flags=re.S).group(1)
    assert re.search(r"^\s*const float\* dL_dalphas;", struct, flags=re.M)
    assert "int gsr_rasterize_backward(const gsr_backward_args* args);" in text
    assert "dL_dalphas" in dict(_lib.BackwardArgs._fields_)
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert new <= exported
