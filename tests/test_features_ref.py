"""CPU checks of the feature-rendering reference (tests/features_ref.py) that tests/test_gpu_features.py holds the
kernels to, of the new C ABI symbols and of the Python argument checks of ``features=``.

The chunked-oracle helper is pinned on ``ragged_37x23`` against an independent path: the per-pixel blend weights of
tests/contrib_ref.py (one oracle backward per pixel), from which ``Fmap = w F`` and ``dL_dF = w^T U`` follow in
float64.  Bar: 1e-6 of max |ref| (float32 references, sums of at most a few dozen terms).
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import common as C
from tests import contrib_ref as CR
from tests import features_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _ragged():
    case = next(c for c in C.SMALL_CASES if c.name == "ragged_37x23")
    inp = C.build(case)
    ref = C.run_oracle(inp)
    return inp, CR.per_pixel_weights(ref, inp["H"], inp["W"])


@pytest.mark.parametrize("Cn", [1, 7])
def test_chunked_oracle_equals_weight_blend(Cn):
    inp, w = _ragged()
    H, W, P = inp["H"], inp["W"], inp["means3D"].shape[0]
    F, U = FR.make_features(P, Cn), FR.make_upstream(Cn, H, W)
    got = FR.oracle_features(inp, F, U)
    w64 = w.astype(np.float64)  # [H*W, P]
    fmap = (w64 @ F.double().numpy()).T.reshape(Cn, H, W)
    dF = w64.T @ U.double().numpy().reshape(Cn, H * W).T
    assert np.abs(fmap).max() > 0 and np.abs(dF).max() > 0
    e_map = np.abs(got["Fmap"] - fmap).max() / np.abs(fmap).max()
    e_dF = np.abs(got["dL_dF"] - dF).max() / np.abs(dF).max()
    print(f"[C={Cn}] Fmap {e_map:.2e} dL_dF {e_dF:.2e}")
    assert e_map <= 1e-6 and e_dF <= 1e-6
    # a feature loss moves the geometry: the summed chunk gradients are not all zero
    for name in FR.GEOM:
        assert got[name].shape[0] == P and np.abs(got[name]).max() > 0, name


def test_symbols_are_declared_and_bound():
    from gaussian_splatting_amd import _lib

    names = _lib.header_symbols(os.path.join(ROOT, "include", "gsr.h"))
    for sym in ("gsr_render_features", "gsr_render_features_backward", "gsr_render_features_chunk"):
        assert sym in names, sym
        assert sym in _lib.SIGNATURES, sym
    assert len(_lib.SIGNATURES["gsr_render_features"][1]) == 13
    assert len(_lib.SIGNATURES["gsr_render_features_backward"][1]) == 25


def _call(features, **over):
    """rasterize_gaussians(features=...) on host tensors: every check below must raise before any device work."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, rasterize_gaussians

    P = 5
    z = torch.zeros
    s = GaussianRasterizationSettings(8, 8, 1.0, 1.0, z(3), 1.0, torch.eye(4), torch.eye(4), 0, z(3), False, False, False)
    a = dict(means3D=z(P, 3), means2D=z(P, 3), sh=torch.Tensor([]), colors=z(P, 3), opac=z(P, 1), scales=z(P, 3),
             rot=z(P, 4), cov=torch.Tensor([]))
    a.update(over)
    return rasterize_gaussians(a["means3D"], a["means2D"], a["sh"], a["colors"], a["opac"], a["scales"], a["rot"],
                               a["cov"], s, features=features)


def test_feature_argument_checks_raise():
    from gaussian_splatting_amd import _C

    with pytest.raises(RuntimeError, match=r"\(num_points, C\)"):
        _call(torch.zeros(5))
    with pytest.raises(RuntimeError, match=r"\(num_points, C\)"):
        _call(torch.zeros(4, 3))  # another point count
    with pytest.raises(RuntimeError, match="C >= 1"):
        _call(torch.zeros(5, 0))
    with pytest.raises(RuntimeError, match="float32"):
        _call(torch.zeros(5, 3, dtype=torch.float64))
    with pytest.raises(TypeError, match="tensor"):
        _call([[0.0] * 3] * 5)
    with pytest.raises(RuntimeError, match="HIP device"):
        _call(torch.zeros(5, 3))  # a host tensor: there is no CPU path
    # contiguity is checked on device tensors (after the device check); the shared check itself, on a meta tensor
    with pytest.raises(RuntimeError, match="contiguous"):
        _check_noncontiguous()
    # cov3D_precomp with a geometry input that requires grad is refused; without one the call goes on (to the
    # device check here)
    cov = dict(scales=torch.Tensor([]), rot=torch.Tensor([]), cov=torch.zeros(5, 6))
    with pytest.raises(RuntimeError, match="cov3D_precomp"):
        _call(torch.zeros(5, 3), means3D=torch.zeros(5, 3, requires_grad=True), **cov)
    with pytest.raises(RuntimeError, match="HIP device"):
        _call(torch.zeros(5, 3, requires_grad=True), **cov)
    assert _C.feature_chunk.__doc__


def _check_noncontiguous():
    """check_features' last test, reached with the device test stubbed out (no HIP device on the CPU runner)."""
    from gaussian_splatting_amd import _C

    keep = _C._require_device
    _C._require_device = lambda t, name: None
    try:
        _C.check_features(torch.zeros(3, 5).t(), 5)
    finally:
        _C._require_device = keep
