"""CPU checks of the depth-distortion reference (tests/distortion_ref.py) that tests/test_gpu_distortion.py holds the
kernels to, of the new C ABI symbols and of the Python argument checks of ``distortion=``.

On ``ragged_37x23``, from the per-pixel blend weights of tests/contrib_ref.py: the symmetric reference and the kernels'
single-pass formulas (``ordered_pass``: D, dD/dw, dD/dt and dD/dalpha) against torch autograd in float64, the Euler
identity ``sum_g w_g dD/dw_g = 2 D`` (D is homogeneous of degree 2 in w), and the geometry reference's ``dL_dopacity``
against central differences of the float64 oracle.  Bars: 1e-12 of max |ref| for the float64 identities (sums of at
most 120 terms); for the finite differences RTOL_BWD = 2e-4, the bar the project holds float32 gradients to (the
reference is the float32 oracle's; the difference quotient's own error at eps = 1e-3 is of order eps^2).
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import common as C
from tests import contrib_ref as CR
from tests import distortion_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = 1e-12
RTOL_BWD = 2e-4


@functools.lru_cache(maxsize=None)
def _ragged():
    case = next(c for c in C.SMALL_CASES if c.name == "ragged_37x23")
    inp = C.build(case)
    ref = C.run_oracle(inp)
    return inp, ref, CR.per_pixel_weights(ref, inp["H"], inp["W"])


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def test_symmetric_reference_matches_autograd():
    """D, dD/dw = 2 S and dD/dt = 2 w sgn of the sort-and-prefix-sum evaluation against autograd of the P x P form."""
    inp, _ref, w = _ragged()
    t = DR.view_depth(inp).double()
    D, S, sgn = DR.symmetric(w, t.numpy())
    assert D.max() > 0
    errs = []
    for n0 in range(0, w.shape[0], 128):
        wt = torch.from_numpy(w[n0:n0 + 128].astype(np.float64)).requires_grad_(True)
        tt = t.clone().requires_grad_(True)
        Dt = (wt[:, :, None] * wt[:, None, :] * (tt[:, None] - tt[None, :]).abs()).sum((1, 2))
        Dt.sum().backward()
        w64 = w[n0:n0 + 128].astype(np.float64)
        on = w64 > 0  # (dD/dw of a Gaussian that does not contribute is not a gradient the kernels form)
        errs.append((_rel(D[n0:n0 + 128], Dt.detach().numpy()), _rel(2 * S[n0:n0 + 128] * on, wt.grad.numpy() * on),
                     np.abs((2 * w64 * sgn[n0:n0 + 128]).sum(0) - tt.grad.numpy()).max()))
    e = np.array(errs).max(0)
    print(f"symmetric vs autograd: D {e[0]:.1e} dD/dw {e[1]:.1e} dD/dt (abs) {e[2]:.1e}")
    assert e[0] <= EXACT and e[1] <= EXACT and e[2] <= EXACT * max(1.0, float(D.max()))
    # Euler: D is homogeneous of degree 2 in w
    euler = _rel((w.astype(np.float64) * 2 * S).sum(1), 2 * D)
    print(f"Euler identity: {euler:.1e}")
    assert euler <= EXACT


@pytest.mark.parametrize("monotone", [True, False])
def test_single_pass_formulas_match_autograd(monotone):
    """The kernels' formulas, pixel by pixel in the oracle's list order: for t non-decreasing along the list the
    ordered D equals the symmetric one; for any t it is the signed form, whose autograd gradients (through w for
    dD/dw, through alpha -> w for dD/dalpha) the single-pass expressions equal."""
    inp, ref, w = _ragged()
    depths = ref.handle.geom()["depths"].astype(np.float64)
    t_all = depths if monotone else np.random.default_rng(5).normal(size=depths.shape[0])
    Dsym, _S, _sgn = DR.symmetric(w, t_all)
    worst = np.zeros(5)
    seen = 0
    for pix in range(0, w.shape[0], 3):
        idx = np.flatnonzero(w[pix] > 0)
        if idx.size < 2:
            continue
        idx = idx[np.argsort(depths[idx], kind="stable")]  # front to back
        wl, tl = w[pix, idx].astype(np.float64), t_all[idx]
        D, g, dt, da = DR.ordered_pass(wl, tl)
        T0 = 1.0 - np.concatenate([[0.0], np.cumsum(wl)[:-1]])
        alpha = torch.from_numpy(wl / T0).requires_grad_(True)
        tt = torch.from_numpy(tl).requires_grad_(True)
        Tt = torch.cat([torch.ones(1, dtype=torch.float64), torch.cumprod(1 - alpha, 0)[:-1]])
        wt = alpha * Tt
        wt.retain_grad()
        behind = torch.tril(torch.ones(idx.size, idx.size, dtype=torch.float64), -1)  # [i, j]: i behind j
        Dt = 2 * (behind * wt[:, None] * wt[None, :] * (tt[:, None] - tt[None, :])).sum()
        Dt.backward()
        Dv = float(Dt.detach())
        scale = max(abs(Dv), 1e-300)
        worst = np.maximum(worst, [abs(D - Dv) / scale, _rel(g, wt.grad.numpy()), _rel(dt, tt.grad.numpy()),
                                   _rel(da, alpha.grad.numpy()),
                                   abs(D - Dsym[pix]) / max(Dsym[pix], 1e-300) if monotone else 0.0])
        seen += 1
    print(f"[monotone={monotone}] {seen} pixels: D {worst[0]:.1e} g {worst[1]:.1e} dD/dt {worst[2]:.1e} "
          f"dD/dalpha {worst[3]:.1e} ordered vs symmetric {worst[4]:.1e}")
    assert seen > 100
    assert (worst <= 1e-10).all()  # (alpha = w / T and the suffix form lose a few digits to cancellation)


def test_geometry_reference_matches_finite_differences():
    """dL_dopacity of the chunked-colour construction against central differences of sum(U * D) under the float64
    oracle, at the three largest entries; U lives on every seventh pixel (~120 oracle backwards per evaluation)."""
    inp, ref, w = _ragged()
    H, W = inp["H"], inp["W"]
    t = DR.view_depth(inp)
    pixels = np.arange(0, H * W, 7)
    U = torch.zeros(1, H, W)
    U.view(-1)[torch.from_numpy(pixels)] = DR.make_upstream(H, W).view(-1)[torch.from_numpy(pixels)]
    got = DR.oracle_distortion(inp, t, U, ref=ref, w=w)
    gop = got["dL_dopacity"][:, 0]
    u = U.double().numpy().reshape(-1)[pixels]

    def loss(op):
        a = dict(inp)
        a["opacities"] = op
        r64 = C.run_oracle(a, precision="f64")
        D, _S, _sgn = DR.symmetric(DR.pixel_weights(r64, H, W, pixels), t.double().numpy())
        return float((u * D).sum())

    eps = 1e-3
    top = np.argsort(-np.abs(gop))[:3]
    for g in top:
        hi, lo = inp["opacities"].clone(), inp["opacities"].clone()
        hi[g] += eps
        lo[g] -= eps
        fd = (loss(hi) - loss(lo)) / (2 * eps)
        e = abs(fd - gop[g]) / abs(gop[g])
        print(f"dL_dopacity[{g}] = {gop[g]:.6e}, central difference {fd:.6e}: {e:.1e}")
        assert abs(gop[g]) > 0 and e <= RTOL_BWD
    for name in DR.GEOM:
        assert got[name].shape[0] == inp["means3D"].shape[0] and np.abs(got[name]).max() > 0, name
    assert np.abs(got["dL_dt"]).max() > 0


def test_symbols_are_declared_bound_and_exported():
    from gaussian_splatting_amd import _lib

    names = _lib.header_symbols(os.path.join(ROOT, "include", "gsr.h"))
    for sym in ("gsr_render_distortion", "gsr_render_distortion_backward"):
        assert sym in names, sym
        assert sym in _lib.SIGNATURES, sym
    assert len(_lib.SIGNATURES["gsr_render_distortion"][1]) == 13
    assert len(_lib.SIGNATURES["gsr_render_distortion_backward"][1]) == 25


def test_the_built_library_exports_the_entry_points():
    from gaussian_splatting_amd import _lib

    lib = _lib.load()
    for sym in ("gsr_render_distortion", "gsr_render_distortion_backward"):
        assert getattr(lib, sym) is not None, sym


def _call(distortion, **over):
    """rasterize_gaussians(distortion=...) on host tensors: every check below must raise before any device work."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, rasterize_gaussians

    P = 5
    z = torch.zeros
    s = GaussianRasterizationSettings(8, 8, 1.0, 1.0, z(3), 1.0, torch.eye(4), torch.eye(4), 0, z(3), False, False, False)
    a = dict(means3D=z(P, 3), means2D=z(P, 3), sh=torch.Tensor([]), colors=z(P, 3), opac=z(P, 1), scales=z(P, 3),
             rot=z(P, 4), cov=torch.Tensor([]))
    a.update(over)
    return rasterize_gaussians(a["means3D"], a["means2D"], a["sh"], a["colors"], a["opac"], a["scales"], a["rot"],
                               a["cov"], s, distortion=distortion)


def _stubbed_check(t, P):
    """check_distortion with the device test stubbed out (no HIP device on the CPU runner)."""
    from gaussian_splatting_amd import _C

    keep = _C._require_device
    _C._require_device = lambda t, name: None
    try:
        _C.check_distortion(t, P)
    finally:
        _C._require_device = keep


def test_distortion_argument_checks_raise():
    from gaussian_splatting_amd import _C

    for call in (_call, lambda t: _C.check_distortion(t, 5)):
        with pytest.raises(RuntimeError, match=r"\(num_points,\)"):
            call(torch.zeros(5, 1))
        with pytest.raises(RuntimeError, match=r"\(num_points,\)"):
            call(torch.zeros(4))  # another point count
        with pytest.raises(RuntimeError, match="float32"):
            call(torch.zeros(5, dtype=torch.float64))
        with pytest.raises(TypeError, match="tensor"):
            call([0.0] * 5)
        with pytest.raises(RuntimeError, match="HIP device"):
            call(torch.zeros(5))  # a host tensor: there is no CPU path
    # contiguity is checked on device tensors (after the device check); here with the device test stubbed out
    with pytest.raises(RuntimeError, match="contiguous"):
        _stubbed_check(torch.zeros(5, 2)[:, 0], 5)
    _stubbed_check(torch.zeros(5), 5)
    # cov3D_precomp with a geometry input that requires grad is refused; without one the call goes on (to the
    # device check here)
    cov = dict(scales=torch.Tensor([]), rot=torch.Tensor([]), cov=torch.zeros(5, 6))
    with pytest.raises(RuntimeError, match="distortion= with cov3D_precomp"):
        _call(torch.zeros(5), means3D=torch.zeros(5, 3, requires_grad=True), **cov)
    with pytest.raises(RuntimeError, match="HIP device"):
        _call(torch.zeros(5, requires_grad=True), **cov)
