"""The forward's staging-time footprint test (csrc/footprint.h) at its edge cases, on the GPU.

A quadrant the test drops wrongly loses every pixel of a splat there: an error of at least alpha T >= T / 255 in
the image, far over the 1e-5 bar.  The scenes put the splats where the test decides: strongly anisotropic,
rotated, means within 1 px of the 8-pixel quadrant boundaries and their crossings, opacities from under the
1/255 threshold up to 0.99, SH degree 3.

* ``edges_48x40``: 3 x 3 tiles with partial right and bottom tiles (whole launches of half-tile or whole-tile
  units);
* ``edges_76x60``: 5 x 4 tiles, enough for the hybrid launch, whose last tiles run as single-quadrant units.

GPU forward and backward against the f32 oracle at the parity bars (tests/test_gpu_parity.py): num_rendered,
radii and n_contrib exact, image and inverse depth 1e-5, gradients 2e-4 of each tensor's maximum (unit upstream
gradient) and 1e-5 absolute (L1-mean upstream gradient); under fwd_quads 2 and 4 and bwd_atomic 0 and 1, and
bitwise equal between two runs under bwd_atomic = 0.
"""
import math

import numpy as np
import pytest
import torch

from tests import common as C

pytestmark = pytest.mark.gpu

ATOL_FWD = 1e-5
RTOL_BWD = 2e-4

# (seeds: ones at which the f32 and f64 oracles agree on every n_contrib -- check_scene asserts it -- so that no
# pixel of the scene hangs on how one exponential rounds)
CASES = [C.Case("edges_48x40", P=300, W=48, H=40, focal=45.0, seed=1),
         C.Case("edges_76x60", P=300, W=76, H=60, focal=70.0, seed=2)]


def build_edges(case):
    """C.build(case) with means moved onto the quadrant grid, needle-shaped splats and wide-ranging opacities."""
    inp = C.build(case)
    P, W, H = case.P, case.W, case.H
    g = torch.Generator().manual_seed(case.seed + 4242)
    u = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)  # noqa: E731
    z = inp["means3D"][:, 2].double()
    # pixel targets: x, y or both within 1 px of a multiple of 8 (thirds of the scene)
    kind = torch.arange(P) % 3
    free_x, free_y = u(P) * (W + 8) - 4, u(P) * (H + 8) - 4
    snap_x = 8 * torch.floor(u(P) * (W // 8 + 1)) + (2 * u(P) - 1)
    snap_y = 8 * torch.floor(u(P) * (H // 8 + 1)) + (2 * u(P) - 1)
    px = torch.where(kind != 1, snap_x, free_x)
    py = torch.where(kind != 0, snap_y, free_y)
    # ndc2Pix inverted: pixel = ((ndc + 1) S - 1) / 2, ndc = view / (z tanfov) under the identity pose
    x = ((2 * px + 1) / W - 1) * inp["tanfovx"] * z
    y = ((2 * py + 1) / H - 1) * inp["tanfovy"] * z
    inp["means3D"] = torch.stack([x, y, z], 1).float().contiguous()
    # needles of 3..20 px by 1/8..1/40 of that, turned about the view axis with a small tilt
    sigma = torch.exp(math.log(3.0) + u(P) * math.log(20.0 / 3.0)) * z / case.focal
    thin = sigma / (8 + 32 * u(P))
    inp["scales"] = torch.stack([sigma, thin, thin], 1).float().contiguous()
    th = u(P) * math.pi
    q = torch.stack([torch.cos(th / 2), 0.08 * (2 * u(P) - 1), 0.08 * (2 * u(P) - 1), torch.sin(th / 2)], 1)
    inp["rotations"] = torch.nn.functional.normalize(q, dim=1).float().contiguous()
    # opacities log-uniform over [0.5 / 255, 0.99], every eighth within 0.2% of the 1/255 threshold
    o = torch.exp(math.log(0.5 / 255) + u(P) * (math.log(0.99) - math.log(0.5 / 255)))
    o = torch.where(torch.arange(P) % 8 == 0, (1 + 2e-3 * (2 * u(P) - 1)) / 255, o)
    inp["opacities"] = o.float().reshape(P, 1).contiguous()
    return inp


def check_scene(case, inp, ref):
    """The scene is what the docstring says, by the oracle's own projected means and conics."""
    geom = ref.handle.geom()
    vis = ref.radii > 0
    assert vis.sum() >= 0.8 * case.P, int(vis.sum())
    m = geom["means2D"][vis].astype(np.float64)
    near = np.abs(m - 8 * np.round(m / 8)) <= 1.0 + 1e-3
    assert near[:, 0].mean() > 0.6 and near[:, 1].mean() > 0.6 and (near[:, 0] & near[:, 1]).mean() > 0.3
    a, b, c, o = (geom["conic_opacity"][vis][:, i].astype(np.float64) for i in range(4))
    disc = np.sqrt(((a - c) / 2) ** 2 + b * b)
    ratio = np.sqrt(((a + c) / 2 + disc) / ((a + c) / 2 - disc))
    assert np.median(ratio) > 4 and ratio.max() > 15, (np.median(ratio), ratio.max())
    assert (np.abs(b) > 0.1 * np.sqrt(a * c)).mean() > 0.5  # rotated
    assert (o < 1 / 255).any() and (o > 0.9).any() and (np.abs(o * 255 - 1) < 3e-3).sum() >= 10
    assert ref.num_rendered > 2 * case.P
    # no pixel sits on a rounding threshold: the f32 and f64 oracles agree, so the GPU is held to the plain bars
    ref64 = C.run_oracle(inp, precision="f64")
    np.testing.assert_array_equal(ref.handle.image()["n_contrib"], ref64.handle.image()["n_contrib"])
    np.testing.assert_allclose(ref.color, ref64.color, atol=ATOL_FWD, rtol=0)


_REFS: dict = {}


def reference(case):
    """(inputs, f32 oracle result, {mode: upstream gradients and the oracle's backward}), once per process."""
    if case.name not in _REFS:
        inp = build_edges(case)
        ref = C.run_oracle(inp)
        check_scene(case, inp, ref)
        grads = {}
        for mode, (gc, gd) in (("unit", C.unit_grads(case.H, case.W)), ("l1", C.l1_grads(case.H, case.W))):
            grads[mode] = (gc, gd, ref.handle.backward(gc, gd))
        _REFS[case.name] = (inp, ref, grads)
    return _REFS[case.name]


def _to_np(t):
    return t.detach().float().cpu().numpy()


@pytest.mark.parametrize("bwd_atomic", [0, 1])
@pytest.mark.parametrize("fwd_quads", [2, 4])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_edge_scene_matches_oracle(case, fwd_quads, bwd_atomic):
    from gaussian_splatting_amd import _C as CM
    from gaussian_splatting_amd import _lib

    inp, ref, grads = reference(case)
    with _lib.options(fwd_quads=fwd_quads, bwd_atomic=bwd_atomic):
        runs = []
        for _ in range(2 if bwd_atomic == 0 else 1):
            fwd = C.run_gpu_forward(inp)
            outs = {mode: C.run_gpu_backward(inp, fwd, gc, gd) for mode, (gc, gd, _) in grads.items()}
            torch.cuda.synchronize()
            runs.append((fwd, outs))
    fwd, outs = runs[0]
    nr, color, radii, _, _, _, invd = fwd
    assert nr == ref.num_rendered
    np.testing.assert_array_equal(_to_np(radii).astype(np.int32), ref.radii)
    st = CM.debug_forward_state(fwd, case.P)
    np.testing.assert_array_equal(st["n_contrib"].numpy(), ref.handle.image()["n_contrib"].astype(np.int64))
    print(f"[{case.name} quads={fwd_quads} atomic={bwd_atomic}] max|dcolor| "
          f"{np.abs(_to_np(color) - ref.color).max():.2e} max|dinvdepth| {np.abs(_to_np(invd) - ref.invdepth).max():.2e}")
    np.testing.assert_allclose(_to_np(color), ref.color, atol=ATOL_FWD, rtol=0)
    np.testing.assert_allclose(_to_np(invd), ref.invdepth, atol=ATOL_FWD, rtol=0)
    for mode, (_, _, r) in grads.items():
        for k, got in zip(C.GRAD_NAMES, outs[mode]):
            got = _to_np(got)
            assert got.shape == r[k].shape, (k, got.shape, r[k].shape)
            print(f"  {mode} {k}: rel err {C.rel_err(got, r[k]):.2e} max abs err {np.abs(got - r[k]).max():.2e}")
            if mode == "l1":
                np.testing.assert_allclose(got, r[k], atol=1e-5, rtol=0, err_msg=k)
            else:
                assert C.rel_err(got, r[k]) <= RTOL_BWD, (k, C.rel_err(got, r[k]))
    if bwd_atomic == 0:  # the record path: no float atomics, so two runs agree bit for bit
        (fwd2, outs2) = runs[1]
        np.testing.assert_array_equal(_to_np(fwd[1]), _to_np(fwd2[1]))
        np.testing.assert_array_equal(_to_np(fwd[6]), _to_np(fwd2[6]))
        for mode in outs:
            for k, x, y in zip(C.GRAD_NAMES, outs[mode], outs2[mode]):
                np.testing.assert_array_equal(_to_np(x), _to_np(y), err_msg=f"{mode} {k}")
