"""The absolute screen-space gradient on the GPU: ``rasterize_gaussians_backward(..., absgrad=True)`` (include/gsr.h
gsr_backward_args.dL_dmean2D_abs; the ABSGRAD instantiations of csrc/render.hip render_bwd, gauss_reduce / gauss_bwd in
csrc/backward.hip) and ``means2D.absgrad`` through the autograd nodes.

Reference: tests/absgrad_ref.py -- one backward of the unchanged oracle per pixel, |dL_dmeans2D[:, :2]| summed in
float64 -- which tests/test_absgrad_ref.py pins on the CPU.  Bar: the project's for unit upstream gradients,
RTOL_BWD = 2e-4 of max |ref| per tensor.  Each reference is computed once per (case, loss) and shared read-only.
"""
import functools

import numpy as np
import pytest
import torch

from tests import absgrad_ref as ABR
from tests import alpha_ref as AR
from tests import common as C
from tests.test_gpu_alpha import _backward, _forward, _module_render

pytestmark = pytest.mark.gpu

RTOL_BWD = 2e-4
DEV = "cuda"
PATHS = ["atomic", "record"]
# (case, loss): partial edge tiles; one SH coefficient; the cov2D clamps; antialiasing under a general pose; a
# background colour, also with a joint colour + depth + alpha loss; many segments and batches in one tile
CASES = [("ragged_37x23", "unit"), ("sh0_M1", "unit"), ("pose_clamped", "unit"), ("pose_general_aa", "unit"),
         ("background", "unit"), ("background", "joint"), ("lists_over_8k", "unit")]
SWEEP_CASE = ("lists_over_8k", "unit")  # P = 10000 in one tile: > 32 segments of 256, runs of 512 Gaussians


def _case(name):
    return next(c for c in C.SMALL_CASES + C.POSE_CASES if c.name == name)


def _np(t):
    return t.detach().float().cpu().numpy()


def _threads(name):
    return 4 if name.startswith("lists_") else 1


@functools.lru_cache(maxsize=None)
def _built(name):
    return C.build(_case(name))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return C.run_oracle(_built(name), nthreads=_threads(name))


def _upstream(inp, loss):
    g_c, g_d = C.unit_grads(inp["H"], inp["W"])
    return g_c, g_d, (AR.alpha_grad(inp["H"], inp["W"]) if loss == "joint" else None)


@functools.lru_cache(maxsize=None)
def _ref(name, loss):
    """(absgrad [P,3], oracle gradients by name) of a named case and loss; computed once, read-only."""
    inp = _built(name)
    g_c, g_d, g_a = _upstream(inp, loss)
    ab, sg = ABR.oracle_absgrad(inp, g_c, g_d, g_a, nthreads=_threads(name), ref=_oracle(name))
    if g_a is None:
        grads = _oracle(name).handle.backward(g_c, g_d, nthreads=_threads(name))
    else:
        grads = AR.oracle_joint_grads(inp, g_c, g_d, g_a, ref=_oracle(name))
    assert C.rel_err(sg, grads["dL_dmeans2D"]) <= 1e-5  # the per-pixel terms are those of the one-call backward
    return ab, grads


def _paths(path, **more):
    from gaussian_splatting_amd import _lib

    return _lib.options(bwd_atomic=1 if path == "atomic" else 0, **more)


def _run(name, loss, absgrad=True, fwd=None):
    """Forward (unless given) and one backward of a named case under the options in force; returns (fwd, tuple)."""
    inp = _built(name)
    g_c, g_d, g_a = _upstream(inp, loss)
    fwd = _forward(inp, return_alpha=g_a is not None) if fwd is None else fwd
    kw = {} if g_a is None else {"dL_dout_alpha": g_a}
    if absgrad:
        kw["absgrad"] = True
    out = _backward(inp, fwd, g_c, g_d, **kw)
    torch.cuda.synchronize()
    return fwd, out


def _check_absgrad(got, ref, tag):
    got = _np(got)
    assert got.shape == ref.shape and got.dtype == np.float32, (tag, got.shape)
    assert np.isfinite(got).all(), tag
    err = C.rel_err(got, ref)
    print(f"[{tag}] absgrad {err:.1e} of max |ref| = {np.abs(ref).max():.3g}")
    assert not got[:, 2].any(), tag
    assert err <= RTOL_BWD, (tag, err)
    return err


# ---- 1. parity on both paths; the other gradients are not disturbed -------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,loss", CASES, ids=[f"{n}-{l}" for n, l in CASES])
def test_absgrad_matches_reference(name, loss, path):
    inp = _built(name)
    if name == "pose_clamped":
        C.assert_clamp_preconditions(inp, _oracle(name))
    ref_abs, ref_grads = _ref(name, loss)
    with _paths(path):
        fwd, out = _run(name, loss)
        _, plain = _run(name, loss, absgrad=False, fwd=fwd)
    assert len(out) == len(plain) + 1 == len(C.GRAD_NAMES) + 1
    _check_absgrad(out[-1], ref_abs, f"{name}/{loss}/{path}")
    radii = _np(fwd[2])
    assert (_np(out[-1])[radii == 0] == 0).all()
    # the absolute sum dominates the signed one the same call returned
    g2 = np.abs(_np(out[0])[:, :2]).astype(np.float64)
    assert (_np(out[-1])[:, :2] >= g2 - RTOL_BWD * np.abs(ref_abs).max()).all()
    for k, a, b in zip(C.GRAD_NAMES, out, plain):
        if path == "record":
            assert torch.equal(a, b), k
        else:
            assert C.rel_err(_np(a), ref_grads[k]) <= RTOL_BWD, (k, C.rel_err(_np(a), ref_grads[k]))


@pytest.mark.parametrize("name,loss", [("ragged_37x23", "unit"), ("background", "joint"), ("lists_over_8k", "unit")])
def test_record_path_is_bitwise_reproducible(name, loss):
    with _paths("record"):
        _, one = _run(name, loss)
        _, two = _run(name, loss)
    assert float(one[-1].abs().max()) > 0
    for a, b in zip(one, two):
        assert torch.equal(a, b)


# ---- 2. every way the per-Gaussian stage can run -----------------------------------------------------------------
_SWEEP = [dict(zero_fill=z, live_list=l) for z in range(4) for l in range(2)] + [dict(bwd_grid=2), dict(bwd_seg_ck=1),
                                                                                        dict(bwd_seg_ck=2)]
_SWEEP = [(p, o) for p in PATHS for o in _SWEEP] + [("atomic", dict(touched_run=0)), ("atomic", dict(touched_run=4))]


@pytest.mark.parametrize("path,opts", _SWEEP, ids=[f"{p}-" + ",".join(f"{k}={v}" for k, v in o.items()) for p, o in _SWEEP])
def test_absgrad_under_every_backward_option(path, opts):
    """zero_fill 0-3 x live_list 0/1 (only zero_fill != 0 with the live list takes the atomic path; the others fall
    to the record path, dense or sparse), the strided grid, one-checkpoint segments and both touched-run forms."""
    name, loss = SWEEP_CASE
    ref_abs, ref_grads = _ref(name, loss)
    with _paths(path, **opts):
        _, out = _run(name, loss)
    _check_absgrad(out[-1], ref_abs, f"{name}/{path}/{opts}")
    assert C.rel_err(_np(out[0]), ref_grads["dL_dmeans2D"]) <= RTOL_BWD


@pytest.mark.parametrize("path", PATHS)
def test_poisoned_buffers_are_fully_written(path, monkeypatch):
    """GSR_POISON: scratch 0xff-filled, outputs NaN-filled before the call -- every element of the new output is
    written, and nothing it is computed from was read unwritten."""
    monkeypatch.setenv("GSR_POISON", "1")
    name, loss = "pose_clamped", "unit"  # (115 of its 300 Gaussians are culled)
    with _paths(path):
        fwd, out = _run(name, loss)
    got = _np(out[-1])
    assert np.isfinite(got).all()
    culled = _np(fwd[2]) == 0
    assert culled.sum() >= 64 and not got[culled].any()  # culled rows among them: written as zeros
    _check_absgrad(out[-1], _ref(name, loss)[0], f"poison/{path}")


# ---- 3. empty, culled, repeated -------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_empty_culled_and_second_backward(path):
    g_c, g_d = C.unit_grads(23, 37)
    with _paths(path):
        inp = dict(C.build(C.Case("tmp", P=10, W=37, H=23)))
        for k in ("means3D", "opacities", "shs", "scales", "rotations"):
            inp[k] = inp[k][:0]
        out = _backward(inp, _forward(inp), g_c, g_d, absgrad=True)
        assert len(out) == len(C.GRAD_NAMES) + 1 and tuple(out[-1].shape) == (0, 3)
        # every Gaussian behind the camera: num_rendered == 0, the absolute gradient all zeros
        inp = dict(C.build(C.Case("behind", P=50, W=37, H=23, bg=(0.1, 0.2, 0.3))))
        inp["means3D"] = inp["means3D"].clone()
        inp["means3D"][:, 2] = -5.0
        fwd = _forward(inp)
        assert fwd[0] == 0
        out = _backward(inp, fwd, g_c, g_d, absgrad=True)
        assert tuple(out[-1].shape) == (50, 3) and float(out[-1].abs().max()) == 0.0
        # two backwards of one forward: the first leaves the accumulator rows (floats 10, 11 too) zero again
        name, loss = "ragged_37x23", "unit"
        fwd, one = _run(name, loss)
        _, two = _run(name, loss, fwd=fwd)
    if path == "record":
        assert torch.equal(one[-1], two[-1])
    _check_absgrad(one[-1], _ref(name, loss)[0], f"first/{path}")
    _check_absgrad(two[-1], _ref(name, loss)[0], f"second/{path}")


# ---- 4. the Python surface --------------------------------------------------------------------------------------
def _loss(inp, outs, loss):
    g_c, g_d, g_a = _upstream(inp, loss)
    v = (outs[0] * g_c.to(DEV)).sum() + (outs[2] * g_d.to(DEV)).sum()
    return v if g_a is None else v + (outs[3] * g_a.to(DEV)).sum()


def test_attribute_appears_only_with_the_keyword():
    name = "ragged_37x23"
    inp = _built(name)
    outs, L = _module_render(inp)
    _loss(inp, outs, "unit").backward()
    assert not hasattr(L["means2D"], "absgrad")
    with _paths("record"):
        outs, La = _module_render(inp, absgrad=True)
        assert len(outs) == 3 and not hasattr(La["means2D"], "absgrad")  # set by the backward, not the forward
        _loss(inp, outs, "unit").backward(retain_graph=True)
        first = La["means2D"].absgrad
        assert tuple(first.shape) == (inp["means3D"].shape[0], 3) and first.dtype == torch.float32
        assert first.device.type == "cuda" and not first.requires_grad
        _check_absgrad(first, _ref(name, "unit")[0], "autograd")
        # the other leaves' gradients are those of the render without the keyword, bit for bit
        outs_p, Lp = _module_render(inp)
        _loss(inp, outs_p, "unit").backward()
        for k in ("means2D", "means3D", "opacities", "shs", "scales", "rotations"):
            assert torch.equal(La[k].grad, Lp[k].grad), k
        # each backward overwrites the attribute (gsplat's convention): a second one sets an equal, new tensor
        _loss(inp, outs, "unit").backward()
        assert La["means2D"].absgrad is not first and torch.equal(La["means2D"].absgrad, first)


@pytest.mark.parametrize("form", ["alpha", "camera", "dc"])
def test_keyword_with_the_other_extensions(form):
    name = "background"
    inp = _built(name)
    loss = "joint" if form == "alpha" else "unit"
    kw = dict(return_alpha=True) if form == "alpha" else dict(cam_grad=True) if form == "camera" else dict(split=True)
    with _paths("record"):
        outs, L = _module_render(inp, absgrad=True, **kw)
        _loss(inp, outs, loss).backward()
        outs_p, Lp = _module_render(inp, **kw)
        _loss(inp, outs_p, loss).backward()
    _check_absgrad(L["means2D"].absgrad, _ref(name, loss)[0], form)
    assert not hasattr(Lp["means2D"], "absgrad")
    leaves = ["means2D", "means3D", "opacities"] + {"camera": ["viewmatrix", "projmatrix", "campos"],
                                                     "dc": ["dc", "rest"], "alpha": ["shs"]}[form]
    for k in leaves:
        assert L[k].grad is not None and torch.equal(L[k].grad, Lp[k].grad), k


@pytest.mark.parametrize("index_filter", [False, True])
def test_densification_stats_from_absgrad(index_filter):
    from gaussian_splatting_amd import densify
    from oracle import densify as od

    name = "ragged_37x23"
    inp = _built(name)
    P = inp["means3D"].shape[0]
    outs, L = _module_render(inp, absgrad=True)
    _loss(inp, outs, "unit").backward()
    radii = outs[1]
    model = type("M", (), {})()
    model.xyz_gradient_accum = torch.zeros(P, 1, device=DEV)
    model.denom = torch.zeros(P, 1, device=DEV)
    filt = (radii > 0).nonzero() if index_filter else (radii > 0)
    densify.add_densification_stats(model, L["means2D"], filt, absgrad=True)
    torch.cuda.synchronize()
    accum, denom = np.zeros((P, 1), np.float32), np.zeros((P, 1), np.float32)
    od.densification_stats(_np(L["means2D"].absgrad), accum, denom, None, _np(radii).astype(np.int32))
    np.testing.assert_array_equal(_np(model.xyz_gradient_accum), accum)
    np.testing.assert_array_equal(_np(model.denom), denom)
    assert accum.max() > 0
    # it is not the signed statistic, and without the attribute the request is refused
    assert float((L["means2D"].absgrad[:, :2].norm(dim=1) - L["means2D"].grad[:, :2].norm(dim=1)).max()) > 0
    with pytest.raises(RuntimeError, match="absgrad"):
        densify.add_densification_stats(model, torch.zeros(P, 3, device=DEV), filt, absgrad=True)


def test_census_with_absgrad_is_refused():
    """render_bwd has no CENSUS x ABSGRAD instantiation: the combination is GSR_ERR_ARGUMENT (include/gsr.h)."""
    from gaussian_splatting_amd import _lib

    lib = _lib.load()
    counters = torch.zeros(16, dtype=torch.int64, device=DEV)
    name, loss = "ragged_37x23", "unit"
    fwd, _ = _run(name, loss)
    assert lib.gsr_census_set(counters.data_ptr()) == 0
    try:
        with pytest.raises(_lib.GsrError, match="census"):
            _run(name, loss, fwd=fwd)
    finally:
        assert lib.gsr_census_set(None) == 0
