"""The per-Gaussian contribution statistics on the GPU: ``_C.contribution_stats`` (include/gsr.h gsr_contrib_stats;
csrc/contrib.hip), ``return_contrib=True`` through the autograd nodes and ``contrib.render_contribution``.

Reference: tests/contrib_ref.py -- one backward of the unchanged oracle per pixel gives the blend weights, from which
the maximum, the count and (in float64) the sums follow -- which tests/test_contrib_ref.py pins on the CPU.  Bars,
the project's own: the two sums RTOL_BWD = 2e-4 of max |ref| (the bar dL_dcolors is held to), ``weight_max``
ATOL_FWD = 1e-5 (the forward's float bar), ``pixel_count`` equal.  Where the oracle's pixel_margins flag a pixel as
near a discrete threshold (1e-5 / 1e-4 / 1e-4), the rows blending there get ``weight_max`` within 1e-2 -- an
alpha-skip or termination flip moves a later weight by less than w / 255, the terminator's own weight by less than
1e-2 -- and ``pixel_count`` within the number of flagged pixels; the strict cases assert that no pixel is flagged.
Each reference is computed once per case and shared read-only.
"""
import functools

import numpy as np
import pytest
import torch

from tests import common as C
from tests import contrib_ref as CR
from tests.test_gpu_alpha import _backward, _forward, _module_render

pytestmark = pytest.mark.gpu

RTOL_BWD = 2e-4
ATOL_FWD = 1e-5
ATOL_NEAR = 1e-2
DEV = "cuda"
STRICT = ["ragged_37x23", "background", "pose_clamped"]
LONG = [("lists_2k_4k", {}), ("lists_2k_4k", {"bwd_seg_ck": 1}), ("lists_2k_4k", {"bwd_seg_ck": 2}),
        ("lists_over_8k", {}), ("pose_general_aa", {})]


def _case(name):
    return next(c for c in C.SMALL_CASES + C.POSE_CASES if c.name == name)


def _np(t):
    return t.detach().cpu().numpy()


def _threads(name):
    return 4 if name.startswith("lists_") else 1


@functools.lru_cache(maxsize=None)
def _built(name):
    return C.build(_case(name))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return C.run_oracle(_built(name), nthreads=_threads(name))


@functools.lru_cache(maxsize=None)
def _wmap(name):
    inp = _built(name)
    return CR.weight_map(inp["H"], inp["W"])


@functools.lru_cache(maxsize=None)
def _ref(name):
    return CR.oracle_contrib(_built(name), _wmap(name), nthreads=_threads(name), ref=_oracle(name))


def _stats(inp, fwd, weight=None, out=None):
    from gaussian_splatting_amd import _C

    nr, _color, _radii, geom, binning, img = fwd[:6]
    st = _C.contribution_stats(geom, binning, img, nr, inp["means3D"].shape[0], inp["H"], inp["W"],
                               pixel_weight=None if weight is None else weight.to(DEV), out=out)
    torch.cuda.synchronize()
    return st


def _cols(st):
    """(weight_sum f64, weight_max f32, pixel_count int64, weighted_sum f64) as numpy arrays."""
    a = _np(st)
    assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 4
    return a[:, 0].astype(np.float64), a[:, 1].copy(), a.view(np.uint32)[:, 2].astype(np.int64), a[:, 3].astype(np.float64)


def _check(st, ref, tag, weighted=True):
    """The parity rule of the module docstring; returns the number of near rows."""
    s, mx, cnt, sw = _cols(st)
    assert np.isfinite(_np(st)[:, [0, 1, 3]]).all(), tag
    flagged = ref["flagged"].reshape(-1)
    near = (ref["w"][flagged] > 0).any(0) if flagged.any() else np.zeros(s.shape, bool)
    con = ref["pixel_count"] > 0
    e_s = C.rel_err(s, ref["weight_sum"])
    e_w = C.rel_err(sw, ref["weighted_sum"]) if weighted else 0.0
    d_mx = np.abs(mx.astype(np.float64) - ref["weight_max"])
    d_cnt = np.abs(cnt - ref["pixel_count"])
    print(f"[{tag}] weight_sum {e_s:.1e} weighted_sum {e_w:.1e} of max |ref|; weight_max strict {d_mx[~near].max():.1e}"
          f" near {d_mx[near].max() if near.any() else 0:.1e}; pixel_count off by <= {int(d_cnt.max())} "
          f"(strict {int(d_cnt[~near].max())}); flagged pixels {int(flagged.sum())}, near rows {int(near.sum())} of "
          f"{int(con.sum())} contributing")
    assert e_s <= RTOL_BWD and e_w <= RTOL_BWD, (tag, e_s, e_w)
    if not weighted:
        assert not sw.any(), tag
    assert d_mx[~near].max() <= ATOL_FWD, (tag, d_mx[~near].max())
    assert (cnt[~near] == ref["pixel_count"][~near]).all(), tag
    if near.any():
        assert d_mx[near].max() <= ATOL_NEAR, (tag, d_mx[near].max())
        assert d_cnt[near].max() <= int(flagged.sum()), (tag, d_cnt[near].max())
    return int(near.sum())


# ---- 1. parity, strict ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STRICT)
def test_statistics_match_reference_strict(name):
    inp, ref = _built(name), _ref(name)
    assert not ref["flagged"].any()  # the precondition: no pixel near a threshold, so no row is excused
    if name == "pose_clamped":
        C.assert_clamp_preconditions(inp, _oracle(name))
    fwd = _forward(inp)
    st = _stats(inp, fwd, _wmap(name))
    assert tuple(st.shape) == (inp["means3D"].shape[0], 4) and st.dtype == torch.float32 and not st.requires_grad
    assert _check(st, ref, name) == 0
    culled = _np(fwd[2]) == 0
    if name == "pose_clamped":
        assert int(culled.sum()) == 115
    assert not _np(st).view(np.uint32)[culled].any()
    # without a map the fourth column stays zero and the others are the same
    plain = _stats(inp, fwd)
    _check(plain, ref, name + "/no map", weighted=False)
    assert torch.equal(plain[:, 1:3].view(torch.int32), st[:, 1:3].view(torch.int32))


# ---- 2. parity, long lists ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,opts", LONG, ids=[n + "".join(f"-{k}={v}" for k, v in o.items()) for n, o in LONG])
def test_statistics_match_reference_long_lists(name, opts):
    from gaussian_splatting_amd import _lib

    inp, ref = _built(name), _ref(name)
    con = int((ref["pixel_count"] > 0).sum())
    assert 0 < int(ref["flagged"].sum()) <= 0.01 * ref["flagged"].size
    if name == "lists_2k_4k":
        assert int(_oracle(name).handle.image()["n_contrib"].max()) > 256  # a tile spans two checkpoints
    with _lib.options(**opts):
        fwd = _forward(inp)
        st = _stats(inp, fwd, _wmap(name))
    near = _check(st, ref, f"{name}/{opts}")
    assert 3 * (con - near) >= con, (near, con)  # at least a third of the contributing rows stay strict


# ---- 3. invariants on the GPU's own state ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_37x23", "dense_opaque", "lists_2k_4k", "pose_general_aa"])
def test_invariants_of_the_forward_state(name):
    inp = _built(name)
    fwd = _forward(inp, return_alpha=True)
    s, mx, cnt, _sw = _cols(_stats(inp, fwd))
    total = float(_np(fwd[7]).astype(np.float64).sum())
    err = abs(s.sum() - total) / total
    print(f"[{name}] sum_g weight_sum = {s.sum():.6f}, sum_pix alpha = {total:.6f}: {err:.1e}")
    assert err <= 1e-5
    assert (s >= mx).all() and (mx <= 0.99).all() and (mx >= 0).all()
    assert ((cnt > 0) == (s > 0)).all() and ((cnt > 0) == (mx > 0)).all()
    assert cnt.max() <= inp["H"] * inp["W"]
    culled = _np(fwd[2]) == 0
    assert not s[culled].any() and not cnt[culled].any() and not mx[culled].any()


# ---- 4. option independence -------------------------------------------------------------------------------------
_SETTINGS = [dict(fwd_quads=4), dict(fwd_quads=2), dict(bwd_seg_ck=1), dict(bwd_seg_ck=2), dict(sort_prefix=0),
             dict(sort_prefix=64, near_mass=0), dict(near_mass=0), dict(near_mass=1, hint=True), dict(bwd_atomic=0),
             dict(bwd_atomic=1), dict(no_backward=True), dict(bwd_grid=1), dict(bwd_grid=2)]


def _forward_under(inp, name, opts):
    """A forward of ``inp`` under ``opts`` (``hint``: with the capacity hint that lets near-first binning apply,
    ``no_backward``: the eval-render forward); returns (fwd, statistics computed under the same options)."""
    from gaussian_splatting_amd import _C as CM
    from gaussian_splatting_amd import _lib

    opts = dict(opts)
    key = (torch.cuda.current_device(), inp["W"], inp["H"])
    if opts.pop("hint", False):
        CM._capacity[key] = (inp["means3D"].shape[0], _oracle(name).num_rendered)
    kw = dict(no_backward=True) if opts.pop("no_backward", False) else {}
    try:
        with _lib.options(**opts):
            fwd = _forward(inp, **kw)
            return fwd, _stats(inp, fwd, _wmap(name))
    finally:
        CM._capacity.pop(key, None)


@pytest.fixture(scope="module")
def base_2k_4k():
    inp = _built("lists_2k_4k")
    fwd = _forward(inp)
    return fwd, _stats(inp, fwd, _wmap("lists_2k_4k"))


@pytest.mark.parametrize("opts", _SETTINGS, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o in _SETTINGS])
def test_maximum_and_count_do_not_depend_on_the_options(opts, base_2k_4k):
    """``weight_max`` and ``pixel_count`` bit for bit those of the default forward, the sums within 2e-4.

    ``fwd_quads=4`` is the hard one: the compiler contracts the exponent ``dx (A dx + B dy) + C dy^2`` of render.hip
    differently in the whole-tile forward than in the half-tile one, so the T in the two forwards' checkpoints
    differs in the last bits (a kernel that started every unit from the checkpoint gave 7 rows a weight_max 1-2 ulp
    off here).  After a whole-tile forward the statistics units therefore re-walk their tile's list for T instead
    (csrc/contrib.hip CKPT)."""
    name = "lists_2k_4k"
    inp = _built(name)
    _, base = base_2k_4k
    assert float(base[:, 1].max()) > 0
    _, st = _forward_under(inp, name, opts)
    a, b = _np(st).view(np.int32).astype(np.int64), _np(base).view(np.int32).astype(np.int64)
    d_mx, d_cnt = np.abs(a[:, 1] - b[:, 1]), np.abs(a[:, 2] - b[:, 2])
    errs = [C.rel_err(_np(st[:, col]), _np(base[:, col])) for col in (0, 3)]
    print(f"[{opts}] weight_max differs in {int((d_mx > 0).sum())} rows (by <= {int(d_mx.max())} ulp), pixel_count in "
          f"{int((d_cnt > 0).sum())} rows (by <= {int(d_cnt.max())}); sums {errs[0]:.1e} / {errs[1]:.1e}")
    assert max(errs) <= RTOL_BWD, errs
    assert torch.equal(st[:, 1:3].view(torch.int32), base[:, 1:3].view(torch.int32))


def test_two_calls_on_one_forward_are_bitwise_equal_in_maximum_and_count(base_2k_4k):
    inp = _built("lists_2k_4k")
    fwd, base = base_2k_4k
    again = _stats(inp, fwd, _wmap("lists_2k_4k"))
    assert torch.equal(again[:, 1:3].view(torch.int32), base[:, 1:3].view(torch.int32))
    for col in (0, 3):
        assert C.rel_err(_np(again[:, col]), _np(base[:, col])) <= RTOL_BWD


@pytest.mark.parametrize("name,opts", [("lists_2k_4k", {}), ("lists_2k_4k", {"bwd_seg_ck": 2, "bwd_grid": 2}),
                                       ("lists_over_8k", {}), ("dense_opaque", {})],
                         ids=["lists_2k_4k", "lists_2k_4k-seg2-strided", "lists_over_8k", "dense_opaque"])
def test_copied_buffers_give_the_same_maximum_and_count(name, opts):
    """Buffers the library has not seen (copies) take the checkpoint-free walk: the same bits in the two columns."""
    from gaussian_splatting_amd import _lib

    inp = _built(name)
    with _lib.options(**opts):
        fwd = _forward(inp)
        own = _stats(inp, fwd, _wmap(name))
        copied = _stats(inp, fwd[:3] + tuple(t.clone() for t in fwd[3:6]), _wmap(name))
    assert float(own[:, 1].max()) > 0
    assert torch.equal(copied[:, 1:3].view(torch.int32), own[:, 1:3].view(torch.int32))
    for col in (0, 3):
        assert C.rel_err(_np(copied[:, col]), _np(own[:, col])) <= RTOL_BWD


# ---- 5. non-interference with the backward --------------------------------------------------------------------
@pytest.mark.parametrize("path", ["atomic", "record"])
@pytest.mark.parametrize("name", ["background", "lists_2k_4k"])
def test_backward_is_unaffected_and_leaves_the_statistics_alone(name, path):
    from gaussian_splatting_amd import _lib

    inp = _built(name)
    g_c, g_d = C.unit_grads(inp["H"], inp["W"])
    with _lib.options(bwd_atomic=1 if path == "atomic" else 0):
        fwd = _forward(inp)
        first = _stats(inp, fwd, _wmap(name))
        with_stats = _backward(inp, fwd, g_c, g_d)
        after = _stats(inp, fwd, _wmap(name))
        fresh = _backward(inp, _forward(inp), g_c, g_d)
        torch.cuda.synchronize()
    for k, a, b in zip(C.GRAD_NAMES, with_stats, fresh):
        if path == "record":
            assert torch.equal(a, b), k
        else:  # (float atomics: the hardware's order)
            assert C.rel_err(_np(a), _np(b)) <= RTOL_BWD, k
    assert torch.equal(after[:, 1:3].view(torch.int32), first[:, 1:3].view(torch.int32))
    for col in (0, 3):
        assert C.rel_err(_np(after[:, col]), _np(first[:, col])) <= RTOL_BWD


# ---- 6. accumulate ----------------------------------------------------------------------------------------------
def test_two_views_accumulate_into_one_buffer():
    a_name, b_name = "sh3_scalerot", "yawed_view"  # one scene, two cameras
    ia, ib = _built(a_name), _built(b_name)
    assert torch.equal(ia["means3D"], ib["means3D"]) and not torch.equal(ia["viewmatrix"], ib["viewmatrix"])
    P = ia["means3D"].shape[0]
    fa, fb = _forward(ia), _forward(ib)
    sa, sb = _stats(ia, fa, _wmap(a_name)), _stats(ib, fb, _wmap(b_name))
    out = torch.zeros(P, 4, device=DEV)
    assert _stats(ia, fa, _wmap(a_name), out=out) is out
    assert _stats(ib, fb, _wmap(b_name), out=out) is out
    s, mx, cnt, sw = _cols(out)
    s_a, mx_a, cnt_a, sw_a = _cols(sa)
    s_b, mx_b, cnt_b, sw_b = _cols(sb)
    assert (mx == np.maximum(mx_a, mx_b)).all() and (cnt == cnt_a + cnt_b).all()
    assert ((cnt_a > 0) & (cnt_b > 0)).any()  # Gaussians seen in both views
    assert C.rel_err(s, s_a + s_b) <= RTOL_BWD and C.rel_err(sw, sw_a + sw_b) <= RTOL_BWD


# ---- 7. buffer handling -------------------------------------------------------------------------------------------
def test_poisoned_output_is_fully_written(monkeypatch):
    """GSR_POISON: scratch 0xff-filled, the output NaN-filled before the call -- every row is written."""
    monkeypatch.setenv("GSR_POISON", "1")
    name = "pose_clamped"
    inp = _built(name)
    fwd = _forward(inp)
    st = _stats(inp, fwd, _wmap(name))
    assert np.isfinite(_np(st)[:, [0, 1, 3]]).all()
    culled = _np(fwd[2]) == 0
    assert culled.sum() >= 64 and not _np(st).view(np.uint32)[culled].any()
    _check(st, _ref(name), "poison")


def test_empty_and_culled_scenes():
    inp = dict(C.build(C.Case("tmp", P=10, W=37, H=23)))
    for k in ("means3D", "opacities", "shs", "scales", "rotations"):
        inp[k] = inp[k][:0]
    st = _stats(inp, _forward(inp), CR.weight_map(23, 37))
    assert tuple(st.shape) == (0, 4) and st.dtype == torch.float32
    # every Gaussian behind the camera: num_rendered == 0, all rows zero
    inp = dict(C.build(C.Case("behind", P=50, W=37, H=23, bg=(0.1, 0.2, 0.3))))
    inp["means3D"] = inp["means3D"].clone()
    inp["means3D"][:, 2] = -5.0
    fwd = _forward(inp)
    assert fwd[0] == 0
    st = _stats(inp, fwd, CR.weight_map(23, 37))
    assert tuple(st.shape) == (50, 4) and not _np(st).view(np.uint32).any()
    # ... and accumulating it changes nothing
    out = torch.full((50, 4), 2.0, device=DEV)
    assert torch.equal(_stats(inp, fwd, out=out), torch.full((50, 4), 2.0, device=DEV))


def test_bad_arguments_raise_and_the_library_stays_usable():
    name = "ragged_37x23"
    inp = _built(name)
    P, H, W = inp["means3D"].shape[0], inp["H"], inp["W"]
    fwd = _forward(inp)
    misaligned = torch.zeros(4 * P + 1, device=DEV)[1:].view(P, 4)
    assert misaligned.is_contiguous() and misaligned.data_ptr() % 16 != 0
    with pytest.raises(RuntimeError, match="aligned"):
        _stats(inp, fwd, out=misaligned)
    with pytest.raises(RuntimeError, match="pixel_weight"):
        _stats(inp, fwd, torch.ones(W, H + 1))
    with pytest.raises(RuntimeError, match="out"):
        _stats(inp, fwd, out=torch.zeros(P, 3, device=DEV))
    _check(_stats(inp, fwd, _wmap(name)), _ref(name), "after errors")


# ---- 8. the Python surface ------------------------------------------------------------------------------------
def _same_statistics(a, b):
    assert torch.equal(a[:, 1:3].view(torch.int32), b[:, 1:3].view(torch.int32))
    for col in (0, 3):
        assert C.rel_err(_np(a[:, col]), _np(b[:, col])) <= RTOL_BWD


def test_keyword_appends_one_non_differentiable_output():
    name = "ragged_37x23"
    inp = _built(name)
    g_c, g_d = C.unit_grads(inp["H"], inp["W"])
    outs_p, Lp = _module_render(inp)
    assert len(outs_p) == 3  # unchanged without the keyword
    outs, L = _module_render(inp, return_contrib=True)
    assert len(outs) == 4
    st = outs[3]
    assert tuple(st.shape) == (inp["means3D"].shape[0], 4) and not st.requires_grad and st.device.type == "cuda"
    _check(st, _ref(name), "node", weighted=False)
    outs_w, _ = _module_render(inp, return_contrib=True, contrib_weight=_wmap(name).to(DEV)[None])
    _check(outs_w[3], _ref(name), "node/weight")
    with pytest.raises(TypeError, match="return_contrib"):
        _module_render(inp, contrib_weight=_wmap(name).to(DEV))


@pytest.mark.record_path
@pytest.mark.parametrize("form", ["plain", "alpha", "absgrad", "dc", "camera"])
def test_keyword_with_the_other_extensions(form):
    name = "background"
    inp = _built(name)
    g_c, g_d = C.unit_grads(inp["H"], inp["W"])
    kw = {"plain": {}, "alpha": dict(return_alpha=True), "absgrad": dict(absgrad=True), "dc": dict(split=True),
          "camera": dict(cam_grad=True)}[form]

    def loss(o):
        v = (o[0] * g_c.to(DEV)).sum() + (o[2] * g_d.to(DEV)).sum()
        return v + o[3].sum() if form == "alpha" else v

    outs, L = _module_render(inp, return_contrib=True, contrib_weight=_wmap(name).to(DEV), **kw)
    outs_p, Lp = _module_render(inp, **kw)
    assert len(outs) == len(outs_p) + 1 == (5 if form == "alpha" else 4)
    st = outs[-1]
    assert not st.requires_grad and tuple(st.shape) == (inp["means3D"].shape[0], 4)
    _check(st, _ref(name), form)
    for a, b in zip(outs, outs_p):
        assert torch.equal(a, b)
    loss(outs).backward()
    loss(outs_p).backward()
    leaves = ["means2D", "means3D", "opacities", "scales", "rotations"] + {
        "camera": ["viewmatrix", "projmatrix", "campos"], "dc": ["dc", "rest"]}.get(form, ["shs"])
    for k in leaves:  # the statistics call leaves the backward what it was, bit for bit (record path)
        assert L[k].grad is not None and torch.equal(L[k].grad, Lp[k].grad), k
    if form == "absgrad":
        assert torch.equal(L["means2D"].absgrad, Lp["means2D"].absgrad)


def test_render_contribution_equals_the_node():
    from diff_gaussian_rasterization import ContributionStats, render_contribution, split
    from tests.test_gpu_camera import _settings

    name = "background"
    inp = _built(name)
    m = _wmap(name).to(DEV)
    outs, L = _module_render(inp, return_contrib=True, contrib_weight=m)
    d = lambda k: inp[k].to(DEV)  # noqa: E731
    s = _settings(inp, d("viewmatrix"), d("projmatrix"), d("campos"))
    color, radii, st = render_contribution(s, d("means3D"), d("opacities"), shs=d("shs"), scales=d("scales"),
                                           rotations=d("rotations"), pixel_weight=m)
    assert torch.equal(color, outs[0]) and torch.equal(radii, outs[1]) and not st.requires_grad
    _same_statistics(st, outs[3])
    named = split(st)
    assert isinstance(named, ContributionStats) and named.pixel_count.dtype == torch.int32
    assert int(named.pixel_count.max()) == int(_ref(name)["pixel_count"].max())
    # a sweep accumulates into one buffer; the separate-SH form renders the same
    out = torch.zeros_like(st)
    for _ in range(2):
        _c, _r, acc = render_contribution(s, d("means3D"), d("opacities"), dc=d("shs")[:, :1].contiguous(),
                                          shs=d("shs")[:, 1:].contiguous(), scales=d("scales"),
                                          rotations=d("rotations"), pixel_weight=m, out=out)
        assert acc is out
    two = split(out)
    assert torch.equal(two.weight_max, named.weight_max) and torch.equal(two.pixel_count, 2 * named.pixel_count)
    assert C.rel_err(_np(two.weight_sum), 2 * _np(named.weight_sum)) <= RTOL_BWD
