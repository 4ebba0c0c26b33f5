"""3DGS-MCMC density control on the GPU (include/gsr_mcmc.h, csrc/mcmc.hip, gaussian_splatting_amd/mcmc.py) against
the float64 reference tests/mcmc_ref.py (pinned by tests/test_mcmc_ref.py).

Tolerances.  Noise: the project's float bar, atol 1e-5, on displacements whose median is above 1e-3 (asserted from
the reference alone, so the bar means something).  Relocation: both sides compute in double and round to float32
once; they differ by libm's last bits and the summation form (at most 2.2e-13), hence by at most one float32 ulp
(1.2e-7 relative): rtol = atol = 1e-6.  Row surgery: bitwise.
"""
import functools

import numpy as np
import pytest
import torch

from tests import mcmc_ref as MR
from tests import test_densify as TD  # the GaussianModel-shaped model and its random parameters (helpers only)

pytestmark = pytest.mark.gpu

NOISE_SIZES = (1, 63, 64, 65, 257, 4099)  # one lane, around a wave, a ragged second workgroup, 17 workgroups
NOISE_SCALE = 80.0
SPECIAL_OPACITIES = (0.0051, 0.3, 0.9, 0.999999)


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    return torch.tensor(np.asarray(a), device=_dev(), dtype=dtype)


# ---- noise ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _noise_case():
    """One draw (numpy seed 0) at the largest size; the smaller sizes are its leading rows.  Returns the float32 inputs
    and the float64 reference's displacement."""
    rng = np.random.default_rng(0)
    P = max(NOISE_SIZES)
    inp = {"xyz": rng.uniform(-3, 3, (P, 3)), "opacity": rng.uniform(-9, -3, (P, 1)),
           "scaling": rng.uniform(-5, -2.5, (P, 3)), "rotation": rng.standard_normal((P, 4)),
           "xi": rng.standard_normal((P, 3))}
    inp = {k: v.astype(np.float32) for k, v in inp.items()}
    delta = MR.noise_delta(inp["opacity"], inp["scaling"], inp["rotation"], inp["xi"], NOISE_SCALE)
    for v in inp.values():
        v.setflags(write=False)
    delta.setflags(write=False)
    return inp, delta


def test_noise_reference_displacement_dwarfs_the_bar():
    _, delta = _noise_case()
    med, top = float(np.median(np.abs(delta))), float(np.abs(delta).max())
    print(f"reference displacement at P = {len(delta)}: median {med:.3g}, max {top:.3g}")
    assert med >= 1e-3 and top <= 1.0


@pytest.mark.parametrize("P", NOISE_SIZES)
def test_noise_matches_reference(P):
    from gaussian_splatting_amd import mcmc

    inp, delta = _noise_case()
    xyz = _t(inp["xyz"][:P])
    mcmc.noise(xyz, _t(inp["opacity"][:P]), _t(inp["scaling"][:P]), _t(inp["rotation"][:P]), _t(inp["xi"][:P]),
               NOISE_SCALE)
    torch.cuda.synchronize()
    want = inp["xyz"][:P].astype(np.float64) + delta[:P]
    got = xyz.cpu().numpy().astype(np.float64)
    print(f"P = {P}: max |xyz - reference| {np.abs(got - want).max():.3g}, max |delta| {np.abs(delta[:P]).max():.3g}")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)


@pytest.mark.parametrize("P", (65, 4099))
def test_noise_leaves_opaque_gaussians_bitwise_unchanged(P):
    """o >= 0.5: the gate is below exp(-49.5), the displacement far below half an ulp of |xyz| >= 0.01."""
    from gaussian_splatting_amd import mcmc

    rng = np.random.default_rng(1)
    xyz = (rng.uniform(0.01, 3, (P, 3)) * rng.choice([-1.0, 1.0], (P, 3))).astype(np.float32)
    op = rng.uniform(0, 9, (P, 1)).astype(np.float32)
    op[0] = 0.0
    got = _t(xyz)
    mcmc.noise(got, _t(op), _t(rng.uniform(-5, -2.5, (P, 3)).astype(np.float32)),
               _t(rng.standard_normal((P, 4)).astype(np.float32)), _t(rng.standard_normal((P, 3)).astype(np.float32)),
               NOISE_SCALE)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), xyz.view(np.uint32))


def test_inject_noise_is_the_low_level_call_on_the_generators_draw():
    from gaussian_splatting_amd import mcmc

    P = 300
    rng = np.random.default_rng(2)
    params = TD._rand_params(P, rng)
    params["opacity"] = rng.uniform(-9, -3, (P, 1)).astype(np.float32)
    model = TD._Model(params, None, np.zeros(P, np.float32), np.zeros(P, np.float32), _dev())
    before = model._xyz.detach().clone()
    param = model._xyz
    mcmc.inject_noise(model, 1.6e-4, generator=torch.Generator(device=_dev()).manual_seed(9))
    xi = torch.randn((P, 3), device=_dev(), generator=torch.Generator(device=_dev()).manual_seed(9))
    want = before.clone()
    mcmc.noise(want, model._opacity.data, model._scaling.data, model._rotation.data, xi, 5e5 * 1.6e-4)
    torch.cuda.synchronize()
    assert model._xyz is param
    assert torch.equal(model._xyz.detach(), want)
    assert float((want - before).abs().max()) > 1e-4  # (it moved)


# ---- relocation -------------------------------------------------------------------------
def _reloc_inputs(P, rng):
    o = rng.uniform(0.006, 0.99, P)
    k = min(P, len(SPECIAL_OPACITIES))
    o[:k] = SPECIAL_OPACITIES[:k]
    op = MR.logit(o).astype(np.float32).reshape(P, 1)
    sc = rng.uniform(-6, -2, (P, 3)).astype(np.float32)
    return op, sc


def _reloc_case(name):
    rng = np.random.default_rng(3)
    if name == "all_clamped":  # P = 3, n = 200: every count exceeds the clamp
        op, sc = _reloc_inputs(3, rng)  # sources 0.0051, 0.3, 0.9 ...
        sampled = np.concatenate([np.arange(3), rng.integers(0, 3, 197)])
        extra = _reloc_inputs(4, rng)  # ... and 0.3, 0.9, 0.999999 in a second call of the same shape (below)
        return op, sc, sampled, extra
    if name == "with_replacement":  # P = 300, n = 40
        op, sc = _reloc_inputs(300, rng)
        sampled = rng.integers(0, 300, 40)
        sampled[:7] = [0, 1, 2, 3, 3, 3, 0]
        return op, sc, sampled, None
    op, sc = _reloc_inputs(4, rng)  # n = 1
    return op, sc, np.array([3]), None


def _check_relocation(op, sc, sampled, **kw):
    from gaussian_splatting_amd import mcmc

    new_op, new_sc, ratio = mcmc.relocation(_t(op), _t(sc), _t(sampled, torch.int64), **kw)
    torch.cuda.synchronize()
    ref_op, ref_sc, ref_ratio = MR.relocation(op, sc, sampled, **kw)
    n = len(sampled)
    assert new_op.shape == (n, 1) and new_sc.shape == (n, 3) and ratio.shape == (n,)
    assert new_op.dtype == torch.float32 and new_sc.dtype == torch.float32 and ratio.dtype == torch.int32
    np.testing.assert_array_equal(ratio.cpu().numpy(), ref_ratio)
    got_op, got_sc = new_op.cpu().numpy(), new_sc.cpu().numpy()
    want_op, want_sc = ref_op.astype(np.float32), ref_sc.astype(np.float32)
    print(f"n = {n}: max |opacity - ref| / |ref| {np.abs((got_op - want_op) / want_op).max():.3g}, "
          f"max |scaling - ref| {np.abs(got_sc - want_sc).max():.3g}, ratios {ref_ratio.min()}..{ref_ratio.max()}")
    np.testing.assert_allclose(got_op, want_op, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got_sc, want_sc, rtol=1e-6, atol=1e-6)
    return ref_ratio


@pytest.mark.parametrize("name", ["all_clamped", "with_replacement", "single"])
def test_relocation_matches_reference(name):
    op, sc, sampled, extra = _reloc_case(name)
    ratio = _check_relocation(op, sc, sampled)
    if name == "all_clamped":
        assert (ratio == 51).all()
        op2, sc2 = extra
        _check_relocation(op2[1:], sc2[1:], sampled)  # sources 0.3, 0.9, 0.999999, the same 200 samples
    elif name == "with_replacement":
        assert ratio.min() == 2 and ratio[3] >= 4 and len(set(ratio)) >= 3
    else:
        assert list(ratio) == [2]


def test_relocation_other_clamp_and_floor():
    """n_max below the counts, and a floor (min_opacity) above x: both arguments reach the kernel."""
    op, sc, sampled, _ = _reloc_case("with_replacement")
    ratio = _check_relocation(op, sc, sampled, n_max=2, min_opacity=0.2)
    assert (ratio == 2).all()


# ---- row surgery ------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_model_rows(got_params, got_moments, want_params, want_moments, exact=True):
    for k, want in want_params.items():
        got = got_params[k]
        assert got.shape == want.shape, (k, got.shape, want.shape)
        if exact or k not in ("opacity", "scaling"):
            np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=k)
        else:
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6, err_msg=k)
        if k in want_moments:
            np.testing.assert_array_equal(_bits(got_moments[k][0]), _bits(want_moments[k][0]), err_msg=k + " exp_avg")
            np.testing.assert_array_equal(_bits(got_moments[k][1]), _bits(want_moments[k][1]), err_msg=k + " exp_avg_sq")
        else:
            assert k not in got_moments


def test_apply_relocation_low_level():
    """P = 70, 9 destinations, groups of widths 3, 3, 45, 1, 3 and 4, f_dc without Adam state."""
    from gaussian_splatting_amd import mcmc

    P, n = 70, 9
    rng = np.random.default_rng(4)
    params = TD._rand_params(P, rng)
    params["opacity"] = MR.logit(rng.uniform(0.006, 0.99, (P, 1))).astype(np.float32)
    moments = TD._rand_moments(P, rng)
    del moments["f_dc"]
    rows = rng.permutation(P)
    dest, pool = rows[:n], rows[n:]
    sampled = rng.choice(pool[:4], n)  # few sources: duplicates
    assert len(set(sampled)) < n and not set(sampled) & set(dest)
    d_sampled, d_dest = _t(sampled, torch.int64), _t(dest, torch.int64)
    new_op, new_sc, _ = mcmc.relocation(_t(params["opacity"]), _t(params["scaling"]), d_sampled)
    dev_p = {k: _t(v) for k, v in params.items()}
    dev_m = {k: (_t(m), _t(v)) for k, (m, v) in moments.items()}
    roles = {name: role for name, _, role in mcmc.GROUPS}
    assert [int(np.prod(params[k].shape[1:])) for k in TD.ATTR] == [3, 3, 45, 1, 3, 4]
    mcmc.apply_relocation([(dev_p[k],) + dev_m.get(k, (None, None)) + (roles[k],) for k in TD.ATTR], d_sampled, d_dest,
                          new_op, new_sc)
    torch.cuda.synchronize()
    step2_op, step2_sc = new_op.cpu().numpy(), new_sc.cpu().numpy()
    want_p, want_m = MR.apply(params, moments, sampled, dest, step2_op, step2_sc)
    got_p = {k: v.cpu().numpy() for k, v in dev_p.items()}
    got_m = {k: (m.cpu().numpy(), v.cpu().numpy()) for k, (m, v) in dev_m.items()}
    _assert_model_rows(got_p, got_m, want_p, want_m)
    # spelled out: the step-2 values at both ends, zero moments at the sources only, the rest untouched
    for idx in (sampled, dest):
        np.testing.assert_array_equal(_bits(got_p["opacity"][idx]), _bits(step2_op))
        np.testing.assert_array_equal(_bits(got_p["scaling"][idx]), _bits(step2_sc))
    np.testing.assert_array_equal(_bits(got_p["f_rest"][dest]), _bits(params["f_rest"][sampled]))
    others = np.setdiff1d(np.arange(P), np.concatenate([sampled, dest]))
    for k in params:
        np.testing.assert_array_equal(_bits(got_p[k][others]), _bits(params[k][others]), err_msg=k)
    not_src = np.setdiff1d(np.arange(P), sampled)
    for k, (m, v) in moments.items():
        assert not got_m[k][0][sampled].any() and not got_m[k][1][sampled].any()
        np.testing.assert_array_equal(_bits(got_m[k][0][not_src]), _bits(m[not_src]), err_msg=k)
        np.testing.assert_array_equal(_bits(got_m[k][1][not_src]), _bits(v[not_src]), err_msg=k)


# ---- the model's methods ----------------------------------------------------------------
def _model(P, seed, with_moments=True, opacity=None):
    rng = np.random.default_rng(seed)
    params = TD._rand_params(P, rng)
    if opacity is not None:
        params["opacity"] = opacity(rng).astype(np.float32).reshape(P, 1)
    moments = TD._rand_moments(P, rng) if with_moments else None
    model = TD._Model(params, moments, np.ones(P, np.float32), np.ones(P, np.float32), _dev())
    return model, params, moments


def _model_arrays(model, moments):
    got_p = {k: getattr(model, a).detach().cpu().numpy() for k, a in TD.ATTR.items()}
    got_m = {}
    for i, (k, a) in enumerate(TD.ATTR.items()):
        prm = getattr(model, a)
        assert model.optimizer.param_groups[i]["params"][0] is prm, k
        st = model.optimizer.state.get(prm)
        if moments is None:
            assert st is None or "exp_avg" not in st
        else:
            assert float(st["step"]) == 7.0  # (the other state entries stay with the parameter)
            got_m[k] = (st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy())
    return got_p, got_m


@pytest.mark.parametrize("with_moments", [True, False])
def test_relocate_gs_matches_reference(with_moments):
    from gaussian_splatting_amd import mcmc

    P = 200

    def opacity(rng):
        raw = rng.normal(0.0, 3.0, P)
        raw[rng.permutation(P)[:12]] = rng.uniform(-9, -6, 12)  # surely dead
        return raw

    model, params, moments = _model(P, 5, with_moments, opacity)
    objs = [getattr(model, a) for a in TD.ATTR.values()]
    dead_idx, sampled_idx = mcmc.relocate_gs(model, generator=torch.Generator(device=_dev()).manual_seed(11))
    torch.cuda.synchronize()
    dead, sampled = dead_idx.cpu().numpy(), sampled_idx.cpu().numpy()
    np.testing.assert_array_equal(dead, np.nonzero(MR.sigmoid(params["opacity"][:, 0]) <= 0.005)[0])
    assert 12 <= len(dead) < P // 4 and len(sampled) == len(dead) and not set(sampled) & set(dead)
    assert sampled_idx.dtype == torch.int64 and dead_idx.dtype == torch.int64
    assert all(getattr(model, a) is o for a, o in zip(TD.ATTR.values(), objs))  # edited in place
    ref_op, ref_sc, _ = MR.relocation(params["opacity"], params["scaling"], sampled)
    want_p, want_m = MR.apply(params, moments or {}, sampled, dead, ref_op, ref_sc)
    got_p, got_m = _model_arrays(model, moments)
    _assert_model_rows(got_p, got_m, want_p, want_m, exact=False)
    assert float(torch.sigmoid(model._opacity.detach()).min()) >= 0.005 - 1e-7  # nobody is dead afterwards
    assert bool(model.xyz_gradient_accum.all())  # (the statistics are not touched)


def test_relocate_gs_without_dead_gaussians_changes_nothing():
    from gaussian_splatting_amd import mcmc

    model, params, moments = _model(150, 6, True, lambda rng: rng.uniform(-2, 6, 150))
    objs = [getattr(model, a) for a in TD.ATTR.values()]
    dead_idx, sampled_idx = mcmc.relocate_gs(model, generator=torch.Generator(device=_dev()).manual_seed(1))
    assert dead_idx.numel() == 0 and sampled_idx.numel() == 0
    assert all(getattr(model, a) is o for a, o in zip(TD.ATTR.values(), objs))
    got_p, got_m = _model_arrays(model, moments)
    _assert_model_rows(got_p, got_m, params, moments)
    # nor with nobody alive: no source to draw from
    model, params, moments = _model(40, 7, True, lambda rng: rng.uniform(-12, -8, 40))
    dead_idx, sampled_idx = mcmc.relocate_gs(model)
    assert dead_idx.numel() == 40 and sampled_idx.numel() == 0
    got_p, got_m = _model_arrays(model, moments)
    _assert_model_rows(got_p, got_m, params, moments)


@pytest.mark.parametrize("with_moments", [True, False])
def test_add_new_gs_appends_rows(with_moments):
    from gaussian_splatting_amd import mcmc

    P, n = 130, 6  # min(1000, int(1.05 * 130)) - 130
    model, params, moments = _model(P, 8, with_moments)
    objs = [getattr(model, a) for a in TD.ATTR.values()]
    sampled_idx = mcmc.add_new_gs(model, cap_max=1000, generator=torch.Generator(device=_dev()).manual_seed(13))
    torch.cuda.synchronize()
    sampled = sampled_idx.cpu().numpy()
    assert sampled.shape == (n,) and sampled.min() >= 0 and sampled.max() < P
    assert all(getattr(model, a) is not o for a, o in zip(TD.ATTR.values(), objs))  # replaced in the optimizer
    grow = lambda a: np.concatenate([a, np.zeros((n,) + a.shape[1:], np.float32)])  # noqa: E731
    ref_op, ref_sc, _ = MR.relocation(params["opacity"], params["scaling"], sampled)
    want_p, want_m = MR.apply({k: grow(v) for k, v in params.items()},
                              {k: (grow(m), grow(v)) for k, (m, v) in (moments or {}).items()}, sampled,
                              np.arange(P, P + n), ref_op, ref_sc)
    got_p, got_m = _model_arrays(model, moments)
    assert got_p["xyz"].shape == (P + n, 3)
    _assert_model_rows(got_p, got_m, want_p, want_m, exact=False)
    for k in got_m:
        assert not got_m[k][0][P:].any() and not got_m[k][1][P:].any()  # zero moments on the new rows
    assert all(getattr(model, a).requires_grad for a in TD.ATTR.values())
    assert model.xyz_gradient_accum.shape == (P + n, 1) and not model.xyz_gradient_accum.any()
    assert model.denom.shape == (P + n, 1) and not model.denom.any()
    assert model.max_radii2D.shape == (P + n,) and not model.max_radii2D.any()


def test_add_new_gs_at_the_cap_replaces_nothing():
    from gaussian_splatting_amd import mcmc

    model, params, moments = _model(130, 9)
    objs = [getattr(model, a) for a in TD.ATTR.values()]
    sampled_idx = mcmc.add_new_gs(model, cap_max=100)
    assert sampled_idx.numel() == 0 and sampled_idx.dtype == torch.int64
    assert all(getattr(model, a) is o for a, o in zip(TD.ATTR.values(), objs))
    got_p, got_m = _model_arrays(model, moments)
    _assert_model_rows(got_p, got_m, params, moments)
    assert model.xyz_gradient_accum.shape == (130, 1) and bool(model.xyz_gradient_accum.all())
