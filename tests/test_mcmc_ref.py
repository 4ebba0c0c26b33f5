"""CPU checks of 3DGS-MCMC density control (include/gsr_mcmc.h, gaussian_splatting_amd/mcmc.py): known answers of the
float64 reference tests/mcmc_ref.py that tests/test_gpu_mcmc.py holds the kernels to, the new C ABI symbols, and the
argument checks of the Python layer (CPU tensors, dtypes, shapes, indices), which raise before any device work.
"""
import math
import os

import numpy as np
import pytest
import torch

from tests import mcmc_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"gsr_mcmc_noise": 8, "gsr_mcmc_scratch_bytes": 1, "gsr_mcmc_relocation": 12, "gsr_mcmc_apply": 9}


# ---- the reference's known answers ----------------------------------------------------
@pytest.mark.parametrize("o", [0.0051, 0.3, 0.9, 0.999999])
def test_one_copy_changes_nothing(o):
    assert MR.relocate_x(o, 1) == pytest.approx(o, rel=1e-15)
    assert MR.scale_factor(o, 1) == pytest.approx(1.0, rel=1e-15)
    assert MR.denominator(0.25, 1) == 0.25  # the sum's single term, exactly


@pytest.mark.parametrize("o,factor", [(0.3, 0.97461335), (0.9, 0.86793785), (0.5, 0.95215195)])
def test_two_copies(o, factor):
    x = MR.relocate_x(o, 2)
    assert x == pytest.approx(1.0 - math.sqrt(1.0 - o), rel=1e-14)
    closed = o / (2.0 * x - x * x / math.sqrt(2.0))
    assert MR.scale_factor(o, 2) == pytest.approx(closed, rel=1e-14)
    assert closed == pytest.approx(factor, abs=5e-9)


def test_fifty_one_copies():
    assert MR.scale_factor(0.9, 51) == pytest.approx(0.75784573, abs=5e-9)


def test_single_sum_equals_the_double_sum():
    """The kernel's form, sum_k C(N, k+1) (-1)^k x^(k+1) / sqrt(k+1) (hockey-stick identity)."""
    worst = 0.0
    for N in (1, 2, 3, 7, 20, 51):
        for o in (0.0051, 0.006, 0.3, 0.9, 0.999999, 1.0 - 2.0 ** -24):
            x = MR.relocate_x(o, N)
            single = sum(math.comb(N, k + 1) * (-1.0) ** k * x ** (k + 1) / math.sqrt(k + 1) for k in range(N))
            worst = max(worst, abs(single - MR.denominator(x, N)) / MR.denominator(x, N))
    print(f"single against double sum: largest relative difference {worst:.2e}")
    assert worst <= 1e-12


def test_counts_above_the_clamp():
    sampled = np.array([2] * 60 + [0] * 50 + [1] * 3 + [4], np.int64)
    r = MR.ratios(sampled)
    assert r.dtype == np.int32
    np.testing.assert_array_equal(r, [51] * 60 + [51] * 50 + [4] * 3 + [2])
    np.testing.assert_array_equal(MR.ratios(sampled, n_max=3), [3] * 113 + [2])
    op = np.full((5, 1), MR.logit(0.9))
    sc = np.zeros((5, 3))
    new_op, new_sc, ratio = MR.relocation(op, sc, sampled)
    assert new_op.shape == (114, 1) and new_sc.shape == (114, 3)
    np.testing.assert_allclose(np.exp(new_sc[:110]), 0.75784573, rtol=0, atol=5e-9)  # N = 51 at o = 0.9
    np.testing.assert_allclose(MR.sigmoid(new_op[:110, 0]), MR.relocate_x(MR.sigmoid(op[0, 0]), 51), rtol=1e-12)


def test_clamp_on_x_at_both_ends():
    # low: o barely alive and 51 copies -> x ~ 1e-4 < min_opacity
    op = np.array([[MR.logit(0.0051)], [40.0]])
    sc = np.zeros((2, 3))
    new_op, _, ratio = MR.relocation(op, sc, np.zeros(60, np.int64))
    assert ratio[0] == 51 and MR.relocate_x(0.0051, 51) < 0.005
    np.testing.assert_allclose(new_op, MR.logit(0.005), rtol=1e-15)
    np.testing.assert_allclose(MR.relocation(op, sc, np.zeros(60, np.int64), min_opacity=0.01)[0], MR.logit(0.01))
    # high: sigmoid(40) rounds to 1 in float64, x = 1 -> 1 - FLT_EPSILON
    assert float(MR.sigmoid(40.0)) == 1.0
    new_op, _, ratio = MR.relocation(op, sc, np.array([1], np.int64))
    assert ratio[0] == 2
    np.testing.assert_allclose(new_op, MR.logit(1.0 - 2.0 ** -23), rtol=1e-15)
    assert np.isfinite(new_op).all()


def test_gate_equals_the_papers_form():
    o = np.concatenate([np.linspace(0.0, 1.0, 4001), MR.sigmoid(np.linspace(-12.0, 12.0, 997))])
    assert np.abs(MR.gate(o) - MR.gate_paper(o)).max() <= 1e-12
    assert MR.gate(0.005) == 0.5 and MR.gate(0.0) > 0.62 and MR.gate(0.5) < 1e-21


def test_noise_reference_on_an_axis_aligned_gaussian():
    """Identity rotation: Sigma = diag(s^2), so delta = s^2 * xi * gate * noise_scale per axis."""
    op = np.array([MR.logit(0.005)])
    sc = np.log(np.array([[0.1, 0.2, 0.3]]))
    d = MR.noise_delta(op, sc, np.array([[2.0, 0.0, 0.0, 0.0]]), np.array([[1.0, -1.0, 2.0]]), 10.0)
    np.testing.assert_allclose(d, [[0.01 * 5.0, -0.04 * 5.0, 0.09 * 10.0]], rtol=1e-12)
    R = MR.build_rotation(np.random.default_rng(0).standard_normal((50, 4)))
    np.testing.assert_allclose(R @ R.transpose(0, 2, 1), np.tile(np.eye(3), (50, 1, 1)), atol=1e-14)


# ---- the C ABI --------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    from gaussian_splatting_amd import _lib, build

    names = _lib.header_symbols(os.path.join(ROOT, "include", "gsr_mcmc.h"))
    assert sorted(names) == sorted(SYMBOLS)
    for sym, nargs in SYMBOLS.items():
        assert sym in _lib.SIGNATURES, sym
        assert len(_lib.SIGNATURES[sym][1]) == nargs, sym
    assert "gsr_mcmc.h" in build.ABI_HEADERS and "mcmc.hip" in build.SOURCES
    assert os.path.join(ROOT, "include", "gsr_mcmc.h") in _lib.HEADERS
    lib = _lib.load()
    for sym in SYMBOLS:
        assert getattr(lib, sym) is not None, sym
    assert lib.gsr_mcmc_scratch_bytes(0) == 0 and lib.gsr_mcmc_scratch_bytes(1000) >= 4000


def test_group_struct_mirror_has_the_headers_layout(tmp_path):
    """_lib.McmcGroup against offsetof / sizeof of gsr_mcmc_group as a C compiler lays the header out (the header is
    plain C: it compiles as C11 with -Werror)."""
    import ctypes
    import subprocess

    from gaussian_splatting_amd import _lib, build

    names = [f for f, _ in _lib.McmcGroup._fields_]
    assert names == ["data", "exp_avg", "exp_avg_sq", "width", "role"]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "gsr_mcmc.h"', "int main(void) {",
             '    printf("%zu\\n", sizeof(gsr_mcmc_group));']
    lines += [f'    printf("%zu %zu\\n", offsetof(gsr_mcmc_group, {f}), sizeof(((gsr_mcmc_group*)0)->{f}));' for f in names]
    lines += ["    return 0;", "}", ""]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run([build.HIPCC, "-x", "c", "-std=c11", "-Wall", "-Werror", "-I", _lib.INCLUDE_DIR, str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert ctypes.sizeof(_lib.McmcGroup) == int(out[0])
    for f, line in zip(names, out[1:]):
        d = getattr(_lib.McmcGroup, f)
        assert [d.offset, d.size] == [int(v) for v in line.split()], f


def test_entry_points_check_their_arguments_before_any_launch():
    """No HIP device is needed for the refusals, nor for P == 0 / n == 0, which return OK without a launch."""
    from gaussian_splatting_amd import _lib

    lib = _lib.load()
    assert lib.gsr_mcmc_noise(0, None, None, None, None, None, 1.0, None) == 0
    assert lib.gsr_mcmc_relocation(0, 5, None, None, None, 51, 0.005, None, None, None, None, None) == 0
    assert lib.gsr_mcmc_relocation(5, 0, None, None, None, 51, 0.005, None, None, None, None, None) == 0
    assert lib.gsr_mcmc_apply(5, 0, None, None, None, None, None, 0, None) == 0
    assert lib.gsr_mcmc_noise(4, None, None, None, None, None, 1.0, None) == 1
    assert b"null" in lib.gsr_last_error()
    assert lib.gsr_mcmc_noise(4, 16, 16, 16, 20, 16, 1.0, None) == 1  # (never dereferenced: refused on alignment)
    assert b"aligned" in lib.gsr_last_error()
    assert lib.gsr_mcmc_relocation(5, 5, None, None, None, 52, 0.005, None, None, None, None, None) == 1
    assert b"n_max" in lib.gsr_last_error()
    g = (_lib.McmcGroup * 1)(_lib.McmcGroup(16, None, None, 3, _lib_role("OPACITY")))
    assert lib.gsr_mcmc_apply(5, 2, 16, 16, 16, 16, g, 1, None) == 1
    assert b"width 1" in lib.gsr_last_error()
    assert lib.gsr_mcmc_apply(5, 2, 16, 16, 16, 16, g, 9, None) == 1


def _lib_role(name):
    from gaussian_splatting_amd import mcmc

    return getattr(mcmc, name)


# ---- the Python layer's refusals --------------------------------------------------------
def test_cpu_tensors_raise():
    from gaussian_splatting_amd import mcmc

    z = torch.zeros
    idx = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        mcmc.noise(z(4, 3), z(4, 1), z(4, 3), z(4, 4), z(4, 3), 1.0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        mcmc.relocation(z(4, 1), z(4, 3), idx)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        mcmc.apply_relocation([(z(4, 3), None, None, mcmc.COPY)], idx, idx + 2, z(2, 1), z(2, 3))
    model = type("M", (), {})()
    model._xyz = model._opacity = z(4, 3)
    for call in (lambda: mcmc.inject_noise(model, 1e-4), lambda: mcmc.relocate_gs(model),
                 lambda: mcmc.add_new_gs(model, 100)):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()


def test_wrong_dtypes_and_shapes_raise(monkeypatch):
    """The dtype and shape checks come after the device check; with that one stubbed they are reached on host
    tensors, and each raises before the library is called."""
    from gaussian_splatting_amd import mcmc

    monkeypatch.setattr(mcmc, "_dev_check", lambda t, name: None)
    monkeypatch.setattr(mcmc._lib, "load", lambda: pytest.fail("the library was called"))
    z = torch.zeros
    idx = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="float32"):
        mcmc.noise(z(4, 3, dtype=torch.float64), z(4, 1), z(4, 3), z(4, 4), z(4, 3), 1.0)
    with pytest.raises(RuntimeError, match="shape"):
        mcmc.noise(z(4, 3), z(4, 1), z(4, 3), z(4, 3), z(4, 3), 1.0)  # rotation [P, 3]
    with pytest.raises(RuntimeError, match="shape"):
        mcmc.noise(z(4, 3), z(4, 1), z(5, 3), z(4, 4), z(4, 3), 1.0)  # another point count
    with pytest.raises(RuntimeError, match="rows"):
        mcmc.noise(z(4, 3), z(5, 1), z(4, 3), z(4, 4), z(4, 3), 1.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        mcmc.noise(z(4, 6)[:, :3], z(4, 1), z(4, 3), z(4, 4), z(4, 3), 1.0)
    with pytest.raises(RuntimeError, match="int64"):
        mcmc.relocation(z(4, 1), z(4, 3), idx.int())
    with pytest.raises(RuntimeError, match="int64"):
        mcmc.relocation(z(4, 1), z(4, 3), idx.reshape(2, 1))
    with pytest.raises(RuntimeError, match="shape"):
        mcmc.relocation(z(4, 1), z(4, 2), idx)
    with pytest.raises(ValueError, match="n_max"):
        mcmc.relocation(z(4, 1), z(4, 3), idx, n_max=52)
    with pytest.raises(RuntimeError, match=r"outside \[0, 4\)"):
        mcmc.relocation(z(4, 1), z(4, 3), idx + 4)
    grp = [(z(4, 3), None, None, mcmc.COPY)]
    with pytest.raises(RuntimeError, match="shape"):
        mcmc.apply_relocation(grp, idx, idx + 2, z(2), z(2, 3))
    with pytest.raises(RuntimeError, match="both"):
        mcmc.apply_relocation([(z(4, 3), z(4, 3), None, mcmc.COPY)], idx, idx + 2, z(2, 1), z(2, 3))
    with pytest.raises(RuntimeError, match="shape"):
        mcmc.apply_relocation([(z(4, 3), z(4, 2), z(4, 3), mcmc.COPY)], idx, idx + 2, z(2, 1), z(2, 3))
    with pytest.raises(RuntimeError, match="role"):
        mcmc.apply_relocation([(z(4, 3), None, None, mcmc.OPACITY)], idx, idx + 2, z(2, 1), z(2, 3))
    with pytest.raises(RuntimeError, match="overlap"):
        mcmc.apply_relocation(grp, idx, torch.tensor([0, 1]), z(2, 1), z(2, 3))


def test_index_checks_raise():
    from gaussian_splatting_amd import mcmc

    t = lambda *v: torch.tensor(v, dtype=torch.int64)  # noqa: E731
    mcmc.check_indices(t(0, 0, 3), 4)
    mcmc.check_indices(t(0, 0, 3), 6, t(1, 2, 5))
    mcmc.check_indices(t(), 4, t())
    for bad in (t(0, 4), t(-1, 0)):
        with pytest.raises(RuntimeError, match=r"sampled: index outside \[0, 4\)"):
            mcmc.check_indices(bad, 4)
        with pytest.raises(RuntimeError, match=r"dest: index outside \[0, 4\)"):
            mcmc.check_indices(t(1, 1), 4, bad)
    with pytest.raises(RuntimeError, match="overlap"):
        mcmc.check_indices(t(0, 2, 2), 6, t(1, 3, 2))
    with pytest.raises(RuntimeError, match="duplicate"):
        mcmc.check_indices(t(0, 0), 6, t(3, 3))
    with pytest.raises(RuntimeError, match="entries"):
        mcmc.check_indices(t(0, 0), 6, t(3))
    with pytest.raises(RuntimeError, match="int64"):
        mcmc.check_indices(torch.tensor([0, 1], dtype=torch.int32), 6)


def test_sample_sources_by_inverse_cdf_above_the_multinomial_limit():
    """Beyond 2^24 categories torch.multinomial refuses; the inverse CDF path (forced here by a small limit) draws in
    proportion to the weights, never a category of weight zero, and is reproducible from the generator."""
    from gaussian_splatting_amd import mcmc

    assert mcmc.MULTINOMIAL_MAX == 1 << 24
    w = torch.tensor([0.0, 1.0, 0.0, 3.0, 0.0, 4.0, 0.0])
    g = torch.Generator().manual_seed(3)
    idx = mcmc.sample_sources(w, 40000, g, multinomial_max=4)
    assert idx.dtype == torch.int64 and idx.shape == (40000,)
    freq = torch.bincount(idx, minlength=7).double() / 40000
    assert freq[[0, 2, 4, 6]].sum() == 0
    np.testing.assert_allclose(freq[[1, 3, 5]].numpy(), [0.125, 0.375, 0.5], atol=0.01)  # (4 sigma = 0.01)
    again = mcmc.sample_sources(w, 40000, torch.Generator().manual_seed(3), multinomial_max=4)
    assert torch.equal(idx, again)
    # at or below the limit it is torch.multinomial's own draw
    a = mcmc.sample_sources(w, 50, torch.Generator().manual_seed(5))
    b = torch.multinomial(w, 50, replacement=True, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a, b)


def test_groups_and_install():
    from gaussian_splatting_amd import densify, mcmc

    assert [(n, a) for n, a, _ in mcmc.GROUPS] == [(n, a) for n, a, _ in densify.GROUPS]
    roles = {n: r for n, _, r in mcmc.GROUPS}
    assert roles == {"xyz": mcmc.COPY, "f_dc": mcmc.COPY, "f_rest": mcmc.COPY, "opacity": mcmc.OPACITY,
                     "scaling": mcmc.SCALING, "rotation": mcmc.COPY}
    cls = type("GaussianModel", (), {})
    mcmc.install(cls)
    assert cls.inject_noise is mcmc.inject_noise and cls.relocate_gs is mcmc.relocate_gs
    assert cls.add_new_gs is mcmc.add_new_gs
    text = open(os.path.join(ROOT, "include", "gsr_mcmc.h")).read()
    for name, val in (("GSR_MCMC_COPY", mcmc.COPY), ("GSR_MCMC_OPACITY", mcmc.OPACITY),
                      ("GSR_MCMC_SCALING", mcmc.SCALING), ("GSR_MCMC_N_MAX", mcmc.N_MAX)):
        assert f"#define {name} {val}" in text, name
