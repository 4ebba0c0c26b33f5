"""3DGS-MCMC density control on MI355X ("3D Gaussian Splatting as Markov Chain Monte Carlo", Kheradmand et al.
2024) over the HIP kernels of ``csrc/mcmc.hip`` (C ABI: include/gsr_mcmc.h, which states every formula).

The strategy keeps a fixed budget of Gaussians instead of cloning, splitting and pruning (``densify.py``):

* ``inject_noise``  every iteration, after the optimizer step: ``xyz += Sigma @ (xi * gate(o) * noise_lr * xyz_lr)``,
  one fused kernel in place;
* ``relocate_gs``   every 100 iterations or so: each dead Gaussian (``sigmoid(_opacity) <= min_opacity``) becomes a copy of
  a live one drawn with probability proportional to its opacity; the source and its copies share the opacity and
  scale of ``relocation``;
* ``add_new_gs``    at the same cadence: the set grows by 5 % up to ``cap_max``, the new rows made the same way.

The reference has none of this.  Like ``densify.py`` the functions take the model first and touch the same attributes
(``_xyz``, ``_features_dc``, ``_features_rest``, ``_opacity``, ``_scaling``, ``_rotation``, ``optimizer``,
``xyz_gradient_accum``, ``denom``, ``max_radii2D``), so ``install(GaussianModel)`` binds them as methods.  The paper's
``opacity_reg`` / ``scale_reg`` L1 terms are plain torch in the training loop.

Random draws are made here with torch (``torch.randn``, ``torch.multinomial``) from the caller's generator; the
kernels do the arithmetic and the row surgery.  Optimizer state: ``exp_avg`` and ``exp_avg_sq`` become zero at every
sampled source; relocated rows keep the moments they hold (the published behaviour); rows added by ``add_new_gs`` start
with zero moments.

Replicas: with ``torch.distributed`` initialised (world > 1) rank 0's sampled indices are broadcast, as
``densify_and_prune`` broadcasts its samples.  The per-step noise is NOT broadcast: ranks pass identically seeded
generators to ``inject_noise`` (and draw nothing else from them), so every replica adds the same noise.

There is no CPU implementation: CPU tensors raise.
"""
from __future__ import annotations

import ctypes
import math

import torch
import torch.distributed as dist

from . import _lib
from .densify import GROUPS as _DENSIFY_GROUPS
from .densify import _replace_in_optimizer, _stream

__all__ = ["inject_noise", "relocation", "relocate_gs", "add_new_gs", "install", "noise", "apply_relocation",
           "check_indices", "sample_sources", "GROUPS", "N_MAX"]

COPY, OPACITY, SCALING = 0, 1, 2  # GSR_MCMC_COPY / _OPACITY / _SCALING
N_MAX = 51                        # GSR_MCMC_N_MAX
_ROLE = {"opacity": OPACITY, "scaling": SCALING}
# optimizer group name, model attribute, what relocation writes into the group's rows
GROUPS = tuple((name, attr, _ROLE.get(name, COPY)) for name, attr, _ in _DENSIFY_GROUPS)
MULTINOMIAL_MAX = 1 << 24  # torch.multinomial refuses more categories


def _dev_check(t: torch.Tensor, name: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name}: MCMC density control runs on HIP device tensors, got {t.device.type} "
                           "(there is no CPU implementation)")


def _f32(t: torch.Tensor, name: str, shape) -> torch.Tensor:
    """A float32 contiguous device tensor of ``shape`` (-1: any), as it is: the kernels edit in place."""
    _dev_check(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected float32, got {t.dtype}")
    if t.dim() != len(shape) or any(w != -1 and w != g for w, g in zip(shape, t.shape)):
        raise RuntimeError(f"{name}: expected shape {tuple(shape)} (-1: any), got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    return t


def _opacity(t: torch.Tensor, name: str = "opacity_raw") -> torch.Tensor:
    _dev_check(t, name)
    if t.dim() == 2 and t.shape[1] == 1:
        return _f32(t, name, (-1, 1))
    return _f32(t, name, (-1,))


def _index(t: torch.Tensor, name: str) -> torch.Tensor:
    _dev_check(t, name)
    if t.dtype != torch.int64 or t.dim() != 1:
        raise RuntimeError(f"{name}: expected a 1-D int64 tensor, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def check_indices(sampled: torch.Tensor, P: int, dest: torch.Tensor = None) -> None:
    """Raise unless ``sampled`` (and ``dest``) are 1-D int64 indices into [0, P); with ``dest``: of one length,
    ``dest`` without duplicates and disjoint from ``sampled`` (the kernels read rows ``sampled`` while they write
    rows ``dest``).  Plain tensor arithmetic on the indices' device; one host read."""
    for t, name in ((sampled, "sampled"), (dest, "dest")):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1:
            raise RuntimeError(f"{name}: expected a 1-D int64 tensor")
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= P):
            raise RuntimeError(f"{name}: index outside [0, {P})")
    if dest is None:
        return
    if dest.numel() != sampled.numel():
        raise RuntimeError(f"dest has {dest.numel()} entries, sampled {sampled.numel()}")
    hits = torch.zeros(P, dtype=torch.int32, device=dest.device)
    hits.index_add_(0, dest, torch.ones_like(dest, dtype=torch.int32))
    if dest.numel() and int(hits.max()) > 1:
        raise RuntimeError("dest: duplicate destination rows")
    if dest.numel() and bool(hits[sampled].any()):
        raise RuntimeError("sampled and dest overlap: a row cannot be both a source and a destination")


def sample_sources(probs: torch.Tensor, n: int, generator: torch.Generator = None,
                   multinomial_max: int = MULTINOMIAL_MAX) -> torch.Tensor:
    """``n`` int64 indices into ``probs`` [K] drawn with replacement, with probability proportional to ``probs``:
    ``torch.multinomial`` up to ``multinomial_max`` categories (2^24, beyond which it refuses), the inverse CDF
    (``cumsum`` in float64 + ``searchsorted``) above.  With ``torch.distributed`` at world > 1, rank 0's draw."""
    probs = probs.detach().reshape(-1)
    if probs.numel() <= multinomial_max:
        idx = torch.multinomial(probs, n, replacement=True, generator=generator)
    else:
        cdf = torch.cumsum(probs.double(), 0)
        u = torch.rand(n, dtype=torch.float64, device=probs.device, generator=generator) * cdf[-1]
        # right=True: the first index whose cdf exceeds u, so a category of probability 0 is never drawn
        idx = torch.searchsorted(cdf, u, right=True).clamp_(max=probs.numel() - 1)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.broadcast(idx, src=0)  # identical replicas
    return idx


# ---- the three kernels' Python faces --------------------------------------------------
def noise(xyz: torch.Tensor, opacity_raw: torch.Tensor, scaling_raw: torch.Tensor, rotation: torch.Tensor,
          xi: torch.Tensor, noise_scale: float) -> None:
    """In place: ``xyz += Sigma @ (xi * gate * noise_scale)`` (gsr_mcmc_noise).  xyz, scaling_raw, xi: [P, 3];
    opacity_raw: [P] or [P, 1]; rotation: [P, 4]; all float32, contiguous, on one HIP device."""
    _f32(xyz, "xyz", (-1, 3))
    P = xyz.shape[0]
    op = _opacity(opacity_raw)
    if op.shape[0] != P:
        raise RuntimeError(f"opacity_raw: expected {P} rows, got {op.shape[0]}")
    _f32(scaling_raw, "scaling_raw", (P, 3))
    _f32(rotation, "rotation", (P, 4))
    _f32(xi, "xi", (P, 3))
    device = xyz.device
    lib = _lib.load()
    with torch.cuda.device(device):
        rc = lib.gsr_mcmc_noise(P, xyz.data_ptr(), op.data_ptr(), scaling_raw.data_ptr(), rotation.data_ptr(),
                                xi.data_ptr(), float(noise_scale), _stream(device))
    _lib.check(rc, "mcmc noise")


def relocation(opacity_raw: torch.Tensor, scaling_raw: torch.Tensor, sampled: torch.Tensor, n_max: int = N_MAX,
               min_opacity: float = 0.005):
    """The raw opacity and scaling that ``sampled[j]`` and its new copy take (gsr_mcmc_relocation; float64 inside):
    ``(new_opacity_raw [n, 1], new_scaling_raw [n, 3], ratio [n] int32)``, ``ratio[j] = min(count + 1, n_max)`` with
    ``count`` the occurrences of ``sampled[j]`` in ``sampled``."""
    op = _opacity(opacity_raw)
    P = op.shape[0]
    _f32(scaling_raw, "scaling_raw", (P, 3))
    sampled = _index(sampled, "sampled")
    if not 1 <= int(n_max) <= N_MAX:
        raise ValueError(f"relocation: n_max = {n_max} outside 1..{N_MAX}")
    check_indices(sampled, P)
    n = sampled.numel()
    device = op.device
    new_op = torch.empty((n, 1), dtype=torch.float32, device=device)
    new_sc = torch.empty((n, 3), dtype=torch.float32, device=device)
    ratio = torch.empty(n, dtype=torch.int32, device=device)
    lib = _lib.load()
    scratch = torch.empty(int(lib.gsr_mcmc_scratch_bytes(P)), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        rc = lib.gsr_mcmc_relocation(P, n, op.data_ptr(), scaling_raw.data_ptr(), sampled.data_ptr(), int(n_max),
                                     float(min_opacity), scratch.data_ptr(), new_op.data_ptr(), new_sc.data_ptr(),
                                     ratio.data_ptr(), _stream(device))
    _lib.check(rc, "mcmc relocation")
    return new_op, new_sc, ratio


def apply_relocation(groups, sampled: torch.Tensor, dest: torch.Tensor, new_opacity_raw: torch.Tensor,
                     new_scaling_raw: torch.Tensor) -> None:
    """The row surgery, in place (gsr_mcmc_apply).  ``groups``: ``(data, exp_avg, exp_avg_sq, role)`` per parameter
    group, ``data`` [P, ...] float32, the moments of ``data``'s shape or both None, ``role`` COPY / OPACITY / SCALING.
    Row ``dest[j]`` becomes row ``sampled[j]``; OPACITY and SCALING groups take ``new_opacity_raw[j]`` /
    ``new_scaling_raw[j]`` at both; moments become zero at ``sampled``."""
    groups = list(groups)
    if not groups:
        return
    P = groups[0][0].shape[0]
    sampled, dest = _index(sampled, "sampled"), _index(dest, "dest")
    n = sampled.numel()
    new_op = _f32(new_opacity_raw, "new_opacity_raw", (n, 1))
    new_sc = _f32(new_scaling_raw, "new_scaling_raw", (n, 3))
    packed = []
    for k, (data, m, v, role) in enumerate(groups):
        _dev_check(data, f"group {k}")
        _f32(data, f"group {k}", (P,) + (-1,) * (data.dim() - 1))
        if (m is None) != (v is None):
            raise RuntimeError(f"group {k}: exp_avg and exp_avg_sq must both be given or both be None")
        for t, name in ((m, "exp_avg"), (v, "exp_avg_sq")):
            if t is not None:
                _f32(t, f"group {k} {name}", tuple(data.shape))
        width = int(math.prod(data.shape[1:]))
        if (role == OPACITY and width != 1) or (role == SCALING and width != 3) or role not in (COPY, OPACITY, SCALING):
            raise RuntimeError(f"group {k}: role {role} with {width} floats per row")
        packed.append(_lib.McmcGroup(data.data_ptr(), m.data_ptr() if m is not None else None,
                                     v.data_ptr() if v is not None else None, width, int(role)))
    check_indices(sampled, P, dest)
    if n == 0:
        return
    device = groups[0][0].device
    arr = (_lib.McmcGroup * len(packed))(*packed)
    with torch.cuda.device(device):
        rc = _lib.load().gsr_mcmc_apply(P, n, sampled.data_ptr(), dest.data_ptr(), new_op.data_ptr(), new_sc.data_ptr(),
                                        arr, len(packed), _stream(device))
    _lib.check(rc, "mcmc apply")


# ---- the model's methods ----------------------------------------------------------------
def _model_groups(model, what: str):
    names = {g["name"] for g in model.optimizer.param_groups}
    if names != {n for n, _, _ in GROUPS}:
        raise RuntimeError(f"{what}: optimizer groups {sorted(names)}, expected the six of "
                           "GaussianModel.training_setup")
    state = {g["name"]: model.optimizer.state.get(g["params"][0], None) for g in model.optimizer.param_groups}
    out = []
    for name, attr, role in GROUPS:
        st = state[name]
        m = v = None
        if st is not None and "exp_avg" in st:
            m, v = st["exp_avg"], st["exp_avg_sq"]
        out.append((name, attr, role, getattr(model, attr), m, v))
    return out


@torch.no_grad()
def inject_noise(model, xyz_lr: float, noise_lr: float = 5e5, generator: torch.Generator = None) -> None:
    """The paper's position noise, once per iteration after the optimizer step: ``xi = torch.randn(P, 3)`` from
    ``generator``, then ``noise(model._xyz, ..., noise_lr * xyz_lr)`` in place.  ``xyz_lr`` is the xyz group's
    current (scheduled) learning rate.  Not broadcast between replicas: pass identically seeded generators."""
    xyz = model._xyz
    _dev_check(xyz, "_xyz")
    xi = torch.randn(xyz.shape, dtype=torch.float32, device=xyz.device, generator=generator)
    noise(xyz.data, model._opacity.data, model._scaling.data, model._rotation.data, xi, float(noise_lr) * float(xyz_lr))


@torch.no_grad()
def relocate_gs(model, min_opacity: float = 0.005, generator: torch.Generator = None):
    """Move every dead Gaussian (``sigmoid(_opacity) <= min_opacity``) onto a live one drawn with probability
    proportional to its opacity.  In place: the parameters stay the same ``nn.Parameter`` objects.  Returns
    ``(dead_idx, sampled_idx)``; with no dead or no live Gaussian nothing is launched and ``sampled_idx`` is empty."""
    _dev_check(model._opacity, "_opacity")
    groups = _model_groups(model, "relocate_gs")
    o = torch.sigmoid(model._opacity.detach()).reshape(-1)
    dead = o <= min_opacity
    dead_idx = dead.nonzero(as_tuple=True)[0]
    alive_idx = (~dead).nonzero(as_tuple=True)[0]
    if dead_idx.numel() == 0 or alive_idx.numel() == 0:
        return dead_idx, dead_idx.new_empty(0)
    sampled_idx = alive_idx[sample_sources(o[alive_idx], dead_idx.numel(), generator)]
    new_op, new_sc, _ = relocation(model._opacity.data, model._scaling.data, sampled_idx, min_opacity=min_opacity)
    apply_relocation([(p.data, m, v, role) for _, _, role, p, m, v in groups], sampled_idx, dead_idx, new_op, new_sc)
    return dead_idx, sampled_idx


@torch.no_grad()
def add_new_gs(model, cap_max: int, grow: float = 1.05, generator: torch.Generator = None) -> torch.Tensor:
    """Grow the set to ``min(cap_max, int(grow * P))`` Gaussians: ``n`` sources drawn from all Gaussians with
    probability proportional to their opacity, their copies appended as rows P .. P + n - 1 with zero moments.  The
    parameters and the optimizer state are replaced (``densify._replace_in_optimizer``) and ``xyz_gradient_accum``,
    ``denom`` and ``max_radii2D`` are zeros of the new size, as ``densify_and_prune`` leaves them.  Returns the sampled
    indices; with ``n = 0`` nothing is replaced."""
    _dev_check(model._xyz, "_xyz")
    groups = _model_groups(model, "add_new_gs")
    P = model._xyz.shape[0]
    n = max(0, min(int(cap_max), int(grow * P)) - P)
    device = model._xyz.device
    if n == 0 or P == 0:
        return torch.empty(0, dtype=torch.int64, device=device)
    sampled_idx = sample_sources(torch.sigmoid(model._opacity.detach()).reshape(-1), n, generator)
    new_op, new_sc, _ = relocation(model._opacity.data, model._scaling.data, sampled_idx)

    def grown(t, fill_zero):
        out = torch.empty((P + n,) + tuple(t.shape[1:]), dtype=torch.float32, device=device)
        out[:P] = t
        if fill_zero:
            out[P:] = 0
        return out

    new, surgery = {}, []
    for name, _attr, role, p, m, v in groups:
        _f32(p.data, name, (P,) + (-1,) * (p.dim() - 1))
        data = grown(p.data, False)  # (the surgery writes every new row)
        gm = grown(m, True) if m is not None else None
        gv = grown(v, True) if v is not None else None
        new[name] = (data, gm, gv)
        surgery.append((data, gm, gv, role))
    dest = torch.arange(P, P + n, dtype=torch.int64, device=device)
    apply_relocation(surgery, sampled_idx, dest, new_op, new_sc)
    replaced = _replace_in_optimizer(model.optimizer, new)
    for name, attr, _ in GROUPS:
        setattr(model, attr, replaced[name])
    model.xyz_gradient_accum = torch.zeros((P + n, 1), device=device)
    model.denom = torch.zeros((P + n, 1), device=device)
    model.max_radii2D = torch.zeros((P + n), device=device)
    return sampled_idx


def install(cls) -> None:
    """Bind the MCMC strategy as ``cls``'s methods (cls = the reference's GaussianModel)."""
    cls.inject_noise = inject_noise
    cls.relocate_gs = relocate_gs
    cls.add_new_gs = add_new_gs
