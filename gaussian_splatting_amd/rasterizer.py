"""Python surface of the rasterizer: the same names and behaviour as the reference's
``diff_gaussian_rasterization/__init__.py`` (``GaussianRasterizationSettings`` :151-180,
``GaussianRasterizer`` :183-274, ``rasterize_gaussians`` :24-46, ``_RasterizeGaussians``
:48-148), running on libgsr through the ``_C`` module of this package.
"""
from __future__ import annotations

import threading
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _C

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "_RasterizeGaussians",
           "_RasterizeGaussiansCamera", "_RenderFeatures", "_RenderDistortion", "_RenderMedian", "cpu_deep_copy_tuple"]


def cpu_deep_copy_tuple(input_tuple):
    """Copy every tensor of a tuple to the host (debug helper kept from the reference surface)."""
    return tuple(item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple)


class GaussianRasterizationSettings(NamedTuple):
    """Per-view settings, field for field the reference's NamedTuple."""

    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    antialiasing: bool


def _rasterize_with_maps(args, features, distortion, kw, median=None, topk=None):
    """``rasterize_gaussians(..., features=F, distortion=t, median=t, topk=K)`` (any of them): the render without the
    keywords, whose node hands its buffers over, then the feature, distortion and / or median node behind it (``topk=``
    alone needs no node); ``feature_map``, ``distortion_map``, ``median_map, median_ids`` and ``topk_ids,
    topk_weights`` go in that order after ``alpha`` and before the contribution statistics."""
    means3D, means2D = args[0], args[1]
    s = args[-1]
    scales, rotations, cov3D = args[-4], args[-3], args[-2]
    opacities = args[-5]
    if not isinstance(means3D, torch.Tensor) or means3D.dim() != 2:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    has_cov = isinstance(cov3D, torch.Tensor) and cov3D.numel() != 0
    geom_in = (means3D, means2D, opacities, scales, rotations)
    # (median= and topk= form no geometry gradient: nothing of theirs to refuse)
    if has_cov and (features is not None or distortion is not None) and torch.is_grad_enabled() and any(
            isinstance(t, torch.Tensor) and t.requires_grad for t in geom_in + (cov3D,)):
        kws = " / ".join(k for k, v in (("features=", features), ("distortion=", distortion)) if v is not None)
        loss = "feature" if distortion is None else "distortion" if features is None else "feature / distortion"
        raise RuntimeError(f"{kws} with cov3D_precomp cannot give a geometry gradient of the {loss} loss (its "
                           "per-Gaussian backward needs scales and rotations): detach the geometry inputs for this "
                           "render, or pass scales and rotations")
    device = means3D.device if means3D.device.type == "cuda" else None
    if features is not None:
        _C.check_features(features, means3D.size(0), device)
    if distortion is not None:
        _C.check_distortion(distortion, means3D.size(0), device)
    if median is not None:
        _C.check_median(median, means3D.size(0), device)
    K = 0 if topk is None else _C.check_topk(topk)
    if K and median is None:
        _C._require_device(means3D, "means3D")
    _RasterizeGaussians._handover.value = True  # (read by the node's forward, which leaves its buffers there)
    try:
        outs = rasterize_gaussians(*args, **kw)
        handed = getattr(_RasterizeGaussians._handover, "value", None)
    finally:
        _RasterizeGaussians._handover.value = None
    if not isinstance(handed, tuple):
        raise RuntimeError("rasterize_gaussians(features= / distortion= / median= / topk=): the render did not hand "
                           "over its buffers")
    empty = means3D.new_empty(0)
    tail = (means3D, means2D, opacities, empty if has_cov else scales, empty if has_cov else rotations, outs[1],
            *handed[:3], s, handed[3])  # both nodes receive the buffers of the one render
    maps = ()
    if features is not None:
        maps += (_RenderFeatures.apply(features, *tail),)
    if distortion is not None:
        maps += (_RenderDistortion.apply(distortion, *tail),)
    if median is not None:  # (one launch serves both keywords)
        maps += _RenderMedian.apply(median, *handed[:3], s, handed[3], K)
    elif K:
        maps += _C.render_select(*handed, means3D.size(0), s.image_height, s.image_width, topk=K,
                                 device=means3D.device)[2:]
    n = 4 if kw.get("return_alpha") else 3
    return outs[:n] + maps + outs[n:]


def _geometry_of(ctx, s, radii):
    """The ``geometry`` argument of a map node's native backward: the camera and radii when a geometry input of the
    node needs a gradient, else None."""
    if not any(ctx.needs_input_grad[1:6]):
        return None
    return dict(viewmatrix=s.viewmatrix.detach(), projmatrix=s.projmatrix.detach(), campos=s.campos.detach(),
                tanfovx=s.tanfovx, tanfovy=s.tanfovy, antialiasing=s.antialiasing, radii=radii)


def _map_node_grads(ctx, s, grad_first, block, means3D, opacities, scales, rotations):
    """A map node's backward tuple: the gradient of its first input, then, from the view block of its loss alone
    (``_C.gauss_backward_views``), those of ``means3D, means2D, opacities, scales, rotations``; None for the rest."""
    grad_first = grad_first if ctx.needs_input_grad[0] else None
    if block is None:
        return (grad_first,) + (None,) * 11
    P = means3D.size(0)
    f32 = dict(dtype=torch.float32, device=means3D.device)
    out = {"dL_dmeans3D": torch.empty((P, 3), **f32), "dL_ddc": torch.empty((P, 1, 3), **f32),
           "dL_dsh": torch.empty((P, 0, 3), **f32), "dL_dopacity": torch.empty((P, 1), **f32),
           "dL_dscales": torch.empty((P, 3), **f32), "dL_drotations": torch.empty((P, 4), **f32)}
    grad_means2D = torch.zeros((P, 3), **f32)
    if P > 0:
        # the view block carries no colour gradient: a zero dc of one coefficient satisfies the SH reads
        _C.gauss_backward_views(means3D, torch.zeros((P, 1, 3), **f32), None, 0, opacities, scales, rotations,
                                s.scale_modifier, block.view(1, -1), out)
        grad_means2D[:, :2] = block[64 + 4 * P:64 + 8 * P].view(P, 4)[:, :2]
    need = ctx.needs_input_grad
    return (grad_first, out["dL_dmeans3D"] if need[1] else None, grad_means2D if need[2] else None,
            out["dL_dopacity"].view(opacities.shape) if need[3] else None,
            out["dL_dscales"] if need[4] else None, out["dL_drotations"] if need[5] else None) + (None,) * 6


class _RenderFeatures(torch.autograd.Function):
    """The feature node behind the rasterizer node: forward = ``_C.render_features`` over the rasterizer node's buffers
    (non-differentiable inputs), backward = ``_C.render_features_backward`` and, when a geometry input needs a
    gradient, ``_C.gauss_backward_views`` over the one view block it fills.  Inputs ``(features, means3D, means2D,
    opacities, scales, rotations, radii, geom, binning, img, raster_settings, num_rendered)``; ``means2D`` only
    receives the feature loss's screen-space gradient, which autograd adds to the colour's."""

    @staticmethod
    def forward(ctx, features, means3D, means2D, opacities, scales, rotations, radii, geom, binning, img, s,
                num_rendered):
        fmap = _C.render_features(geom, binning, img, num_rendered, means3D.size(0), s.image_height, s.image_width,
                                  features)
        ctx.raster_settings = s
        ctx.num_rendered = num_rendered
        ctx.save_for_backward(features, fmap, means3D, opacities, scales, rotations, radii, geom, binning, img)
        return fmap

    @staticmethod
    def backward(ctx, grad_fmap):
        s = ctx.raster_settings
        features, fmap, means3D, opacities, scales, rotations, radii, geom, binning, img = ctx.saved_tensors
        P = means3D.size(0)
        geometry = _geometry_of(ctx, s, radii)
        if geometry is not None and P > 0 and (scales.numel() == 0 or rotations.numel() == 0):
            raise RuntimeError("features=: a geometry gradient of the feature loss needs scales and rotations")
        dL_dF, block = _C.render_features_backward(geom, binning, img, ctx.num_rendered, P, s.image_height,
                                                   s.image_width, features, fmap, grad_fmap.contiguous(),
                                                   geometry=geometry)
        return _map_node_grads(ctx, s, dL_dF, block, means3D, opacities, scales, rotations)


class _RenderDistortion(torch.autograd.Function):
    """The distortion node behind the rasterizer node, built like ``_RenderFeatures``: forward =
    ``_C.render_distortion`` over the rasterizer node's buffers, backward = ``_C.render_distortion_backward`` and,
    when a geometry input needs a gradient, ``_C.gauss_backward_views`` over the one view block it fills.  Inputs
    ``(t, means3D, means2D, opacities, scales, rotations, radii, geom, binning, img, raster_settings,
    num_rendered)``; the per-pixel moments the backward needs stay inside the node."""

    @staticmethod
    def forward(ctx, t, means3D, means2D, opacities, scales, rotations, radii, geom, binning, img, s, num_rendered):
        dmap, moments = _C.render_distortion(geom, binning, img, num_rendered, means3D.size(0), s.image_height,
                                             s.image_width, t)
        ctx.raster_settings = s
        ctx.num_rendered = num_rendered
        ctx.save_for_backward(t, dmap, moments, means3D, opacities, scales, rotations, radii, geom, binning, img)
        return dmap

    @staticmethod
    def backward(ctx, grad_dmap):
        s = ctx.raster_settings
        t, dmap, moments, means3D, opacities, scales, rotations, radii, geom, binning, img = ctx.saved_tensors
        P = means3D.size(0)
        geometry = _geometry_of(ctx, s, radii)
        if geometry is not None and P > 0 and (scales.numel() == 0 or rotations.numel() == 0):
            raise RuntimeError("distortion=: a geometry gradient of the distortion loss needs scales and rotations")
        dL_dt, block = _C.render_distortion_backward(geom, binning, img, ctx.num_rendered, P, s.image_height,
                                                     s.image_width, t, dmap, moments, grad_dmap.contiguous(),
                                                     geometry=geometry)
        return _map_node_grads(ctx, s, dL_dt, block, means3D, opacities, scales, rotations)


class _RenderMedian(torch.autograd.Function):
    """The median node behind the rasterizer node: forward = ``_C.render_select`` over the rasterizer node's buffers
    (with the top-K planes too when ``topk=`` came with ``median=``: one launch), backward =
    ``_C.render_median_backward``.  Inputs ``(t, geom, binning, img, raster_settings, num_rendered, K)``; ``t`` is the
    only differentiable one -- the median is piecewise constant in the blend weights, so the geometry receives a
    gradient only through whatever torch built ``t`` from.  Outputs ``(median_map, median_ids[, topk_ids,
    topk_weights])``, all but the first non-differentiable."""

    @staticmethod
    def forward(ctx, t, geom, binning, img, s, num_rendered, K):
        med, ids, tk_ids, tk_w = _C.render_select(geom, binning, img, num_rendered, t.size(0), s.image_height,
                                                  s.image_width, t=t, topk=K)
        ctx.P = t.size(0)
        ctx.save_for_backward(ids)
        rest = (ids,) if not K else (ids, tk_ids, tk_w)
        ctx.mark_non_differentiable(*rest)
        return (med,) + rest

    @staticmethod
    def backward(ctx, grad_med, *_rest):
        (ids,) = ctx.saved_tensors
        dL_dt = _C.render_median_backward(ids, grad_med.contiguous(), ctx.P) if ctx.needs_input_grad[0] else None
        return (dL_dt,) + (None,) * 6


def rasterize_gaussians(*args, return_alpha=False, absgrad=False, return_contrib=False, contrib_weight=None,
                        features=None, distortion=None, median=None, topk=None):
    """``rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
    raster_settings)`` (vendored, :24-46), or the 3DGS-accel form with ``dc`` before ``sh``.

    ``return_alpha=True`` (an extension): returns ``(color, radii, invdepths, alpha)``, ``alpha`` [1,H,W] the
    accumulated opacity ``1 - final_T`` of every pixel, differentiable like the other two maps.

    ``absgrad=True`` (an extension, gsplat's convention): the backward of this render also sets
    ``means2D.absgrad`` [P,3] (float32, on the device): per Gaussian the sum over pixels of the ABSOLUTE value of
    each pixel's term of ``means2D.grad`` (AbsGS; include/gsr.h gsr_backward_args.dL_dmean2D_abs), column 2 zero.  Each
    backward overwrites it.  Without the keyword no attribute is set and nothing more is launched or allocated.

    ``return_contrib=True`` (an extension): one more output, LAST (after ``alpha`` when both are asked for): the
    per-Gaussian contribution statistics [P,4] of this render (include/gsr.h gsr_contrib_stats; named views:
    ``gaussian_splatting_amd.contrib.split``), computed in the node's forward from the buffers it saves anyway and
    not differentiable.  ``contrib_weight`` ([H,W] or [1,H,W], only with ``return_contrib``) is the per-pixel map of
    the ``weighted_sum`` column.  Without the keywords nothing more is launched or allocated.

    ``features=F`` (an extension, gsplat's N-D features): ``F`` a contiguous float32 [P,C] device tensor, any C >= 1.
    One more output ``feature_map`` [C,H,W], after ``alpha`` when that is present and before the contribution
    statistics: ``sum_g alpha_g T_g F[g]`` per pixel with this render's own blend weights, no background term
    (include/gsr.h gsr_render_features; one more pass over the buffers the node saves anyway instead of ceil(C/3)
    renders).  Differentiable with respect to ``F`` and, through an autograd node of its own behind the rasterizer
    node (``_RenderFeatures``), to ``means3D``, ``opacities``, ``scales``, ``rotations`` and ``means2D`` (so
    ``means2D.grad`` carries the feature loss too); when only ``F`` requires grad the backward does the ``F`` work
    alone.  The feature loss does not reach the camera tensors or ``means2D.absgrad``; with ``cov3D_precomp`` a
    geometry input that requires grad is refused.  Without the keyword nothing more is launched or allocated.

    ``distortion=t`` (an extension, the Mip-NeRF 360 / 2DGS / gsplat ``distloss`` term): ``t`` a contiguous float32
    [P] device tensor of the caller's choice (view depth, ``1/z``, a contracted distance).  One more output
    ``distortion_map`` [1,H,W], after ``feature_map`` when that is present and before the contribution statistics:
    per pixel ``D = 2 sum_i w_i (t_i A_{i-1} - B_{i-1})`` over its contributors front to back with this render's own
    blend weights (``A``, ``B`` the running sums of ``w`` and ``w t``; include/gsr.h gsr_render_distortion).  That is
    ``sum_{i,j} w_i w_j |t_i - t_j|`` whenever ``t`` is non-decreasing along the blend order (any increasing function
    of view depth) and the SIGNED form ``2 sum_{i behind j} w_i w_j (t_i - t_j)`` otherwise; no background term.
    Differentiable with respect to ``t`` (so to whatever torch built it from, ``means3D`` and camera tensors
    included) and, through an autograd node of its own (``_RenderDistortion``), to the geometry exactly as
    ``features=``, with the same limits: the kernel's geometry part does not reach the camera tensors or
    ``means2D.absgrad``, and ``cov3D_precomp`` with a geometry input that requires grad is refused.  Without the
    keyword nothing more is launched or allocated.  The distortion loss and the median depth below are meant to be
    used from one render.

    ``median=t`` (an extension, the median depth of 2DGS / GOF / RaDe-GS / PGSR): ``t`` as for ``distortion=``.  Two
    more outputs after ``distortion_map``: ``median_map`` [1,H,W], per pixel ``t`` of its median contributor -- the
    last one blended while the transmittance is above one half (the one that takes it to one half or below, or the
    pixel's last contributor) -- and ``median_ids`` [1,H,W] int32, that contributor's Gaussian index; a pixel without
    a contributor holds 0.0 and -1 (include/gsr.h gsr_render_select).  ``median_map`` is differentiable with respect
    to ``t`` ONLY: it is a copy of ``t``, piecewise constant in the blend weights, so there is no geometry gradient
    through the kernel (2DGS forms none either); the gradient reaches ``means3D`` and the camera tensors through
    whatever torch built ``t`` from (autograd node ``_RenderMedian``).  ``median_ids`` is not differentiable.
    ``cov3D_precomp`` with geometry inputs that require grad is accepted.

    ``topk=K`` (an extension; ``1 <= K <= _C.select_max_k()``, 8): two more outputs after the median's, ``topk_ids``
    [K,H,W] int32 and ``topk_weights`` [K,H,W] float32: per pixel the K contributors of largest blend weight in
    descending weight, the earlier in blend order first on equal weights; ranks beyond the pixel's contributor count
    hold -1 and 0.0.  For picking, id buffers, lifting 2D masks or labels onto Gaussians, per-pixel debugging.  Not
    differentiable: ``features=`` is the differentiable blend.  With ``median=`` both come from one launch.  Without
    the keywords nothing more is launched or allocated."""
    if len(args) not in (9, 10):
        raise TypeError(f"rasterize_gaussians(): expected 9 or 10 arguments, got {len(args)}")
    if features is not None or distortion is not None or median is not None or topk is not None:
        return _rasterize_with_maps(args, features, distortion,
                                    dict(return_alpha=return_alpha, absgrad=absgrad, return_contrib=return_contrib,
                                         contrib_weight=contrib_weight), median=median, topk=topk)
    _RasterizeGaussians._return_alpha.value = bool(return_alpha)  # (read and cleared by the node's forward)
    _RasterizeGaussians._absgrad.value = bool(absgrad)            # (likewise)
    if contrib_weight is not None and not return_contrib:
        raise TypeError("rasterize_gaussians(): contrib_weight needs return_contrib=True")
    _RasterizeGaussians._contrib.value = (contrib_weight,) if return_contrib else None  # (likewise)
    # Camera-pose gradients: when a camera tensor of the settings requires grad (and grad mode is on) the three
    # enter the autograd node as explicit inputs after the settings; every other render takes the path below.
    s = args[-1]
    cam = (s.viewmatrix, s.projmatrix, s.campos)
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in cam):
        _RasterizeGaussians._no_backward.value = False  # (the camera tensors alone make a backward possible)
        return _RasterizeGaussiansCamera.apply(*args, *cam)
    # (a render no backward can follow -- grad disabled, or no input requires grad -- skips the atomic backward's
    # accumulator zeroing; autograd's needs_input_grad cannot tell, it ignores the grad mode)
    _RasterizeGaussians._no_backward.value = not (torch.is_grad_enabled() and any(
        isinstance(a, torch.Tensor) and a.requires_grad for a in args[:-1]))
    return _RasterizeGaussians.apply(*args)


class _RasterizeGaussians(torch.autograd.Function):
    """Autograd node: forward = _C.rasterize_gaussians, backward = _C.rasterize_gaussians_backward.

    Inputs ``(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings)``
    as in the vendored rasterizer (:48-148), or ``(means3D, means2D, dc, sh, ...)`` as in the 3DGS-accel build
    (separate_sh=True callers, gaussian_renderer/__init__.py:106-125): ``dc`` is ``_features_dc`` [P,1,3] and
    ``sh`` then ``_features_rest`` [P,M,3]; the two get their own gradients, with no concatenation.
    ``means2D`` only carries the screen-space gradient (the reference's trick for densification statistics);
    its value is never read.
    """

    _no_backward = threading.local()
    _return_alpha = threading.local()  # set by rasterize_gaussians(..., return_alpha=True) for its one call
    _absgrad = threading.local()       # set by rasterize_gaussians(..., absgrad=True) for its one call
    _contrib = threading.local()       # set by rasterize_gaussians(..., return_contrib=True): (contrib_weight,)
    _handover = threading.local()      # True for a call with a map keyword: the forward leaves its buffers

    @staticmethod
    def _absgrad_kw(ctx):
        """``{"absgrad": True}`` for a node rendered with the keyword, else no keyword at all."""
        return {} if ctx.absgrad_of is None else {"absgrad": True}

    @staticmethod
    def _set_absgrad(ctx, grads):
        """Takes the absolute gradient (last) off the backward's tuple of an absgrad node and sets it on the
        node's means2D, overwriting that of an earlier backward."""
        if ctx.absgrad_of is None:
            return grads
        ctx.absgrad_of.absgrad = grads[-1]
        return grads[:-1]

    @staticmethod
    def _upstream(ctx, grad_out_color, grad_out_depth, grad_alpha):
        """The upstream gradients as _C.rasterize_gaussians_backward takes them: ``(color, depth, keywords)``.
        A node with an alpha output does not materialise missing gradients, so an unused alpha map costs
        nothing (None -> NULL); colour and depth are then filled in as autograd would have."""
        if not ctx.with_alpha:
            return grad_out_color, grad_out_depth, {}
        s = ctx.raster_settings
        f32 = dict(dtype=torch.float32, device=ctx.saved_tensors[1].device)
        if grad_out_color is None:
            grad_out_color = torch.zeros((3, s.image_height, s.image_width), **f32)
        if grad_out_depth is None:
            grad_out_depth = torch.zeros((1, s.image_height, s.image_width), **f32)
        return grad_out_color, grad_out_depth, ({} if not grad_alpha or grad_alpha[0] is None else
                                                {"dL_dout_alpha": grad_alpha[0]})

    @staticmethod
    def forward(ctx, *args):
        if len(args) == 10:
            means3D, means2D, dc, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, s = args
        else:
            means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, s = args
            dc = None
        head = (s.bg, means3D, colors_precomp, opacities, scales, rotations, s.scale_modifier, cov3Ds_precomp,
                s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width)
        tail = (s.sh_degree, s.campos, s.prefiltered, s.antialiasing, s.debug)
        sh_args = (sh,) if dc is None else (dc, sh)
        no_backward = getattr(_RasterizeGaussians._no_backward, "value", False)
        _RasterizeGaussians._no_backward.value = False  # (set by rasterize_gaussians for this call only)
        with_alpha = getattr(_RasterizeGaussians._return_alpha, "value", False)
        _RasterizeGaussians._return_alpha.value = False
        ctx.with_alpha = with_alpha
        # absgrad: the node keeps means2D (its value is never read) and its backward sets means2D.absgrad
        ctx.absgrad_of = means2D if getattr(_RasterizeGaussians._absgrad, "value", False) else None
        _RasterizeGaussians._absgrad.value = False
        contrib = getattr(_RasterizeGaussians._contrib, "value", None)
        _RasterizeGaussians._contrib.value = None
        if with_alpha:
            num_rendered, color, radii, geom, binning, img, invdepths, alpha = _C.rasterize_gaussians(
                *head, *sh_args, *tail, no_backward=no_backward, return_alpha=True)
            ctx.set_materialize_grads(False)
        else:
            num_rendered, color, radii, geom, binning, img, invdepths = _C.rasterize_gaussians(
                *head, *sh_args, *tail, no_backward=no_backward)
        ctx.raster_settings = s
        ctx.num_rendered = num_rendered
        ctx.separate_sh = dc is not None
        saved = (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, opacities, geom, binning, img)
        ctx.save_for_backward(*saved, *(() if dc is None else (dc,)))
        outs = (color, radii, invdepths, alpha) if with_alpha else (color, radii, invdepths)
        if getattr(_RasterizeGaussians._handover, "value", None) is True:
            # features= / distortion= / median= / topk=: the buffers saved above are handed to the nodes behind this one
            # (rasterize_gaussians), nothing else
            _RasterizeGaussians._handover.value = (geom, binning, img, num_rendered)
        if contrib is None:
            ctx.mark_non_differentiable(radii)
            return outs
        # the statistics of this forward, from the buffers saved above (read-only: the backward is unaffected)
        stats = _C.contribution_stats(geom, binning, img, num_rendered, means3D.size(0), s.image_height, s.image_width,
                                      pixel_weight=contrib[0])
        ctx.mark_non_differentiable(radii, stats)
        return outs + (stats,)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, grad_out_depth, *grad_alpha):
        s = ctx.raster_settings
        saved = ctx.saved_tensors
        grad_out_color, grad_out_depth, alpha_kw = _RasterizeGaussians._upstream(ctx, grad_out_color, grad_out_depth,
                                                                                 grad_alpha)
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, opacities, geom, binning,
         img) = saved[:11]
        dc = saved[11] if ctx.separate_sh else None
        head = (s.bg, means3D, radii, colors_precomp, opacities, scales, rotations, s.scale_modifier, cov3Ds_precomp,
                s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, grad_out_color, grad_out_depth)
        tail = (s.sh_degree, s.campos, geom, ctx.num_rendered, binning, img, s.antialiasing, s.debug)

        def fit(g, like):  # inputs given as empty tensors get no gradient
            return None if like is None or like.numel() == 0 else g

        if dc is None:
            (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh,
             grad_scales, grad_rotations) = _RasterizeGaussians._set_absgrad(ctx, _C.rasterize_gaussians_backward(
                 *head, sh, *tail, **alpha_kw, **_RasterizeGaussians._absgrad_kw(ctx)))
            return (grad_means3D, grad_means2D, fit(grad_sh, sh), fit(grad_colors_precomp, colors_precomp),
                    grad_opacities, fit(grad_scales, scales), fit(grad_rotations, rotations),
                    fit(grad_cov3Ds_precomp, cov3Ds_precomp), None)
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_dc, grad_sh,
         grad_scales, grad_rotations) = _RasterizeGaussians._set_absgrad(ctx, _C.rasterize_gaussians_backward(
             *head, dc, sh, *tail, **alpha_kw, **_RasterizeGaussians._absgrad_kw(ctx)))
        return (grad_means3D, grad_means2D, fit(grad_dc, dc), fit(grad_sh, sh),
                fit(grad_colors_precomp, colors_precomp), grad_opacities, fit(grad_scales, scales),
                fit(grad_rotations, rotations), fit(grad_cov3Ds_precomp, cov3Ds_precomp), None)


class _RasterizeGaussiansCamera(torch.autograd.Function):
    """``_RasterizeGaussians`` with the settings' ``viewmatrix``, ``projmatrix`` and ``campos`` as three further
    inputs after ``raster_settings`` (the same tensors: the forward reads them from the settings), so that
    ``loss.backward()`` reaches them and whatever they were built from.  The forward is ``_RasterizeGaussians``'s;
    the backward also runs the camera backward (``_C.rasterize_gaussians_backward(..., camera=True)``).  No
    reference counterpart; conventions in include/gsr.h ``gsr_camera_backward``."""

    @staticmethod
    def forward(ctx, *args):
        return _RasterizeGaussians.forward(ctx, *args[:-3])

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, grad_out_depth, *grad_alpha):
        s = ctx.raster_settings
        saved = ctx.saved_tensors
        grad_out_color, grad_out_depth, alpha_kw = _RasterizeGaussians._upstream(ctx, grad_out_color, grad_out_depth,
                                                                                 grad_alpha)
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, opacities, geom, binning,
         img) = saved[:11]
        dc = saved[11] if ctx.separate_sh else None
        cam_in = (s.viewmatrix, s.projmatrix, s.campos)
        view, proj, campos = (t.detach() for t in cam_in)
        head = (s.bg, means3D, radii, colors_precomp, opacities, scales, rotations, s.scale_modifier, cov3Ds_precomp,
                view, proj, s.tanfovx, s.tanfovy, grad_out_color, grad_out_depth)
        tail = (s.sh_degree, campos, geom, ctx.num_rendered, binning, img, s.antialiasing, s.debug)
        sh_args = (sh,) if dc is None else (dc, sh)
        *grads, g_view, g_proj, g_campos = _RasterizeGaussians._set_absgrad(ctx, _C.rasterize_gaussians_backward(
            *head, *sh_args, *tail, camera=True, **alpha_kw, **_RasterizeGaussians._absgrad_kw(ctx)))

        def fit(g, like):  # inputs given as empty tensors get no gradient
            return None if like is None or like.numel() == 0 else g

        n = len(sh_args) + 8  # the inputs before the three camera tensors, the settings among them
        cam_grads = tuple(g.reshape(t.shape).to(t.device) if ctx.needs_input_grad[n + i] else None
                          for i, (g, t) in enumerate(zip((g_view, g_proj, g_campos), cam_in)))
        if dc is None:
            (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh,
             grad_scales, grad_rotations) = grads
            return (grad_means3D, grad_means2D, fit(grad_sh, sh), fit(grad_colors_precomp, colors_precomp),
                    grad_opacities, fit(grad_scales, scales), fit(grad_rotations, rotations),
                    fit(grad_cov3Ds_precomp, cov3Ds_precomp), None) + cam_grads
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_dc, grad_sh,
         grad_scales, grad_rotations) = grads
        return (grad_means3D, grad_means2D, fit(grad_dc, dc), fit(grad_sh, sh),
                fit(grad_colors_precomp, colors_precomp), grad_opacities, fit(grad_scales, scales),
                fit(grad_rotations, rotations), fit(grad_cov3Ds_precomp, cov3Ds_precomp), None) + cam_grads


class GaussianRasterizer(nn.Module):
    """nn.Module front-end; argument checks and empty-tensor placeholders as in the reference (:242-261)."""

    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        with torch.no_grad():
            s = self.raster_settings
            return _C.mark_visible(positions, s.viewmatrix, s.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, dc=None, return_alpha=False, absgrad=False, return_contrib=False,
                contrib_weight=None, features=None, distortion=None, median=None, topk=None):
        """Same checks as the reference (:242-261).  ``dc=`` (keyword) selects the 3DGS-accel separate-SH
        input: ``dc`` = ``_features_dc`` [P,1,3] and ``shs`` = ``_features_rest`` [P,M,3]
        (gaussian_renderer/__init__.py:115-125).  ``return_alpha=True`` returns ``(color, radii, invdepths,
        alpha)`` with the differentiable accumulated-alpha map [1,H,W] (``rasterize_gaussians``).
        ``absgrad=True``: the backward also sets ``means2D.absgrad`` (``rasterize_gaussians``).
        ``return_contrib=True`` [+ ``contrib_weight=``]: the per-Gaussian contribution statistics [P,4] as the last
        output (``rasterize_gaussians``).  ``features=`` [P,C]: one more differentiable output ``feature_map``
        [C,H,W], after ``alpha`` and before the statistics; ``distortion=`` [P]: one more differentiable output
        ``distortion_map`` [1,H,W], after ``feature_map``; ``median=`` [P]: ``median_map`` [1,H,W] (differentiable
        with respect to ``median`` only) and ``median_ids`` [1,H,W] int32 after it; ``topk=K``: ``topk_ids`` and
        ``topk_weights`` [K,H,W] after those, not differentiable (``rasterize_gaussians``)."""
        s = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide exactly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or (
                (scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        empty = torch.Tensor([])
        shs = empty if shs is None else shs
        colors_precomp = empty if colors_precomp is None else colors_precomp
        scales = empty if scales is None else scales
        rotations = empty if rotations is None else rotations
        cov3D_precomp = empty if cov3D_precomp is None else cov3D_precomp
        # (no keyword at all without the request: the call is then the one without the feature)
        contrib_kw = dict(return_contrib=True, contrib_weight=contrib_weight) if return_contrib else (
            {} if contrib_weight is None else dict(contrib_weight=contrib_weight))
        if features is not None:
            contrib_kw = dict(contrib_kw, features=features)
        if distortion is not None:
            contrib_kw = dict(contrib_kw, distortion=distortion)
        if median is not None:
            contrib_kw = dict(contrib_kw, median=median)
        if topk is not None:
            contrib_kw = dict(contrib_kw, topk=topk)
        if dc is None:
            return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                       cov3D_precomp, s, return_alpha=return_alpha, absgrad=absgrad, **contrib_kw)
        dc = empty if colors_precomp.numel() != 0 else dc
        return rasterize_gaussians(means3D, means2D, dc, shs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, s, return_alpha=return_alpha, absgrad=absgrad, **contrib_kw)
