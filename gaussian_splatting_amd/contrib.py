"""Per-Gaussian contribution statistics for importance pruning (include/gsr.h ``gsr_contrib_stats``; kernel in
``csrc/contrib.hip``).

For every Gaussian and one view: the sum, the maximum and the number of the blend weights ``w = alpha * T`` the
forward used, and optionally their sum weighted by a per-pixel map -- what LightGaussian's global significance,
RadSplat's max-blend-weight pruning and the visibility-count prunes need.  Three ways to get them:

* ``rasterize_gaussians(..., return_contrib=True)`` / ``GaussianRasterizer.forward(..., return_contrib=True)``: one
  more output of a training render;
* ``render_contribution(...)``: a render no backward follows plus the statistics, for sweeps over the views;
* ``_C.contribution_stats(...)`` on the buffers of any forward.

The statistics are a [P,4] float32 tensor; ``split`` names its columns.  Accumulating over views (``out=``) adds the
sums and counts and maxes the maximum; across ranks, all-reduce the columns with SUM, MAX, SUM, SUM.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _C
from .rasterizer import GaussianRasterizationSettings

__all__ = ["ContributionStats", "split", "render_contribution"]


class ContributionStats(NamedTuple):
    """Views of the columns of a [P,4] statistics tensor (no copies)."""

    weight_sum: torch.Tensor    # [P] float32: sum of w over the Gaussian's contributing pixels
    weight_max: torch.Tensor    # [P] float32: max of w over them
    pixel_count: torch.Tensor   # [P] int32: their number (the uint32 bits: counts wrap at 2^32)
    weighted_sum: torch.Tensor  # [P] float32: sum of w * pixel_weight; zero without a map


def split(stats: torch.Tensor) -> ContributionStats:
    """The named column views of a statistics tensor [P,4] float32."""
    if stats.dim() != 2 or stats.size(1) != 4 or stats.dtype != torch.float32:
        raise RuntimeError(f"split: expected a float32 [P,4] tensor, got {stats.dtype} {tuple(stats.shape)}")
    return ContributionStats(stats[:, 0], stats[:, 1], stats.view(torch.int32)[:, 2], stats[:, 3])


def render_contribution(raster_settings: GaussianRasterizationSettings, means3D, opacities, shs=None,
                        colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, dc=None,
                        pixel_weight: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """One view's render and its contribution statistics, under ``torch.no_grad()``: a forward no backward will
    follow (it skips the atomic backward's zeroing) and the statistics call.  Arguments as
    ``GaussianRasterizer.forward`` without ``means2D``; ``pixel_weight`` ([H,W] or [1,H,W]) fills ``weighted_sum``;
    with ``out`` ([P,4], zeroed by the caller before the first view) the view is accumulated into it.

    Returns ``(color [3,H,W], radii [P], stats [P,4])``; ``stats`` is ``out`` when given."""
    s = raster_settings
    if (shs is None) == (colors_precomp is None):
        raise Exception("Please provide exactly one of either SHs or precomputed colors!")
    if ((scales is None or rotations is None) and cov3D_precomp is None) or (
            (scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
    empty = torch.Tensor([])
    e = lambda t: empty if t is None else t  # noqa: E731
    sh_args = (e(shs),) if dc is None else (empty if colors_precomp is not None else dc, e(shs))
    with torch.no_grad():
        num_rendered, color, radii, geom, binning, img, _invdepth = _C.rasterize_gaussians(
            s.bg, means3D, e(colors_precomp), opacities, e(scales), e(rotations), s.scale_modifier, e(cov3D_precomp),
            s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width, *sh_args, s.sh_degree,
            s.campos, s.prefiltered, s.antialiasing, s.debug, no_backward=True)
        stats = _C.contribution_stats(geom, binning, img, num_rendered, means3D.size(0), s.image_height,
                                      s.image_width, pixel_weight=pixel_weight, out=out)
    return color, radii, stats
