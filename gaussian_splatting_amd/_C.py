"""Drop-in replacement of the reference's ``diff_gaussian_rasterization._C`` module.

Same three functions, same positional arguments, same return tuples as the
pybind11 module of the reference (``ext.cpp:15-19``; tensor handling in
``rasterize_points.cu:45-274``), implemented over the C ABI of libgsr.so
(include/gsr.h).  Only HIP-device tensors are accepted: there is no CPU path.

Error behaviour follows the reference: a malformed ``means3D`` raises
``RuntimeError("means3D must have dimensions (num_points, 3)")``
(rasterize_points.cu:69-71) and any failure inside the native library raises
``RuntimeError`` with the library's message.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from typing import Optional

import torch

from . import _lib

__all__ = ["rasterize_gaussians", "rasterize_gaussians_backward", "rasterize_gaussians_backward_screen",
           "gauss_backward_views", "view_block_floats", "view_pack_floats", "view_block_pack", "view_block_unpack", "view_block_index",
           "views_live_floats", "views_live_list",
           "mark_visible", "adamUpdate", "fusedssim",
           "fusedssim_backward", "forward_rebuilds", "debug_forward_state", "render_alpha", "contribution_stats",
           "render_features", "render_features_backward", "feature_chunk", "check_features",
           "render_distortion", "render_distortion_backward", "check_distortion",
           "render_select", "render_median_backward", "check_median", "check_topk", "select_max_k"]


# Sync-free forward (gsr_forward_args.capacity_hint): the binning buffer is sized from a capacity
# hint -- a decaying maximum of recent num_rendered for the same (device, W, H) and point
# count, plus a margin -- so the forward never waits for the host mid-way.  A hint that
# turns out too small only costs a redo of the binning stage inside the library
# (forward_rebuilds() counts them).  One entry per (device, W, H): a new point count (after
# densification) replaces the old entry instead of piling up next to it.
# GSR_SYNC_FORWARD=1 restores the reference's synchronising forward.
_capacity: dict = {}
_CAP_MARGIN = 1.05
_CAP_DECAY = 0.98  # per forward; with the 1.05 margin a view 7% smaller than the last does not shrink the hint below the next
_INT_MAX = 2**31 - 1


def _capacity_hint(key, P: int) -> int:
    if os.environ.get("GSR_SYNC_FORWARD", "0") == "1":
        return 0
    p, last = _capacity.get(key, (P, 0))
    if p != P:
        return 0
    return min(_INT_MAX, int(last * _CAP_MARGIN) + 1024) if last > 0 else 0


def _note_rendered(key, P: int, nr: int) -> None:
    p, last = _capacity.get(key, (P, 0))
    _capacity[key] = (P, max(int(nr), int(last * _CAP_DECAY)) if p == P else int(nr))


def forward_rebuilds() -> int:
    """Forwards (process-wide) whose capacity hint was too small, so the binning stage was redone."""
    return int(_lib.load().gsr_forward_rebuilds())


# GSR_POISON=1 (the GPU test suite sets it): every scratch buffer the library requests is
# filled with 0xff bytes and every output the kernels are meant to overwrite completely is
# filled with NaN before the call, so a read of memory no kernel wrote, or an output element
# no kernel wrote, shows up in the parity tests instead of depending on what the caching
# allocator happened to hand out.
def _poison() -> bool:
    return os.environ.get("GSR_POISON", "0") == "1"


def _empty(shape, **kw) -> torch.Tensor:
    t = torch.empty(shape, **kw)
    if _poison():
        t.fill_(float("nan") if t.dtype.is_floating_point else -1)
    return t


def _stream_handle(device: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_device(t: torch.Tensor, name: str) -> None:
    if t.device.type != "cuda":
        raise RuntimeError(f"{name}: the MI355X rasterizer needs HIP device tensors, got a {t.device.type} tensor "
                           "(there is no CPU implementation)")


class _Inputs:
    """Keeps contiguous fp32 views alive for the duration of a native call."""

    def __init__(self, device: torch.device):
        self.device = device
        self.keep = []

    def opt(self, t: Optional[torch.Tensor], name: str, align16: bool = False) -> Optional[int]:
        """Device pointer of an optional input; an empty tensor means 'absent' (data_ptr()==nullptr)."""
        if t is None or t.numel() == 0:
            return None
        return self.req(t, name, align16)

    def radii(self, t: torch.Tensor) -> int:
        """Device pointer of the int32 radii, kept alive (a contiguous copy if needed) for the call."""
        _require_device(t, "radii")
        if t.dtype != torch.int32:
            raise RuntimeError(f"radii: expected an int32 tensor, got {t.dtype}")
        if t.device != self.device:
            raise RuntimeError(f"radii: tensor on {t.device}, expected {self.device}")
        t = t.contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def req(self, t: torch.Tensor, name: str, align16: bool = False, small: bool = False) -> int:
        if small and t.device.type != "cuda":
            t = t.to(self.device)  # bg / matrices / campos: 3-16 floats
        _require_device(t, name)
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name}: expected a float32 tensor, got {t.dtype}")
        if t.device != self.device:
            raise RuntimeError(f"{name}: tensor on {t.device}, expected {self.device}")
        t = t.contiguous()
        if align16 and t.data_ptr() % 16:
            t = t.clone()
        self.keep.append(t)
        return t.data_ptr()


class _Resizer:
    """The reference's resizeFunctional (rasterize_points.cu:29-43) as a C callback."""

    def __init__(self, tensor: torch.Tensor):
        # The callback closes over the tensor, not over self: a bound method would make a
        # reference cycle (self -> cb -> method -> self), so the multi-GB buffers would live
        # until Python's cyclic GC ran -- about twenty steps of them at 5M@4K (200 GB reserved).
        def resize(_ctx, nbytes):
            try:
                tensor.resize_(int(nbytes))
                if _poison():
                    tensor.fill_(255)
                return tensor.data_ptr()
            except Exception:  # e.g. out of memory: the library reports GSR_ERR_ALLOC
                return None

        self.cb = _lib.ALLOC_FN(resize)


def _present(t) -> bool:
    return t is not None and t.numel() != 0 and t.size(0) != 0


# The geometry buffers this process's forwards returned, by device address (weak: a freed buffer drops out).
# A backward given any other tensor at such an address -- a copy, a buffer restored from a checkpoint, a
# view -- makes the library forget that address's forward state first (include/gsr.h gsr_geom_forget), so
# the backward takes the record path after writing the record inputs instead of trusting a stale mark.
_FORWARD_GEOMS: "weakref.WeakValueDictionary[int, torch.Tensor]" = weakref.WeakValueDictionary()


def _own_geometry(geomBuffer: torch.Tensor) -> None:
    if geomBuffer.numel() == 0:
        return
    t = _FORWARD_GEOMS.get(geomBuffer.data_ptr())
    if t is None or t._cdata != geomBuffer._cdata:
        _lib.load().gsr_geom_forget(geomBuffer.data_ptr())


def render_alpha(imgBuffer: torch.Tensor, image_height: int, image_width: int) -> torch.Tensor:
    """The accumulated alpha ``1 - final_T`` [1,H,W] of the forward that filled ``imgBuffer`` (include/gsr.h
    gsr_render_alpha), on the current stream; zeros for the empty buffer of a forward of no Gaussians."""
    H, W = int(image_height), int(image_width)
    device = imgBuffer.device
    if imgBuffer.numel() == 0:
        return torch.zeros((1, H, W), dtype=torch.float32, device=device)
    _require_device(imgBuffer, "imgBuffer")
    alpha = _empty((1, H, W), dtype=torch.float32, device=device)  # every pixel is written
    with torch.cuda.device(device):
        rc = _lib.load().gsr_render_alpha(W, H, imgBuffer.data_ptr(), alpha.data_ptr(), _stream_handle(device))
    _lib.check(rc, "render_alpha")
    return alpha


def contribution_stats(geomBuffer: torch.Tensor, binningBuffer: torch.Tensor, imgBuffer: torch.Tensor,
                       num_rendered: int, P: int, image_height: int, image_width: int,
                       pixel_weight: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-Gaussian contribution statistics [P,4] float32 of the forward that filled the three buffers (include/gsr.h
    gsr_contrib_stats), on the current stream: columns ``weight_sum``, ``weight_max``, ``pixel_count`` (uint32 bits:
    view the column as int32) and ``weighted_sum`` (the blend weights times ``pixel_weight`` [H,W] or [1,H,W]; zero
    without it).  With ``out`` (contiguous float32 [P,4]) the view's statistics are combined into it -- sums and
    counts add, the maximum maxes -- and it is returned.  Read-only on the buffers (copies are accepted, a backward
    may precede or follow); not differentiable."""
    P, H, W = int(P), int(image_height), int(image_width)
    device = geomBuffer.device
    f32 = dict(dtype=torch.float32, device=device)
    if out is not None:
        if (tuple(out.shape) != (P, 4) or out.dtype != torch.float32 or not out.is_contiguous()
                or out.device != device):
            raise RuntimeError(f"out must be a contiguous float32 {(P, 4)} tensor on {device}")
    pw = None
    if pixel_weight is not None:
        if tuple(pixel_weight.shape) not in ((H, W), (1, H, W)):
            raise RuntimeError(f"pixel_weight: expected {(H, W)} or {(1, H, W)}, got {tuple(pixel_weight.shape)}")
        if pixel_weight.dtype != torch.float32:
            raise RuntimeError(f"pixel_weight: expected a float32 tensor, got {pixel_weight.dtype}")
        pw = pixel_weight.detach().to(device).contiguous()
    if P == 0:
        return out if out is not None else torch.zeros((0, 4), **f32)
    _require_device(geomBuffer, "geomBuffer")
    stats = out if out is not None else _empty((P, 4), **f32)  # every row is written
    with torch.cuda.device(device):
        rc = _lib.load().gsr_contrib_stats(
            P, int(num_rendered), W, H, geomBuffer.data_ptr() if geomBuffer.numel() else None,
            binningBuffer.data_ptr() if binningBuffer.numel() else None,
            imgBuffer.data_ptr() if imgBuffer.numel() else None, 0, int(binningBuffer.numel()),
            pw.data_ptr() if pw is not None else None, int(out is not None), stats.data_ptr(),
            _stream_handle(device))
    _lib.check(rc, "contribution_stats")
    return stats


def feature_chunk() -> int:
    """Channels one wave of the feature kernels blends at once (include/gsr.h gsr_render_features_chunk): a feature
    render of C channels runs ceil(C / feature_chunk()) waves per tile."""
    return int(_lib.load().gsr_render_features_chunk())


def check_features(features, P: int, device=None) -> None:
    """The argument check of every ``features=`` entry: a contiguous float32 HIP-device [P,C] tensor, C >= 1 (on
    ``device`` when given)."""
    if not isinstance(features, torch.Tensor):
        raise TypeError(f"features: expected a tensor, got {type(features).__name__}")
    if features.dim() != 2 or features.size(0) != int(P) or features.size(1) < 1:
        raise RuntimeError(f"features must have dimensions (num_points, C) with C >= 1, i.e. ({int(P)}, C); got "
                           f"{tuple(features.shape)}")
    if features.dtype != torch.float32:
        raise RuntimeError(f"features: expected a float32 tensor, got {features.dtype}")
    _require_device(features, "features")
    if device is not None and features.device != device:
        raise RuntimeError(f"features: tensor on {features.device}, expected {device}")
    if not features.is_contiguous():
        raise RuntimeError("features: expected a contiguous [P,C] tensor (call .contiguous())")


def _feature_buffers(geomBuffer, binningBuffer, imgBuffer):
    return (geomBuffer.data_ptr() if geomBuffer.numel() else None,
            binningBuffer.data_ptr() if binningBuffer.numel() else None,
            imgBuffer.data_ptr() if imgBuffer.numel() else None, 0, int(binningBuffer.numel()))


def render_features(geomBuffer: torch.Tensor, binningBuffer: torch.Tensor, imgBuffer: torch.Tensor,
                    num_rendered: int, P: int, image_height: int, image_width: int,
                    features: torch.Tensor) -> torch.Tensor:
    """The feature map [C,H,W] of ``features`` [P,C] blended with the weights of the forward that filled the three
    buffers (include/gsr.h gsr_render_features), on the current stream: ``sum_g alpha_g T_g features[g]`` per pixel,
    no background.  Read-only on the buffers (copies are accepted, a backward may precede or follow), bitwise
    reproducible; zeros when there are no Gaussians or none was rendered."""
    P, H, W = int(P), int(image_height), int(image_width)
    check_features(features, P)
    device = features.device
    C = int(features.size(1))
    f32 = dict(dtype=torch.float32, device=device)
    if P == 0:
        return torch.zeros((C, H, W), **f32)
    out = _empty((C, H, W), **f32)  # every element is written
    with torch.cuda.device(device):
        rc = _lib.load().gsr_render_features(P, C, int(num_rendered), W, H,
                                             *_feature_buffers(geomBuffer, binningBuffer, imgBuffer),
                                             features.data_ptr(), out.data_ptr(), _stream_handle(device))
    _lib.check(rc, "render_features")
    return out


def render_features_backward(geomBuffer: torch.Tensor, binningBuffer: torch.Tensor, imgBuffer: torch.Tensor,
                             num_rendered: int, P: int, image_height: int, image_width: int, features: torch.Tensor,
                             feature_map: torch.Tensor, dL_dfeature_map: torch.Tensor, geometry=None) -> tuple:
    """The backward of ``render_features`` (include/gsr.h gsr_render_features_backward): returns ``(dL_dfeatures
    [P,C], view_block)``.  ``geometry`` None (frozen geometry): only ``dL_dfeatures``, ``view_block`` is None.
    Otherwise a dict with ``viewmatrix, projmatrix, campos, tanfovx, tanfovy, antialiasing, radii``: the feature
    loss's per-Gaussian screen-space sums are also written, as a view block of ``view_block_floats(P)`` floats
    for ``gauss_backward_views`` (one view; ``dL_dmeans2D`` is
    ``view_block[64 + 4 * P:64 + 8 * P].view(P, 4)[:, :2]``)."""
    P, H, W = int(P), int(image_height), int(image_width)
    check_features(features, P)
    device = features.device
    C = int(features.size(1))
    f32 = dict(dtype=torch.float32, device=device)
    for name, t in (("feature_map", feature_map), ("dL_dfeature_map", dL_dfeature_map)):
        if tuple(t.shape) != (C, H, W) or t.dtype != torch.float32 or t.device != device:
            raise RuntimeError(f"{name}: expected a float32 {(C, H, W)} tensor on {device}, got {t.dtype} "
                               f"{tuple(t.shape)} on {t.device}")
    if P == 0:
        return torch.zeros((0, C), **f32), (None if geometry is None else torch.zeros(view_block_floats(0), **f32))
    ins = _Inputs(device)
    dL_dF = _empty((P, C), **f32)  # every element is written
    block = None
    cam = (None, None, None, 0.0, 0.0, 0, None)
    scratch = torch.empty(0, dtype=torch.uint8, device=device)
    rs = _Resizer(scratch)
    if geometry is not None:
        g = geometry
        block = _empty((view_block_floats(P),), **f32)
        campos = g["campos"] if g["campos"].device.type == "cuda" else g["campos"].to(device)
        cam = (ins.req(g["viewmatrix"], "viewmatrix", small=True), ins.req(g["projmatrix"], "projmatrix", small=True),
               ins.req(campos, "campos"), float(g["tanfovx"]), float(g["tanfovy"]), int(bool(g["antialiasing"])),
               ins.radii(g["radii"]))
    with torch.cuda.device(device):
        rc = _lib.load().gsr_render_features_backward(
            P, C, int(num_rendered), W, H, *_feature_buffers(geomBuffer, binningBuffer, imgBuffer),
            features.data_ptr(), ins.req(feature_map, "feature_map"), ins.req(dL_dfeature_map, "dL_dfeature_map"),
            dL_dF.data_ptr(), block.data_ptr() if block is not None else None, *cam, rs.cb, None,
            _stream_handle(device))
    _lib.check(rc, "render_features_backward")
    return dL_dF, block


def check_distortion(t, P: int, device=None) -> None:
    """The argument check of every ``distortion=`` entry: a contiguous float32 HIP-device [P] tensor (on ``device``
    when given)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"distortion: expected a tensor, got {type(t).__name__}")
    if t.dim() != 1 or t.size(0) != int(P):
        raise RuntimeError(f"distortion must have dimensions (num_points,), i.e. ({int(P)},); got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"distortion: expected a float32 tensor, got {t.dtype}")
    _require_device(t, "distortion")
    if device is not None and t.device != device:
        raise RuntimeError(f"distortion: tensor on {t.device}, expected {device}")
    if not t.is_contiguous():
        raise RuntimeError("distortion: expected a contiguous [P] tensor (call .contiguous())")


def render_distortion(geomBuffer: torch.Tensor, binningBuffer: torch.Tensor, imgBuffer: torch.Tensor,
                      num_rendered: int, P: int, image_height: int, image_width: int, t: torch.Tensor) -> tuple:
    """``(distortion_map [1,H,W], moments [2,H,W])`` of the per-Gaussian scalar ``t`` [P] under the weights of the
    forward that filled the three buffers (include/gsr.h gsr_render_distortion), on the current stream: per pixel
    ``D = 2 sum_i w_i (t_i A_{i-1} - B_{i-1})`` over its contributors front to back, which is ``sum_{i,j} w_i w_j
    |t_i - t_j|`` for ``t`` non-decreasing along the list and the signed form otherwise; ``moments`` holds every
    pixel's ``sum_i w_i`` and ``sum_i w_i (t_i - t_1)`` (about its first contributor) for the backward.  Read-only on the buffers (copies are accepted, a
    backward may precede or follow), bitwise reproducible; zeros when there are no Gaussians or none was rendered."""
    P, H, W = int(P), int(image_height), int(image_width)
    check_distortion(t, P)
    device = t.device
    f32 = dict(dtype=torch.float32, device=device)
    if P == 0:
        return torch.zeros((1, H, W), **f32), torch.zeros((2, H, W), **f32)
    dmap, moments = _empty((1, H, W), **f32), _empty((2, H, W), **f32)  # every element is written
    with torch.cuda.device(device):
        rc = _lib.load().gsr_render_distortion(P, int(num_rendered), W, H,
                                               *_feature_buffers(geomBuffer, binningBuffer, imgBuffer),
                                               t.data_ptr(), dmap.data_ptr(), moments.data_ptr(),
                                               _stream_handle(device))
    _lib.check(rc, "render_distortion")
    return dmap, moments


def render_distortion_backward(geomBuffer: torch.Tensor, binningBuffer: torch.Tensor, imgBuffer: torch.Tensor,
                               num_rendered: int, P: int, image_height: int, image_width: int, t: torch.Tensor,
                               distortion_map: torch.Tensor, moments: torch.Tensor, dL_ddistortion_map: torch.Tensor,
                               geometry=None) -> tuple:
    """The backward of ``render_distortion`` (include/gsr.h gsr_render_distortion_backward): returns ``(dL_dt [P],
    view_block)``.  ``geometry`` None (only ``t`` needs a gradient): ``dL_dt`` alone, ``view_block`` is None.
    Otherwise the dict ``render_features_backward`` takes, and the distortion loss's per-Gaussian screen-space sums
    are also written, as a view block for ``gauss_backward_views`` exactly as there."""
    P, H, W = int(P), int(image_height), int(image_width)
    check_distortion(t, P)
    device = t.device
    f32 = dict(dtype=torch.float32, device=device)
    for name, m, c in (("distortion_map", distortion_map, 1), ("moments", moments, 2),
                       ("dL_ddistortion_map", dL_ddistortion_map, 1)):
        if tuple(m.shape) != (c, H, W) or m.dtype != torch.float32 or m.device != device:
            raise RuntimeError(f"{name}: expected a float32 {(c, H, W)} tensor on {device}, got {m.dtype} "
                               f"{tuple(m.shape)} on {m.device}")
    if P == 0:
        return torch.zeros((0,), **f32), (None if geometry is None else torch.zeros(view_block_floats(0), **f32))
    ins = _Inputs(device)
    dL_dt = _empty((P,), **f32)  # every element is written
    block = None
    cam = (None, None, None, 0.0, 0.0, 0, None)
    scratch = torch.empty(0, dtype=torch.uint8, device=device)
    rs = _Resizer(scratch)
    if geometry is not None:
        g = geometry
        block = _empty((view_block_floats(P),), **f32)
        campos = g["campos"] if g["campos"].device.type == "cuda" else g["campos"].to(device)
        cam = (ins.req(g["viewmatrix"], "viewmatrix", small=True), ins.req(g["projmatrix"], "projmatrix", small=True),
               ins.req(campos, "campos"), float(g["tanfovx"]), float(g["tanfovy"]), int(bool(g["antialiasing"])),
               ins.radii(g["radii"]))
    with torch.cuda.device(device):
        rc = _lib.load().gsr_render_distortion_backward(
            P, int(num_rendered), W, H, *_feature_buffers(geomBuffer, binningBuffer, imgBuffer), t.data_ptr(),
            ins.req(distortion_map, "distortion_map"), ins.req(moments, "moments"),
            ins.req(dL_ddistortion_map, "dL_ddistortion_map"), dL_dt.data_ptr(),
            block.data_ptr() if block is not None else None, *cam, rs.cb, None, _stream_handle(device))
    _lib.check(rc, "render_distortion_backward")
    return dL_dt, block


def select_max_k() -> int:
    """The largest ``topk=`` this build supports (include/gsr.h gsr_render_select_max_k)."""
    return int(_lib.load().gsr_render_select_max_k())


def check_median(t, P: int, device=None) -> None:
    """The argument check of every ``median=`` entry: a contiguous float32 HIP-device [P] tensor (on ``device`` when
    given), as ``check_distortion``."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"median: expected a tensor, got {type(t).__name__}")
    if t.dim() != 1 or t.size(0) != int(P):
        raise RuntimeError(f"median must have dimensions (num_points,), i.e. ({int(P)},); got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"median: expected a float32 tensor, got {t.dtype}")
    _require_device(t, "median")
    if device is not None and t.device != device:
        raise RuntimeError(f"median: tensor on {t.device}, expected {device}")
    if not t.is_contiguous():
        raise RuntimeError("median: expected a contiguous [P] tensor (call .contiguous())")


def check_topk(K) -> int:
    """The argument check of every ``topk=`` entry: an int (not a bool) in ``1 .. select_max_k()``; returns it."""
    if isinstance(K, bool) or not isinstance(K, int):
        raise TypeError(f"topk: expected an int, got {type(K).__name__}")
    top = select_max_k()
    if not 1 <= K <= top:
        raise ValueError(f"topk: expected 1 <= K <= {top}, got {K}")
    return K


def render_select(geomBuffer: torch.Tensor, binningBuffer: torch.Tensor, imgBuffer: torch.Tensor, num_rendered: int,
                  P: int, image_height: int, image_width: int, t: Optional[torch.Tensor] = None, topk: int = 0,
                  device=None) -> tuple:
    """``(median_map [1,H,W] f32, median_ids [1,H,W] i32, topk_ids [K,H,W] i32, topk_weights [K,H,W] f32)`` of the
    forward that filled the three buffers (include/gsr.h gsr_render_select), in one pass on the current stream; the
    first two are None without ``t`` and the last two without ``topk``.  Per pixel the median contributor is the last
    one blended while the transmittance is above one half, ``median_map`` the copy of its ``t``; the top-K are the
    contributors of largest blend weight, descending, earlier first on ties.  No contributor / rank beyond the count:
    id -1, value 0.  Read-only on the buffers (copies are accepted, a backward may precede or follow), bitwise
    reproducible, not differentiable (``render_median_backward`` is the scatter to ``t``).  ``device``: where the
    buffers live, needed only without ``t``."""
    P, H, W = int(P), int(image_height), int(image_width)
    K = check_topk(topk) if topk != 0 or isinstance(topk, bool) else 0
    if t is None and K == 0:
        raise ValueError("render_select: nothing to select (no t and topk = 0)")
    if t is not None:
        check_median(t, P)
        device = t.device
    else:
        device = torch.device(geomBuffer.device if device is None else device)
        if device.type != "cuda":
            raise RuntimeError(f"render_select: the MI355X rasterizer needs HIP device buffers, got {device.type}")
    f32, i32 = dict(dtype=torch.float32, device=device), dict(dtype=torch.int32, device=device)
    # every element is written
    med, mid = (_empty((1, H, W), **f32), _empty((1, H, W), **i32)) if t is not None else (None, None)
    ids, wts = (_empty((K, H, W), **i32), _empty((K, H, W), **f32)) if K else (None, None)
    if _poison():  # (-1, _empty's integer poison, is a value the kernel writes)
        for x in (mid, ids):
            if x is not None:
                x.fill_(-2)
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None  # noqa: E731
    with torch.cuda.device(device):
        rc = _lib.load().gsr_render_select(P, int(num_rendered), W, H,
                                           *_feature_buffers(geomBuffer, binningBuffer, imgBuffer), ptr(t), K,
                                           ptr(med), ptr(mid), ptr(ids), ptr(wts), _stream_handle(device))
    _lib.check(rc, "render_select")
    return med, mid, ids, wts


def render_median_backward(median_ids: torch.Tensor, dL_dmedian_map: torch.Tensor, P: int) -> torch.Tensor:
    """The backward of ``render_select``'s median map (include/gsr.h gsr_render_median_backward): ``dL_dt`` [P], the
    upstream gradient [1,H,W] scattered to each pixel's median Gaussian.  Float atomics in the hardware's order: not
    bitwise reproducible."""
    P = int(P)
    device = median_ids.device
    _require_device(median_ids, "median_ids")
    if median_ids.dtype != torch.int32 or median_ids.dim() != 3 or median_ids.size(0) != 1:
        raise RuntimeError(f"median_ids: expected an int32 [1,H,W] tensor, got {median_ids.dtype} "
                           f"{tuple(median_ids.shape)}")
    _, H, W = median_ids.shape
    g = dL_dmedian_map
    if tuple(g.shape) != (1, H, W) or g.dtype != torch.float32 or g.device != device:
        raise RuntimeError(f"dL_dmedian_map: expected a float32 {(1, H, W)} tensor on {device}, got {g.dtype} "
                           f"{tuple(g.shape)} on {g.device}")
    f32 = dict(dtype=torch.float32, device=device)
    if P == 0:
        return torch.zeros((0,), **f32)
    ins = _Inputs(device)
    median_ids = median_ids.contiguous()
    dL_dt = _empty((P,), **f32)  # every element is written
    with torch.cuda.device(device):
        rc = _lib.load().gsr_render_median_backward(P, int(W), int(H), median_ids.data_ptr(),
                                                    ins.req(g, "dL_dmedian_map"), dL_dt.data_ptr(),
                                                    _stream_handle(device))
    _lib.check(rc, "render_median_backward")
    return dL_dt


def _scene_view(ins: _Inputs, *, means3D, dc, sh, degree, colors, opacities, scales, scale_modifier, rotations,
                cov3D_precomp, background, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, W, H, antialiasing,
                align_sh=False):
    """The ``Scene`` and ``View`` every rasterizer call passes (include/gsr.h gsr_scene / gsr_view), from the
    tensors, validated and kept alive by ``ins``.  ``dc`` goes in only with SH colours (the split layout); an empty
    optional tensor is absent; ``campos`` may live on the host."""
    split = dc is not None and _present(dc) and not _present(colors)
    if campos is not None and campos.device.type != "cuda":
        campos = campos.to(ins.device)
    # (pointers are taken in the reference's argument order: the first malformed tensor is the one reported)
    p_bg = ins.req(background, "bg", small=True)
    scene = _lib.Scene(
        P=means3D.size(0), D=int(degree), M=sh.size(1) if _present(sh) else 0, means3D=ins.req(means3D, "means3D"),
        dc=ins.req(dc, "dc") if split else None, shs=ins.opt(sh, "sh", align16=align_sh),
        colors_precomp=ins.opt(colors, "colors_precomp"), opacities=ins.req(opacities, "opacities"),
        scales=ins.opt(scales, "scales"), scale_modifier=float(scale_modifier),
        rotations=ins.opt(rotations, "rotations", align16=True), cov3D_precomp=ins.opt(cov3D_precomp, "cov3D_precomp"))
    view = _lib.View(
        width=W, height=H, background=p_bg, viewmatrix=ins.req(viewmatrix, "viewmatrix", small=True),
        projmatrix=ins.req(projmatrix, "projmatrix", small=True), campos=ins.opt(campos, "campos"),
        tan_fovx=float(tan_fovx), tan_fovy=float(tan_fovy), antialiasing=int(bool(antialiasing)))
    return scene, view


def _unpack_backward(args, who: str) -> tuple:
    """The vendored rasterizer's 24 positional backward arguments, or the 3DGS-accel build's 25 with ``dc`` before
    ``sh``: always the 25 (``dc`` None for 24), then whether it was the accel form."""
    if len(args) == 25:
        return (*args, True)
    if len(args) != 24:
        raise TypeError(f"{who}(): expected 24 or 25 positional arguments, got {len(args)}")
    (background, means3D, radii, colors, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
     projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_invdepth, sh, degree, campos, geomBuffer, R,
     binningBuffer, imageBuffer, antialiasing, debug) = args
    return (background, means3D, radii, colors, opacities, scales, rotations, scale_modifier, cov3D_precomp,
            viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_invdepth, None, sh, degree, campos,
            geomBuffer, R, binningBuffer, imageBuffer, antialiasing, debug, False)


def rasterize_gaussians(*args, no_backward: bool = False, return_alpha: bool = False) -> tuple:
    """RasterizeGaussiansCUDA (rasterize_points.cu:45-146).

    Positional arguments, as the pybind function takes them:
    ``(bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
    tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, antialiasing, debug)``
    -- the vendored rasterizer's 20 -- or the 3DGS-accel build's 21, which insert ``dc`` ([P,1,3]) before ``sh``
    (then the rest coefficients [P,M,3]); see include/gsr.h gsr_scene.dc.

    Returns ``(num_rendered, color[3,H,W], radii[P] int32, geomBuffer, binningBuffer, imgBuffer, invdepth[1,H,W])``.

    ``no_backward`` (an extension): no backward will follow (an eval / no_grad render), so the forward does not
    zero the atomic backward's accumulator rows beside its render ("bwd_atomic" 0 for this call; a backward
    of it would take the record path).

    ``return_alpha`` (an extension): the accumulated alpha ``1 - final_T`` [1,H,W] is appended to the returned
    tuple (one more small kernel, include/gsr.h gsr_render_alpha; zeros when there are no Gaussians).  Without
    it nothing more is launched or allocated.
    """
    if len(args) == 21:
        (background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
         projmatrix, tan_fovx, tan_fovy, image_height, image_width, dc, sh, degree, campos, prefiltered,
         antialiasing, debug) = args
    elif len(args) == 20:
        (background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
         projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, antialiasing,
         debug) = args
        dc = None
    else:
        raise TypeError(f"rasterize_gaussians(): expected 20 or 21 positional arguments, got {len(args)}")
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    _require_device(means3D, "means3D")
    device = means3D.device
    lib = _lib.load()
    P = means3D.size(0)
    H, W = int(image_height), int(image_width)
    f32 = dict(dtype=torch.float32, device=device)
    alloc = _empty if P > 0 else torch.zeros  # every pixel / Gaussian is written when P > 0
    out_color = alloc((3, H, W), **f32)
    out_invdepth = alloc((1, H, W), **f32)
    radii = alloc((P,), dtype=torch.int32, device=device)
    geom = torch.empty(0, dtype=torch.uint8, device=device)
    binning = torch.empty(0, dtype=torch.uint8, device=device)
    img = torch.empty(0, dtype=torch.uint8, device=device)
    if P == 0:
        fwd = (0, out_color, radii, geom, binning, img, out_invdepth)
        return fwd + (torch.zeros((1, H, W), **f32),) if return_alpha else fwd

    ins = _Inputs(device)
    rg, rb, ri = _Resizer(geom), _Resizer(binning), _Resizer(img)
    key = (device.index, W, H)
    scene, view = _scene_view(
        ins, means3D=means3D, dc=dc, sh=sh, degree=degree, colors=colors, opacities=opacity, scales=scales,
        scale_modifier=scale_modifier, rotations=rotations, cov3D_precomp=cov3D_precomp, background=background,
        viewmatrix=viewmatrix, projmatrix=projmatrix, campos=campos, tan_fovx=tan_fovx, tan_fovy=tan_fovy, W=W, H=H,
        antialiasing=antialiasing, align_sh=True)
    a = _lib.ForwardArgs(
        scene=scene, view=view, geom_alloc=rg.cb, binning_alloc=rb.cb, image_alloc=ri.cb,
        prefiltered=int(bool(prefiltered)), debug=int(bool(debug)), stream=_stream_handle(device),
        out_color=out_color.data_ptr(), out_invdepth=out_invdepth.data_ptr(), radii=radii.data_ptr(),
        capacity_hint=_capacity_hint(key, P))
    with torch.cuda.device(device):
        if no_backward:
            with _lib.thread_options(bwd_atomic=0):
                rc = lib.gsr_rasterize_forward(ctypes.byref(a))
        else:
            rc = lib.gsr_rasterize_forward(ctypes.byref(a))
    _lib.check(rc, "rasterize_gaussians")
    _FORWARD_GEOMS[geom.data_ptr()] = geom
    _note_rendered(key, P, a.num_rendered)
    # The binning buffer's layout (its capacity) is recovered by the backward from the buffer's
    # size (include/gsr.h gsr_backward_args.binning_bytes), so nothing rides on the tensor object.
    fwd = (int(a.num_rendered), out_color, radii, geom, binning, img, out_invdepth)
    return fwd + (render_alpha(img, H, W),) if return_alpha else fwd


def rasterize_gaussians_backward(*args, out=None, camera=False, dL_dout_alpha=None, absgrad=False):
    """RasterizeGaussiansBackwardCUDA (rasterize_points.cu:149-248).

    Positional arguments: the vendored rasterizer's 24 ``(bg, means3D, radii, colors, opacities, scales,
    rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color,
    dL_dout_invdepth, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, antialiasing, debug)``,
    or the 3DGS-accel build's 25 with ``dc`` before ``sh``.

    Returns ``(dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)``,
    or, with ``dc``, ``(..., dL_dcov3D, dL_ddc, dL_dsh, ...)`` (9 tensors, as the accel build returns them).
    ``out`` (an extension, not in the reference) may map any of the names ``dL_dmeans3D, dL_ddc, dL_dsh,
    dL_dopacity, dL_dscales, dL_drotations`` to preallocated contiguous float32 tensors of the right shape --
    e.g. views of one flat gradient arena that is then all-reduced without a copy.
    ``camera=True`` (an extension too) also runs the camera backward (include/gsr.h gsr_camera_backward) and
    returns the tuple above followed by ``(dL_dviewmatrix [4,4], dL_dprojmatrix [4,4], dL_dcampos [3])``: the
    gradients of the three camera tensors as the forward reads them, entry ``k`` of a flat gradient belonging to
    ``tensor.contiguous().view(-1)[k]``.
    ``dL_dout_alpha`` (an extension): the gradient [1,H,W] of the accumulated-alpha output
    (``rasterize_gaussians(..., return_alpha=True)``); its share is added to every returned gradient it reaches
    (include/gsr.h gsr_backward_args.dL_dalphas) and, with ``camera=True``, to the camera gradients.  None or
    an empty tensor: no alpha loss, the call and its results are those without the keyword.
    ``absgrad=True`` (an extension): the absolute screen-space gradient [P,3] (include/gsr.h
    gsr_backward_args.dL_dmean2D_abs: per Gaussian the sum over pixels of the absolute value of each pixel's term of
    ``dL_dmeans2D``, column 2 zero) is appended as the LAST element of the returned tuple, after the camera
    gradients when ``camera=True``.  Without it the call and its results are those without the keyword.
    """
    (background, means3D, radii, colors, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
     projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_invdepth, dc, sh, degree, campos, geomBuffer, R,
     binningBuffer, imageBuffer, antialiasing, debug, accel) = _unpack_backward(args, "rasterize_gaussians_backward")
    _require_device(means3D, "means3D")
    device = means3D.device
    lib = _lib.load()
    P = means3D.size(0)
    H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))
    M = sh.size(1) if _present(sh) else 0
    split = accel and dc is not None and _present(dc) and not _present(colors)
    f32 = dict(dtype=torch.float32, device=device)
    alloc = _empty if P > 0 else torch.zeros
    out = dict(out or {})

    def buf(name, shape):
        t = out.get(name)
        if t is None:
            return alloc(shape, **f32)
        if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
            raise RuntimeError(f"out[{name}] must be a contiguous float32 {tuple(shape)} tensor on {device}")
        return t

    dL_dmeans2D = alloc((P, 3), **f32)
    dL_dcolors = alloc((P, 3), **f32)
    dL_dopacity = buf("dL_dopacity", (P, 1))
    dL_dmeans3D = buf("dL_dmeans3D", (P, 3))
    dL_dcov3D = alloc((P, 6), **f32)
    # the accel build always returns a [P,1,3] dc gradient (zeros when colours were precomputed)
    dL_ddc = buf("dL_ddc", (P, 1, 3)) if accel else None
    dL_dsh = buf("dL_dsh", (P, M, 3))
    dL_dscales = buf("dL_dscales", (P, 3))
    dL_drotations = buf("dL_drotations", (P, 4))
    has_inv = dL_dout_invdepth is not None and dL_dout_invdepth.numel() != 0 and dL_dout_invdepth.size(0) != 0
    dL_dinvdepths = alloc((P, 1), **f32) if has_inv else None
    if accel:
        result = (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_ddc, dL_dsh, dL_dscales,
                  dL_drotations)
    else:
        result = (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)
    if P == 0:
        result = result + tuple(torch.zeros(s, **f32) for s in ((4, 4), (4, 4), (3,))) if camera else result
        return result + (torch.zeros((P, 3), **f32),) if absgrad else result
    dL_dabs = alloc((P, 3), **f32) if absgrad else None  # every element is written
    # the camera backward reads dL/dconic, which the backward otherwise does not store
    dL_dconic = alloc((P, 4), **f32) if camera else None
    if accel and not split:
        dL_ddc.zero_()  # no SH evaluation: the dc gradient is zero, as the accel build's zero-initialised tensor

    ins = _Inputs(device)
    scratch = torch.empty(0, dtype=torch.uint8, device=device)
    rs = _Resizer(scratch)
    _own_geometry(geomBuffer)
    has_alpha = dL_dout_alpha is not None and dL_dout_alpha.numel() != 0
    if has_alpha and dL_dout_alpha.numel() != H * W:
        raise RuntimeError(f"dL_dout_alpha: expected {(1, H, W)} values, got {tuple(dL_dout_alpha.shape)}")
    scene, view = _scene_view(
        ins, means3D=means3D, dc=dc, sh=sh, degree=degree, colors=colors, opacities=opacities, scales=scales,
        scale_modifier=scale_modifier, rotations=rotations, cov3D_precomp=cov3D_precomp, background=background,
        viewmatrix=viewmatrix, projmatrix=projmatrix, campos=campos, tan_fovx=tan_fovx, tan_fovy=tan_fovy, W=W, H=H,
        antialiasing=antialiasing)
    a = _lib.BackwardArgs(
        scene=scene, view=view, R=int(R), radii=ins.radii(radii), geom_buffer=geomBuffer.data_ptr(),
        binning_buffer=binningBuffer.data_ptr() if binningBuffer.numel() else None,
        image_buffer=imageBuffer.data_ptr(), binning_capacity=0, binning_bytes=int(binningBuffer.numel()),
        dL_dpix=ins.req(dL_dout_color, "dL_dout_color"),
        dL_dinvdepths=ins.req(dL_dout_invdepth, "dL_dout_invdepth") if has_inv else None,
        dL_dalphas=ins.req(dL_dout_alpha, "dL_dout_alpha") if has_alpha else None,
        dL_dmean2D=dL_dmeans2D.data_ptr(), dL_dmean2D_abs=dL_dabs.data_ptr() if absgrad else None,
        dL_dconic=dL_dconic.data_ptr() if camera else None, dL_dopacity=dL_dopacity.data_ptr(),
        dL_dcolor=dL_dcolors.data_ptr(), dL_dinvdepth=dL_dinvdepths.data_ptr() if has_inv else None,
        dL_dmean3D=dL_dmeans3D.data_ptr(), dL_dcov3D=dL_dcov3D.data_ptr(),
        dL_ddc=dL_ddc.data_ptr() if split else None, dL_dsh=dL_dsh.data_ptr() if M > 0 else None,
        dL_dscale=dL_dscales.data_ptr(), dL_drot=dL_drotations.data_ptr(), debug=int(bool(debug)),
        scratch_alloc=rs.cb, stream=_stream_handle(device))
    with torch.cuda.device(device):
        rc = lib.gsr_rasterize_backward(ctypes.byref(a))
    _lib.check(rc, "rasterize_gaussians_backward")
    if not camera:
        return result + (dL_dabs,) if absgrad else result
    # every element of the three is written
    dL_dview, dL_dproj, dL_dcampos = _empty((4, 4), **f32), _empty((4, 4), **f32), _empty((3,), **f32)
    cam_scratch = torch.empty(0, dtype=torch.uint8, device=device)
    rc_s = _Resizer(cam_scratch)
    # (with precomputed colours the camera backward takes no SH input)
    p_dc, p_sh = (None, None) if scene.colors_precomp else (scene.dc, scene.shs)
    with torch.cuda.device(device):
        rc = lib.gsr_camera_backward(
            P, scene.D, scene.M, W, H, scene.means3D, p_dc, p_sh, scene.colors_precomp, scene.opacities, scene.scales,
            scene.scale_modifier, scene.rotations, scene.cov3D_precomp, view.viewmatrix, view.projmatrix, view.campos,
            view.tan_fovx, view.tan_fovy, a.radii, a.geom_buffer, a.dL_dmean2D, a.dL_dconic, a.dL_dopacity,
            a.dL_dcolor, a.dL_dinvdepth, view.antialiasing, rc_s.cb, None, _stream_handle(device),
            dL_dview.data_ptr(), dL_dproj.data_ptr(), dL_dcampos.data_ptr())
    _lib.check(rc, "camera_backward")
    result = result + (dL_dview, dL_dproj, dL_dcampos)
    return result + (dL_dabs,) if absgrad else result


def debug_forward_state(fwd, P: int) -> dict:
    """The forward's private tile lists and per-pixel state (include/gsr.h gsr_debug_forward_state),
    for parity tests: ``ranges`` [tiles, 2], ``point_list`` [R] (Gaussian indices, tile-major, each
    tile in (depth, index) order), ``n_contrib`` [H, W], ``final_T`` [H, W]; int64 / float32 CPU
    tensors.  ``fwd`` is the tuple ``rasterize_gaussians`` returned."""
    num_rendered, color, _radii, geom, binning, img, _inv = fwd
    H, W = int(color.size(1)), int(color.size(2))
    device = color.device
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    i32 = dict(dtype=torch.int32, device=device)
    ranges = torch.zeros((tiles, 2), **i32)
    plist = torch.zeros((max(int(num_rendered), 1),), **i32)
    n_contrib = torch.zeros((H, W), **i32)
    final_T = torch.zeros((H, W), dtype=torch.float32, device=device)
    lib = _lib.load()
    with torch.cuda.device(device):
        rc = lib.gsr_debug_forward_state(int(P), W, H, int(num_rendered), 0, int(binning.numel()), geom.data_ptr(),
                                         binning.data_ptr() if binning.numel() else None, img.data_ptr(),
                                         ranges.data_ptr(), plist.data_ptr(), n_contrib.data_ptr(),
                                         final_T.data_ptr(), _stream_handle(device))
    _lib.check(rc, "debug_forward_state")
    u = lambda t: t.cpu().numpy().view("uint32").astype("int64")  # noqa: E731
    return {"ranges": torch.from_numpy(u(ranges)), "point_list": torch.from_numpy(u(plist)[:int(num_rendered)] >> 4),
            "n_contrib": torch.from_numpy(u(n_contrib)), "final_T": final_T.cpu()}


def debug_sort_state(fwd, P: int) -> dict:
    """The forward's reachable-prefix sort state (include/gsr.h gsr_debug_sort_state): ``sorted_len``
    [tiles] (entries of each tile list in final order) and ``redo_count`` (tiles the forward
    rendered again because a wave passed its sorted prefix); int64 CPU tensor / int."""
    num_rendered, color, _radii, geom, binning, img, _inv = fwd
    H, W = int(color.size(1)), int(color.size(2))
    device = color.device
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    sl = torch.zeros(tiles, dtype=torch.int32, device=device)
    rc = torch.zeros(1, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        r = _lib.load().gsr_debug_sort_state(int(P), W, H, geom.data_ptr(), sl.data_ptr(), rc.data_ptr(),
                                             _stream_handle(device))
    _lib.check(r, "debug_sort_state")
    return {"sorted_len": sl.cpu().long(), "redo_count": int(rc.item())}


def debug_near_state(fwd, P: int) -> dict:
    """The forward's near-first binning state (include/gsr.h gsr_debug_near_state): ``zcut`` (the depth bin
    of its cut, None when there was none) and ``near_len`` [tiles] (entries keyed and sorted per tile;
    the whole list lengths when there was no cut); int / int64 CPU tensor."""
    num_rendered, color, _radii, geom, binning, img, _inv = fwd
    H, W = int(color.size(1)), int(color.size(2))
    device = color.device
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    zc = torch.zeros(1, dtype=torch.int32, device=device)
    nr = torch.zeros((tiles, 2), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        r = _lib.load().gsr_debug_near_state(int(P), W, H, geom.data_ptr(), zc.data_ptr(), nr.data_ptr(),
                                             _stream_handle(device))
    _lib.check(r, "debug_near_state")
    cut = int(zc.item()) & 0xFFFFFFFF
    st = debug_forward_state(fwd, P)
    rg = st["ranges"]
    if cut == 0xFFFFFFFF:
        return {"zcut": None, "near_len": rg[:, 1] - rg[:, 0]}
    n = nr.cpu().numpy().view("uint32").astype("int64")
    return {"zcut": cut, "near_len": torch.from_numpy(n[:, 1] - n[:, 0])}


def view_block_floats(P: int) -> int:
    """Floats in one view block (include/gsr.h, multi-GPU view exchange)."""
    return int(_lib.load().gsr_view_block_floats(int(P)))


def view_pack_floats(entries: int) -> int:
    """Floats of a packed (sparse) view block holding ``entries`` entries (include/gsr.h)."""
    return int(_lib.load().gsr_view_pack_floats(int(entries)))


def _range(P, rng):
    g0, g1 = (0, P) if rng is None else (int(rng[0]), int(rng[1]))
    if not 0 <= g0 <= g1 <= P:
        raise RuntimeError(f"Gaussian range [{g0}, {g1}) outside [0, {P})")
    return g0, g1


def view_block_pack(view_block: torch.Tensor, packed: torch.Tensor, scratch: torch.Tensor, count: torch.Tensor,
                    P: int, rng=None) -> None:
    """Pack a dense view block into ``packed`` (capacity from its size); the entry count lands in
    ``count`` (an int32 device tensor of one element) and in the packed header (include/gsr.h
    gsr_view_block_pack).  Only Gaussians with a non-zero render gradient are kept; with ``rng`` =
    (g0, g1) only those of Gaussians [g0, g1) (one chunk of a chunked exchange)."""
    g0, g1 = _range(P, rng)
    _require_device(view_block, "view_block")
    nb = view_block_floats(P)
    if view_block.numel() != nb or view_block.dtype != torch.float32 or not view_block.is_contiguous():
        raise RuntimeError(f"view_block must be a contiguous float32 tensor of {nb} values")
    cap = (packed.numel() - 64) // 12
    if packed.dtype != torch.float32 or not packed.is_contiguous() or cap < 0:
        raise RuntimeError("packed must be a contiguous float32 tensor of at least 64 values")
    need = int(_lib.load().gsr_view_pack_scratch_bytes(int(P)))
    if scratch.numel() * scratch.element_size() < need or count.numel() != 1 or count.dtype != torch.int32:
        raise RuntimeError("view_block_pack: scratch too small or count not an int32 scalar tensor")
    lib = _lib.load()
    with torch.cuda.device(view_block.device):
        rc = lib.gsr_view_block_pack_range(int(P), g0, g1, view_block.data_ptr(), packed.data_ptr(), int(cap),
                                           scratch.data_ptr(), count.data_ptr(), _stream_handle(view_block.device))
    _lib.check(rc, "view_block_pack")


def view_block_unpack(packed: torch.Tensor, blocks: torch.Tensor, P: int) -> None:
    """Unpack ``packed`` ([n_views, packed_floats]) into dense view blocks ``blocks``
    ([n_views, view_block_floats(P)]; include/gsr.h gsr_view_block_unpack)."""
    _require_device(packed, "packed")
    nb = view_block_floats(P)
    if packed.dim() != 2 or blocks.dim() != 2 or blocks.size(1) != nb or packed.size(0) != blocks.size(0):
        raise RuntimeError(f"packed [n_views, k] and blocks [n_views, {nb}] expected")
    if not (packed.is_contiguous() and blocks.is_contiguous()):
        raise RuntimeError("packed and blocks must be contiguous")
    cap = (packed.size(1) - 64) // 12
    lib = _lib.load()
    with torch.cuda.device(packed.device):
        rc = lib.gsr_view_block_unpack(int(P), int(packed.size(0)), packed.data_ptr(), int(packed.size(1)),
                                       blocks.data_ptr(), int(cap), _stream_handle(packed.device))
    _lib.check(rc, "view_block_unpack")


def view_block_index(packed: torch.Tensor, flags: torch.Tensor, P: int, rng=None) -> None:
    """Index ``packed`` ([n_views, packed_floats]) for ``gauss_backward_views(..., flags=flags)``:
    ``flags`` ([n_views, P] int32) is cleared and, for each packed entry i of view v, flags[v, g] =
    i << 4 | its flag bits (include/gsr.h gsr_view_block_index); with ``rng`` = (g0, g1) only the
    flags of Gaussians [g0, g1) (the packed blocks of one chunk)."""
    g0, g1 = _range(P, rng)
    _require_device(packed, "packed")
    if packed.dim() != 2 or flags.dim() != 2 or tuple(flags.shape) != (packed.size(0), P):
        raise RuntimeError(f"packed [n_views, k] and flags [n_views, {P}] expected")
    if flags.dtype != torch.int32 or not (packed.is_contiguous() and flags.is_contiguous()):
        raise RuntimeError("packed (float32) and flags (int32) must be contiguous")
    cap = (packed.size(1) - 64) // 12
    lib = _lib.load()
    with torch.cuda.device(packed.device):
        rc = lib.gsr_view_block_index_range(int(P), g0, g1, int(packed.size(0)), packed.data_ptr(),
                                            int(packed.size(1)), flags.data_ptr(), int(cap),
                                            _stream_handle(packed.device))
    _lib.check(rc, "view_block_index")


def views_live_floats(P: int) -> int:
    """int32 words of a live-list buffer for ``views_live_list`` (include/gsr.h)."""
    return int(_lib.load().gsr_views_live_floats(int(P)))


def views_live_list(flags: torch.Tensor, live: torch.Tensor, P: int, rng=None) -> None:
    """The Gaussians some view flags (``flags`` from ``view_block_index``) into ``live``
    (int32, ``views_live_floats(P)`` words), for ``gauss_backward_views(..., live=live)``; with
    ``rng`` = (g0, g1) only Gaussians [g0, g1)."""
    g0, g1 = _range(P, rng)
    _require_device(flags, "flags")
    if flags.dim() != 2 or flags.size(1) != P or flags.dtype != torch.int32 or not flags.is_contiguous():
        raise RuntimeError(f"flags must be a contiguous int32 [n_views, {P}] tensor")
    if live.dtype != torch.int32 or live.numel() < views_live_floats(P) or not live.is_contiguous():
        raise RuntimeError(f"live must be a contiguous int32 tensor of {views_live_floats(P)} words")
    lib = _lib.load()
    with torch.cuda.device(flags.device):
        rc = lib.gsr_views_live_list_range(int(P), g0, g1, int(flags.size(0)), flags.data_ptr(), live.data_ptr(),
                                           _stream_handle(flags.device))
    _lib.check(rc, "views_live_list")


def rasterize_gaussians_backward_screen(*args, view_block: torch.Tensor) -> None:
    """The backward of ``rasterize_gaussians_backward`` up to the per-Gaussian render-gradient
    sums, written with the camera into ``view_block`` (a float32 tensor of
    ``view_block_floats(P)`` values; include/gsr.h ``gsr_backward_args.view_block``).
    Arguments as ``rasterize_gaussians_backward`` (24, or 25 with ``dc``); colours from SH and
    cov3D from scales / rotations.  The rest of the backward, over any number of gathered
    views, is ``gauss_backward_views``."""
    (background, means3D, radii, colors, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
     projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_invdepth, dc, sh, degree, campos, geomBuffer, R,
     binningBuffer, imageBuffer, antialiasing, debug, _accel) = _unpack_backward(
         args, "rasterize_gaussians_backward_screen")
    if _present(colors) or _present(cov3D_precomp):
        raise RuntimeError("rasterize_gaussians_backward_screen: precomputed colours / cov3D are per view; "
                           "use rasterize_gaussians_backward")
    _require_device(means3D, "means3D")
    device = means3D.device
    P = means3D.size(0)
    nb = view_block_floats(P)
    if (view_block.dtype != torch.float32 or not view_block.is_contiguous() or view_block.numel() != nb
            or view_block.device != device):
        raise RuntimeError(f"view_block must be a contiguous float32 tensor of {nb} values on {device}")
    if P == 0:
        return
    H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))
    has_inv = dL_dout_invdepth is not None and dL_dout_invdepth.numel() != 0 and dL_dout_invdepth.size(0) != 0
    ins = _Inputs(device)
    scratch = torch.empty(0, dtype=torch.uint8, device=device)
    rs = _Resizer(scratch)
    _own_geometry(geomBuffer)
    scene, view = _scene_view(
        ins, means3D=means3D, dc=dc, sh=sh, degree=degree, colors=None, opacities=opacities, scales=scales,
        scale_modifier=scale_modifier, rotations=rotations, cov3D_precomp=None, background=background,
        viewmatrix=viewmatrix, projmatrix=projmatrix, campos=campos, tan_fovx=tan_fovx, tan_fovy=tan_fovy, W=W, H=H,
        antialiasing=antialiasing)
    a = _lib.BackwardArgs(
        scene=scene, view=view, R=int(R), radii=ins.radii(radii), geom_buffer=geomBuffer.data_ptr(),
        binning_buffer=binningBuffer.data_ptr() if binningBuffer.numel() else None,
        image_buffer=imageBuffer.data_ptr(), binning_capacity=0, binning_bytes=int(binningBuffer.numel()),
        dL_dpix=ins.req(dL_dout_color, "dL_dout_color"),
        dL_dinvdepths=ins.req(dL_dout_invdepth, "dL_dout_invdepth") if has_inv else None,
        view_block=view_block.data_ptr(), debug=int(bool(debug)), scratch_alloc=rs.cb,
        stream=_stream_handle(device))
    with torch.cuda.device(device):
        rc = _lib.load().gsr_rasterize_backward(ctypes.byref(a))
    _lib.check(rc, "rasterize_gaussians_backward_screen")


def gauss_backward_views(means3D, dc, sh, degree, opacities, scales, rotations, scale_modifier, blocks, out,
                         flags=None, live=None) -> None:
    """The per-Gaussian backward summed over ``blocks`` ([n_views, view_block_floats(P)] float32,
    e.g. an all-gathered exchange buffer), written into ``out`` (names as the ``out=`` of
    ``rasterize_gaussians_backward``: dL_dmeans3D, dL_ddc (when dc is given), dL_dsh,
    dL_dopacity, dL_dscales, dL_drotations; contiguous float32).  With ``flags`` (from
    ``view_block_index``), ``blocks`` are packed blocks ([n_views, packed_floats]) read in place;
    with ``live`` too (``views_live_list``) only the listed Gaussians' rows are written -- the
    caller zeroes ``out`` beforehand."""
    _require_device(means3D, "means3D")
    device = means3D.device
    P = means3D.size(0)
    nb = view_block_floats(P) if flags is None else int(blocks.size(1)) if blocks.dim() == 2 else -1
    if blocks.dim() != 2 or blocks.size(1) != nb or blocks.dtype != torch.float32 or not blocks.is_contiguous():
        raise RuntimeError(f"blocks must be a contiguous float32 [n_views, {nb}] tensor")
    if flags is not None and (tuple(flags.shape) != (blocks.size(0), P) or flags.dtype != torch.int32 or
                              not flags.is_contiguous()):
        raise RuntimeError(f"flags must be a contiguous int32 [{blocks.size(0)}, {P}] tensor")
    M = sh.size(1) if _present(sh) else 0
    need = {"dL_dmeans3D": (P, 3), "dL_dsh": (P, M, 3), "dL_dopacity": (P, 1), "dL_dscales": (P, 3),
            "dL_drotations": (P, 4)}
    if _present(dc):
        need["dL_ddc"] = (P, 1, 3)
    for k, shp in need.items():
        t = out.get(k)
        if t is None or tuple(t.shape) != shp or t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
            raise RuntimeError(f"out[{k}] must be a contiguous float32 {shp} tensor on {device}")
    if P == 0:
        return
    lib = _lib.load()
    ins = _Inputs(device)
    geo = (P, int(degree), M, ins.req(means3D, "means3D"), ins.opt(dc, "dc") if _present(dc) else None,
           ins.opt(sh, "sh"), ins.req(opacities, "opacities"), ins.req(scales, "scales"),
           ins.req(rotations, "rotations", align16=True), float(scale_modifier), int(blocks.size(0)),
           blocks.data_ptr(), nb)
    outs = (out["dL_dmeans3D"].data_ptr(), out["dL_ddc"].data_ptr() if _present(dc) else None,
            out["dL_dsh"].data_ptr() if M > 0 else None, out["dL_dopacity"].data_ptr(), out["dL_dscales"].data_ptr(),
            out["dL_drotations"].data_ptr(), _stream_handle(device))
    with torch.cuda.device(device):
        if flags is None:
            rc = lib.gsr_gauss_backward_views(*geo, *outs)
        elif live is None:
            rc = lib.gsr_gauss_backward_views_packed(*geo, flags.data_ptr(), *outs)
        else:
            rc = lib.gsr_gauss_backward_views_live(*geo, flags.data_ptr(), live.data_ptr(), *outs)
    _lib.check(rc, "gauss_backward_views")


def mark_visible(means3D, viewmatrix, projmatrix) -> torch.Tensor:
    """markVisible (rasterize_points.cu:250-274): bool[P], view-space z > 0.2."""
    _require_device(means3D, "means3D")
    device = means3D.device
    lib = _lib.load()
    P = means3D.size(0)
    present = torch.zeros(P, dtype=torch.bool, device=device)
    if P == 0:
        return present
    ins = _Inputs(device)
    with torch.cuda.device(device):
        rc = lib.gsr_mark_visible(P, ins.req(means3D, "means3D"), ins.req(viewmatrix, "viewmatrix", small=True),
                                  ins.req(projmatrix, "projmatrix", small=True), present.data_ptr(),
                                  _stream_handle(device))
    _lib.check(rc, "mark_visible")
    return present


def adamUpdate(param, param_grad, exp_avg, exp_avg_sq, visible, lr, b1, b2, eps, N, M):
    """The 3DGS-accel build's ``_C.adamUpdate`` (SparseGaussianAdam's per-group call; include/gsr_adam.h)."""
    from .optim import adam_update

    adam_update(param, param_grad, exp_avg, exp_avg_sq, visible, lr, b1, b2, eps, N, M)


# ---- fused SSIM as utils/loss_utils.py:16-37 expects it from this module ------------------
# The reference's loss_utils tries ``from diff_gaussian_rasterization._C import fusedssim,
# fusedssim_backward`` (the 3DGS-accel rasterizer's two-function variant: the forward returns
# only the map, the backward takes the upstream gradient and recomputes what it needs).  Both
# run on the same gfx950 kernels as fused_ssim_cuda (csrc/ssim.hip).
def fusedssim(C1, C2, img1, img2):
    """SSIM map of img1 vs img2 ([C,H,W] or [B,C,H,W], float32, HIP device), 'same' padding."""
    import fused_ssim_cuda

    a, b = (img1.unsqueeze(0), img2.unsqueeze(0)) if img1.dim() == 3 else (img1, img2)
    ssim_map = fused_ssim_cuda.fusedssim(C1, C2, a, b, False)[0]
    return ssim_map[0] if img1.dim() == 3 else ssim_map


def fusedssim_backward(C1, C2, img1, img2, opt_grad):
    """dL/dimg1 given dL/dmap; the derivative maps are recomputed (one extra forward pass)."""
    import fused_ssim_cuda

    squeeze = img1.dim() == 3
    a, b, g = (t.unsqueeze(0) for t in (img1, img2, opt_grad)) if squeeze else (img1, img2, opt_grad)
    _, d1, d2, d3 = fused_ssim_cuda.fusedssim(C1, C2, a, b, True)
    grad = fused_ssim_cuda.fusedssim_backward(C1, C2, a, b, g, d1, d2, d3)
    return grad[0] if squeeze else grad
