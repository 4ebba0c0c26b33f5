"""ctypes binding of libgsr.so (the C ABI in include/gsr.h, gsr_knn.h, gsr_ssim.h).

The library is built in-tree (``python -m gaussian_splatting_amd.build``) and
loaded from ``gaussian_splatting_amd/lib/libgsr.so``.  There is no fallback: if
the library is missing or cannot be loaded, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os
import re
import threading

_PKG = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_PKG, "lib", "libgsr.so")
LIB_PATH = os.environ.get("GSR_LIBRARY", DEFAULT_LIB)
INCLUDE_DIR = os.path.join(os.path.dirname(_PKG), "include")
HEADER_PATH = os.path.join(INCLUDE_DIR, "gsr.h")
HEADERS = [os.path.join(INCLUDE_DIR, h) for h in ("gsr.h", "gsr_knn.h", "gsr_ssim.h", "gsr_adam.h", "gsr_densify.h", "gsr_mcmc.h",
                                                      "gsr_ply.h")]

ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)

_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float

class AdamGroup(ctypes.Structure):
    """gsr_adam_group (include/gsr_adam.h)."""

    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("numel", ctypes.c_longlong), ("M", ctypes.c_int),
                ("lr", ctypes.c_float), ("eps", ctypes.c_float)]


class DensifyGroup(ctypes.Structure):
    """gsr_densify_group (include/gsr_densify.h)."""

    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("src_exp_avg", ctypes.c_void_p),
                ("src_exp_avg_sq", ctypes.c_void_p), ("dst_exp_avg", ctypes.c_void_p),
                ("dst_exp_avg_sq", ctypes.c_void_p), ("width", ctypes.c_int), ("role", ctypes.c_int)]


class McmcGroup(ctypes.Structure):
    """gsr_mcmc_group (include/gsr_mcmc.h)."""

    _fields_ = [("data", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("width", ctypes.c_int), ("role", ctypes.c_int)]


class DensifyParams(ctypes.Structure):
    """gsr_densify_params (include/gsr_densify.h)."""

    _fields_ = [("grad_threshold", ctypes.c_float), ("clone_extent", ctypes.c_float),
                ("min_opacity", ctypes.c_float), ("big_extent", ctypes.c_float), ("use_screen_size", ctypes.c_int),
                ("split_n", ctypes.c_int), ("split_div", ctypes.c_float)]


# The rasterizer's argument structs (include/gsr.h); tests/test_abi_layout.py holds every field's offset and size
# against a C program's offsetof / sizeof.
class Scene(ctypes.Structure):
    """gsr_scene."""

    _fields_ = [("P", _i), ("D", _i), ("M", _i), ("means3D", _vp), ("dc", _vp), ("shs", _vp),
                ("colors_precomp", _vp), ("opacities", _vp), ("scales", _vp), ("scale_modifier", _f),
                ("rotations", _vp), ("cov3D_precomp", _vp)]


class View(ctypes.Structure):
    """gsr_view."""

    _fields_ = [("width", _i), ("height", _i), ("background", _vp), ("viewmatrix", _vp), ("projmatrix", _vp),
                ("campos", _vp), ("tan_fovx", _f), ("tan_fovy", _f), ("antialiasing", _i)]


class _Args(ctypes.Structure):
    """An argument struct whose first field is its own sizeof (the struct_size rule of include/gsr.h)."""

    def __init__(self, **fields):
        super().__init__(struct_size=ctypes.sizeof(self), **fields)


class ForwardArgs(_Args):
    """gsr_forward_args."""

    _fields_ = [("struct_size", ctypes.c_size_t), ("scene", Scene), ("view", View),
                ("geom_alloc", ALLOC_FN), ("geom_ctx", _vp), ("binning_alloc", ALLOC_FN), ("binning_ctx", _vp),
                ("image_alloc", ALLOC_FN), ("image_ctx", _vp), ("prefiltered", _i), ("debug", _i), ("stream", _vp),
                ("out_color", _vp), ("out_invdepth", _vp), ("radii", _vp), ("capacity_hint", _i),
                ("num_rendered", _i), ("binning_capacity", _i)]


class BackwardArgs(_Args):
    """gsr_backward_args."""

    _fields_ = [("struct_size", ctypes.c_size_t), ("scene", Scene), ("view", View), ("R", _i), ("radii", _vp),
                ("geom_buffer", _vp), ("binning_buffer", _vp), ("image_buffer", _vp), ("binning_capacity", _i),
                ("binning_bytes", ctypes.c_size_t), ("dL_dpix", _vp), ("dL_dinvdepths", _vp), ("dL_dalphas", _vp),
                ("dL_dmean2D", _vp), ("dL_dmean2D_abs", _vp), ("dL_dconic", _vp), ("dL_dopacity", _vp),
                ("dL_dcolor", _vp), ("dL_dinvdepth", _vp), ("dL_dmean3D", _vp), ("dL_dcov3D", _vp), ("dL_ddc", _vp),
                ("dL_dsh", _vp), ("dL_dscale", _vp), ("dL_drot", _vp), ("view_block", _vp), ("debug", _i),
                ("scratch_alloc", ALLOC_FN), ("scratch_ctx", _vp), ("stream", _vp)]


# argument lists, in include/gsr.h order
SIGNATURES = {
    "gsr_rasterize_forward": (_i, [ctypes.POINTER(ForwardArgs)]),
    "gsr_rasterize_backward": (_i, [ctypes.POINTER(BackwardArgs)]),
    "gsr_render_alpha": (_i, [_i, _i, _vp, _vp, _vp]),
    "gsr_contrib_stats": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _i, ctypes.c_size_t, _vp, _i, _vp, _vp]),
    "gsr_render_features": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _i, ctypes.c_size_t, _vp, _vp, _vp]),
    "gsr_render_features_backward": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _i, ctypes.c_size_t, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _vp, _vp, _f, _f, _i, _vp, ALLOC_FN, _vp, _vp]),
    "gsr_render_features_chunk": (_i, []),
    "gsr_render_distortion": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _i, ctypes.c_size_t, _vp, _vp, _vp, _vp]),
    "gsr_render_distortion_backward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _i, ctypes.c_size_t, _vp, _vp, _vp, _vp,
                                            _vp, _vp, _vp, _vp, _vp, _f, _f, _i, _vp, ALLOC_FN, _vp, _vp]),
    "gsr_render_select": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _i, ctypes.c_size_t, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "gsr_render_select_max_k": (_i, []),
    "gsr_render_median_backward": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "gsr_camera_backward": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _f, _f,
                                 _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, ALLOC_FN, _vp, _vp, _vp, _vp, _vp]),
    "gsr_mark_visible": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
    "gsr_view_block_floats": (ctypes.c_ulonglong, [_i]),
    "gsr_view_pack_floats": (ctypes.c_ulonglong, [ctypes.c_longlong]),
    "gsr_view_pack_scratch_bytes": (ctypes.c_ulonglong, [_i]),
    "gsr_view_block_pack": (_i, [_i, _vp, _vp, ctypes.c_longlong, _vp, _vp, _vp]),
    "gsr_view_block_pack_range": (_i, [_i, _i, _i, _vp, _vp, ctypes.c_longlong, _vp, _vp, _vp]),
    "gsr_view_block_index_range": (_i, [_i, _i, _i, _i, _vp, ctypes.c_longlong, _vp, ctypes.c_longlong, _vp]),
    "gsr_views_live_list_range": (_i, [_i, _i, _i, _i, _vp, _vp, _vp]),
    "gsr_view_block_unpack": (_i, [_i, _i, _vp, ctypes.c_longlong, _vp, ctypes.c_longlong, _vp]),
    "gsr_view_block_index": (_i, [_i, _i, _vp, ctypes.c_longlong, _vp, ctypes.c_longlong, _vp]),
    "gsr_views_live_floats": (ctypes.c_ulonglong, [_i]),
    "gsr_views_live_list": (_i, [_i, _i, _vp, _vp, _vp]),
    "gsr_gauss_backward_views": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _vp, ctypes.c_longlong, _vp,
                                      _vp, _vp, _vp, _vp, _vp, _vp]),
    "gsr_gauss_backward_views_packed": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _vp, ctypes.c_longlong,
                                             _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gsr_gauss_backward_views_live": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _vp, ctypes.c_longlong,
                                           _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gsr_debug_forward_state": (_i, [_i, _i, _i, _i, _i, ctypes.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gsr_forward_rebuilds": (ctypes.c_longlong, []),
    "gsr_debug_sort_state": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "gsr_debug_near_state": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "gsr_option_set": (_i, [ctypes.c_char_p, _i]),
    "gsr_host_stats": (_i, [ctypes.POINTER(ctypes.c_double), _i, _i]),
    "gsr_option_get": (_i, [ctypes.c_char_p]),
    "gsr_option_set_thread": (_i, [ctypes.c_char_p, _i]),
    "gsr_option_clear_thread": (_i, [ctypes.c_char_p]),
    "gsr_geom_forget": (_i, [_vp]),
    "gsr_last_error": (ctypes.c_char_p, []),
    "gsr_version": (ctypes.c_char_p, []),
    "gsr_build_id": (ctypes.c_char_p, []),
    "gsr_profile_enable": (_i, [_i]),
    "gsr_profile_collect": (_i, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong), _i]),
    "gsr_profile_reset": (None, []),
    "gsr_census_set": (_i, [ctypes.c_void_p]),
    "gsr_profile_stage_name": (ctypes.c_char_p, [_i]),
    "gsr_knn_mean_dist2": (_i, [_i, _vp, _vp, ALLOC_FN, _vp, _vp]),
    "gsr_fused_ssim_forward": (_i, [_i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gsr_fused_ssim_backward": (_i, [_i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gsr_adam_update": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _i, _i, _vp]),
    "gsr_adam_update_multi": (_i, [ctypes.POINTER(AdamGroup), _i, _vp, _i, _f, _f, _vp]),
    "gsr_densify_stats": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gsr_densify_scratch_bytes": (ctypes.c_ulonglong, [_i]),
    "gsr_densify_plan": (_i, [_i, _vp, _vp, _vp, _vp, ctypes.POINTER(DensifyParams), _vp, _vp,
                              ctypes.POINTER(ctypes.c_longlong), _vp]),
    "gsr_densify_apply": (_i, [_i, _vp, ctypes.POINTER(DensifyGroup), _i, _vp, _vp, _vp, _vp,
                               ctypes.POINTER(DensifyParams), _vp]),
    "gsr_mcmc_noise": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _f, _vp]),
    "gsr_mcmc_scratch_bytes": (ctypes.c_ulonglong, [_i]),
    "gsr_mcmc_relocation": (_i, [_i, _i, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "gsr_mcmc_apply": (_i, [_i, _i, _vp, _vp, _vp, _vp, ctypes.POINTER(McmcGroup), _i, _vp]),
    "gsr_ply_open": (_i, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]),
    "gsr_ply_close": (None, [_vp]),
    "gsr_ply_vertex_count": (ctypes.c_longlong, [_vp]),
    "gsr_ply_property_count": (_i, [_vp]),
    "gsr_ply_property_name": (ctypes.c_char_p, [_vp, _i]),
    "gsr_ply_property_type": (_i, [_vp, _i, ctypes.POINTER(_i), ctypes.POINTER(ctypes.c_char)]),
    "gsr_ply_read_raw": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_void_p),
                              ctypes.POINTER(ctypes.c_longlong)]),
    "gsr_ply_read_float": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_void_p),
                                ctypes.POINTER(ctypes.c_longlong)]),
    "gsr_ply_write": (_i, [ctypes.c_char_p, ctypes.c_longlong, _i, ctypes.POINTER(ctypes.c_char_p), ctypes.c_char_p,
                           ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_longlong)]),
}

_lock = threading.Lock()
_lib = None


class GsrError(RuntimeError):
    """A failure reported by libgsr (the reference raises RuntimeError / AT_ERROR too)."""


def header_symbols(paths=None) -> list:
    """Function names declared in the C ABI headers (include/gsr.h, include/gsr_knn.h)."""
    names = set()
    for path in ([paths] if isinstance(paths, str) else (paths or HEADERS)):
        with open(path) as f:
            names |= set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", f.read()))
    return sorted(names - {"gsr_alloc_fn"})


def load():
    """Load libgsr.so once; raises GsrError if it is missing (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise GsrError(f"libgsr.so not found at {LIB_PATH}; build it with "
                           "`python -m gaussian_splatting_amd.build` (hipcc, gfx950)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if LIB_PATH == DEFAULT_LIB and os.environ.get("GSR_SKIP_BUILD_ID_CHECK", "0") != "1":
            # the in-tree library must be the build of THIS tree's sources (build.py input_hash)
            from gaussian_splatting_amd import build as _build

            got = lib.gsr_build_id().decode()
            try:
                want = _build.input_hash()
            except OSError as e:  # an install without the csrc sources: nothing to compare with
                import warnings

                warnings.warn(f"libgsr build-id check skipped: the sources are not readable ({e})")
                want = got
            if got != want:
                raise GsrError(f"{LIB_PATH} was built from other sources (build id {got[:16]}, this tree "
                               f"{want[:16]}); rebuild it with `python -m gaussian_splatting_amd.build`")
        _lib = lib
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().gsr_last_error().decode(errors="replace")
        raise GsrError(f"{what} failed (code {rc}): {msg}")


def version() -> str:
    return load().gsr_version().decode()


def build_id() -> str:
    """sha256 of the sources and flags the loaded library was compiled from (include/gsr.h gsr_build_id)."""
    return load().gsr_build_id().decode()


# ---- runtime options (include/gsr.h gsr_option_set) ---------------------------------
OPTIONS = ("fused_bin", "fwd_quads", "bwd_seg_ck", "host_total", "zero_fill", "live_list", "sort_prefix",
           "count_wait", "bwd_grid", "bwd_atomic", "near_mass", "touched_run")


def option_get(name: str) -> int:
    v = int(load().gsr_option_get(name.encode()))
    if v < 0:
        raise GsrError(f"unknown libgsr option {name!r}")
    return v


def option_set(name: str, value: int) -> None:
    check(load().gsr_option_set(name.encode(), int(value)), "option_set")


class thread_options:
    """Context manager: options for the library calls THIS thread makes in the block (include/gsr.h
    gsr_option_set_thread), over the process-wide values; the overrides are cleared on exit (no nesting)."""

    def __init__(self, **values):
        self.values = values

    def __enter__(self):
        lib = load()
        for k, v in self.values.items():
            check(lib.gsr_option_set_thread(k.encode(), int(v)), "option_set_thread")
        return self

    def __exit__(self, *exc):
        lib = load()
        for k in self.values:
            lib.gsr_option_clear_thread(k.encode())


class options:
    """Context manager: set libgsr options for a block and restore them afterwards.

        with _lib.options(zero_fill=2, live_list=0):
            ...
    """

    def __init__(self, **values):
        self.values = values
        self.saved = {}

    def __enter__(self):
        for k, v in self.values.items():
            self.saved[k] = option_get(k)
            option_set(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            option_set(k, v)
        return False


def host_stats(reset: bool = False) -> dict:
    """Host-side statistics of the library (include/gsr.h gsr_host_stats): for the forwards' count
    waits, whole forward calls and whole backward calls, {calls, total_ms, max_ms}."""
    v = (ctypes.c_double * 9)()
    load().gsr_host_stats(v, 9, int(bool(reset)))
    return {k: {"calls": int(v[3 * i]), "total_ms": v[3 * i + 1], "max_ms": v[3 * i + 2]}
            for i, k in enumerate(("count_wait", "forward", "backward"))}


# ---- stage profiler ---------------------------------------------------------------
def stage_names() -> list:
    lib = load()
    out, i = [], 0
    while True:
        n = lib.gsr_profile_stage_name(i).decode()
        if not n:
            return out
        out.append(n)
        i += 1


def profile_enable(on: bool = True, stages=None) -> None:
    """Time all stages (stages=None) or only the named ones; on=False turns timing off."""
    if not on:
        mask = 0
    elif stages is None:
        mask = -1
    else:
        names = stage_names()
        mask = 0
        for s in stages:
            mask |= 1 << names.index(s)
    load().gsr_profile_enable(mask)


def profile_reset() -> None:
    load().gsr_profile_reset()


def profile_collect() -> dict:
    """Per-stage (total_ms, calls) accumulated since the last reset."""
    lib = load()
    n = 32
    ms = (ctypes.c_double * n)()
    calls = (ctypes.c_longlong * n)()
    k = lib.gsr_profile_collect(ms, calls, n)
    return {lib.gsr_profile_stage_name(i).decode(): (ms[i], calls[i]) for i in range(k)}


# ---- census (include/gsr.h "Census"): work counts of the render kernels ----------------------
CENSUS_NAMES = ("fwd_entries_staged", "fwd_quadrant_evals", "fwd_pairs_alpha", "fwd_pairs_blended",
                "bwd_entries_staged", "bwd_quadrant_evals", "bwd_pairs_grad", "bwd_entry_reductions",
                "bwd_evals_idle", "fwd_evals_idle")


def census(fn, device=None) -> dict:
    """Run ``fn()`` (forward / backward calls) with the census render kernels and return the counts
    it added.  Diagnostic only: the census kernels are slower than the production ones."""
    import torch

    buf = torch.zeros(len(CENSUS_NAMES), dtype=torch.int64, device=device or "cuda")
    lib = load()
    torch.cuda.synchronize()
    lib.gsr_census_set(ctypes.c_void_p(buf.data_ptr()))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.gsr_census_set(None)
    return dict(zip(CENSUS_NAMES, (int(v) for v in buf.cpu().tolist())))
