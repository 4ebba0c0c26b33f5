"""Shared helpers for the parity tests: small seeded scenes, the oracle call and the
GPU call with the same arguments, and comparison utilities."""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from gaussian_splatting_amd import synthetic as syn


@dataclass
class Case:
    """One rasterizer invocation, in the positional vocabulary of _C.rasterize_gaussians."""

    name: str
    P: int
    W: int
    H: int
    focal: float = 60.0
    sh_degree: int = 3
    M: Optional[int] = None  # SH coefficients stored (default (max degree 3 + 1)^2 = 16)
    mode_color: str = "sh"  # "sh" | "precomp"
    mode_cov: str = "scalerot"  # "scalerot" | "precomp"
    antialiasing: bool = False
    bg: tuple = (0.0, 0.0, 0.0)
    scale_modifier: float = 1.0
    yaw: float = 0.0
    seed: int = 0
    scale_range: tuple = (0.02, 0.25)
    z_range: tuple = (2.0, 8.0)
    opacity_std: float = 1.5
    extra: dict = field(default_factory=dict)
    # general camera pose (make_pose_camera); any of these makes the case a pose case, whose scene is generated
    # in the camera's own frame and mapped to world space by the camera-to-world pose
    pitch: float = 0.0
    roll: float = 0.0
    center: Optional[tuple] = None  # camera centre in world space (pose cases: default the origin)
    focal_y: Optional[float] = None  # default: focal (square pixels)
    principal: tuple = (0.0, 0.0)  # added to P[0,2], P[1,2] (NDC units)
    xy_spread: float = 1.1  # the scene spans +-xy_spread * tanfov * z


def is_pose_case(case: Case) -> bool:
    return (case.pitch != 0.0 or case.roll != 0.0 or case.center is not None or case.focal_y is not None
            or tuple(case.principal) != (0.0, 0.0))


def pose_rotation(yaw: float, pitch: float, roll: float) -> np.ndarray:
    """Camera-to-world rotation Ry(yaw) Rx(pitch) Rz(roll), degrees, float64; Ry is make_camera's."""
    cy, sy = math.cos(math.radians(yaw)), math.sin(math.radians(yaw))
    cx, sx = math.cos(math.radians(pitch)), math.sin(math.radians(pitch))
    cz, sz = math.cos(math.radians(roll)), math.sin(math.radians(roll))
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    return Ry @ Rx @ Rz


def make_pose_camera(W, H, fx, fy, yaw, pitch, roll, center, principal=(0, 0)) -> syn.Camera:
    """A pinhole camera at ``center`` (world space) with camera-to-world rotation Ry Rx Rz (degrees), focal lengths
    fx != fy in pixels and a principal-point offset, by the conventions of synthetic.make_camera:
    viewmatrix = getWorld2View2(R, T)^T, projmatrix = viewmatrix @ P^T, campos = inverse(viewmatrix)[3, :3]."""
    fovx = 2 * math.atan(W / (2 * fx))  # focal2fov
    fovy = 2 * math.atan(H / (2 * fy))
    R_c2w = pose_rotation(yaw, pitch, roll)
    T = -R_c2w.T @ np.asarray(center, np.float64)
    wv = torch.tensor(syn.world2view(R_c2w, T)).transpose(0, 1).contiguous()
    P = syn.projection(syn.ZNEAR, syn.ZFAR, fovx, fovy)
    P[0, 2] += principal[0]
    P[1, 2] += principal[1]
    pm = torch.tensor(P).transpose(0, 1)
    full = (wv.unsqueeze(0).bmm(pm.unsqueeze(0))).squeeze(0).contiguous()
    campos = wv.inverse()[3, :3].contiguous()
    return syn.Camera(W, H, math.tan(fovx * 0.5), math.tan(fovy * 0.5), wv, full, campos)


def case_pose(case: Case):
    """(camera-to-world rotation [3,3] float64, camera centre [3] float64) of a case's camera."""
    if not is_pose_case(case):  # make_camera: yawed about +y around (0, 0, 7)
        R = pose_rotation(case.yaw, 0.0, 0.0)
        return R, np.array([0.0, 0.0, 7.0]) + R @ np.array([0.0, 0.0, -7.0])
    return pose_rotation(case.yaw, case.pitch, case.roll), np.asarray(case.center or (0.0, 0.0, 0.0), np.float64)


def case_camera(case: Case) -> syn.Camera:
    if not is_pose_case(case):
        return syn.make_camera(case.W, case.H, case.focal, case.yaw)
    center = case_pose(case)[1]
    return make_pose_camera(case.W, case.H, case.focal, case.focal_y if case.focal_y is not None else case.focal,
                            case.yaw, case.pitch, case.roll, center, case.principal)


def camera_frame_scene(case: Case, cam: syn.Camera) -> syn.Scene:
    """synthetic.make_scene's recipe (same draws in the same order) with xy_spread in place of 1.1, in the frame of
    ``cam`` (x, y within +-xy_spread * tanfov * z, z in z_range)."""
    P = case.P
    g = torch.Generator().manual_seed(case.seed)
    z = torch.empty(P).uniform_(case.z_range[0], case.z_range[1], generator=g)
    x = torch.empty(P).uniform_(-case.xy_spread, case.xy_spread, generator=g) * cam.tanfovx * z
    y = torch.empty(P).uniform_(-case.xy_spread, case.xy_spread, generator=g) * cam.tanfovy * z
    means = torch.stack([x, y, z], 1)
    lo, hi = math.log(case.scale_range[0]), math.log(case.scale_range[1])
    scales = torch.exp(torch.empty(P, 3).uniform_(lo, hi, generator=g))
    rots = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=1)
    opac = torch.sigmoid(torch.randn(P, 1, generator=g) * case.opacity_std)
    shs = torch.randn(P, 16, 3, generator=g) * 0.05
    shs[:, 0, :] = torch.randn(P, 3, generator=g) * 0.5
    return syn.Scene(means.contiguous(), shs.contiguous(), opac.contiguous(), scales.contiguous(), rots.contiguous(), 3)


def to_world(means_cam: torch.Tensor, R_c2w: np.ndarray, center: np.ndarray) -> torch.Tensor:
    """Camera-frame points to world space (float64 arithmetic, stored float32)."""
    return torch.from_numpy((means_cam.double().numpy() @ R_c2w.T + center).astype(np.float32)).contiguous()


def build(case: Case):
    """Inputs as torch CPU float32 tensors (scene + camera + settings)."""
    cam = case_camera(case)
    if is_pose_case(case):
        sc = camera_frame_scene(case, cam)
        sc.means3D = to_world(sc.means3D, *case_pose(case))
    elif case.xy_spread != 1.1:
        sc = camera_frame_scene(case, syn.make_camera(case.W, case.H, case.focal, 0.0))
    else:
        base = syn.make_camera(case.W, case.H, case.focal, 0.0)
        sc = syn.make_scene(case.P, base, sh_degree=3, seed=case.seed, scale_range=case.scale_range,
                            opacity_std=case.opacity_std, z_range=case.z_range)
    M = case.M if case.M is not None else 16
    shs = sc.shs[:, :M, :].contiguous()
    inp = dict(
        bg=torch.tensor(case.bg, dtype=torch.float32),
        means3D=sc.means3D, opacities=sc.opacities, shs=shs, sh_degree=case.sh_degree,
        scales=sc.scales, rotations=sc.rotations, colors_precomp=None, cov3D_precomp=None,
        viewmatrix=cam.viewmatrix, projmatrix=cam.projmatrix, campos=cam.campos,
        tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, H=case.H, W=case.W, scale_modifier=case.scale_modifier,
        antialiasing=case.antialiasing,
    )
    if case.mode_color == "precomp":
        g = torch.Generator().manual_seed(case.seed + 7)
        inp["colors_precomp"] = torch.rand(case.P, 3, generator=g)
        inp["shs"] = None
    if case.mode_cov == "precomp":
        inp["cov3D_precomp"] = cov3d_reference(sc.scales * case.scale_modifier, sc.rotations)
        inp["scales"] = None
        inp["rotations"] = None
    return inp


def cov3d_reference(s: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """build_scaling_rotation + strip_symmetric (utils/general_utils.py:78-110), restated on CPU."""
    q = torch.nn.functional.normalize(r, dim=1)
    w, x, y, z = q.unbind(1)
    R = torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    L = R * s[:, None, :]
    S = L @ L.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).contiguous()


def run_oracle(inp, precision="f32", nthreads=1):
    from oracle import oracle

    return oracle.forward(
        inp["means3D"], inp["opacities"], inp["viewmatrix"], inp["projmatrix"], inp["campos"], inp["tanfovx"],
        inp["tanfovy"], inp["H"], inp["W"], bg=inp["bg"], shs=inp["shs"], sh_degree=inp["sh_degree"],
        colors_precomp=inp["colors_precomp"], scales=inp["scales"], rotations=inp["rotations"],
        cov3D_precomp=inp["cov3D_precomp"], scale_modifier=inp["scale_modifier"],
        antialiasing=inp["antialiasing"], precision=precision, nthreads=nthreads)


def _dev(t, device):
    return torch.Tensor([]) if t is None else t.to(device)


def run_gpu_forward(inp, device="cuda", prefiltered=False, debug=False):
    from gaussian_splatting_amd import _C

    d = lambda k: _dev(inp[k], device)  # noqa: E731
    return _C.rasterize_gaussians(
        d("bg"), d("means3D"), d("colors_precomp"), d("opacities"), d("scales"), d("rotations"),
        inp["scale_modifier"], d("cov3D_precomp"), d("viewmatrix"), d("projmatrix"), inp["tanfovx"],
        inp["tanfovy"], inp["H"], inp["W"], d("shs"), inp["sh_degree"], d("campos"), prefiltered,
        inp["antialiasing"], debug)


def run_gpu_backward(inp, fwd, grad_color, grad_invdepth, device="cuda", debug=False, out=None):
    from gaussian_splatting_amd import _C

    d = lambda k: _dev(inp[k], device)  # noqa: E731
    num_rendered, color, radii, geom, binning, img, invdepth = fwd
    gi = torch.Tensor([]) if grad_invdepth is None else grad_invdepth.to(device)
    return _C.rasterize_gaussians_backward(
        d("bg"), d("means3D"), radii, d("colors_precomp"), d("opacities"), d("scales"), d("rotations"),
        inp["scale_modifier"], d("cov3D_precomp"), d("viewmatrix"), d("projmatrix"), inp["tanfovx"],
        inp["tanfovy"], grad_color.to(device), gi, d("shs"), inp["sh_degree"], d("campos"), geom, num_rendered,
        binning, img, inp["antialiasing"], debug, out=out)


GRAD_NAMES = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
              "dL_drotations"]


def rel_err(a: np.ndarray, b: np.ndarray) -> float:
    """max |a-b| / max(|b|, tiny): a scale-free error for gradient tensors."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    den = max(np.abs(b).max(), 1e-30)
    return float(np.abs(a - b).max() / den)


def unit_grads(H, W, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3, H, W, generator=g), torch.randn(1, H, W, generator=g)


def l1_grads(H, W, seed=3):
    return syn.upstream_grads(H, W, seed)


SMALL_CASES = [
    Case("sh3_scalerot", P=300, W=64, H=48),
    Case("ragged_37x23", P=120, W=37, H=23, focal=30.0),
    Case("sh1_of_16", P=250, W=64, H=64, sh_degree=1),
    Case("sh0_M1", P=250, W=48, H=40, sh_degree=0, M=1),
    Case("sh2_M9", P=250, W=48, H=40, sh_degree=2, M=9),
    Case("colors_precomp", P=300, W=64, H=48, mode_color="precomp"),
    Case("cov3d_precomp", P=300, W=64, H=48, mode_cov="precomp"),
    Case("antialiasing", P=300, W=64, H=48, antialiasing=True),
    Case("background", P=200, W=64, H=48, bg=(0.2, 0.5, 0.9)),
    Case("scale_modifier", P=200, W=64, H=48, scale_modifier=0.7),
    Case("yawed_view", P=300, W=64, H=48, yaw=15.0),
    Case("dense_opaque", P=2000, W=64, H=64, opacity_std=3.0, scale_range=(0.05, 0.3)),
    # tile lists past one wave's sort (binning.hip K4 classes): (1024, 2048], (2048, 4096], (4096, 8192],
    # > 8192 entries
    Case("lists_1k_2k", P=1800, W=32, H=32, scale_range=(0.1, 0.4)),
    Case("lists_2k_4k", P=5000, W=32, H=32, scale_range=(0.1, 0.4)),
    Case("lists_4k_8k", P=10000, W=32, H=32, scale_range=(0.1, 0.4)),
    Case("lists_over_8k", P=10000, W=16, H=16, scale_range=(0.1, 0.4)),
]

# General camera poses (tests/golden/camera_pose.npz pins make_pose_camera against the reference's own Python).
# A separate list: tests index SMALL_CASES by position.
_GENERAL = dict(P=300, W=64, H=48, yaw=-18.0, pitch=12.0, roll=25.0, center=(0.3, -0.4, 0.2), focal=60.0, focal_y=75.0)
POSE_CASES = [
    Case("pose_general", **_GENERAL),
    Case("pose_roll90", P=300, W=64, H=48, roll=90.0),  # the view rotation is a signed permutation
    Case("pose_pitch", P=300, W=64, H=48, pitch=20.0, center=(0.0, 0.5, 0.0)),
    Case("pose_aniso_focal", P=300, W=64, H=48, focal=50.0, focal_y=80.0),  # identity pose
    Case("pose_back", P=300, W=64, H=48, yaw=160.0, pitch=-10.0),  # viewmatrix[10] < 0
    Case("pose_principal", principal=(0.2, -0.1), **_GENERAL),
    Case("pose_clamped", xy_spread=1.6, **_GENERAL),  # x/z, y/z beyond 1.3 tanfov (tests assert it)
    Case("pose_general_aa", antialiasing=True, **_GENERAL),
    Case("pose_general_cov3d", mode_cov="precomp", **_GENERAL),
    Case("pose_general_precomp", mode_color="precomp", **_GENERAL),
    Case("pose_general_sh1", sh_degree=1, **_GENERAL),  # M = 16, D < 3: the global-memory SH path
]


# Depth-layer scenes: depths that cluster in a sliver of their range, tie exactly, or span the whole key range --
# what the per-tile bucket sort (binning.hip) gives to its fallback networks, and the near-first cut's histogram
# sees in one bin.  Built by build_depth from Case.extra["layers"]: (amount, z0, width[, "log"]) per layer, amount
# a fraction of P (float), a count (int) or None (every Gaussian not yet taken); the layer's Gaussians get the
# depth z0 + U[0, width) ("log": log-uniform in [z0, width]).  tests/test_depth_skew_ref.py proves from the
# oracle and tests/sort_model.py what each scene reaches; tests/test_gpu_depth_skew.py runs them.
# A separate list: tests index SMALL_CASES by position.
_OUTLIERS = [(0.0025, 2.0, 0.5), (0.0025, 40.0, 10.0)]
_WALL = dict(W=64, H=64, scale_range=(0.03, 0.15), extra=dict(layers=_OUTLIERS + [(None, 5.0, 1e-4)]))
_WALL8 = dict(W=32, H=32, scale_range=(0.1, 0.4), extra=dict(layers=[(4, 2.0, 0.5), (4, 40.0, 10.0), (None, 5.0, 1e-4)]))
_FG_WALL = dict(W=32, H=32, scale_range=(0.1, 0.4),
                extra=dict(layers=[(0.004, 2.0, 0.1), (0.001, 40.0, 10.0), (None, 5.0, 1e-4)]))
DEPTH_CASES = [
    Case("wall_129_256", P=1500, **_WALL),    # tile_sort_kernel's fallbacks: sort_list<64, 4>,
    Case("wall_257_512", P=4000, **_WALL),    # sort_list<64, 8>
    Case("wall_513_1024", P=8000, **_WALL),   # and sort_list<64, 16>
    Case("wall_class0_1k", P=1800, **_WALL8),  # long lists (1024, 4096]: the keys in registers
    Case("wall_class0_3k", P=5000, **_WALL8),
    Case("wall_class1", P=10000, W=16, H=16, scale_range=(0.1, 0.4), extra=_WALL8["extra"]),  # one list of 10000
    # runs of equal depth: the index bits order them (seed 1: with seed 0 the f32 oracle's n_contrib differs from
    # the f64 oracle's at one pixel, and the GPU tests hold these scenes to exact bars)
    Case("wall_equal", P=5000, W=32, H=32, scale_range=(0.1, 0.4), seed=1,
         extra=dict(layers=[(4, 2.0, 0.5), (4, 40.0, 10.0), (None, 5.0, 0.0)])),
    Case("moderate_pass", P=5000, W=32, H=32, scale_range=(0.1, 0.4), extra=dict(layers=[(0.10, 5.0, 1e-5)])),
    Case("hot_bin_65536", P=65536 + 8, W=16, H=16,  # one bin of exactly 2^16 keys: its square is 0 mod 2^32
         extra=dict(layers=[(4, 2.0, 0.5), (4, 40.0, 10.0), (65536, 5.0, 0.0)])),
    Case("fg_wall_4k", P=4500, **_FG_WALL),   # a near-first cut between a thin foreground and the wall
    Case("fg_wall_8k", P=8000, **_FG_WALL),
    Case("depth_extremes", P=5000, W=32, H=32, scale_range=(0.1, 0.4), extra=dict(layers=[(None, 0.2005, 3e4, "log")])),
]


def depth_case(name: str) -> Case:
    return next(c for c in DEPTH_CASES if c.name == name)


def build_depth(case: Case):
    """build(case) under the identity camera (view-space depth is world z exactly) with the layers' Gaussians moved
    to their new depths along their view rays: x and y scale by z_new / z_old, so screen positions stay."""
    assert not is_pose_case(case) and case.yaw == 0.0
    inp = build(case)
    means = inp["means3D"].clone()
    g = torch.Generator().manual_seed(case.seed + 1000)
    perm = torch.randperm(case.P, generator=g)
    z_old = means[:, 2].clone()
    z_new = z_old.clone()
    at = 0
    for amount, z0, width, *mode in case.extra["layers"]:
        cnt = case.P - at if amount is None else amount if isinstance(amount, int) else int(round(amount * case.P))
        idx = perm[at:at + cnt]
        at += cnt
        u = torch.rand(cnt, generator=g)
        if mode == ["log"]:
            z_new[idx] = torch.exp(math.log(z0) + u * (math.log(width) - math.log(z0)))
        else:
            z_new[idx] = z0 + u * width  # (float32: a width of 1e-4 at z = 5 leaves ~210 distinct depths)
    assert at <= case.P
    s = z_new / z_old
    inp["means3D"] = torch.stack([means[:, 0] * s, means[:, 1] * s, z_new], 1).contiguous()
    return inp


_DEPTH_REFS: dict = {}


def depth_reference(name: str):
    """(case, inputs, f32 oracle result, per-tile key lists) of a depth-layer scene, computed once per process and
    shared by the tests that use it (read only)."""
    if name not in _DEPTH_REFS:
        from tests import sort_model

        case = depth_case(name)
        inp = build_depth(case)
        ref = run_oracle(inp)
        rb = ref.handle.binning()
        keys = sort_model.tile_keys(ref.handle.geom()["depths"], rb["point_list"], rb["ranges"])
        _DEPTH_REFS[name] = (case, inp, ref, keys)
    return _DEPTH_REFS[name]


def zbin_of(depths) -> np.ndarray:
    """The near-first cut's depth bin of float32 depths (csrc/gsr_common.h zbin: 256 bins of 2^19 float codes from
    0.2, clamped at both ends)."""
    b = (np.ascontiguousarray(depths, dtype=np.float32).view(np.uint32) >> 19).astype(np.int64)
    base = int(np.array([0.2], np.float32).view(np.uint32)[0] >> 19)
    return np.clip(b - base, 0, 255)


def pose_case(name: str) -> Case:
    return next(c for c in POSE_CASES if c.name == name)


def assert_clamp_preconditions(inp, ref):
    """pose_clamped tests something only if visible Gaussians (radius > 0) lie beyond 1.3 tanfov in view-space
    x/z alone, in y/z alone and in both, so that the limx and limy clamps of cov2D (CR/forward.cu:82-90) and the
    x / y gradient masks of its backward each act alone and together.  View-space means are formed here from the
    view matrix in float64 and checked against the oracle's depths."""
    V = inp["viewmatrix"].double().numpy()
    pv = np.concatenate([inp["means3D"].double().numpy(), np.ones((inp["means3D"].shape[0], 1))], 1) @ V[:, :3]
    vis = ref.radii > 0
    np.testing.assert_allclose(pv[vis, 2], ref.handle.geom()["depths"][vis], rtol=1e-5)
    cx = np.abs(pv[:, 0] / pv[:, 2]) > 1.3 * inp["tanfovx"]
    cy = np.abs(pv[:, 1] / pv[:, 2]) > 1.3 * inp["tanfovy"]
    counts = int((vis & cx & ~cy).sum()), int((vis & cy & ~cx).sum()), int((vis & cx & cy).sum())
    assert min(counts) >= 1, counts
    return counts


def rounding_flip_caps(inp, ref32, nthreads=1):
    """Caps for the forward threshold-flip rule (tests/test_gpu_parity.py): how many pixels may lie over 1e-5,
    and how many may end their walk at another contributor, before "every such pixel is explained" stops being
    believable.  Derived from the references alone: the same two counts for the f32 oracle against the f64
    oracle on these inputs -- the flips that rounding alone produces -- times 4, plus 4 pixels, as slack for a
    different but legitimate rounding order.  Returns (cap_over, cap_n_contrib, (oracle_over, oracle_n_contrib))."""
    ref64 = run_oracle(inp, precision="f64", nthreads=nthreads)
    d = np.maximum(np.abs(ref32.color - ref64.color).max(0), np.abs(ref32.invdepth - ref64.invdepth)[0])
    over = int((d > 1e-5).sum())
    nc = int((ref32.handle.image()["n_contrib"] != ref64.handle.image()["n_contrib"]).sum())
    return 4 * over + 4, 4 * nc + 4, (over, nc)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RASTER_FIXTURES = sorted(f[len("raster_"):-len(".npz")] for f in os.listdir(GOLDEN)
                         if f.startswith("raster_") and f.endswith(".npz") and not f.endswith(".images.npz"))


class _Merged(dict):
    files = property(lambda self: list(self))


def load_raster(name):
    """A rasterizer golden vector (tests/golden/make_golden.py): (inp, expected, (grad_color, grad_invdepth)).
    A vector too large for one file keeps its output images beside it in raster_<name>.images.npz."""
    z = _Merged(np.load(os.path.join(GOLDEN, f"raster_{name}.npz")))
    images = os.path.join(GOLDEN, f"raster_{name}.images.npz")
    if os.path.exists(images):
        z.update(np.load(images))
    inp = dict(bg=None, means3D=None, opacities=None, shs=None, sh_degree=0, scales=None, rotations=None,
               colors_precomp=None, cov3D_precomp=None)
    for k in z.files:
        if k.startswith("in_"):
            v = z[k]
            inp[k[3:]] = torch.from_numpy(v.copy()) if v.ndim > 0 else v.item()
    for k in ("H", "W", "sh_degree"):
        inp[k] = int(inp[k])
    for k in ("tanfovx", "tanfovy", "scale_modifier"):
        inp[k] = float(inp[k])
    inp["antialiasing"] = bool(inp["antialiasing"])
    exp = {k[4:]: z[k] for k in z.files if k.startswith("out_")}
    exp["num_rendered"] = int(exp["num_rendered"])
    grads = None
    if "grad_color" in z.files:
        grads = (torch.from_numpy(z["grad_color"].copy()), torch.from_numpy(z["grad_invdepth"].copy()))
    return inp, exp, grads
