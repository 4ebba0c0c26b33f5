"""Generate the golden fixtures under tests/golden/ (run in the build container only).

    python tests/golden/make_golden.py [--reference /root/reference]

Two kinds of vectors, both small .npz files of inputs and expected outputs:

1. REFERENCE vectors -- produced by importing the reference's own Python functions
   (they run on CPU; SURVEY.md section 8c lists them):
     camera.npz   utils/graphics_utils.py:38-71 getWorld2View2 / getProjectionMatrix composed as
                  scene/cameras.py:86-89 (world_view_transform, full_proj_transform, camera_center)
     camera_pose.npz  the same two functions, raw outputs, for the general poses of tests/common.py
                  POSE_CASES (rotation Ry Rx Rz, centre off the origin, fx != fy): pins make_pose_camera
     sh_eval.npz  utils/sh_utils.py:57-112 eval_sh, composed as gaussian_renderer/__init__.py:86-96
                  (convert_SHs_python: colours = clamp_min(eval_sh(...) + 0.5, 0))
     l1_grad.npz  utils/loss_utils.py:16-19 l1_loss, its autograd gradient (the upstream-gradient
                  convention of train.py:155)
     ssim.npz     utils/loss_utils.py ssim/_ssim (conv2d SSIM), mean and autograd gradient: pins
                  oracle/ssim.py, the oracle of the fused-SSIM kernels
     cov3d.npz    scene/gaussian_model.py:32-42 build_covariance_from_scaling_rotation with
                  utils/general_utils.py:65-110 (build_rotation, build_scaling_rotation,
                  strip_symmetric) -- GaussianModel.get_covariance, the cov3D_precomp input of
                  compute_cov3D_python (gaussian_renderer/__init__.py:86-87); compiled from the
                  reference's source with "cuda" read as "cpu".  Pins the oracle's computeCov3D
                  and the HIP cov3D_precomp path
     densify_reference.npz   scene/gaussian_model.py densify_and_prune / add_densification_stats (compiled the
                  same way) on the seeded inputs of tests/test_densify.py: pins oracle/densify.py
     ply_reference_*.ply, ply_reference.npz   scene/dataset_readers.py storePly / fetchPly and
                  GaussianModel.save_ply / construct_list_of_attributes, run through this repository's
                  drop-in plyfile: the files they wrote and what they read back (tests/test_ply.py)
   These pin the camera conventions, the SH polynomial and the loss-gradient convention of the
   oracle and the HIP path.  The reference's rasterizer itself cannot run here (CUDA source,
   no nvcc, and BACKWARD::render is missing from the source).

2. RASTERIZER vectors -- raster_<case>.npz: inputs and the float64 oracle's outputs
   (oracle/gsr_oracle.c, the C restatement, which tests/test_oracle_autograd.py pins against
   torch autograd of an independent restatement and tests/test_golden.py against the vectors
   above).  The GPU parity tests compare the HIP path with these on the box, where neither the
   reference nor (by design) any generator runs.

Nothing from the reference is copied into the fixtures except these input/output arrays.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

# (W, H, focal, yaw_deg) cameras; the geometry (camera yawed about +y around (0,0,7)) is
# gaussian_splatting_amd/synthetic.py's, the matrix conventions are the reference's.
CAMERAS = [(64, 48, 60.0, 0.0), (37, 23, 30.0, 15.0), (1920, 1080, 1600.0, 5.0), (256, 256, 213.0, -35.0)]

RASTER_CASES = ["sh3_scalerot", "ragged_37x23", "sh1_of_16", "colors_precomp", "cov3d_precomp", "antialiasing",
                "background", "scale_modifier", "yawed_view", "pose_general"]
RASTER_POSE_CASES = ["pose_general"]  # those of tests/common.py POSE_CASES: --only raster_pose writes just these


def camera_pose(yaw_deg: float, pivot_z: float = 7.0):
    th = math.radians(yaw_deg)
    c, s = math.cos(th), math.sin(th)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    center = np.array([0.0, 0.0, pivot_z]) + R @ np.array([0.0, 0.0, -pivot_z])
    return R, -R.T @ center


def make_camera_vectors(gu):
    out = {}
    for i, (W, H, f, yaw) in enumerate(CAMERAS):
        R, T = camera_pose(yaw)
        fovx, fovy = gu.focal2fov(f, W), gu.focal2fov(f, H)
        wv = torch.tensor(gu.getWorld2View2(R, T)).transpose(0, 1)
        pm = gu.getProjectionMatrix(znear=0.01, zfar=100.0, fovX=fovx, fovY=fovy).transpose(0, 1)
        full = wv.unsqueeze(0).bmm(pm.unsqueeze(0)).squeeze(0)
        campos = wv.inverse()[3, :3]
        out[f"cam{i}_inputs"] = np.array([W, H, f, yaw, fovx, fovy], np.float64)
        out[f"cam{i}_R"], out[f"cam{i}_T"] = R, T
        out[f"cam{i}_viewmatrix"] = wv.numpy()
        out[f"cam{i}_projmatrix"] = full.numpy()
        out[f"cam{i}_campos"] = campos.numpy()
    np.savez_compressed(os.path.join(HERE, "camera.npz"), **out)


# the distinct cameras of tests/common.py POSE_CASES (the other cases reuse pose_general's)
POSE_CAMERAS = ["pose_general", "pose_roll90", "pose_pitch", "pose_aniso_focal", "pose_back", "pose_principal"]


def make_camera_pose_vectors(reference):
    """camera_pose.npz: per pose camera (one row each, "names") the inputs (W, H, fx, fy, yaw, pitch, roll,
    centre, principal, fovx, fovy, R, T) and the reference's raw getWorld2View2(R, T) and
    getProjectionMatrix(0.01, 100, fovx, fovy).  The reference's projection has no principal point; the test adds
    the case's offset to P[0,2], P[1,2]."""
    from tests import common as C

    sys.path.insert(0, reference)
    try:
        from utils import graphics_utils as gu
    finally:
        sys.path.remove(reference)
    rows = {k: [] for k in ("inputs", "R", "T", "world2view", "projection")}
    for name in POSE_CAMERAS:
        c = C.pose_case(name)
        fy = c.focal_y if c.focal_y is not None else c.focal
        R, center = C.case_pose(c)
        T = -R.T @ center
        fovx, fovy = gu.focal2fov(c.focal, c.W), gu.focal2fov(fy, c.H)
        rows["inputs"].append(np.array([c.W, c.H, c.focal, fy, c.yaw, c.pitch, c.roll, *center, *c.principal,
                                        fovx, fovy], np.float64))
        rows["R"].append(R)
        rows["T"].append(T)
        rows["world2view"].append(gu.getWorld2View2(R, T))
        rows["projection"].append(gu.getProjectionMatrix(znear=0.01, zfar=100.0, fovX=fovx, fovY=fovy).numpy())
    out = {k: np.stack(v) for k, v in rows.items()}
    out["names"] = np.array(POSE_CAMERAS)
    np.savez_compressed(os.path.join(HERE, "camera_pose.npz"), **out)


def make_raster_pose_vectors(reference=None):
    """raster_pose_general.npz alone (the other raster vectors stay as they are)."""
    from tests import common as C

    for name in RASTER_POSE_CASES:
        assert name in RASTER_CASES
        save_raster(name, C.build(C.pose_case(name)), C, with_backward=True)


def make_sh_vectors(sh_utils):
    """A small synthetic scene seen by a yawed camera; colours from the reference's eval_sh for every
    degree.  Rendering with shs= must equal rendering with colors_precomp= these colours."""
    from gaussian_splatting_amd import synthetic as syn

    cam = syn.make_camera(64, 48, 60.0, 10.0)
    sc = syn.make_scene(96, syn.make_camera(64, 48, 60.0, 0.0), sh_degree=3, seed=11, scale_range=(0.02, 0.25),
                        z_range=(2.0, 8.0))
    feats = sc.shs * 6.0  # larger higher-order terms than the benchmark scene, so every degree matters
    P = sc.P
    out = dict(means3D=sc.means3D.numpy(), scales=sc.scales.numpy(), rotations=sc.rotations.numpy(),
               opacities=sc.opacities.numpy(), features=feats.numpy(), viewmatrix=cam.viewmatrix.numpy(),
               projmatrix=cam.projmatrix.numpy(), campos=cam.campos.numpy(),
               camera=np.array([cam.width, cam.height, cam.tanfovx, cam.tanfovy], np.float64))
    for deg in range(4):
        # gaussian_renderer/__init__.py:86-96 (convert_SHs_python branch)
        shs_view = feats.transpose(1, 2).view(-1, 3, 16)
        dir_pp = sc.means3D - cam.campos.repeat(P, 1)
        dir_pp_normalized = dir_pp / dir_pp.norm(dim=1, keepdim=True)
        sh2rgb = sh_utils.eval_sh(deg, shs_view, dir_pp_normalized)
        out[f"colors_deg{deg}"] = torch.clamp_min(sh2rgb + 0.5, 0.0).numpy()
    out["rgb2sh_in"] = np.linspace(0, 1, 7, dtype=np.float32)
    out["rgb2sh_out"] = sh_utils.RGB2SH(torch.tensor(out["rgb2sh_in"])).numpy()
    np.savez_compressed(os.path.join(HERE, "sh_eval.npz"), **out)


def make_l1_vectors(loss_utils):
    g = torch.Generator().manual_seed(5)
    img = torch.rand(3, 12, 10, generator=g, requires_grad=True)
    gt = torch.rand(3, 12, 10, generator=g)
    loss = loss_utils.l1_loss(img, gt)
    loss.backward()
    np.savez_compressed(os.path.join(HERE, "l1_grad.npz"), image=img.detach().numpy(), gt=gt.numpy(),
                        loss=np.array(loss.item()), grad=img.grad.numpy())


def make_ssim_vectors(loss_utils):
    """utils/loss_utils.py ssim (conv2d, 11x11 window, sigma 1.5) -- the function the reference's
    fused-ssim test compares its kernels against (submodules/fused-ssim/tests/test.py:23-52,78-87) --
    evaluated in float64 on CPU: the mean SSIM and its autograd gradient w.r.t. img1."""
    out = {}
    g = torch.Generator().manual_seed(9)
    for i, shape in enumerate([(1, 3, 37, 53), (2, 2, 40, 45), (1, 1, 16, 9)]):
        img1 = torch.rand(shape, generator=g, dtype=torch.float64)
        img2 = (0.7 * img1 + 0.3 * torch.rand(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
        x = img1.clone().requires_grad_(True)
        val = loss_utils.ssim(x, img2)
        val.backward()
        out[f"img1_{i}"], out[f"img2_{i}"] = img1.numpy(), img2.numpy()
        out[f"value_{i}"], out[f"grad_{i}"] = np.array(val.item()), x.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "ssim.npz"), **out)


class _CudaToCpu(__import__("ast").NodeTransformer):
    """Reads the device literal "cuda" as "cpu" -- the only change made to the reference's code."""

    def visit_Constant(self, node):
        if node.value == "cuda":
            node.value = "cpu"
        return node


def _reference_covariance(reference):
    """GaussianModel.get_covariance's function (scene/gaussian_model.py:32-42, built by setup_functions)
    with build_scaling_rotation / build_rotation / strip_symmetric (utils/general_utils.py:65-110),
    compiled from the reference's source with the device literal "cuda" read as "cpu" so it runs here.
    (scene/ does not import in this container: cameras.py needs cv2.)"""
    import ast

    ns = {"torch": torch, "np": np}
    gu = ast.parse(open(os.path.join(reference, "utils/general_utils.py")).read())
    funcs = [n for n in gu.body if isinstance(n, ast.FunctionDef)]
    exec(compile(_CudaToCpu().visit(ast.Module(body=funcs, type_ignores=[])), "general_utils", "exec"), ns)
    gm = ast.parse(open(os.path.join(reference, "scene/gaussian_model.py")).read())
    cls = next(n for n in gm.body if isinstance(n, ast.ClassDef) and n.name == "GaussianModel")
    setup = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "setup_functions")
    inner = next(n for n in setup.body if isinstance(n, ast.FunctionDef)
                 and n.name == "build_covariance_from_scaling_rotation")
    exec(compile(_CudaToCpu().visit(ast.Module(body=[inner], type_ignores=[])), "gaussian_model", "exec"), ns)
    return ns["build_covariance_from_scaling_rotation"], ns["build_rotation"]


def make_cov3d_vectors(reference):
    """cov3d.npz: the reference's own covariance (GaussianModel.get_covariance =
    build_covariance_from_scaling_rotation(get_scaling, modifier, _rotation), the cov3D_precomp input of
    compute_cov3D_python, gaussian_renderer/__init__.py:86-87) on the scene of the cov3d_precomp case, with
    un-normalised raw quaternions (get_covariance passes _rotation; build_rotation normalises), plus the
    normalised quaternion get_rotation would give (the rasterizer's scales/rotations input)."""
    from tests import common as C

    cov_fn, build_rotation = _reference_covariance(reference)
    case = next(c for c in C.SMALL_CASES if c.name == "cov3d_precomp")
    inp = C.build(C.Case(case.name, P=case.P, W=case.W, H=case.H, seed=case.seed))  # scales/rotations form
    g = torch.Generator().manual_seed(21)
    raw_rot = inp["rotations"] * (0.5 + 2.0 * torch.rand(case.P, 1, generator=g))  # as stored in _rotation
    out = {}
    for tag, mod in (("", 1.0), ("_mod", 0.7)):
        cov = cov_fn(inp["scales"], mod, raw_rot)
        out["cov3D" + tag] = cov.numpy().astype(np.float32)
        out["modifier" + tag] = np.array(mod)
    out["scales"] = inp["scales"].numpy()
    out["raw_rotations"] = raw_rot.numpy()
    out["rotations"] = torch.nn.functional.normalize(raw_rot).numpy()  # get_rotation (rotation_activation)
    out["R"] = build_rotation(raw_rot).numpy()
    np.savez_compressed(os.path.join(HERE, "cov3d.npz"), **out)


def _reference_gaussian_model(reference):
    """GaussianModel (scene/gaussian_model.py) and build_rotation / strip_symmetric / ...
    (utils/general_utils.py) compiled from the reference's source with the literal device "cuda" read as
    "cpu" -- the only change -- so its densification runs on a CPU-only host."""
    import ast

    from torch import nn

    from gaussian_splatting_amd.ply import BasicPointCloud

    ns = {"torch": torch, "nn": nn, "np": np, "os": os, "BasicPointCloud": BasicPointCloud}
    gu = ast.parse(open(os.path.join(reference, "utils/general_utils.py")).read())
    funcs = [n for n in gu.body if isinstance(n, ast.FunctionDef)]
    exec(compile(_CudaToCpu().visit(ast.Module(body=funcs, type_ignores=[])), "general_utils", "exec"), ns)
    gm = ast.parse(open(os.path.join(reference, "scene/gaussian_model.py")).read())
    cls = [n for n in gm.body if isinstance(n, ast.ClassDef) and n.name == "GaussianModel"]
    exec(compile(_CudaToCpu().visit(ast.Module(body=cls, type_ignores=[])), "gaussian_model", "exec"), ns)
    return ns["GaussianModel"]


def _source_rows(out, src):
    """For every row of ``out`` the index of the bitwise-equal row of ``src`` (-1 for an all-zero row that
    is no row of ``src``); raises when a row is neither."""
    key = {r.tobytes(): i for i, r in enumerate(src.reshape(len(src), -1))}
    assert len(key) == len(src), "source rows are not unique"
    idx = np.empty(len(out), np.int32)
    for j, r in enumerate(out.reshape(len(out), -1)):
        i = key.get(r.tobytes())
        if i is None:
            assert not r.any(), j
            i = -1
        idx[j] = i
    return idx


def make_densify_vectors(reference):
    """densify_reference.npz: the reference's own add_densification_stats (with train.py:212-213) and
    densify_and_prune (scene/gaussian_model.py) on the inputs of tests/test_densify.py
    test_oracle_matches_reference_code, per case ``s<max_screen>_m<moments>``:
      accum / denom / max_radii   the statistics after add_densification_stats
      samples                     the normal samples densify_and_split draws (CPU generator, seed 123)
      xyz / scaling               the two parameters densification computes, as the reference returns them
      rows                        for every output Gaussian the input row its f_dc / f_rest / opacity / rotation
                                  equal bit for bit (checked here for all four)
      moment_rows                 the same for the optimizer's exp_avg / exp_avg_sq of all six groups
                                  (-1: zeros, a new Gaussian), checked here for all twelve
    so the test rebuilds the reference's full output from its own seeded inputs."""
    from torch import nn

    from oracle import densify as od
    from tests import test_densify as td

    GM = _reference_gaussian_model(reference)
    out = {}
    for max_screen, moments in td.REFERENCE_CASES:
        tag = td.reference_tag(max_screen, moments)
        P = td.REFERENCE_P
        params, mom, accum, denom = td._case(P, 11, moments)
        m = GM(3)
        for k, a in td.ATTR.items():
            setattr(m, a, nn.Parameter(torch.tensor(params[k]).requires_grad_(True)))
        m.optimizer = torch.optim.Adam([{"params": [getattr(m, td.ATTR[k])], "lr": 1e-3, "name": k} for k in td.ATTR],
                                       lr=0.0, eps=1e-15)
        if mom is not None:
            for k, a in td.ATTR.items():
                m.optimizer.state[getattr(m, a)] = {"step": torch.tensor(3.0), "exp_avg": torch.tensor(mom[k][0]),
                                                    "exp_avg_sq": torch.tensor(mom[k][1])}
        m.percent_dense = 0.01
        # the statistics through the reference's add_densification_stats and train.py:212-213
        vg, radii = td.reference_stats_inputs(P)
        m.xyz_gradient_accum = torch.tensor(accum).reshape(P, 1).clone()
        m.denom = torch.tensor(denom).reshape(P, 1).clone()
        m.max_radii2D = torch.zeros(P)
        vpt = torch.zeros(P, 3, requires_grad=True)
        vpt.grad = torch.tensor(vg)
        vis = torch.tensor(radii) > 0
        m.max_radii2D[vis] = torch.max(m.max_radii2D[vis], torch.tensor(radii)[vis])
        m.add_densification_stats(vpt, vis)
        out[tag + "_accum"] = m.xyz_gradient_accum.numpy().copy()
        out[tag + "_denom"] = m.denom.numpy().copy()
        out[tag + "_max_radii"] = m.max_radii2D.numpy().copy()
        # the samples the reference will draw: same seed, same stds, same call
        st = od.State(params, mom or {}, out[tag + "_accum"], out[tag + "_denom"])
        with np.errstate(divide="ignore", invalid="ignore"):
            grads = st.accum / st.denom
        grads[np.isnan(grads)] = 0
        od.densify_and_clone(st, grads, 2e-4, 2.0, 0.01)
        sel = od.split_mask(st, grads, 2e-4, 2.0, 0.01)
        stds = torch.exp(torch.tensor(st.params["scaling"][sel])).repeat(2, 1)
        torch.manual_seed(123)
        out[tag + "_samples"] = torch.normal(mean=torch.zeros((stds.size(0), 3)), std=stds).numpy()
        torch.manual_seed(123)
        m.densify_and_prune(2e-4, 0.005, 2.0, max_screen, torch.ones(P, dtype=torch.int32))
        got = {k: getattr(m, a).detach().numpy() for k, a in td.ATTR.items()}
        out[tag + "_xyz"], out[tag + "_scaling"] = got["xyz"], got["scaling"]
        rows = _source_rows(got["f_rest"], params["f_rest"])
        assert (rows >= 0).all()
        for k in ("f_dc", "f_rest", "opacity", "rotation"):
            np.testing.assert_array_equal(got[k], params[k][rows], err_msg=k)
        out[tag + "_rows"] = rows
        if mom is not None:
            state = {k: m.optimizer.state[getattr(m, a)] for k, a in td.ATTR.items()}
            mrows = _source_rows(state["f_rest"]["exp_avg"].numpy(), mom["f_rest"][0])
            for k in td.ATTR:
                for j, name in enumerate(("exp_avg", "exp_avg_sq")):
                    np.testing.assert_array_equal(state[k][name].numpy(), td.moment_rows(mom[k][j], mrows),
                                                  err_msg=f"{k} {name}")
            out[tag + "_moment_rows"] = mrows
        out[tag + "_tmp_radii_is_none"] = np.array(m.tmp_radii is None)
    np.savez_compressed(os.path.join(HERE, "densify_reference.npz"), **out)


def make_ply_vectors(reference):
    """The reference's own PLY code, compiled from its source files with this repository's drop-in
    ``plyfile`` in their globals (the ``scene`` package itself needs cv2): ``storePly`` / ``fetchPly``
    (scene/dataset_readers.py:120-143) and ``GaussianModel.construct_list_of_attributes`` / ``save_ply``
    (scene/gaussian_model.py:288-321), on the inputs of tests/test_ply.py.  Stored: the two files they
    wrote (ply_reference_store.ply, ply_reference_save.ply) and, in ply_reference.npz, what fetchPly read
    back and the attribute list."""
    import ast
    import shutil
    import tempfile

    import plyfile

    from gaussian_splatting_amd import ply
    from tests import test_ply as tp

    assert os.path.dirname(os.path.dirname(os.path.abspath(plyfile.__file__))) == ROOT
    ns = {"np": np, "os": os, "PlyData": plyfile.PlyData, "PlyElement": plyfile.PlyElement,
          "BasicPointCloud": ply.BasicPointCloud, "mkdir_p": lambda d: os.makedirs(d, exist_ok=True)}
    wanted = {"storePly", "fetchPly", "construct_list_of_attributes", "save_ply"}
    for f in ("scene/dataset_readers.py", "scene/gaussian_model.py"):
        tree = ast.parse(open(os.path.join(reference, f)).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.FunctionDef) and node.name in wanted and node.name not in ns:
                exec(compile(ast.Module(body=[node], type_ignores=[]), os.path.join(reference, f), "exec"), ns)
    assert wanted <= set(ns), wanted - set(ns)
    tmp = tempfile.mkdtemp()
    try:
        xyz, rgb = tp.reference_store_inputs()
        a = os.path.join(tmp, "ref.ply")
        ns["storePly"](a, xyz, rgb)
        pc = ns["fetchPly"](a)
        shutil.copyfile(a, os.path.join(HERE, "ply_reference_store.ply"))
        src = tp.reference_save_model()
        src.construct_list_of_attributes = lambda: ns["construct_list_of_attributes"](src)
        b = os.path.join(tmp, "ref", "point_cloud.ply")
        ns["save_ply"](src, b)
        shutil.copyfile(b, os.path.join(HERE, "ply_reference_save.ply"))
        np.savez_compressed(os.path.join(HERE, "ply_reference.npz"), fetch_points=pc.points, fetch_colors=pc.colors,
                            fetch_normals=pc.normals, attributes=np.array(ns["construct_list_of_attributes"](src)))
    finally:
        shutil.rmtree(tmp)


def make_raster_vectors():
    from tests import common as C
    from gaussian_splatting_amd import synthetic as syn

    cases = {c.name: c for c in C.SMALL_CASES + C.POSE_CASES}
    for name in RASTER_CASES:
        inp = C.build(cases[name])
        save_raster(name, inp, C, with_backward=True)
    # the reference's CPU-runnable config (BASELINE.json configs[0]): 10k Gaussians, 256x256, SH0, forward only
    scene, cam = syn.config_scene("10k_256_sh0", seed=0)
    inp = dict(bg=torch.zeros(3), means3D=scene.means3D, opacities=scene.opacities, shs=scene.shs, sh_degree=0,
               scales=scene.scales, rotations=scene.rotations, colors_precomp=None, cov3D_precomp=None,
               viewmatrix=cam.viewmatrix, projmatrix=cam.projmatrix, campos=cam.campos, tanfovx=cam.tanfovx,
               tanfovy=cam.tanfovy, H=cam.height, W=cam.width, scale_modifier=1.0, antialiasing=False)
    save_raster("10k_256_sh0", inp, C, with_backward=False)


def save_raster(name, inp, C, with_backward):
    ref = C.run_oracle(inp, precision="f64", nthreads=os.cpu_count())
    out = {}
    for k, v in inp.items():
        if v is None:
            continue
        out["in_" + k] = v.numpy() if torch.is_tensor(v) else np.array(v)
    out["out_color"] = ref.color.astype(np.float32)
    out["out_invdepth"] = ref.invdepth.astype(np.float32)
    out["out_radii"] = ref.radii.astype(np.int32)
    out["out_num_rendered"] = np.array(ref.num_rendered)
    if with_backward:
        gc, gd = C.unit_grads(inp["H"], inp["W"])
        out["grad_color"], out["grad_invdepth"] = gc.numpy(), gd.numpy()
        g = ref.handle.backward(gc.double().numpy(), gd.double().numpy(), nthreads=os.cpu_count())
        for k in C.GRAD_NAMES:
            out["out_" + k] = g[k].astype(np.float32)
    write_raster(name, out)


IMAGE_KEYS = ("out_color", "out_invdepth")
MAX_FIXTURE_BYTES = 1 << 20


def write_raster(name, out):
    """raster_<name>.npz; when that would pass 1 MiB, the output images go to raster_<name>.images.npz
    (tests/common.py load_raster reads both)."""
    path = os.path.join(HERE, f"raster_{name}.npz")
    np.savez_compressed(path, **out)
    if os.path.getsize(path) > MAX_FIXTURE_BYTES:
        np.savez_compressed(path, **{k: v for k, v in out.items() if k not in IMAGE_KEYS})
        np.savez_compressed(os.path.join(HERE, f"raster_{name}.images.npz"), **{k: out[k] for k in IMAGE_KEYS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--only", choices=("densify", "ply", "camera_pose", "raster_pose"),
                    help="write only these vectors, leave the others as they are")
    args = ap.parse_args()
    if args.only:
        {"densify": make_densify_vectors, "ply": make_ply_vectors, "camera_pose": make_camera_pose_vectors,
         "raster_pose": make_raster_pose_vectors}[args.only](args.reference)
        return
    sys.path.insert(0, args.reference)
    from utils import graphics_utils as gu, loss_utils, sh_utils  # the reference's own Python

    make_camera_vectors(gu)
    make_l1_vectors(loss_utils)
    make_ssim_vectors(loss_utils)
    sys.path.remove(args.reference)
    make_cov3d_vectors(args.reference)
    make_densify_vectors(args.reference)
    make_ply_vectors(args.reference)
    make_sh_vectors(sh_utils)
    make_camera_pose_vectors(args.reference)
    make_raster_vectors()
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            print(f"{f:32s} {os.path.getsize(os.path.join(HERE, f)):>9d} B")


if __name__ == "__main__":
    main()
