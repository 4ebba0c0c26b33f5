#!/usr/bin/env python3
"""Measure the camera backward (gsr_camera_backward, csrc/camera.hip) on one MI355X.

    python tools/bench_camera.py [--config 1m_1080p_sh3] [--reps 30] [--rounds 5]

Two figures, one JSON line:

(a) Time.  The ordinary backward of one forward, with and without the camera backward behind it
    (_C.rasterize_gaussians_backward(..., camera=True / False)), each timed with device events around ``reps``
    back-to-back calls, the two alternating for ``rounds`` rounds; reported are the medians, the spread of
    each and the difference, which is the camera backward (its two launches and the dL/dconic stores the
    ordinary backward then makes).
(b) Accuracy at a size the dense float64 reference cannot reach: the rigid-motion identity
    (tests/torch_ref_camera.py twist_sides) between the camera gradients and the backward's own dL/dmeans3D /
    dL/dcov3D, the Gaussian side summed in float64 on the host.  With SH colours it holds for the three
    translations; the rotational twists are reported and expected to differ.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussian_splatting_amd import _C, _lib  # noqa: E402
from gaussian_splatting_amd import synthetic as syn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1m_1080p_sh3", choices=sorted(syn.CONFIGS))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_camera needs a HIP device"
    dev = "cuda"
    cfg = syn.CONFIGS[a.config]
    W, H = cfg["width"], cfg["height"]
    scene, cam = syn.config_scene(a.config, seed=0, yaw_deg=5.0)
    sc = scene.to(dev)
    e = torch.Tensor([]).to(dev)
    bg = torch.zeros(3, device=dev)
    view, proj, campos = cam.viewmatrix.to(dev), cam.projmatrix.to(dev), cam.campos.to(dev)
    gc, gd = (t.to(dev) for t in syn.upstream_grads(H, W))
    fwd = _C.rasterize_gaussians(bg, sc.means3D, e, sc.opacities, sc.scales, sc.rotations, 1.0, e, view, proj,
                                 cam.tanfovx, cam.tanfovy, H, W, sc.shs, scene.sh_degree, campos, False, False, False)
    nr, _color, radii, geom, binning, img, _invd = fwd

    def backward(camera):
        return _C.rasterize_gaussians_backward(bg, sc.means3D, radii, e, sc.opacities, sc.scales, sc.rotations, 1.0, e,
                                               view, proj, cam.tanfovx, cam.tanfovy, gc, gd, sc.shs, scene.sh_degree,
                                               campos, geom, nr, binning, img, False, False, camera=camera)

    def timed(camera):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            backward(camera)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / a.reps  # us per call

    for _ in range(5):  # warm-up of both shapes
        backward(False)
        backward(True)
    torch.cuda.synchronize()
    plain, with_cam = [], []
    for _ in range(a.rounds):
        plain.append(timed(False))
        with_cam.append(timed(True))
    med_p, med_c = statistics.median(plain), statistics.median(with_cam)

    # (b) the identity on this frame
    from tests import torch_ref_camera as TRC
    from tests.test_pose_equivariance import _grad_full

    out = backward(True)
    names = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
             "dL_drotations"] + TRC.CAMERA_NAMES
    g = {k: t.detach().cpu().numpy() for k, t in zip(names, out) if k in ("dL_dmeans3D", "dL_dcov3D") or
         k in TRC.CAMERA_NAMES}
    inp = dict(viewmatrix=cam.viewmatrix, projmatrix=cam.projmatrix, campos=cam.campos, means3D=scene.means3D,
               scales=scene.scales, rotations=scene.rotations, scale_modifier=1.0, cov3D_precomp=None)
    G, S = _grad_full(g["dL_dcov3D"].astype(np.float64)), TRC.world_cov(inp)
    sides = np.array([TRC.twist_sides(tw, g, inp, G, S) for tw in TRC.TWISTS])
    resid = np.abs(sides[:, 0] - sides[:, 1]) / np.abs(sides).max()
    print(json.dumps({
        "metric": "camera backward device time", "config": a.config, "P": scene.P, "num_rendered": int(nr),
        "unit": "us", "value": med_c - med_p,
        "backward_us": med_p, "backward_with_camera_us": med_c,
        "backward_us_rounds": [round(x, 1) for x in plain],
        "backward_with_camera_us_rounds": [round(x, 1) for x in with_cam],
        "reps_per_round": a.reps, "bwd_atomic": _lib.option_get("bwd_atomic"),
        "identity_residual_translations": float(resid[3:].max()),
        "identity_residual_rotations_sh": float(resid[:3].max()),
        "identity_residuals": [float(x) for x in resid],
        "camera_side": [float(x) for x in sides[:, 0]], "gaussian_side": [float(x) for x in sides[:, 1]]}))


if __name__ == "__main__":
    main()
