#!/usr/bin/env python3
"""Measure the depth-distortion map (gsr_render_distortion / gsr_render_distortion_backward) on one MI355X.

    python tools/bench_distortion.py [--config 1m_1080p_sh3] [--reps 30] [--rounds 5]

One JSON line.  Timed with device events around ``reps`` back-to-back calls, the calls alternating for ``rounds``
rounds (medians and every round are reported), all on the buffers of one SH forward, t = view depth:
  fwd / bwd_geom / bwd_frozen            the distortion forward, its backward with the geometry part (the kernel, the
                                         view block and gauss_backward_views) and without it (only dL_dt)
  feat_fwd / feat_bwd_geom / feat_bwd_frozen   the same three calls of a feature pass with C = 1 over the same buffers
Before timing, a second forward call is checked against the first (bit for bit), a constant t against zero and a
shifted t against the unshifted map (1e-5), and the frozen dL_dt against the full variant's (1e-6).
"""
import argparse
import json
import os
import statistics
import sys

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
    assert torch.cuda.is_available(), "bench_distortion needs a HIP device"
    dev = "cuda"
    cfg = syn.CONFIGS[a.config]
    W, H = cfg["width"], cfg["height"]
    scene, cam = syn.config_scene(a.config, seed=0, yaw_deg=5.0)
    sc = scene.to(dev)
    P = scene.P
    e = torch.Tensor([]).to(dev)
    bg = torch.zeros(3, device=dev)
    view, proj, campos = cam.viewmatrix.to(dev), cam.projmatrix.to(dev), cam.campos.to(dev)
    gen = torch.Generator().manual_seed(29)
    nr, _color, radii, geom, binning, img, _invd = _C.rasterize_gaussians(
        bg, sc.means3D, e, sc.opacities, sc.scales, sc.rotations, 1.0, e, view, proj, cam.tanfovx, cam.tanfovy, H, W,
        sc.shs, scene.sh_degree, campos, False, False, False)
    bufs = (geom, binning, img, nr, P, H, W)
    geometry = dict(viewmatrix=view, projmatrix=proj, campos=campos, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                    antialiasing=False, radii=radii)
    zero_dc = torch.zeros(P, 1, 3, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    out = {"dL_dmeans3D": torch.empty((P, 3), **f32), "dL_ddc": torch.empty((P, 1, 3), **f32),
           "dL_dsh": torch.empty((P, 0, 3), **f32), "dL_dopacity": torch.empty((P, 1), **f32),
           "dL_dscales": torch.empty((P, 3), **f32), "dL_drotations": torch.empty((P, 4), **f32)}

    def views(block):
        _C.gauss_backward_views(sc.means3D, zero_dc, None, 0, sc.opacities, sc.scales, sc.rotations, 1.0,
                                block.view(1, -1), out)

    t = (torch.cat([sc.means3D, torch.ones(P, 1, device=dev)], 1) @ view[:, 2]).contiguous()
    U = torch.randn(1, H, W, generator=gen).to(dev)
    F = t.view(P, 1).contiguous()

    def bwd_geom(dmap, moments):
        dt, block = _C.render_distortion_backward(*bufs, t, dmap, moments, U, geometry=geometry)
        views(block)
        return dt

    def feat_bwd_geom(fmap):
        dF, block = _C.render_features_backward(*bufs, F, fmap, U, geometry=geometry)
        views(block)
        return dF

    # checks that hold at any size
    dmap, moments = _C.render_distortion(*bufs, t)
    assert torch.equal(_C.render_distortion(*bufs, t)[0], dmap), "the map is not reproducible"
    assert float(_C.render_distortion(*bufs, torch.full_like(t, 3.0))[0].abs().max()) <= 1e-5, "constant t"
    assert float((_C.render_distortion(*bufs, t + 2.5)[0] - dmap).abs().max()) <= 1e-5, "shifted t"
    full = bwd_geom(dmap, moments)
    frozen = _C.render_distortion_backward(*bufs, t, dmap, moments, U)[0]
    assert float((full - frozen).abs().max()) <= 1e-6 * float(full.abs().max()), "frozen dL_dt differs"
    fmap = _C.render_features(*bufs, F)

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / a.reps  # us per call

    res = {"metric": "distortion map device time", "config": a.config, "P": P, "num_rendered": int(nr), "unit": "us",
           "reps_per_round": a.reps, "bwd_atomic": _lib.option_get("bwd_atomic"), "max_D": float(dmap.max())}
    calls = {"fwd": lambda: _C.render_distortion(*bufs, t), "bwd_geom": lambda: bwd_geom(dmap, moments),
             "bwd_frozen": lambda: _C.render_distortion_backward(*bufs, t, dmap, moments, U),
             "feat_fwd": lambda: _C.render_features(*bufs, F), "feat_bwd_geom": lambda: feat_bwd_geom(fmap),
             "feat_bwd_frozen": lambda: _C.render_features_backward(*bufs, F, fmap, U)}
    for fn in calls.values():  # warm-up of every shape
        fn()
        fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            rounds[k].append(timed(fn))
    for k, v in rounds.items():
        res[k + "_us"] = round(statistics.median(v), 1)
        res[k + "_us_rounds"] = [round(x, 1) for x in v]
    res["value"] = res["fwd_us"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
