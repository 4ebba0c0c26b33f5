#!/usr/bin/env python3
"""Measure N-channel feature rendering (gsr_render_features / gsr_render_features_backward) on one MI355X.

    python tools/bench_features.py [--config 1m_1080p_sh3] [--channels 3,16,64] [--reps 30] [--rounds 5]

One JSON line.  For each channel count C, timed with device events around ``reps`` back-to-back calls, the calls
alternating for ``rounds`` rounds (medians and every round are reported):
  fwd           the feature forward on the buffers of one SH forward
  bwd_geom      the feature backward with the geometry part: the kernel, the view block and gauss_backward_views
  bwd_frozen    the feature backward without it (only dL_dfeatures)
  baseline      what the feature path replaces: ceil(C/3) x (a forward with colors_precomp = three channels + its
                backward) through the existing rasterizer
Before timing, the C = 3 map of a scene's precomputed colours is checked against that scene's own colour (1e-5), a
second forward call against the first (bit for bit), and the frozen dL_dfeatures against the full variant's (1e-6).
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
    ap.add_argument("--channels", default="3,16,64")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_features needs a HIP device"
    dev = "cuda"
    cfg = syn.CONFIGS[a.config]
    W, H = cfg["width"], cfg["height"]
    scene, cam = syn.config_scene(a.config, seed=0, yaw_deg=5.0)
    sc = scene.to(dev)
    P = scene.P
    e = torch.Tensor([]).to(dev)
    bg = torch.zeros(3, device=dev)
    view, proj, campos = cam.viewmatrix.to(dev), cam.projmatrix.to(dev), cam.campos.to(dev)
    gen = torch.Generator().manual_seed(21)

    def forward(colors=None):
        shs = sc.shs if colors is None else e
        return _C.rasterize_gaussians(bg, sc.means3D, e if colors is None else colors, sc.opacities, sc.scales,
                                      sc.rotations, 1.0, e, view, proj, cam.tanfovx, cam.tanfovy, H, W, shs,
                                      scene.sh_degree, campos, False, False, False)

    def colour_backward(fwd, colors, g_c, g_d):
        nr, _c, radii, geom, binning, img = fwd[:6]
        return _C.rasterize_gaussians_backward(bg, sc.means3D, radii, colors, sc.opacities, sc.scales, sc.rotations, 1.0,
                                               e, view, proj, cam.tanfovx, cam.tanfovy, g_c, g_d, e, scene.sh_degree,
                                               campos, geom, nr, binning, img, False, False)

    nr, _color, radii, geom, binning, img, _invd = forward()
    bufs = (geom, binning, img, nr, P, H, W)
    geometry = dict(viewmatrix=view, projmatrix=proj, campos=campos, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                    antialiasing=False, radii=radii)
    zero_dc = torch.zeros(P, 1, 3, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    out = {"dL_dmeans3D": torch.empty((P, 3), **f32), "dL_ddc": torch.empty((P, 1, 3), **f32),
           "dL_dsh": torch.empty((P, 0, 3), **f32), "dL_dopacity": torch.empty((P, 1), **f32),
           "dL_dscales": torch.empty((P, 3), **f32), "dL_drotations": torch.empty((P, 4), **f32)}

    def bwd_geom(F, fmap, U):
        dF, block = _C.render_features_backward(*bufs, F, fmap, U, geometry=geometry)
        _C.gauss_backward_views(sc.means3D, zero_dc, None, 0, sc.opacities, sc.scales, sc.rotations, 1.0,
                                block.view(1, -1), out)
        return dF

    # checks that hold at any size
    col = torch.rand(P, 3, generator=gen).to(dev)
    f_col = forward(col)
    m = _C.render_features(*f_col[3:6], f_col[0], P, H, W, col)
    assert float((m - f_col[1]).abs().max()) <= 1e-5, "the map of the colours is not the colour"
    assert torch.equal(_C.render_features(*f_col[3:6], f_col[0], P, H, W, col), m), "the map is not reproducible"

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / a.reps  # us per call

    res = {"metric": "feature rendering device time", "config": a.config, "P": P, "num_rendered": int(nr),
           "unit": "us", "reps_per_round": a.reps, "chunk": _C.feature_chunk(),
           "bwd_atomic": _lib.option_get("bwd_atomic")}
    g_d = torch.zeros(1, H, W, device=dev)
    for Cn in [int(c) for c in a.channels.split(",")]:
        F = torch.randn(P, Cn, generator=gen).to(dev)
        U = torch.randn(Cn, H, W, generator=gen).to(dev)
        fmap = _C.render_features(*bufs, F)
        full = bwd_geom(F, fmap, U)
        frozen = _C.render_features_backward(*bufs, F, fmap, U)[0]
        assert float((full - frozen).abs().max()) <= 1e-6 * float(full.abs().max()), "frozen dL_dF differs"
        n3 = (Cn + 2) // 3
        cols = [torch.zeros(P, 3, device=dev) for _ in range(n3)]
        ups = [torch.zeros(3, H, W, device=dev) for _ in range(n3)]
        for k in range(n3):
            n = min(3, Cn - 3 * k)
            cols[k][:, :n] = F[:, 3 * k:3 * k + n]
            ups[k][:n] = U[3 * k:3 * k + n]

        def baseline():
            for k in range(n3):
                colour_backward(forward(cols[k]), cols[k], ups[k], g_d)

        calls = {"fwd": lambda: _C.render_features(*bufs, F), "bwd_geom": lambda: bwd_geom(F, fmap, U),
                 "bwd_frozen": lambda: _C.render_features_backward(*bufs, F, fmap, U), "baseline": baseline}
        for fn in calls.values():  # warm-up of every shape
            fn()
            fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, fn in calls.items():
                rounds[k].append(timed(fn))
        r = {}
        for k, v in rounds.items():
            r[k + "_us"] = round(statistics.median(v), 1)
            r[k + "_us_rounds"] = [round(x, 1) for x in v]
        r["feature_path_us"] = round(r["fwd_us"] + r["bwd_geom_us"], 1)
        res[f"C{Cn}"] = r
    res["value"] = res[f"C{a.channels.split(',')[0]}"]["fwd_us"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
