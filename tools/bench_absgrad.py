#!/usr/bin/env python3
"""Measure the absolute screen-space gradient (gsr_backward_args.dL_dmean2D_abs) on one MI355X.

    python tools/bench_absgrad.py [--config 1m_1080p_sh3] [--reps 30] [--rounds 5] [--bwd-atomic 0|1]

One JSON line: the backward with and without ``absgrad=True``, each timed with device events around ``reps``
back-to-back calls, the two alternating for ``rounds`` rounds; reported are the medians, every round and the
difference (the ABSGRAD instantiation of render_bwd and the per-Gaussian stage's extra output against the plain
backward).  Before timing, the result is checked for what holds at any size: every other gradient of the call
with the keyword is that of the call without it (bit for bit on the record path, closely on the atomic path),
the absolute sums dominate the signed ones, column 2 and the culled rows are zero.
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
    ap.add_argument("--bwd-atomic", type=int, default=None, choices=(0, 1), help="default: the library's")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_absgrad needs a HIP device"
    if a.bwd_atomic is not None:
        _lib.option_set("bwd_atomic", a.bwd_atomic)
    dev = "cuda"
    cfg = syn.CONFIGS[a.config]
    W, H = cfg["width"], cfg["height"]
    scene, cam = syn.config_scene(a.config, seed=0, yaw_deg=5.0)
    sc = scene.to(dev)
    e = torch.Tensor([]).to(dev)
    bg = torch.zeros(3, device=dev)
    view, proj, campos = cam.viewmatrix.to(dev), cam.projmatrix.to(dev), cam.campos.to(dev)
    gc, gd = (t.to(dev) for t in syn.upstream_grads(H, W))

    nr, _color, radii, geom, binning, img, _invd = _C.rasterize_gaussians(
        bg, sc.means3D, e, sc.opacities, sc.scales, sc.rotations, 1.0, e, view, proj, cam.tanfovx, cam.tanfovy, H, W,
        sc.shs, scene.sh_degree, campos, False, False, False)

    def backward(absgrad):
        kw = {"absgrad": True} if absgrad else {}
        return _C.rasterize_gaussians_backward(bg, sc.means3D, radii, e, sc.opacities, sc.scales, sc.rotations, 1.0, e,
                                               view, proj, cam.tanfovx, cam.tanfovy, gc, gd, sc.shs, scene.sh_degree,
                                               campos, geom, nr, binning, img, False, False, **kw)

    plain, with_abs = backward(False), backward(True)
    ab, g2 = with_abs[-1], with_abs[0]
    atomic = _lib.option_get("bwd_atomic")
    for x, y in zip(plain, with_abs):
        if atomic:
            assert float((x - y).abs().max()) <= 2e-4 * max(float(x.abs().max()), 1e-30), "another gradient moved"
        else:
            assert torch.equal(x, y), "another gradient moved"
    assert float((g2[:, :2].abs() - ab[:, :2]).max()) <= 2e-4 * float(ab.max()), "abs < |signed|"
    assert not ab[:, 2].any() and not ab[radii == 0].any()
    nz = ab[:, :2].sum(1) > 0
    ratio = float((ab[:, :2].sum(1)[nz] > 1.5 * g2[:, :2].abs().sum(1)[nz]).float().mean())

    def timed(flag):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            backward(flag)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / a.reps  # us per call

    for _ in range(5):  # warm-up of both shapes
        backward(False)
        backward(True)
    torch.cuda.synchronize()
    t_plain, t_abs = [], []
    for _ in range(a.rounds):
        t_plain.append(timed(False))
        t_abs.append(timed(True))
    out = {"metric": "absgrad backward device time", "config": a.config, "P": scene.P, "num_rendered": int(nr),
           "unit": "us", "reps_per_round": a.reps, "bwd_atomic": atomic,
           "rows_nonzero": int(nz.sum()), "share_abs_over_1p5_signed": round(ratio, 3),
           "max_abs_over_max_grad": round(float(ab.max() / g2[:, :2].abs().max()), 2),
           "backward_us": statistics.median(t_plain), "backward_absgrad_us": statistics.median(t_abs),
           "backward_us_rounds": [round(x, 1) for x in t_plain],
           "backward_absgrad_us_rounds": [round(x, 1) for x in t_abs]}
    out["value"] = out["backward_absgrad_us"] - out["backward_us"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
