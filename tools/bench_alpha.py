#!/usr/bin/env python3
"""Measure the accumulated-alpha output (gsr_render_alpha, gsr_backward_args.dL_dalphas) on one MI355X.

    python tools/bench_alpha.py [--config 1m_1080p_sh3] [--reps 30] [--rounds 5]

One JSON line: the forward with and without ``return_alpha`` and the backward with and without an alpha gradient,
each timed with device events around ``reps`` back-to-back calls, the two of a pair alternating for ``rounds``
rounds; reported are the medians, every round and the differences (the alpha kernel with its output's allocation;
the ALPHA instantiation of render_bwd against the plain one).  Before timing, the map is checked against the
forward's own per-pixel state (1 - final_T, bit for bit) at this size.
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
    assert torch.cuda.is_available(), "bench_alpha needs a HIP device"
    dev = "cuda"
    cfg = syn.CONFIGS[a.config]
    W, H = cfg["width"], cfg["height"]
    scene, cam = syn.config_scene(a.config, seed=0, yaw_deg=5.0)
    sc = scene.to(dev)
    e = torch.Tensor([]).to(dev)
    bg = torch.zeros(3, device=dev)
    view, proj, campos = cam.viewmatrix.to(dev), cam.projmatrix.to(dev), cam.campos.to(dev)
    gc, gd = (t.to(dev) for t in syn.upstream_grads(H, W))
    ga = torch.randn(1, H, W, generator=torch.Generator().manual_seed(11)).to(dev)

    def forward(alpha):
        return _C.rasterize_gaussians(bg, sc.means3D, e, sc.opacities, sc.scales, sc.rotations, 1.0, e, view, proj,
                                      cam.tanfovx, cam.tanfovy, H, W, sc.shs, scene.sh_degree, campos, False, False,
                                      False, return_alpha=alpha)

    fwd = forward(True)
    nr, _color, radii, geom, binning, img, _invd, alpha = fwd
    state = _C.debug_forward_state(fwd[:7], scene.P)
    assert torch.equal(alpha[0].cpu(), 1 - state["final_T"]), "alpha != 1 - final_T"

    def backward(with_alpha):
        return _C.rasterize_gaussians_backward(bg, sc.means3D, radii, e, sc.opacities, sc.scales, sc.rotations, 1.0, e,
                                               view, proj, cam.tanfovx, cam.tanfovy, gc, gd, sc.shs, scene.sh_degree,
                                               campos, geom, nr, binning, img, False, False,
                                               dL_dout_alpha=ga if with_alpha else None)

    def timed(fn, flag):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            fn(flag)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / a.reps  # us per call

    out = {"metric": "accumulated alpha device time", "config": a.config, "P": scene.P, "num_rendered": int(nr),
           "unit": "us", "reps_per_round": a.reps, "bwd_atomic": _lib.option_get("bwd_atomic"),
           "alpha_mean": float(alpha.mean())}
    # (the backward pair first: it needs the buffers of the forward above, which the timed forwards replace)
    for name, fn in (("backward", backward), ("forward", forward)):
        for _ in range(5):  # warm-up of both shapes
            fn(False)
            fn(True)
        torch.cuda.synchronize()
        plain, with_a = [], []
        for _ in range(a.rounds):
            plain.append(timed(fn, False))
            with_a.append(timed(fn, True))
        out[f"{name}_us"] = statistics.median(plain)
        out[f"{name}_with_alpha_us"] = statistics.median(with_a)
        out[f"{name}_alpha_cost_us"] = statistics.median(with_a) - statistics.median(plain)
        out[f"{name}_us_rounds"] = [round(x, 1) for x in plain]
        out[f"{name}_with_alpha_us_rounds"] = [round(x, 1) for x in with_a]
    out["value"] = out["forward_alpha_cost_us"] + out["backward_alpha_cost_us"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
