#!/usr/bin/env python3
"""Measure the per-pixel selections (gsr_render_select / gsr_render_median_backward) on one MI355X.

    python tools/bench_select.py [--config 1m_1080p_sh3] [--reps 30] [--rounds 5]

One JSON line.  Timed with device events around ``reps`` back-to-back calls, the calls alternating for ``rounds``
rounds (medians, every round and min-max are reported), all on the buffers of one SH forward, t = view depth:
  median / top1 / top4 / top8 / median_top4   the select pass with the median only, K = 1, 4, 8 without it, and both
  distortion_fwd                              the distortion forward over the same buffers, in the same rounds
  median_bwd                                  the scatter backward of the median map
Before timing, a second select call is checked against the first (bit for bit), the K = 8 planes against the K = 4
and K = 1 calls', the median map against ``t[median_ids]`` and the backward against ``torch.bincount`` in float64
(each row within float32 summation's own bound).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussian_splatting_amd import _C  # noqa: E402
from gaussian_splatting_amd import synthetic as syn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1m_1080p_sh3", choices=sorted(syn.CONFIGS))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_select needs a HIP device"
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
    nr, _color, _radii, geom, binning, img, _invd = _C.rasterize_gaussians(
        bg, sc.means3D, e, sc.opacities, sc.scales, sc.rotations, 1.0, e, view, proj, cam.tanfovx, cam.tanfovy, H, W,
        sc.shs, scene.sh_degree, campos, False, False, False)
    bufs = (geom, binning, img, nr, P, H, W)
    t = (torch.cat([sc.means3D, torch.ones(P, 1, device=dev)], 1) @ view[:, 2]).contiguous()
    U = torch.randn(1, H, W, generator=gen).to(dev)

    # checks that hold at any size
    med, mid, ids8, w8 = _C.render_select(*bufs, t=t, topk=8)
    again = _C.render_select(*bufs, t=t, topk=8)
    assert all(torch.equal(x, y) for x, y in zip((med, mid, ids8, w8), again)), "the selections are not reproducible"
    for k in (1, 4):
        _, _, ids, w = _C.render_select(*bufs, topk=k, device=geom.device)
        assert torch.equal(ids, ids8[:k]) and torch.equal(w, w8[:k]), f"K = {k} planes differ from K = 8's"
    hit = mid >= 0
    assert torch.equal(med[hit], t[mid[hit].long()]) and not med[~hit].any(), "the median map is not t[median_ids]"
    dt = _C.render_median_backward(mid, U, P)
    # (a float32 sum of n terms in any order is within n 2^-24 sum |terms| of the exact one)
    g = mid[hit].long()
    want = torch.bincount(g, weights=U[hit].double(), minlength=P)
    bound = torch.bincount(g, minlength=P) * 2.0 ** -24 * torch.bincount(g, weights=U[hit].double().abs(), minlength=P)
    bwd_err = (dt.double() - want).abs()
    assert bool((bwd_err <= bound).all()), "median backward"

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / a.reps  # us per call

    res = {"metric": "select pass device time", "config": a.config, "P": P, "num_rendered": int(nr), "unit": "us",
           "reps_per_round": a.reps, "pixels_with_a_median": int(hit.sum()),
           "pixels_with_8_contributors": int((ids8[7] >= 0).sum()),
           "median_bwd_max_err_of_max_ref": float(bwd_err.max() / want.abs().max()),
           "most_pixels_one_median": int(torch.bincount(g, minlength=P).max())}
    d = geom.device
    calls = {"median": lambda: _C.render_select(*bufs, t=t),
             "top1": lambda: _C.render_select(*bufs, topk=1, device=d),
             "top4": lambda: _C.render_select(*bufs, topk=4, device=d),
             "top8": lambda: _C.render_select(*bufs, topk=8, device=d),
             "median_top4": lambda: _C.render_select(*bufs, t=t, topk=4),
             "distortion_fwd": lambda: _C.render_distortion(*bufs, t),
             "median_bwd": lambda: _C.render_median_backward(mid, U, P)}
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
        res[k + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
    res["value"] = res["median_top4_us"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
