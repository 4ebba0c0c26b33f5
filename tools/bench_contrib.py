#!/usr/bin/env python3
"""Measure the per-Gaussian contribution statistics (gsr_contrib_stats) on one MI355X.

    python tools/bench_contrib.py [--config 1m_1080p_sh3] [--reps 30] [--rounds 5]

One JSON line: the statistics call (without and with a per-pixel weight map, and on copies of the buffers, which
take the checkpoint-free walk) and, for comparison, the backward call on the same forward, each timed with device
events around ``reps`` back-to-back calls, the four alternating for
``rounds`` rounds; reported are the medians and every round.  Before timing, the result is checked for what holds
at any size: the sums telescope to the accumulated alpha, weight_sum >= weight_max, pixel_count > 0 iff
weight_sum > 0, culled rows are zero, a second call gives the same maximum and count bit for bit, and a backward
after the call is the backward without it (closely on the atomic path, bit for bit on the record path).
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
    assert torch.cuda.is_available(), "bench_contrib needs a HIP device"
    dev = "cuda"
    cfg = syn.CONFIGS[a.config]
    W, H = cfg["width"], cfg["height"]
    scene, cam = syn.config_scene(a.config, seed=0, yaw_deg=5.0)
    sc = scene.to(dev)
    e = torch.Tensor([]).to(dev)
    bg = torch.zeros(3, device=dev)
    view, proj, campos = cam.viewmatrix.to(dev), cam.projmatrix.to(dev), cam.campos.to(dev)
    gc, gd = (t.to(dev) for t in syn.upstream_grads(H, W))
    wmap = torch.rand(H, W, generator=torch.Generator().manual_seed(11)).to(dev) + 0.5

    def forward():
        return _C.rasterize_gaussians(bg, sc.means3D, e, sc.opacities, sc.scales, sc.rotations, 1.0, e, view, proj,
                                      cam.tanfovx, cam.tanfovy, H, W, sc.shs, scene.sh_degree, campos, False, False,
                                      False, return_alpha=True)

    nr, _color, radii, geom, binning, img, _invd, alpha = forward()

    def backward(buffers=(geom, binning, img)):
        g, b, i = buffers
        return _C.rasterize_gaussians_backward(bg, sc.means3D, radii, e, sc.opacities, sc.scales, sc.rotations, 1.0, e,
                                               view, proj, cam.tanfovx, cam.tanfovy, gc, gd, sc.shs, scene.sh_degree,
                                               campos, g, nr, b, i, False, False)

    def stats(weight=None, buffers=(geom, binning, img)):
        return _C.contribution_stats(*buffers, nr, scene.P, H, W, pixel_weight=weight)

    # buffers the library has not seen (copies): every unit re-walks its tile's list for T instead of reading the
    # forward's checkpoint (csrc/contrib.hip CKPT), as after a whole-tile ("fwd_quads" 4) forward
    copies = tuple(t.clone() for t in (geom, binning, img))

    st = stats(wmap)
    after = backward()
    f2 = forward()
    fresh = backward(f2[3:6])
    atomic = _lib.option_get("bwd_atomic")
    for x, y in zip(after, fresh):
        if atomic:
            assert float((x - y).abs().max()) <= 2e-4 * max(float(x.abs().max()), 1e-30), "the backward moved"
        else:
            assert torch.equal(x, y), "the backward moved"
    s, mx, cnt, sw = st[:, 0].double(), st[:, 1], st.view(torch.int32)[:, 2], st[:, 3]
    total = float(alpha.double().sum())
    assert abs(float(s.sum()) - total) <= 1e-5 * total, "the sums do not telescope to the accumulated alpha"
    assert bool((st[:, 0] >= mx).all()) and bool(((cnt > 0) == (st[:, 0] > 0)).all())
    assert not st[radii == 0].view(torch.int32).any()
    again = stats(wmap)
    assert torch.equal(again[:, 1:3].view(torch.int32), st[:, 1:3].view(torch.int32)), "maximum / count not reproducible"
    assert float(sw.sum()) > 0 and not stats()[:, 3].any()
    rewalk = stats(wmap, copies)
    assert torch.equal(rewalk[:, 1:3].view(torch.int32), st[:, 1:3].view(torch.int32)), "the checkpoint-free walk differs"

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / a.reps  # us per call

    calls = {"stats": stats, "stats_weighted": lambda: stats(wmap), "stats_rewalk": lambda: stats(None, copies),
             "backward": backward}
    for _ in range(5):  # warm-up of every shape
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            rounds[k].append(timed(fn))
    res = {"metric": "contribution statistics device time", "config": a.config, "P": scene.P, "num_rendered": int(nr),
           "unit": "us", "reps_per_round": a.reps, "bwd_atomic": atomic,
           "rows_contributing": int((cnt > 0).sum()), "pairs": int(cnt.long().sum()),
           "max_pixel_count": int(cnt.max()), "max_weight": round(float(mx.max()), 4)}
    for k, v in rounds.items():
        res[k + "_us"] = statistics.median(v)
        res[k + "_us_rounds"] = [round(x, 1) for x in v]
    res["value"] = res["stats_us"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
