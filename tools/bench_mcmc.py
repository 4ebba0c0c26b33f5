#!/usr/bin/env python3
"""Measure the 3DGS-MCMC kernels (gsr_mcmc_noise, gsr_mcmc_relocation + gsr_mcmc_apply) on one MI355X against the
torch formulation of the same steps, written here; the torch formulation is the baseline, not the product.

    python tools/bench_mcmc.py [--points 1000000] [--fraction 0.05] [--reps 50] [--noise-reps 5000] [--sets 6]
                               [--rounds 7]

One JSON line.  Each entry is timed with device events around back-to-back calls (``reps``; ``noise-reps`` for the
fused noise, so that its window is tens of milliseconds too), the entries alternating for ``rounds`` rounds after a
warm-up of every shape; medians and every round are reported.
  noise_fused       gsr_mcmc_noise through the C ABI: one kernel, in place
  noise_torch       build_rotation, L = R S, Sigma = L L^T, bmm(Sigma, xi * gate * scale), xyz.add_
                    (both rotate over ``sets`` copies of the inputs, together larger than the Infinity Cache, so every
                    call reads from HBM as it does between two training iterations)
  relocate_fused    mcmc.relocation + mcmc.apply_relocation on a GaussianModel-shaped set of groups (SH degree 3, Adam
                    moments everywhere), ``fraction`` of the Gaussians relocated; the Python faces as a user calls
                    them, index checks and their host reads included
  relocate_kernels  gsr_mcmc_relocation + gsr_mcmc_apply alone (the memset and eight launches behind relocate_fused)
  relocate_torch    bincount, the float64 single sum over a gathered coefficient table, indexed row copies and moment
                    resets per group (no index checks)
The noise kernel's achieved bytes/s use the 68 B per Gaussian it has to move (56 read, 12 written).  Before timing,
the fused results are checked against the torch formulation (noise 1e-5; relocation 1e-6, copies bitwise).
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussian_splatting_amd import _lib, mcmc  # noqa: E402

NOISE_BYTES = 68
HBM_ACHIEVABLE = 6.3e12  # B/s, streaming


def build_rotation(r):
    q = r / torch.norm(r, dim=1, keepdim=True)
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def noise_torch(xyz, opacity_raw, scaling_raw, rotation, xi, noise_scale):
    L = build_rotation(rotation) * torch.exp(scaling_raw)[:, None, :]
    sigma = L @ L.transpose(1, 2)
    gate = torch.sigmoid(-100.0 * (torch.sigmoid(opacity_raw) - 0.005))
    xyz.add_(torch.bmm(sigma, (xi * gate * noise_scale)[:, :, None]).squeeze(-1))


def coefficient_table(device, n_max=mcmc.N_MAX):
    """coef[N, k] = C(N, k+1) (-1)^k / sqrt(k+1), float64 (zero for k >= N)."""
    t = torch.zeros((n_max + 1, n_max), dtype=torch.float64)
    for N in range(1, n_max + 1):
        for k in range(N):
            t[N, k] = math.comb(N, k + 1) * (-1.0) ** k / math.sqrt(k + 1)
    return t.to(device)


def relocate_torch(groups, opacity_raw, scaling_raw, sampled, dest, coef, min_opacity=0.005):
    P = opacity_raw.shape[0]
    ratio = (torch.bincount(sampled, minlength=P)[sampled] + 1).clamp_(max=mcmc.N_MAX)
    o = torch.sigmoid(opacity_raw.double().reshape(-1)[sampled])
    x = -torch.expm1(torch.log1p(-o) / ratio)
    powers = torch.cumprod(x[:, None].expand(-1, coef.shape[1]), dim=1)
    den = (coef[ratio] * powers).sum(1)
    new_op = torch.logit(x.clamp(min_opacity, 1.0 - 2.0 ** -23)).float()[:, None]
    new_sc = (scaling_raw.double()[sampled] + torch.log(o / den)[:, None]).float()
    for data, m, v, role in groups:
        if role == mcmc.OPACITY:
            data[dest] = new_op
            data[sampled] = new_op
        elif role == mcmc.SCALING:
            data[dest] = new_sc
            data[sampled] = new_sc
        else:
            data[dest] = data[sampled]
        m[sampled] = 0
        v[sampled] = 0
    return new_op, new_sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--fraction", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--noise-reps", type=int, default=5000)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mcmc needs a HIP device"
    dev = torch.device("cuda", 0)
    P = a.points
    gen = torch.Generator(device=dev).manual_seed(0)

    def uniform(lo, hi, *shape):
        return torch.rand(shape, device=dev, generator=gen) * (hi - lo) + lo

    xyz = uniform(-3, 3, P, 3)
    opacity = uniform(-9, 3, P, 1)
    scaling = uniform(-5, -2.5, P, 3)
    rotation = torch.randn((P, 4), device=dev, generator=gen)
    xi = torch.randn((P, 3), device=dev, generator=gen)
    noise_scale = 5e5 * 1.6e-4

    # the fused kernel computes what the torch formulation computes
    a_xyz, b_xyz = xyz.clone(), xyz.clone()
    mcmc.noise(a_xyz, opacity, scaling, rotation, xi, noise_scale)
    noise_torch(b_xyz, opacity, scaling, rotation, xi, noise_scale)
    noise_err = float((a_xyz - b_xyz).abs().max())
    moved = float((a_xyz - xyz).abs().median())
    assert noise_err <= 1e-5 and moved > 0, (noise_err, moved)

    # relocation: `fraction` of the rows are destinations, their sources drawn from the others by opacity
    n = int(a.fraction * P)
    perm = torch.randperm(P, device=dev, generator=gen)
    dest, alive = perm[:n].contiguous(), perm[n:]
    sampled = alive[torch.multinomial(torch.sigmoid(opacity[alive, 0]), n, replacement=True, generator=gen)]
    shapes = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
    base = {"xyz": xyz, "opacity": opacity, "scaling": scaling, "rotation": rotation}
    roles = {name: role for name, _, role in mcmc.GROUPS}

    def make_groups():
        out = []
        for name, shape in shapes.items():
            data = base[name].clone() if name in base else torch.randn((P,) + shape, device=dev, generator=gen)
            out.append((data, torch.randn_like(data), torch.rand_like(data), roles[name]))
        return out

    coef = coefficient_table(dev)
    g_fused, g_torch = make_groups(), make_groups()
    for fused, other in zip(g_fused, g_torch):
        for t0, t1 in zip(fused[:3], other[:3]):
            t1.copy_(t0)

    def relocate_fused(groups=g_fused):
        new_op, new_sc, _ = mcmc.relocation(opacity, scaling, sampled)
        mcmc.apply_relocation(groups, sampled, dest, new_op, new_sc)
        return new_op, new_sc

    f_op, f_sc = relocate_fused()
    t_op, t_sc = relocate_torch(g_torch, opacity, scaling, sampled, dest, coef)
    reloc_err = max(float((f_op - t_op).abs().max()), float((f_sc - t_sc).abs().max()))
    assert reloc_err <= 1e-6 * max(1.0, float(t_op.abs().max()), float(t_sc.abs().max())), reloc_err
    for (d0, m0, v0, role), (d1, m1, v1, _) in zip(g_fused, g_torch):
        if role == mcmc.COPY:
            assert torch.equal(d0, d1)
        assert torch.equal(m0, m1) and torch.equal(v0, v1)

    # the noise is timed HBM-cold, as a training iteration leaves it: the calls rotate over `sets` copies of the five
    # arrays (56 MB each at 1M), together larger than the 256 MiB Infinity Cache
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    sets = [tuple(t.clone() for t in (xyz, opacity, scaling, rotation, xi)) for _ in range(a.sets)]
    ptrs = [tuple(t.data_ptr() for t in s) for s in sets]

    def noise_fused(i):
        rc = lib.gsr_mcmc_noise(P, *ptrs[i % a.sets], noise_scale, stream)
        assert rc == 0, rc

    # the two relocation entry points alone, as relocate_fused calls them after its checks
    scratch = torch.empty(int(lib.gsr_mcmc_scratch_bytes(P)), dtype=torch.uint8, device=dev)
    k_op, k_sc = torch.empty_like(f_op), torch.empty_like(f_sc)
    k_ratio = torch.empty(n, dtype=torch.int32, device=dev)
    k_groups = (_lib.McmcGroup * len(g_fused))(*[
        _lib.McmcGroup(d.data_ptr(), m.data_ptr(), v.data_ptr(), int(math.prod(d.shape[1:])), role)
        for d, m, v, role in g_fused])

    def relocate_kernels(i):
        rc = lib.gsr_mcmc_relocation(P, n, opacity.data_ptr(), scaling.data_ptr(), sampled.data_ptr(), mcmc.N_MAX, 0.005,
                                     scratch.data_ptr(), k_op.data_ptr(), k_sc.data_ptr(), k_ratio.data_ptr(), stream)
        rc = rc or lib.gsr_mcmc_apply(P, n, sampled.data_ptr(), dest.data_ptr(), k_op.data_ptr(), k_sc.data_ptr(),
                                      k_groups, len(g_fused), stream)
        assert rc == 0, rc

    def timed(fn, reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(reps):
            fn(i)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / reps  # us per call

    calls = {"noise_fused": (noise_fused, a.noise_reps),
             "noise_torch": (lambda i: noise_torch(*sets[i % a.sets], noise_scale), a.reps),
             "relocate_fused": (lambda i: relocate_fused(), a.reps),
             "relocate_kernels": (relocate_kernels, a.reps),
             "relocate_torch": (lambda i: relocate_torch(g_torch, opacity, scaling, sampled, dest, coef), a.reps)}
    for fn, _ in calls.values():  # warm-up of every shape (and every set)
        for i in range(2 * a.sets):
            fn(i)
    torch.cuda.synchronize()
    rounds = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, (fn, reps) in calls.items():
            rounds[k].append(timed(fn, reps))
    res = {"metric": "3DGS-MCMC step device time", "unit": "us", "P": P, "n_relocated": n,
           "reps_per_round": a.reps, "noise_reps_per_round": a.noise_reps, "noise_buffer_sets": a.sets,
           "rounds": a.rounds, "command": "python tools/bench_mcmc.py " + " ".join(sys.argv[1:]),
           "noise_max_abs_diff_vs_torch": noise_err, "relocation_max_abs_diff_vs_torch": reloc_err}
    for k, v in rounds.items():
        res[k + "_us"] = round(statistics.median(v), 2)
        res[k + "_us_rounds"] = [round(x, 2) for x in v]
    res["noise_bytes_per_gaussian"] = NOISE_BYTES
    res["noise_fused_TBps"] = round(NOISE_BYTES * P / (res["noise_fused_us"] * 1e-6) / 1e12, 3)
    res["noise_fused_share_of_achievable_hbm"] = round(res["noise_fused_TBps"] * 1e12 / HBM_ACHIEVABLE, 3)
    res["noise_speedup_vs_torch"] = round(res["noise_torch_us"] / res["noise_fused_us"], 2)
    res["relocate_speedup_vs_torch"] = round(res["relocate_torch_us"] / res["relocate_fused_us"], 2)
    res["relocate_kernels_speedup_vs_torch"] = round(res["relocate_torch_us"] / res["relocate_kernels_us"], 2)
    res["value"] = res["noise_fused_us"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
