"""The 3DGS-MCMC reference (include/gsr_mcmc.h): numpy, float64 throughout, the formulas taken literally -- the
relocation's double sum with ``math.comb``, the rewritten gate, ``Sigma = R diag(s^2) R^T`` as a matrix product.
tests/test_mcmc_ref.py pins it with known answers; tests/test_gpu_mcmc.py holds the kernels to it.
"""
import math

import numpy as np

N_MAX = 51
GATE_K, GATE_X0 = 100.0, 0.005
FLT_EPSILON = float(np.finfo(np.float32).eps)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p / (1.0 - p))


def gate(o):
    """1 / (1 + exp(k (o - x0))): the paper's sigmoid(100 ((1 - o) - 0.995)) without forming 1 - o."""
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(GATE_K * (np.asarray(o, np.float64) - GATE_X0)))


def gate_paper(o):
    o = np.asarray(o, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-(100.0 * ((1.0 - o) - 0.995))))


def build_rotation(q):
    """R(q) [P, 3, 3] of raw quaternions (r, x, y, z), normalised first (utils/general_utils.py:78-99)."""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
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


def noise_delta(opacity_raw, scaling_raw, rotation, xi, noise_scale):
    """Sigma @ (xi * gate * noise_scale), [P, 3] float64."""
    o = sigmoid(np.asarray(opacity_raw).reshape(-1))
    s = np.exp(np.asarray(scaling_raw, np.float64))
    R = build_rotation(rotation)
    sigma = np.einsum("pij,pj,pkj->pik", R, s * s, R)
    v = np.asarray(xi, np.float64) * (gate(o) * float(noise_scale))[:, None]
    return np.einsum("pij,pj->pi", sigma, v)


def noise(xyz, opacity_raw, scaling_raw, rotation, xi, noise_scale):
    return np.asarray(xyz, np.float64) + noise_delta(opacity_raw, scaling_raw, rotation, xi, noise_scale)


def ratios(sampled, n_max=N_MAX):
    """N_j = min(count[sampled[j]] + 1, n_max), int32 [n]."""
    sampled = np.asarray(sampled, np.int64)
    count = np.bincount(sampled, minlength=int(sampled.max()) + 1 if sampled.size else 0)
    return np.minimum(count[sampled] + 1, n_max).astype(np.int32)


def relocate_x(o, N):
    """x = 1 - (1 - o)^(1/N) (o = 1, where float64's sigmoid saturates, gives 1)."""
    with np.errstate(divide="ignore"):
        return float(-np.expm1(np.log1p(-np.float64(o)) / N))


def denominator(x, N):
    """sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k x^(k+1) / sqrt(k+1)."""
    den = 0.0
    for i in range(1, N + 1):
        for k in range(i):
            den += math.comb(i - 1, k) * (-1.0) ** k * x ** (k + 1) / math.sqrt(k + 1)
    return den


def scale_factor(o, N):
    """o / den: what the source's scale is multiplied by."""
    return float(o) / denominator(relocate_x(o, N), N)


def relocation(opacity_raw, scaling_raw, sampled, n_max=N_MAX, min_opacity=0.005):
    """(new_opacity_raw [n, 1], new_scaling_raw [n, 3], ratio [n]) in float64 (ratio int32)."""
    op = np.asarray(opacity_raw, np.float64).reshape(-1)
    sc = np.asarray(scaling_raw, np.float64)
    sampled = np.asarray(sampled, np.int64)
    ratio = ratios(sampled, n_max)
    new_op = np.empty((len(sampled), 1))
    new_sc = np.empty((len(sampled), 3))
    for j, (s, N) in enumerate(zip(sampled, ratio)):
        o = float(sigmoid(op[s]))
        x = relocate_x(o, int(N))
        new_op[j, 0] = logit(min(max(x, float(min_opacity)), 1.0 - FLT_EPSILON))
        new_sc[j] = sc[s] + math.log(o / denominator(x, int(N)))
    return new_op, new_sc, ratio


def apply(params, moments, sampled, dest, new_op, new_sc):
    """The row surgery on copies: ``params`` {name: [P, ...] float32}, ``moments`` {name: (exp_avg, exp_avg_sq)} for the
    groups that have state; "opacity" and "scaling" take ``new_op`` / ``new_sc`` (rounded to float32) at both ``dest``
    and ``sampled``, every other group copies row sampled -> dest; moments become zero at ``sampled``."""
    sampled, dest = np.asarray(sampled, np.int64), np.asarray(dest, np.int64)
    out = {k: v.copy() for k, v in params.items()}
    mom = {k: (m.copy(), v.copy()) for k, (m, v) in moments.items()}
    for k, arr in out.items():
        if k == "opacity":
            val = np.asarray(new_op, np.float64).astype(np.float32).reshape((-1,) + arr.shape[1:])
            arr[dest] = val
            arr[sampled] = val
        elif k == "scaling":
            val = np.asarray(new_sc, np.float64).astype(np.float32)
            arr[dest] = val
            arr[sampled] = val
        else:
            arr[dest] = params[k][sampled]
        if k in mom:
            mom[k][0][sampled] = 0
            mom[k][1][sampled] = 0
    return out, mom
