"""Reference for the per-pixel selections (include/gsr.h gsr_render_select / gsr_render_median_backward), built on the
unchanged oracle.  TEST INFRASTRUCTURE ONLY (shared by tests/test_select_ref.py and tests/test_gpu_select.py).

Per pixel, from the blend weights ``w[pix, g]`` of tests/contrib_ref.py (one one-hot oracle backward per pixel) and the
oracle's own tile lists (``ref.handle.binning()``: ``point_list``, ``ranges``), which fix the order 1..n of the pixel's
contributors -- the entries of its tile's list with ``w > 0``.  In float64:

    T_i = 1 - sum_{j<i} w_j                          (w_j = T_j - T_{j+1})
    median: the last i with T_i > 0.5                (2DGS's rule, T before entry i is blended)
    top-K:  a stable descending sort of w            (equal weights keep list order)

and per pixel a ``decided`` flag each: the median is decided iff ``min_i |T_i - 0.5| > MARGIN`` and the top-K iff every
pair of adjacent ranks among the first ``K + 1`` differs by more than ``MARGIN`` relative to the larger of the two, with
``MARGIN = 1e-5``, the project's forward bar (ATOL_FWD): a float32 blend within that of a tie may legitimately select
the other contributor.
"""
from __future__ import annotations

import numpy as np

from tests import common as C
from tests import contrib_ref as CR

MARGIN = 1e-5


def select_pixel(w, ids, K, t=None) -> dict:
    """One pixel's selections from its contributors' weights ``w`` [n] and Gaussian indices ``ids`` [n] in list order
    (float64 arithmetic): ``median_id``, ``median`` (``t[median_id]``, 0.0 without a contributor or without ``t``),
    ``topk_ids`` [K] (-1 padded), ``topk_weights`` [K] (0 padded), ``decided_median``, ``decided_topk``."""
    w = np.asarray(w, np.float64)
    ids = np.asarray(ids, np.int64)
    out = dict(median_id=-1, median=0.0, topk_ids=np.full(K, -1, np.int64), topk_weights=np.zeros(K),
               decided_median=True, decided_topk=True)
    if w.size == 0:
        return out
    T = 1.0 - np.concatenate([[0.0], np.cumsum(w)[:-1]])  # T_i, before entry i is blended
    m = int(np.flatnonzero(T > 0.5)[-1])  # (T_1 = 1: never empty)
    out["median_id"] = int(ids[m])
    out["median"] = float(t[ids[m]]) if t is not None else 0.0
    out["decided_median"] = bool(np.abs(T - 0.5).min() > MARGIN)
    order = np.argsort(-w, kind="stable")
    k = min(K, w.size)
    out["topk_ids"][:k] = ids[order[:k]]
    out["topk_weights"][:k] = w[order[:k]]
    head = w[order[:K + 1]]
    out["decided_topk"] = bool((head[:-1] - head[1:] > MARGIN * head[:-1]).all())
    return out


def pixel_lists(ref, H, W):
    """For every pixel (flat, row-major) its tile's list of Gaussian indices in the oracle's order."""
    b = ref.handle.binning()
    pl, ranges = b["point_list"].astype(np.int64), b["ranges"].astype(np.int64)
    gx = (W + 15) // 16
    return [pl[ranges[(y // 16) * gx + x // 16, 0]:ranges[(y // 16) * gx + x // 16, 1]]
            for y in range(H) for x in range(W)]


def oracle_select(inp, K, t=None, nthreads=1, ref=None, w=None) -> dict:
    """The reference selections of ``inp`` (read-only arrays): ``median_ids`` [H,W] int64, ``median`` [H,W] float64
    (``t`` float32 [P] copied exactly), ``topk_ids`` / ``topk_weights`` [K,H,W], ``decided_median`` / ``decided_topk``
    [H,W] bool, ``crosses`` [H,W] bool (the transmittance reaches one half), ``count`` [H,W] (contributors), ``lists``
    (``pixel_lists``) and ``n_contrib`` [H,W].  ``ref`` / ``w``: the oracle forward of ``inp`` and its per-pixel
    weights, if the caller has them."""
    ref = C.run_oracle(inp, nthreads=nthreads) if ref is None else ref
    H, W = inp["H"], inp["W"]
    w = CR.per_pixel_weights(ref, H, W, nthreads) if w is None else w
    tn = None if t is None else np.asarray(t.numpy() if hasattr(t, "numpy") else t, np.float32)
    lists = pixel_lists(ref, H, W)
    N = H * W
    out = dict(median_ids=np.full(N, -1, np.int64), median=np.zeros(N), topk_ids=np.full((K, N), -1, np.int64),
               topk_weights=np.zeros((K, N)), decided_median=np.ones(N, bool), decided_topk=np.ones(N, bool),
               crosses=np.zeros(N, bool), count=np.zeros(N, np.int64))
    for pix in range(N):
        lst = lists[pix]
        wl = w[pix, lst]
        on = wl > 0
        assert int(on.sum()) == int((w[pix] > 0).sum())  # every contributor is on the pixel's tile's list, once
        r = select_pixel(wl[on], lst[on], K, tn)
        out["median_ids"][pix], out["median"][pix] = r["median_id"], r["median"]
        out["topk_ids"][:, pix], out["topk_weights"][:, pix] = r["topk_ids"], r["topk_weights"]
        out["decided_median"][pix], out["decided_topk"][pix] = r["decided_median"], r["decided_topk"]
        out["crosses"][pix] = 1.0 - float(wl[on].astype(np.float64).sum()) <= 0.5
        out["count"][pix] = int(on.sum())
    for k in ("median_ids", "median", "decided_median", "decided_topk", "crosses", "count"):
        out[k] = out[k].reshape(H, W)
    for k in ("topk_ids", "topk_weights"):
        out[k] = out[k].reshape(K, H, W)
    out["n_contrib"] = ref.handle.image()["n_contrib"].astype(np.int64)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    out["lists"] = lists
    return out


def scatter_backward(median_ids, U, P) -> np.ndarray:
    """``dL_dt`` [P] float64 of the median map: ``np.bincount`` of the upstream ``U`` over the pixels' median ids."""
    ids = np.asarray(median_ids).reshape(-1)
    u = np.asarray(U, np.float64).reshape(-1)
    keep = ids >= 0
    return np.bincount(ids[keep], weights=u[keep], minlength=P)[:P]
