"""CPU checks of the contribution-statistics reference (tests/contrib_ref.py) that tests/test_gpu_contrib.py holds the
kernel to, and of ``densify.prune_mask_by_contribution``.

The reference takes the per-pixel blend weights from one oracle backward per pixel.  Pinned here, on the oracle
alone: the per-pixel sums equal the single backward's column (1e-6 of its maximum: float32 summation of up to a few
hundred terms), the telescoping identity sum_g weight_sum = sum_pix (1 - final_T) (1e-6 relative; every blended
weight is T_before - T_after), and 0 < weight_max <= 0.99 (alpha's clamp, T <= 1) on contributing rows.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import common as C
from tests import contrib_ref as CR

# partial edge tiles; 115 culled rows; one tile of 10000 entries (54 blend, one near-threshold pixel)
NAMES = ["ragged_37x23", "pose_clamped", "lists_over_8k"]


def _case(name):
    return next(c for c in C.SMALL_CASES + C.POSE_CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def _ref(name):
    inp = C.build(_case(name))
    nt = 4 if name.startswith("lists_") else 1
    ref = C.run_oracle(inp, nthreads=nt)
    return inp, ref, CR.oracle_contrib(inp, CR.weight_map(inp["H"], inp["W"]), nthreads=nt, ref=ref)


@pytest.mark.parametrize("name", NAMES)
def test_per_pixel_weights_sum_to_the_one_call_column(name):
    _inp, _ref32, r = _ref(name)
    for a, b, tag in ((r["weight_sum"], r["one_call_sum"], "sum"), (r["weighted_sum"], r["one_call_weighted"], "weighted")):
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"[{name}] {tag}: {err:.1e} of max {np.abs(b).max():.4g}")
        assert err <= 1e-6, (tag, err)


@pytest.mark.parametrize("name", NAMES)
def test_telescoping_identity(name):
    _inp, _ref32, r = _ref(name)
    total = (1.0 - r["final_T"]).sum()
    err = abs(r["weight_sum"].sum() - total) / total
    print(f"[{name}] sum_g weight_sum = {r['weight_sum'].sum():.6f}, sum_pix (1 - final_T) = {total:.6f}: {err:.1e}")
    assert err <= 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_maximum_count_and_culled_rows(name):
    _inp, ref32, r = _ref(name)
    con = r["pixel_count"] > 0
    assert con.any() and (r["weight_max"][con] > 0).all() and (r["weight_max"] <= 0.99).all()
    assert (r["weight_sum"][con] >= r["weight_max"][con]).all()
    assert not r["weight_sum"][~con].any() and not r["weight_max"][~con].any()
    culled = ref32.radii == 0
    assert not con[culled].any()
    if name == "pose_clamped":
        assert int(culled.sum()) == 115
    # a pixel's contributors are the n_contrib entries the reference's walk ends at, minus the skipped ones
    per_pixel = (r["w"] > 0).sum(1).reshape(r["final_T"].shape)
    assert (per_pixel <= ref32.handle.image()["n_contrib"]).all()
    assert r["flagged"].sum() == {"ragged_37x23": 0, "pose_clamped": 0, "lists_over_8k": 1}[name]


def test_prune_mask_by_contribution():
    from gaussian_splatting_amd.densify import prune_mask_by_contribution as pm

    score = torch.tensor([0.5, 0.1, 0.5, 0.0, 0.9, 0.5, 0.1])
    P = score.numel()
    for ratio in (0.0, 0.1, 0.3, 0.5, 4 / 7, 1.0):
        mask = pm(score, keep_ratio=ratio)
        assert mask.dtype == torch.bool and tuple(mask.shape) == (P,)
        assert int((~mask).sum()) == math.ceil(ratio * P)
    # ties by index: three rows score 0.5; keeping 3 rows keeps 0.9 and the first two of them
    assert (~pm(score, keep_ratio=3 / 7)).nonzero().flatten().tolist() == [0, 2, 4]
    assert (~pm(score, keep_ratio=2 / 7)).nonzero().flatten().tolist() == [0, 4]
    assert pm(score, threshold=0.2).tolist() == [False, True, False, True, False, False, True]
    # both: kept only if both keep it
    assert (~pm(score, keep_ratio=1.0, threshold=0.6)).nonzero().flatten().tolist() == [4]
    assert (~pm(score, keep_ratio=2 / 7, threshold=0.05)).nonzero().flatten().tolist() == [0, 4]
    # any shape of P values, a column view of a statistics tensor included; ~mask is prune_points' valid_points_mask
    stats = torch.zeros(P, 4)
    stats[:, 1] = score
    assert torch.equal(pm(stats[:, 1], keep_ratio=0.5), pm(score, keep_ratio=0.5))
    assert pm(torch.zeros(0), keep_ratio=0.5).numel() == 0
    with pytest.raises(ValueError):
        pm(score)
    with pytest.raises(ValueError):
        pm(score, keep_ratio=1.5)


def test_split_names_the_columns():
    from gaussian_splatting_amd.contrib import ContributionStats, split

    stats = torch.arange(12, dtype=torch.float32).reshape(3, 4).clone()
    stats.view(torch.int32)[:, 2] = torch.tensor([7, 0, 2 ** 31 - 1], dtype=torch.int32)
    s = split(stats)
    assert isinstance(s, ContributionStats)
    assert s.weight_sum.tolist() == [0.0, 4.0, 8.0] and s.weight_max.tolist() == [1.0, 5.0, 9.0]
    assert s.pixel_count.dtype == torch.int32 and s.pixel_count.tolist() == [7, 0, 2 ** 31 - 1]
    assert s.weighted_sum.tolist() == [3.0, 7.0, 11.0]
    s.weight_sum[0] = 5.0  # views, not copies
    assert stats[0, 0] == 5.0
    with pytest.raises(RuntimeError):
        split(torch.zeros(3, 3))
