"""The masked large-k search's threshold helper on hand-made candidate blocks, and the CPU shard
at k = 100 under a mask and over tombstones (it keeps the chunked matmul: this pins that the CPU
behaviour did not move)."""
import math

import numpy as np
import torch

from codename_symbiont_amd.index.shard import HbmIndexShard, filter_large_k_threshold
from codename_symbiont_amd.ops import reference as R

INF = math.inf


def test_threshold_is_the_kth_largest_finite_entry_less_the_margin():
    cand = torch.tensor([
        [0.5, -INF, 0.9, 0.1, -INF, 0.7, 0.3, -INF],     # 5 finite
        [-INF, -INF, 0.2, -INF, -INF, -INF, 0.4, -INF],  # 2 finite
        [-INF] * 8,                                      # none
        [-0.5, -0.1, -0.9, -0.2, -0.3, -0.4, -0.6, -0.7],
        [0.25] * 8,                                      # equal scores are distinct rows
    ])
    m = 2.0 ** -12
    t3 = filter_large_k_threshold(cand, 3, m)
    assert t3.dtype == torch.float32 and t3.shape == (5,) and t3.is_contiguous()
    assert torch.equal(t3, torch.tensor([0.5 - m, -INF, -INF, -0.3 - m, 0.25 - m]))
    t5 = filter_large_k_threshold(cand, 5, m)
    assert torch.equal(t5, torch.tensor([0.1 - m, -INF, -INF, -0.5 - m, 0.25 - m]))
    assert torch.equal(filter_large_k_threshold(cand, 8, 0.0),
                       torch.tensor([-INF, -INF, -INF, -0.9, 0.25]))
    # a block narrower than k holds fewer than k entries
    assert torch.equal(filter_large_k_threshold(cand, 9, m), torch.full((5,), -INF))
    # the margin only lowers
    assert bool((filter_large_k_threshold(cand, 1, 0.5) <= filter_large_k_threshold(cand, 1, 0.0)).all())


def test_threshold_ignores_entries_that_are_not_scores():
    """A gated-off seed pass leaves its block unwritten: NaN and +inf count as missing."""
    cand = torch.tensor([[math.nan, 0.5, INF, 0.25, -INF, 0.125]])
    assert torch.equal(filter_large_k_threshold(cand, 2, 0.0), torch.tensor([0.25]))
    assert torch.equal(filter_large_k_threshold(cand, 4, 0.0), torch.tensor([-INF]))


def test_threshold_is_a_lower_bound_on_the_kth_best_of_any_superset():
    g = torch.Generator().manual_seed(3)
    full = torch.randn(7, 500, generator=g)
    sub = full[:, ::9].clone()
    sub[:, ::4] = -INF
    k = 10
    kth_full = torch.topk(full, k, dim=1).values[:, k - 1]
    assert bool((filter_large_k_threshold(sub, k, 2.0 ** -12) < kth_full).all())


def _cpu_check(s, r, rows, q, k, allow):
    ref_s, ref_i = R.filtered_topk_ref(rows, q, k, allow)
    fin = torch.isfinite(ref_s)
    assert s.shape == (q.shape[0], k) and r.dtype == torch.int32
    assert torch.equal(torch.isfinite(s), fin)
    assert bool((r[~fin] == -1).all())
    assert bool(allow[r.long()[fin]].all())
    assert float((s[fin] - ref_s[fin]).abs().max()) <= 2e-3
    hit = ((r.long()[:, :, None] == ref_i[:, None, :]) & fin[:, :, None]).any(-1).sum()
    assert float(hit) / float(fin.sum()) > 0.995


def test_cpu_shard_k100_under_a_mask_and_over_tombstones():
    D, n, k, nq = 384, 64 * 37 + 19, 100, 9
    sh = HbmIndexShard(D, n + 100, device="cpu")
    sh.fill_random(n, seed=5)
    assert not sh._filter_large_k_serves(k)
    g = torch.Generator().manual_seed(11)
    q = torch.nn.functional.normalize(torch.randn(nq, D, generator=g), dim=-1).bfloat16()
    rows = sh.unit_rows()[:n].clone()
    rng = np.random.default_rng(4)
    for allow in (torch.from_numpy(rng.random(n) < 0.5), torch.from_numpy(rng.random(n) < 0.02)):
        s, r = sh.search(q, k, allow=allow)
        _cpu_check(s, r, rows, q, k, allow)
    dead = torch.from_numpy(rng.random(n) < 0.05)
    dead[700:1000] = True
    sh.delete_rows(torch.nonzero(dead).flatten())
    s, r = sh.search(q, k)
    _cpu_check(s, r, rows, q, k, ~dead)
    assert not bool(dead[r.long().clamp_min(0)].any())
