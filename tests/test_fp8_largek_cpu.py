"""Host-side pieces of the fp8 large-k route (index/shard.py): which shards the emitting e4m3
scan serves, the internal all-rows mask, the one-ulp threshold, and that a CPU fp8 shard keeps
the chunked matmul."""
import math

import numpy as np
import torch

from codename_symbiont_amd.index import shard as S
from codename_symbiont_amd.ops import reference as R


def _cpu_shard(D=256, n=500, cap=700, dtype="fp8"):
    sh = S.HbmIndexShard(D, cap, device="cpu", dtype=dtype)
    sh.fill_random(n, seed=3)
    return sh


def _queries(nq, D, seed=11):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(nq, D, generator=g), dim=-1).bfloat16()


def test_which_shards_the_route_serves():
    assert S.FILTER_LARGE_K_FP8_DIMS == S.FILTER_FP8_DIMS
    assert S.HbmIndexShard.FP8_LARGE_K_MIN_ROWS == S.HbmIndexShard.SEED_MIN_ROWS == 1 << 20
    sh = _cpu_shard()
    sh.FP8_LARGE_K_MIN_ROWS = 0
    assert not any(sh._filter_large_k_serves(k) for k in (1, 32, 33, 100, 128, 129))   # a CPU shard
    # the predicate reads the device's type only, so a GPU shard's answers can be asked here
    sh.device = torch.device("cuda")
    try:
        assert [k for k in (1, 16, 32, 33, 100, 128, 129, 1000) if sh._filter_large_k_serves(k)] \
            == [33, 100, 128]
        del sh.FP8_LARGE_K_MIN_ROWS                        # the default gate: 500 rows are below it
        assert not any(sh._filter_large_k_serves(k) for k in (33, 100, 128))
        sh.FP8_LARGE_K_MIN_ROWS = 500
        assert sh._filter_large_k_serves(100)
        sh.FP8_LARGE_K_MIN_ROWS = 501
        assert not sh._filter_large_k_serves(100)
        sh.FP8_LARGE_K_MIN_ROWS, sh.dim = 0, 320           # a width the scan is not built for
        assert not sh._filter_large_k_serves(100)
    finally:
        sh.device = torch.device("cpu")
    # a bf16 shard's answer does not depend on the fp8 gate
    b = _cpu_shard(384, dtype="bf16")
    b.device = torch.device("cuda")
    try:
        assert b._filter_large_k_serves(100) == bool(b.scan_mq)
        assert not b._filter_large_k_serves(32) and not b._filter_large_k_serves(129)
    finally:
        b.device = torch.device("cpu")


def test_all_rows_mask_is_make_masks():
    for n in (64 * 7, 64 * 7 + 19, 1, 63, 65):
        sh = _cpu_shard(n=n)
        m = sh._all_rows()
        ref = sh.make_mask(torch.ones(n, dtype=torch.bool))
        assert m.visible == n and m.tiles is None and m.n_live is None
        assert torch.equal(m.words, ref.words), n
        assert m.count() == n
        assert sh._all_rows() is m                         # cached by the visible rows
        sh.append_unit(_queries(5, sh.dim))
        m2 = sh._all_rows()
        assert m2 is not m and m2.visible == n + 5
        assert torch.equal(m2.words, sh.make_mask(torch.ones(n + 5, dtype=torch.bool)).words)
    # tombstones do not enter it
    sh = _cpu_shard(n=200)
    sh.delete_rows([3, 70])
    assert sh._all_rows().count() == 200 and sh._live().count() == 198


def test_one_ulp_threshold():
    inf, nan = math.inf, math.nan
    c = torch.tensor([[5.0, 1.0, 3.0, -inf, 2.0],
                      [5.0, -inf, -inf, -inf, 1.0],
                      [nan, 4.0, nan, 0.0, 0.0],
                      [-inf, -inf, -inf, -inf, -inf]])
    t = S.filter_large_k_threshold_ulp(c, 3)
    assert t.dtype == torch.float32 and t.shape == (4,) and not bool(torch.isnan(t).any())
    assert float(t[0]) == float(np.nextafter(np.float32(2.0), np.float32(-inf)))
    assert float(t[1]) == -inf                              # two finite candidates, k = 3
    assert float(t[2]) < 0.0 and float(t[2]) == float(np.nextafter(np.float32(0.0), np.float32(-inf)))
    assert float(t[3]) == -inf
    # strictly below the k-th, and nothing lies between
    assert bool((c[0] > t[0]).sum() == 3)
    # fewer columns than k: -inf for every query
    assert bool((S.filter_large_k_threshold_ulp(c, 6) == -inf).all())
    assert bool((S.filter_large_k_threshold_ulp(torch.full((2, 4), nan), 2) == -inf).all())


def test_cpu_fp8_shard_keeps_the_matmul(monkeypatch):
    D, n, k, nq = 256, 500, 100, 7
    sh = _cpu_shard(D, n)
    q = _queries(nq, D)
    calls = []
    real = S.HbmIndexShard._search_matmul
    monkeypatch.setattr(S.HbmIndexShard, "_search_matmul",
                        lambda self, *a, **kw: (calls.append(kw.get("mask")), real(self, *a, **kw))[1])
    rows = sh.unit_rows()[:n]
    allow = torch.from_numpy(np.random.default_rng(2).random(n) < 0.5)
    s, r = sh.search(q, k)
    sm, rm = sh.search(q, k, allow=allow)
    assert len(calls) == 2 and calls[0] is None and calls[1] is not None
    monkeypatch.undo()
    # what the matmul gives: float(q) . decode(x), exact over the (allowed) rows
    s0, r0 = sh._search_matmul(q, k)
    assert torch.equal(s, s0) and torch.equal(r, r0)
    for (gs, gr), al in (((s, r), torch.ones(n, dtype=torch.bool)), ((sm, rm), allow)):
        ref_s, ref_i = R.filtered_topk_ref(rows, q, k, al)
        assert torch.allclose(gs, ref_s, atol=1e-5)
        assert bool(al[gr.long()].all())
        assert torch.equal(torch.sort(gr.long(), 1).values, torch.sort(ref_i, 1).values)
