"""What the grouped fp8 route decides on the host, without a GPU: the wrapper's argument checks
(all of them run before the extension is touched), which searches the grouped scan serves, and the
arithmetic of the rule that leaves a chunk to the per-mask loop at 256 queries per block."""
import pytest
import torch

from codename_symbiont_amd.index.shard import HbmIndexShard
from codename_symbiont_amd.ops import kernels as K


def _no_extension(monkeypatch):
    def hip():
        raise AssertionError("the wrapper loaded the extension")
    monkeypatch.setattr(K, "hip", hip)


def test_wrapper_checks_run_before_the_extension(monkeypatch):
    _no_extension(monkeypatch)
    D, n, nq, kmax, n_rblk = 384, 640, 5, 16, 2
    nw = n // 64
    ok = dict(rows_u8=torch.zeros(n, D, dtype=torch.uint8), n_valid=n,
              mask8=torch.zeros(nw, 8, dtype=torch.int64),
              qgroup=torch.zeros(nq, dtype=torch.int32),
              tiles=torch.zeros(nw, dtype=torch.int32), n_live=torch.zeros(1, dtype=torch.int32),
              q_e4m3=torch.zeros(nq, D, dtype=torch.uint8), kmax=kmax, n_rblk=n_rblk,
              cand_s=torch.zeros(nq, n_rblk * 2 * kmax),
              cand_i=torch.zeros(nq, n_rblk * 2 * kmax, dtype=torch.int32))
    # host tensors of the right dtypes and shapes are refused as host tensors, nothing else
    with pytest.raises(ValueError, match="device tensor"):
        K.index_scan_filter_group_fp8(**ok)
    for what, exc, match, kw in (
            ("bf16 rows", ValueError, "e4m3 bytes", dict(rows_u8=torch.zeros(n, D, dtype=torch.bfloat16))),
            ("bf16 queries", ValueError, "e4m3 bytes", dict(q_e4m3=torch.zeros(nq, D, dtype=torch.bfloat16))),
            ("float queries", ValueError, "e4m3 bytes", dict(q_e4m3=torch.zeros(nq, D))),
            ("int32 rows", ValueError, "e4m3 bytes", dict(rows_u8=torch.zeros(n, D, dtype=torch.int32)))):
        with pytest.raises(exc, match=match):
            K.index_scan_filter_group_fp8(**{**ok, **kw})


def _fp8_shard(D=384, n=500):
    sh = HbmIndexShard(D, n + 100, device="cpu", dtype="fp8")
    sh.fill_random(n, seed=1)
    return sh


def _groups(sh, G, nq=12):
    n = sh.visible
    g = torch.Generator().manual_seed(G)
    masks = [torch.rand(n, generator=g) < 0.4 for _ in range(G)]
    return sh.make_mask_groups(masks, [i % G for i in range(nq)]), masks


def test_group_scan_serves():
    sh = _fp8_shard()
    three, one = _groups(sh, 3)[0], _groups(sh, 1)[0]
    assert len(three) == 3 and len(one) == 1
    # a CPU fp8 shard: never
    assert not sh._group_scan_serves(10, three)
    # the same questions as a GPU shard would answer them (the method reads no device memory)
    sh.device = torch.device("cuda")
    try:
        assert sh._group_scan_serves(10, three)
        assert sh._group_scan_serves(16, three) and sh._group_scan_serves(32, three)
        assert not sh._group_scan_serves(40, three)
        assert not sh._group_scan_serves(0, three)
        assert not sh._group_scan_serves(10, one)
        for D in (256, 512, 768, 1024):
            other = _fp8_shard(D, 200)
            other.device = torch.device("cuda")
            assert other._group_scan_serves(32, three), D
            other.device = torch.device("cpu")
        sh.dim = 320                                   # a width no masked fp8 scan is built for
        assert not sh._group_scan_serves(10, three)
        sh.dim = 384
    finally:
        sh.device = torch.device("cpu")


def test_cpu_fp8_shard_grouped_search_loops(monkeypatch):
    """A CPU fp8 shard under MaskGroups: one masked search per mask, and the grouped wrapper is
    never called."""
    def barred(*a, **kw):
        raise AssertionError("a CPU shard took the grouped scan")
    monkeypatch.setattr(K, "index_scan_filter_group_fp8", barred)
    sh = _fp8_shard()
    mg, masks = _groups(sh, 3)
    took = []
    real = HbmIndexShard._search_masked
    monkeypatch.setattr(HbmIndexShard, "_search_masked",
                        lambda self, *a, **kw: (took.append(1), real(self, *a, **kw))[1])
    q = torch.nn.functional.normalize(torch.randn(12, 384, generator=torch.Generator().manual_seed(3)), dim=-1)
    s, r = sh.search(q, 5, allow=mg)
    assert len(took) == 3 and s.shape == (12, 5)
    own = torch.stack(masks)[torch.arange(12) % 3]
    assert bool(torch.gather(own, 1, r.long()).all())


def test_loop_keeps_chunk_at_256_queries_per_block(monkeypatch):
    """On fp8 a query block is 256 queries at every width and kmax, so grouping can add a query
    block only above 256 queries; the tile floor and the disjointness test are the shared ones.
    (No extension: the fp8 branch asks it nothing.)"""
    _no_extension(monkeypatch)
    sh = _fp8_shard()
    T = HbmIndexShard.GROUP_LOOP_MIN_TILES
    keep = lambda nq_of, live, k=10: sh._loop_keeps_chunk({"nq_of": nq_of, "live": live}, k)
    disjoint = lambda g: [T] * g + [g * T]
    # 256 queries or fewer: one block together, one block each -- never the loop
    assert not keep([128, 128], disjoint(2))
    assert not keep([64] * 4, disjoint(4))
    assert not keep([1, 255], disjoint(2), k=32)
    # above 256: two blocks together against one each
    assert keep([129, 128], disjoint(2))
    assert keep([200, 200], disjoint(2), k=32)
    assert keep([128] * 4, disjoint(4))
    assert keep([300, 300], disjoint(2))            # three blocks against two
    assert keep([512, 512], disjoint(2))            # four against two
    assert not keep([257, 255], disjoint(2))        # 512 -> two blocks, the larger group has two
    # five groups, overlapping masks, a small union, no tile counts
    assert not keep([128] * 5, disjoint(5))
    assert not keep([200, 200], [T, T, T])          # the same tiles: union far below the sum
    assert not keep([200, 200], [T // 4, T // 4, T // 2])
    assert not keep([200, 200], None)
    assert not keep([400], [T, T])                  # one group
