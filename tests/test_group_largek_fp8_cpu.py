"""What the grouped large-k fp8 route decides on the host, without a GPU: the new wrapper's
argument checks (all of them run before the extension is touched), the truth table of
_group_large_k_serves, the chunking of 9 and 17 masks, and that CPU shards at k = 40 under
MaskGroups still answer through the per-mask loop with unchanged results."""
import pytest
import torch

from codename_symbiont_amd.index.shard import HbmIndexShard, MaskGroups
from codename_symbiont_amd.ops import kernels as K


def _no_extension(monkeypatch):
    def hip():
        raise AssertionError("the wrapper loaded the extension")
    monkeypatch.setattr(K, "hip", hip)


def test_wrapper_checks_run_before_the_extension(monkeypatch):
    _no_extension(monkeypatch)
    D, n, nq, cap = 384, 640, 5, 64
    nw = n // 64
    ok = dict(rows_u8=torch.zeros(n, D, dtype=torch.uint8), n_valid=n,
              mask8=torch.zeros(nw, 8, dtype=torch.int64),
              qgroup=torch.zeros(nq, dtype=torch.int32),
              tiles=torch.zeros(nw, dtype=torch.int32), n_live=torch.zeros(1, dtype=torch.int32),
              q_e4m3=torch.zeros(nq, D, dtype=torch.uint8), thr=torch.zeros(nq),
              cand_s=torch.zeros(nq, cap), cand_i=torch.zeros(nq, cap, dtype=torch.int32),
              cand_n=torch.zeros(nq, dtype=torch.int32), cap=cap, n_rblk=2)
    # host tensors of the right dtypes and shapes are refused as host tensors, nothing else
    with pytest.raises(ValueError, match="device tensor"):
        K.index_scan_emit_group_fp8(**ok)
    for what, match, kw in (
            ("bf16 rows", "e4m3 bytes", dict(rows_u8=torch.zeros(n, D, dtype=torch.bfloat16))),
            ("bf16 queries", "e4m3 bytes", dict(q_e4m3=torch.zeros(nq, D, dtype=torch.bfloat16))),
            ("float queries", "e4m3 bytes", dict(q_e4m3=torch.zeros(nq, D))),
            ("int32 rows", "e4m3 bytes", dict(rows_u8=torch.zeros(n, D, dtype=torch.int32)))):
        with pytest.raises(ValueError, match=match):
            K.index_scan_emit_group_fp8(**{**ok, **kw})


def test_wrapper_refusals_in_order(monkeypatch):
    """Every later refusal, reached on host tensors by letting the device check pass: none of
    them asks the extension for anything."""
    _no_extension(monkeypatch)
    real = K._chk

    def chk(t, dtype, name, ndim=None):          # _chk without "must be a device tensor"
        if t.dtype != dtype:
            raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: must be contiguous")
        if ndim is not None and t.dim() != ndim:
            raise ValueError(f"{name}: expected {ndim}-d, got {tuple(t.shape)}")

    assert callable(real)
    monkeypatch.setattr(K, "_chk", chk)
    D, n, nq, cap = 384, 640, 5, 64
    nw = n // 64
    ok = dict(rows_u8=torch.zeros(n, D, dtype=torch.uint8), n_valid=n,
              mask8=torch.zeros(nw, 8, dtype=torch.int64),
              qgroup=torch.zeros(nq, dtype=torch.int32),
              tiles=torch.zeros(nw, dtype=torch.int32), n_live=torch.zeros(1, dtype=torch.int32),
              q_e4m3=torch.zeros(nq, D, dtype=torch.uint8), thr=torch.zeros(nq),
              cand_s=torch.zeros(nq, cap), cand_i=torch.zeros(nq, cap, dtype=torch.int32),
              cand_n=torch.zeros(nq, dtype=torch.int32), cap=cap, n_rblk=2)
    # with every check passed the wrapper goes on to the extension
    with pytest.raises(AssertionError, match="loaded the extension"):
        K.index_scan_emit_group_fp8(**ok)
    for what, exc, match, kw in (
            ("width", ValueError, "wide", dict(rows_u8=torch.zeros(n, 320, dtype=torch.uint8),
                                              q_e4m3=torch.zeros(nq, 320, dtype=torch.uint8))),
            ("query width", ValueError, "wide", dict(q_e4m3=torch.zeros(nq, 256, dtype=torch.uint8))),
            ("int32 mask8", TypeError, "mask8", dict(mask8=torch.zeros(nw, 8, dtype=torch.int32))),
            ("1-d mask8", ValueError, "mask8", dict(mask8=torch.zeros(nw, dtype=torch.int64))),
            ("four slots", ValueError, "mask8 must be contiguous",
             dict(mask8=torch.zeros(nw, 4, dtype=torch.int64))),
            ("transposed mask8", ValueError, "mask8",
             dict(mask8=torch.zeros(8, nw, dtype=torch.int64).t())),
            ("short mask8", ValueError, "shorter than",
             dict(mask8=torch.zeros(nw - 1, 8, dtype=torch.int64))),
            ("int64 qgroup", TypeError, "qgroup", dict(qgroup=torch.zeros(nq, dtype=torch.int64))),
            ("short qgroup", ValueError, "one group per query",
             dict(qgroup=torch.zeros(nq - 1, dtype=torch.int32))),
            ("long qgroup", ValueError, "one group per query",
             dict(qgroup=torch.zeros(nq + 1, dtype=torch.int32))),
            ("short slab", ValueError, "shorter than",
             dict(rows_u8=torch.zeros(n - 1, D, dtype=torch.uint8))),
            ("short tile list", ValueError, "shorter than",
             dict(tiles=torch.zeros(nw - 1, dtype=torch.int32))),
            ("thr f64", ValueError, "float32", dict(thr=torch.zeros(nq, dtype=torch.float64))),
            ("thr missing", ValueError, "float32", dict(thr=None)),
            ("short thr", ValueError, "one threshold per query", dict(thr=torch.zeros(nq - 1))),
            ("long thr", ValueError, "one threshold per query", dict(thr=torch.zeros(nq + 1))),
            ("short cand_n", ValueError, "cand_n",
             dict(cand_n=torch.zeros(nq - 1, dtype=torch.int32))),
            ("workspace", ValueError, "workspace", dict(cand_s=torch.zeros(nq * cap - 1))),
            ("workspace ids", ValueError, "workspace",
             dict(cand_i=torch.zeros(nq * cap - 1, dtype=torch.int32))),
            ("cap", ValueError, "cap >= 1", dict(cap=0)),
            ("n_rblk", ValueError, "n_rblk >= 1", dict(n_rblk=0)),
            ("n_valid", ValueError, "n_valid >= 0", dict(n_valid=-1)),
            ("no n_live", ValueError, "n_rblk >= 1", dict(n_live=torch.zeros(0, dtype=torch.int32))),
            ("int64 gate", TypeError, "gate", dict(gate=torch.zeros(1, dtype=torch.int64))),
            ("2-d gate", ValueError, "gate", dict(gate=torch.zeros(1, 1, dtype=torch.int32))),
            ("empty gate", ValueError, "one int32 flag", dict(gate=torch.zeros(0, dtype=torch.int32)))):
        with pytest.raises(exc, match=match):
            K.index_scan_emit_group_fp8(**{**ok, **kw})


def _shard(dtype="fp8", D=384, n=500):
    sh = HbmIndexShard(D, n + 100, device="cpu", dtype=dtype)
    sh.fill_random(n, seed=1)
    return sh


def _groups(sh, G, nq=12):
    n = sh.visible
    g = torch.Generator().manual_seed(G)
    masks = [torch.rand(n, generator=g) < 0.4 for _ in range(G)]
    return sh.make_mask_groups(masks, [i % G for i in range(nq)]), masks


def test_group_large_k_serves_truth_table():
    sh = _shard()
    three, one = _groups(sh, 3)[0], _groups(sh, 1)[0]
    assert len(three) == 3 and len(one) == 1
    sh.FP8_LARGE_K_MIN_ROWS = 0
    # a CPU fp8 shard: never
    assert not sh._group_large_k_serves(100, three)
    # the same questions as a GPU shard would answer them (the method reads no device memory)
    sh.device = torch.device("cuda")
    try:
        assert [sh._group_large_k_serves(k, three) for k in (32, 33, 100, 128, 129)] == \
            [False, True, True, True, False]
        assert not sh._group_large_k_serves(0, three)
        assert not sh._group_large_k_serves(100, one)               # one group: _search_masked
        # rows either side of the gate
        sh.FP8_LARGE_K_MIN_ROWS = sh.visible
        assert sh._group_large_k_serves(100, three)
        sh.FP8_LARGE_K_MIN_ROWS = sh.visible + 1
        assert not sh._group_large_k_serves(100, three)
        del sh.FP8_LARGE_K_MIN_ROWS                                 # the class default: 2^20 rows
        assert HbmIndexShard.FP8_LARGE_K_MIN_ROWS == 1 << 20
        assert not sh._group_large_k_serves(100, three)
        sh.FP8_LARGE_K_MIN_ROWS = 0
        for D in (256, 512, 768, 1024):
            other = _shard("fp8", D, 200)
            other.FP8_LARGE_K_MIN_ROWS = 0
            assert not other._group_large_k_serves(100, three)      # on the CPU
            other.device = torch.device("cuda")
            assert other._group_large_k_serves(100, three), D
            other.device = torch.device("cpu")
        sh.dim = 320                                   # a width no masked fp8 scan is built for
        assert not sh._group_large_k_serves(100, three)
        sh.dim = 384
        sh.dtype = "bf16"                              # bf16 shards: out of this route
        assert not sh._group_large_k_serves(100, three)
        sh.dtype = "fp8"
        assert sh._group_large_k_serves(100, three)
        # the list-scan rule is untouched: it serves k <= 32 and nothing above
        assert sh._group_scan_serves(32, three) and not sh._group_scan_serves(33, three)
    finally:
        sh.device = torch.device("cpu")


def test_loop_keeps_chunk_above_k_32(monkeypatch):
    """The rule that leaves a chunk to the per-mask loop (two to four large disjoint masks whose
    queries need one more query block together) holds at k > 32 too, except at the width where
    the grouped emitting scan was measured ahead in exactly that case (384); at k <= 32 nothing
    changes.  (No extension: the fp8 branch asks it nothing.)"""
    _no_extension(monkeypatch)
    T = HbmIndexShard.GROUP_LOOP_MIN_TILES
    assert HbmIndexShard.GROUP_LOOP_LARGE_K_SCAN_DIMS == (384,)
    disjoint = lambda g: [T] * g + [g * T]
    for D in (256, 384, 512, 768, 1024):
        sh = _shard("fp8", D, 200)
        keep = lambda nq_of, live, k: sh._loop_keeps_chunk({"nq_of": nq_of, "live": live}, k)
        for k in (10, 32):
            assert keep([200, 200], disjoint(2), k) and keep([128] * 4, disjoint(4), k), (D, k)
        for k in (33, 100, 128):
            assert keep([200, 200], disjoint(2), k) == (D != 384), (D, k)
            assert keep([128] * 4, disjoint(4), k) == (D != 384), (D, k)
            # what never kept the loop still does not
            assert not keep([128, 128], disjoint(2), k)             # one query block together
            assert not keep([128] * 5, disjoint(5), k)              # five groups
            assert not keep([200, 200], [T, T, T], k)               # the same tiles
            assert not keep([200, 200], None, k)


@pytest.mark.parametrize("dtype", ["fp8", "bf16"])
def test_cpu_shards_at_k_40_still_loop(dtype, monkeypatch):
    """A CPU shard under MaskGroups at k = 40: one masked search per mask, neither grouped wrapper
    is called, and the results are those of each group's single-mask search."""
    def barred(*a, **kw):
        raise AssertionError("a CPU shard took a grouped scan")
    monkeypatch.setattr(K, "index_scan_filter_group_fp8", barred)
    monkeypatch.setattr(K, "index_scan_emit_group_fp8", barred)
    monkeypatch.setattr(HbmIndexShard, "_search_group_chunk_large_k", barred)
    sh = _shard(dtype)
    sh.FP8_LARGE_K_MIN_ROWS = 0
    mg, masks = _groups(sh, 3)
    took = []
    real = HbmIndexShard._search_masked
    monkeypatch.setattr(HbmIndexShard, "_search_masked",
                        lambda self, *a, **kw: (took.append(1), real(self, *a, **kw))[1])
    q = torch.nn.functional.normalize(
        torch.randn(12, 384, generator=torch.Generator().manual_seed(3)), dim=-1)
    s, r = sh.search(q, 40, allow=mg)
    assert len(took) == 3 and s.shape == (12, 40)
    own = torch.stack(masks)[torch.arange(12) % 3]
    assert bool(torch.gather(own, 1, r.long()).all())
    for g in range(3):
        idx = [i for i in range(12) if i % 3 == g]
        sg, rg = sh.search(q[idx], 40, allow=masks[g])
        assert torch.equal(s[idx], sg) and torch.equal(r[idx].long(), rg.long())


@pytest.mark.parametrize("G,sizes", [(9, [8, 1]), (17, [8, 8, 1]), (8, [8]), (16, [8, 8])])
def test_chunking_arithmetic(G, sizes, monkeypatch):
    """Masks go to the scans in chunks of up to eight: (first group, groups) per chunk, every
    query in exactly one chunk with its group renumbered inside it.  (Host-only: filter_tiles is
    stubbed, a CPU shard's masks carry no tile list.)"""
    monkeypatch.setattr(K, "filter_tiles", lambda words, n: (None, None))
    sh = _shard()
    nq = 40
    mg, _ = _groups(sh, G, nq)
    assert isinstance(mg, MaskGroups) and len(mg) == G and mg.n_chunks == len(sizes)
    seen = []
    for c, size in enumerate(sizes):
        ch = mg.chunk(c)
        assert ch["groups"] == (8 * c, size)
        assert ch["mask8"].shape == (mg.masks[0].words.numel(), 8)
        assert bool((ch["mask8"][:, size:] == 0).all())
        idx, qg = ch["idx"].tolist(), ch["qgroup"].tolist()
        assert idx == sorted(idx) and len(idx) == len(qg) == sum(ch["nq_of"])
        assert all(mg.group_of[i] == 8 * c + g for i, g in zip(idx, qg))
        assert ch["nq_of"] == [mg.group_of.count(8 * c + j) for j in range(size)]
        assert ch["live"] is None
        seen += idx
    assert sorted(seen) == list(range(nq))
