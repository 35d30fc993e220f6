"""The block grid of the stream scans under a CU reserve (HbmIndexShard._i8_geometry,
_scan_reserve): host arithmetic only, no GPU."""
import math

import pytest

from codename_symbiont_amd.index.shard import HbmIndexShard

NS = [1, 70, 8191, 8192, 20_000, 70_000, 1_000_003, 25_000_000, 100_000_000]
NQS = [16, 255, 256, 257, 512, 2048]
CUS = [8, 64, 255, 256, 304]


def _shard(dim=384):
    sh = HbmIndexShard(dim, 4096, device="cpu", prune="i8")
    assert sh.stream and sh.mx4_on and sh.img_mx4 is not None
    return sh


@pytest.mark.parametrize("n_cus", CUS)
def test_reserved_grid_covers_the_rows_within_the_limits(n_cus):
    sh = _shard()
    for n in NS:
        for nq in NQS:
            full = sh._i8_geometry(n, nq, n_cus)
            prev = None
            for R in sorted({0, 1, 16, 32, 64, 96, 128, n_cus // 2, n_cus - 1} & set(range(n_cus))):
                rsplit, rows_per_blk, n_rblk = sh._i8_geometry(n, nq, n_cus, R)
                what = (n, nq, n_cus, R)
                assert rows_per_blk % 128 == 0 and rows_per_blk > 0, what
                assert n_rblk * rows_per_blk >= n > (n_rblk - 1) * rows_per_blk, what
                assert 1 <= n_rblk <= 1024, what
                assert n_rblk <= math.ceil(n / 8192), what     # (>= ~8192 rows per block)
                assert rsplit == full[0], what
                if R == 0:
                    assert (rsplit, rows_per_blk, n_rblk) == full, what
                else:
                    # the fp4 form: 4 one-wave blocks per workgroup, one workgroup per CU --
                    # the workgroups fit the CUs outside the reserve (one block of slack: the
                    # grid is rounded to whole 128-row tiles and to the nearest block count)
                    n_qblk = math.ceil(nq / 256)
                    wgs = math.ceil(n_rblk * n_qblk / 4)
                    assert wgs <= max(1, n_cus - R) + 1, what
                    assert n_rblk <= prev, what          # a larger reserve never adds blocks
                prev = n_rblk


def test_headline_grid():
    sh = _shard()
    assert sh._i8_geometry(100_000_000, 256, 256) == (2, 97664, 1024)
    for R, blocks in ((16, 960), (32, 896), (64, 768), (96, 640), (128, 512)):
        _, rows_per_blk, n_rblk = sh._i8_geometry(100_000_000, 256, 256, R)
        assert abs(n_rblk - blocks) <= 1 and math.ceil(n_rblk / 4) <= 256 - R, (R, n_rblk)


def test_reserve_applies_only_to_the_split_phase_fp4_case():
    sh = _shard()
    sh.scan_reserve = 64
    sh._tier_mx4 = True
    assert sh._scan_reserve(True, 256, 256) == 64
    assert sh._scan_reserve(True, 32, 256) == 31            # (at least one CU scans)
    assert sh._scan_reserve(False, 256, 256) == 0           # a plain search()
    assert sh._scan_reserve(True, 256, sh.tail_dense_max_nq + 1) == 0   # (no fp4 tier enqueued)
    sh._tier_mx4 = False
    assert sh._scan_reserve(True, 256, 256) == 0            # the hint says int8
    sh._tier_mx4 = True
    sh.scan_reserve = 0
    assert sh._scan_reserve(True, 256, 256) == 0
    sh.scan_reserve = 64
    sh.prune_route = False
    assert sh._scan_reserve(True, 256, 256) == 0
    sh.prune_route = True
    sh._i8_heavy = 64                                        # the split image: the LDS-ring scan
    assert sh._scan_reserve(True, 256, 256) == 0
    # the LDS-ring int8 tier (768) and shards without the fp4 stream image keep every CU
    ring = _shard(768)
    ring.scan_reserve, ring._tier_mx4 = 64, True
    assert ring.i8_ring and ring._scan_reserve(True, 256, 256) == 0


def test_begin_passes_the_reserve_only_when_it_left_the_cus_to_the_shard(monkeypatch):
    """search_begin(n_cus=None) is the split-phase case; an explicit n_cus, like a plain
    search(), is not (checked on the arguments _pruned_begin hands to _scan_reserve)."""
    sh = _shard()
    seen = []

    class Stop(Exception):
        pass

    def spy(split, n_cus, NQ):
        seen.append(split)
        raise Stop

    monkeypatch.setattr(sh, "_scan_reserve", spy)
    monkeypatch.setattr(sh, "_tile_sample_plan", lambda *a, **kw: (5, 64, 4096, None))
    monkeypatch.setattr(sh, "_n_cus", lambda: 256)
    import torch

    q = torch.zeros(16, 384, dtype=torch.bfloat16)
    for kw, want in ((dict(split=True, n_cus=None), True), (dict(split=True, n_cus=128), False),
                     (dict(split=False, n_cus=None), False)):
        with pytest.raises(Stop):
            sh._pruned_begin(q, 10, kw["n_cus"], split=kw["split"])
        assert seen.pop() is want
