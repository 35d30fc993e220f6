"""The non-temporal row stream of the MX-fp4 stream scan at width 384 (index_stream.hip, NT_).

The flag changes the cache policy of the sub-tile loads and nothing else, so the nt form must emit
exactly the default form's candidates -- same counts, same rows, same score bits -- in the thin
and the CU-granular form, with the centroid test on and off, past a skipped row block and behind
a closed gate.  Direct kernel calls through the ops wrapper, on a 1000-row shard.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 384
CAP = 4096
_KERNEL = {}


def _unit(x):
    return torch.nn.functional.normalize(x, dim=-1)


def _near(c, m, e, g):
    return _unit(c + e * torch.randn(m, D, device=DEV, generator=g) / math.sqrt(D))


def _kernel_data():
    """A 1000-row shard (random rows, two runs replaced by a crowd near one direction) and the
    fp4 images of 300 queries: the first 8 of every 32-query set sit near the crowd (threshold
    0.5: the crowd's rows), the rest are random (threshold 0: about half the rows), so every set
    and every wave emits."""
    if _KERNEL:
        return _KERNEL
    from codename_symbiont_amd.index.shard import HbmIndexShard
    from codename_symbiont_amd.ops._ext import hip, stream_handle

    g = torch.Generator(device=DEV).manual_seed(171)
    sh = HbmIndexShard(D, 4096, prune="i8")
    c = _unit(torch.randn(D, device=DEV, generator=g))
    x = _unit(torch.randn(1000, D, device=DEV, generator=g))
    x[16:48] = _near(c, 32, 0.3, g)
    x[900:968] = _near(c, 68, 0.3, g)
    sh.append_f32(x)
    assert sh.visible == 1000 and sh.img_mx4 is not None
    nq = 300
    q = _unit(torch.randn(nq, D, device=DEV, generator=g))
    is_near = (torch.arange(nq, device=DEV) % 32) < 8
    q[is_near] = _near(c, int(is_near.sum()), 0.1, g)
    q4, qs4, _ = sh.mx4_query_image(q.bfloat16())
    torch.cuda.synchronize()
    _KERNEL.update(sh=sh, h=hip(), st=stream_handle(sh.device), q4=q4.clone(), qs4=qs4.clone(),
                   thr4=torch.where(is_near, 0.5, 0.0).float().contiguous())
    return _KERNEL


def _scan(kd, nq, n_valid, rows_per_blk, n_rblk, wide, nt, cent=False, skip=None, gate=None,
          runs=None, fill=None):
    """One launch -> (cs, ci, cnt) after a sync; ``fill``: the buffers start from this value and
    the launch does not clear the counters."""
    from codename_symbiont_amd.ops import kernels as K

    h, sh = kd["h"], kd["sh"]
    cs = torch.full((nq, CAP), -7.0 if fill is None else float(fill), device=DEV)
    ci = torch.full((nq, CAP), -7 if fill is None else int(fill), dtype=torch.int32, device=DEV)
    cnt = torch.full((nq,), 0 if fill is None else int(fill), dtype=torch.int32, device=DEV)
    kw, keep = {}, None
    if cent:
        n_sets = -(-nq // 32)
        keep = (torch.empty(n_sets, D // 2, dtype=torch.uint8, device=DEV),
                torch.empty(n_sets, kd["qs4"].shape[1], dtype=torch.int32, device=DEV),
                torch.empty(n_sets, device=DEV))
        h.mx4_centroids(kd["q4"].data_ptr(), kd["qs4"].data_ptr(), nq, D, keep[0].data_ptr(),
                        keep[1].data_ptr(), keep[2].data_ptr(), kd["st"])
        kw = dict(cent4=keep[0].data_ptr(), centqs=keep[1].data_ptr(), centR=keep[2].data_ptr(),
                  bounds4=sh.mx4_bounds.data_ptr())
    img = sh.img_mx4
    K.index_scan_stream(img.data_ptr(), n_valid, img.shape[0] * 32, rows_per_blk, n_rblk,
                        kd["q4"].data_ptr(), kd["qs4"].data_ptr(), nq, kd["thr4"].data_ptr(),
                        cs.data_ptr(), ci.data_ptr(), cnt.data_ptr(), CAP, 1, kd["st"],
                        skip=0 if skip is None else skip.data_ptr(), dim=D, form=1,
                        gate=0 if gate is None else gate.data_ptr(), gate_want=0,
                        zero_cnt=0 if fill is not None else 1,
                        runs=0 if runs is None else runs.data_ptr(), wide=wide, nt=nt, **kw)
    torch.cuda.synchronize()
    del keep
    return cs, ci, cnt


def _sorted_lists(cs, ci, cnt):
    """Each query's candidates as (rows, score bits) sorted by row (unused slots last)."""
    assert int(cnt.max()) <= CAP, "candidate overflow: the case is mis-sized"
    used = torch.arange(CAP, device=DEV)[None, :] < cnt[:, None]
    rows = torch.where(used, ci.long(), torch.full_like(ci, 1 << 30, dtype=torch.int64))
    rows, order = torch.sort(rows, dim=1)
    bits = torch.gather(cs.view(torch.int32), 1, order)
    return rows, torch.where(rows < (1 << 30), bits, torch.zeros_like(bits))


def _assert_same(a, b, what):
    assert torch.equal(a[2], b[2]), f"{what}: candidate counts differ"
    ra, ba = _sorted_lists(*a)
    rb, bb = _sorted_lists(*b)
    assert torch.equal(ra, rb), f"{what}: candidate rows differ"
    assert torch.equal(ba, bb), f"{what}: candidate scores differ"
    return rb


# (n_valid, rows_per_blk, blocks): a multiple of 4 blocks, not a multiple, fewer than 4
GRIDS = [(1000, 64, 16), (1000, 96, 11), (70, 32, 3)]


@pytest.mark.parametrize("nq", [16, 256, 300])
@pytest.mark.parametrize("cent", [False, True])
@pytest.mark.parametrize("wide", [0, 1])
def test_nt_scan_emits_the_default_forms_candidates(wide, cent, nq):
    kd = _kernel_data()
    for n_valid, rows_per_blk, n_rblk in GRIDS:
        what = f"wide={wide} cent={cent} nq={nq} grid=({n_valid},{rows_per_blk},{n_rblk})"
        ref = _scan(kd, nq, n_valid, rows_per_blk, n_rblk, wide, nt=0, cent=cent)
        got = _scan(kd, nq, n_valid, rows_per_blk, n_rblk, wide, nt=1, cent=cent)
        assert int(ref[2].min()) > 0, f"{what}: a query without candidates tests nothing"
        rows = _assert_same(ref, got, what)
        assert int(rows[rows < (1 << 30)].max()) < n_valid, f"{what}: a row past n_valid"


@pytest.mark.parametrize("wide", [0, 1])
def test_nt_scan_skips_routed_blocks(wide):
    kd = _kernel_data()
    n_valid, rows_per_blk, n_rblk, nq = 1000, 96, 11, 300
    skip = torch.zeros(n_rblk, dtype=torch.int32, device=DEV)
    skip[torch.tensor([1, 4, 5, 10], device=DEV)] = 1
    ref = _scan(kd, nq, n_valid, rows_per_blk, n_rblk, wide, nt=0, skip=skip, cent=True)
    got = _scan(kd, nq, n_valid, rows_per_blk, n_rblk, wide, nt=1, skip=skip, cent=True)
    rows = _assert_same(ref, got, f"wide={wide} skip")
    rows = rows[rows < (1 << 30)]
    assert rows.numel() > 0 and not bool(skip[rows // rows_per_blk].any()), "a skipped block emitted"
    full = _scan(kd, nq, n_valid, rows_per_blk, n_rblk, wide, nt=1, cent=True)
    assert int(full[2].sum()) > int(got[2].sum()), "the skipped blocks hold candidates"


@pytest.mark.parametrize("wide", [0, 1])
def test_nt_scan_behind_a_closed_gate_writes_nothing(wide):
    kd = _kernel_data()
    gate = torch.ones(1, dtype=torch.int32, device=DEV)
    runs = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    cs, ci, cnt = _scan(kd, 300, 1000, 96, 11, wide, nt=1, gate=gate, runs=runs, fill=3)
    assert bool((cnt == 3).all()) and bool((ci == 3).all()) and bool((cs == 3.0).all())
    assert int(runs.item()) == 5
    gate.zero_()
    cs, ci, cnt = _scan(kd, 300, 1000, 96, 11, wide, nt=1, gate=gate, runs=runs)
    assert int(runs.item()) == 6 and int(cnt.min()) > 0


def test_nt_is_refused_by_the_launcher_too():
    """(the wrapper's check is tests/test_scan_nt_cpu.py's; the native launcher has its own)"""
    kd = _kernel_data()
    h, sh = kd["h"], kd["sh"]
    img = sh.img_i8
    q8, sq, _ = sh.prune_query_image(_unit(torch.randn(16, D, device=DEV)).bfloat16())
    cs = torch.empty(16, CAP, device=DEV)
    ci = torch.empty(16, CAP, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(16, dtype=torch.int32, device=DEV)
    thr = torch.full((16,), 1e9, device=DEV)
    with pytest.raises(ValueError, match="index_scan_stream"):
        h.index_scan_stream(img.data_ptr(), 1000, img.shape[0] * 32, 64, 16, q8.data_ptr(), 0, 16,
                            thr.data_ptr(), cs.data_ptr(), ci.data_ptr(), cnt.data_ptr(), CAP, 1,
                            kd["st"], dim=D, form=0, nt=1)
    with pytest.raises(ValueError, match="index_scan_stream"):
        h.index_scan_stream(sh.img_mx4.data_ptr(), 1000, sh.img_mx4.shape[0] * 32, 64, 16,
                            kd["q4"].data_ptr(), kd["qs4"].data_ptr(), 16, kd["thr4"].data_ptr(),
                            cs.data_ptr(), ci.data_ptr(), cnt.data_ptr(), CAP, 1, kd["st"], dim=D,
                            form=1, depth=4, nt=1)
    torch.cuda.synchronize()
