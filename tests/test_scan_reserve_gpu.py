"""The CU-granular form of the stream scan (index_stream.hip, PACK) and the CU reserve of the
split-phase pruned search (HbmIndexShard.scan_reserve).

Direct kernel calls: the CU-granular form packs 4 / NW thin workgroups into one four-wave
workgroup, so its candidates must be those of the thin form bit for bit -- on grids whose last
workgroup is partly or wholly empty, with one and two query blocks, skipped row blocks, a closed
gate and every ring depth.  End to end: search_begin / search_end under a reserve return what the
full bf16 scan returns, whatever the tier hint says, and a plain search() ignores the reserve.
All at dim 384 on bf16 shards with pruning on.
"""
import math

import pytest
import torch

from codename_symbiont_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 384
CAP = 4096


def _unit(x):
    return torch.nn.functional.normalize(x, dim=-1)


def _near(c, m, e, g):
    return _unit(c + e * torch.randn(m, D, device=DEV, generator=g) / math.sqrt(D))


# ------------------------------------------------------------------------------ direct calls
_KERNEL = {}


def _kernel_data():
    """One 1000-row shard (random rows, two runs of them replaced by a crowd near one direction)
    and the query images of 300 queries: in every 32-query set the first 8 sit near the crowd's direction and
    the rest are random (every set and wave emits; the near ones from the crowd's sub-tiles)."""
    if _KERNEL:
        return _KERNEL
    from codename_symbiont_amd.index.shard import HbmIndexShard
    from codename_symbiont_amd.ops._ext import hip, stream_handle

    g = torch.Generator(device=DEV).manual_seed(71)
    sh = HbmIndexShard(D, 4096, prune="i8")
    c = _unit(torch.randn(D, device=DEV, generator=g))
    x = _unit(torch.randn(1000, D, device=DEV, generator=g))
    x[16:48] = _near(c, 32, 0.3, g)        # (inside the 70-row grids too)
    x[900:968] = _near(c, 68, 0.3, g)
    sh.append_f32(x)
    assert sh.visible == 1000 and sh.img_mx4 is not None and sh.img_i8 is not None
    nq = 300
    q = _unit(torch.randn(nq, D, device=DEV, generator=g))
    is_near = (torch.arange(nq, device=DEV) % 32) < 8
    q[is_near] = _near(c, int(is_near.sum()), 0.1, g)
    q = q.bfloat16()
    t = torch.where(is_near, 0.5, 0.0).float()   # the crowd's rows / about half the random rows
    q8, sq, _ = sh.prune_query_image(q)
    q4, qs4, _ = sh.mx4_query_image(q)
    torch.cuda.synchronize()
    _KERNEL.update(sh=sh, h=hip(), st=stream_handle(sh.device), q=q, q8=q8.clone(),
                   thr8=(t / sq).contiguous(), q4=q4.clone(), qs4=qs4.clone(), thr4=t.contiguous())
    return _KERNEL


def _centroids(K, nq):
    h, sh = K["h"], K["sh"]
    n_sets = -(-nq // 32)
    c4 = torch.empty(n_sets, D // 2, dtype=torch.uint8, device=DEV)
    cqs = torch.empty(n_sets, K["qs4"].shape[1], dtype=torch.int32, device=DEV)
    cR = torch.empty(n_sets, device=DEV)
    h.mx4_centroids(K["q4"].data_ptr(), K["qs4"].data_ptr(), nq, D, c4.data_ptr(), cqs.data_ptr(),
                    cR.data_ptr(), K["st"])
    return dict(cent4=c4.data_ptr(), centqs=cqs.data_ptr(), centR=cR.data_ptr(),
                bounds4=sh.mx4_bounds.data_ptr()), (c4, cqs, cR)


def _scan(K, form, nq, n_valid, rows_per_blk, n_rblk, wide, depth=0, cent=False, skip=None,
          gate=None, gate_want=0, runs=None, fill=None):
    """One index_scan_stream launch -> (cs, ci, cnt) after a sync; ``fill``: the buffers start
    from this value and the launch does not clear the counters."""
    h, sh = K["h"], K["sh"]
    img = sh.img_mx4 if form else sh.img_i8
    cs = torch.full((nq, CAP), -7.0 if fill is None else float(fill), device=DEV)
    ci = torch.full((nq, CAP), -7 if fill is None else int(fill), dtype=torch.int32, device=DEV)
    cnt = torch.full((nq,), 0 if fill is None else int(fill), dtype=torch.int32, device=DEV)
    kw, keep = _centroids(K, nq) if cent else ({}, None)
    Q, qsc, thr = (K["q4"], K["qs4"].data_ptr(), K["thr4"]) if form else (K["q8"], 0, K["thr8"])
    h.index_scan_stream(img.data_ptr(), n_valid, img.shape[0] * 32, rows_per_blk, n_rblk,
                        Q.data_ptr(), qsc, nq, thr.data_ptr(), cs.data_ptr(), ci.data_ptr(),
                        cnt.data_ptr(), CAP, 1, K["st"], skip=0 if skip is None else skip.data_ptr(),
                        dim=D, form=form, gate=0 if gate is None else gate.data_ptr(),
                        gate_want=gate_want, zero_cnt=0 if fill is not None else 1,
                        runs=0 if runs is None else runs.data_ptr(), wide=wide, depth=depth, **kw)
    torch.cuda.synchronize()
    del keep
    return cs, ci, cnt


def _sorted_lists(cs, ci, cnt):
    """Each query's candidates as a (row, score bits) list sorted by row (unused slots last)."""
    assert int(cnt.max()) <= CAP, "candidate overflow: the case is mis-sized"
    used = torch.arange(CAP, device=DEV)[None, :] < cnt[:, None]
    rows = torch.where(used, ci.long(), torch.full_like(ci, 1 << 30, dtype=torch.int64))
    rows, order = torch.sort(rows, dim=1)
    bits = torch.gather(cs.view(torch.int32), 1, order)
    return rows, torch.where(rows < (1 << 30), bits, torch.zeros_like(bits))


# (n_valid, rows_per_blk, blocks): a multiple of 4 blocks, not a multiple, fewer than 4, and
# four blocks past the rows (a last workgroup whose every group has an empty row block)
GRIDS = [(1000, 64, 16), (1000, 96, 11), (70, 32, 3), (1000, 64, 20)]
# (form, centroid test, depth): MX-fp4 with the centroid test on and off, int8, each depth
FORMS = [(1, False, 0), (1, True, 0), (0, False, 0), (1, True, 4), (1, True, 5), (1, False, 5)]


@pytest.mark.parametrize("nq", [16, 256, 300])
@pytest.mark.parametrize("form,cent,depth", FORMS)
def test_cu_granular_scan_emits_the_thin_forms_candidates(form, cent, depth, nq):
    K = _kernel_data()
    for n_valid, rows_per_blk, n_rblk in GRIDS:
        what = f"form={form} cent={cent} depth={depth} nq={nq} grid=({n_valid},{rows_per_blk},{n_rblk})"
        thin = _scan(K, form, nq, n_valid, rows_per_blk, n_rblk, wide=0, cent=cent)
        wide = _scan(K, form, nq, n_valid, rows_per_blk, n_rblk, wide=1, depth=depth, cent=cent)
        assert torch.equal(thin[2], wide[2]), f"{what}: candidate counts differ"
        assert int(thin[2].min()) > 0, f"{what}: a query without candidates tests nothing"
        rt, bt = _sorted_lists(*thin)
        rw, bw = _sorted_lists(*wide)
        assert torch.equal(rt, rw), f"{what}: candidate rows differ"
        assert torch.equal(bt, bw), f"{what}: candidate scores differ"
        assert int(rt[rt < (1 << 30)].max()) < n_valid, f"{what}: a row past n_valid"


@pytest.mark.parametrize("form", [0, 1])
def test_cu_granular_scan_skips_routed_blocks(form):
    K = _kernel_data()
    n_valid, rows_per_blk, n_rblk, nq = 1000, 96, 11, 300
    skip = torch.zeros(n_rblk, dtype=torch.int32, device=DEV)
    skip[torch.tensor([1, 4, 5, 10], device=DEV)] = 1
    thin = _scan(K, form, nq, n_valid, rows_per_blk, n_rblk, wide=0, skip=skip, cent=bool(form))
    wide = _scan(K, form, nq, n_valid, rows_per_blk, n_rblk, wide=1, skip=skip, cent=bool(form))
    rt, bt = _sorted_lists(*thin)
    rw, bw = _sorted_lists(*wide)
    assert torch.equal(thin[2], wide[2]) and torch.equal(rt, rw) and torch.equal(bt, bw)
    got = rw[rw < (1 << 30)]
    assert got.numel() > 0 and not bool(skip[got // rows_per_blk].any()), "a skipped block emitted"
    full = _scan(K, form, nq, n_valid, rows_per_blk, n_rblk, wide=1, cent=bool(form))
    assert int(full[2].sum()) > int(wide[2].sum()), "the skipped blocks hold candidates"


@pytest.mark.parametrize("form", [0, 1])
def test_cu_granular_scan_behind_a_closed_gate_writes_nothing(form):
    K = _kernel_data()
    gate = torch.ones(1, dtype=torch.int32, device=DEV)
    runs = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    cs, ci, cnt = _scan(K, form, 300, 1000, 96, 11, wide=1, gate=gate, gate_want=0, runs=runs,
                        fill=3)
    assert bool((cnt == 3).all()) and bool((ci == 3).all()) and bool((cs == 3.0).all())
    assert int(runs.item()) == 5
    # ... and the open gate counts one run and emits
    gate.zero_()
    cs, ci, cnt = _scan(K, form, 300, 1000, 96, 11, wide=1, gate=gate, gate_want=0, runs=runs)
    assert int(runs.item()) == 6 and int(cnt.min()) > 0


def test_scan_depth_is_checked():
    K = _kernel_data()
    with pytest.raises(ValueError, match="index_scan_stream"):
        _scan(K, 0, 16, 1000, 64, 16, wide=1, depth=4)       # (the depths are the fp4 form's)
    with pytest.raises(ValueError, match="index_scan_stream"):
        _scan(K, 1, 16, 1000, 64, 16, wide=0, depth=6)


# ------------------------------------------------------------------------------ end to end
def _e2e_shard(n, seed):
    """(shard, reference shard, crowd direction): n - 300 random rows, then a crowd of 300
    near-duplicates (the fresh-row tail); the sampled search's row-count gates lowered on the
    instance; the reference holds the same rows and runs the full bf16 list scan."""
    from codename_symbiont_amd.index.shard import HbmIndexShard

    g = torch.Generator(device=DEV).manual_seed(seed)
    sh = HbmIndexShard(D, n + 1024, prune="i8")
    c = _unit(torch.randn(D, device=DEV, generator=g))
    sh.append_f32(torch.randn(n - 300, D, device=DEV, generator=g))
    sh.append_f32(_near(c, 300, 0.1, g))
    sh.SEED_MIN_ROWS = 0
    sh.PRUNE_MIN_SHIFT = 0
    assert sh.visible == n
    return sh, c, g


def _reference(sh, q, k):
    from codename_symbiont_amd.index.shard import HbmIndexShard

    n = sh.visible
    ref = HbmIndexShard(D, n, prune=None)
    ref.rows[:n].copy_(sh.rows[:n])
    ref.count = ref.visible = n
    ref.scan_mq = False
    return ref.search(q, k)


def _same(s, r, s0, r0, rows, q, what):
    """Ids and scores of the full bf16 scan; an id may differ only where its own exact score
    ties the reference's at that rank."""
    torch.cuda.synchronize()
    err = float((s - s0).abs().max())
    assert err <= 2e-5, f"{what}: scores off by {err:.3g}"
    tie = (R.row_scores_ref(rows, q, r) - s0).abs() <= 2e-5
    bad = (r != r0) & ~tie
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} ids differ from the full bf16 scan"
    srt = torch.sort(r.long(), dim=1).values
    assert not bool((srt[:, 1:] == srt[:, :-1]).any()), f"{what}: a row returned twice"


@pytest.mark.parametrize("n", [20_000, 70_000])
@pytest.mark.parametrize("reserve", [0, 64, -1])
def test_reserved_search_matches_the_full_bf16_scan(n, reserve):
    k, nq = 10, 256
    sh, c, g = _e2e_shard(n, seed=n)
    n_cus = sh._n_cus()
    sh.scan_reserve = n_cus - 1 if reserve < 0 else reserve
    rows = sh.unit_rows().float()
    qs = {"near": _near(c, nq, 0.1, g).bfloat16(),
          "heldout": _unit(torch.randn(nq, D, device=DEV, generator=g)).bfloat16()}
    refs = {kind: _reference(sh, q, k) for kind, q in qs.items()}
    blocks_all = sh._i8_geometry(n, nq, n_cus)[2]
    assert blocks_all == math.ceil(n / 8192)

    def split_search(kind, hint_mx4):
        """search_begin / search_end of ``kind`` queries; the hint was left by the search
        before (its tier flag has landed: every search here ends in a sync)."""
        ctx = sh.search_begin(qs[kind], k)
        assert "full" not in ctx, "the pruned search did not take this shard"
        assert ctx["hint_mx4"] == hint_mx4, (kind, ctx["hint_mx4"])
        assert ctx["wide"] == (hint_mx4 and sh.scan_reserve > 0)
        want = sh._i8_geometry(n, nq, n_cus, sh.scan_reserve if ctx["wide"] else 0)
        assert ctx["geo"] == want and want[2] <= blocks_all
        s, r = sh.search_end(ctx)
        what = f"n={n} reserve={sh.scan_reserve} {kind} hint_mx4={hint_mx4}"
        _same(s, r, *refs[kind], rows, qs[kind], what)
        # (the tier flag: 0 = the fp4 tier ran, 1 = the int8 tier)
        assert (int(sh._mx4_last.item()) == 0) == (kind == "near"), what

    split_search("near", False)      # a wrong hint: the fp4 tier runs in the thin form
    split_search("near", True)       # the case the reserve is for
    split_search("heldout", True)    # a wrong hint: the int8 tier on the reserve's grid
    split_search("heldout", False)
    split_search("near", False)
    # a plain search() keeps every CU whatever the hint and the reserve
    sh.mq_stats = True
    for kind in ("near", "heldout"):
        s, r = sh.search(qs[kind], k)
        _same(s, r, *refs[kind], rows, qs[kind], f"n={n} reserve={sh.scan_reserve} plain {kind}")
        assert sh._pruned_last["n_rblk"] == blocks_all
    sh.mq_stats = False


@pytest.mark.parametrize("reserve", [0, 64, -1])
def test_reserved_search_with_an_append_into_the_partial_subtile(reserve):
    """Rows appended between the halves land in the partly filled 32-row sub-tile (and raise its
    shared int8 scale); the search still returns the full bf16 scan of the rows begin saw."""
    n0, k, nq = 20_000, 10, 256
    sh, c, g = _e2e_shard(n0, seed=5)
    sh.append_unit(_near(c, 11, 0.1, g).bfloat16())
    n = sh.visible
    assert n == n0 + 11 and n % 32 != 0
    sh.scan_reserve = sh._n_cus() - 1 if reserve < 0 else reserve
    rows = sh.unit_rows().float()[:n]
    q = torch.cat([sh.rows[n - 11:n].clone(), _near(c, nq - 11, 0.1, g).bfloat16()])
    s0, r0 = _reference(sh, q, k)
    sh.search(q, k)                   # leaves the fp4 hint
    torch.cuda.synchronize()
    spike = torch.zeros(13, D, device=DEV)
    spike[torch.arange(13), torch.arange(13) * 5] = 1.0
    spike = _unit(spike + 0.01 * torch.randn(13, D, device=DEV, generator=g)).bfloat16()
    ctx = sh.search_begin(q, k)
    assert "full" not in ctx and ctx["n"] == n and ctx["hint_mx4"]
    assert ctx["wide"] == (sh.scan_reserve > 0)
    sh.append_unit(spike)             # rewrites sub-tile n >> 5 in place
    s, r = sh.search_end(ctx)
    _same(s, r, s0, r0, rows, q, f"append between the halves, reserve={sh.scan_reserve}")
    assert int(sh._mx4_last.item()) == 0
    assert bool((r[:11, 0] == torch.arange(n - 11, n, device=DEV, dtype=torch.int32)).all())
