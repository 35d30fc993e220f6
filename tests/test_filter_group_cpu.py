"""A mask per query on CPU shards: ``HbmIndexShard.make_mask_groups`` / ``search(allow=MaskGroups)``
(the per-group loop over the existing exact routes), ``VectorStore.search(filter=[...])`` against
one search per request, ``SearchBatcher`` carrying filters, and the fp32 oracle
``ops.reference.grouped_filtered_topk_ref`` against a brute-force loop."""
from __future__ import annotations

import asyncio
import math

import numpy as np
import pytest
import torch

from codename_symbiont_amd.index.filter import Filter
from codename_symbiont_amd.index.shard import HbmIndexShard, MaskGroups, Payload
from codename_symbiont_amd.index.store import VectorStore
from codename_symbiont_amd.ops import reference as R

D = 32
N = 64 * 9 + 21


def _shard(n=N, dim=D, dtype="bf16", seed=3):
    sh = HbmIndexShard(dim, n + 200, device="cpu", dtype=dtype)
    g = torch.Generator().manual_seed(seed)
    sh.append_f32(torch.randn(n, dim, generator=g))
    return sh


def _queries(nq=11, dim=D, seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(nq, dim, generator=g), dim=-1).bfloat16()


def _allow(n, share, seed):
    return torch.from_numpy(np.random.default_rng(seed).random(n) < share)


# ---- oracle ---------------------------------------------------------------------------------------
def test_oracle_equals_brute_force_loop():
    g = torch.Generator().manual_seed(1)
    rows = torch.nn.functional.normalize(torch.randn(300, D, generator=g), dim=-1).bfloat16()
    q = _queries(13)
    allows = [_allow(300, 0.5, 2), _allow(300, 0.02, 3), torch.zeros(300, dtype=torch.bool),
              torch.ones(300, dtype=torch.bool)]
    group_of = [i % 4 for i in range(13)]
    k = 8
    s, r = R.grouped_filtered_topk_ref(rows, q, k, allows, group_of)
    assert s.shape == (13, k) and r.shape == (13, k)
    sc = q.float() @ rows.float().t()
    for i in range(13):
        a = allows[group_of[i]]
        best = sorted(((float(sc[i, j]), j) for j in range(300) if a[j]), reverse=True)[:k]
        m = len(best)
        assert torch.equal(torch.isfinite(s[i]), torch.arange(k) < m)
        assert [int(x) for x in r[i, :m]] == [j for _, j in best]
        assert torch.allclose(s[i, :m], torch.tensor([v for v, _ in best]), atol=1e-6)
        assert bool((r[i, m:] == -1).all()) and bool((s[i, m:] == -math.inf).all())
    # a [G, n] tensor is taken like the list; one group is filtered_topk_ref
    s2, r2 = R.grouped_filtered_topk_ref(rows, q, k, torch.stack(allows), torch.tensor(group_of))
    assert torch.equal(s, s2) and torch.equal(r, r2)
    s1, r1 = R.grouped_filtered_topk_ref(rows, q, k, [allows[0]], [0] * 13)
    f1, g1 = R.filtered_topk_ref(rows, q, k, allows[0])
    assert torch.equal(s1, f1) and torch.equal(r1, g1)
    with pytest.raises(ValueError):
        R.grouped_filtered_topk_ref(rows, q, k, allows, group_of[:-1])
    with pytest.raises(IndexError):
        R.grouped_filtered_topk_ref(rows, q, k, allows, [4] * 13)


# ---- make_mask_groups ------------------------------------------------------------------------------
def test_make_mask_groups_merges_same_object_and_equal_masks():
    sh = _shard()
    a, b = _allow(N, 0.5, 4), _allow(N, 0.1, 5)
    ma, mb = sh.make_mask(a), sh.make_mask(b)
    ma2 = sh.make_mask(a.clone())                       # an equal RowMask, another object
    rows_b = torch.nonzero(b).flatten().tolist()        # the same rows, another input form
    mg = sh.make_mask_groups([ma, mb, ma, ma2, rows_b], [0, 1, 2, 3, 4, 1, 0])
    assert isinstance(mg, MaskGroups) and len(mg) == 2
    assert mg.masks[0] is ma and mg.masks[1] is mb
    assert mg.group_of == [0, 1, 0, 0, 1, 1, 0]
    assert mg.visible == N and mg.dead_gen == sh.dead_gen
    # masks no query names are dropped; group_of may be a tensor
    mg = sh.make_mask_groups([ma, mb], torch.tensor([1, 1, 1]))
    assert len(mg) == 1 and mg.masks[0] is mb and mg.group_of == [0, 0, 0]


def test_make_mask_groups_refusals():
    sh = _shard()
    a = _allow(N, 0.5, 4)
    ma = sh.make_mask(a)
    with pytest.raises(ValueError):
        sh.make_mask_groups([], [])
    with pytest.raises(IndexError):
        sh.make_mask_groups([ma], [0, 1])
    with pytest.raises(IndexError):
        sh.make_mask_groups([ma], [-1])
    # a mask of another number of visible rows
    sh.append_f32(torch.randn(70, D))
    with pytest.raises(ValueError, match="visible"):
        sh.make_mask_groups([ma, sh.make_mask(_allow(N + 70, 0.5, 6))], [0, 1])
    # a mask from before a delete, at build time and at search time
    mb = sh.make_mask(_allow(N + 70, 0.3, 7))
    mc = sh.make_mask(_allow(N + 70, 0.3, 8))
    mg = sh.make_mask_groups([mb, mc], [0, 1, 0])
    q = _queries(3)
    sh.search(q, 5, allow=mg)
    sh.delete_rows([3, 4])
    with pytest.raises(ValueError, match="before a delete"):
        sh.make_mask_groups([mb, mc], [0, 1, 0])
    with pytest.raises(ValueError, match="before a delete"):
        sh.search(q, 5, allow=mg)
    # the number of queries must be the one the groups were made for
    mg = sh.make_mask_groups([_allow(N + 70, 0.3, 7), _allow(N + 70, 0.3, 8)], [0, 1, 0])
    with pytest.raises(ValueError, match="queries"):
        sh.search(_queries(4), 5, allow=mg)


@pytest.mark.parametrize("dtype,k", [("bf16", 10), ("bf16", 40), ("fp8", 10)])
def test_grouped_search_is_the_per_group_searches(dtype, k):
    dim = D if dtype == "bf16" else 256                 # (fp8 rows: 256 wide at the least)
    sh = _shard(dim=dim, dtype=dtype)
    nq = 23
    q = _queries(nq, dim)
    allows = [_allow(N, 0.5, 11), _allow(N, 0.5, 12), torch.zeros(N, dtype=torch.bool),
              torch.ones(N, dtype=torch.bool), _allow(N, 0.01, 13)]
    group_of = [(i * 3) % 5 for i in range(nq)]         # interleaved, never sorted
    mg = sh.make_mask_groups(allows, group_of)
    s, r = sh.search(q, k, allow=mg)
    assert s.shape == (nq, k) and r.shape == (nq, k)
    assert s.dtype == torch.float32 and r.dtype == torch.int32
    for g, a in enumerate(allows):
        idx = [i for i in range(nq) if group_of[i] == g]
        sg, rg = sh.search(q[idx], k, allow=a)
        assert torch.equal(s[idx], sg) and torch.equal(r[idx].long(), rg.long()), g
    # search_begin / search_end take the groups too
    s2, r2 = sh.search_end(sh.search_begin(q, k, allow=mg))
    assert torch.equal(s, s2) and torch.equal(r, r2)
    if dtype == "bf16":
        ref_s, ref_i = R.grouped_filtered_topk_ref(sh.unit_rows()[:N], q, k, allows, group_of)
        assert torch.equal(torch.isfinite(s), torch.isfinite(ref_s))
        fin = torch.isfinite(ref_s)
        assert torch.allclose(s[fin], ref_s[fin], atol=2e-3)
        assert bool((r[~fin] == -1).all())
    # tombstones: a mask made after the delete allows no dead row
    dead = torch.nonzero(allows[0]).flatten()[:50].tolist()
    sh.delete_rows(dead)
    mg = sh.make_mask_groups(allows, group_of)
    s, r = sh.search(q, k, allow=mg)
    assert not bool(torch.isin(r.long(), torch.tensor(dead)).any())


# ---- VectorStore -----------------------------------------------------------------------------------
DOCS = ("doc-a", "doc-b", "doc-c", "doc-d")
SD = 16


def _store(dtype="bf16", n_points=120, dim=SD):
    st = VectorStore(dim, 512, device="cpu", dtype=dtype)
    rng = np.random.default_rng(21)
    ids = [f"p{i}" for i in range(n_points)]
    pls = [Payload(DOCS[i % 4], f"http://{i % 2}.example", f"s{i}", i,
                   "m0" if i < n_points // 2 else "m1", 0) for i in range(n_points)]
    st.upsert(ids, rng.standard_normal((n_points, dim)).astype(np.float32), pls)
    return st


# A CPU search is an fp32 matmul, whose summation order depends on the batch: one request's scores
# move by rounding when it is searched with others.  |q . x| sums D <= 256 products of unit
# vectors' components, so two orders differ by at most D * 2^-24 * sum|q_i x_i| <= 256 * 6e-8.
ATOL = 2e-5


def _same(s, r, s1, r1, what=""):
    """Scores equal to ATOL with the same (-inf, -1) tail; rows equal outside runs of scores
    closer than 2 ATOL (where rounding may order them either way)."""
    s, r, s1, r1 = (np.asarray(x).reshape(-1) for x in (s, r, s1, r1))
    fin = np.isfinite(s1)
    assert np.array_equal(np.isfinite(s), fin), what
    assert (r[~fin] == -1).all() and (r1[~fin] == -1).all(), what
    assert np.allclose(s[fin], s1[fin], rtol=0, atol=ATOL), what
    near = np.zeros(s.shape, bool)
    d = np.abs(np.diff(np.where(fin, s1, 0.0))) < 2 * ATOL
    near[1:] |= d
    near[:-1] |= d
    assert (r == r1)[fin & ~near].all(), what


def _filters():
    return [Filter(must={"original_document_id": "doc-a"}),
            None,
            Filter(must_not={"original_document_id": "doc-b"}),
            Filter(point_ids=["p3", "p5", "p8", "p13"]),
            Filter(must={"original_document_id": "doc-a"}),       # equal to entry 0
            Filter(must={"model_name": "m1"}, must_not={"original_document_id": ["doc-c", "doc-d"]}),
            None,
            Filter(must={"original_document_id": "no such document"}),
            Filter(must_not={"original_document_id": "doc-b"})]


@pytest.mark.parametrize("dtype,k", [("bf16", 10), ("fp8", 10), ("bf16", 40)])
def test_store_filter_list_equals_one_search_per_request(dtype, k):
    dim = SD if dtype == "bf16" else 256                # (fp8 rows: 256 wide at the least)
    st = _store(dtype, dim=dim)
    flts = _filters()
    q = np.random.default_rng(5).standard_normal((len(flts), dim)).astype(np.float32)
    s, r = st.search(q, k, filter=flts)
    assert s.shape == (len(flts), k) and r.shape == (len(flts), k)
    assert s.dtype == np.float32 and r.dtype == np.int64
    for i, f in enumerate(flts):
        si, ri = st.search(q[i], k, filter=f)
        _same(s[i], r[i], si[0], ri[0], i)
    fin = np.isfinite(s)
    assert int(fin[3].sum()) == 4 and int(fin[7].sum()) == 0 and (r[7] == -1).all()
    assert {st.lookup(int(g))[0] for g in r[3][fin[3]]} == {"p3", "p5", "p8", "p13"}
    assert all(st.lookup(int(g))[1].original_document_id != "doc-b" for g in r[2][fin[2]])
    # a tuple is taken like a list; all-None is the plain search; the same list again (the
    # cached groups) gives the same answer
    s2, r2 = st.search(q, k, filter=tuple(flts))
    assert np.array_equal(s, s2) and np.array_equal(r, r2)
    s0, r0 = st.search(q, k, filter=[None] * len(flts))
    p0, q0 = st.search(q, k)
    assert np.array_equal(s0, p0) and np.array_equal(r0, q0)
    # the None entries are one plain search of those queries
    pn, qn = st.search(q[[1, 6]], k)
    assert np.array_equal(s[[1, 6]], pn) and np.array_equal(r[[1, 6]], qn)
    # after a delete the masks are made again: no deleted point comes back
    st.delete(point_ids=["p0", "p4", "p8"])
    s, r = st.search(q, k, filter=flts)
    got = {st.lookup(int(g))[0] for g in r[np.isfinite(s)]}
    assert not got & {"p0", "p4", "p8"}
    for i, f in enumerate(flts):
        si, ri = st.search(q[i], k, filter=f)
        _same(s[i], r[i], si[0], ri[0], i)


def test_store_filter_list_errors_and_single_forms_unchanged():
    st = _store()
    q = np.random.default_rng(6).standard_normal((3, SD)).astype(np.float32)
    f = Filter(must={"original_document_id": "doc-a"})
    with pytest.raises(ValueError, match="filters for 3 queries"):
        st.search(q, 5, filter=[f, None])
    with pytest.raises(ValueError):
        st.search(q, 5, filter=[])
    with pytest.raises(TypeError):
        st.search(q, 5, filter=[f, "doc-a", None])
    with pytest.raises(TypeError):
        st.search(q, 5, filter=[f, {"must": {}}, None])
    with pytest.raises(TypeError):
        st.search(q, 5, filter="doc-a")
    # more distinct filters than the mask LRU holds
    many = [Filter(point_ids=[f"p{i}", f"p{i + 40}"]) for i in range(VectorStore.FILTER_CACHE_MAX + 4)]
    qm = np.random.default_rng(7).standard_normal((len(many), SD)).astype(np.float32)
    s, r = st.search(qm, 3, filter=many)
    for i in range(len(many)):
        assert {st.lookup(int(g))[0] for g in r[i][np.isfinite(s[i])]} == {f"p{i}", f"p{i + 40}"}


def test_store_filter_list_with_group_attached_raises():
    class Group:
        def __init__(self):
            self.shard = HbmIndexShard(SD, 64, device="cpu")
            self.count = 0

    st = VectorStore(SD, 64, device="cpu", group=Group())
    with pytest.raises(ValueError, match="single-shard"):
        st.search(np.zeros((2, SD), np.float32), 3, filter=[None, Filter(point_ids=["x"])])


# ---- SearchBatcher ---------------------------------------------------------------------------------
def test_batcher_carries_filters_and_keeps_the_two_argument_call():
    from codename_symbiont_amd.services.batcher import SearchBatcher

    st = _store()
    calls = []

    def two_args(qs, k):                                # a search_fn that knows no filters
        calls.append(("plain", len(qs)))
        return st.search(qs, k)

    def three_args(qs, k, filters=None):
        calls.append(("filters", None if filters is None else list(filters)))
        return st.search(qs, k, filters)

    flts = _filters()
    q = np.random.default_rng(8).standard_normal((len(flts), SD)).astype(np.float32)

    async def run(fn, fs, ks):
        b = SearchBatcher(fn, window_ms=200.0, max_q=len(fs))
        try:
            if fs[0] == "positional":
                return await asyncio.gather(*[b.search(q[i], ks[i]) for i in range(len(fs))])
            return await asyncio.gather(*[b.search(q[i], ks[i], filter=fs[i])
                                          for i in range(len(fs))])
        finally:
            b._task.cancel()

    ks = [3 + i % 4 for i in range(len(flts))]
    # no request has a filter: search_fn(qs, k), with a two-argument function
    out = asyncio.run(run(two_args, ["positional"] * len(flts), ks))
    assert calls == [("plain", len(flts))]
    for i, (s, r) in enumerate(out):
        si, ri = st.search(q[i], max(ks))
        _same(s, r, si[0, :ks[i]], ri[0, :ks[i]], i)
    calls.clear()
    out = asyncio.run(run(two_args, [None] * len(flts), ks))
    assert calls == [("plain", len(flts))]
    # some do: search_fn(qs, k, filters), one entry per request in request order
    calls.clear()
    out = asyncio.run(run(three_args, flts, ks))
    assert len(calls) == 1 and calls[0][0] == "filters"
    assert [None if f is None else f.key() for f in calls[0][1]] == \
        [None if f is None else f.key() for f in flts]
    for i, (s, r) in enumerate(out):
        si, ri = st.search(q[i], max(ks), filter=flts[i])
        assert s.shape == (ks[i],)
        _same(s, r, si[0, :ks[i]], ri[0, :ks[i]], i)
